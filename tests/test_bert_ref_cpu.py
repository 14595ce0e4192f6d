"""The references of tests/bert_util.py held against independent formulations, in float64 to 1e-12 of
each tensor's largest value: embed_reference against oracle.restatement.bert_embeddings (replayed
dropout, gradients back to the three tables), add_ln_reference against torch's layer_norm,
attn_reference against a per-(sequence, head) loop over torch.softmax; torch.autograd.gradcheck of
the formula behind each (embed_forward, add_ln_forward, attn_forward) at a tiny shape; the uniform rows
of a fully masked sequence and the zero padding row of dword."""
import pytest
import torch
import torch.nn.functional as F

from bert_util import (NEG, add_ln_forward, add_ln_reference, attn_forward, attn_inputs, attn_mask, attn_reference,
                       bert_dropout, embed_forward, embed_inputs, embed_reference, ln_inputs)
from oracle import restatement as R

F64 = torch.float64


def _close(got, want, name):
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    assert err <= 1e-12 * max(scale, 1e-300), "%s: err %.3e of max %.3e" % (name, err, scale)


def test_attn_mask_pattern():
    m = attn_mask(33)
    assert m.shape == (4, 33) and m.sum(1).tolist() == [33, 22, 0, 30]
    assert m[3, 1] == 0 and m[3, 3] == 0 and m[3, 0] == 1 and m[3, 31] == 1 and m[3, 32] == 0
    assert attn_mask(1).sum(1).tolist() == [1, 1, 0, 1]
    assert attn_mask(4)[3].tolist() == [1, 1, 1, 0]


def test_embed_inputs_have_padding_and_duplicates():
    for nseq, L in ((1, 5), (3, 7)):
        ids = embed_inputs(nseq, L, 8, 11, L + 2, 1)["ids"].view(-1)
        assert ids[0] == 0 and ids[-1] == ids[1] and ids.min() >= 0 and ids.max() < 11
    assert embed_inputs(1, 1, 8, 11, 1, 1)["ids"].item() > 0


@pytest.mark.parametrize("p_drop", [0.0, 0.1])
def test_embed_reference_vs_bert_embeddings(p_drop):
    nseq, L, H, V = 3, 7, 12, 11
    T = nseq * L
    inp = embed_inputs(nseq, L, H, V, L + 2, 7)
    keep = bert_dropout(5, T, H, 1, p_drop).embed(0, T) if p_drop else None
    P = {"bert.embeddings.word_embeddings.weight": inp["word"].double().requires_grad_(),
         "bert.embeddings.position_embeddings.weight": inp["pos"].double().requires_grad_(),
         "bert.embeddings.token_type_embeddings.weight": inp["type"].double().requires_grad_(),
         "bert.embeddings.LayerNorm.weight": inp["gamma"].double().requires_grad_(),
         "bert.embeddings.LayerNorm.bias": inp["beta"].double().requires_grad_()}
    want = R.bert_embeddings(P, inp["ids"], eps=1e-12, keep=keep.reshape(nseq, L, H) if p_drop else None,
                             p_drop=p_drop).reshape(T, H)
    (want * inp["dout"].double()).sum().backward()
    ref = embed_reference(inp["word"], inp["pos"], inp["type"][0], inp["ids"], inp["gamma"], inp["beta"], 1e-12,
                          keep, p_drop, dout=inp["dout"])
    _close(ref["out"], want.detach(), "out")
    if p_drop:
        assert 0.8 < keep.double().mean().item() < 0.97 and (ref["out"][~keep] == 0).all()
    gw = P["bert.embeddings.word_embeddings.weight"].grad.clone()
    assert gw[0].abs().max() > 0                     # the padding id occurs: plain indexing gives it a gradient
    assert (ref["dword"][0] == 0).all()              # nn.Embedding(padding_idx=0) does not
    gw[0] = 0
    _close(ref["dword"], gw, "dword")
    _close(ref["dpos"], P["bert.embeddings.position_embeddings.weight"].grad, "dpos")
    assert (ref["dpos"][L:] == 0).all() and ref["dpos"].shape == (L + 2, H)
    _close(ref["dtype0"], P["bert.embeddings.token_type_embeddings.weight"].grad[0], "dtype0")
    _close(ref["dgamma"], P["bert.embeddings.LayerNorm.weight"].grad, "dgamma")
    _close(ref["dbeta"], P["bert.embeddings.LayerNorm.bias"].grad, "dbeta")
    # the chain the kernels run: dword = scatter-add of ds but for the padding id, dpos / dtype0 column sums
    ds = ref["ds"]
    dw = torch.zeros(V, H, dtype=F64).index_add_(0, inp["ids"].view(-1), ds)
    dw[0] = 0
    _close(ref["dword"], dw, "dword from ds")
    _close(ref["dpos"][:L], ds.reshape(nseq, L, H).sum(0), "dpos from ds")
    _close(ref["dtype0"], ds.sum(0), "dtype0 from ds")
    s_in = inp["word"].double()[inp["ids"].view(-1)] + inp["pos"].double()[:L].repeat(nseq, 1) + inp["type"].double()[0]
    _close(ref["stats"][:, 0], s_in.mean(1), "mean")
    _close(ref["stats"][:, 1], (s_in.var(1, unbiased=False) + 1e-12) ** -0.5, "rstd")


@pytest.mark.parametrize("p_drop", [0.0, 0.1])
def test_add_ln_reference_vs_layer_norm(p_drop):
    T, H = 6, 20
    inp = ln_inputs(T, H, 3)
    keep = bert_dropout(9, T, H, 1, p_drop).dense(0, 0, 0, T) if p_drop else None
    x, res, gamma, beta = (inp[k].double().requires_grad_() for k in ("x", "res", "gamma", "beta"))
    s = (x * keep.double() / (1 - p_drop) if p_drop else x) + res
    want = F.layer_norm(s, (H,), gamma, beta, 1e-12)
    (want * inp["dout"].double()).sum().backward()
    ref = add_ln_reference(inp["x"], inp["res"], inp["gamma"], inp["beta"], 1e-12, keep, p_drop, dout=inp["dout"])
    _close(ref["out"], want.detach(), "out")
    _close(ref["dx"], x.grad, "dx")
    _close(ref["dres"], res.grad, "dres")
    _close(ref["dgamma"], gamma.grad, "dgamma")
    _close(ref["dbeta"], beta.grad, "dbeta")
    _close(ref["stats"][:, 0], s.detach().mean(1), "mean")
    _close(ref["stats"][:, 1], (s.detach().var(1, unbiased=False) + 1e-12) ** -0.5, "rstd")
    if p_drop:
        assert (~keep).any() and (ref["dx"][~keep] == 0).all()
        _close(ref["dx"][keep], ref["dres"][keep] / (1 - p_drop), "dx = dres / (1 - p) where kept")
    else:
        _close(ref["dx"], ref["dres"], "dx = dres without dropout")


@pytest.mark.parametrize("p_drop", [0.0, 0.1])
def test_attn_reference_vs_softmax_loop(p_drop):
    L, heads = 6, 2
    mask = attn_mask(L)
    nseq, H = mask.shape[0], heads * 64
    inp = attn_inputs(nseq, L, heads, 2)
    keep = bert_dropout(4, nseq * L, H, heads, p_drop).attn(0, 0, nseq, L) if p_drop else None
    q, k, v = (inp[n].double().requires_grad_() for n in ("q", "k", "v"))
    rows = []
    for s in range(nseq):
        add = (1.0 - mask[s].double()) * NEG
        cols = []
        for h in range(heads):
            sl = (slice(s * L, (s + 1) * L), slice(h * 64, (h + 1) * 64))
            p = torch.softmax(q[sl] @ k[sl].T / 8.0 + add[None, :], -1)
            if p_drop:
                p = p * keep[s, h].double() / (1 - p_drop)
            cols.append(p @ v[sl])
        rows.append(torch.cat(cols, 1))
    want = torch.cat(rows, 0)
    (want * inp["dctx"].double()).sum().backward()
    ref = attn_reference(inp["q"], inp["k"], inp["v"], mask, heads, keep, p_drop, dctx=inp["dctx"])
    _close(ref["ctx"], want.detach(), "ctx")
    _close(ref["dq"], q.grad, "dq")
    _close(ref["dk"], k.grad, "dk")
    _close(ref["dv"], v.grad, "dv")
    # the saved statistics: max and 1 / sum of exp(s - max) over the keys of the mask (sequence 0: all)
    s0 = (inp["q"].double()[:L, :64] @ inp["k"].double()[:L, :64].T) / 8.0
    _close(ref["m"][:L, 0], s0.max(1).values, "row max")
    _close(ref["il"][:L, 0], 1.0 / torch.exp(s0 - s0.max(1, keepdim=True).values).sum(1), "1 / row sum")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_fully_masked_sequence_is_uniform(dtype):
    L, heads = 5, 1
    mask = attn_mask(L)
    assert mask[2].sum() == 0
    inp = attn_inputs(4, L, heads, 8)
    ref = attn_reference(inp["q"], inp["k"], inp["v"], mask, heads, None, 0.0, dctx=inp["dctx"], dtype=dtype)
    for t in ref.values():
        assert torch.isfinite(t).all()
    rows = slice(2 * L, 3 * L)
    mean_v = inp["v"].to(dtype)[rows].mean(0, keepdim=True).expand(L, -1)
    assert (ref["ctx"][rows] - mean_v).abs().max().item() <= 4 * torch.finfo(dtype).eps
    assert (ref["m"][rows] == NEG).all() and (ref["il"][rows] == 1.0 / L).all()
    # masked keys of the other sequences take no probability: their dv is exactly zero
    dead = (mask == 0).reshape(-1)
    dead[rows] = False
    assert dead.any() and (ref["dv"][dead] == 0).all() and (ref["dk"][dead] == 0).all()


def test_gradcheck_embed():
    nseq, L, H, V = 2, 3, 8, 5
    e = embed_inputs(nseq, L, H, V, L + 1, 3)
    keep = bert_dropout(1, nseq * L, H, 1, 0.3).embed(0, nseq * L)
    assert (~keep).any()
    args = [e[k].double().requires_grad_() for k in ("word", "pos")] + \
           [e["type"][0].double().requires_grad_(), e["gamma"].double().requires_grad_(), e["beta"].double().requires_grad_()]

    def f(word, pos, type0, gamma, beta):
        return embed_forward(word, pos, type0, e["ids"], gamma, beta, 1e-12, keep, 0.3)[:3]
    assert torch.autograd.gradcheck(f, args, eps=1e-6, atol=1e-6)


def test_gradcheck_add_ln():
    T, H = 3, 8
    a = ln_inputs(T, H, 1)
    keep = bert_dropout(2, T, H, 1, 0.3).dense(0, 0, 0, T)
    assert (~keep).any()
    args = [a[k].double().requires_grad_() for k in ("x", "res", "gamma", "beta")]
    assert torch.autograd.gradcheck(lambda *t: add_ln_forward(*t, 1e-12, keep, 0.3), args, eps=1e-6, atol=1e-6)


def test_gradcheck_attn():
    """Without the fully masked sequence: its scores sit at finfo.min, where a finite difference of q or
    k is absorbed while autograd (like the kernels) differentiates the formula."""
    L, heads = 5, 1
    mask = attn_mask(L)[[0, 1, 3]]
    a = attn_inputs(3, L, heads, 5)
    keep = bert_dropout(1, 3 * L, 64, heads, 0.3).attn(0, 0, 3, L)
    assert (~keep).any()
    args = [a[n].double().requires_grad_() for n in ("q", "k", "v")]
    # ctx and the row sum (the row maximum is piecewise linear: no finite difference across its kinks)
    assert torch.autograd.gradcheck(lambda q, k, v: attn_forward(q, k, v, mask, heads, keep, 0.3)[0], args,
                                    eps=1e-6, atol=1e-6)
