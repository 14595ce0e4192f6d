"""The references of tests/pool_util.py held against code that already exists, in float64 to 1e-12 of
each tensor's largest value: mha_pool_reference against oracle.restatement.mha_news (replayed
dropout, gradients back to the embeddings), attn_pool_reference against scaled_dp_attention and
layer_norm; and the outputs the references make identically zero."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import restatement as R
from pool_util import attn_pool_inputs, attn_pool_reference, mha_pool_inputs, mha_pool_reference, pool_mask

F64 = torch.float64


def _close(got, want, name):
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    assert err <= 1e-12 * max(scale, 1e-300), "%s: err %.3e of max %.3e" % (name, err, scale)


def test_pool_mask_pattern():
    m = pool_mask(32)
    assert m.shape == (8, 32) and m.sum(1).tolist() == [0, 1, 32, 31, 16, 30, 2, 1]
    assert m[5, 1] == 0 and m[5, 3] == 0 and m[5, 0] == 1 and m[7, 31] == 1 and m[7, :31].sum() == 0
    assert pool_mask(1).sum(1).tolist() == [0, 1, 1, 1, 1, 1, 1, 1]
    assert pool_mask(2).sum(1).tolist() == [0, 1, 2, 1, 1, 2, 2, 1]
    assert pool_mask(4)[5].tolist() == [1, 1, 1, 1]


@pytest.mark.parametrize("p_drop", [0.0, 0.2])
@pytest.mark.parametrize("dv", [32, 64], ids=["H384", "H768"])
def test_mha_pool_reference_vs_mha_news(dv, p_drop):
    heads, dk, L, E = 12, 64, 17, 24
    H, NK = heads * dv, heads * dk
    mask = pool_mask(L)
    n = mask.shape[0]
    inp = mha_pool_inputs(n, L, heads, dk, dv, 5 + dv)
    g = torch.Generator().manual_seed(91)
    emb = torch.randn(1, n, L, E, generator=g, dtype=F64).requires_grad_()
    w = torch.randn(NK + H, E, generator=g, dtype=F64) * 0.1
    b = torch.randn(NK + H, generator=g, dtype=F64) * 0.1
    P = {"encoderN.mha.keyProject.weight": w[:NK], "encoderN.mha.keyProject.bias": b[:NK],
         "encoderN.mha.valueProject.weight": w[NK:], "encoderN.mha.valueProject.bias": b[NK:],
         "encoderN.layerNorm.weight": inp["gamma"].double(), "encoderN.layerNorm.bias": inp["beta"].double(),
         "encoderN.query_words": inp["q"].double().reshape(1, H)}
    keep = R.dropout_keep(7, 11, n * L, H, p_drop)
    assert bool(keep.all()) == (p_drop == 0)
    tok, news = R.mha_news(emb, mask.reshape(1, n, L).double(), P, heads=heads, dropout_keep=keep, p_drop=p_drop)
    ((news[0] * inp["dnews"].double()).sum() + (tok.reshape(n * L, H) * inp["dz"].double()).sum()).backward()

    y = F.linear(emb.detach().reshape(n * L, E), w, b)
    ref = mha_pool_reference(y, mask, heads, dk, dv, inp["gamma"], inp["beta"], inp["q"], keep, p_drop,
                             dnews=inp["dnews"], dz=inp["dz"])
    _close(ref["news"], news[0].detach(), "news")
    _close(ref["Z"], tok.detach().reshape(n * L, H), "token output")
    _close(torch.matmul(ref["dy"], w), emb.grad.reshape(n * L, E), "d emb")
    _close(ref["dbias"], ref["dy"].sum(0), "dbias")
    # the saved statistics are those of the attention output
    _close(ref["stats"][:, 0], ref["O"].mean(1), "mean")
    _close(ref["stats"][:, 1], (ref["O"].var(1, unbiased=False) + 1e-5) ** -0.5, "rstd")


@pytest.mark.parametrize("form", ["tied", "key", "ln"])
def test_attn_pool_reference_vs_scaled_dp_attention(form):
    D, L = 150, 9
    mask = pool_mask(L)
    n = mask.shape[0]
    inp = attn_pool_inputs(n, L, D, 3)
    x = inp["x"].double().requires_grad_()
    key = inp["key"].double().requires_grad_()
    q = inp["q"].double().requires_grad_()
    gamma, beta = inp["gamma"].double().requires_grad_(), inp["beta"].double().requires_grad_()
    z = R.layer_norm(x, gamma, beta) if form == "ln" else x
    zs = z.reshape(n, L, D)
    ks = key.reshape(n, L, D) if form == "key" else zs
    want = R.scaled_dp_attention(q.reshape(1, D), ks, zs, mask.reshape(n, 1, L).double()).squeeze(-2)
    (want * inp["dout"].double()).sum().backward()
    ref = attn_pool_reference(inp["x"], inp["key"] if form == "key" else None, inp["q"], mask,
                              inp["gamma"] if form == "ln" else None, inp["beta"] if form == "ln" else None, None, 0.0,
                              1.0 / math.sqrt(D), False, dout=inp["dout"])
    _close(ref["out"], want.detach(), "out")
    _close(ref["Z"], z.detach(), "Z")
    _close(ref["dx"], x.grad, "dx")
    _close(ref["dq"], q.grad, "dq")
    if form == "key":
        _close(ref["dk"], key.grad, "dk")
        tanh = attn_pool_reference(inp["x"], inp["key"], inp["q"], mask, None, None, None, 0.0, 1.0 / math.sqrt(D), True,
                                   dout=inp["dout"])
        _close(tanh["dk"], key.grad * (1 - key.detach() ** 2), "dk through tanh")
    if form == "ln":
        _close(ref["dgamma"], gamma.grad, "dgamma")
        _close(ref["dbeta"], beta.grad, "dbeta")
        assert ref["stats"].shape == (n * L, 2)
    else:
        assert ref["stats"] is None and "dgamma" not in ref


def test_attn_pool_reference_dropout_and_dz():
    """Z = LN(x) * keep / (1 - p), and dz reaches dx, dgamma, dbeta as a second loss term."""
    D, L, p = 64, 5, 0.2
    mask = pool_mask(L)
    n = mask.shape[0]
    inp = attn_pool_inputs(n, L, D, 4)
    keep = R.dropout_keep(3, 8, n * L, D, p)
    assert 0.7 < keep.double().mean().item() < 0.9
    ref = attn_pool_reference(inp["x"], None, inp["q"], mask, inp["gamma"], inp["beta"], keep, p, 0.3, False,
                              dout=inp["dout"], dz=inp["dz"])
    ln = R.layer_norm(inp["x"].double(), inp["gamma"].double(), inp["beta"].double())
    _close(ref["Z"], ln * keep.double() / (1 - p), "Z")
    assert (ref["Z"][~keep] == 0).all()
    no_dz = attn_pool_reference(inp["x"], None, inp["q"], mask, inp["gamma"], inp["beta"], keep, p, 0.3, False,
                                dout=inp["dout"])
    _close(ref["dbeta"] - no_dz["dbeta"], (inp["dz"].double() * keep.double() / (1 - p)).sum(0), "dbeta of dz")


def test_single_slot_gives_zero_dq_and_dk():
    """L = 1: a softmax of one element has no gradient, so dq (and dk of a separate key) are exactly 0."""
    mask = pool_mask(1)
    n = mask.shape[0]
    inp = mha_pool_inputs(n, 1, 12, 64, 32, 1)
    keep = R.dropout_keep(1, 2, n, 384, 0.2)
    ref = mha_pool_reference(inp["y"], mask, 12, 64, 32, inp["gamma"], inp["beta"], inp["q"], keep, 0.2,
                             dnews=inp["dnews"], dz=inp["dz"])
    assert (ref["dq"] == 0).all() and ref["dy"].abs().max() > 0
    assert (ref["dy"][:, :12 * 64] == 0).all()        # one key: its score has no gradient either
    a = attn_pool_inputs(n, 1, 3, 2)
    for dt in (torch.float64, torch.float32):
        r = attn_pool_reference(a["x"], a["key"], a["q"], mask, None, None, None, 0.0, 0.5, True, dout=a["dout"],
                                dtype=dt)
        assert (r["dq"] == 0).all() and (r["dk"] == 0).all() and r["dx"].abs().max() > 0


@pytest.mark.parametrize("with_dz", [False, True])
def test_fully_masked_sequence_is_zero(with_dz):
    L = 6
    mask = pool_mask(L)
    n = mask.shape[0]
    assert mask[0].sum() == 0
    inp = mha_pool_inputs(n, L, 8, 64, 32, 9)
    H = 256
    dz = inp["dz"] if with_dz else None
    ref = mha_pool_reference(inp["y"], mask, 8, 64, 32, inp["gamma"], inp["beta"], inp["q"], None, 0.0,
                             dnews=inp["dnews"], dz=dz)
    for v in ref.values():
        assert torch.isfinite(v).all()
    assert (ref["news"][0] == 0).all() and (ref["probs"][0] == 0).all() and (ref["O"][:L] == 0).all()
    assert (ref["probs"][mask == 0] == 0).all()
    assert (ref["dy"][(mask == 0).reshape(-1)] == 0).all()      # masked tokens carry no gradient, dz or not
    # the same batch without sequence 0: its tokens reach dgamma / dbeta through dz alone
    rest = mha_pool_reference(inp["y"][L:], mask[1:], 8, 64, 32, inp["gamma"], inp["beta"], inp["q"], None, 0.0,
                              dnews=inp["dnews"][1:], dz=dz[L:] if with_dz else None)
    _close(ref["dq"], rest["dq"], "dq")
    if with_dz:
        # Z of a masked token is beta (O = 0, x_hat = 0): dbeta takes its dz, dgamma nothing
        _close(ref["dbeta"] - rest["dbeta"], dz[:L].double().sum(0), "dbeta of the masked sequence")
        _close(ref["dgamma"], rest["dgamma"], "dgamma")
    else:
        _close(ref["dbeta"], rest["dbeta"], "dbeta")
        _close(ref["dgamma"], rest["dgamma"], "dgamma")

    a = attn_pool_inputs(n, L, 10, 6)
    r = attn_pool_reference(a["x"], None, a["q"], mask, a["gamma"], a["beta"], None, 0.0, 0.4, False, dout=a["dout"],
                            dz=a["dz"] if with_dz else None)
    assert (r["out"][0] == 0).all() and (r["probs"][0] == 0).all()
    if with_dz:
        assert r["dx"][:L].abs().max() > 0       # dz still reaches dx through the LayerNorm
    else:
        assert (r["dx"][(mask == 0).reshape(-1)] == 0).all()
    k = attn_pool_reference(a["x"], a["key"], a["q"], mask, None, None, None, 0.0, 0.4, True, dout=a["dout"])
    assert (k["dk"][(mask == 0).reshape(-1)] == 0).all() and (k["dx"][:L] == 0).all()
