"""The one-layer BERT news encoder (-encn transformer) on the GPU, level by level:

  kernel   K.sha_attn_fwd / K.sha_attn_bwd (csrc/sha_attn.hip) called directly into NaN-filled buffers with
           padded leading dimensions and gaps between the q, k and v column blocks, against the float64
           reference of tests/sha_attn_util.py with the dropout mask replayed;
  module   encoders.Transformer_Encoder (autograd wrapper TransformerNewsFn) against the reference model's
           golden tests/golden/transformer_news.npz in eval, and against the float64 composition with the
           three replayed dropout masks in training;
  model    build_model("transformer", "attn", 152) logits, scores and gradients against a float64 CPU
           composition of that encoder with oracle.restatement's pooling, scorer and NLL;
  graph    one captured train step replayed against eager, and the device RNG pair's advance per replay.

nr_sha_attn_* launch one kernel each for every shape; their structural boundaries (the 16-row thread
tiles, the 64-column chunks, the backward's LDS request crossing 64 KB) each have a case on either side
(sha_attn_util.KERNEL_CASES).

The bar of the kernel-level cases is test_birnn_gpu.py's: with e32 = max|ref32 - ref64| per tensor (the
same reference evaluated in float32 on the CPU), the kernel must stay within
32 e32 + 32 * 2^-24 * max|ref64|, and that bar may itself never exceed 1e-4 * max|ref64|
(tests/test_sha_attn_ref_cpu.py shows on the CPU that it never does).  Every case prints its err / e32
ratios ("sha-ratio" lines, pytest -s).  Measured on an MI355X, the largest ratio of any case and
tensor: 2.91 (probs at L 30, D 384)."""
import copy
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from sha_attn_util import (KERNEL_CASES, KERNEL_OFFSET, KERNEL_SEED, TENSORS, bar_of, case_references,
                           encoder_keeps, encoder_reference, sha_inputs, sha_keep, sha_mask)

NAN = float("nan")
GAP_K, GAP_V, PAD_Q, PAD_C, PAD_D = 4, 12, 8, 4, 12     # column gaps before k and v; leading-dimension pads
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transformer_news.npz")


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _layout(D):
    koff = D + GAP_K
    voff = koff + D + GAP_V
    return koff, voff, voff + D


def run_kernels(nseq, L, D, p, inp, mask, mask_dtype=torch.int64):
    """One nr_sha_attn_fwd and one nr_sha_attn_bwd (on the forward's own probs, as TransformerNewsFn runs
    them) into NaN-filled buffers -> {name: the whole buffer on the CPU, padding included}.  The gap and
    padding columns of qkv hold NaN: a kernel that read them would spread it."""
    from newsrec_amd import kernels as K
    T = nseq * L
    koff, voff, W = _layout(D)
    qkv = _nan(T, W + PAD_Q)
    for n, c in (("q", 0), ("k", koff), ("v", voff)):
        qkv[:, c:c + D] = inp[n].cuda()
    m = mask.to(mask_dtype).cuda().reshape(-1)
    ctx = _nan(T, D + PAD_C)
    probs = _nan(nseq * L * L + 64)                       # 64 guard floats behind the documented size
    kw = dict(koff=koff, voff=voff, p_drop=p, seed=KERNEL_SEED, offset=KERNEL_OFFSET)
    K.sha_attn_fwd(qkv[:, :W], m, nseq, L, D, ctx[:, :D], probs, **kw)
    dctx = _nan(T, D + PAD_D)
    dctx[:, :D] = inp["dctx"].cuda()
    dqkv = _nan(T, W + PAD_Q)
    K.sha_attn_bwd(qkv[:, :W], m, nseq, L, D, probs, dctx[:, :D], dqkv[:, :W], **kw)
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in dict(ctx=ctx, probs_buf=probs, dqkv=dqkv).items()}


def _unpack(out, nseq, L, D):
    koff, voff, W = _layout(D)
    return dict(ctx=out["ctx"][:, :D], probs=out["probs_buf"][:nseq * L * L].view(nseq, L, L),
                dq=out["dqkv"][:, :D], dk=out["dqkv"][:, koff:koff + D], dv=out["dqkv"][:, voff:W])


@pytest.mark.parametrize("nseq,L,D,p", KERNEL_CASES, ids=["n%d-L%d-D%d-p%g" % c for c in KERNEL_CASES])
def test_kernels_vs_reference(nseq, L, D, p):
    inp, mask, keep, ref = case_references(nseq, L, D, p)
    out = run_kernels(nseq, L, D, p, inp, mask)
    koff, voff, W = _layout(D)

    # ---- exact properties: the layout
    assert torch.isnan(out["ctx"][:, D:]).all(), "ctx: written past column %d" % D
    assert torch.isnan(out["probs_buf"][nseq * L * L:]).all(), "probs: written past nseq*L*L"
    dqkv = out["dqkv"]
    for a, b in ((D, koff), (koff + D, voff), (W, dqkv.shape[1])):
        assert torch.isnan(dqkv[:, a:b]).all(), "dqkv: written in columns [%d, %d)" % (a, b)
    got = _unpack(out, nseq, L, D)
    for name, t in got.items():
        assert torch.isfinite(t).all(), "%s: unwritten or non-finite values" % name
    # ---- exact properties: the mask
    masked = (mask == 0)[:, None, :].expand(nseq, L, L)
    assert (got["probs"][masked] == 0).all(), "probs is not exactly 0 at a masked key"
    empty = (mask != 0).sum(1) == 0
    assert empty.any() or nseq < 3
    rows = empty.repeat_interleave(L)
    assert (got["probs"][empty] == 0).all()
    for name in ("ctx", "dq", "dk", "dv"):
        assert (got[name][rows] == 0).all(), "%s of a title without a token is not exactly zero" % name
    sums = got["probs"].sum(-1)
    live = (~empty)[:, None].expand(nseq, L)
    assert (sums[live] - 1).abs().max() < 1e-5

    # ---- the reference and the bar
    late = []
    for name in TENSORS:
        want = ref[torch.float64][name]
        bar, e32, scale = bar_of(ref, name)
        if scale == 0:
            assert (got[name] == 0).all(), name
            continue
        err = (got[name].double() - want.reshape(got[name].shape)).abs().max().item()
        print("sha-ratio n%d-L%d-D%d-p%g %-5s err %.3e e32 %.3e err/e32 %s bar %.3e max %.3e"
              % (nseq, L, D, p, name, err, e32, "%.2f" % (err / e32) if e32 > 0 else "-", bar, scale))
        assert bar <= 1e-4 * scale, "%s: the bar %.3e exceeds 1e-4 of max %.3e" % (name, bar, scale)
        if not err <= bar:
            late.append("%s: err %.3e > bar %.3e (e32 %.3e, max %.3e)" % (name, err, bar, e32, scale))
    assert not late, "; ".join(late)

    again = run_kernels(nseq, L, D, p, inp, mask)      # no atomics: a second call gives the same bits
    for name in out:
        assert _bits_equal(out[name], again[name]), "%s differs between two calls" % name


@pytest.mark.parametrize("mask_dtype", [torch.uint8, torch.float64, torch.float32])
def test_mask_dtypes_give_the_same_bits(mask_dtype):
    nseq, L, D, p = 4, 5, 64, 0.1
    inp, mask, _, _ = case_references(nseq, L, D, p)
    a = run_kernels(nseq, L, D, p, inp, mask)
    b = run_kernels(nseq, L, D, p, inp, mask, mask_dtype)
    for name in a:
        assert _bits_equal(a[name], b[name]), name


def test_dropout_drops_exactly_the_replayed_entries():
    """With v = the first L unit vectors, ctx[s*L + i][j] is the dropped probability itself: exactly 0 where
    the replayed keep mask is False, probs / (1 - p) rounded once where it is True."""
    nseq, L, D, p = 4, 30, 64, 0.1
    inp = sha_inputs(nseq, L, D, 77)
    inp["v"] = torch.eye(L, D).repeat(nseq, 1)
    mask = sha_mask(nseq, L)
    got = _unpack(run_kernels(nseq, L, D, p, inp, mask), nseq, L, D)
    keep = sha_keep(KERNEL_SEED, KERNEL_OFFSET, nseq, L, p)
    assert 0.05 < (~keep).float().mean() < 0.15
    pd = got["ctx"].view(nseq, L, D)[:, :, :L]
    assert (got["ctx"].view(nseq, L, D)[:, :, L:] == 0).all()
    probs = got["probs"]
    assert (pd[~keep] == 0).all(), "a dropped entry reached ctx"
    live = keep & (probs != 0)
    assert (pd[live] != 0).all(), "a kept entry is missing from ctx"
    one = torch.tensor(1.0, dtype=torch.float32)
    assert torch.equal(pd[keep], probs[keep] * (one / (one - torch.tensor(p, dtype=torch.float32))))
    # a device (seed, offset) pair with the call's offset added gives the same mask
    from newsrec_amd import kernels as K
    T = nseq * L
    qkv = torch.cat([inp["q"], inp["k"], inp["v"]], 1).cuda()
    ctx, pr = _nan(T, D), _nan(nseq * L * L)
    rng = torch.tensor([KERNEL_SEED, KERNEL_OFFSET - 5], dtype=torch.int64, device="cuda")
    K.sha_attn_fwd(qkv, mask.cuda().reshape(-1), nseq, L, D, ctx, pr, p_drop=p, seed=1, offset=5, rng=rng)
    assert _bits_equal(ctx.cpu(), got["ctx"].contiguous())


# ---------------------------------------------------------------------- the module

@pytest.fixture(params=["bf16x6", "f32"])
def gemm_prec(request):
    """Both GEMM arithmetics, as in tests/test_birnn_gpu.py."""
    from newsrec_amd import _lib as Lb, kernels as Kn
    old = Kn.set_gemm_precision(Lb.GEMM_BF16X6 if request.param == "bf16x6" else Lb.GEMM_F32)
    yield request.param
    Kn.set_gemm_precision(old)


def _golden():
    z = np.load(GOLDEN)
    return {k: torch.from_numpy(z[k]) for k in z.files}


def _param_names(z):
    return [k for k in z if k.startswith(("project.", "bert.", "query_words"))]


def _golden_encoder(z):
    from newsrec_amd import encoders as E
    from model_util import Cfg
    H, E_ = z["project.weight"].shape
    mod = E.Transformer_Encoder(Cfg("transformer", "attn", H, bert_dim=E_)).cuda()
    mod.load_state_dict({k: z[k].float() for k in _param_names(z)}, strict=True)   # the reference's full state_dict
    return mod


def grad_bar(name, refs):
    """The gradient bar 1e-3 * max|ref| of one parameter.  The key bias is the one parameter whose exact
    gradient is ZERO: it shifts every score of a query row by the same q_i . b_k, the softmax ignores the
    shift, so db_k = colsum(dK) cancels term by term and the float64 reference holds only its own
    cancellation noise (checked here: under 1e-12 of the key weight's gradient).  A float32 sum cannot
    cancel below the rounding of its summands, so this one bar is taken at their scale, 1e-3 of max|ref|
    of the key WEIGHT's gradient (dW_k = dK^T x0 sums the same dK rows against O(1) inputs)."""
    ref = refs[name]
    if name.endswith("attention.self.key.bias"):
        w = refs[name[:-len("bias")] + "weight"].abs().max().item()
        assert ref.abs().max().item() < 1e-12 * w, "the key bias gradient of the reference is not noise"
        return 1e-3 * w
    scale = ref.abs().max().item()
    assert scale > 0, name
    return 1e-3 * scale


def _check_grads(mod, x, z_grads):
    grads = {"x": x.grad}
    grads.update({n: p.grad for n, p in mod.named_parameters()})
    assert len(grads) == 20
    for n, got in grads.items():
        assert got is not None, n
        torch.testing.assert_close(got.cpu().double(), z_grads[n], rtol=0, atol=grad_bar(n, z_grads),
                                   msg=lambda s, n=n: n + ": " + s)


def test_state_dict_is_the_references():
    z = _golden()
    mod = _golden_encoder(z)
    assert sorted(mod.state_dict().keys()) == sorted(_param_names(z)) and len(_param_names(z)) == 19
    for k, v in mod.state_dict().items():
        assert tuple(v.shape) == tuple(z[k].shape), k


def test_module_vs_golden(gemm_prec):
    z = _golden()
    mod = _golden_encoder(z).eval()
    x = z["x"].float().cuda().requires_grad_()
    tok, news = mod(x, attn_mask=z["mask"].cuda())
    assert tok.shape == z["tok"].shape and news.shape == z["news"].shape
    ((tok * z["a"].float().cuda()).sum() + (news * z["b"].float().cuda()).sum()).backward()
    torch.cuda.synchronize()
    torch.testing.assert_close(tok.detach().cpu().double(), z["tok"], rtol=0, atol=1e-4)
    torch.testing.assert_close(news.detach().cpu().double(), z["news"], rtol=0, atol=1e-4)
    assert (news[1, 1] == 0).all(), "the title without a token must pool to exact zeros"
    _check_grads(mod, x, {k[5:]: v for k, v in z.items() if k.startswith("grad.")})


def test_module_news_only_gradient(gemm_prec):
    """An unused token output costs no dtok: the backward runs from dnews alone."""
    z = _golden()
    mod = _golden_encoder(z).eval()
    x = z["x"].float().cuda().requires_grad_()
    _, news = mod(x, attn_mask=z["mask"].cuda())
    (news * z["b"].float().cuda()).sum().backward()
    P = {k: z[k].clone().requires_grad_() for k in _param_names(z)}
    x64 = z["x"].clone().requires_grad_()
    (encoder_reference(P, x64, z["mask"])[1] * z["b"]).sum().backward()
    _check_grads(mod, x, dict({n: p.grad for n, p in P.items()}, x=x64.grad))


def test_module_mask_none_is_all_ones():
    z = _golden()
    mod = _golden_encoder(z).eval()
    x = z["x"].float().cuda()
    with torch.no_grad():
        a = mod(x)
        b = mod(x, attn_mask=torch.ones(z["mask"].shape, dtype=torch.int64, device="cuda"))
    assert _bits_equal(a[0], b[0]) and _bits_equal(a[1], b[1])


def test_module_training_with_replayed_dropout(gemm_prec):
    z = _golden()
    mod = _golden_encoder(z).train()
    ps = (0.1, 0.1, 0.1)
    assert (mod.bert.attention.self.dropout.p, mod.bert.attention.output.dropout.p, mod.bert.output.dropout.p) == ps
    n, L, H = z["mask"].numel() // z["mask"].shape[-1], z["mask"].shape[-1], mod.hidden_dim
    T = n * L
    seed, off = mod._rng.seed, mod._rng.offset
    x = z["x"].float().cuda().requires_grad_()
    tok, news = mod(x, attn_mask=z["mask"].cuda())
    assert mod._rng.offset - off == T * L + 2 * T * H, "the stream must advance by T*L + 2*T*H"
    ((tok * z["a"].float().cuda()).sum() + (news * z["b"].float().cuda()).sum()).backward()
    torch.cuda.synchronize()
    keeps = encoder_keeps(seed, off, n, L, H, ps)
    assert all(k is not None and not k.all() for k in keeps)
    P = {k: z[k].clone().requires_grad_() for k in _param_names(z)}
    x64 = z["x"].clone().requires_grad_()
    wt, wn = encoder_reference(P, x64, z["mask"], keeps, ps)
    ((wt * z["a"]).sum() + (wn * z["b"]).sum()).backward()
    torch.testing.assert_close(tok.detach().cpu().double(), wt.detach(), rtol=0, atol=1e-4)
    torch.testing.assert_close(news.detach().cpu().double(), wn.detach(), rtol=0, atol=1e-4)
    _check_grads(mod, x, dict({k: p.grad for k, p in P.items()}, x=x64.grad))
    # a site whose rate is 0 draws nothing, the others keep their counters
    mod.bert.attention.output.dropout.p = 0.0
    off2 = mod._rng.offset
    with torch.no_grad():
        tok2 = mod(x.detach(), attn_mask=z["mask"].cuda())[0]
    ps2 = (0.1, 0.0, 0.1)
    with torch.no_grad():
        want2 = encoder_reference({k: z[k] for k in _param_names(z)}, z["x"], z["mask"],
                                  encoder_keeps(seed, off2, n, L, H, ps2), ps2)[0]
    torch.testing.assert_close(tok2.cpu().double(), want2, rtol=0, atol=1e-4)


def test_encode_tokens_equals_forward():
    """The fused entry (gather inside the GEMM, scatter epilogue) against forward(table[ids]); ids include
    the pad id 0, repeats and an all-pad title; the table's row 0 receives exactly zero gradient."""
    z = _golden()
    mod = _golden_encoder(z).eval()
    E_ = z["x"].shape[-1]
    g = torch.Generator().manual_seed(3)
    table = torch.randn(11, E_, generator=g)
    table[0] = 0
    ids = torch.tensor([[[5, 3, 0, 0, 0], [1, 1, 7, 5, 0], [10, 2, 3, 4, 6]],
                        [[0, 0, 0, 0, 0], [9, 8, 9, 8, 9], [5, 3, 0, 0, 1]]]).cuda()
    mask = (ids != 0).long()
    wt = torch.randn(2, 3, 5, mod.hidden_dim, generator=g).cuda()
    wn = torch.randn(2, 3, mod.hidden_dim, generator=g).cuda()
    res = []
    for fused in (True, False):
        t = table.clone().cuda().requires_grad_()
        mod.zero_grad()
        if fused:
            tok, news = mod.encode_tokens(t, ids, mask, pad_row=0, want_tokens=True)
        else:
            tok, news = mod(torch.nn.functional.embedding(ids, t, padding_idx=0), mask)
        ((tok * wt).sum() + (news * wn).sum()).backward()
        res.append([tok.detach(), news.detach(), t.grad] + [p.grad.clone() for p in mod.parameters()])
    assert (res[0][2][0] == 0).all(), "table row 0 received a gradient"
    assert (res[0][1][1, 0] == 0).all(), "the all-pad title must pool to exact zeros"
    for a, b in zip(*res):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)
    tok, news = mod.encode_tokens(table.cuda(), ids, mask)      # without tokens: None, and the same news
    assert tok is None
    torch.testing.assert_close(news, res[0][1], rtol=1e-5, atol=1e-5)


def test_hidden_dim_limits():
    from newsrec_amd import encoders as E
    from model_util import Cfg
    for H in (150, 1028):
        with pytest.raises(ValueError, match="1024"):
            E.Transformer_Encoder(Cfg("transformer", "attn", H))


# ---------------------------------------------------------------------- the model

MB, MC, MN, ML, MV, MH = 2, 3, 4, 5, 64, 152


def _model_batch(seed):
    g = torch.Generator().manual_seed(seed)

    def titles(n):
        tok = torch.randint(1, MV, (n, ML), generator=g)
        lens = torch.randint(1, ML + 1, (n,), generator=g)
        mask = (torch.arange(ML)[None] < lens[:, None]).long()
        return tok * mask, mask
    ct, cm = titles(MB * MC)
    ht, hm = titles(MB * MN)
    his_mask = torch.ones(MB, MN, 1, dtype=torch.float64)
    his_mask[1, -1] = 0
    return {"cdd_encoded_index": ct.view(MB, MC, ML), "cdd_attn_mask": cm.view(MB, MC, ML),
            "his_encoded_index": ht.view(MB, MN, ML), "his_attn_mask": hm.view(MB, MN, ML),
            "his_mask": his_mask, "user_id": torch.tensor([1, 2]), "label": torch.tensor([0, 2])}


def _set_dropout(model, p):
    b = model.encoderN.bert
    for d in (b.attention.self.dropout, b.attention.output.dropout, b.output.dropout):
        d.p = p


def _transformer_model(seed=11, p=0.1):
    from newsrec_amd.manager import build_model
    torch.manual_seed(seed)
    model = build_model("transformer", "attn", MH, vocab=MV)
    with torch.no_grad():
        # O(1) pre-activations: project is a default nn.Linear (weights U(+-1/sqrt(E))), so x0 = table[ids] W^T
        # has std (table std) / sqrt(3): the table at 2.  With a small table (0.5, x0 at 0.3) the pooling
        # query's gradient is a 1e-3 residue of its terms (6e-5 against dnews of 6e-2) and plain float32
        # torch on the CPU already misses the float64 value by 1.1e-3 of its maximum; at 2 that float32
        # composition is within 2e-5 of the maximum for every parameter (key bias aside, see grad_bar).
        model.embedding.bert_word_embedding.weight.mul_(2.0)
        model.embedding.bert_word_embedding.weight[0] = 0
    _set_dropout(model, p)
    return model


def test_build_model_dispatch():
    from newsrec_amd import encoders as E
    from newsrec_amd.manager import build_model
    model = build_model("transformer", "attn", MH, vocab=MV)
    assert isinstance(model.encoderN, E.Transformer_Encoder)
    assert model.name == "twotower__transformer__attn"
    with pytest.raises(ValueError, match="cnn, mha, rnn or transformer"):
        build_model("nope", "attn", MH, vocab=MV)
    with pytest.raises(ValueError):
        build_model("transformer", "attn", 150, vocab=MV)


def _model_reference(model, x, training, keeps=None, ps=(0.0, 0.0, 0.0)):
    """Float64 CPU composition: sha_attn_util's encoder over table[tokens] of candidates + history (one
    pass, as TwoTower runs it), then oracle.restatement's attention pooling, scorer and NLL."""
    from oracle import restatement as R
    P = {n: p.detach().cpu().double().requires_grad_() for n, p in model.named_parameters()}
    tokens = torch.cat([x["cdd_encoded_index"].view(-1, ML), x["his_encoded_index"].view(-1, ML)], 0)
    masks = torch.cat([x["cdd_attn_mask"].view(-1, ML), x["his_attn_mask"].view(-1, ML)], 0)
    emb = R.word_embedding(P["embedding.bert_word_embedding.weight"], tokens)
    news = encoder_reference(P, emb, masks, keeps, ps, pre="encoderN.")[1]
    cdd, his = news[:MB * MC].view(MB, MC, MH), news[MB * MC:].view(MB, MN, MH)
    user = R.attn_pool_user(his, x["his_mask"], P)
    score = R.compute_score(cdd, user)
    if not training:
        return torch.sigmoid(score).detach(), None
    logits = torch.nn.functional.log_softmax(score, 1)
    R.nll_loss(logits, x["label"]).backward()
    return logits.detach(), {n: p.grad for n, p in P.items()}


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_model_train_step_vs_float64(gemm_prec, p):
    model = _transformer_model(p=p)
    model.train()
    x = _model_batch(4)
    n = MB * (MC + MN)
    seed, off = model.encoderN._rng.seed, model.encoderN._rng.offset
    logits, loss = model.forward_loss({k: v.cuda() for k, v in x.items()})
    loss.backward()
    torch.cuda.synchronize()
    ps = (p, p, p)
    keeps = encoder_keeps(seed, off, n, ML, MH, ps) if p > 0 else None
    assert model.encoderN._rng.offset - off == (n * ML * ML + 2 * n * ML * MH if p > 0 else 0)
    want, grads = _model_reference(model, x, True, keeps, ps)
    torch.testing.assert_close(logits.detach().cpu().double(), want, rtol=0, atol=1e-3 * want.abs().max().item())
    for name, prm in model.named_parameters():
        ref = grads[name]
        assert prm.grad is not None and ref is not None, name
        torch.testing.assert_close(prm.grad.cpu().double(), ref, rtol=0, atol=grad_bar(name, grads),
                                   msg=lambda s, name=name: name + ": " + s)
    assert (model.embedding.bert_word_embedding.weight.grad[0] == 0).all()


def test_model_eval_scores_vs_float64(gemm_prec):
    model = _transformer_model()
    model.eval()
    x = _model_batch(6)
    with torch.no_grad():
        scores = model({k: v.cuda() for k, v in x.items()})[0]
    want, _ = _model_reference(model, x, False)
    torch.testing.assert_close(scores.cpu().double(), want, rtol=0, atol=1e-3 * want.abs().max().item())


# ---------------------------------------------------------------------- graph capture

def _capture(p):
    from newsrec_amd.manager import get_optim, train_step
    m_eager = _transformer_model(5, p=p)
    m_eager.train()
    m_graph = copy.deepcopy(m_eager)
    o_eager, o_graph = get_optim(m_eager, capturable=False), get_optim(m_graph, capturable=True)
    batches = [{k: v.cuda() for k, v in _model_batch(s).items()} for s in (1, 2, 3)]
    static = {k: v.clone() for k, v in batches[0].items()}
    for b in batches[:2]:                        # eager warm-up of both (allocator, optimizer state)
        train_step(m_eager, o_eager, b, check_labels=False)
        for k, v in b.items():
            static[k].copy_(v)
        train_step(m_graph, o_graph, static, check_labels=False)
    torch.cuda.synchronize()
    for k, v in batches[2].items():
        static[k].copy_(v)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        train_step(m_graph, o_graph, static, check_labels=False).detach()
    # the graph addresses the static batch and the optimizer's state: both must outlive every replay
    return m_eager, o_eager, m_graph, graph, batches, (static, o_graph)


def test_graph_replay_matches_eager():
    from newsrec_amd.manager import train_step
    m_eager, o_eager, m_graph, graph, batches, alive = _capture(0.0)
    before = m_graph.encoderN.project.weight.detach().clone()
    graph.replay()
    train_step(m_eager, o_eager, batches[2], check_labels=False)
    torch.cuda.synchronize()
    assert not torch.equal(before, m_graph.encoderN.project.weight), "the replay did not train"
    for (n, a), (_, b) in zip(m_eager.named_parameters(), m_graph.named_parameters()):
        torch.testing.assert_close(b, a, rtol=1e-4, atol=2e-5, msg=n)


def test_graph_replay_advances_the_rng_pair():
    _, _, m_graph, graph, _, alive = _capture(0.1)
    n = MB * (MC + MN)
    step = n * ML * ML + 2 * n * ML * MH
    state = m_graph.encoderN._rng.state
    seen = [state.clone()]
    for _ in range(2):
        graph.replay()
        seen.append(state.clone())
    torch.cuda.synchronize()
    seen = [s.cpu() for s in seen]
    assert seen[0][0] == seen[1][0] == seen[2][0] == m_graph.encoderN._rng.seed
    assert seen[1][1] - seen[0][1] == step and seen[2][1] - seen[1][1] == step
    for prm in m_graph.parameters():
        assert torch.isfinite(prm).all()
