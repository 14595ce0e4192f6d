"""The references of tests/attn_util.py held against code that already exists, in float64 to 1e-12 of
each tensor's largest value: mha_attn_reference against oracle.restatement.multihead_attention with the
projections supplied here (the output, and the gradient back to x through both projections),
mha_user_pool_reference against oracle.restatement.mha_user; the pattern of attn_mask, and the outputs the
references make identically zero."""
import pytest
import torch
import torch.nn.functional as F

from attn_util import attn_inputs, attn_mask, mha_attn_reference, mha_user_pool_reference
from oracle import restatement as R

F64 = torch.float64
DTYPES = (torch.bool, torch.uint8, torch.int64, torch.float32, torch.float64)


def _close(got, want, name):
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    assert err <= 1e-12 * max(scale, 1e-300), "%s: err %.3e of max %.3e" % (name, err, scale)


def test_attn_mask_pattern():
    for dt in DTYPES:
        m = attn_mask(32, dt)
        assert m.dtype == dt and m.shape == (9, 32)
        assert (m != 0).sum(1).tolist() == [0, 1, 32, 31, 16, 30, 2, 1, 11]
        assert (m[8] != 0).nonzero().flatten().tolist() == list(range(0, 32, 3))
        m = attn_mask(49, dt)
        assert m.shape == (11, 49)
        assert (m != 0).sum(1).tolist() == [0, 1, 49, 48, 24, 47, 2, 1, 17, 33, 17]
        assert not (m[9, 16:32] != 0).any() and (m[9, :16] != 0).all() and (m[9, 32:] != 0).all()
        assert not (m[10, :32] != 0).any() and (m[10, 32:] != 0).all()
        # the same pattern in every dtype
        assert torch.equal(m != 0, attn_mask(49, torch.int64) != 0)
    assert attn_mask(33, torch.int64).shape == (11, 33) and (attn_mask(33) != 0)[10].sum() == 1
    assert (attn_mask(1) != 0).sum(1).tolist() == [0, 1, 1, 1, 1, 1, 1, 1, 1]


@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
@pytest.mark.parametrize("L", [1, 17, 64])
def test_attn_mask_float_values(L, dt):
    """Kept slots hold values other than 1, some cleared slots hold -0.0 -- which counts as masked."""
    m = attn_mask(L, dt)
    neg0 = (m == 0) & torch.signbit(m)
    assert neg0.any() and neg0[0, 0]
    assert torch.equal(m != 0, attn_mask(L, torch.int64) != 0)       # the row sums count -0.0 as masked
    kept = m[m != 0]
    assert set(kept.tolist()) <= {2.0, -1.0, 0.5} and (L == 1 or len(set(kept.tolist())) == 3)
    assert attn_mask(L, torch.uint8).max() == 255
    i64 = attn_mask(L, torch.int64)
    assert L == 1 or ((i64 != 0) & (i64 & 0xFFFFFFFF == 0)).any()   # nonzero only above bit 32


@pytest.mark.parametrize("L,heads,dk,dv,mdt", [(17, 3, 16, 16, torch.float64), (49, 2, 32, 32, torch.float32),
                                               (33, 3, 64, 32, torch.int64)])
def test_mha_attn_reference_vs_multihead_attention(L, heads, dk, dv, mdt):
    E = 24
    NQ, NV = heads * dk, heads * dv
    mask = attn_mask(L, mdt)
    n = mask.shape[0]
    g = torch.Generator().manual_seed(L)
    x = torch.randn(n, L, E, generator=g, dtype=F64).requires_grad_()
    wk, wv = torch.randn(NQ, E, generator=g, dtype=F64) * 0.2, torch.randn(NV, E, generator=g, dtype=F64) * 0.2
    bk = (torch.randn(NQ, generator=g, dtype=F64) * 0.1).requires_grad_()
    bv = (torch.randn(NV, generator=g, dtype=F64) * 0.1).requires_grad_()
    dout = torch.randn(n * L, NV, generator=g, dtype=F64)
    m = (mask != 0).to(F64)
    want = R.multihead_attention(x, wk, bk, wv, bv, heads, R.pairwise_mask(m))
    (want.reshape(n * L, NV) * dout).sum().backward()

    xs = x.detach().reshape(n * L, E)
    ref = mha_attn_reference(F.linear(xs, wk, bk.detach()), F.linear(xs, wv, bv.detach()), mask, heads, dk, dv, dout=dout)
    _close(ref["out"], want.detach().reshape(n * L, NV), "out")
    _close(ref["dqk"] @ wk + ref["dv"] @ wv, x.grad.reshape(n * L, E), "dx")
    _close(ref["dbias_k"], bk.grad, "dbias_k")
    _close(ref["dbias_v"], bv.grad, "dbias_v")
    _close(ref["dbias_k"], ref["dqk"].sum(0), "dbias_k = column sums")
    _close(ref["dbias_v"], ref["dv"].sum(0), "dbias_v = column sums")


@pytest.mark.parametrize("L,heads,dk,dv,mdt", [(17, 12, 32, 32, torch.float64), (49, 12, 64, 32, torch.uint8)])
def test_mha_user_pool_reference_vs_mha_user(L, heads, dk, dv, mdt):
    E = 20
    NQ, H = heads * dk, heads * dv
    mask = attn_mask(L, mdt)
    n = mask.shape[0]
    g = torch.Generator().manual_seed(L + 1)
    his = torch.randn(n, L, E, generator=g, dtype=F64)
    w = torch.randn(NQ + H, E, generator=g, dtype=F64) * 0.2
    b = torch.randn(NQ + H, generator=g, dtype=F64) * 0.1
    q = torch.randn(H, generator=g, dtype=F64)
    P = {"encoderU.mha.keyProject.weight": w[:NQ], "encoderU.mha.keyProject.bias": b[:NQ],
         "encoderU.mha.valueProject.weight": w[NQ:], "encoderU.mha.valueProject.bias": b[NQ:],
         "encoderU.query_news": q.reshape(1, H)}
    want = R.mha_user(his, (mask != 0).to(F64).reshape(n, L, 1), P, heads=heads).reshape(n, H)
    # the projections of R < n*L distinct news read through a row table, four padding columns
    y = torch.cat([F.linear(his.reshape(n * L, E), w, b), torch.full((n * L, 4), float("nan"), dtype=F64)], 1)
    perm = torch.randperm(n * L, generator=g)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(n * L)
    _close(mha_user_pool_reference(y[perm], inv, mask, heads, dk, dv, q), want, "user vector through yrows")
    _close(mha_user_pool_reference(y, None, mask, heads, dk, dv, q), want, "user vector")
    assert (mha_user_pool_reference(y, None, mask, heads, dk, dv, q)[0] == 0).all()     # the empty history


@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
@pytest.mark.parametrize("L", [6, 40])
def test_masked_tokens_and_empty_sequence_are_exactly_zero(L, dt):
    heads, dk, dv = 3, 16, 16
    mask = attn_mask(L, torch.float32)
    n = mask.shape[0]
    inp = attn_inputs(n, L, heads, dk, dv, 3)
    ref = mha_attn_reference(inp["qk"], inp["v"], mask, heads, dk, dv, dout=inp["dout"], dtype=dt)
    dead = (mask == 0).reshape(-1)
    assert dead[:L].all() and (~dead).any()
    for k in ("out", "dqk", "dv"):
        assert torch.isfinite(ref[k]).all()
        assert (ref[k][dead] == 0).all(), "%s rows of masked tokens are not exactly zero" % k
        assert (ref[k][~dead].abs().amax(1) > 0).all() or k == "dqk"
    assert ref["dqk"].abs().max() > 0


def test_single_slot_gives_zero_dqk():
    """L = 1: a softmax of one element has no gradient, dqk is exactly 0 in float64 and float32."""
    mask = attn_mask(1, torch.float64)
    n = mask.shape[0]
    inp = attn_inputs(n, 1, 12, 64, 32, 4)
    for dt in (torch.float64, torch.float32):
        ref = mha_attn_reference(inp["qk"], inp["v"], mask, 12, 64, 32, dout=inp["dout"], dtype=dt)
        assert (ref["dqk"] == 0).all() and (ref["dbias_k"] == 0).all()
        assert torch.equal(ref["out"][1:], inp["v"][1:].to(dt)) and (ref["out"][0] == 0).all()
        assert torch.equal(ref["dv"][1:], inp["dout"][1:].to(dt)) and (ref["dv"][0] == 0).all()


def test_rows_with_repeats_equal_a_gather_done_first():
    L, heads, dk, dv, R_ = 9, 2, 16, 16, 20
    mask = attn_mask(L)
    n = mask.shape[0]
    inp = attn_inputs(n, L, heads, dk, dv, 5, rows=R_)
    rows = torch.randint(0, R_, (n * L,), generator=torch.Generator().manual_seed(1))
    assert rows.unique().numel() < n * L
    a = mha_attn_reference(inp["qk"], inp["v"], mask, heads, dk, dv, dout=inp["dout"], rows=rows)
    b = mha_attn_reference(inp["qk"][rows], inp["v"][rows], mask, heads, dk, dv, dout=inp["dout"])
    for k in ("out", "dqk", "dv", "dbias_k", "dbias_v"):
        assert torch.equal(a[k], b[k]), k
    assert a["dqk"].shape == (n * L, heads * dk)       # the gradients stay per token


def test_scores_max_is_over_kept_pairs():
    mask = attn_mask(5)
    n = mask.shape[0]
    inp = attn_inputs(n, 5, 1, 16, 16, 6)
    qk = inp["qk"].clone()
    qk[:5] *= 100                                      # the empty sequence: none of its scores is kept
    ref = mha_attn_reference(qk, inp["v"], mask, 1, 16, 16)
    rest = mha_attn_reference(inp["qk"], inp["v"], mask, 1, 16, 16)
    assert ref["scores_max"] == rest["scores_max"] and ref["scores_max"] > 0
