"""Kernel-level tests of csrc/score_adam.hip's scorer, XSoftmax, single-tensor Adam and row-copy
entries, each called directly through newsrec_amd.kernels and compared with the closed-form float64
references of tests/score_util.py (held against autograd and torch.optim.Adam on the CPU by
tests/test_score_ref_cpu.py):

  nr_score_fwd / nr_score_bwd          all three heads, forward and backward, the cdd_idx gather,
                                       C past the 64-lane and the 256-thread loops, large scores
  nr_score_nll_fwd / nr_score_nll_bwd  C > 64
  nr_xsoftmax_fwd / nr_xsoftmax_bwd    cols 1 .. 300, every mask dtype, poisoned masked slots
  nr_adam                              float4 body, n % 4 tail, grid-stride round, device step count
  nr_gather_rows_f32, nr_transpose_f32 padded destinations, the float4 / scalar choice

Inputs and outputs are views into larger NaN-filled buffers wherever the ABI takes a leading
dimension (or, for flat outputs, the head of a longer buffer): a read past a row shows as a NaN in
the result, a write past it as a guard word that is no longer NaN.  Every test prints the largest
error it measured as a fraction of its bar (run with -s)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from newsrec_amd import _lib as L
from newsrec_amd import kernels as K
from oracle import restatement as R
from score_util import (adam_reference, f32, nll_reference, score_reference, score_tolerance,
                        xsoftmax_bwd_reference)
from topk_util import scale32

NAN = float("nan")
MODES = [L.SCORE_RAW, L.SCORE_LOG_SOFTMAX, L.SCORE_SIGMOID]
MODE_IDS = ["raw", "log_softmax", "sigmoid"]
# the bars of test_model_gpu.test_score_nll_kernel_vs_torch, which holds these kernels' siblings
LOGIT_RTOL, LOGIT_ATOL = 1e-5, 1e-5
GRAD_RTOL, GRAD_ATOL = 1e-4, 1e-6

SCORE_CASES = [
    (1, 1, 1),       # all minima
    (3, 4, 64),      # one candidate per wave, one trip over H
    (7, 5, 150),     # C > 4 waves (wave 0 takes a second candidate), H tail (150 = 2 * 64 + 22)
    (2, 65, 3),      # second trip of the wave-0 log-sum-exp loops (C > 64), H < 64
    (2, 130, 65),    # third trip, H = 64 + 1
    (1, 257, 8),     # second trip of the `tid + 256` store loop of the raw / sigmoid heads
    (5, 20, 400),    # the large config
]


# ---------------------------------------------------------------- guarded storage

def _guarded(t, pad_cols, extra_rows=0):
    """t [r, c] (CPU) -> (NaN-filled CUDA buffer [r + extra_rows, c + pad_cols], its [:r, :c] view holding t)"""
    r, c = t.shape
    buf = torch.full((r + extra_rows, c + pad_cols), NAN, device="cuda")
    buf[:r, :c] = t.float().cuda()
    return buf, buf[:r, :c]


def _nan_view(r, c, pad_cols, extra_rows):
    buf = torch.full((r + extra_rows, c + pad_cols), NAN, device="cuda")
    return buf, buf[:r, :c]


def _nan_flat(n, shape=None):
    """(NaN-filled CUDA buffer of n + 64 floats, its contiguous head of n reshaped)"""
    buf = torch.full((n + 64,), NAN, device="cuda")
    head = buf[:n]
    return buf, head.view(shape) if shape is not None else head


def _guards_intact(buf, r, c):
    """Everything of the 2-D buffer outside [:r, :c] is still NaN, everything inside finite."""
    inside = torch.zeros_like(buf, dtype=torch.bool)
    inside[:r, :c] = True
    return bool(torch.isnan(buf[~inside]).all()) and bool(torch.isfinite(buf[inside]).all())


def _tail_intact(buf, n):
    return bool(torch.isnan(buf[n:]).all()) and buf.numel() == n + 64


def _ratio(got, want, rtol, atol):
    """max |got - want| / (atol + rtol |want|): <= 1 is torch.testing.assert_close's criterion (NaN fails)."""
    got = got.detach().double().cpu().reshape(want.shape)
    r = ((got - want).abs() / (atol + rtol * want.abs())).max().item()
    return r if r == r else float("inf")


def _score_inputs(B, C, H, seed, rows=None):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows or B * C, H, generator=g), torch.randn(B, H, generator=g),
            torch.randn(B, C, generator=g))


def _score_fwd(cdd, user, B, C, H, mode, idx=None):
    """nr_score_fwd on guarded storage -> (logits view [B*C] on the device, float64 CPU copy [B, C])"""
    _, cv = _guarded(cdd, 3)
    _, uv = _guarded(user, 5)
    lbuf, logits = _nan_flat(B * C)
    K.score_fwd(cv, uv, B, C, H, mode, logits, cdd_idx=idx.cuda() if idx is not None else None)
    torch.cuda.synchronize()
    assert _tail_intact(lbuf, B * C), "nr_score_fwd wrote past logits[B*C]"
    got = logits.double().cpu().view(B, C)
    assert torch.isfinite(got).all()
    return (cv, uv, logits), got


def _check_head(got, ref, tol, mode, what):
    """Raw scores: the derived fp32 dot-product bound, nothing else.  Heads: the logit bars."""
    if mode == L.SCORE_RAW:
        r = ((got - ref["s"]).abs() / tol.clamp_min(1e-300)).max().item()
        print("%s raw: max err / dot-product bound = %.3f" % (what, r))
    else:
        r = _ratio(got, ref["out"], LOGIT_RTOL, LOGIT_ATOL)
        print("%s %s: max err / (%.0e + %.0e |want|) = %.3f" % (what, MODE_IDS[mode], LOGIT_ATOL, LOGIT_RTOL, r))
    assert r <= 1.0, what


# ---------------------------------------------------------------- scorer

@pytest.mark.parametrize("B,C,H", SCORE_CASES)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_score_fwd_bwd(mode, B, C, H):
    """nr_score_fwd and nr_score_bwd on N(0,1) inputs against float64: cdd a [:, :H] view of
    [B*C, H+3], user of [B, H+5], logits the head of a longer buffer, dcdd / duser views into
    [B*C+2, H+3] / [B+2, H+5].  The backward reads the forward's own fp32 logits, as the autograd
    Function hands them over."""
    cdd, user, dl = _score_inputs(B, C, H, 1000 * mode + 31 * B + 7 * C + H)
    ref = score_reference(cdd, user, B, C, mode, dlogits=dl)
    what = "score B=%d C=%d H=%d" % (B, C, H)
    (cv, uv, logits), got = _score_fwd(cdd, user, B, C, H, mode)
    _check_head(got, ref, score_tolerance(cdd, user, B, C), mode, what)

    dcbuf, dcv = _nan_view(B * C, H, 3, 2)
    dubuf, duv = _nan_view(B, H, 5, 2)
    K.score_bwd(cv, uv, logits, dl.cuda().contiguous(), B, C, H, mode, dcv, duv)
    torch.cuda.synchronize()
    assert _guards_intact(dcbuf, B * C, H), "dcdd: a guard word was written or an element left unwritten"
    assert _guards_intact(dubuf, B, H), "duser: a guard word was written or an element left unwritten"
    rc = _ratio(dcv, ref["dcdd"], GRAD_RTOL, GRAD_ATOL)
    ru = _ratio(duv, ref["duser"], GRAD_RTOL, GRAD_ATOL)
    print("%s %s bwd: max err / (%.0e + %.0e |want|): dcdd %.3f duser %.3f"
          % (what, MODE_IDS[mode], GRAD_ATOL, GRAD_RTOL, rc, ru))
    assert rc <= 1.0 and ru <= 1.0, what


def _gather_ids(n):
    """n ids into a 40-row table: repeats, rows 0 and 39, and idx[i] != i almost everywhere."""
    idx = ((torch.arange(n) * 7 + 3) % 17) * 2 + 1
    idx[n // 2] = idx[1]
    idx[0], idx[-1] = 39, 0
    return idx


@pytest.mark.parametrize("B,C,H", [(3, 4, 64), (7, 5, 150), (2, 20, 3)])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_score_fwd_gather(mode, B, C, H):
    """nr_score_fwd with cdd_idx (predict_fast's news-table gather): a 40-row table of leading
    dimension H + 3.  The reference with the ids differs from the one without by far more than the
    bar, so a kernel that ignored the ids would fail."""
    table, user, _ = _score_inputs(B, C, H, 77 + B + C + H, rows=40)
    idx = _gather_ids(B * C)
    assert len(set(idx.tolist())) < B * C and idx.min() == 0 and idx.max() == 39
    assert (idx != torch.arange(B * C)).float().mean() > 0.8
    ref = score_reference(table, user, B, C, mode, idx=idx)
    tol = score_tolerance(table, user, B, C, idx=idx)
    _, got = _score_fwd(table, user, B, C, H, mode, idx=idx)
    _check_head(got, ref, tol, mode, "gather B=%d C=%d H=%d" % (B, C, H))
    plain = score_reference(table, user, B, C, mode)              # rows b*C+c of the table: B*C <= 40
    bar = tol if mode == L.SCORE_RAW else LOGIT_ATOL + LOGIT_RTOL * ref["out"].abs()
    assert ((plain["out"] - ref["out"]).abs() > 10 * bar).float().mean() > 0.5


def _rows_scoring(cdd, user, target):
    """cdd with each row moved along its user vector so that its float64 score is target[b, c]
    (up to the fp32 rounding of the row; the reference is computed from the rows as stored)."""
    B, C = target.shape
    H = cdd.shape[1]
    scale = float(scale32(H))
    x, u = cdd.double().view(B, C, H), user.double()
    s0 = (x * u[:, None]).sum(-1) * scale
    x = x + ((target - s0) / scale)[:, :, None] * (u / (u * u).sum(-1, keepdim=True))[:, None, :]
    return x.reshape(B * C, H).float()


@pytest.mark.parametrize("B,C,H", [(3, 4, 64), (2, 65, 3), (2, 130, 65), (1, 257, 8)])
def test_score_log_softmax_range(B, C, H):
    """Scores spanning -60 .. +60: the log-softmax stays finite, within the logit bar, and
    logsumexp(logits) per impression is 0 within 1e-5.  For C > 64 the scores of candidates 0 .. 63
    lie in [-60, -35] and those from 64 on in [35, 60], the largest in the last column: the maximum is
    found on a later trip of the wave-0 loop, 95 above anything the first trip saw (exp(95)
    overflows fp32, so a maximum taken over the first trip alone cannot pass).  Only the largest score
    reaches 60, the rest of the upper group stays under 50: one logit per row is near 0."""
    cdd, user, _ = _score_inputs(B, C, H, 5 + C)
    g = torch.Generator().manual_seed(C)
    r = torch.rand(B, C, generator=g, dtype=torch.float64)
    if C > 64:
        target = torch.where(torch.arange(C)[None] < 64, -60 + 25 * r, 35 + 15 * r)
    else:
        target = -60 + 110 * r
    target[:, 0], target[:, C - 1] = -60.0, 60.0
    cdd = _rows_scoring(cdd, user, target)
    ref = score_reference(cdd, user, B, C, L.SCORE_LOG_SOFTMAX)
    assert (ref["s"] - target).abs().max() < 1e-3 and ref["out"].min() < -110
    _, got = _score_fwd(cdd, user, B, C, H, L.SCORE_LOG_SOFTMAX)
    _check_head(got, ref, None, L.SCORE_LOG_SOFTMAX, "range +-60 B=%d C=%d H=%d" % (B, C, H))
    lse = torch.logsumexp(got, 1).abs().max().item()
    print("range +-60 B=%d C=%d H=%d: max |logsumexp(logits)| = %.3e (bar 1e-5)" % (B, C, H, lse))
    assert lse <= 1e-5


@pytest.mark.parametrize("B,C,H", [(3, 4, 64), (2, 65, 3), (1, 257, 8)])
def test_score_sigmoid_range(B, C, H):
    """Scores out to +-100 under the sigmoid head: exp(-s) overflows fp32 from s = -88.8 down, and
    1 / (1 + inf) must be 0, not NaN.  Finite, in [0, 1], within the logit atol of float64."""
    cdd, user, _ = _score_inputs(B, C, H, 9 + C)
    g = torch.Generator().manual_seed(C + 1)
    target = -100 + 200 * torch.rand(B, C, generator=g, dtype=torch.float64)
    pins = torch.tensor([-100.0, -89.0, -88.0, -60.0, 0.0, 60.0, 88.0, 89.0, 100.0], dtype=torch.float64)
    flat = target.view(-1)
    k = min(len(pins), flat.numel() - 2)
    flat[1:1 + k] = pins[:k]
    target[:, 0], target[:, C - 1] = -100.0, 100.0
    cdd = _rows_scoring(cdd, user, target)
    ref = score_reference(cdd, user, B, C, L.SCORE_SIGMOID)
    assert (ref["s"] - target).abs().max() < 1e-3
    _, got = _score_fwd(cdd, user, B, C, H, L.SCORE_SIGMOID)
    assert (got >= 0).all() and (got <= 1).all()
    err = (got - ref["out"]).abs().max().item()
    print("sigmoid +-100 B=%d C=%d H=%d: max |err| = %.3e (bar %.0e)" % (B, C, H, err, LOGIT_ATOL))
    assert err <= LOGIT_ATOL
    assert got[0, 0] < 1e-30 and got[0, C - 1] == 1.0


@pytest.mark.parametrize("B,C,H,labels", [(3, 65, 16, [64, -100, 7]), (2, 130, 65, [129, -100])])
def test_score_nll_wide(B, C, H, labels):
    """nr_score_nll_fwd / nr_score_nll_bwd at C > 64 (second and third trips of the wave-0 loops)
    against nll_reference, one label ignored; the bars of test_score_nll_kernel_vs_torch; three runs
    on the one self-cleaning ticket."""
    cdd, user, _ = _score_inputs(B, C, H, 3 * B + C)
    label = torch.tensor(labels)
    ref = nll_reference(cdd, user, label, B, C)
    _, cv = _guarded(cdd, 3)
    _, uv = _guarded(user, 5)
    lab = label.cuda()
    one = torch.ones(1, device="cuda")
    for run in range(3):
        lbuf, logits = _nan_flat(B * C, (B, C))
        loss = torch.full((1,), NAN, device="cuda")
        K.score_nll_fwd(cv, uv, lab, B, C, H, logits, loss)
        dcbuf, dcv = _nan_view(B * C, H, 3, 2)
        dubuf, duv = _nan_view(B, H, 5, 2)
        K.score_nll_bwd(cv, uv, logits, lab, one, None, B, C, H, dcv, duv)
        torch.cuda.synchronize()
        assert _tail_intact(lbuf, B * C) and _guards_intact(dcbuf, B * C, H) and _guards_intact(dubuf, B, H)
        rs = (_ratio(logits, ref["logits"], LOGIT_RTOL, LOGIT_ATOL), _ratio(loss[0], ref["loss"], 1e-5, 1e-6),
              _ratio(dcv, ref["dcdd"], GRAD_RTOL, GRAD_ATOL), _ratio(duv, ref["duser"], GRAD_RTOL, GRAD_ATOL))
        print("nll B=%d C=%d H=%d run %d: err / bar: logits %.3f loss %.3f dcdd %.3f duser %.3f" % ((B, C, H, run) + rs))
        assert max(rs) <= 1.0
        b_ign = labels.index(-100)
        assert (dcv[b_ign * C:(b_ign + 1) * C] == 0).all() and (duv[b_ign] == 0).all()
    assert K.self_cleaning_check("cuda") == []


# ---------------------------------------------------------------- XSoftmax

XS_SHAPES = [(1, 1), (5, 2), (9, 63), (4, 64), (7, 65), (3, 130), (6, 300)]
XS_DTYPES = [torch.bool, torch.uint8, torch.int64, torch.float32, torch.float64]


@functools.lru_cache(maxsize=None)
def _xs_inputs(rows, cols):
    """(x fp32 with poisoned masked slots, keep bool, dy): row 0 fully masked, row 1 one kept entry in
    the last column, row 2 fully kept, the rest kept with p = 0.6; row r shifted by (r - rows//2) 1000;
    masked slots hold NaN, +inf, 3e38 in rotation."""
    g = torch.Generator().manual_seed(rows * 1000 + cols)
    keep = torch.rand(rows, cols, generator=g) < 0.6
    keep[0] = False
    if rows > 1:
        keep[1] = False
        keep[1, cols - 1] = True
    if rows > 2:
        keep[2] = True
    x = torch.randn(rows, cols, generator=g) + ((torch.arange(rows) - rows // 2) * 1000.0)[:, None]
    poison = torch.tensor([NAN, float("inf"), 3e38])
    nmask = int((~keep).sum())
    x[~keep] = poison[torch.arange(nmask) % 3]
    dy = torch.randn(rows, cols, generator=g)
    return x, keep, dy


def _typed_mask(keep, dtype):
    if not dtype.is_floating_point:
        return keep.to(dtype)
    vals = torch.tensor([0.5, -2.0], dtype=dtype)[torch.arange(keep.numel()) % 2].view(keep.shape)
    return torch.where(keep, vals, torch.zeros((), dtype=dtype))   # non-unit non-zero where set


@pytest.mark.parametrize("rows,cols", XS_SHAPES)
@pytest.mark.parametrize("mdt", XS_DTYPES, ids=[str(d).split(".")[1] for d in XS_DTYPES])
def test_xsoftmax_kernels(mdt, rows, cols):
    """K.xsoftmax_fwd / K.xsoftmax_bwd directly: cols through the second and later trips of the per-lane
    loops, every mask dtype (any non-zero keeps), NaN / inf / 3e38 in the masked slots of x."""
    x, keep, dy = _xs_inputs(rows, cols)
    mask = _typed_mask(keep, mdt)
    assert torch.equal(mask.bool(), keep)
    want = R.xsoftmax(x.double(), mask)
    assert torch.isfinite(want).all()
    n = rows * cols
    obuf, out = _nan_flat(n, (rows, cols))
    K.xsoftmax_fwd(x.cuda(), mask.cuda(), out)
    torch.cuda.synchronize()
    assert _tail_intact(obuf, n)
    got = out.double().cpu()
    assert torch.isfinite(got).all()
    assert (got[~keep] == 0).all() and (got[0] == 0).all()
    if rows > 1:
        assert got[1, cols - 1] == 1.0 and got[1].sum() == 1.0
    kept_rows = keep.any(1)
    sums = (got[kept_rows].sum(1) - 1).abs().max().item() if kept_rows.any() else 0.0
    err = (got - want).abs().max().item()
    assert sums <= 1e-6 and err <= 1e-6, (sums, err)

    dbuf, dx = _nan_flat(n, (rows, cols))
    K.xsoftmax_bwd(out, dy.cuda(), dx)
    torch.cuda.synchronize()
    assert _tail_intact(dbuf, n)
    gdx = dx.double().cpu()
    berr = (gdx - xsoftmax_bwd_reference(got, dy)).abs().max().item()
    print("xsoftmax %dx%d %s: fwd max |err| %.3e, |row sum - 1| %.3e (bars 1e-6); bwd %.3e (bar 1e-5)"
          % (rows, cols, mdt, err, sums, berr))
    assert torch.isfinite(gdx).all() and (gdx[~keep] == 0).all()
    assert berr <= 1e-5


# ---------------------------------------------------------------- nr_adam

# 2_098_355 = 2048 * 256 * 4 + 4 * 300 + 3: one full round of the 2048-workgroup grid-stride loop, a
# second partial round, and a 3-element tail
ADAM_N = [1, 3, 4, 5, 1023, 4097, 2_098_355]
ADAM_SETTINGS = [("wd0-step1", 0.0, 1.0, 1, False), ("wd-gscale-step7", 0.01, 1.0 / 128, 7, False),
                 ("wd-gscale-devstep7", 0.01, 1.0 / 128, 7, True)]
ADAM_HP = dict(lr=f32(1e-3), b1=f32(0.9), b2=f32(0.999), eps=f32(1e-8))


@functools.lru_cache(maxsize=None)
def _adam_inputs(n):
    """p ~ N(0,1); g, g2 ~ N(0,1) 10^-k, k cycling over 0..2 along the tensor; m, v small positive; from
    n = 8 on a slice with g = g2 = m = v = 0 (away from the n % 4 tail).  -> (p, g, g2, m, v, slice)"""
    gen = torch.Generator().manual_seed(n)
    dec = 10.0 ** -(torch.arange(n) % 3).float()
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * dec
    g2 = torch.randn(n, generator=gen) * dec
    m = torch.randn(n, generator=gen).abs() * 0.01
    v = torch.randn(n, generator=gen).abs() * 0.001
    z = slice(n // 3, n // 3 + min(n // 4, 64)) if n >= 8 else slice(0, 0)
    for t in (g, g2, m, v):
        t[z] = 0
    return p, g, g2, m, v, z


def _adam_check(got, want, what):
    """Each output is at most four fp32 roundings from exact: 2^-22 of the tensor's largest value."""
    worst = 0.0
    for name, a, b in zip("pmv", got, want):
        err = (a.double().cpu() - b).abs().max().item()
        bar = 2.0 ** -22 * b.abs().max().item()
        worst = max(worst, err / bar)
        assert err <= bar, "%s %s: err %.3e, bar %.3e" % (what, name, err, bar)
    return worst


@pytest.mark.parametrize("n", ADAM_N)
@pytest.mark.parametrize("name,wd,gscale,step,dev_step", ADAM_SETTINGS, ids=[s[0] for s in ADAM_SETTINGS])
def test_adam_single_tensor(name, wd, gscale, step, dev_step, n):
    """nr_adam through K.adam against adam_reference, which is fed the same fp32 inputs and the
    fp32-rounded hyper-parameters the kernel receives; a second step from the kernel's own state with
    the reference restarted from it, so that errors do not accumulate into the bar."""
    p0, g1, g2, m0, v0, z = _adam_inputs(n)
    hp = dict(ADAM_HP, wd=f32(wd))
    p, m, v = p0.cuda(), m0.cuda(), v0.cuda()
    step_t = torch.tensor(step, dtype=torch.int64, device="cuda") if dev_step else None
    worst = []
    for k, g in enumerate((g1, g2)):
        before = [t.cpu() for t in (p, m, v)]
        if dev_step:
            step_t.fill_(step + k)
        K.adam(p, g.cuda(), m, v, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], step_t if dev_step else step + k,
               grad_scale=gscale)
        torch.cuda.synchronize()
        if dev_step:
            assert step_t.item() == step + k                   # read, never written
        want = adam_reference(before[0], g, before[1], before[2], hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"],
                              gscale, step + k)
        worst.append(_adam_check((p, m, v), want, "n=%d %s step %d" % (n, name, step + k)))
        if wd == 0:                                            # (with weight decay the slice's gradient is wd p)
            assert (m[z] == 0).all() and (v[z] == 0).all()
            assert torch.equal(p[z].cpu(), p0[z])              # bitwise: g = m = v = 0 moves nothing
    assert (p.cpu() - p0).abs().max() > 1e-6                   # the two steps moved the parameters
    print("adam n=%d %s: max err / (2^-22 max|want|) = %.3f, %.3f" % (n, name, worst[0], worst[1]))


def test_adam_device_step_matches_host_step():
    """The bias corrections formed on the device from an int64 scalar give the bits of the host form."""
    n = 4097
    p0, g1, _, m0, v0, _ = _adam_inputs(n)
    outs = []
    for step in (7, torch.tensor(7, dtype=torch.int64, device="cuda")):
        p, m, v = p0.cuda(), m0.cuda(), v0.cuda()
        K.adam(p, g1.cuda(), m, v, ADAM_HP["lr"], ADAM_HP["b1"], ADAM_HP["b2"], ADAM_HP["eps"], f32(0.01), step,
               grad_scale=1.0 / 128)
        torch.cuda.synchronize()
        outs.append((p, m, v))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_adam_refuses_misaligned_view():
    """nr_adam's float4 accesses need 16-byte alignment: a view offset by one float is refused
    (NR_EINVAL(2)) before anything is launched."""
    for which in range(4):
        ts = [torch.zeros(8, device="cuda") for _ in range(4)]
        buf = torch.ones(9, device="cuda")
        ts[which] = buf[1:]
        assert ts[which].data_ptr() % 16 == 4
        with pytest.raises(L.HipError, match="invalid argument 2"):
            K.adam(ts[0], ts[1], ts[2], ts[3], 1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
        torch.cuda.synchronize()
        assert (buf == 1).all() and all((t == 0).all() for i, t in enumerate(ts) if i != which)


# ---------------------------------------------------------------- row copies

def _sources(V, cols):
    """[V, cols] sources: contiguous, leading dimension cols + 1, cols + 4, and a base offset by one float."""
    g = torch.Generator().manual_seed(V + cols)
    vals = torch.randn(V, cols, generator=g).cuda()
    out = {"contiguous": vals.clone()}
    for pad in (1, 4):
        buf = torch.full((V, cols + pad), NAN, device="cuda")
        buf[:, :cols] = vals
        out["ld=cols+%d" % pad] = buf[:, :cols]
    flat = torch.full((V * cols + 1,), NAN, device="cuda")
    flat[1:] = vals.reshape(-1)
    out["base+1"] = flat[1:].view(V, cols)
    assert out["base+1"].data_ptr() % 16 == 4 and out["contiguous"].data_ptr() % 16 == 0
    return vals, out


@pytest.mark.parametrize("cols", [1, 3, 4, 150, 260])
def test_gather_rows_padded(cols):
    """K.gather_rows into a [:n, :cols] view of a NaN-filled [n+1, cols+4]; sources that take the float4
    path (cols, lds, ldd multiples of 4 and 16-byte bases: cols 4 and 260 -- 65 float4, the second
    trip -- contiguous or ld = cols + 4) and the scalar path (everything else); exact."""
    V, n = 50, 77
    vals, srcs = _sources(V, cols)
    idx = torch.randint(0, V, (n,), generator=torch.Generator().manual_seed(cols))
    idx[0], idx[1], idx[2] = V - 1, 0, V - 1
    idx_d = idx.cuda()
    want = vals[idx_d]
    for name, src in srcs.items():
        buf, out = _nan_view(n, cols, 4, 1)
        assert K.gather_rows(src, idx_d, out) is out
        torch.cuda.synchronize()
        assert torch.equal(out, want), (cols, name)
        assert _guards_intact(buf, n, cols), (cols, name)


@pytest.mark.parametrize("rows,cols", [(64, 64), (65, 1), (1, 65), (130, 67)])
def test_transpose_padded(rows, cols):
    """K.transpose into a [:cols, :rows] view of a NaN-filled [cols+1, rows+5]: whole tiles, one row or
    column past a tile, three tiles by two with ragged edges; padded sources too; exact."""
    _, srcs = _sources(rows, cols)
    for name, src in srcs.items():
        buf, out = _nan_view(cols, rows, 5, 1)
        assert K.transpose(src, out) is out
        torch.cuda.synchronize()
        assert torch.equal(out, src.t()), (rows, cols, name)
        assert _guards_intact(buf, cols, rows), (rows, cols, name)
