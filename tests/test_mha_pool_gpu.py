"""The fused MHA news-encoder tail (csrc/mha_pool.hip) called directly, K.mha_pool_fwd / K.mha_pool_bwd
with the projections y supplied by the test (no GEMM in the path), against the float64 reference of
tests/pool_util.py: all four dispatch() geometries, the forward and every backward form -- fused with
the attention recomputed, fused on the saved O, split LN pass + per-head pass, the last two with and
without the ws gradient copies (3 copies: fewer than the titles, so blockIdx % copies wraps; 32 copies).

Which kernels a test id launches (geometry hHkDKvDV, H = heads * dv):
  forward                  mha_pool_fwd_kernel<DK, DV, H/64, NP>   NP 0 (f32), 3 (bf16x6), 1 (bf16)
  recompute / saved[_ws*]  mha_pool_bwd_kernel<DK, DV, H/64, NP, SAVED>; 6 waves of 2 heads at 12
                           heads, 4 waves of 2 heads at 8
  split[_ws*]              mha_ln_bwd_kernel<H/64>, then mha_head_bwd_kernel<DK, DV, NP> on a
                           (titles, ceil(heads / 4)) grid: gy = 3 at 12 heads, 2 at 8
  *_ws3, *_ws32            ... and copies_reduce_kernel

Every matrix has a leading dimension wider than its row with NaN in the padding, every output starts as
NaN (the accumulated vectors as zero with a NaN tail): the padding must come back NaN bit for bit, every
row of dy written, rows of masked tokens exactly zero.

The bar is tied to the reference: the same reference evaluated in float32 on the CPU differs from
float64 by e32 = max|ref32 - ref64| per tensor, and the kernels must stay within 32 e32 + 32 * 2^-24 *
max|ref64| (the convention of tests/test_rnn_gpu.py), a bar that may itself never exceed 1e-4 *
max|ref64|.  Every case prints its err / e32 ratios ("mha-pool-ratio" lines, pytest -s).  The backward
runs with GEMM_F32 (bf16x6 callers get the same exact f32 products there); NR_GEMM_BF16 has its own
test at the 3e-2 bar of tests/test_cnn_keypool_gpu.py.

Measured on an MI355X at this commit (three runs; the atomic sums vary a little between runs), the
largest err / e32 of any case, per kernel family and output -- no output needed a multiplier above 32,
the largest err / bar of any line was 0.07:
  forward f32      news 1.3  probs 2.7  mean 1.7  rstd 0.8  zout 1.2  oout 1.7
  forward bf16x6   news 1.3  probs 2.7  mean 3.0  rstd 0.8  zout 1.4  oout 1.9
  recompute        dy 1.7  dbias 1.7  dq 1.5  dgamma 2.1  dbeta 1.4
  saved[_ws*]      dy 1.7  dbias 2.2  dq 1.5  dgamma 1.6  dbeta 1.3
  split[_ws*]      dy 1.7  dbias 2.2  dq 1.5  dgamma 1.6  dbeta 1.5   (seg: the distinct-row sums 1.3)
  NR_GEMM_BF16     err / max|ref64| at most 7e-3 (dq); on oout 3.5e-3 against 2e-7 with f32 products

One-line errors tried on a scratch build, each caught: the - sg term of ln_row_dO dropped (every split
case of test_backward, 66, and the split forms of the other tests); scale_attn = 1 / sqrt(dv) (the 20
test_forward and 70 test_backward cases of the two dk != dv geometries); dz skipped in
mha_ln_bwd_kernel (the 36 split cases of test_backward with dz); dbeta summed without the dropout
scale in pool_ln_bwd (the 56 fused cases of test_backward with p_drop = 0.2).
"""
import functools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import restatement as R
from pool_util import mha_pool_inputs, mha_pool_reference, pool_mask

NAN = float("nan")
NAN_BITS = torch.tensor(NAN).view(torch.int32).item()
SEED, OFFSET = 9, 3
F64, F32 = torch.float64, torch.float32

GEOMS = {"h12k64v32": (12, 64, 32), "h12k64v64": (12, 64, 64), "h8k64v32": (8, 64, 32), "h12k32v32": (12, 32, 32)}
# saved O, dob (split), ws copies
FORMS = {"recompute": (False, False, 0), "saved": (True, False, 0), "saved_ws3": (True, False, 3),
         "saved_ws32": (True, False, 32), "split": (True, True, 0), "split_ws3": (True, True, 3),
         "split_ws32": (True, True, 32)}
MULT = {}      # output -> a multiplier of e32 above 32 (see the module docstring); none needed


def _cases():
    out = []
    for g in GEOMS:
        for L in (32, 17):          # the full 32x32 tile; a length that straddles the 16-row half
            for p in (0.0, 0.2):
                out.append((g, L, p, (L == 32) == (p > 0)))      # dz alternates with p_drop
    for g in ("h12k64v32", "h12k64v64"):
        for L in (31, 2, 1):        # one padded row; two slots; a softmax of one element
            out.append((g, L, 0.2, L != 2))
    return out


CASES = _cases()


def _id(c):
    return "%s-L%d-p%s%s" % (c[0], c[1], c[2], "-dz" if c[3] else "")


def make_case(geom, L, p_drop, with_dz, rows=None, yrows=None, seed=SEED, offset=OFFSET, tag=None):
    """Seeded inputs, the mask, the replayed dropout and the float64 / float32 references of one case.
    ``rows``: y is a table of that many rows read through ``yrows`` (default: a seeded index with
    repeats); the reference gathers first."""
    heads, dk, dv = GEOMS[geom]
    mask = pool_mask(L)
    n, H = mask.shape[0], heads * dv
    inp = mha_pool_inputs(n, L, heads, dk, dv, 100 * L + heads + dk + dv + int(10 * p_drop), rows=rows)
    if rows is not None and yrows is None:
        yrows = torch.randint(0, rows, (n * L,), generator=torch.Generator().manual_seed(L))
        assert yrows.unique().numel() < n * L
    keep = R.dropout_keep(seed, offset, n * L, H, p_drop) if p_drop > 0 else None
    y_tok = inp["y"] if yrows is None else inp["y"][yrows]
    ref = {dt: mha_pool_reference(y_tok, mask, heads, dk, dv, inp["gamma"], inp["beta"], inp["q"], keep, p_drop,
                                  dnews=inp["dnews"], dz=inp["dz"] if with_dz else None, dtype=dt)
           for dt in (F64, F32)}
    return types.SimpleNamespace(geom=geom, heads=heads, dk=dk, dv=dv, L=L, n=n, T=n * L, H=H, NY=heads * (dk + dv),
                                 p_drop=p_drop, with_dz=with_dz, mask=mask, inp=inp, keep=keep, ref=ref, yrows=yrows,
                                 tag=tag or "%s-L%d-p%s%s" % (geom, L, p_drop, "-dz" if with_dz else ""))


@functools.lru_cache(maxsize=None)
def case(*key, **kw):
    """make_case, computed once per key and shared by the forward and backward tests."""
    return make_case(*key, **kw)


# ---------------------------------------------------------------------- buffers

@pytest.fixture(scope="module", autouse=True)
def _leave_no_blocks_behind():
    """The later modules of the suite see the caching allocator as they would without this one (a test
    of tests/test_row_grad_gpu.py depends on which block a freed gradient's successor gets): drop the
    cached forwards and the cached blocks this module's buffers came from."""
    yield
    fwd_f32.cache_clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


def _padded(t, pad):
    """t on the device inside a NaN buffer ``pad`` columns wider; -> (buffer, the view holding t)."""
    buf = _nan(t.shape[0], t.shape[1] + pad)
    buf[:, :t.shape[1]] = t.cuda()
    return buf, buf[:, :t.shape[1]]


def _vec(n, fill=NAN, tail=3):
    """A vector of n ``fill`` followed by ``tail`` NaN; -> (buffer, the view of the n)."""
    buf = _nan(n + tail)
    buf[:n] = fill
    return buf, buf[:n]


def _all_nan_bits(t):
    return bool((t.contiguous().view(torch.int32) == NAN_BITS).all())


def _prec(name):
    from newsrec_amd import _lib as L
    return {"f32": L.GEMM_F32, "bf16x6": L.GEMM_BF16X6, "bf16": L.GEMM_BF16}[name]


def run_fwd(c, prec, mask=None, rng=None, seed=SEED, offset=OFFSET):
    """One nr_mha_pool_fwd with zout and oout into NaN-filled buffers: ldy, ldo wider by 4 (the entry
    wants multiples of 4), ldn and ldz by odd amounts.  -> the device buffers by name."""
    from newsrec_amd import kernels as K
    b = types.SimpleNamespace()
    b.ybuf, b.y = _padded(c.inp["y"], 4)
    b.mask = (c.mask if mask is None else mask).cuda()
    b.yrows = c.yrows.cuda() if c.yrows is not None else None
    b.gamma, b.beta, b.q = c.inp["gamma"].cuda(), c.inp["beta"].cuda(), c.inp["q"].cuda()
    b.news, b.zout, b.oout = _nan(c.n, c.H + 3), _nan(c.T, c.H + 5), _nan(c.T, c.H + 4)
    b.stats, b.probs = _vec(2 * c.T)[0], _vec(c.T, tail=5)[0]
    b.rng, b.seed, b.offset = rng, seed, offset
    K.mha_pool_fwd(b.y, b.mask, c.n, c.L, c.heads, c.dk, c.dv, b.gamma, b.beta, b.q, b.news[:, :c.H], b.stats, b.probs,
                   p_drop=c.p_drop, seed=seed, offset=offset, zout=b.zout[:, :c.H], yrows=b.yrows, rng=rng,
                   oout=b.oout[:, :c.H], prec=_prec(prec))
    torch.cuda.synchronize()
    return b


@functools.lru_cache(maxsize=None)
def fwd_f32(key):
    """The GEMM_F32 forward of a case, run once: test_forward checks it, the backward tests run on its
    stats / probs / oout (and check that they leave them as they were)."""
    return run_fwd(case(*key), "f32")


def run_bwd(c, f, form, prec="f32", preload=0.0, seg=None, dy_extra=0, dy_pad=5):
    """One nr_mha_pool_bwd of ``form`` on the forward's outputs ``f``; dy and dob start as NaN, the
    accumulated vectors as ``preload``, ws as zero; lddy wider than the row by ``dy_pad``, lddz and ldn by
    3, lddob by 4.  -> the buffers by name, on the CPU (dy stays on the device with ``seg``)."""
    from newsrec_amd import kernels as K
    saved, split, copies = FORMS[form]
    _, dnews = _padded(c.inp["dnews"], 3)
    dz = _padded(c.inp["dz"], 3)[1] if c.with_dz else None
    dy = _nan(c.T + dy_extra, c.NY + dy_pad)
    vec = {k: _vec(w, preload) for k, w in (("dbias", c.NY), ("dq", c.H), ("dgamma", c.H), ("dbeta", c.H))}
    dob = _nan(c.T, 12) if split else None
    ws = torch.zeros(copies, (3 * c.H + c.NY + 3) // 4 * 4, device="cuda") if copies else None
    K.mha_pool_bwd(f.y, f.mask, c.n, c.L, c.heads, c.dk, c.dv, f.gamma, f.beta, f.q, f.stats, f.probs, dnews,
                   dy[:, :c.NY] if seg is not None else dy[:c.T, :c.NY], vec["dbias"][1], vec["dq"][1], vec["dgamma"][1],
                   vec["dbeta"][1], p_drop=c.p_drop, seed=f.seed, offset=f.offset, dz=dz, yrows=f.yrows, rng=f.rng,
                   o=f.oout[:, :c.H] if saved else None, dob=dob[:, :8] if split else None, prec=_prec(prec), ws=ws,
                   ws_copies=copies, seg=seg, dyu_row0=c.T if seg is not None else 0)
    torch.cuda.synchronize()
    if ws is not None:
        assert not bool(ws.any().item()), "ws is not left zero"
    if dob is not None:
        assert _all_nan_bits(dob[:, 8:]), "dob: written past column 8"
    out = {k: v[0].cpu() for k, v in vec.items()}
    out["dy"] = dy if seg is not None else dy.cpu()
    return out


# ---------------------------------------------------------------------- checks

def compare(c, what, pairs, late):
    """pairs: (name, got, key into the references or a (ref64, ref32) pair[, slack added to the bar]).
    Prints the ratio line of each, asserts its bar against the 1e-4 cap and collects the misses in
    ``late``."""
    for name, got, key, *slack in pairs:
        want, w32 = (c.ref[F64][key], c.ref[F32][key]) if isinstance(key, str) else key
        got = got.double().reshape(want.shape)
        scale = want.abs().max().item()
        e32 = (w32.double() - want).abs().max().item()
        bar = MULT.get(name, 32) * e32 + 32 * 2.0 ** -24 * scale
        err = (got - want).abs().max().item()
        print("mha-pool-ratio %s %s %-6s err %.3e e32 %.3e err/e32 %s bar %.3e max %.3e"
              % (c.tag, what, name, err, e32, "%.2f" % (err / e32) if e32 > 0 else "-", bar, scale))
        assert bar <= 1e-4 * scale, "%s: the bar %.3e exceeds 1e-4 of max %.3e" % (name, bar, scale)
        if not err <= bar + sum(slack):
            late.append("%s: err %.3e > bar %.3e (e32 %.3e, max %.3e)" % (name, err, bar, e32, scale))


def check_fwd_layout(c, f, mask=None):
    """Nothing written past a row's width, everything inside it written; the exact zeros."""
    m = ((c.mask if mask is None else mask) != 0)
    for name, buf, width in (("news", f.news, c.H), ("zout", f.zout, c.H), ("oout", f.oout, c.H)):
        assert _all_nan_bits(buf[:, width:]), "%s: written past column %d" % (name, width)
        assert torch.isfinite(buf[:, :width]).all(), "%s: unwritten or non-finite values" % name
    assert _all_nan_bits(f.stats[2 * c.T:]) and _all_nan_bits(f.probs[c.T:]), "stats / probs: written past T rows"
    assert torch.isfinite(f.stats[:2 * c.T]).all() and torch.isfinite(f.probs[:c.T]).all()
    assert _all_nan_bits(f.ybuf[:, c.NY:])
    assert (f.news[0, :c.H] == 0).all(), "news of the fully masked title is not zero"
    assert (f.probs[:c.T].cpu()[~m.reshape(-1)] == 0).all(), "probs of masked tokens are not zero"
    assert (f.oout[:, :c.H].cpu()[~m.reshape(-1)] == 0).all(), "O of masked tokens is not zero"
    if c.keep is not None:
        assert (f.zout[:, :c.H].cpu()[~c.keep] == 0).all(), "zout is not zero where the dropout drops"


def fwd_pairs(c, f):
    st = f.stats[:2 * c.T].cpu().reshape(c.T, 2)
    r64, r32 = c.ref[F64]["stats"], c.ref[F32]["stats"]
    return [("news", f.news[:, :c.H].cpu(), "news"), ("probs", f.probs[:c.T].cpu(), "probs"),
            ("mean", st[:, 0], (r64[:, 0], r32[:, 0])), ("rstd", st[:, 1], (r64[:, 1], r32[:, 1])),
            ("zout", f.zout[:, :c.H].cpu(), "Z"), ("oout", f.oout[:, :c.H].cpu(), "O")]


def check_bwd(c, out, what, late, preload=0.0):
    dy = out["dy"]
    assert _all_nan_bits(dy[:, c.NY:]), "dy: written past column %d" % c.NY
    assert torch.isfinite(dy[:, :c.NY]).all(), "dy: rows not written, or non-finite values"
    assert (dy[:, :c.NY][(c.mask == 0).reshape(-1)] == 0).all(), "dy rows of masked tokens are not exactly zero"
    pairs = [("dy", dy[:, :c.NY], "dy")]
    for name, w in (("dbias", c.NY), ("dq", c.H), ("dgamma", c.H), ("dbeta", c.H)):
        assert _all_nan_bits(out[name][w:]) and torch.isfinite(out[name][:w]).all(), name
        if c.ref[F64][name].abs().max() == 0:
            # L = 1: one pooling score per title, p in {0, 1}, ds = p (dp - p dp) is exactly 0 in the
            # kernels' own arithmetic too -- no rounding residue to allow for
            assert (out[name][:w] == preload).all(), "%s must be exactly zero" % name
        # onto a preloaded value up to n + 1 additions land (the titles' atomics, the copies' sum), each
        # rounding at the magnitude of constant + gradient: that many half-ulps on top of the bar
        slack = (c.n + 1) * 2.0 ** -24 * (c.ref[F64][name] + preload).abs().max().item() if preload else 0.0
        pairs.append((name, out[name][:w].double() - preload, name, slack))
    compare(c, what, pairs, late)


# ---------------------------------------------------------------------- forward, backward forms

@pytest.mark.parametrize("prec", ["f32", "bf16x6"])
@pytest.mark.parametrize("key", CASES, ids=[_id(c) for c in CASES])
def test_forward(key, prec):
    c = case(*key)
    f = fwd_f32(key) if prec == "f32" else run_fwd(c, prec)
    check_fwd_layout(c, f)
    late = []
    compare(c, "fwd-" + prec, fwd_pairs(c, f), late)
    assert not late, "; ".join(late)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("key", CASES, ids=[_id(c) for c in CASES])
def test_backward(key, form):
    """Every form against the reference (never against one another).  At L = 1 dq is exactly zero."""
    c = case(*key)
    f = fwd_f32(key)
    before = [t.clone() for t in (f.ybuf, f.oout, f.stats, f.probs)]
    out = run_bwd(c, f, form)
    for a, t in zip(before, (f.ybuf, f.oout, f.stats, f.probs)):
        assert torch.equal(a.view(torch.int32), t.view(torch.int32)), "the backward changed one of its inputs"
    late = []
    check_bwd(c, out, form, late)
    assert not late, "; ".join(late)
    if c.L == 1:
        assert (out["dq"][:c.H] == 0).all()


@pytest.mark.parametrize("form", ["recompute", "saved", "saved_ws3", "split", "split_ws32"])
def test_backward_accumulates(form):
    """The accumulate contract: dbias, dq, dgamma, dbeta preloaded with a constant come back as
    constant + gradient, from the plain forms and through the ws copies."""
    key = ("h12k64v64", 17, 0.2, True)
    c, f = case(*key), fwd_f32(key)
    out = run_bwd(c, f, form, preload=0.75)
    late = []
    check_bwd(c, out, form + "-acc", late, preload=0.75)
    assert not late, "; ".join(late)


# ---------------------------------------------------------------------- other argument forms

def _fwd_bwd(c, f, forms, what):
    check_fwd_layout(c, f)
    late = []
    compare(c, what + "-fwd", fwd_pairs(c, f), late)
    for form in forms:
        check_bwd(c, run_bwd(c, f, form), what + "-" + form, late)
    assert not late, "; ".join(late)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64, torch.float64, torch.float32],
                         ids=["u8", "i64", "f64", "f32"])
def test_mask_dtypes(dtype):
    """Every mask dtype of kernels.mask_arg; the floating masks with values other than 1 (nonzero = a
    token, whatever the value)."""
    c = case("h12k64v64", 17, 0.2, True)
    m = c.mask.to(dtype)
    if dtype.is_floating_point:
        m = m * torch.where(torch.arange(c.L) % 2 == 0, 2.5, -1.0).to(dtype)
    elif dtype == torch.int64:
        m = m << 40                   # nonzero only above bit 32
    _fwd_bwd(c, run_fwd(c, "f32", mask=m), ["recompute", "split_ws3"], "mask-" + str(dtype).split(".")[1])


def test_yrows_table():
    """yrows: the projections are a table of fewer rows read through an index with repeats; dy stays
    per token."""
    c = case("h8k64v32", 17, 0.2, False, rows=40)
    _fwd_bwd(c, run_fwd(c, "f32"), ["recompute", "saved", "split"], "yrows")


def test_device_rng_key():
    """rng: the dropout key comes from the device pair (seed, base) with the entry's offset added to
    the base -- the reference's keep mask is dropout_keep(seed, base + k)."""
    seed, base, k = 12345, 1000, 77
    c = case("h12k32v32", 17, 0.2, True, seed=seed, offset=base + k)
    rng = torch.tensor([seed, base], dtype=torch.int64, device="cuda")
    f = run_fwd(c, "f32", rng=rng, seed=1, offset=k)     # the host seed is not the one used
    _fwd_bwd(c, f, ["recompute", "saved_ws32", "split"], "rng")


@pytest.mark.parametrize("form", ["recompute", "saved", "split"])
def test_seg_direct_rows(form):
    """seg / dyu_row0: a token alone in its distinct row's segment writes its gradient row to dy row
    dyu_row0 + u; after segment_sum_multi the per-distinct-row sums are the reference's dy summed per
    distinct row over the unmasked tokens."""
    from newsrec_amd import kernels as K
    geom, L, V = "h12k64v64", 17, 60
    mask = pool_mask(L)
    T = mask.numel()
    ids = torch.randint(1, V, (T,), generator=torch.Generator().manual_seed(6))
    ur = K.UniqueRows(ids.cuda(), V, grad_mask=mask.cuda())
    inv = ur.inv.cpu()
    U = int(ur.counts[0].item())
    c = make_case(geom, L, 0.2, True, rows=ur.cap, yrows=inv, tag="%s-L%d-seg" % (geom, L))
    ref = c.ref
    f = run_fwd(c, "f32")
    check_fwd_layout(c, f)
    out = run_bwd(c, f, form, seg=ur, dy_extra=ur.cap, dy_pad=4)     # segment_sum_multi wants ld % 4 == 0
    dyall = out["dy"]
    ur.segment_sum_multi(dyall[:T, :c.NY], dyall[T:, :c.NY])
    torch.cuda.synchronize()
    dyall = dyall.cpu()
    assert _all_nan_bits(dyall[:, c.NY:]), "dy: written past column %d" % c.NY
    seg = ur.seg_off.cpu().long()
    counts = seg[1:U + 1] - seg[:U]
    assert (counts == 1).any() and (counts > 1).any()
    sums = {}
    live = (mask != 0).reshape(-1)
    for dt in (F64, F32):
        sums[dt] = torch.zeros(U, c.NY, dtype=dt).index_add_(0, inv[live], ref[dt]["dy"][live])
    assert torch.isfinite(dyall[T:T + U, :c.NY]).all()
    late = []
    pairs = [("dyu", dyall[T:T + U, :c.NY], (sums[F64], sums[F32]))]
    pairs += [(k, out[k][:ref[F64][k].numel()], k) for k in ("dbias", "dq", "dgamma", "dbeta")]
    compare(c, "seg-" + form, pairs, late)
    assert not late, "; ".join(late)


# ---------------------------------------------------------------------- NR_GEMM_BF16

@pytest.mark.parametrize("geom", list(GEOMS))
def test_bf16_products(geom):
    """NR_GEMM_BF16: one bf16 product in the forward and the backward, at 3e-2 of each tensor's
    largest value (the bf16 level of tests/test_cnn_keypool_gpu.py) -- and visibly worse than the f32
    run of the same case on the attention output, so the bf16 path was in fact taken."""
    key = (geom, 32, 0.0, False)
    c = case(*key)
    f = run_fwd(c, "bf16")
    check_fwd_layout(c, f)
    got = dict((n, g) for n, g, _ in fwd_pairs(c, f))
    refs = dict((n, k) for n, _, k in fwd_pairs(c, f))
    for form in ("recompute", "split"):
        out = run_bwd(c, f, form, prec="bf16")
        assert torch.isfinite(out["dy"][:, :c.NY]).all() and _all_nan_bits(out["dy"][:, c.NY:])
        for k in ("dy", "dbias", "dq", "dgamma", "dbeta"):
            got[form + " " + k] = out[k][:, :c.NY] if k == "dy" else out[k][:c.ref[F64][k].numel()]
            refs[form + " " + k] = k
    late = []
    for name, g in got.items():
        want = c.ref[F64][refs[name]] if isinstance(refs[name], str) else refs[name][0]
        scale = want.abs().max().item()
        err = (g.double().reshape(want.shape) - want).abs().max().item()
        print("mha-pool-ratio %s bf16 %-16s err %.3e max %.3e err/max %.2e" % (c.tag, name, err, scale, err / scale))
        if not err <= 3e-2 * scale:
            late.append("%s: err %.3e > 3e-2 of max %.3e" % (name, err, scale))
    assert not late, "; ".join(late)
    O = c.ref[F64]["O"]
    err_bf16 = (f.oout[:, :c.H].cpu().double() - O).abs().max().item()
    err_f32 = (fwd_f32(key).oout[:, :c.H].cpu().double() - O).abs().max().item()
    assert err_bf16 > 4 * err_f32, "oout: bf16 err %.3e is not worse than f32's %.3e" % (err_bf16, err_f32)


# ---------------------------------------------------------------------- argument errors

def _err_buffers(heads, dk, dv, n, L):
    """NaN-filled arguments of the right sizes for one forward and one backward call."""
    T, H, NY = n * L, heads * dv, heads * (dk + dv)
    a = types.SimpleNamespace(T=T, H=H, NY=NY)
    a.y, a.mask = torch.zeros(T, NY, device="cuda"), torch.ones(n, L, dtype=torch.int64, device="cuda")
    a.gamma, a.beta, a.q = (torch.ones(H, device="cuda") for _ in range(3))
    a.dnews, a.o = torch.ones(n, H, device="cuda"), torch.zeros(T, H, device="cuda")
    a.out = {k: _nan(*s) for k, s in (("news", (n, H)), ("stats", (T, 2)), ("probs", (T,)), ("zout", (T, H)),
                                      ("oout", (T, H)), ("dy", (T, NY)), ("dbias", (NY,)), ("dq", (H,)),
                                      ("dgamma", (H,)), ("dbeta", (H,)), ("dob", (T, 8)))}
    return a


def _expect(code, entry, a, fn):
    from newsrec_amd import _lib as L
    with pytest.raises(L.HipError, match=r"^%s: invalid argument %d$" % (entry, code)):
        fn()
    torch.cuda.synchronize()
    for k, v in a.out.items():
        assert _all_nan_bits(v), "%s was written by a call that failed its argument check" % k


@pytest.mark.parametrize("heads,dk,dv,L,code", [(12, 64, 32, 33, 0), (12, 48, 32, 8, 8), (12, 64, 24, 8, 9)],
                         ids=["L33", "geometry", "H-not-64k"])
def test_shape_errors(heads, dk, dv, L, code):
    from newsrec_amd import kernels as K
    n = 2
    a = _err_buffers(heads, dk, dv, n, L)
    o = a.out
    _expect(code, "nr_mha_pool_fwd", a, lambda: K.mha_pool_fwd(
        a.y, a.mask, n, L, heads, dk, dv, a.gamma, a.beta, a.q, o["news"], o["stats"], o["probs"], zout=o["zout"],
        oout=o["oout"], prec=_prec("f32")))
    for kw in ({}, {"o": a.o}, {"o": a.o, "dob": o["dob"]}):
        _expect(code, "nr_mha_pool_bwd", a, lambda: K.mha_pool_bwd(
            a.y, a.mask, n, L, heads, dk, dv, a.gamma, a.beta, a.q, a.o[:, :2].contiguous(), a.o[:, 0].contiguous(),
            a.dnews, o["dy"], o["dbias"], o["dq"], o["dgamma"], o["dbeta"], prec=_prec("f32"), **kw))


def test_backward_argument_errors():
    from newsrec_amd import _lib as Lb, kernels as K
    heads, dk, dv, n, L = 12, 64, 32, 1, 1
    a = _err_buffers(heads, dk, dv, n, L)
    o = a.out
    stats, probs = torch.zeros(a.T, 2, device="cuda"), torch.zeros(a.T, device="cuda")

    def bwd(dy=o["dy"], **kw):
        K.mha_pool_bwd(a.y, a.mask, n, L, heads, dk, dv, a.gamma, a.beta, a.q, stats, probs, a.dnews, dy, o["dbias"],
                       o["dq"], o["dgamma"], o["dbeta"], prec=_prec("f32"), **kw)

    # lddob < 8
    o["dob4"] = _nan(a.T, 4)
    assert o["dob4"].stride(0) == 4
    _expect(3, "nr_mha_pool_bwd", a, lambda: bwd(o=a.o, dob=o["dob4"]))
    # dy_rows * lddy * 4 >= 2^32: a one-row view whose row stride alone reaches it (nothing that large
    # is allocated, and nothing is launched)
    wide = torch.as_strided(o["dy"], (1, a.NY), (1 << 30, 1))
    assert wide.stride(0) == 1 << 30
    _expect(6, "nr_mha_pool_bwd", a, lambda: bwd(dy=wide))
    # ws without the saved O: kernels.mha_pool_bwd refuses that itself, the entry with its own code
    ws = torch.zeros(3, (3 * a.H + a.NY + 3) // 4 * 4, device="cuda")
    with pytest.raises(Lb.HipError, match="ws needs the saved O"):
        bwd(ws=ws, ws_copies=3)
    z = Lb.ptr(None)
    mp, mdt = K.mask_arg(a.mask, a.T)
    _expect(5, "nr_mha_pool_bwd", a, lambda: Lb.call(
        "nr_mha_pool_bwd", Lb.ptr(a.y), a.y.stride(0), z, mp, mdt, n, L, heads, dk, dv, Lb.ptr(a.gamma), Lb.ptr(a.beta),
        0.0, 0, 0, z, Lb.ptr(a.q), Lb.ptr(stats), Lb.ptr(probs), Lb.ptr(a.dnews), a.dnews.stride(0), z, 0, z, 0, z, 0,
        Lb.ptr(o["dy"]), o["dy"].stride(0), Lb.ptr(o["dbias"]), Lb.ptr(o["dq"]), Lb.ptr(o["dgamma"]), Lb.ptr(o["dbeta"]),
        Lb.ptr(ws), 3, z, 0, a.T, z, _prec("f32"), Lb.stream_ptr(a.y)))
    assert not bool(ws.any().item())
