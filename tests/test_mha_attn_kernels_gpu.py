"""The tied-QK attention core (csrc/mha_attn.hip) called directly, K.mha_attn_fwd / K.mha_attn_bwd, and
the fused eval user encoder K.mha_user_pool_fwd (csrc/mha_pool.hip), against the float64 references of
tests/attn_util.py on the attn_mask(L) batch: prefixes, the empty sequence, holes, every third slot and,
past L = 32, a masked middle block of 16 keys and a sequence whose first 32 slots are masked.

Which kernels a case launches (dispatch() of mha_attn.hip):
  L <= 32   mha_attn_fwd_kernel / mha_attn_bwd_kernel<32, dk, dv>: one wave per two heads, a row per lane
            (dk, dv) in (64,32) (32,32) (64,64) (64,16) (16,16), L in 1, 2, 16, 17, 31, 32
  L  > 32   mha_attn_fwd_split_kernel / mha_attn_bwd_split_kernel<dk, dv>: four waves per head, 16 keys each,
            partial (max, sum, P V) merged through LDS
            (dk, dv) in (32,32) (64,64) (16,16) (64,32), L in 33, 47, 48, 49, 63, 64
each at 12 heads and, at one length per instantiation, at 3 heads (the second half-wave of the last
workgroup idle when two heads share a wave) and at 1 head; the mask dtype cycles over bool, u8, int64,
float32, float64 (kept slots with values other than 1, -0.0 in cleared ones), so that every dtype meets
both families.

qk and v are column views of one Y buffer, dqk and dv of one dY buffer (as the callers hold them); Y, dout
carry NaN padding columns, out and dY sit inside NaN buffers with a spare row above and below and spare
columns: the padding must come back NaN bit for bit, every element inside the views written, rows of
masked tokens and of the empty sequence exactly zero.  dbias starts from seeded non-zero values with a
NaN tail.

The bar is tied to the reference: the same reference evaluated in float32 on the CPU differs from float64
by e32 = max|ref32 - ref64| per tensor, and the kernels must stay within 32 e32 + 32 * 2^-24 * max|ref64|
(the convention of tests/test_mha_pool_gpu.py and tests/test_rnn_gpu.py), a bar that may itself never
exceed 1e-4 * max|ref64|; where max|ref64| is 0 (dqk at L = 1) the kernel's output must be exactly 0.
dbias is compared after its start is taken off, with the rounding of the n accumulating additions onto
that start added to the bar (check_bwd).  Every case prints its err / e32 ratios ("mha-attn-ratio"
lines, pytest -s).  nr_mha_user_pool_fwd keeps the bars of tests/test_attn_gpu.py: 2e-5 * max|ref64| with
f32 and bf16x6 products, 3e-2 with bf16.

Measured on an MI355X at this commit, the largest err / e32 of any case, per kernel family and output -- no
output needed a multiplier above 32 (dbias included), the largest err / bar of any line was 0.05:
  L <= 32 kernels   out 1.3 (rows table 1.3, large scores 1.0)  dqk 1.7  dv 1.5  dbias_k 1.5  dbias_v 2.3
  split kernels     out 1.5 (rows table 0.7, large scores 0.4)  dqk 2.1  dv 1.4  dbias_k 1.3  dbias_v 1.8
  user pool         f32 1.6, bf16x6 1.6 (err / max|ref64| at most 1.2e-7 in both); bf16 err / max|ref64| at
                    most 3.5e-3; at L = 1 the f32 and bf16x6 vectors are exact
Every case passed as the kernels stand: none of the arms listed above hid a fault.

One-line errors tried on a scratch build of mha_attn.hip (none changes an address or a launch), each
caught: the dS_ji term of dKp dropped in both backward kernels (the 65 test_backward cases with L > 1;
at L = 1 dqk is zero either way); f[ww] = 1 in the split forward's merge (all 32 split test_forward cases,
the split rows-table and large-score cases); row_ok ignored in softmax_row (33 test_forward and
33 test_backward cases of the L <= 32 kernels, through the exact zeros of masked rows) and in split_scores
(all 32 + 32 split cases likewise); scale = 1 / sqrt(dv) (the 21 + 21 forward and backward cases of the
dk != dv geometries (64,32) and (64,16) with L > 1, in both families).
"""
import functools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from attn_util import attn_inputs, attn_mask, mha_attn_reference, mha_user_pool_reference

NAN = float("nan")
NAN_BITS = torch.tensor(NAN).view(torch.int32).item()
F64, F32 = torch.float64, torch.float32
PAD = 4                   # spare columns (the entries want leading dimensions that are multiples of 4)

INST = {32: ((64, 32), (32, 32), (64, 64), (64, 16), (16, 16)), 64: ((32, 32), (64, 64), (16, 16), (64, 32))}
LENGTHS = {32: (1, 2, 16, 17, 31, 32), 64: (33, 47, 48, 49, 63, 64)}
MASK_DTYPES = (torch.bool, torch.uint8, torch.int64, torch.float32, torch.float64)
MULT = {}      # output -> a multiplier of e32 above 32 (see the module docstring); none needed


def _cases():
    out = []
    for lmax in (32, 64):
        for i, (dk, dv) in enumerate(INST[lmax]):
            shapes = [(L, 12) for L in LENGTHS[lmax]]
            shapes += [(LENGTHS[lmax][(i + 3) % 6], 3), (LENGTHS[lmax][(i + 4) % 6], 1)]
            for L, heads in shapes:
                out.append((L, heads, dk, dv, MASK_DTYPES[len(out) % len(MASK_DTYPES)]))
    return out


CASES = _cases()
for _lmax in (32, 64):      # every mask dtype meets both kernel families
    assert {c[4] for c in CASES if (c[0] <= 32) == (_lmax == 32)} == set(MASK_DTYPES)


def _id(c):
    return "L%d-h%dk%dv%d-%s" % (c[0], c[1], c[2], c[3], str(c[4]).split(".")[1])


def make_case(L, heads, dk, dv, mdt, rows=None, qk_scale=None, with_bwd=True):
    """Seeded inputs, the mask and the float64 / float32 references of one case.  ``rows``: qk / v are
    a table of that many rows read through a seeded index with repeats; the reference gathers first.
    ``qk_scale``: qk times that factor."""
    mask = attn_mask(L, mdt)
    n = mask.shape[0]
    inp = attn_inputs(n, L, heads, dk, dv, 1000 * L + 10 * heads + dk + dv, rows=rows)
    if qk_scale is not None:
        inp["qk"] = inp["qk"] * qk_scale
    idx = None
    if rows is not None:
        idx = torch.randint(0, rows, (n * L,), generator=torch.Generator().manual_seed(L))
        assert rows < n * L and idx.unique().numel() < n * L
    ref = {dt: mha_attn_reference(inp["qk"], inp["v"], mask, heads, dk, dv, dout=inp["dout"] if with_bwd else None,
                                  rows=idx, dtype=dt) for dt in (F64, F32)}
    return types.SimpleNamespace(L=L, heads=heads, dk=dk, dv=dv, n=n, T=n * L, NQ=heads * dk, NV=heads * dv, mask=mask,
                                 inp=inp, ref=ref, rows=idx, tag=_id((L, heads, dk, dv, mdt)))


@functools.lru_cache(maxsize=None)
def case(*key, **kw):
    """make_case, computed once per key and shared by the forward and backward tests."""
    return make_case(*key, **kw)


@pytest.fixture(scope="module", autouse=True)
def _leave_no_blocks_behind():
    """The later modules of the suite see the caching allocator as they would without this one (a test
    of tests/test_row_grad_gpu.py depends on which block a freed gradient's successor gets)."""
    yield
    case.cache_clear()
    pool_case.cache_clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------- buffers

def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


def _all_nan_bits(t):
    return bool((t.contiguous().view(torch.int32) == NAN_BITS).all())


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _framed(rows, cols):
    """A NaN buffer with a spare row above and below and PAD spare columns; -> (buffer, the view)."""
    buf = _nan(rows + 2, cols + PAD)
    return buf, buf[1:rows + 1, :cols]


def _frame_untouched(buf, rows, cols):
    return _all_nan_bits(buf[0]) and _all_nan_bits(buf[rows + 1]) and _all_nan_bits(buf[:, cols:])


def y_buffer(c, qk, v, spare_rows=0):
    """[qk | v | NaN] in one buffer, ``spare_rows`` all-NaN rows below; -> (Y, the qk view, the v view)."""
    Y = _nan(qk.shape[0] + spare_rows, c.NQ + c.NV + PAD)
    Y[:qk.shape[0], :c.NQ] = qk.cuda()
    Y[:qk.shape[0], c.NQ:c.NQ + c.NV] = v.cuda()
    return Y, Y[:, :c.NQ], Y[:, c.NQ:c.NQ + c.NV]


def run_fwd(c, Y, qk, v, rows=None):
    """One nr_mha_attn_fwd into a framed NaN buffer; the checks every forward must pass; -> out (CPU)."""
    from newsrec_amd import kernels as K
    before = Y.clone()
    obuf, out = _framed(c.T, c.NV)
    K.mha_attn_fwd(qk, v, c.mask.cuda(), c.n, c.L, c.heads, c.dk, c.dv, out, rows=rows)
    torch.cuda.synchronize()
    assert _same_bits(before, Y), "the forward changed its inputs"
    assert _frame_untouched(obuf, c.T, c.NV), "out: written outside its %d x %d view" % (c.T, c.NV)
    out = out.cpu()
    assert torch.isfinite(out).all(), "out: unwritten or non-finite values"
    dead = (c.mask == 0).reshape(-1)
    assert (out[dead] == 0).all(), "out rows of masked tokens are not exactly zero"
    assert (out[:c.L] == 0).all(), "out of the empty sequence is not zero"
    return out


def run_bwd(c, Y, qk, v, with_dbias=True):
    """One nr_mha_attn_bwd: dqk and dv column views of one framed NaN dY, dout inside a wider NaN buffer,
    dbias from its seeded start with a NaN tail.  -> dict of CPU tensors (dbias with the start taken off)."""
    from newsrec_amd import kernels as K
    dobuf = _nan(c.T, c.NV + PAD)
    dobuf[:, :c.NV] = c.inp["dout"].cuda()
    dybuf, dy = _framed(c.T, c.NQ + c.NV)
    dbuf = _nan(c.NQ + c.NV + 3)
    dbuf[:c.NQ + c.NV] = c.inp["dbias0"].cuda()
    before = [t.clone() for t in (Y, dobuf)]
    K.mha_attn_bwd(qk, v, c.mask.cuda(), c.n, c.L, c.heads, c.dk, c.dv, dobuf[:, :c.NV], dy[:, :c.NQ],
                   dy[:, c.NQ:], dbias=dbuf if with_dbias else None)
    torch.cuda.synchronize()
    for a, t in zip(before, (Y, dobuf)):
        assert _same_bits(a, t), "the backward changed one of its inputs"
    assert _frame_untouched(dybuf, c.T, c.NQ + c.NV), "dqk / dv: written outside the dY view"
    assert _all_nan_bits(dbuf[c.NQ + c.NV:]), "dbias: written past heads*(dk+dv)"
    dy = dy.cpu()
    assert torch.isfinite(dy).all(), "dqk / dv: unwritten or non-finite values"
    dead = (c.mask == 0).reshape(-1)
    assert (dy[dead] == 0).all(), "dqk / dv rows of masked tokens are not exactly zero"
    db = dbuf[:c.NQ + c.NV].cpu()
    assert torch.isfinite(db).all()
    if not with_dbias:
        assert _same_bits(db, c.inp["dbias0"]), "dbias changed by a call that was not given it"
    db = db.double() - c.inp["dbias0"].double()
    return {"dqk": dy[:, :c.NQ], "dv": dy[:, c.NQ:], "dbias_k": db[:c.NQ], "dbias_v": db[c.NQ:]}


# ---------------------------------------------------------------------- checks

def compare(c, what, pairs, late):
    """pairs: (name, got, key into the references[, slack added to the bar]).  Prints the ratio line of
    each, asserts its bar against the 1e-4 cap and collects the misses in ``late``."""
    for name, got, key, *slack in pairs:
        want, w32 = c.ref[F64][key], c.ref[F32][key]
        got = got.double().reshape(want.shape)
        scale = want.abs().max().item()
        e32 = (w32.double() - want).abs().max().item()
        bar = MULT.get(name, 32) * e32 + 32 * 2.0 ** -24 * scale
        err = (got - want).abs().max().item()
        print("mha-attn-ratio %s %s %-7s err %.3e e32 %.3e err/e32 %s bar %.3e max %.3e"
              % (c.tag, what, name, err, e32, "%.2f" % (err / e32) if e32 > 0 else "-", bar, scale))
        if scale == 0:
            if not (got == 0).all():
                late.append("%s must be exactly zero (err %.3e)" % (name, err))
            continue
        assert bar <= 1e-4 * scale, "%s: the bar %.3e exceeds 1e-4 of max %.3e" % (name, bar, scale)
        if not err <= bar + sum(slack):
            late.append("%s: err %.3e > bar %.3e (e32 %.3e, max %.3e)" % (name, err, bar, e32, scale))


def bwd_pairs(c, got):
    """dbias: the kernel adds one partial column sum per sequence onto the start, each addition rounding
    by at most 2^-24 of the running value, which never exceeds |start| + sum_s |column sum of sequence
    s|: n such roundings on top of the bar (exactly zero where the gradient is, as at L = 1: adding 0
    does not round)."""
    pairs = [("dqk", got["dqk"], "dqk"), ("dv", got["dv"], "dv")]
    for name, g, lo, hi in (("dbias_k", "dqk", 0, c.NQ), ("dbias_v", "dv", c.NQ, c.NQ + c.NV)):
        per_seq = c.ref[F64][g].reshape(c.n, c.L, -1).sum(1).abs().sum(0)
        run = (c.inp["dbias0"][lo:hi].double().abs() + per_seq).max().item()
        pairs.append((name, got[name], name, c.n * 2.0 ** -24 * run))
    return pairs


# ---------------------------------------------------------------------- nr_mha_attn_fwd / nr_mha_attn_bwd

@pytest.mark.parametrize("key", CASES, ids=[_id(c) for c in CASES])
def test_forward(key):
    c = case(*key)
    Y, qk, v = y_buffer(c, c.inp["qk"], c.inp["v"])
    out = run_fwd(c, Y, qk, v)
    late = []
    compare(c, "fwd", [("out", out, "out")], late)
    assert not late, "; ".join(late)


@pytest.mark.parametrize("key", CASES, ids=[_id(c) for c in CASES])
def test_backward(key):
    """dqk, dv and the accumulated dbias against the reference; without dbias the same dqk and dv bit for
    bit.  At L = 1 dqk (and with it dbias_k's gradient) is exactly zero."""
    c = case(*key)
    Y, qk, v = y_buffer(c, c.inp["qk"], c.inp["v"])
    got = run_bwd(c, Y, qk, v)
    late = []
    compare(c, "bwd", bwd_pairs(c, got), late)
    assert not late, "; ".join(late)
    plain = run_bwd(c, Y, qk, v, with_dbias=False)
    assert _same_bits(got["dqk"], plain["dqk"]) and _same_bits(got["dv"], plain["dv"])
    if c.L == 1:
        assert (got["dqk"] == 0).all() and (got["dbias_k"] == 0).all()


REPEAT = [(17, 12, 64, 32, torch.int64), (31, 3, 64, 64, torch.float32), (49, 12, 32, 32, torch.float64),
          (63, 1, 64, 32, torch.uint8)]


@pytest.mark.parametrize("key", REPEAT, ids=[_id(c) for c in REPEAT])
def test_two_calls_give_the_same_bits(key):
    """No atomics touch out, dqk or dv: two forward calls, and two backward calls, agree bit for bit."""
    c = case(*key)
    Y, qk, v = y_buffer(c, c.inp["qk"], c.inp["v"])
    assert _same_bits(run_fwd(c, Y, qk, v), run_fwd(c, Y, qk, v))
    a, b = run_bwd(c, Y, qk, v), run_bwd(c, Y, qk, v)
    assert _same_bits(a["dqk"], b["dqk"]) and _same_bits(a["dv"], b["dv"])


ROWS = [(17, 12, 64, 32, torch.int64), (31, 3, 16, 16, torch.float64), (49, 12, 32, 32, torch.bool),
        (63, 3, 64, 64, torch.float32)]


@pytest.mark.parametrize("key", ROWS, ids=[_id(c) for c in ROWS])
def test_forward_rows_table(key):
    """rows, in load_rows and in load_rows_split: qk / v are a table of R < n*L rows read through an index
    with repeats, below it three all-NaN rows that no index names.  Equal to the reference that gathers
    first, and bit-identical to the same call on the gathered, dense Y."""
    L = key[0]
    R_ = attn_mask(L).shape[0] * L // 3
    c = make_case(*key, rows=R_, with_bwd=False)
    Y, qk, v = y_buffer(c, c.inp["qk"], c.inp["v"], spare_rows=3)
    assert Y.shape[0] == R_ + 3 and int(c.rows.max()) < R_
    out = run_fwd(c, Y, qk, v, rows=c.rows.cuda())
    late = []
    compare(c, "fwd-rows", [("out", out, "out")], late)
    assert not late, "; ".join(late)
    Yd, qkd, vd = y_buffer(c, c.inp["qk"][c.rows], c.inp["v"][c.rows])
    assert _same_bits(out, run_fwd(c, Yd, qkd, vd))


BIG = [(31, 12, 64, 32, torch.int64), (49, 12, 32, 32, torch.float32)]


@pytest.mark.parametrize("key", BIG, ids=[_id(c) for c in BIG])
def test_forward_large_scores(key):
    """Scores past 89, where exp overflows float32 unless the row maximum is taken off first (in the split
    kernel: the wave's maximum, then the merged one).  Forward only: P is one-hot there, dqk is pure
    cancellation and the reference's own float32 error equals its magnitude."""
    base = case(*key)
    c = make_case(*key, qk_scale=(95.0 / base.ref[F64]["scores_max"].item()) ** 0.5, with_bwd=False)
    assert c.ref[F64]["scores_max"].item() > 89
    Y, qk, v = y_buffer(c, c.inp["qk"], c.inp["v"])
    out = run_fwd(c, Y, qk, v)
    late = []
    compare(c, "fwd-big", [("out", out, "out")], late)
    assert not late, "; ".join(late)


def test_wrapper_and_entry_refusals_launch_nothing():
    """kernels.mha_attn_fwd / mha_attn_bwd refuse host tensors, wrong row counts, a short dbias and a row
    table that is not int64; the entries a length and a (dk, dv) they have no kernel for.  No output is
    touched."""
    from newsrec_amd import _lib as Lb, kernels as K
    n, L, heads, dk, dv = 2, 5, 2, 64, 32
    T, NQ, NV = n * L, heads * dk, heads * dv
    qk, v, dout = torch.zeros(T, NQ, device="cuda"), torch.zeros(T, NV, device="cuda"), torch.zeros(T, NV, device="cuda")
    mask = torch.ones(n, L, dtype=torch.int64, device="cuda")
    outs = {"out": _nan(T, NV), "dqk": _nan(T, NQ), "dv": _nan(T, NV), "dbias": _nan(NQ + NV)}

    def fwd(qk=qk, v=v, mask=mask, out=outs["out"], rows=None, L=L, dk=dk):
        K.mha_attn_fwd(qk, v, mask, n, L, heads, dk, dv, out, rows=rows)

    def bwd(qk=qk, dout=dout, dqk=outs["dqk"], dvv=outs["dv"], dbias=None, mask=mask, dk=dk):
        K.mha_attn_bwd(qk, v, mask, n, L, heads, dk, dv, dout, dqk, dvv, dbias=dbias)

    idx = torch.zeros(T, dtype=torch.int64, device="cuda")
    calls = [lambda: fwd(qk=qk.cpu()), lambda: fwd(out=outs["out"].cpu()), lambda: bwd(dout=dout.cpu()),
             lambda: fwd(qk=qk[:T - 1]), lambda: fwd(out=outs["out"][:T - 1]), lambda: bwd(dout=dout[:T - 1]),
             lambda: bwd(dqk=outs["dqk"][1:]), lambda: bwd(dvv=outs["dv"][:T - 1]), lambda: bwd(qk=qk[:T - 1]),
             lambda: bwd(dbias=outs["dbias"][:NQ + NV - 1]), lambda: bwd(dbias=outs["dbias"].double()),
             lambda: fwd(rows=idx.int()), lambda: fwd(rows=idx.cpu()), lambda: fwd(rows=idx[:T - 1]),
             lambda: fwd(mask=mask[:, :L - 1]), lambda: bwd(mask=mask.int()), lambda: fwd(qk=qk[:, :NQ - 4]),
             lambda: fwd(qk=qk.double())]
    for i, f in enumerate(calls):
        with pytest.raises(Lb.HipError):
            f()
        torch.cuda.synchronize()
        assert all(_all_nan_bits(t) for t in outs.values()), "call %d wrote an output" % i
    for f, name, code in ((lambda: fwd(dk=48, qk=torch.zeros(T, 96, device="cuda")), "nr_mha_attn_fwd", 8),
                          (lambda: bwd(dk=48, qk=torch.zeros(T, 96, device="cuda"), dqk=_nan(T, 96)), "nr_mha_attn_bwd", 8)):
        with pytest.raises(Lb.HipError, match=r"^%s: invalid argument %d$" % (name, code)):
            f()
        torch.cuda.synchronize()
        assert all(_all_nan_bits(t) for t in outs.values())


# ---------------------------------------------------------------------- nr_mha_user_pool_fwd

POOL_GEOMS = {"h12k32v32": (12, 32, 32), "h12k64v32": (12, 64, 32), "h12k64v64": (12, 64, 64)}
POOL_LENGTHS = {"h12k32v32": (1, 17, 32, 33, 49, 64), "h12k64v32": (1, 17, 32, 33, 49, 64),
                "h12k64v64": (1, 33, 53)}        # H = 768: L = 53 is the largest LDS allocation the entry accepts
POOL_IDENTITY = {"h12k32v32": 49, "h12k64v32": 17, "h12k64v64": 33}
POOL_CASES = [(g, L, False) for g in POOL_GEOMS for L in POOL_LENGTHS[g]] + [(g, L, True) for g, L in POOL_IDENTITY.items()]
POOL_BAR = {"f32": 2e-5, "bf16x6": 2e-5, "bf16": 3e-2}


@functools.lru_cache(maxsize=None)
def pool_case(geom, L, identity):
    """y [R, heads*(dk+dv)] = [0.5 N(0,1) keys | N(0,1) values], a table of R = n*L/2 + 1 rows read through
    a seeded index with repeats (identity: R = n*L, yrows = 0 .. n*L - 1); the history mask cycles over the
    dtypes with L; the float64 and float32 references."""
    heads, dk, dv = POOL_GEOMS[geom]
    mdt = MASK_DTYPES[(L + dk // 32) % len(MASK_DTYPES)]
    mask = attn_mask(L, mdt)
    n = mask.shape[0]
    R_ = n * L if identity else n * L // 2 + 1
    inp = attn_inputs(n, L, heads, dk, dv, 77 * L + dk + dv, rows=R_)
    y = torch.cat([inp["qk"], inp["v"]], 1)
    yrows = torch.arange(n * L) if identity else \
        torch.randint(0, R_, (n * L,), generator=torch.Generator().manual_seed(L + 5))
    ref = {dt: mha_user_pool_reference(y, yrows, mask, heads, dk, dv, inp["q"], dtype=dt) for dt in (F64, F32)}
    return types.SimpleNamespace(heads=heads, dk=dk, dv=dv, L=L, n=n, H=heads * dv, NY=heads * (dk + dv), R=R_, y=y,
                                 yrows=yrows, mask=mask, q=inp["q"], ref=ref,
                                 tag="%s-L%d-%s%s" % (geom, L, str(mdt).split(".")[1], "-identity" if identity else ""))


def _prec(name):
    from newsrec_amd import _lib as L
    return {"f32": L.GEMM_F32, "bf16x6": L.GEMM_BF16X6, "bf16": L.GEMM_BF16}[name]


@pytest.mark.parametrize("prec", list(POOL_BAR))
@pytest.mark.parametrize("key", POOL_CASES, ids=["%s-L%d%s" % (g, L, "-identity" if i else "") for g, L, i in POOL_CASES])
def test_user_pool(key, prec):
    """y with NaN padding columns and three all-NaN rows that no yrows entry names, out a view of a NaN
    buffer with spare rows and columns: the padding stays NaN, every user vector is written, the empty
    history gives exact zeros."""
    from newsrec_amd import kernels as K
    c = pool_case(*key)
    assert K.mha_user_pool_supported(c.L, c.heads, c.dk, c.dv)
    ybuf = _nan(c.R + 3, c.NY + PAD)
    ybuf[:c.R, :c.NY] = c.y.cuda()
    before = ybuf.clone()
    obuf, out = _framed(c.n, c.H)
    K.mha_user_pool_fwd(ybuf[:, :c.NY], c.yrows.cuda(), c.mask.cuda(), c.n, c.L, c.heads, c.dk, c.dv, c.q.cuda(), out,
                        prec=_prec(prec))
    torch.cuda.synchronize()
    assert _same_bits(before, ybuf), "the kernel changed y"
    assert _frame_untouched(obuf, c.n, c.H), "out: written outside its %d x %d view" % (c.n, c.H)
    out = out.cpu()
    assert torch.isfinite(out).all(), "out: unwritten or non-finite values"
    assert (out[0] == 0).all(), "the empty history's user vector is not exactly zero"
    want = c.ref[F64]
    scale = want.abs().max().item()
    e32 = (c.ref[F32].double() - want).abs().max().item()
    err = (out.double() - want).abs().max().item()
    print("mha-attn-ratio user-pool %s %-6s err %.3e e32 %.3e err/e32 %s err/max %.2e max %.3e"
          % (c.tag, prec, err, e32, "%.2f" % (err / e32) if e32 > 0 else "-", err / scale, scale))
    assert err <= POOL_BAR[prec] * scale, "err %.3e > %g of max %.3e" % (err, POOL_BAR[prec], scale)
