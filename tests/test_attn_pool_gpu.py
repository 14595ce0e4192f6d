"""The learned-query pooling kernels (csrc/attn_pool.hip) called directly, K.attn_pool_fwd /
K.attn_pool_bwd, against the float64 reference of tests/pool_util.py: the LayerNorm + dropout branch
(the unfused MHA news-encoder tail the model takes whenever kernels.mha_pool_supported is false), the
tied and separate-key forms, key_tanh, dz, zout, widths that are no multiple of 4 or 64, and the
largest LDS image (over 64 KB: the hipFuncSetAttribute branch of both entries).

Every matrix has a leading dimension wider than its row with NaN in the padding, dx / dk and every
forward output start as NaN: the padding must come back NaN bit for bit, every row written, out and
probs of the fully masked sequence and dk of masked tokens exactly zero.

The bar is that of tests/test_mha_pool_gpu.py: with e32 = max|ref32 - ref64| of the same reference in
float32 on the CPU, err <= 32 e32 + 32 * 2^-24 * max|ref64| per tensor, a bar that may itself never
exceed 1e-4 * max|ref64|.  Every case prints its err / e32 ratios ("attn-pool-ratio" lines, pytest -s).

Measured on an MI355X at this commit (three runs; the atomic sums vary a little between runs), the
largest err / e32 of any case per output -- no output needed a multiplier above 32, the largest err /
bar of any line was 0.06:
  out 3.7  probs 4.2  zout 1.0  mean 1.2  rstd 1.0  dx 4.4  dk 2.1  dq 2.0  dgamma 3.3  dbeta 2.5

One-line errors tried on a scratch build, each caught: 1 - K instead of 1 - K^2 behind key_tanh (the 6
key_tanh cases of test_kernels_vs_reference, test_mask_dtypes, test_explicit_scale); the - sg term of
the LayerNorm backward dropped, and eps left out of rstd in the forward (each: all 11 LayerNorm cases
of test_kernels_vs_reference, and the mask, rng, scale and accumulate tests).
"""
import functools
import math
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import restatement as R
from pool_util import attn_pool_inputs, attn_pool_reference, pool_mask

NAN = float("nan")
NAN_BITS = torch.tensor(NAN).view(torch.int32).item()
SEED, OFFSET = 21, 5
F64, F32 = torch.float64, torch.float32
MULT = {}      # output -> a multiplier of e32 above 32 (see the module docstring); none needed

# LayerNorm, separate key, key_tanh, p_drop, zout and dz
VARIANTS = {
    "ln_drop": dict(ln=True, key=False, key_tanh=False, p=0.2, z=True),
    "tied": dict(ln=False, key=False, key_tanh=False, p=0.0, z=False),
    "key_tanh": dict(ln=False, key=True, key_tanh=True, p=0.0, z=False),
    "key_plain": dict(ln=False, key=True, key_tanh=False, p=0.2, z=False),
    "ln_key": dict(ln=True, key=True, key_tanh=False, p=0.0, z=True),
}
# (384,30) the unfused MHA tail; (150,50) the CNN / user pooling width, no multiple of 4 or 64; (64,64)
# full L, one feature per lane; (400,33) L just past one 32-row pass of the 4 waves; (768,50) the
# largest LDS image (156.5 KB in the backward); (3,5), (3,1) fewer features than lanes, one row
CASES = [(D, L, v) for D, L in ((384, 30), (150, 50), (64, 64), (400, 33)) for v in VARIANTS]
CASES += [(D, L, v) for D, L in ((768, 50), (3, 5), (3, 1)) for v in ("ln_drop", "key_tanh")]


@functools.lru_cache(maxsize=None)
def case(D, L, variant, scale=None, seed=SEED, offset=OFFSET):
    v = VARIANTS[variant]
    mask = pool_mask(L)
    n = mask.shape[0]
    inp = attn_pool_inputs(n, L, D, 1000 * D + 10 * L + list(VARIANTS).index(variant))
    keep = R.dropout_keep(seed, offset, n * L, D, v["p"]) if v["p"] > 0 else None
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    ref = {dt: attn_pool_reference(inp["x"], inp["key"] if v["key"] else None, inp["q"], mask,
                                   inp["gamma"] if v["ln"] else None, inp["beta"] if v["ln"] else None, keep, v["p"],
                                   scale, v["key_tanh"], dout=inp["dout"], dz=inp["dz"] if v["z"] else None, dtype=dt)
           for dt in (F64, F32)}
    return types.SimpleNamespace(D=D, L=L, n=n, T=n * L, v=v, mask=mask, inp=inp, keep=keep, ref=ref, scale=scale,
                                 tag="D%d-L%d-%s" % (D, L, variant))


@pytest.fixture(scope="module", autouse=True)
def _leave_no_blocks_behind():
    """The later modules of the suite see the caching allocator as they would without this one (a test
    of tests/test_row_grad_gpu.py depends on which block a freed gradient's successor gets): drop the
    cached blocks this module's buffers came from."""
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


def _padded(t, pad):
    buf = _nan(t.shape[0], t.shape[1] + pad)
    buf[:, :t.shape[1]] = t.cuda()
    return buf, buf[:, :t.shape[1]]


def _vec(n, fill=NAN, tail=3):
    buf = _nan(n + tail)
    buf[:n] = fill
    return buf, buf[:n]


def _all_nan_bits(t):
    return bool((t.contiguous().view(torch.int32) == NAN_BITS).all())


def run_kernels(c, mask=None, rng=None, seed=SEED, offset=OFFSET, scale="case", preload=0.0):
    """One nr_attn_pool_fwd and one nr_attn_pool_bwd on its saved stats / probs, into NaN-filled
    buffers with padded leading dimensions -> {name: the whole buffer on the CPU}."""
    from newsrec_amd import kernels as K
    v, D, T, n = c.v, c.D, c.T, c.n
    _, x = _padded(c.inp["x"], 3)
    key = _padded(c.inp["key"], 5)[1] if v["key"] else None
    q = c.inp["q"].cuda()
    gamma, beta = (c.inp["gamma"].cuda(), c.inp["beta"].cuda()) if v["ln"] else (None, None)
    m = (c.mask if mask is None else mask).cuda()
    out, zout = _nan(n, D + 3), _nan(T, D + 1) if v["z"] else None
    stats = _vec(2 * T)[0] if v["ln"] else None
    probs = _vec(T, tail=5)[0]
    scale = c.scale if scale == "case" else scale
    drop = dict(p_drop=v["p"], seed=seed, offset=offset, rng=rng)
    K.attn_pool_fwd(x, q, m, n, c.L, out[:, :D], probs, key=key, gamma=gamma, beta=beta, stats=stats, scale=scale,
                    zout=zout[:, :D] if zout is not None else None, **drop)
    _, dout = _padded(c.inp["dout"], 3)
    dz = _padded(c.inp["dz"], 3)[1] if v["z"] else None
    dx = _nan(T, D + 7)
    dk = _nan(T, D + 1) if v["key"] else None
    dq = _vec(D, preload)
    dgamma, dbeta = (_vec(D, preload), _vec(D, preload)) if v["ln"] else ((None, None), (None, None))
    K.attn_pool_bwd(x, q, m, n, c.L, probs, dout, dx[:, :D], dq[1], key=key, dk=dk[:, :D] if dk is not None else None,
                    key_tanh=v["key_tanh"], gamma=gamma, beta=beta, stats=stats, dgamma=dgamma[1], dbeta=dbeta[1],
                    scale=scale, dz=dz, **drop)
    torch.cuda.synchronize()
    res = dict(out=out, zout=zout, stats=stats, probs=probs, dx=dx, dk=dk, dq=dq[0], dgamma=dgamma[0], dbeta=dbeta[0])
    return {k: t.cpu() for k, t in res.items() if t is not None}


def check(c, o, what, preload=0.0):
    D, T, L = c.D, c.T, c.L
    live = (c.mask != 0).reshape(-1)
    for name in ("out", "zout", "dx", "dk"):
        if name in o:
            assert _all_nan_bits(o[name][:, D:]), "%s: written past column %d" % (name, D)
            assert torch.isfinite(o[name][:, :D]).all(), "%s: rows not written, or non-finite values" % name
    for name, w in (("stats", 2 * T), ("probs", T), ("dq", D), ("dgamma", D), ("dbeta", D)):
        if name in o:
            assert _all_nan_bits(o[name][w:]) and torch.isfinite(o[name][:w]).all(), name
    assert (o["out"][0, :D] == 0).all(), "out of the fully masked sequence is not zero"
    assert (o["probs"][:T][~live] == 0).all(), "probs of masked tokens are not zero"
    if c.keep is not None and "zout" in o:
        assert (o["zout"][:, :D][~c.keep] == 0).all(), "zout is not zero where the dropout drops"
    if "dk" in o:
        assert (o["dk"][:, :D][~live] == 0).all(), "dk rows of masked tokens are not exactly zero"
    if not c.v["z"]:
        assert (o["dx"][:, :D][~live] == 0).all(), "dx rows of masked tokens are not exactly zero"
    pairs = [("out", o["out"][:, :D], "out"), ("probs", o["probs"][:T], "probs"), ("dx", o["dx"][:, :D], "dx"),
             ("dq", o["dq"][:D].double() - preload, "dq")]
    if "zout" in o:
        pairs.append(("zout", o["zout"][:, :D], "Z"))
    if "dk" in o:
        pairs.append(("dk", o["dk"][:, :D], "dk"))
    if "stats" in o:
        st = o["stats"][:2 * T].reshape(T, 2)
        r64, r32 = c.ref[F64]["stats"], c.ref[F32]["stats"]
        pairs += [("mean", st[:, 0], (r64[:, 0], r32[:, 0])), ("rstd", st[:, 1], (r64[:, 1], r32[:, 1])),
                  ("dgamma", o["dgamma"][:D].double() - preload, "dgamma"),
                  ("dbeta", o["dbeta"][:D].double() - preload, "dbeta")]
    late = []
    for name, got, key in pairs:
        want, w32 = (c.ref[F64][key], c.ref[F32][key]) if isinstance(key, str) else key
        got = got.double().reshape(want.shape)
        scale = want.abs().max().item()
        e32 = (w32.double() - want).abs().max().item()
        bar = MULT.get(name, 32) * e32 + 32 * 2.0 ** -24 * scale
        err = (got - want).abs().max().item()
        print("attn-pool-ratio %s %s %-6s err %.3e e32 %.3e err/e32 %s bar %.3e max %.3e"
              % (c.tag, what, name, err, e32, "%.2f" % (err / e32) if e32 > 0 else "-", bar, scale))
        assert bar <= 1e-4 * scale, "%s: the bar %.3e exceeds 1e-4 of max %.3e" % (name, bar, scale)
        # onto a preloaded value up to n additions land (one atomic per sequence), each rounding at the
        # magnitude of constant + gradient: that many half-ulps on top of the bar
        slack = c.n * 2.0 ** -24 * (want + preload).abs().max().item() if preload and name in ("dq", "dgamma", "dbeta") else 0.0
        if not err <= bar + slack:
            late.append("%s: err %.3e > bar %.3e (e32 %.3e, max %.3e)" % (name, err, bar, e32, scale))
    assert not late, "; ".join(late)


@pytest.mark.parametrize("D,L,variant", CASES, ids=["D%d-L%d-%s" % c for c in CASES])
def test_kernels_vs_reference(D, L, variant):
    """At L = 1 the softmax has one element, p in {0, 1}: ds = p (dp - p dp) scale is exactly 0 in the
    kernel's own arithmetic, so dq and dk are exactly zero (no rounding residue to allow for)."""
    c = case(D, L, variant)
    o = run_kernels(c)
    check(c, o, "vs-ref")
    if L == 1:
        assert (o["dq"][:D] == 0).all(), "dq at L = 1 is not exactly zero"
        if "dk" in o:
            assert (o["dk"][:, :D] == 0).all(), "dk at L = 1 is not exactly zero"


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64, torch.float64, torch.float32],
                         ids=["u8", "i64", "f64", "f32"])
@pytest.mark.parametrize("variant", ["ln_drop", "key_tanh"])
def test_mask_dtypes(variant, dtype):
    c = case(150, 50, variant)
    m = c.mask.to(dtype)
    if dtype.is_floating_point:
        m = m * torch.where(torch.arange(c.L) % 2 == 0, 2.5, -1.0).to(dtype)
    elif dtype == torch.int64:
        m = m << 40                   # nonzero only above bit 32
    check(c, run_kernels(c, mask=m), "mask-" + str(dtype).split(".")[1])


def test_device_rng_key():
    """rng: the dropout key comes from the device pair (seed, base) with the entry's offset added to the
    base -- the reference's keep mask is dropout_keep(seed, base + k)."""
    seed, base, k = 4321, 500, 33
    c = case(150, 50, "ln_drop", seed=seed, offset=base + k)
    rng = torch.tensor([seed, base], dtype=torch.int64, device="cuda")
    check(c, run_kernels(c, rng=rng, seed=1, offset=k), "rng")


@pytest.mark.parametrize("variant", ["ln_drop", "key_tanh"])
def test_explicit_scale(variant):
    c = case(150, 50, variant, scale=0.37)
    assert abs(c.scale - 1 / math.sqrt(150)) > 0.2
    check(c, run_kernels(c), "scale")
    d = case(150, 50, variant)        # scale=None is 1 / sqrt(D)
    check(d, run_kernels(d, scale=None), "scale-default")


@pytest.mark.parametrize("variant", ["ln_drop", "key_plain"])
def test_backward_accumulates(variant):
    """dq, dgamma, dbeta are accumulated: preloaded with a constant they come back as constant +
    gradient."""
    c = case(384, 30, variant)
    check(c, run_kernels(c, preload=0.75), "acc", preload=0.75)


# ---------------------------------------------------------------------- argument errors

def _expect(code, entry, outs, fn):
    from newsrec_amd import _lib as L
    with pytest.raises(L.HipError, match=r"^%s: invalid argument %d$" % (entry, code)):
        fn()
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert _all_nan_bits(v), "%s was written by a call that failed its argument check" % k


@pytest.mark.parametrize("what", ["L65", "gamma-without-stats", "key-without-dk", "lds"])
def test_argument_errors(what):
    """Refused by the entries before any launch: nothing is written."""
    from newsrec_amd import kernels as K
    n, L, D = (1, 64, 1024) if what == "lds" else (2, 65, 8) if what == "L65" else (2, 8, 8)
    T = n * L
    x, key, dout = torch.ones(T, D, device="cuda"), torch.ones(T, D, device="cuda"), torch.ones(n, D, device="cuda")
    q, gamma, beta = (torch.ones(D, device="cuda") for _ in range(3))
    mask = torch.ones(n, L, dtype=torch.int64, device="cuda")
    o = {k: _nan(*s) for k, s in (("out", (n, D)), ("probs", (T,)), ("stats", (T, 2)), ("zout", (T, D)), ("dx", (T, D)),
                                  ("dk", (T, D)), ("dq", (D,)), ("dgamma", (D,)), ("dbeta", (D,)))}
    saved = torch.zeros(T, device="cuda"), torch.zeros(T, 2, device="cuda")

    def fwd(**kw):
        K.attn_pool_fwd(x, q, mask, n, L, o["out"], o["probs"], zout=o["zout"], **kw)

    def bwd(**kw):
        K.attn_pool_bwd(x, q, mask, n, L, saved[0], dout, o["dx"], o["dq"], **kw)

    ln = dict(gamma=gamma, beta=beta, dgamma=o["dgamma"], dbeta=o["dbeta"])
    if what == "L65":
        _expect(0, "nr_attn_pool_fwd", o, lambda: fwd(gamma=gamma, beta=beta, stats=o["stats"]))
        _expect(0, "nr_attn_pool_bwd", o, lambda: bwd(stats=saved[1], key=key, dk=o["dk"], **ln))
    elif what == "gamma-without-stats":
        _expect(2, "nr_attn_pool_fwd", o, lambda: fwd(gamma=gamma, beta=beta))
        _expect(2, "nr_attn_pool_bwd", o, lambda: bwd(**ln))
    elif what == "key-without-dk":
        _expect(3, "nr_attn_pool_bwd", o, lambda: bwd(key=key))
    else:   # smem_bwd(64, 1024) = 264,704 B > 160 KB; the forward refuses what its backward could not run
        _expect(3, "nr_attn_pool_fwd", o, lambda: fwd())
        _expect(4, "nr_attn_pool_bwd", o, lambda: bwd())
