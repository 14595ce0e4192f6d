"""The seven store-side epilogues of nr_gemm_f32* on every kernel family that runs them, against the
float64 closed forms of tests/gemm_epi_util.py (held to autograd in tests/test_gemm_epi_ref_cpu.py,
which also pins that every case routes to the kernel its row names).

Families (gemm_epi_util.KERNELS): the generic kernel (its own `if` chain; K % 32 != 0, and ld % 4 != 0
with scalar loads), and through the shared epilogue_t the exact-f32 64 x 64 and 128 x 128 kernels, the
128 x 128 bf16-plane kernel with 3 planes and 1, and the 256 x 256 one with 3 planes and 1 under a
device-resident M (1600 of a bound of 1800: tile row 6 half live, tile row 7 empty).  Each at both B
layouts and at N % 4 == 0 (the float4 path of epilogue_t) and N % 4 != 0 (its scalar path).

Storage of every case: C is the [M, N] window at row 4, column 4 of a NaN-filled block of M + 8 rows
with ldc = round4(N) + 8; aux sits likewise in a block of its own with ld = round4(N) + 12; bias is a
slice of a NaN-padded vector; the unread padding of A and B is NaN as well.  A bias-free epilogue gets
an all-NaN bias.  After the call everything outside the live window must be bit-identical to before
(rows [*m_dev, M) of C and of aux included; the whole aux block where the epilogue only reads it), and
the window finite and within the bar (gemm_epi_util, derived there).

Further: each of the five float4-path downgrades of make_args alone (ldc % 4, C / bias / aux off by
one float, aux ld % 4); a device-resident K; the static form's K == 0 (the generic kernel's epilogue
on zero accumulators); and nr_gemm_f32_pair with an NR_EPI_ACCUM + bias input gradient, bitwise equal
to the two single calls.  Every test prints its worst error / bar ratio ("EPI_RATIO <kernel> ...")."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_epi_util as U
from gemm_guard_util import NAN, Block, _bits
from newsrec_amd import _lib as L
from newsrec_amd import kernels as K

_DEV = {}           # operands on the GPU, per (shape, ...): uploaded once


@pytest.fixture(scope="module", autouse=True)
def _own_memory_pool():
    """Every GPU allocation of this module comes from a memory pool of its own, released at the end:
    the few hundred blocks of many sizes it allocates and frees would otherwise stay cached in the
    default pool and change which block a later test's allocation is served from
    (tests/test_row_grad_gpu.py relies on the allocator handing a just-freed block out again)."""
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
        _DEV.clear()
    del pool


def _round4(n):
    return (n + 3) // 4 * 4


def _a_operand(shape, k_live=None):
    key = ("a", shape.key, k_live)
    if key not in _DEV:
        t = torch.full((shape.M, shape.lda), NAN)
        t[:, :shape.K if k_live is None else k_live] = U.inputs(shape)["a"][:, :k_live]
        _DEV[key] = t.cuda()
    return K.operand(_DEV[key][:, :shape.K], L.KCONTIG)


def _b_operand(shape, layout, n, k_live=None):
    key = ("b", shape.key, layout, n, k_live)
    if key not in _DEV:
        b = U.inputs(shape)["b"][:, :n]
        kl = shape.K if k_live is None else k_live
        if layout == "kc":
            t = torch.full((n, shape.ldb_kc), NAN)
            t[:, :kl] = b[:kl].t()
        else:
            t = torch.full((shape.K, shape.ldb_mn), NAN)
            t[:kl, :n] = b[:kl]
        _DEV[key] = t.cuda()
    t = _DEV[key]
    return K.operand(t[:, :shape.K], L.KCONTIG) if layout == "kc" else K.operand(t[:, :n], L.MNCONTIG)


def _run(kernel, epi, layout, n, ldc_odd=False, c_off=0, bias_off=0, aux_ld_odd=False, aux_off=0, k_dev=None,
         prec=None):
    """One call on guarded storage, checked; returns (C block, aux block or None, worst error / bar)."""
    s = kernel.shape
    d = U.inputs(s)
    live = s.m_dev if kernel.form == "mdev" else s.M
    c = Block(s.M, n, _round4(n) + 8 + (1 if ldc_odd else 0), 4 + c_off, d["c0"][:, :n] if epi in U.READS_C else None)
    aux = None
    if epi in U.USES_AUX:
        src = None if epi in U.WRITES_AUX else (d["aux_gate"] if epi == L.EPI_ACCUM_GATE else d["aux_grad"])[:, :n]
        aux = Block(s.M, n, _round4(n) + 12 + (1 if aux_ld_odd else 0), 4 + aux_off, src)
    bvec = torch.full((n + 12,), NAN)
    if epi in U.READS_BIAS:
        bvec[4 + bias_off:4 + bias_off + n] = d["bias"][:n]
    bias = bvec.cuda()[4 + bias_off:4 + bias_off + n]
    kw = dict(bias=bias, epilogue=epi, c_rows=K.operand(aux.win, L.KCONTIG) if aux is not None else None,
              prec=U.PREC[kernel.prec] if prec is None else prec)
    args = (s.M, n, s.K, _a_operand(s, k_dev), _b_operand(s, layout, n, k_dev), c.win)
    if kernel.form == "static":
        assert k_dev is None
        K.gemm(*args, **kw)
    else:
        K.gemm_dyn(*args, m_dev=torch.tensor([s.m_dev], dtype=torch.int32, device="cuda") if kernel.form == "mdev" else None,
                   k_dev=torch.tensor([k_dev], dtype=torch.int32, device="cuda") if k_dev is not None else None, **kw)
    torch.cuda.synchronize()
    name = "%s %s %s N=%d" % (kernel.id, U.EPI_NAME[epi], layout, n)
    want_c, want_x, bar_c, bar_x = U.wanted(kernel, epi, n, k=k_dev)
    got = c.check(live, name + " C")
    assert torch.isfinite(got).all(), name
    err = (got.double() - want_c).abs().max().item()
    ratio = err / bar_c
    if aux is not None:
        got_x = aux.check(live if epi in U.WRITES_AUX else 0, name + " aux")
        if epi in U.WRITES_AUX:
            assert torch.isfinite(got_x).all(), name
            err_x = (got_x.double() - want_x).abs().max().item()
            assert err_x <= bar_x, "%s aux: err %.3e > bar %.3e" % (name, err_x, bar_x)
            ratio = max(ratio, err_x / bar_x)
    print("EPI_RATIO %s %s err=%.3e bar=%.3e ratio=%.4f" % (kernel.id, name, err, bar_c, ratio))
    assert err <= bar_c, "%s: err %.3e > bar %.3e" % (name, err, bar_c)
    if epi == L.EPI_ACCUM_GATE:   # a closed gate (negative, +0.0, -0.0) stores exactly +0.0
        closed = ~(d["aux_gate"][:live, :n] > 0)
        assert closed.sum() > live * n // 4 and (_bits(got)[closed] == 0).all(), name
    return c, aux, ratio


_CASES, _IDS = U.matrix_cases()


@pytest.mark.parametrize("kernel,epi,layout,n", _CASES, ids=_IDS)
def test_epilogue_matrix(kernel, epi, layout, n):
    _run(kernel, epi, layout, n)


# the rows that are one kernel under several `prec`: the results must not differ in a bit
_SAME = [(["f32_64-f32", "f32_64-bf16x6"], "mid"), (["generic-f32", "generic-bf16x6", "generic-bf16"], "small")]


@pytest.mark.parametrize("epi", [e for _, e in U.EPILOGUES], ids=[n for n, _ in U.EPILOGUES])
@pytest.mark.parametrize("ids", [s[0] for s in _SAME], ids=[s[1] for s in _SAME])
def test_one_kernel_under_each_prec_is_bitwise_equal(ids, epi):
    kernels = [U.KERNEL[i] for i in ids]
    for layout in U.layouts(kernels[0].shape):
        for n in U.widths(kernels[0].shape):
            outs = [_run(k, epi, layout, n) for k in kernels]
            for c, aux, _ in outs[1:]:
                assert torch.equal(_bits(c.dev), _bits(outs[0][0].dev)), (ids, layout, n)
                if aux is not None:
                    assert torch.equal(_bits(aux.dev), _bits(outs[0][1].dev)), (ids, layout, n)


# ---- the float4 path's downgrades (make_args, g.vec), each alone

_DOWN = {"ldc_odd": dict(ldc_odd=True), "c_off": dict(c_off=1), "bias_off": dict(bias_off=1),
         "aux_ld_odd": dict(aux_ld_odd=True), "aux_off": dict(aux_off=1)}
_DOWN_CASES = [(k, e, dn) for k in ("f32_64-bf16x6", "split_128_3-dyn")
               for e in (L.EPI_ACCUM_GATE, L.EPI_STORE_GELU, L.EPI_ACCUM)
               for dn in _DOWN if e in U.USES_AUX or not dn.startswith("aux")]


@pytest.mark.parametrize("kid,epi,down", _DOWN_CASES, ids=["%s-%s-%s" % (k, U.EPI_NAME[e], dn) for k, e, dn in _DOWN_CASES])
def test_float4_downgrades(kid, epi, down):
    """N = 136 with one misalignment: the scalar path, same margins, same values as the aligned call
    (both within the bar of the float64 reference, and of each other)."""
    kernel = U.KERNEL[kid]
    aligned, aligned_aux, _ = _run(kernel, epi, "mn", 136)
    got, got_aux, _ = _run(kernel, epi, "mn", 136, **_DOWN[down])
    _, _, bar_c, bar_x = U.wanted(kernel, epi, 136)
    assert (got.win.double() - aligned.win.double()).abs().max().item() <= bar_c
    if epi in U.WRITES_AUX:
        assert (got_aux.win.double() - aligned_aux.win.double()).abs().max().item() <= bar_x


# ---- device-resident K

@pytest.mark.parametrize("n", [136, 134])
@pytest.mark.parametrize("layout", ["kc", "mn"])
@pytest.mark.parametrize("kid", ["f32_128-dyn", "split_128_3-dyn", "split_128_1-dyn"])
def test_accum_device_k(kid, layout, n):
    """k_dev = 64 under a bound of 96: C0 + bias + the sum over the first 64 k only (the operands hold
    NaN at k >= 64)."""
    _run(U.KERNEL[kid], L.EPI_ACCUM, layout, n, k_dev=64)


# ---- K == 0, static form: the generic kernel's epilogue on zero accumulators

@pytest.mark.parametrize("prec", ["f32", "bf16x6", "bf16"])
@pytest.mark.parametrize("epi", [L.EPI_STORE, L.EPI_ACCUM, L.EPI_ACCUM_GATE, L.EPI_STORE_GELU, L.EPI_GELU_GRAD],
                         ids=["store", "accum", "accum_gate", "store_gelu", "gelu_grad"])
def test_k_zero_static(epi, prec):
    """STORE: the bias; ACCUM: C0 + bias; ACCUM_GATE: C0 where aux > 0, else 0; STORE_GELU: aux = bias,
    C = gelu(bias); GELU_GRAD: 0 -- exactly, but for gelu(bias) (its bar with a zero GEMM term)."""
    s, n = U.SMALL, 50
    d = U.inputs(s)
    c = Block(s.M, n, 60, 4, d["c0"][:, :n] if epi in U.READS_C else None)
    aux = None
    if epi in U.USES_AUX:
        src = None if epi in U.WRITES_AUX else (d["aux_gate"] if epi == L.EPI_ACCUM_GATE else d["aux_grad"])[:, :n]
        aux = Block(s.M, n, 64, 4, src)
    bvec = torch.full((n + 12,), NAN)
    if epi in U.READS_BIAS:
        bvec[4:4 + n] = d["bias"][:n]
    ops = torch.full((s.M, 72), NAN, device="cuda")   # never read: K == 0
    K.gemm(s.M, n, 0, K.operand(ops, L.KCONTIG), K.operand(ops[:n], L.KCONTIG), c.win, bias=bvec.cuda()[4:4 + n],
           epilogue=epi, c_rows=K.operand(aux.win, L.KCONTIG) if aux is not None else None, prec=U.PREC[prec])
    torch.cuda.synchronize()
    got = c.check(s.M, "K=0 C")
    bias, c0 = d["bias"][:n], d["c0"][:, :n]
    if aux is not None:
        got_x = aux.check(s.M if epi in U.WRITES_AUX else 0, "K=0 aux")
    if epi == L.EPI_STORE:
        assert torch.equal(got, bias.expand(s.M, n))
    elif epi == L.EPI_ACCUM:
        assert torch.equal(got, c0 + bias)                      # one fp32 add each, as the kernel's
    elif epi == L.EPI_ACCUM_GATE:
        assert torch.equal(got, torch.where(d["aux_gate"][:, :n] > 0, c0, torch.zeros_like(c0)))
    elif epi == L.EPI_GELU_GRAD:
        assert (got == 0).all()
    else:
        assert torch.equal(got_x, bias.expand(s.M, n))
        want = U.gelu(bias.double()).expand(s.M, n)
        bound = U.bar(epi, 0.0, 0.0, 0, 0, want)
        err = (got.double() - want).abs().max().item()
        print("EPI_RATIO k_zero store_gelu err=%.3e bar=%.3e ratio=%.4f" % (err, bound, err / bound))
        assert err <= bound


# ---- nr_gemm_f32_pair: an NR_EPI_ACCUM + bias input gradient beside a weight gradient

def test_pair_accum_with_bias_is_bitwise_the_single_calls():
    """dx [96, 64] += dY [96, 96] W [96, 64] + bias beside dW += dYᵀ x (one K split into zeros): the
    header promises the same arithmetic in the same order, so both outputs equal the single calls' bit
    for bit, and dx the float64 reference within the f32 bar."""
    g = torch.Generator().manual_seed(77)
    rows, D, NY = 96, 64, 96
    dY, W = torch.randn(rows, NY, generator=g), torch.randn(NY, D, generator=g) / NY ** 0.5
    x, bias, c0 = torch.randn(rows, D, generator=g), torch.randn(D, generator=g), torch.randn(rows, D, generator=g)
    dYd, Wd, xd = dY.cuda(), W.cuda(), x.cuda()
    bvec = torch.full((D + 8,), NAN)
    bvec[4:4 + D] = bias
    bd = bvec.cuda()[4:4 + D]

    def outs():
        return Block(rows, D, D + 8, 4, c0), Block(NY, D, D + 12, 4, torch.zeros(NY, D))

    def descs(dx, dw):
        return (K.gemm_desc(rows, D, NY, K.operand(dYd, L.KCONTIG), K.operand(Wd, L.MNCONTIG), dx.win, bias=bd,
                            epilogue=L.EPI_ACCUM, prec=L.GEMM_BF16X6),
                K.gemm_desc(NY, D, rows, K.operand(dYd, L.MNCONTIG), K.operand(xd, L.MNCONTIG), dw.win,
                            epilogue=L.EPI_ATOMIC, prec=L.GEMM_BF16X6))

    dx1, dw1 = outs()
    K.gemm(rows, D, NY, K.operand(dYd, L.KCONTIG), K.operand(Wd, L.MNCONTIG), dx1.win, bias=bd, epilogue=L.EPI_ACCUM,
           prec=L.GEMM_BF16X6)
    K.gemm(NY, D, rows, K.operand(dYd, L.MNCONTIG), K.operand(xd, L.MNCONTIG), dw1.win, epilogue=L.EPI_ATOMIC,
           prec=L.GEMM_BF16X6)
    for order in (0, 1):   # either order of the two descriptions
        dx2, dw2 = outs()
        ds = descs(dx2, dw2)
        K.gemm_pair(ds[order], ds[1 - order], dx2.win)
        torch.cuda.synchronize()
        assert torch.equal(_bits(dx2.dev), _bits(dx1.dev)) and torch.equal(_bits(dw2.dev), _bits(dw1.dev))
    got = dx1.check(rows, "pair dx")
    dw1.check(NY, "pair dW")
    want = U.reference(L.EPI_ACCUM, dY.double() @ W.double(), bias, c0=c0)[0]
    bound = U.bar(L.EPI_ACCUM, dY.abs().max().item(), W.abs().max().item(), NY, 0, want)
    err = (got.double() - want).abs().max().item()
    print("EPI_RATIO pair accum err=%.3e bar=%.3e ratio=%.4f" % (err, bound, err / bound))
    assert err <= bound
