"""Shared by tests/test_gemm_epi_kernels_gpu.py and tests/test_gemm_epi_ref_cpu.py: the seven store-side
GEMM epilogues as closed forms in float64, the table of kernel families the GPU tests run them on (one
row per kernel x form x arithmetic, at the smallest shape that cuts a tile in M and in N on that
kernel), the inputs and float64 products of those shapes (computed once per process), the error bars,
and each case as an argument line of tests/gemm_route_dump.cpp, so that the kernel a case means is
pinned without a GPU.

Bars.  The GEMM term is the project's existing bound (tests/test_gemm_big_gpu.py::_tol): for f32 and
bf16x6 1e-5 max|a| max|b| sqrt(K) + 1e-6, for bf16 4e-7 max|a| max|b| K + 1e-6 against the product of
the bf16-rounded operands.  The two GELU epilogues get twice that (|gelu'| <= 1.13, plus the erff / expf
roundings; test_big_plain_epilogues grants the same factor), and every epilogue 2^-22 max|want| for
the fp32 roundings of its adds and function evaluations.  The generic kernel computes exact f32
products whatever `prec` says (include/newsrec_hip.h), so its rows take the f32 bar under every prec."""
import collections
import math

import torch

from newsrec_amd import _lib as L

F64 = torch.float64

# (name, code) of the store-side epilogues, and what each touches
EPILOGUES = [("store", L.EPI_STORE), ("relu", L.EPI_STORE_RELU), ("tanh", L.EPI_STORE_TANH),
             ("accum", L.EPI_ACCUM), ("accum_gate", L.EPI_ACCUM_GATE), ("store_gelu", L.EPI_STORE_GELU),
             ("gelu_grad", L.EPI_GELU_GRAD)]
EPI_NAME = {code: name for name, code in EPILOGUES}
READS_BIAS = {L.EPI_STORE, L.EPI_STORE_RELU, L.EPI_STORE_TANH, L.EPI_ACCUM, L.EPI_STORE_GELU}
USES_AUX = {L.EPI_ACCUM_GATE, L.EPI_STORE_GELU, L.EPI_GELU_GRAD}
WRITES_AUX = {L.EPI_STORE_GELU}
READS_C = {L.EPI_ACCUM, L.EPI_ACCUM_GATE}
GELU_EPIS = {L.EPI_STORE_GELU, L.EPI_GELU_GRAD}

PREC = {"f32": L.GEMM_F32, "bf16x6": L.GEMM_BF16X6, "bf16": L.GEMM_BF16}


# ---- closed forms

def normal_cdf(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def normal_pdf(x):
    return torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu(x):
    return x * normal_cdf(x)


def gelu_grad(x):
    return normal_cdf(x) + x * normal_pdf(x)


def reference(epi, pre, bias=None, c0=None, aux=None):
    """(C, aux written or None) of one epilogue in float64.  pre: the product A B [M, N]; bias [N]
    (None = zeros; ignored by the bias-free epilogues whatever it holds); c0: C on entry; aux: the
    auxiliary matrix on entry."""
    pre = pre.to(F64)
    b = 0.0 if bias is None or epi not in READS_BIAS else bias.to(F64)
    if epi == L.EPI_STORE:
        return pre + b, None
    if epi == L.EPI_STORE_RELU:
        return torch.clamp(pre + b, min=0.0), None
    if epi == L.EPI_STORE_TANH:
        return torch.tanh(pre + b), None
    if epi == L.EPI_ACCUM:
        return c0.to(F64) + pre + b, None
    if epi == L.EPI_ACCUM_GATE:
        return torch.where(aux.to(F64) > 0, c0.to(F64) + pre, torch.zeros_like(pre)), None
    if epi == L.EPI_STORE_GELU:
        x = pre + b
        return gelu(x), x
    if epi == L.EPI_GELU_GRAD:
        return pre * gelu_grad(aux.to(F64)), None
    raise ValueError("not a store-side epilogue: %r" % (epi,))


# ---- bars

def gemm_tol(amax, bmax, k, planes):
    """The GEMM term; planes: 1 = bf16 arithmetic, else fp32-class (exact f32 or bf16x6)."""
    if planes == 1:
        return 4e-7 * amax * bmax * k + 1e-6
    return 1e-5 * amax * bmax * math.sqrt(k) + 1e-6


def bar(epi, amax, bmax, k, planes, want, aux_out=False):
    """Bound on |got - want|; aux_out: for the pre-activation NR_EPI_STORE_GELU writes (no GELU in it)."""
    t = gemm_tol(amax, bmax, k, planes)
    if epi in GELU_EPIS and not aux_out:
        t *= 2.0
    return t + 2.0 ** -22 * want.abs().max().item()


# ---- the family table

# M, K: the extents (for the m_dev form M is the host bound and m_dev the device-resident count);
# n_vec / n_scalar: N % 4 == 0 (float4 epilogue where the kernel has one) / N % 4 != 0; lda: A [M][K];
# ldb_kc: B [N][K]; ldb_mn: B [K][N] (None: that layout is not part of the row)
Shape = collections.namedtuple("Shape", "key M K n_vec n_scalar lda ldb_kc ldb_mn m_dev")
# family / tile / planes: what gemm_route.h must say (planes: 3 bf16x6, 1 bf16, 0 exact f32)
Kernel = collections.namedtuple("Kernel", "id family tile planes form prec shape")

SMALL = Shape("small", 70, 70, 52, 50, 72, 72, 52, None)       # K % 32 != 0: generic kernel
ODD_LD = Shape("odd_ld", 70, 64, None, 50, 67, 67, None, None)  # ld % 4 != 0: generic kernel, scalar loads
MID = Shape("mid", 150, 96, 136, 134, 96, 96, 136, None)       # 3 x 3 tiles of 64, 2 x 2 of 128
BIG = Shape("big", 1800, 512, 1024, 1026, 512, 512, 1028, 1600)  # 8 tile rows of 256: row 6 holds 64 live rows, row 7 none

KERNELS = [
    Kernel("generic-f32", "generic", 64, 0, "static", "f32", SMALL),
    Kernel("generic-bf16x6", "generic", 64, 0, "static", "bf16x6", SMALL),
    Kernel("generic-bf16", "generic", 64, 0, "static", "bf16", SMALL),
    Kernel("generic_odd_ld-f32", "generic", 64, 0, "static", "f32", ODD_LD),
    Kernel("generic_odd_ld-bf16x6", "generic", 64, 0, "static", "bf16x6", ODD_LD),
    Kernel("f32_64-f32", "f32_64", 64, 0, "static", "f32", MID),
    Kernel("f32_64-bf16x6", "f32_64", 64, 0, "static", "bf16x6", MID),
    Kernel("f32_128-dyn", "f32_128", 128, 0, "dyn", "f32", MID),
    Kernel("split_128_3-dyn", "split_128", 128, 3, "dyn", "bf16x6", MID),
    Kernel("split_128_1-static", "split_128", 128, 1, "static", "bf16", MID),
    Kernel("split_128_1-dyn", "split_128", 128, 1, "dyn", "bf16", MID),
    Kernel("big_3-mdev", "big", 256, 3, "mdev", "bf16x6", BIG),
    Kernel("big_1-mdev", "big", 256, 1, "mdev", "bf16", BIG),
]
KERNEL = {k.id: k for k in KERNELS}


def layouts(shape):
    return ["kc"] + (["mn"] if shape.ldb_mn is not None else [])


def widths(shape):
    return [n for n in (shape.n_vec, shape.n_scalar) if n is not None]


def matrix_cases():
    """(kernel, epilogue code, B layout, N) of the full matrix, with ids."""
    cases, ids = [], []
    for k in KERNELS:
        for name, epi in EPILOGUES:
            for lay in layouts(k.shape):
                for n in widths(k.shape):
                    cases.append((k, epi, lay, n))
                    ids.append("%s-%s-%s-N%d" % (k.id, name, lay, n))
    return cases, ids


def route_argv(kernel, epi, layout, n, name="case"):
    """The case as arguments of tests/gemm_route_dump.cpp."""
    s = kernel.shape
    ldb = s.ldb_kc if layout == "kc" else s.ldb_mn
    return [name, str(s.M), str(n), str(s.K), "kc", str(s.lda), layout, str(ldb), str(epi), kernel.form, kernel.prec]


def route_fields(kernel, epi, layout):
    """What the dumped line must say of the case."""
    return {"family": kernel.family, "tile": "%dx%d" % (kernel.tile, kernel.tile), "planes": str(kernel.planes),
            "modes": "0,%d" % (0 if layout == "kc" else 3), "epi": str(epi), "splits": "1"}


def parse_route(line):
    head, rest = line.split(": ", 1)
    toks = rest.split(" ")
    out = {"name": head.split(" ")[0], "prec": head.split(" ")[1], "family": toks[0]}
    out.update(t.split("=", 1) for t in toks[1:])
    return out


# ---- inputs and products, once per process

_INPUTS, _PRODUCTS = {}, {}


def n_max(shape):
    return max(widths(shape))


def inputs(shape):
    """fp32 CPU inputs of a shape: a [M, K], b [K, n_max] (a narrower case takes its first N columns),
    bias [n_max], c0 and aux_grad [M, n_max] (C on entry; the pre-activations of NR_EPI_GELU_GRAD) and
    aux_gate [M, n_max]: every 7th element +0.0, every 7th -0.0 (gate closed), the rest of either sign."""
    if shape.key not in _INPUTS:
        g = torch.Generator().manual_seed(1000 + len(shape.key) + shape.M)
        n = n_max(shape)
        d = {"a": torch.randn(shape.M, shape.K, generator=g),
             "b": torch.randn(shape.K, n, generator=g) / math.sqrt(shape.K),
             "bias": torch.randn(n, generator=g) * 0.5,
             "c0": torch.randn(shape.M, n, generator=g),
             "aux_grad": torch.randn(shape.M, n, generator=g) * 1.5}
        gate = torch.randn(shape.M, n, generator=g)
        i = torch.arange(shape.M * n).view(shape.M, n) % 7
        gate[i == 0] = 0.0
        gate[i == 3] = -0.0
        d["aux_gate"] = gate
        _INPUTS[shape.key] = d
    return _INPUTS[shape.key]


def product(shape, planes, k=None):
    """a b in float64 over the first k of K (None: all), [M, n_max]; planes == 1: of the bf16-rounded
    operands.  Cached: every epilogue, layout and width of a shape shares one product."""
    key = (shape.key, planes == 1, k)
    if key not in _PRODUCTS:
        d = inputs(shape)
        a, b = d["a"], d["b"]
        if k is not None:
            a, b = a[:, :k], b[:k]
        if planes == 1:
            a, b = a.bfloat16(), b.bfloat16()
        _PRODUCTS[key] = a.to(F64) @ b.to(F64)
    return _PRODUCTS[key]


def wanted(kernel, epi, n, k=None, bias=True):
    """(C, aux written or None, bar of C, bar of aux) of a case, over rows [0, live M).  bias False: the
    call passes no usable bias (NULL, or all NaN to a bias-free epilogue)."""
    s = kernel.shape
    d = inputs(s)
    m = s.m_dev if kernel.form == "mdev" else s.M
    pre = product(s, kernel.planes, k)[:m, :n]
    aux = d["aux_gate"] if epi == L.EPI_ACCUM_GATE else d["aux_grad"]
    c, x = reference(epi, pre, d["bias"][:n] if bias else None, d["c0"][:m, :n], aux[:m, :n])
    amax, bmax = d["a"].abs().max().item(), d["b"].abs().max().item()
    kk = s.K if k is None else k
    return (c, x, bar(epi, amax, bmax, kk, kernel.planes, c),
            bar(epi, amax, bmax, kk, kernel.planes, x, aux_out=True) if x is not None else None)
