"""Shared by tests/test_gemm_map_kernels_gpu.py and tests/test_gemm_map_ref_cpu.py: the row maps
(NR_ROWS_GATHER, NR_ROWS_CONV3), the MN-contiguous A operand, split-K and the four adding / scattering
epilogues (NR_EPI_ATOMIC, _SCATTER, _SCATTER_STORE, _SCATTER_ZEROED) of nr_gemm_f32* as a table of
cases, one per kernel family x problem x width, with the inputs (built once per process on the CPU,
fixed seeds), the float64 references, the bars, and each case as an argument line of
tests/gemm_route_dump.cpp, so that the kernel a case means is pinned without a GPU.

Token geometry of the small shapes: 32 titles of L = 5 tokens, T = 160 = 64 + 64 + 32 = 128 + 32 (cuts
a 64-row and a 128-row tile), 5 divides none of 64, 128 and 32 (titles straddle tile and k-tile
edges), and 160 is a multiple of 32, so it is also a valid contraction.

Inputs.  A load-side table has V = 99 rows, rows 0 and 98 all NaN: row 0 is what the loaders read for
a CONV3 tap outside the title before they replace the value by zero, row 98 is what ids at and past a
device-resident extent name; live ids lie in [1, 97].  The padding columns of every stored operand
are NaN, and so are the rows of a plain operand at and past *m_dev / *k_dev.  SCATTER ids name 61
destination rows with repeats (row 0 the pad row, rows 54..59 absent, row 60 a guard row);
SCATTER_STORE ids are distinct (every 16th the pad row), rows past *m_dev name the guard row (the last).

Bars.  gemm_epi_util.gemm_tol(max|a|, max|b|, live K, planes) times c, the largest number of accumulator
values added into one destination element (1 for the stores, the K splits for NR_EPI_ATOMIC, the
reference's own count of contributions times the splits for NR_EPI_SCATTER), plus 2^-22 c max|want|
for the fp32 additions.  c comes from the route and the reference, never from the kernel."""
import collections
import math

import torch
import torch.nn.functional as F

from gemm_epi_util import F64, PREC, gemm_tol, parse_route  # noqa: F401  (re-exported to the tests)
from newsrec_amd import _lib as L

NAN = float("nan")
SEQ = 5             # tokens per title
V_LOAD = 99         # rows of a load-side table
V_SCATTER = 61      # destination rows of NR_EPI_SCATTER
V_STORE, V_STORE_BIG = 201, 2001   # destination rows of NR_EPI_SCATTER_STORE / _ZEROED

STORES = (L.EPI_SCATTER_STORE, L.EPI_SCATTER_ZEROED)
SCATTERS = (L.EPI_SCATTER,) + STORES
EPI_NAME = {L.EPI_STORE: "store", L.EPI_ATOMIC: "atomic", L.EPI_SCATTER: "scatter",
            L.EPI_SCATTER_STORE: "scatter_store", L.EPI_SCATTER_ZEROED: "scatter_zeroed"}

# family: the MAP_RATIO label (kernel family and planes); tile "BMxBN"; planes 3 bf16x6, 1 bf16, 0 exact
# f32; form static | dyn (mdev in the route's terms when m_dev is set); problem: a builder below; seg:
# columns per CONV3 tap; seq: tokens per title; split: the split_k passed; splits: what the route must
# say; m_dev / k_dev: device-resident extents or None; work: workspace=True; variant: "" | "odd_ld"
Case = collections.namedtuple(
    "Case", "id family tile planes form prec problem M N K seg seq split splits epi m_dev k_dev work variant")

# one operand as stored: `store` [rows][ld] host tensor (NaN padding), the view store[:, :cols] is what the
# call names; layout kc | mn; map plain | gather | conv3 with its ids
Operand = collections.namedtuple("Operand", "store cols layout map ids seg")


def round4(n):
    return (n + 3) // 4 * 4


# ---- inputs

def _seed(*key):
    s = 17
    for k in key:
        for ch in str(k):
            s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def load_ids(n, live=None, mult=11):
    """n ids in [1, V_LOAD - 2]; at and past `live`: the poison row V_LOAD - 1."""
    ids = 1 + (mult * torch.arange(n) + 3) % (V_LOAD - 2)
    if live is not None:
        ids[live:] = V_LOAD - 1
    return ids


def scatter_ids(n):
    """Ids with repeats over rows 1..53 of 61; every 16th the pad row 0."""
    ids = 1 + (7 * torch.arange(n)) % 53
    ids[::16] = 0
    return ids


def store_ids(n, live=None):
    """Distinct ids (but for the pad row 0 at every 16th); at and past `live`: the guard row."""
    big = n > V_STORE - 2
    v, mult = (V_STORE_BIG, 739) if big else (V_STORE, 37)
    ids = 1 + (mult * torch.arange(n)) % (v - 2)
    ids[::16] = 0
    if live is not None:
        ids[live:] = v - 1
    return ids, v


def table(g, width, ld, scale=1.0):
    """A load-side table [V_LOAD][ld]: rows 0 and V_LOAD - 1 and the columns past `width` NaN."""
    t = torch.full((V_LOAD, ld), NAN)
    t[1:V_LOAD - 1, :width] = torch.randn(V_LOAD - 2, width, generator=g) * scale
    return t


def padded(x, ld, live_rows=None):
    """x [r][c] stored with rows `ld` apart: padding columns, and rows at and past live_rows, NaN."""
    t = torch.full((x.shape[0], ld), NAN)
    r = x.shape[0] if live_rows is None else live_rows
    t[:r, :x.shape[1]] = x[:r]
    return t


def conv_cols(rows, seq):
    """rows [T][seg] of T / seq titles -> the zero-padded three-tap concatenation [T][3 seg]: columns
    [j seg, (j + 1) seg) of token t hold token t + j - 1 of the same title, zero outside it."""
    t, seg = rows.shape
    x = F.pad(rows.view(t // seq, seq, seg), (0, 0, 1, 1))
    return torch.cat([x[:, j:j + seq] for j in range(3)], dim=2).reshape(t, 3 * seg)


def scatter_sum(rows, cmap, ids, seq, seg, v, pad_row=0):
    """index_add_ of rows [m][N] (float64) through a destination row map into [v][N or seg]; the pad
    row's contributions are zero.  With rows of ones: the number of contributions per element."""
    m = rows.shape[0]
    if cmap == "gather":
        src = rows.clone()
        src[ids[:m] == pad_row] = 0
        return torch.zeros(v, rows.shape[1], dtype=rows.dtype).index_add_(0, ids[:m], src)
    out = torch.zeros(v, seg, dtype=rows.dtype)
    pos = torch.arange(m) % seq
    for j in range(3):
        ok = (pos + j - 1 >= 0) & (pos + j - 1 < seq)
        src_rows = torch.arange(m)[ok]
        dst = ids[src_rows + j - 1]
        src = rows[src_rows, j * seg:(j + 1) * seg].clone()
        src[dst == pad_row] = 0
        out.index_add_(0, dst, src)
    return out


_PROBLEMS = {}


class Problem:
    """The host side of a case: A, B (Operand), the logical operands a [M][K] and b [K][N] (fp32; rows
    of a past m_live and k past k_live are not part of the result), bias or None, and for the scatter
    epilogues the destination map (cmap, cids, cseg, v: destination rows)."""
    cmap = cids = bias = None
    cseg = 1
    v = 0


def problem(c):
    key = (c.problem, c.M, c.N, c.K, c.seg, c.seq, c.m_dev, c.k_dev, c.variant)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = _build(c)
    return _PROBLEMS[key]


def _build(c):
    g = _seed(c.problem, c.M, c.N, c.K, c.seg)
    M, N, K, p = c.M, c.N, c.K, Problem()
    p.m_live = c.m_dev if c.m_dev is not None else M
    p.k_live = c.k_dev if c.k_dev is not None else K
    ks = 1.0 / math.sqrt(K)
    odd = 1 if c.variant == "odd_ld" else 0

    def plain_kc(x, live=None, odd_ld=0):     # x [rows][K]
        return Operand(padded(x, round4(x.shape[1]) + 4 + odd_ld, live), x.shape[1], "kc", "plain", None, 1)

    def plain_mn(x, live=None, odd_ld=0, pad=0):   # x [K][rows]: stored rows are k
        return Operand(padded(x, round4(x.shape[1]) + pad + odd_ld, live), x.shape[1], "mn", "plain", None, 1)

    def rows_of(t, width, ids):
        return t[ids.clamp(max=V_LOAD - 2), :width]   # the poison row's stand-in is never part of a result

    if c.problem == "gather_fwd":             # table[ids] Wᵀ + bias
        t, ids = table(g, K, round4(K) + 4), load_ids(M, c.m_dev)
        w = torch.randn(N, K, generator=g) * ks
        p.A, p.B = Operand(t, K, "kc", "gather", ids, 1), plain_kc(w)
        p.a, p.b, p.bias = rows_of(t, K, ids), w.t().contiguous(), torch.randn(N, generator=g) * 0.5
    elif c.problem == "conv_fwd":             # cols W3ᵀ + bias
        t, ids = table(g, c.seg, c.seg + 4), load_ids(M)
        w = torch.randn(N, K, generator=g) * ks
        p.A, p.B = Operand(t, c.seg, "kc", "conv3", ids, c.seg), plain_kc(w, odd_ld=odd)
        p.a, p.b, p.bias = conv_cols(rows_of(t, c.seg, ids), c.seq), w.t().contiguous(), torch.randn(N, generator=g) * 0.5
    elif c.problem in ("scatter_gather", "scatter_conv3", "scatter_store"):   # dY W through a row map
        dy, w = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g) * ks
        p.A, p.B = plain_kc(dy, c.m_dev), plain_mn(w, pad=4 if N == 1024 else 0)   # ld 72 / 1028 at both widths
        p.a, p.b = dy, w
        if c.problem == "scatter_store":
            p.cmap, (p.cids, p.v) = "gather", store_ids(M, c.m_dev)
        else:
            p.cmap, p.cids, p.v = ("gather" if c.problem == "scatter_gather" else "conv3"), scatter_ids(M), V_SCATTER
            p.cseg = c.seg
    elif c.problem == "wgrad_plain":          # dYᵀ x
        dy, x = torch.randn(K, M, generator=g), torch.randn(K, N, generator=g) * ks
        p.A, p.B = plain_mn(dy, c.k_dev), plain_mn(x, c.k_dev)
        p.a, p.b = dy.t().contiguous(), x
    elif c.problem == "wgrad_gather":         # dYᵀ table[ids]
        dy, ids = torch.randn(K, M, generator=g), load_ids(K, c.k_dev)
        t = table(g, N, round4(N) + (0 if N > 500 else 4), ks)
        p.A, p.B = plain_mn(dy, c.k_dev), Operand(t, N, "mn", "gather", ids, 1)
        p.a, p.b = dy.t().contiguous(), rows_of(t, N, ids)
    elif c.problem == "wgrad_conv3":          # dYᵀ cols
        dy, ids = torch.randn(K, M, generator=g), load_ids(K)
        t = table(g, c.seg, c.seg + 4, ks)
        p.A, p.B = plain_mn(dy, odd_ld=odd), Operand(t, c.seg, "mn", "conv3", ids, c.seg)
        p.a, p.b = dy.t().contiguous(), conv_cols(rows_of(t, c.seg, ids), c.seq)
    # the mode pairs only the generic kernel has (store + bias)
    elif c.problem == "mn_gather_a":          # A [K][M] gathered: stored row k = table[ids[k]]
        t, ids = table(g, M, round4(M) + 4), load_ids(K)
        w = torch.randn(N, K, generator=g) * ks
        p.A, p.B = Operand(t, M, "mn", "gather", ids, 1), plain_kc(w)
        p.a, p.b, p.bias = rows_of(t, M, ids).t().contiguous(), w.t().contiguous(), torch.randn(N, generator=g)
    elif c.problem == "kc_gather_b":          # B [N][K] gathered
        x, ids = torch.randn(M, K, generator=g), load_ids(N)
        t = table(g, K, round4(K) + 4, ks)
        p.A, p.B = plain_kc(x), Operand(t, K, "kc", "gather", ids, 1)
        p.a, p.b, p.bias = x, rows_of(t, K, ids).t().contiguous(), torch.randn(N, generator=g)
    elif c.problem == "kc_conv3_b":           # B [N tokens][3 seg] through the taps
        x, ids = torch.randn(M, K, generator=g), load_ids(N)
        t = table(g, c.seg, c.seg + 4, ks)
        p.A, p.B = plain_kc(x), Operand(t, c.seg, "kc", "conv3", ids, c.seg)
        p.a, p.b, p.bias = x, conv_cols(rows_of(t, c.seg, ids), c.seq).t().contiguous(), torch.randn(N, generator=g)
    elif c.problem == "mn_conv3_a":           # A [K tokens][M = 3 seg] through the taps
        t, ids = table(g, c.seg, c.seg + 4), load_ids(K)
        w = torch.randn(K, N, generator=g) * ks
        p.A, p.B = Operand(t, c.seg, "mn", "conv3", ids, c.seg), plain_mn(w)
        p.a, p.b, p.bias = conv_cols(rows_of(t, c.seg, ids), c.seq).t().contiguous(), w, torch.randn(N, generator=g)
    else:
        raise ValueError(c.problem)
    assert p.a.shape == (M, K) and p.b.shape == (K, N), (c.id, p.a.shape, p.b.shape)
    return p


# ---- references and bars

_ACC = {}


def accumulators(c):
    """a b in float64 over the live rows and the live k, [m_live][N]; planes == 1: of the bf16-rounded
    operands.  Cached: the epilogues, splits and forms of a problem share it."""
    p = problem(c)
    key = (id(p), c.planes == 1)
    if key not in _ACC:
        a, b = p.a[:p.m_live, :p.k_live], p.b[:p.k_live]
        if c.planes == 1:
            a, b = a.bfloat16(), b.bfloat16()
        _ACC[key] = a.to(F64) @ b.to(F64)
    return _ACC[key]


def dest_shape(c):
    """(rows, columns) of the destination matrix."""
    p = problem(c)
    if c.epi in SCATTERS:
        return p.v, (p.cseg if p.cmap == "conv3" else c.N)
    return c.M, c.N


def entry_fill(c):
    """The destination window on entry, fp32 [rows][cols] (None: NaN, the store epilogue): finite random
    values everywhere; NR_EPI_SCATTER_ZEROED: the rows the live ids name zero."""
    if c.epi == L.EPI_STORE:
        return None
    rows, cols = dest_shape(c)
    c0 = torch.randn(rows, cols, generator=_seed("c0", c.problem, rows, cols))
    if c.epi == L.EPI_SCATTER_ZEROED:
        p = problem(c)
        named = p.cids[:p.m_live]
        c0[named[named != 0]] = 0.0
    return c0


def wanted(c):
    """(want float64 [rows][cols], touched bool [rows][cols], bar, contributions c) of a case: the
    destination after the call where `touched`; everything else must keep its bits."""
    p = problem(c)
    acc = accumulators(c)
    rows, cols = dest_shape(c)
    touched = torch.zeros(rows, cols, dtype=torch.bool)
    contrib = 1
    if c.epi == L.EPI_STORE:
        want = torch.zeros(rows, cols, dtype=F64)
        want[:p.m_live] = acc + (p.bias.to(F64) if p.bias is not None else 0.0)
        touched[:p.m_live] = True
    elif c.epi == L.EPI_ATOMIC:
        want = entry_fill(c).to(F64) + acc
        touched[:] = True
        contrib = c.splits
    elif c.epi == L.EPI_SCATTER:
        counts = scatter_sum(torch.ones_like(acc), p.cmap, p.cids, c.seq, p.cseg, p.v)
        want = entry_fill(c).to(F64) + scatter_sum(acc, p.cmap, p.cids, c.seq, p.cseg, p.v)
        touched = counts > 0
        contrib = int(counts.max().item()) * c.splits
    else:   # the distinct-row stores: the named rows hold the accumulators, not entry + accumulators
        want = entry_fill(c).to(F64)
        ids = p.cids[:p.m_live]
        live = ids != 0
        want[ids[live]] = acc[live]
        touched[ids[live]] = True
    amax = p.a[:p.m_live, :p.k_live].abs().max().item() if p.k_live else 0.0
    bmax = p.b[:p.k_live].abs().max().item() if p.k_live else 0.0
    wmax = want[touched].abs().max().item()
    return want, touched, contrib * gemm_tol(amax, bmax, p.k_live, c.planes) + 2.0 ** -22 * contrib * wmax, contrib


# ---- the case table

FAST = [("f32_64", 64, 0, "static", "f32"), ("f32_64", 64, 0, "static", "bf16x6"),
        ("f32_128", 128, 0, "dyn", "f32"), ("split_128_3", 128, 3, "dyn", "bf16x6"),
        ("split_128_1", 128, 1, "static", "bf16"), ("split_128_1", 128, 1, "dyn", "bf16")]
T = 32 * SEQ
ST, AT, SC, SS, SZ = L.EPI_STORE, L.EPI_ATOMIC, L.EPI_SCATTER, L.EPI_SCATTER_STORE, L.EPI_SCATTER_ZEROED


def _splits(k, want):
    kc = ((k + want - 1) // want + 31) // 32 * 32
    return max((k + kc - 1) // kc, 1)


def _case(fam, problem_, m, n, k, epi, seg=1, seq=SEQ, split=1, splits=None, m_dev=None, k_dev=None, work=False,
          variant="", tile=None):
    family, t, planes, form, prec = fam
    tile = tile or "%dx%d" % (t, t)
    cid = "%s-%s-%s-%s-%dx%dx%d" % (family, form, prec, problem_, m, n, k)
    if epi in SCATTERS and problem_ == "scatter_store":
        cid += "-" + EPI_NAME[epi]
    for tag, val in (("seg", seg if seg > 1 else None), ("seq", seq if seq != SEQ else None),
                     ("split", split if split > 1 else None), ("mdev", m_dev), ("kdev", k_dev),
                     ("ws", 1 if work else None), (variant, 1 if variant else None)):
        if val is not None:
            cid += "-%s%s" % (tag, "" if tag == variant else val)
    return Case(cid, family, tile, planes, form, prec, problem_, m, n, k, seg, seq, split,
                splits if splits is not None else _splits(k, split), epi, m_dev, k_dev, work, variant)


def small_cases():
    """The eight problems on the 64-tile and 128-tile families, and the device extents on the latter."""
    out = []
    for fam in FAST:
        for n in (160, 158):
            out.append(_case(fam, "gather_fwd", T, n, 64, ST))
            for seg in (64, 128):
                out.append(_case(fam, "conv_fwd", T, n, 3 * seg, ST, seg=seg))
        for n in (72, 70):
            for sp in (1, 2):
                out.append(_case(fam, "scatter_gather", T, n, 160, SC, split=sp))
            for epi in (SS, SZ):
                out.append(_case(fam, "scatter_store", T, n, 160, epi))
            for m in (160, 158):
                for sp in (1, 2):
                    out.append(_case(fam, "wgrad_plain", m, n, T, AT, split=sp))
            out.append(_case(fam, "wgrad_gather", 160, n, T, AT, split=2))
        out.append(_case(fam, "scatter_conv3", T, 72, 160, SC, seg=24))
        # seg 64 is eligible for the 64 x 64 kernel only (whole tap tiles), seg 128 for the 128-tile ones
        seg = 64 if fam[1] == 64 else 128
        out.append(_case(fam, "wgrad_conv3", 160, 3 * seg, T, AT, seg=seg, split=2))
        if fam[3] == "dyn":
            for n in (160, 158):
                out.append(_case(fam, "gather_fwd", T, n, 64, ST, m_dev=100))
            for n in (72, 70):
                out.append(_case(fam, "scatter_store", T, n, 160, SS, m_dev=100))
                for kd in (128, 96):   # of the bound 160; the kernels split the live K two ways
                    out.append(_case(fam, "wgrad_gather", 160, n, T, AT, split=2, k_dev=kd))
                    out.append(_case(fam, "wgrad_plain", 160, n, T, AT, split=2, k_dev=kd))
    return out


GENERIC = ("generic", 64, 0, "static", "f32")


def generic_cases():
    """Static form, f32 (every prec runs the same code there): the eight problems at a contraction
    (or a leading dimension) the fast kernels do not take, the four mode pairs only this kernel has,
    and one title per token (seq_len = 1) as a CONV3 scatter map."""
    g = GENERIC
    return [
        _case(g, "gather_fwd", T, 158, 70, ST),
        _case(g, "conv_fwd", T, 158, 192, ST, seg=64, variant="odd_ld"),
        _case(g, "scatter_gather", T, 70, 155, SC, split=2),
        _case(g, "scatter_conv3", T, 72, 155, SC, seg=24),
        _case(g, "scatter_store", T, 70, 155, SS),
        _case(g, "scatter_store", T, 70, 155, SZ),
        _case(g, "wgrad_plain", 158, 70, 155, AT, split=2),
        _case(g, "wgrad_gather", 160, 70, 155, AT, split=2),
        _case(g, "wgrad_conv3", 160, 192, T, AT, seg=64, split=2, variant="odd_ld"),
        _case(g, "mn_gather_a", 70, 50, 45, ST),
        _case(g, "kc_gather_b", 70, 50, 45, ST),
        _case(g, "kc_conv3_b", 70, 50, 96, ST, seg=32),
        _case(g, "mn_conv3_a", 192, 50, 45, ST, seg=64),
        _case(g, "scatter_conv3", T, 72, 160, SC, seg=24, seq=1),
    ]


def seq1_load_cases():
    """seq_len = 1 as a CONV3 load operand (only the centre tap exists), on the 64 x 64 kernel."""
    return [_case(FAST[0], "conv_fwd", T, 158, 192, ST, seg=64, seq=1)]


BIG = [("big_3", 256, 3, "dyn", "bf16x6"), ("big_1", 256, 1, "dyn", "bf16")]


def big_cases():
    """The 256-row kernel: the gathered forward and the distinct-row table gradient under a device M
    (1600 of 1800: tile row 6 holds 64 live rows, tile row 7 none), and the split-K weight gradients
    (4 splits of 512) with atomics, through the workspace, and under a device K."""
    out = []
    for fam in BIG:
        for n in (1024, 1026):
            out.append(_case(fam, "gather_fwd", 1800, n, 512, ST, m_dev=1600, tile="256x256"))
            out.append(_case(fam, "scatter_store", 1800, n, 512, SS, m_dev=1600, tile="256x256"))
        out.append(_case(fam, "scatter_store", 1800, 1024, 512, SZ, m_dev=1600, tile="256x256"))
        if fam[2] == 3:   # the stream-K tail through the workspace is the bf16x6 kernel's
            out.append(_case(fam, "scatter_store", 1800, 1024, 512, SZ, m_dev=1600, work=True, tile="256x256"))
        for prob in ("wgrad_gather", "wgrad_plain"):
            shapes = [(264, 520), (262, 518)] if prob == "wgrad_gather" else [(264, 520)]
            for m, n in shapes:
                kw = dict(split=4, splits=4, tile="256x128")
                out.append(_case(fam, prob, m, n, 2048, AT, **kw))
                # the binding reaches the dynamic form with a workspace only through a device extent
                # (or a CU cap): the workspace case passes *k_dev = K
                out.append(_case(fam, prob, m, n, 2048, AT, k_dev=2048, work=True, **kw))
                out.append(_case(fam, prob, m, n, 2048, AT, k_dev=1600, **kw))   # the last split: 64 live k
                out.append(_case(fam, prob, m, n, 2048, AT, k_dev=1024, **kw))   # the last two splits empty
        out.append(_case(fam, "wgrad_gather", 264, 1024, 2048, AT, split=4, splits=4, k_dev=1600, tile="256x256"))
    return out


def all_cases():
    return small_cases() + seq1_load_cases() + generic_cases() + big_cases()


# ---- routes

_MODE = {"kc": 0, "mn": 3, "plain": 0, "gather": 1, "conv3": 2}


def route_form(c):
    return "mdev" if c.m_dev is not None else ("dyn" if c.form == "dyn" else "static")


def route_argv(c):
    """The case as arguments of tests/gemm_route_dump.cpp."""
    p = problem(c)
    argv = [c.id, str(c.M), str(c.N), str(c.K), p.A.layout, str(p.A.store.shape[1]), p.B.layout,
            str(p.B.store.shape[1]), str(c.epi), route_form(c), c.prec,
            "amap=" + p.A.map, "bmap=" + p.B.map, "aseg=%d" % p.A.seg, "bseg=%d" % p.B.seg, "seq=%d" % c.seq,
            "split=%d" % c.split, "work=%d" % (1 if c.work else 0)]
    if p.cmap:
        argv += ["cmap=" + p.cmap, "cseg=%d" % p.cseg]
    return argv


def route_fields(c):
    """What the dumped line must say of the case."""
    p = problem(c)
    generic = c.family == "generic"
    epi = c.epi
    if epi == L.EPI_SCATTER_ZEROED:   # the fast kernels store (rows zero on entry), the generic one adds
        epi = L.EPI_SCATTER if generic else L.EPI_SCATTER_STORE
    adding = c.epi in (L.EPI_ATOMIC, L.EPI_SCATTER)
    return {"family": c.family.rsplit("_", 1)[0] if c.family[-2:] in ("_3", "_1") else c.family,
            "tile": c.tile, "planes": str(c.planes),
            "modes": "%d,%d" % (_MODE[p.A.layout] + _MODE[p.A.map], _MODE[p.B.layout] + _MODE[p.B.map]),
            "tr": "0" if generic or adding else "1", "epi": str(epi), "splits": str(c.splits),
            "slab": "1" if c.work and c.epi == L.EPI_ATOMIC else "0",
            "tail": "16" if c.epi == L.EPI_SCATTER_ZEROED and c.family.startswith("big") else "0"}
