"""The distinct-row kernels of csrc/dedup.hip and csrc/conv3_rows.hip, each against the plain
statements of tests/dedup_util.py (held against numpy / autograd / conv1d in test_dedup_ref_cpu.py).

* nr_segment_rows_sum, _multi, _multi_zero: segment geometry chosen by the case (dedup_util.GEOMETRY),
  integer data, exact equality, at every width class of the two passes; src and dst are column and row
  slices of wider, longer buffers (NaN around src, a sentinel around dst), so a read or a store outside
  [rows, width] shows.
* nr_segment_rows_sum_conv3 and nr_conv3_rows_fwd: the same on the title edges (L = 1, 2, 3, 30).
* nr_cnn_pack_weights / nr_cnn_unpack_grads: exact copies, past one grid of threads.
* nr_unique_rows: vocabulary sizes around the scan tile and around the switch between LDS and global
  tile totals, full count workgroups of distinct / equal ids, fill_row, out-of-range ids.

The only tolerances are the two derived bounds of the random-data cases: 2 n 2^-24 sum|terms| for a sum
of n fp32 terms in any order (dedup_util.sum_bound)."""
import functools

import pytest
import torch

import dedup_util as D
from newsrec_amd import _lib as L
from newsrec_amd import functions as F
from newsrec_amd import kernels as K

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = -12345.0     # never a sum of int_rows entries times a plausible count, never zero
F64 = torch.float64

# width: float4 columns w4 = W / 4 against the fix-up workgroup's 1024 threads -- 1 and 9 (9 divides
# no power of two: idle threads behind the last thread group), 64, 288 (the train step's 1152: three
# groups), 513 (one group, idle threads), 1024 (one group, no idle thread), 1025 (a second column trip in
# both passes)
WIDTHS = [4, 36, 256, 1152, 2052, 4096, 4100]
WMAX = max(WIDTHS)
CASES = sorted(D.GEOMETRY)


@functools.lru_cache(maxsize=2)
def _case_rows(name):
    """(case, its integer rows at the widest width on the GPU, the exact sums as float32 on the CPU)"""
    c = D.geometry_case(name)
    rows = D.int_rows(c.ids.numel(), WMAX, seed=len(name))
    want = D.segment_sum_reference(rows, c.ref, torch.int64)
    assert int(want.abs().max()) < 2 ** 24
    return c, rows.cuda(), want.float()


def _check_unique(ur, ref, T):
    """Every output of nr_unique_rows against the reference; tokens inside a segment as sorted sets."""
    torch.cuda.synchronize()
    U, Up, bad, Tc = ref.counts
    assert tuple(ur.counts.tolist()) == ref.counts
    assert torch.equal(ur.uids[:Up].cpu(), ref.uids)
    assert torch.equal(ur.inv.cpu(), ref.inv)
    off = ur.seg_off[:Up + 1].cpu().long()
    assert torch.equal(off, ref.seg_off)
    lens = ref.seg_off[1:U + 1] - ref.seg_off[:U]
    rows = torch.repeat_interleave(torch.arange(U), lens)
    assert torch.equal(ur.seg_of[:Tc].cpu().long(), rows)
    tok = ur.seg_tok[:Tc].cpu().long()
    assert Tc == 0 or (int(tok.min()) >= 0 and int(tok.max()) < T)
    want = torch.cat(ref.segs) if U else torch.zeros(0, dtype=torch.int64)
    assert torch.equal(torch.sort(rows * max(T, 1) + tok).values, rows * max(T, 1) + want)
    return off


def _case_csr(name):
    c = D.geometry_case(name)
    ur = K.UniqueRows(c.ids.cuda(), c.V)
    off = _check_unique(ur, c.ref, c.ids.numel())
    segs = D.segment_classes(off[:c.ref.counts[0] + 1])   # the device's own CSR holds the case's classes
    for need in c.needs:
        assert D.has_class(segs, **need), (name, need)
    return c, ur, segs


def _sum_call(ur, method, rows, T, W):
    """src = buf[:T, :W] of a NaN-filled [T + 1, W + 4], dst = buf[:cap, :W] of a sentinel-filled
    [cap + 1, W + 8] -> the whole dst buffer on the CPU."""
    src = torch.full((T + 1, W + 4), NAN, device="cuda")
    src[:T, :W] = rows[:, :W]
    dst = torch.full((ur.cap + 1, W + 8), SENT, device="cuda")
    getattr(ur, method)(src[:T, :W], dst[:ur.cap, :W])
    torch.cuda.synchronize()
    return dst.cpu()


def _check_window(buf, want, what):
    """buf[:rows, :cols] equals `want` exactly (no NaN), everything around it is still the sentinel."""
    r, c = want.shape
    inside = buf[:r, :c]
    assert not torch.isnan(inside).any(), what
    bad = torch.nonzero(inside != want)
    assert bad.numel() == 0, (what, "first differing (row, column):", bad[0].tolist(), len(bad))
    outside = buf.clone()
    outside[:r, :c] = SENT
    assert (outside == SENT).all(), (what, "stored outside [:%d, :%d]" % (r, c))


def _single_rows(ref):
    U = ref.counts[0]
    single = torch.zeros(ref.counts[1], dtype=torch.bool)
    single[:U] = (ref.seg_off[1:U + 1] - ref.seg_off[:U]) == 1
    return single


# ---- nr_segment_rows_sum / _multi: geometry x width, integer data, exact

@pytest.mark.parametrize("name,W", [(n, w) for n in CASES for w in WIDTHS])
def test_segment_sum_exact(name, W):
    c, rows, want = _case_rows(name)
    _, ur, _ = _case_csr(name)
    Up = c.ref.counts[1]
    assert ur.cap >= Up
    got = _sum_call(ur, "segment_sum", rows, c.ids.numel(), W)
    _check_window(got, want[:, :W], (name, W))   # pad rows [U, U_pad) zero, rows from U_pad on untouched


@pytest.mark.parametrize("name,W", [(n, w) for n in CASES for w in WIDTHS])
def test_segment_sum_multi_exact(name, W):
    """Rows of two or more tokens as nr_segment_rows_sum's (bitwise), one-token rows left alone."""
    c, rows, want = _case_rows(name)
    _, ur, segs = _case_csr(name)
    single = _single_rows(c.ref)
    assert single.any() and not single.all()
    if name == "sparse":
        assert 0 in D.single_only_ranges(segs)    # a pass-1 workgroup with nothing to sum
    T = c.ids.numel()
    full = _sum_call(ur, "segment_sum", rows, T, W)
    got = _sum_call(ur, "segment_sum_multi", rows, T, W)
    expect = want[:, :W].clone()
    expect[single] = SENT
    _check_window(got, expect, (name, W))
    multi = torch.nonzero(~single).reshape(-1)
    assert torch.equal(got[multi].view(torch.int32), full[multi].view(torch.int32))


# ---- nr_segment_rows_sum_multi_zero against the two calls, one case per segment class

def _zero_case(name):
    if name == "masked":
        ids, V, gm = D.masked_case()
        return ids, V, gm, D.unique_rows_reference(ids, V, 0, gm)
    c = D.geometry_case(name)
    return c.ids, c.V, None, c.ref


@pytest.mark.parametrize("name,cls", [("aligned", "whole"), ("offset", "cut_wave"), ("wave_block", "cut_block"),
                                      ("sparse", "single"), ("masked", "empty")])
def test_segment_sum_multi_zero_exact(name, cls):
    W, ZW, pad_row = 256, 12, 0
    ids, V, gm, ref = _zero_case(name)
    assert V % 16 and D.has_class(D.segment_classes(ref.seg_off[:ref.counts[0] + 1]), cls)
    T = ids.numel()
    ur = K.UniqueRows(ids.cuda(), V, grad_mask=None if gm is None else gm.cuda())
    _check_unique(ur, ref, T)
    rows = D.int_rows(T, W, seed=5)
    src = torch.full((T + 1, W + 4), NAN, device="cuda")
    src[:T, :W] = rows.cuda()

    def run(fused):
        dst = torch.full((ur.cap + 1, W + 8), SENT, device="cuda")
        z = torch.full((V + 1, ZW + 4), SENT, device="cuda")   # padded row stride, one row more
        if fused:
            assert ur.segment_sum_multi_zero(src[:T, :W], dst[:ur.cap, :W], z[:V, :ZW], pad_row) is True
        else:
            ur.segment_sum_multi(src[:T, :W], dst[:ur.cap, :W])
            assert ur.zero_absent_rows(z[:V, :ZW], pad_row) is True
        torch.cuda.synchronize()
        return dst.cpu(), z.cpu()

    (d0, z0), (d1, z1) = run(False), run(True)
    assert torch.equal(d0.view(torch.int32), d1.view(torch.int32)) and torch.equal(z0.view(torch.int32),
                                                                                   z1.view(torch.int32))
    expect = D.segment_sum_reference(rows, ref, torch.int64).float()
    expect[_single_rows(ref)] = SENT
    _check_window(d1, expect, name)
    present = torch.zeros(V + 1, dtype=torch.bool)
    present[ids[(ids >= 0) & (ids < V)]] = True
    present[pad_row] = False
    zwant = torch.full((V + 1, ZW + 4), SENT)
    zwant[:V, :ZW][~present[:V]] = 0.0
    assert torch.equal(z1, zwant)


# ---- grad_mask: every mask dtype, empty segments, T_csr < T

@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8, torch.int64, torch.float32, torch.float64])
def test_grad_mask_segments_exact(dtype):
    ids, V, gm = D.masked_case()
    T, W = ids.numel(), 36
    ref = D.unique_rows_reference(ids, V, 0, gm)
    ur = K.UniqueRows(ids.cuda(), V, grad_mask=gm.to(dtype).cuda())
    off = _check_unique(ur, ref, T)
    U, Up, _, Tc = ref.counts
    assert Tc < T
    segs = D.segment_classes(off[:U + 1])
    empty = [u for u, s in enumerate(segs) if s.cls == "empty"]
    assert len(empty) == 2
    rows = D.int_rows(T, W, seed=6)
    want = D.segment_sum_reference(rows, ref, torch.int64).float()
    assert (want[empty] == 0).all() and (want[U:] == 0).all()
    _check_window(_sum_call(ur, "segment_sum", rows.cuda(), T, W), want, str(dtype))


# ---- random data: the derived bound, one case per fix-up path

@pytest.mark.parametrize("name,cls", [("offset", "cut_wave"), ("wave_block", "cut_block")])
def test_segment_sum_random_within_the_fp32_bound(name, cls):
    W = 1152
    c, ur, segs = _case_csr(name)
    assert D.has_class(segs, cls) and (cls == "cut_block" or not D.has_class(segs, "cut_block"))
    T = c.ids.numel()
    src = torch.randn(T, W, generator=torch.Generator().manual_seed(12))
    got = _sum_call(ur, "segment_sum", src.cuda(), T, W)
    U, Up = c.ref.counts[:2]
    want = D.segment_sum_reference(src, c.ref)
    n = (c.ref.seg_off[1:] - c.ref.seg_off[:-1]).double()[:, None]
    bound = D.sum_bound(n, D.segment_sum_reference(src.abs(), c.ref))
    err = (got[:Up, :W].double() - want).abs()
    print("%s: max err %.3e, max err / bound %.3f" % (name, float(err.max()),
                                                      float((err[:U] / bound[:U]).max())))
    assert (err <= bound).all()


# ---- nr_segment_rows_sum_conv3

CONV3_TITLES = {1: 901, 2: 450, 3: 360, 30: 360}
HOT, CONV3_V = 1, 303


def _conv3_ids(Lq):
    """Titles of Lq tokens: id HOT at position 0 of three titles in four and (Lq > 1) at position Lq - 1 of
    three in four -- more than 8 ranges of tokens -- the last title's last token among them; the rest
    uniform over 298 ids."""
    n = CONV3_TITLES[Lq]
    ids = torch.randint(2, 300, (n, Lq), generator=torch.Generator().manual_seed(40 + Lq))
    i = torch.arange(n)
    ids[i % 4 != 3, 0] = HOT
    if Lq > 1:
        ids[i % 4 != 0, Lq - 1] = HOT
    return ids.reshape(-1)


def _conv3_setup(Lq):
    ids = _conv3_ids(Lq)
    T = ids.numel()
    ref = D.unique_rows_reference(ids, CONV3_V)
    ur = K.UniqueRows(ids.cuda(), CONV3_V)
    off = _check_unique(ur, ref, T)
    segs = D.segment_classes(off[:ref.counts[0] + 1])
    hot = int(ref.inv[0])
    assert int(ref.uids[hot]) == HOT and segs[hot].cls == "cut_block"
    assert segs[int(ref.inv[T - 1])].end - segs[int(ref.inv[T - 1])].start >= 2   # the last token: not alone
    pos = ref.segs[hot] % Lq
    assert (pos == 0).any() and (pos == Lq - 1).any()
    return ids, T, ref, ur


def _conv3_call(ur, src_rows, T, tw, Lq):
    src = torch.full((T + 1, tw + 4), NAN, device="cuda")
    src[:T, :tw] = src_rows.cuda()
    dst = torch.full((ur.cap + 1, 3 * tw + 8), SENT, device="cuda")
    ur.segment_sum_conv3(src[:T, :tw], dst[:ur.cap, :3 * tw], tw, Lq)
    torch.cuda.synchronize()
    return dst.cpu()


@pytest.mark.parametrize("tw", [4, 160])
@pytest.mark.parametrize("Lq", [1, 2, 3, 30])
def test_segment_sum_conv3_exact(Lq, tw):
    ids, T, ref, ur = _conv3_setup(Lq)
    rows = D.int_rows(T, tw, seed=Lq + tw)
    want = D.segment_sum_conv3_reference(rows, Lq, ref, torch.int64).float()
    if Lq == 1:   # no neighbour inside the title: the outer taps are zero
        assert (want[:, :tw] == 0).all() and (want[:, 2 * tw:] == 0).all()
    _check_window(_conv3_call(ur, rows, T, tw, Lq), want, (Lq, tw))


def test_segment_sum_conv3_random_within_the_fp32_bound():
    Lq, tw = 30, 160
    ids, T, ref, ur = _conv3_setup(Lq)
    src = torch.randn(T, tw, generator=torch.Generator().manual_seed(13))
    got = _conv3_call(ur, src, T, tw, Lq)
    U, Up = ref.counts[:2]
    want = D.segment_sum_conv3_reference(src, Lq, ref)
    n = D.segment_sum_conv3_reference(torch.ones(T, tw), Lq, ref)   # contributing terms per element
    bound = D.sum_bound(n, D.segment_sum_conv3_reference(src.abs(), Lq, ref))
    err = (got[:Up, :3 * tw].double() - want).abs()
    print("conv3: max err %.3e, longest sum %d terms" % (float(err.max()), int(n.max())))
    assert (err <= bound).all()


# ---- nr_conv3_rows_fwd

def _conv3_fwd_call(P, U, tw, H, inv, Lq, bias, relu):
    T = inv.numel()
    Pb = torch.full((U + 1, 3 * tw + 4), NAN, device="cuda")
    Pb[:U, :3 * tw] = P.cuda()
    out = torch.full((T + 1, tw + 4), SENT, device="cuda")
    K.conv3_rows_fwd(Pb[:U, :3 * tw], tw, H, inv.cuda(), Lq, None if bias is None else bias.cuda(),
                     out[:T, :tw], relu=relu)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("Lq", [1, 2, 30])
@pytest.mark.parametrize("tw,H", [(4, 1), (4, 4), (160, 150), (160, 160), (32, 25)])
def test_conv3_rows_fwd_exact(tw, H, Lq):
    """Integer P and bias: exact, with and without ReLU and bias; columns [H, tw) exactly zero (for
    (32, 25) one partial float4 and one whole), P and out inside wider, longer buffers."""
    n, U = 9, 20
    T = n * Lq
    g = torch.Generator().manual_seed(tw + H + Lq)
    inv = torch.randint(0, U, (T,), generator=g)
    P = D.int_rows(U, 3 * tw, seed=tw * H + Lq)
    bias_i = D.int_rows(1, H, seed=H)[0]
    for relu in (False, True):
        for bias in (None, bias_i):
            want = D.conv3_rows_reference(P, inv, Lq, bias, H, relu)
            assert (want[:, H:] == 0).all()
            if not relu and T * H >= 100:
                assert (want < 0).any()
            got = _conv3_fwd_call(P, U, tw, H, inv, Lq, bias, relu)
            _check_window(got, want.float(), (tw, H, Lq, relu, bias is not None))


def test_conv3_rows_fwd_random_within_the_fp32_bound():
    tw, H, Lq, n, U = 160, 150, 30, 40, 200
    T = n * Lq
    g = torch.Generator().manual_seed(14)
    inv = torch.randint(0, U, (T,), generator=g)
    P = torch.randn(U, 3 * tw, generator=g)
    bias = torch.randn(H, generator=g)
    got = _conv3_fwd_call(P, U, tw, H, inv, Lq, bias, True)
    want = D.conv3_rows_reference(P, inv, Lq, bias, H, True)
    # three taps and the bias: a sum of 4 terms; ReLU is 1-Lipschitz, so the bound carries through it
    bound = D.sum_bound(4, D.conv3_rows_abs_reference(P, inv, Lq, bias, H))
    err = (got[:T, :H].double() - want[:, :H]).abs()
    print("conv3 fwd: max err %.3e, max err / bound %.3f" % (float(err.max()), float((err / bound).max())))
    assert (err <= bound).all()
    assert (got[:T, H:tw] == 0).all() and (got[:T, tw:] == SENT).all() and (got[T] == SENT).all()


# ---- nr_cnn_pack_weights / nr_cnn_unpack_grads

PACK_SHAPES = [(1, 1, 1), (3, 5, 4), (150, 768, 160), (20, 64, 32)]
GRID_THREADS = 1024 * 256    # both kernels' launch: a second grid-stride trip above this many elements


def _guarded(n):
    """A sentinel-filled flat buffer of n + 4 floats: the kernel gets the first n."""
    return torch.full((n + 4,), SENT, device="cuda")


def _exact_flat(buf, want):
    n = want.numel()
    got = buf.cpu()
    assert torch.equal(got[:n].view(torch.int32), want.reshape(-1).contiguous().view(torch.int32))
    assert (got[n:] == SENT).all()


@pytest.mark.parametrize("with_w3tt", [True, False])
@pytest.mark.parametrize("H,E,Hp", PACK_SHAPES)
def test_cnn_pack_unpack_exact(H, E, Hp, with_w3tt):
    if (H, E, Hp) == (150, 768, 160):
        assert 3 * Hp * E > GRID_THREADS and 3 * H * E > GRID_THREADS
    g = torch.Generator().manual_seed(H * E + Hp)
    cw, wq, bq = (torch.randn(H, E, 3, generator=g), torch.randn(H, H, generator=g), torch.randn(H, generator=g))
    w3t, wqp, bqp, w3tt = _guarded(3 * Hp * E), _guarded(Hp * Hp), _guarded(Hp), _guarded(3 * Hp * E)
    cwd, wqd, bqd = cw.cuda(), wq.cuda(), bq.cuda()
    L.call("nr_cnn_pack_weights", L.ptr(cwd), L.ptr(wqd), L.ptr(bqd), H, E, Hp, L.ptr(w3t), L.ptr(wqp), L.ptr(bqp),
           L.ptr(w3tt) if with_w3tt else None, L.stream_ptr(cwd))
    torch.cuda.synchronize()
    r3, rq, rb, r3t = D.pack_reference(cw, wq, bq, Hp)
    _exact_flat(w3t, r3)
    _exact_flat(wqp, rq)
    _exact_flat(bqp, rb)
    if with_w3tt:
        _exact_flat(w3tt, r3t)
        assert torch.equal(w3tt[:3 * Hp * E].view(E, 3 * Hp).t().contiguous(), w3t[:3 * Hp * E].view(3 * Hp, E))
    else:
        assert (w3tt == SENT).all()
    p3 = w3t[:3 * Hp * E].view(3, Hp, E).cpu()
    assert (p3[:, H:] == 0).all() and (wqp[:Hp * Hp].view(Hp, Hp).cpu()[H:] == 0).all()
    assert (wqp[:Hp * Hp].view(Hp, Hp).cpu()[:, H:] == 0).all() and (bqp[:Hp].cpu()[H:] == 0).all()

    def unpack(d3, dq, db):
        dcw, dwq, dbq = _guarded(3 * H * E), _guarded(H * H), _guarded(H)
        L.call("nr_cnn_unpack_grads", L.ptr(d3), L.ptr(dq), L.ptr(db), H, E, Hp, L.ptr(dcw), L.ptr(dwq), L.ptr(dbq),
               L.stream_ptr(d3))
        torch.cuda.synchronize()
        return dcw, dwq, dbq

    # the round trip, then gradients that are nonzero in the padded rows and columns too
    for got, want in zip(unpack(w3t, wqp, bqp), (cw, wq, bq)):
        _exact_flat(got, want)
    d3, dq, db = (torch.randn(3 * Hp, E, generator=g), torch.randn(Hp, Hp, generator=g), torch.randn(Hp, generator=g))
    for got, want in zip(unpack(d3.cuda(), dq.cuda(), db.cuda()), D.unpack_reference(d3, dq, db, H, E, Hp)):
        _exact_flat(got, want)


@pytest.mark.parametrize("H,E,Hp", [(3, 5, 4), (150, 768, 160)])
def test_cnn_weights_fn_gradient_exact(H, E, Hp):
    g = torch.Generator().manual_seed(H + Hp)
    cw, wq, bq = (torch.randn(H, E, 3, generator=g), torch.randn(H, H, generator=g), torch.randn(H, generator=g))
    leaves = [t.cuda().requires_grad_() for t in (cw, wq, bq)]
    outs = F.CNNWeightsFn.apply(*leaves, Hp)
    for got, want in zip(outs, D.pack_reference(cw, wq, bq, Hp)):
        assert torch.equal(got.detach().cpu(), want)
    assert not outs[3].requires_grad
    d3, dq, db = (torch.randn(3 * Hp, E, generator=g), torch.randn(Hp, Hp, generator=g), torch.randn(Hp, generator=g))
    torch.autograd.backward(outs[:3], [d3.cuda(), dq.cuda(), db.cuda()])
    torch.cuda.synchronize()
    for leaf, want in zip(leaves, D.unpack_reference(d3, dq, db, H, E, Hp)):
        assert torch.equal(leaf.grad.cpu(), want)


# ---- nr_unique_rows edges

TILE = 4096           # dedup.hip: SCAN_PER x SCAN_THREADS ids per scan workgroup
TILES_LDS = 256       # dedup.hip: COUNT_TILES_LDS -- more tiles than this: tile totals by global atomics


def _edge_ids(V, T, seed):
    """Random ids over [0, V) plus 0, V - 1 and the ids on both sides of every scan-tile edge."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, V, (T,), generator=g)
    ids[torch.rand(T, generator=g) < 0.2] = V // 2     # one long segment
    forced = [0, V - 1] + [e + d for e in (TILE, 2 * TILE, TILES_LDS * TILE) for d in (-2, -1, 0, 1)]
    forced = [v for v in forced if 0 <= v < V]
    ids[torch.randperm(T, generator=g)[:len(forced)]] = torch.tensor(forced)
    return ids, forced


@pytest.mark.parametrize("V", [4095, 4096, 4097, 8193, TILES_LDS * TILE, TILES_LDS * TILE + 1])
def test_unique_rows_tile_edges(V):
    T = 1500
    ids, forced = _edge_ids(V, T, V)
    ref = D.unique_rows_reference(ids, V)
    assert set(forced) <= set(ref.uids[:ref.counts[0]].tolist())
    ur = K.UniqueRows(ids.cuda(), V)
    _check_unique(ur, ref, T)
    assert K.self_cleaning_check("cuda") == []


@pytest.mark.parametrize("kind,T", [("distinct", 512), ("distinct", 513), ("equal", 512)])
def test_unique_rows_full_count_workgroup(kind, T):
    """512 tokens are one count / fill workgroup: all distinct (every token its own hash entry), one
    more (a second workgroup of one token), all equal (one entry of 512)."""
    V = 700
    g = torch.Generator().manual_seed(T)
    ids = torch.randperm(V, generator=g)[:T] if kind == "distinct" else torch.full((T,), 7, dtype=torch.int64)
    ref = D.unique_rows_reference(ids, V)
    assert ref.counts[0] == (T if kind == "distinct" else 1)
    _check_unique(K.UniqueRows(ids.cuda(), V), ref, T)


def test_unique_rows_fill_row():
    V, T, fill = 4097, 300, 4096
    ids, _ = _edge_ids(V, T, 3)
    ref = D.unique_rows_reference(ids, V, fill)
    U, Up = ref.counts[:2]
    assert U % 32 and (ref.uids[U:] == fill).all()
    _check_unique(K.UniqueRows(ids.cuda(), V, fill_row=fill), ref, T)


@pytest.mark.parametrize("V", [100, 8193])
def test_unique_rows_out_of_range_ids(V):
    """A negative id and one >= V in one batch: flagged once, dropped from the CSR, inv 0 there, and the
    workspace left clean."""
    T = 400
    ids = torch.randint(0, V, (T,), generator=torch.Generator().manual_seed(V))
    ids[17], ids[311] = -3, V + 5
    ref = D.unique_rows_reference(ids, V)
    assert ref.counts[2] == 1 and ref.counts[3] == T - 2
    ur = K.UniqueRows(ids.cuda(), V)
    _check_unique(ur, ref, T)
    assert ur.inv[17].item() == 0 and ur.inv[311].item() == 0
    tok = ur.seg_tok[:T - 2].cpu()
    assert not ((tok == 17) | (tok == 311)).any()
    assert K.self_cleaning_check("cuda") == []
    ids2 = torch.randint(0, V, (T,), generator=torch.Generator().manual_seed(V + 1))   # the next call is exact
    _check_unique(K.UniqueRows(ids2.cuda(), V), D.unique_rows_reference(ids2, V), T)
