"""The references and case builders of tests/dedup_util.py held against independent statements of the
same operations (numpy, index_add_, autograd, conv1d, permute / pad), and every segment-geometry case
held to the classes it is named for -- all without a GPU, so that tests/test_dedup_kernels_gpu.py
compares the kernels with something already checked."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dedup_util as D

F64 = torch.float64


def _random_ids(T, V, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, V, (T,), generator=g)
    ids[torch.rand(T, generator=g) < 0.3] = 0
    return ids


# ---- ids_from_lengths / unique_rows_reference

def test_ids_from_lengths_fixes_the_csr():
    lens = [3, 0, 1, 70, 0, 0, 2]
    ids = D.ids_from_lengths(lens, seed=1)
    assert torch.equal(torch.bincount(ids, minlength=len(lens)), torch.tensor(lens))
    assert not torch.equal(ids, torch.sort(ids).values)   # shuffled
    assert torch.equal(ids, D.ids_from_lengths(lens, seed=1))
    ref = D.unique_rows_reference(ids, len(lens))
    assert ref.seg_off[:5].tolist() == [0, 3, 4, 74, 76]
    assert ref.counts == (4, 32, 0, 76) and ref.seg_off[4:].tolist() == [76] * 29


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("T,V,fill", [(1, 5, 0), (500, 37, 3), (3000, 5000, 11)])
def test_unique_rows_reference_vs_numpy(T, V, fill, masked):
    ids = _random_ids(T, V, T + V)
    gm = (torch.rand(T, generator=torch.Generator().manual_seed(9)) < 0.6) if masked else None
    ref = D.unique_rows_reference(ids, V, fill, gm)
    want, winv = np.unique(ids.numpy(), return_inverse=True)
    U, Up, bad, Tc = ref.counts
    assert (U, Up, bad) == (len(want), (len(want) + 31) // 32 * 32, 0)
    assert Tc == (T if gm is None else int(gm.sum()))
    assert (ref.uids[:U].numpy() == want).all() and (ref.uids[U:] == fill).all()
    assert (ref.inv.numpy() == winv.reshape(-1)).all()
    on = np.ones(T, bool) if gm is None else gm.numpy()
    for u in range(U):
        assert (ref.segs[u].numpy() == np.nonzero((ids.numpy() == want[u]) & on)[0]).all()
        assert int(ref.seg_off[u + 1] - ref.seg_off[u]) == ref.segs[u].numel()
    assert int(ref.seg_off[0]) == 0 and (ref.seg_off[U:] == Tc).all()


def test_unique_rows_reference_drops_out_of_range_ids():
    ids = torch.tensor([4, -1, 2, 9, 2, 7])
    ref = D.unique_rows_reference(ids, 8)
    assert ref.counts == (3, 32, 1, 4)
    assert ref.uids[:3].tolist() == [2, 4, 7] and ref.inv.tolist() == [1, 0, 0, 0, 0, 2]
    assert [s.tolist() for s in ref.segs] == [[2, 4], [0], [5]]


# ---- the sums

@pytest.mark.parametrize("masked", [False, True])
def test_segment_sum_reference_vs_index_add(masked):
    T, V, W = 700, 40, 12
    ids = _random_ids(T, V, 3)
    gm = (torch.rand(T, generator=torch.Generator().manual_seed(4)) < 0.5) if masked else None
    ref = D.unique_rows_reference(ids, V, 0, gm)
    src = torch.randn(T, W, generator=torch.Generator().manual_seed(5), dtype=F64)
    on = torch.ones(T, dtype=torch.bool) if gm is None else gm
    want = torch.zeros(ref.counts[1], W, dtype=F64).index_add_(0, ref.inv[on], src[on])
    torch.testing.assert_close(D.segment_sum_reference(src, ref), want, rtol=1e-13, atol=1e-13)
    rows = D.int_rows(T, W, 6)
    wanti = torch.zeros(ref.counts[1], W, dtype=torch.int64).index_add_(0, ref.inv[on], rows[on].long())
    got = D.segment_sum_reference(rows, ref, torch.int64)
    assert got.dtype == torch.int64 and torch.equal(got, wanti)


@pytest.mark.parametrize("L", [1, 2, 3, 30])
def test_segment_sum_conv3_reference_is_the_conv_gradient(L):
    """d/dP of sum <dC, conv3_rows_reference(P, inv, relu off, no bias)> by float64 autograd."""
    n, V, tw = 12, 9, 8
    T = n * L
    ids = _random_ids(T, V, 20 + L)
    ref = D.unique_rows_reference(ids, V)
    g = torch.Generator().manual_seed(L)
    P = torch.randn(ref.counts[1], 3 * tw, generator=g, dtype=F64, requires_grad=True)
    dC = torch.randn(T, tw, generator=g, dtype=F64)
    (D.conv3_rows_reference(P, ref.inv, L, None, tw, False) * dC).sum().backward()
    torch.testing.assert_close(D.segment_sum_conv3_reference(dC, L, ref), P.grad, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("L,E,H,tw", [(1, 5, 4, 4), (2, 3, 1, 4), (30, 7, 25, 32), (5, 6, 8, 8)])
def test_conv3_rows_reference_vs_conv1d(L, E, H, tw, relu):
    n, U = 6, 11
    T = n * L
    g = torch.Generator().manual_seed(L * 100 + H)
    X = torch.randn(U, E, generator=g, dtype=F64)
    Wc = torch.randn(H, E, 3, generator=g, dtype=F64)
    bias = torch.randn(H, generator=g, dtype=F64)
    inv = torch.randint(0, U, (T,), generator=g)
    P = torch.zeros(U, 3 * tw, dtype=F64)
    for j in range(3):
        P[:, j * tw:j * tw + H] = X @ Wc[:, :, j].t()
    want = F.conv1d(X[inv].view(n, L, E).transpose(1, 2), Wc, bias, padding=1).transpose(1, 2).reshape(T, H)
    if relu:
        want = want.clamp_min(0)
    got = D.conv3_rows_reference(P, inv, L, bias, H, relu)
    assert got.shape == (T, tw) and (got[:, H:] == 0).all()
    torch.testing.assert_close(got[:, :H], want, rtol=1e-12, atol=1e-12)
    nobias = D.conv3_rows_reference(P, inv, L, None, H, False)
    torch.testing.assert_close(nobias[:, :H] + bias, D.conv3_rows_reference(P, inv, L, bias, H, False)[:, :H],
                               rtol=1e-12, atol=1e-12)
    mag = D.conv3_rows_abs_reference(P, inv, L, bias, H)
    assert (mag >= got[:, :H].abs() - 1e-12).all()


# ---- pack / unpack

@pytest.mark.parametrize("H,E,Hp", [(1, 1, 1), (3, 5, 4), (20, 64, 32)])
def test_pack_unpack_reference_vs_permute_and_pad(H, E, Hp):
    g = torch.Generator().manual_seed(H + E)
    cw, wq, bq = (torch.randn(H, E, 3, generator=g), torch.randn(H, H, generator=g), torch.randn(H, generator=g))
    w3t, wqp, bqp, w3tt = D.pack_reference(cw, wq, bq, Hp)
    want3 = F.pad(cw.permute(2, 0, 1), (0, 0, 0, Hp - H)).reshape(3 * Hp, E)
    assert torch.equal(w3t, want3) and torch.equal(w3tt, want3.t())
    assert torch.equal(wqp, F.pad(wq, (0, Hp - H, 0, Hp - H))) and torch.equal(bqp, F.pad(bq, (0, Hp - H)))
    for got, want in zip(D.unpack_reference(w3t, wqp, bqp, H, E, Hp), (cw, wq, bq)):
        assert torch.equal(got, want)   # the round trip
    d3, dq, db = (torch.randn(3 * Hp, E, generator=g), torch.randn(Hp, Hp, generator=g), torch.randn(Hp, generator=g))
    dcw, dwq, dbq = D.unpack_reference(d3, dq, db, H, E, Hp)
    assert torch.equal(dcw, d3.view(3, Hp, E)[:, :H].permute(1, 2, 0))
    assert torch.equal(dwq, dq[:H, :H]) and torch.equal(dbq, db[:H])


# ---- segment classes and the geometry cases

def test_segment_classes_by_hand():
    R = D.SEG_RANGE
    off = [0, 0, 1, R, R + 2, 3 * R, 3 * R + 1, 11 * R, 11 * R + 1, 20 * R + 2]
    segs = D.segment_classes(off)
    assert [s.cls for s in segs] == ["empty", "single", "whole", "whole", "cut_wave", "single", "cut_wave",
                                     "single", "cut_block"]
    assert [s.slot for s in segs][1:] == [0, 1, 0, 1, 0, 1, 0, 1]
    assert [s.pieces for s in segs] == [0, 1, 1, 1, 2, 1, D.FIX_WAVE_PIECES, 1, D.FIX_WAVE_PIECES + 2]
    assert D.has_class(segs, "cut_wave", slot=1, pieces=8) and not D.has_class(segs, "cut_wave", slot=0, pieces=8)
    assert D.has_class(segs, "cut_wave", end_aligned=True) and not D.has_class(segs, "cut_wave", end_aligned=False)
    assert D.has_class(segs, "cut_block", end_aligned=False)
    assert not D.has_class(segs, "whole", fills_range=True)
    assert D.single_only_ranges(D.segment_classes([0, 1, 2] + [2 + R])) == []
    assert D.single_only_ranges(D.segment_classes(list(range(R + 1)) + [2 * R + 5])) == [0]


@pytest.mark.parametrize("name", sorted(D.GEOMETRY))
def test_geometry_case_contains_its_classes(name):
    c = D.geometry_case(name)
    present = [n for n in c.lens if n]
    assert [s.end - s.start for s in c.segs] == present   # the CSR is the running sum of the lengths
    assert c.ref.counts[0] == len(present) and c.ref.counts[3] == sum(present) == c.ids.numel()
    for need in c.needs:
        assert D.has_class(c.segs, **need), (name, need)
    assert c.V % 16 and c.ref.counts[0] < c.V    # absent ids; V off the zero fill's 16 rows a workgroup


def test_long_cases_cover_both_sides_of_the_unrolled_loop():
    """Whole-workgroup path: group g of G sums the pieces g, g + G, ...: the segment's first piece on
    its own (group 0), then 8 at a time while 8 remain, then the tail one by one.  Over the long
    segments of a case some group must run the tail alone (G = 3 only: with one group the path starts
    at 9 pieces), the unrolled loop alone, both, and the unrolled loop twice."""
    def trips(pieces, G, g):
        mine = len(range(g, pieces, G)) - (1 if g == 0 else 0)
        return mine // 8, mine % 8

    for name, G in (("long_g1", 1), ("long_g3", 3)):
        pieces = {s.pieces for s in D.geometry_case(name).segs if s.cls == "cut_block"}
        assert {8 * G + 1, 8 * G + 2, 17 * G + 2} <= pieces and 8 * G in {s.pieces for s in D.geometry_case(name).segs}
        seen = {trips(p, G, g) for p in pieces for g in range(G)}
        assert G == 1 or any(u == 0 and t > 0 for u, t in seen)
        assert any(u == 1 and t == 0 for u, t in seen) and any(u == 1 and t > 0 for u, t in seen)
        assert any(u == 2 and t > 0 for u, t in seen)
    assert D.FIX_THREADS // (1152 // 4) == 3 and D.FIX_THREADS // (4096 // 4) == 1


def test_sparse_case_edges():
    c = D.geometry_case("sparse")
    U, Up, _, T = c.ref.counts
    assert U % 32 and Up > U and T % D.SEG_RANGE and c.segs[-1].end == T
    assert 0 in D.single_only_ranges(c.segs)
    absent_between = [v for v in range(int(c.ref.uids[U - 1])) if c.lens[v] == 0]
    assert absent_between


def test_masked_case_has_empty_segments():
    ids, V, gm = D.masked_case()
    ref = D.unique_rows_reference(ids, V, 0, gm)
    segs = D.segment_classes(ref.seg_off[:ref.counts[0] + 1])
    assert ref.counts[3] == int(gm.sum()) < ids.numel()
    empties = [u for u, s in enumerate(segs) if s.cls == "empty"]
    assert len(empties) == 2 and all(0 < u < len(segs) - 1 for u in empties)
    assert D.has_class(segs, "single") and D.has_class(segs, "cut_wave") and D.has_class(segs, "whole")
    assert ref.counts[0] == len(np.unique(ids.numpy()))   # distinctness ignores the mask


# ---- integer rows

def test_int_rows_make_every_token_count():
    rows = D.int_rows(500, 16, 2)
    assert rows.dtype == torch.float32 and rows.abs().min() >= 1 and rows.abs().max() <= 8
    assert torch.equal(rows, rows.round()) and (rows < 0).any() and (rows > 0).any()
    assert 8 * 2 ** 21 <= 2 ** 24     # sums of fewer than 2^21 rows are exact in fp32
    c = D.geometry_case("offset")
    src = D.int_rows(c.ids.numel(), 8, 3)
    full = D.segment_sum_reference(src, c.ref, torch.int64)
    for u, toks in enumerate(c.ref.segs):
        if toks.numel() < 2:
            continue
        for t in toks.tolist():   # the segment without token t, with token t doubled: every column differs
            assert ((full[u] - src[t].long()) != full[u]).all() and ((full[u] + src[t].long()) != full[u]).all()


def test_sum_bound():
    assert D.sum_bound(4, 3.0) == 2 * 4 * 2.0 ** -24 * 3.0
