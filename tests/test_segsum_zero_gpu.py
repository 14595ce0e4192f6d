"""nr_segment_rows_sum_multi_zero (the zero fill of the absent table rows inside the segment sum's
fix-up launch) against the two launches it replaces: nr_segment_rows_sum_multi followed by
nr_unique_rows_zero_absent on the same distinct-row workspace.  Every output -- the per-distinct-row
sums, the zero-filled matrix, Adam's row flags -- and the workspace itself must be bit-for-bit what
the two calls leave; outputs are NaN-prefilled and over-wide, so a row or column that must not be
written shows."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from newsrec_amd import kernels as K

NAN = float("nan")


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _ids(V, T, kind, gen):
    if kind == "all_absent":
        return torch.zeros(0, dtype=torch.int64)
    if kind == "random":
        ids = torch.randint(0, V, (T,), generator=gen)
        ids[: min(T, 5)] = 0   # the pad id occurs (its row is zeroed all the same)
        return ids
    # every id present: no row is absent; "pad_only" zeroes the pad row, "all_present" has no pad row
    assert T >= V
    return torch.cat([torch.arange(V), torch.randint(0, V, (T - V,), generator=gen)])[torch.randperm(T, generator=gen)]


def _cases():
    out = []
    for V in (100, 17):        # 17: fewer rows than two zero-fill workgroups take (2 x 16)
        for T in (0, 64, 200):
            kinds = ["all_absent"] if T == 0 else ["random"] + (["all_present", "pad_only"] if T >= V else [])
            out += [(V, T, k) for k in kinds]
    out.append((5000, 3000, "random"))   # several workgroups of each role: 12 fix-up, 313 zero-fill
    return out


@pytest.mark.parametrize("with_flags", [True, False])
@pytest.mark.parametrize("W", [8, 1152])
@pytest.mark.parametrize("V,T,kind", _cases())
def test_fused_zero_fill_equals_the_two_calls(V, T, kind, W, with_flags):
    gen = torch.Generator().manual_seed(V * 1000 + T + W)
    ids = _ids(V, T, kind, gen).cuda()
    T = ids.numel()
    pad_row = -1 if kind == "all_present" else 0
    gm = (torch.rand(T, generator=gen) < 0.7).long().cuda() if T else None
    ur = K.UniqueRows(ids, V, fill_row=0, grad_mask=gm)
    src = torch.randn(max(T, 1), W, generator=gen).cuda()

    def run(fused):
        dst = torch.full((ur.cap, W + 4), NAN, device="cuda")
        z = torch.full((V, W + 4), NAN, device="cuda")
        flags = torch.full((V,), 0xAB, dtype=torch.uint8, device="cuda") if with_flags else None
        if fused:
            assert ur.segment_sum_multi_zero(src, dst[:, :W], z[:, :W], pad_row, flags) is True
        else:
            ur.segment_sum_multi(src, dst[:, :W])
            assert ur.zero_absent_rows(z[:, :W], pad_row, flags) is True
        torch.cuda.synchronize()
        return dst, z, flags, ur._work.clone(), ur.counts.clone()

    a, b = run(False), run(True)
    assert torch.equal(_bits(a[0]), _bits(b[0]))      # the sums (one-token rows stay NaN in both)
    assert torch.equal(_bits(a[1]), _bits(b[1]))      # the zero-filled matrix
    if with_flags:
        assert torch.equal(a[2], b[2])
    assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])   # the distinct-row workspace, the counts

    # and against the definition: absent rows and the pad row zero, present rows and the columns past
    # the width untouched; flags 1 for a present row
    present = torch.zeros(V, dtype=torch.bool)
    present[ids.cpu()] = True
    if pad_row >= 0:
        present[pad_row] = False
    z = b[1].cpu()
    assert torch.isnan(z[present]).all() and torch.isnan(z[:, W:]).all()
    assert (z[~present][:, :W] == 0.0).all()
    if kind in ("all_present", "pad_only"):
        assert int((~present).sum()) == (0 if kind == "all_present" else 1)
    if kind == "all_absent":
        assert not present.any()
    if with_flags:
        assert torch.equal(b[2].cpu(), present.to(torch.uint8))
    # the sums' own columns past the width are untouched too
    assert torch.isnan(b[0][:, W:]).all()


def test_replaced_scan_falls_back_to_the_plain_calls():
    """After another nr_unique_rows call on the vocabulary the presence scan is gone: the fused method
    runs the plain segment sum and the full zero fill, and says so as zero_absent_rows does."""
    g = torch.Generator().manual_seed(2)
    V, T, W = 300, 500, 64
    ids = torch.randint(0, V, (T,), generator=g).cuda()
    ur = K.UniqueRows(ids, V)
    src = torch.randn(T, W, generator=g).cuda()
    want = torch.full((ur.cap, W), NAN, device="cuda")
    ur.segment_sum_multi(src, want)
    K.UniqueRows(ids[:50].contiguous(), V)
    dst = torch.full((ur.cap, W), NAN, device="cuda")
    z = torch.full((V, W), NAN, device="cuda")
    assert ur.segment_sum_multi_zero(src, dst, z, 0) is False
    torch.cuda.synchronize()
    assert torch.equal(_bits(dst), _bits(want)) and (z == 0.0).all()


def test_bad_arguments_are_refused_before_any_launch():
    from newsrec_amd import _lib as L
    g = torch.Generator().manual_seed(3)
    V, T, W = 64, 100, 8
    ids = torch.randint(0, V, (T,), generator=g).cuda()
    ur = K.UniqueRows(ids, V)
    src = torch.randn(T, W, generator=g).cuda()
    dst = torch.full((ur.cap, W), NAN, device="cuda")
    z = torch.full((V, 6), NAN, device="cuda")   # width 6: not a multiple of 4
    with pytest.raises(L.HipError, match="invalid argument 0"):
        ur.segment_sum_multi_zero(src, dst, z, 0)
    torch.cuda.synchronize()
    assert torch.isnan(dst).all() and torch.isnan(z).all()
