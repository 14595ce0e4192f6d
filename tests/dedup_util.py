"""Shared by tests/test_dedup_kernels_gpu.py and tests/test_dedup_ref_cpu.py: plain torch statements
(CPU, float64 / int64) of the distinct-row kernels of csrc/dedup.hip and csrc/conv3_rows.hip, and the
builders of the token batches the kernel tests run on.

Segment geometry.  ``ids_from_lengths`` makes id v occur lens[v] times, so the CSR nr_unique_rows
builds (ascending id order) has seg_off = running sum of the nonzero lens: a case written as a list of
lengths fixes exactly where every segment starts and ends relative to the segment sum's ranges of
SEG_RANGE positions.  ``segment_classes`` names what the two passes of nr_segment_rows_sum do with each
segment; GEOMETRY lists, per case, the classes it is there for, and the CPU test holds every case to
that list, so a case cannot drift off the path it is named for.

Integer data.  ``int_rows`` draws every entry from +-{1..8}: all partial sums of fewer than 2^21 rows
stay below 2^24 in magnitude, so an fp32 sum in any order is exact, the expected result is an integer
tensor and the comparison is an equality.  No entry is zero, so a row left out, added twice or sent to
another segment changes every column of the result."""
import collections

import torch

# csrc/dedup.hip: SEG_RANGE (CSR positions per pass-1 workgroup), FIX_WAVE_PIECES (a cut segment of at
# most this many pieces is summed by one wave of the fix-up pass, a longer one by the whole workgroup),
# FIX_THREADS (the fix-up workgroup: G = FIX_THREADS // (width / 4) thread groups share a long segment)
SEG_RANGE = 64
FIX_WAVE_PIECES = 8
FIX_THREADS = 1024

F64 = torch.float64
U24 = 2.0 ** -24    # fp32 unit roundoff


# ---- builders

def ids_from_lengths(lens, seed):
    """ids [sum(lens)] int64: id v occurs lens[v] times (0: absent), tokens shuffled by a seeded
    permutation."""
    lens = torch.as_tensor(lens, dtype=torch.int64)
    ids = torch.repeat_interleave(torch.arange(lens.numel()), lens)
    return ids[torch.randperm(ids.numel(), generator=torch.Generator().manual_seed(seed))]


def int_rows(T, W, seed):
    """float32 [T, W], entries from +-{1, ..., 8}, never zero."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.randint(1, 9, (T, W), generator=g)
    sign = torch.randint(0, 2, (T, W), generator=g) * 2 - 1
    return (mag * sign).float()


# ---- nr_unique_rows

UniqueRef = collections.namedtuple("UniqueRef", "uids inv seg_off segs counts")


def unique_rows_reference(ids, V, fill_row=0, grad_mask=None):
    """uids [U_pad] (ascending distinct ids, then fill_row), inv [T] (0 at an out-of-range id), seg_off
    [U_pad + 1], segs: per distinct row the ascending tokens with grad_mask set (all without a mask),
    counts = (U, U_pad, bad, T_csr).  Ids outside [0, V) are counted as bad and dropped."""
    ids = ids.cpu().long()
    T = ids.numel()
    ok = (ids >= 0) & (ids < V)
    on = ok if grad_mask is None else ok & (grad_mask.cpu().reshape(-1) != 0)
    present = torch.zeros(V, dtype=torch.bool)
    present[ids[ok]] = True
    distinct = torch.nonzero(present).reshape(-1)
    U = distinct.numel()
    U_pad = (U + 31) // 32 * 32
    pos = torch.cumsum(present.long(), 0) - 1
    inv = torch.zeros(T, dtype=torch.int64)
    inv[ok] = pos[ids[ok]]
    uids = torch.full((U_pad,), fill_row, dtype=torch.int64)
    uids[:U] = distinct
    tok = torch.nonzero(on).reshape(-1)
    rows = inv[tok]
    segs = [tok[rows == u] for u in range(U)]
    seg_off = torch.zeros(U_pad + 1, dtype=torch.int64)
    for u in range(U):
        seg_off[u + 1] = seg_off[u] + segs[u].numel()
    seg_off[U:] = tok.numel()
    return UniqueRef(uids, inv, seg_off, segs, (U, U_pad, int((~ok).sum() > 0), tok.numel()))


# ---- segment sums

def segment_sum_reference(src, ref, dtype=F64):
    """[U_pad, W]: row u = sum of src[t] over ref.segs[u]; empty and pad rows zero.  dtype float64, or
    int64 for integer data."""
    src = src.cpu().to(dtype)
    out = torch.zeros(ref.counts[1], src.shape[1], dtype=dtype)
    for u, toks in enumerate(ref.segs):
        if toks.numel():
            out[u] = src[toks].sum(0)
    return out


def segment_sum_conv3_reference(src, L, ref, dtype=F64):
    """[U_pad, 3 * tw], src [T, tw]: column block `tap` of row u = sum over the tokens t of ref.segs[u]
    of src[t + 1 - tap], for the t whose title (L consecutive tokens) holds row t + 1 - tap."""
    src = src.cpu().to(dtype)
    tw = src.shape[1]
    out = torch.zeros(ref.counts[1], 3 * tw, dtype=dtype)
    for u, toks in enumerate(ref.segs):
        for tap in range(3):
            p = toks % L + 1 - tap
            r = (toks + 1 - tap)[(p >= 0) & (p < L)]
            if r.numel():
                out[u, tap * tw:(tap + 1) * tw] = src[r].sum(0)
    return out


# ---- nr_conv3_rows_fwd

def conv3_rows_reference(P, inv, L, bias, H, relu):
    """[T, tw] float64, P [U, 3 * tw]: out[t][:H] = act(bias + sum_j P[inv[t + j - 1]][j * tw : j * tw + H])
    over the taps j whose token t + j - 1 lies in t's title; out[t][H:] = 0.  Differentiable in P."""
    P = P.to(F64)
    inv = inv.cpu().long()
    T, tw = inv.numel(), P.shape[1] // 3
    t = torch.arange(T)
    acc = torch.zeros(T, H, dtype=F64)
    for j in range(3):
        p = t % L + j - 1
        ok = (p >= 0) & (p < L)
        rows = inv[(t + j - 1).clamp(0, T - 1)]
        acc = acc + torch.where(ok[:, None], P[rows, j * tw:j * tw + H], torch.zeros((), dtype=F64))
    if bias is not None:
        acc = acc + bias.to(F64)[:H]
    if relu:
        acc = acc.clamp_min(0)
    return torch.cat([acc, torch.zeros(T, tw - H, dtype=F64)], 1)


def conv3_rows_abs_reference(P, inv, L, bias, H):
    """|bias| + sum of the |terms| of conv3_rows_reference's [:, :H]: the error bound's magnitude."""
    return conv3_rows_reference(P.abs(), inv, L, None if bias is None else bias.abs(), H, False)[:, :H]


# ---- nr_cnn_pack_weights / nr_cnn_unpack_grads

def pack_reference(cw, wq, bq, Hp):
    """conv weight [H, E, 3], key projection [H, H] / [H] -> w3t [3 Hp, E] (row tap * Hp + h), wqp
    [Hp, Hp], bqp [Hp] zero-padded, w3tt [E, 3 Hp] = w3t transposed."""
    H, E, _ = cw.shape
    w3t = torch.zeros(3 * Hp, E, dtype=cw.dtype)
    wqp = torch.zeros(Hp, Hp, dtype=cw.dtype)
    bqp = torch.zeros(Hp, dtype=cw.dtype)
    for tap in range(3):
        for h in range(H):
            w3t[tap * Hp + h] = cw[h, :, tap]
    for r in range(H):
        wqp[r, :H] = wq[r]
    bqp[:H] = bq
    w3tt = torch.zeros(E, 3 * Hp, dtype=cw.dtype)
    for e in range(E):
        w3tt[e] = w3t[:, e]
    return w3t, wqp, bqp, w3tt


def unpack_reference(dw3t, dwqp, dbqp, H, E, Hp):
    """The gradients of pack_reference's inputs from those of w3t / wqp / bqp."""
    dcw = torch.zeros(H, E, 3, dtype=dw3t.dtype)
    for tap in range(3):
        for h in range(H):
            dcw[h, :, tap] = dw3t[tap * Hp + h]
    return dcw, dwqp[:H, :H].clone(), dbqp[:H].clone()


# ---- what the segment sum does with each segment

Seg = collections.namedtuple("Seg", "cls slot pieces start end")


def segment_classes(seg_off):
    """Per segment of a CSR (seg_off [n + 1]): cls = empty | single (one token) | whole (inside one
    range: stored by pass 1) | cut_wave (cut by a range boundary, at most FIX_WAVE_PIECES pieces) |
    cut_block (more); slot: the per-range scratch slot of its first piece (0: the segment starts at or
    before the range's first position, 1: inside the range); pieces: the ranges it touches."""
    off = [int(x) for x in seg_off]
    out = []
    for sb, se in zip(off[:-1], off[1:]):
        if se == sb:
            out.append(Seg("empty", 0, 0, sb, se))
            continue
        b0, b1 = sb // SEG_RANGE, (se - 1) // SEG_RANGE
        pieces = b1 - b0 + 1
        slot = 1 if sb > b0 * SEG_RANGE else 0
        if se - sb == 1:
            cls = "single"
        elif pieces == 1:
            cls = "whole"
        else:
            cls = "cut_wave" if pieces <= FIX_WAVE_PIECES else "cut_block"
        out.append(Seg(cls, slot, pieces, sb, se))
    return out


def has_class(segs, cls, slot=None, pieces=None, end_aligned=None, fills_range=None):
    """Some segment of `segs` (segment_classes) is of class cls with, where given, that first-piece slot,
    that number of pieces, its end on (off) a range boundary, its extent exactly one whole range."""
    for s in segs:
        if s.cls != cls:
            continue
        if slot is not None and s.slot != slot:
            continue
        if pieces is not None and s.pieces != pieces:
            continue
        if end_aligned is not None and (s.end % SEG_RANGE == 0) != end_aligned:
            continue
        if fills_range is not None and (s.start % SEG_RANGE == 0 and s.end - s.start == SEG_RANGE) != fills_range:
            continue
        return True
    return False


def single_only_ranges(segs):
    """The ranges whose every position belongs to a one-token segment (nr_segment_rows_sum_multi drops
    all of them: the range's workgroup has nothing to sum)."""
    T = segs[-1].end if segs else 0
    mixed = set()
    for s in segs:
        if s.cls not in ("single", "empty"):
            mixed.update(range(s.start // SEG_RANGE, (s.end - 1) // SEG_RANGE + 1))
    return [b for b in range((T + SEG_RANGE - 1) // SEG_RANGE) if b not in mixed]


def _sparse_lens():
    # a whole range of one-token ids with absent ids between them, then lengths 1..97 with every third
    # id absent
    return [1, 0] * 70 + [((i * 37) % 97 + 1) if i % 3 else 0 for i in range(60)]


# case -> (segment lengths by id, trailing absent ids, the classes the case is there for as has_class
# keyword sets).  The pieces of the long cases are 8 G, 8 G + 1, 8 G + 2 and 17 G + 2 for G = 1 and G = 3
# thread groups (widths of 1024 float4 and more, and the step's 288): the fix-up's whole-workgroup path
# gives group g the pieces g, g + G, ... -- the first on its own, then eight at a time, then one by one.
GEOMETRY = {
    "aligned": ([64, 64, 128, 1, 63, 64], 3, [
        dict(cls="whole", slot=0, fills_range=True),
        dict(cls="cut_wave", slot=0, pieces=2, end_aligned=True),
        dict(cls="single", slot=0),
        dict(cls="whole", slot=1, end_aligned=True)]),
    "offset": ([1, 64, 63, 65, 127, 2, 130, 7], 5, [
        dict(cls="single"),
        dict(cls="cut_wave", slot=1, pieces=2, end_aligned=False),
        dict(cls="whole", slot=1, end_aligned=True),
        dict(cls="cut_wave", slot=0, pieces=2, end_aligned=False),
        dict(cls="cut_wave", slot=1, pieces=2, end_aligned=True),
        dict(cls="cut_wave", slot=1, pieces=3)]),
    "wave_block": ([512, 513, 62, 450, 449, 5, 1], 1, [
        dict(cls="single"),
        dict(cls="cut_wave", slot=0, pieces=8),
        dict(cls="cut_block", slot=0, pieces=9),
        dict(cls="cut_block", slot=1, pieces=9),
        dict(cls="cut_wave", slot=1, pieces=8)]),
    "long_g1": ([8 * 64, 9 * 64, 10 * 64, 33, 15 * 64 + 2, 18 * 64, 3, 1], 2, [
        dict(cls="single"),
        dict(cls="cut_wave", slot=0, pieces=8),
        dict(cls="cut_block", slot=0, pieces=9),
        dict(cls="cut_block", slot=0, pieces=10),
        dict(cls="cut_block", slot=1, pieces=16),
        dict(cls="cut_block", slot=1, pieces=19)]),
    "long_g3": ([24 * 64, 25 * 64, 10, 25 * 64 - 8, 52 * 64, 5, 1], 7, [
        dict(cls="single"),
        dict(cls="cut_block", slot=0, pieces=24),
        dict(cls="cut_block", slot=0, pieces=25),
        dict(cls="cut_block", slot=1, pieces=26),
        dict(cls="cut_block", slot=1, pieces=53)]),
    "sparse": (_sparse_lens(), 9, [
        dict(cls="single"),
        dict(cls="whole"),
        dict(cls="cut_wave", slot=1)]),
}

Case = collections.namedtuple("Case", "name lens V ids ref segs needs")
_CASES = {}


def geometry_case(name):
    """The case built once per process: ids (shuffled), V, the reference CSR, its segment classes."""
    if name not in _CASES:
        lens, absent, needs = GEOMETRY[name]
        lens = list(lens) + [0] * absent
        ids = ids_from_lengths(lens, seed=sum(ord(c) for c in name))
        ref = unique_rows_reference(ids, len(lens))
        segs = segment_classes(ref.seg_off[:ref.counts[0] + 1])
        _CASES[name] = Case(name, lens, len(lens), ids, ref, segs, needs)
    return _CASES[name]


def masked_case():
    """ids and a 0/1 grad_mask (int64): ids 2 and 5 occur without any gradient-carrying token (empty
    segments between non-empty ones), the others lose a part of their tokens; one segment stays cut by
    several ranges, one keeps a single token."""
    lens = [300, 40, 9, 1, 0, 17, 130, 3, 0, 0, 66]
    ids = ids_from_lengths(lens, seed=77)
    gm = (torch.rand(ids.numel(), generator=torch.Generator().manual_seed(78)) < 0.7).long()
    gm[(ids == 2) | (ids == 5)] = 0
    gm[ids == 3] = 1
    first7 = torch.nonzero(ids == 7).reshape(-1)
    gm[first7] = 0
    gm[first7[0]] = 1
    return ids, len(lens), gm


def sum_bound(n, abs_sum):
    """2 n 2^-24 sum|x_i|: (n - 1) u sum|x_i| bounds an fp32 sum of n terms in any order to first order
    in u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4); the factor 2 covers
    the higher-order terms."""
    return 2.0 * n * U24 * abs_sum
