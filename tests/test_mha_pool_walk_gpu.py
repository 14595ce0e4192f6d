"""The persistent title walk of the split backward's head pass (mha_head_bwd_kernel, csrc/mha_pool.hip):
grid.x is capped at S = nr_mha_pool_walk_workgroups(2, ...) workgroups per head group, workgroup b walks
titles b, b + S, ..., and each title's index data (row offsets through yrows, dy offsets, mask bits) is
fetched one title ahead, clamped at the last title.

Title counts are chosen around S on the running device (the ids name them symbolically: the module is
collected without a GPU too): 1, 2, S - 1, S (one title per workgroup, the prefetch clamped at once),
S + 1 (one workgroup walks a second title), 2 S + 3 (three titles for a few).  The instantiated NRMS
geometry only: 12 heads, dk 64, dv 32.

Helpers, references and bars are those of tests/test_mha_pool_gpu.py: every output against the float64
statement of tests/pool_util.py at 32 e32 + 32 * 2^-24 * max|ref64| (that module's docstring), the NaN
padding / exact-zero checks of its check_fwd_layout / check_bwd.  The float64 reference and the forward
of a case are computed once and shared by the tests that use the case.

Unchanged arithmetic: dy (no atomics in it) of a title is bit for bit the same wherever in a walk the
title falls, and the same as when it runs as the only title of its workgroup
(test_walked_titles_match_single_titles_bitwise).
"""
import functools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import restatement as R
from pool_util import mha_pool_inputs, mha_pool_reference

import test_mha_pool_gpu as T

F64, F32 = T.F64, T.F32
HEADS, DK, DV = T.GEOMS["h12k64v32"]
COUNTS = ["1", "2", "S-1", "S", "S+1", "2S+3"]


@functools.lru_cache(maxsize=None)
def walk_cap():
    """S: the head pass's grid.x cap on this device."""
    from newsrec_amd import _lib as L
    s = L.load().nr_mha_pool_walk_workgroups(2, HEADS, DK, DV, L.GEMM_F32)
    assert s >= 1, "nr_mha_pool_walk_workgroups: %d" % s
    return s


def count(name):
    s = walk_cap()
    return {"1": 1, "2": 2, "S-1": max(s - 1, 1), "S": s, "S+1": s + 1, "S+2": s + 2, "2S+3": 2 * s + 3}[name]


def walk_mask(n, L):
    """Title 0 fully masked (check_fwd_layout wants it), seeded prefix lengths 1..L after it (trailing
    zeros), every third title with a hole at slot 1 (interior zeros) and one whose only token is the
    last slot."""
    g = torch.Generator().manual_seed(1000 * L + n)
    lens = torch.randint(1, L + 1, (n,), generator=g)
    m = (torch.arange(L)[None] < lens[:, None]).to(torch.int64)
    m[0] = 0
    if L > 2:
        m[1::3, 1] = 0
    if n > 2:
        m[2] = 0
        m[2, L - 1] = 1
    return m


@functools.lru_cache(maxsize=None)
def case(nname, L, p_drop, with_dz, rows_div=0):
    """T.make_case with a title count and mask of this module's: the namespace T.run_fwd / T.run_bwd /
    T.check_* take.  rows_div: y is a table of T // rows_div rows read through a seeded yrows with
    repeats."""
    n = count(nname)
    mask = walk_mask(n, L)
    H, Tn = HEADS * DV, n * L
    rows = max(Tn // rows_div, 1) if rows_div else None
    inp = mha_pool_inputs(n, L, HEADS, DK, DV, 7 * L + n + int(10 * p_drop), rows=rows)
    yrows = torch.randint(0, rows, (Tn,), generator=torch.Generator().manual_seed(L + n)) if rows else None
    return finish_case(n, L, p_drop, with_dz, mask, inp, yrows, "walk-n%s-L%d-p%s" % (nname, L, p_drop))


def finish_case(n, L, p_drop, with_dz, mask, inp, yrows, tag, seed=T.SEED, offset=T.OFFSET):
    H, Tn = HEADS * DV, n * L
    keep = R.dropout_keep(seed, offset, Tn, H, p_drop) if p_drop > 0 else None
    y_tok = inp["y"] if yrows is None else inp["y"][yrows]
    ref = {dt: mha_pool_reference(y_tok, mask, HEADS, DK, DV, inp["gamma"], inp["beta"], inp["q"], keep, p_drop,
                                  dnews=inp["dnews"], dz=inp["dz"] if with_dz else None, dtype=dt)
           for dt in (F64, F32)}
    return types.SimpleNamespace(geom="h12k64v32", heads=HEADS, dk=DK, dv=DV, L=L, n=n, T=Tn, H=H,
                                 NY=HEADS * (DK + DV), p_drop=p_drop, with_dz=with_dz, mask=mask, inp=inp,
                                 keep=keep, ref=ref, yrows=yrows, tag=tag)


@functools.lru_cache(maxsize=None)
def fwd(key):
    return T.run_fwd(case(*key), "f32")


@pytest.fixture(scope="module", autouse=True)
def _leave_no_blocks_behind():
    """As tests/test_mha_pool_gpu.py: later modules see the caching allocator as without this one."""
    T.FORMS.setdefault("split_ws1", (True, True, 1))     # one copy: every workgroup's atomics on one vector
    yield
    fwd.cache_clear()
    case.cache_clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _check(c, f, forms, what):
    T.check_fwd_layout(c, f)
    late = []
    T.compare(c, what + "-fwd", T.fwd_pairs(c, f), late)
    for form in forms:
        T.check_bwd(c, T.run_bwd(c, f, form), what + "-" + form, late)
    assert not late, "; ".join(late)


# ---------------------------------------------------------------------- title counts around the walk

@pytest.mark.parametrize("L,p_drop", [(3, 0.2), (2, 0.0)], ids=["L3-p0.2", "L2-p0"])
@pytest.mark.parametrize("nname", COUNTS)
def test_title_counts(nname, L, p_drop):
    """The forward and the split backward (plain, 1 and 32 gradient copies) at each title count; dz
    rides with the dropout case."""
    key = (nname, L, p_drop, p_drop > 0)
    _check(case(*key), fwd(key), ["split", "split_ws1", "split_ws32"], "counts")


# ---------------------------------------------------------------------- token geometry under the walk

@pytest.mark.parametrize("L,p_drop,form", [(1, 0.2, "split_ws32"), (7, 0.0, "split_ws1"), (30, 0.2, "split_ws1"),
                                           (32, 0.0, "split_ws32")],
                         ids=["L1", "L7", "L30", "L32"])
def test_token_geometry(L, p_drop, form):
    """S + 2 titles (two workgroups walk a second title) of every title length class: one token, a
    length below the 16-row half, the bench's 30, the full tile; y read through yrows with repeats."""
    key = ("S+2", L, p_drop, p_drop == 0, 2)
    c = case(*key)
    assert c.yrows.unique().numel() < c.T
    _check(c, fwd(key), [form, "split"], "geom")


def test_device_rng_pair():
    """The dropout key from a fixed device (seed, base) pair: the head pass rebuilds dO's dropout from
    the same element index under the walk."""
    seed, base, k = 4321, 500, 9
    n, L = count("S+1"), 3
    mask = walk_mask(n, L)
    inp = mha_pool_inputs(n, L, HEADS, DK, DV, 99)
    c = finish_case(n, L, 0.2, True, mask, inp, None, "walk-rng", seed=seed, offset=base + k)
    rng = torch.tensor([seed, base], dtype=torch.int64, device="cuda")
    f = T.run_fwd(c, "f32", rng=rng, seed=1, offset=k)
    _check(c, f, ["split_ws32"], "rng")


def test_seg_direct_rows():
    """dsto with ~0 entries and direct per-row destinations (seg / dyu_row0, as
    test_mha_pool_gpu.test_seg_direct_rows) with S + 2 titles: the prefetched dy offsets of the second
    titles are the LN pass's."""
    from newsrec_amd import kernels as K
    n, L, V = count("S+2"), 7, 900
    mask = walk_mask(n, L)
    Tn = mask.numel()
    ids = torch.randint(1, V, (Tn,), generator=torch.Generator().manual_seed(6))
    ur = K.UniqueRows(ids.cuda(), V, grad_mask=mask.cuda())
    inv = ur.inv.cpu()
    U = int(ur.counts[0].item())
    inp = mha_pool_inputs(n, L, HEADS, DK, DV, 17, rows=ur.cap)
    c = finish_case(n, L, 0.2, True, mask, inp, inv, "walk-seg")
    f = T.run_fwd(c, "f32")
    T.check_fwd_layout(c, f)
    out = T.run_bwd(c, f, "split", seg=ur, dy_extra=ur.cap, dy_pad=4)
    dyall = out["dy"]
    ur.segment_sum_multi(dyall[:Tn, :c.NY], dyall[Tn:, :c.NY])
    torch.cuda.synchronize()
    dyall = dyall.cpu()
    assert T._all_nan_bits(dyall[:, c.NY:])
    seg = ur.seg_off.cpu().long()
    counts = seg[1:U + 1] - seg[:U]
    assert (counts == 1).any() and (counts > 1).any()
    live = (mask != 0).reshape(-1)
    sums = {dt: torch.zeros(U, c.NY, dtype=dt).index_add_(0, inv[live], c.ref[dt]["dy"][live]) for dt in (F64, F32)}
    assert torch.isfinite(dyall[Tn:Tn + U, :c.NY]).all()
    late = []
    pairs = [("dyu", dyall[Tn:Tn + U, :c.NY], (sums[F64], sums[F32]))]
    pairs += [(k, out[k][:c.ref[F64][k].numel()], k) for k in ("dbias", "dq", "dgamma", "dbeta")]
    T.compare(c, "walk-seg", pairs, late)
    assert not late, "; ".join(late)


# ---------------------------------------------------------------------- unchanged arithmetic, sentinels

def _titles(c, f, sel):
    """The case and forward buffers of titles ``sel`` of (c, f) alone, rows gathered (p_drop = 0: the
    dropout's element index would move with the rows)."""
    assert c.p_drop == 0 and c.yrows is None and not c.with_dz
    sel = torch.as_tensor(sel)
    tok = (sel[:, None] * c.L + torch.arange(c.L)[None]).reshape(-1)
    n = sel.numel()
    c2 = types.SimpleNamespace(**vars(c))
    c2.n, c2.T, c2.mask = n, n * c.L, c.mask[sel]
    c2.inp = dict(c.inp, dnews=c.inp["dnews"][sel])
    f2 = types.SimpleNamespace(**vars(f))
    f2.y, f2.mask, f2.oout = f.y[tok.cuda()], f.mask[sel.cuda()], f.oout[tok.cuda()]
    f2.stats = f.stats[:2 * c.T].reshape(c.T, 2)[tok.cuda()].reshape(-1).contiguous()
    f2.probs = f.probs[:c.T][tok.cuda()].contiguous()
    return c2, f2, tok


def test_walked_titles_match_single_titles_bitwise():
    """dy of a title does not depend on where in a walk it falls.  Titles of every walk position of the
    2 S + 3 case (first, second and third title of a workgroup, the last title, the one before it) run
    again as a batch of their own -- fewer titles than S: one title per workgroup, no second title, the
    prefetch clamped at once, which is all the one-title-per-workgroup kernel did -- and give the same
    dy bit for bit.

    (The comparison against the fused backward on the saved O is not available as an exact check: on
    the parent commit's build the two forms differ in the last bits at every case tried here -- 13 of
    6,912 dy words at 2 titles of L = 3, 40,204 of 1,181,952 at S + 1 titles, S = 341 -- and in the same
    number of words, at the same first position, with the walk.)"""
    key = ("2S+3", 2, 0.0, False)
    c, f = case(*key), fwd(key)
    s = walk_cap()
    sel = sorted({1, 2, s - 1, s, s + 1, 2 * s - 1, 2 * s, 2 * s + 1, 2 * s + 2} & set(range(c.n)))
    if len(sel) >= s:          # a device holding fewer workgroups than the titles picked
        sel = sel[:max(s - 1, 1)]
    full = T.run_bwd(c, f, "split")["dy"][:, :c.NY]
    c2, f2, tok = _titles(c, f, sel)
    part = T.run_bwd(c2, f2, "split")["dy"][:, :c.NY]
    assert torch.isfinite(part).all()
    diff = part.view(torch.int32) != full[tok].view(torch.int32)
    assert not diff.any(), "%d of %d dy words differ, first at %s" % (
        int(diff.sum()), diff.numel(), diff.nonzero()[0].tolist())


def test_sentinels_past_the_titles():
    """dy, o and news inside taller and wider NaN buffers: rows past nseq * L (past nseq for news) and
    columns past the width come back NaN bit for bit -- the clamped prefetch of the walk's last title
    and the forward write nothing outside."""
    from newsrec_amd import kernels as K
    key = ("S+1", 3, 0.2, True)
    c = case(*key)
    ybuf, y = T._padded(c.inp["y"], 4)
    mask = c.mask.cuda()
    gamma, beta, q = c.inp["gamma"].cuda(), c.inp["beta"].cuda(), c.inp["q"].cuda()
    news, zout, oout = T._nan(c.n + 2, c.H + 3), T._nan(c.T + 3, c.H + 5), T._nan(c.T + 3, c.H + 4)
    stats, probs = T._vec(2 * c.T, tail=7)[0], T._vec(c.T, tail=5)[0]
    K.mha_pool_fwd(y, mask, c.n, c.L, c.heads, c.dk, c.dv, gamma, beta, q, news[:c.n, :c.H], stats, probs,
                   p_drop=c.p_drop, seed=T.SEED, offset=T.OFFSET, zout=zout[:c.T, :c.H], oout=oout[:c.T, :c.H],
                   prec=T._prec("f32"))
    torch.cuda.synchronize()
    for name, buf, rows in (("news", news, c.n), ("zout", zout, c.T), ("oout", oout, c.T)):
        assert T._all_nan_bits(buf[rows:]), "%s: rows past the titles written" % name
        assert T._all_nan_bits(buf[:, c.H:]), "%s: columns past the width written" % name
        assert torch.isfinite(buf[:rows, :c.H]).all(), name
    assert T._all_nan_bits(stats[2 * c.T:]) and T._all_nan_bits(probs[c.T:])
    f = types.SimpleNamespace(y=y, ybuf=ybuf, mask=mask, yrows=None, gamma=gamma, beta=beta, q=q, news=news[:c.n],
                              zout=zout[:c.T], oout=oout[:c.T], stats=stats, probs=probs, rng=None, seed=T.SEED,
                              offset=T.OFFSET)
    late = []
    T.compare(c, "sentinel-fwd", T.fwd_pairs(c, f), late)
    for form in ("split", "split_ws32"):
        out = T.run_bwd(c, f, form, dy_extra=5)
        assert T._all_nan_bits(out["dy"][c.T:]), "dy: rows past nseq * L written"
        out["dy"] = out["dy"][:c.T]
        T.check_bwd(c, out, "sentinel-" + form, late)
    assert not late, "; ".join(late)


def test_walk_query():
    """The query entry: a positive cap for the head pass of every instantiated geometry, the same value
    on a second call; invalid arguments negative."""
    from newsrec_amd import _lib as L
    fn = L.load().nr_mha_pool_walk_workgroups
    for heads, dk, dv in T.GEOMS.values():
        s = fn(2, heads, dk, dv, L.GEMM_F32)
        assert s >= 1 and fn(2, heads, dk, dv, L.GEMM_F32) == s
    assert fn(1, HEADS, DK, DV, L.GEMM_F32) == 0        # the fused backward: one workgroup per title
    assert fn(2, 13, DK, DV, L.GEMM_F32) < 0 and fn(7, HEADS, DK, DV, L.GEMM_F32) < 0
    assert fn(2, HEADS, 48, DV, L.GEMM_F32) < 0
