"""One workgroup, several units: the persistent walk of the fast GEMM kernels (csrc/gemm_walk.h --
the unit sequence, the pending epilogue behind the next unit's first loads, the
skip of splits a device-resident K leaves empty) and the big kernel's unit loop, at small sizes.  The
other kernel tests mostly run one unit per workgroup.

Cases, inputs and bars: tests/gemm_walk_util.py and tests/gemm_epi_util.py (`bar`, `gemm_tol`);
tests/test_gemm_route_cpu.py pins the kernel each case runs on.  Storage is guarded as in
tests/test_gemm_epi_kernels_gpu.py (gemm_guard_util.Block): nothing outside the live window may change.
Every test prints its worst error / bar ratio ("WALK_RATIO ...")."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_epi_util as U
import gemm_walk_util as W
from gemm_guard_util import NAN, Block, _bits
from newsrec_amd import _lib as L
from newsrec_amd import kernels as K


def _operand(x, layout, ld, k_live):
    """x [rows, K] as a K-contiguous [rows][ld] or MN-contiguous [K][ld] operand; NaN in the padding
    and at k >= k_live."""
    rows, k = x.shape
    if layout == "kc":
        t = torch.full((rows, ld), NAN)
        t[:, :k_live] = x[:, :k_live]
        return K.operand(t.cuda()[:, :k], L.KCONTIG)
    t = torch.full((k, ld), NAN)
    t[:k_live, :rows] = x[:, :k_live].t()
    return K.operand(t.cuda()[:, :rows], L.MNCONTIG)


def _call(case, max_cus, c, k_dev=None):
    s = case.kernel.shape
    d = U.inputs(s)
    k_live = s.K if k_dev is None else k_dev
    a = _operand(d["a"], case.a_layout, W.lda(case), k_live)
    b = _operand(d["b"][:, :case.n].t(), case.b_layout, W.ldb(case), k_live)
    kw = dict(epilogue=case.epi, split_k=case.split_k, prec=U.PREC[case.kernel.prec])
    if case.kernel.form == "static":
        K.gemm(s.M, case.n, s.K, a, b, c.win, **kw)
    else:
        dev = lambda v: torch.tensor([v], dtype=torch.int32, device="cuda")
        K.gemm_dyn(s.M, case.n, s.K, a, b, c.win, m_dev=dev(s.m_dev) if case.kernel.form == "mdev" else None,
                   k_dev=dev(k_dev) if k_dev is not None else None, max_cus=max_cus, **kw)
    torch.cuda.synchronize()


def _check(case, c, live, want, k, name):
    d = U.inputs(case.kernel.shape)
    got = c.check(live, name)
    assert torch.isfinite(got).all(), name
    bound = U.bar(case.epi, d["a"].abs().max().item(), d["b"].abs().max().item(), k, case.kernel.planes, want)
    err = (got.double() - want).abs().max().item()
    print("WALK_RATIO %s err=%.3e bar=%.3e ratio=%.4f" % (name, err, bound, err / bound))
    assert err <= bound, "%s: err %.3e > bar %.3e" % (name, err, bound)


@pytest.mark.parametrize("case", W.STORE_CASES, ids=[c.id for c in W.STORE_CASES])
def test_capped_grid_is_bitwise_the_full_grid(case):
    """max_cus = 1 (two workgroups walk six units; on the big kernel one walks 28) against max_cus = 0:
    each element is produced by one unit in the same k order whatever the grid, so C is the same bit
    for bit -- and within the bar of the float64 product."""
    s = case.kernel.shape
    live = s.m_dev if case.kernel.form == "mdev" else s.M
    blocks = []
    for max_cus in (case.max_cus, 0):
        c = Block(s.M, case.n, case.n + 8, 4)
        _call(case, max_cus, c)
        blocks.append(c)
    assert torch.equal(_bits(blocks[0].dev), _bits(blocks[1].dev)), case.id
    want = U.product(s, case.kernel.planes)[:live, :case.n]
    _check(case, blocks[0], live, want, s.K, "store " + case.id)


@pytest.mark.parametrize("case", W.ATOMIC_CASES, ids=[c.id for c in W.ATOMIC_CASES])
def test_empty_splits_are_skipped(case):
    """NR_EPI_ATOMIC, three K splits under a bound of K, k_dev = 32: only split 0 holds any k (the
    operands are NaN from k = 32 on).  C += the product over the first 32 k in rows [0, m_dev); rows
    past m_dev and the block's margin (finite, so that a stray atomic add would show) are untouched.
    On the 128 x 128 kernels two workgroups walk twelve units, eight of them empty.  The big kernel's case
    has six units on six workgroups (gemm_walk_util: its re-split never leaves more units than
    workgroups), so it covers the skip of an empty unit, not a multi-unit walk with an empty unit in it."""
    s = case.kernel.shape
    d = U.inputs(s)
    g = torch.Generator().manual_seed(5)
    c = Block(s.M, case.n, case.n + 8, 4, fill=d["c0"][:, :case.n],
              margin=torch.randn(s.M + 8, case.n + 8, generator=g))
    _call(case, case.max_cus, c, k_dev=case.k_dev)
    want = d["c0"][:s.m_dev, :case.n].double() + U.product(s, case.kernel.planes, case.k_dev)[:s.m_dev, :case.n]
    _check(case, c, s.m_dev, want, case.k_dev, "atomic " + case.id)


def test_more_units_than_resident_workgroups():
    """Static form, exact-f32 64 x 64 kernel, 34 x 34 = 1156 units: more than the workgroups a device
    holds at once (at most 4 per CU), so the grid is capped and some workgroups walk two units."""
    case = W.STATIC_CASE
    s = case.kernel.shape
    c = Block(s.M, case.n, case.n + 8, 4)
    _call(case, 0, c)
    _check(case, c, s.M, U.product(s, 0), s.K, "static " + case.id)
