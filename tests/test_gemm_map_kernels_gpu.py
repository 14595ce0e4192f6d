"""The row maps (NR_ROWS_GATHER, NR_ROWS_CONV3), the MN-contiguous A operand, split-K and the epilogues
that add into or scatter over a table (NR_EPI_ATOMIC, _SCATTER, _SCATTER_STORE, _SCATTER_ZEROED) of
nr_gemm_f32* on every kernel family, against the float64 references of tests/gemm_map_util.py (held to
autograd in tests/test_gemm_map_ref_cpu.py, which also pins that every case routes to the kernel its
row names).

Storage of every case: the operands' padding columns, table rows 0 and V - 1 and the rows of a plain
operand past a device-resident extent are NaN (gemm_map_util); the destination is a window at row 4,
column 4 of a block of rows + 8 rows with ld = round4(columns) + 8.  For NR_EPI_STORE the block is NaN.
For the adding and scattering epilogues the whole block -- window, margins, absent rows, pad row,
guard row -- holds finite random values (a stray atomic add into NaN would leave the bits unchanged):
NR_EPI_ATOMIC and NR_EPI_SCATTER must leave entry + sums, NR_EPI_SCATTER_STORE the accumulators
themselves in the named rows (not entry + accumulators), NR_EPI_SCATTER_ZEROED the same with the
named rows zero on entry.  The bias of an epilogue that does not read it is all NaN.  After the call
the elements the reference says are touched must be finite and within the bar, and every other
element of the block bit-identical to before.

Every case prints "MAP_RATIO <family> <case> c= err= bar= ratio=".  Worst err / bar per family on an
MI355X: f32_64 0.020, f32_128 0.020, split_128_3 0.013, split_128_1 0.009, big_3 0.018, big_1 0.009,
generic 0.011."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_map_util as U
from gemm_guard_util import NAN, Block, _bits
from newsrec_amd import _lib as L
from newsrec_amd import kernels as K

_DEV = {}           # operands and row tables on the GPU, per problem: uploaded once
_MAP = {"plain": L.ROWS_PLAIN, "gather": L.ROWS_GATHER, "conv3": L.ROWS_CONV3}


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


def _dev(p, name, host):
    key = (id(p), name)
    if key not in _DEV:
        _DEV[key] = host.cuda()
    return _DEV[key]


def _operand(c, p, side):
    op = p.A if side == "A" else p.B
    t = _dev(p, side, op.store)[:, :op.cols]
    layout = L.KCONTIG if op.layout == "kc" else L.MNCONTIG
    if op.map == "plain":
        return K.operand(t, layout)
    return K.operand(t, layout, rows=_dev(p, side + "ids", op.ids), mapping=_MAP[op.map], seq_len=c.seq, seg=op.seg)


def _run(c):
    """One call on guarded storage, checked; returns (destination block, error / bar)."""
    p = U.problem(c)
    rows, cols = U.dest_shape(c)
    ld = U.round4(cols) + 8
    margin = None
    if c.epi != L.EPI_STORE:
        margin = torch.randn(rows + 8, ld, generator=U._seed("margin", rows, ld))
    blk = Block(rows, cols, ld, 4, U.entry_fill(c), margin)
    bvec = torch.full((c.N + 12,), NAN)
    if c.epi == L.EPI_STORE and p.bias is not None:
        bvec[4:4 + c.N] = p.bias
    kw = dict(bias=bvec.cuda()[4:4 + c.N], epilogue=c.epi, split_k=c.split, prec=U.PREC[c.prec])
    if c.epi in U.SCATTERS:
        kw.update(c_rows=K.rows_map(_dev(p, "cids", p.cids), _MAP[p.cmap], seq_len=c.seq, seg=p.cseg), pad_row=0)
    args = (c.M, c.N, c.K, _operand(c, p, "A"), _operand(c, p, "B"), blk.win)
    if c.form == "static":
        K.gemm(*args, **kw)
    else:
        def extent(v):
            return torch.tensor([v], dtype=torch.int32, device="cuda") if v is not None else None
        K.gemm_dyn(*args, m_dev=extent(c.m_dev), k_dev=extent(c.k_dev), workspace=c.work, **kw)
    torch.cuda.synchronize()
    want, touched, bar, contrib = U.wanted(c)
    got = blk.check_touched(touched, c.id)
    assert torch.isfinite(got[touched]).all(), c.id
    err = (got.double() - want)[touched].abs().max().item()
    print("MAP_RATIO %s %s c=%d err=%.3e bar=%.3e ratio=%.4f" % (c.family, c.id, contrib, err, bar, err / bar))
    assert err <= bar, "%s: err %.3e > bar %.3e" % (c.id, err, bar)
    return blk, err / bar


_CASES = U.all_cases()


@pytest.mark.parametrize("case", _CASES, ids=[c.id for c in _CASES])
def test_map_matrix(case):
    _run(case)


# the exact-f32 64 x 64 kernel under its two `prec`: one kernel.  Where one accumulator value reaches each
# destination element (c = 1: the stores, and one add into the entry value) the results must not differ
# in a bit.  Where several are added atomically (split-K, repeated scatter ids) the hardware orders the
# adds differently from launch to launch -- two launches under ONE prec differ as well -- so the results
# are the same fp32 values added in another order: within the bar's fp32-addition term
# 2^-22 c max|want| of each other, and each within the whole bar of float64.
_F32_64 = [c for c in _CASES if c.family == "f32_64" and c.prec == "f32"]


@pytest.mark.parametrize("case", _F32_64, ids=[c.id for c in _F32_64])
def test_f32_64_is_one_kernel_under_each_prec(case):
    a, _ = _run(case)
    b, _ = _run(case._replace(prec="bf16x6", id=case.id.replace("-f32-", "-bf16x6-")))
    want, touched, _, contrib = U.wanted(case)
    if contrib == 1:
        assert torch.equal(_bits(a.dev), _bits(b.dev)), case.id
    else:
        diff = (a.dev.double() - b.dev.double()).abs().max().item()
        assert diff <= 2.0 ** -22 * contrib * want[touched].abs().max().item(), (case.id, diff)


# split-K through the workspace: plain partial stores and one reduction in split order
_SLAB = [c for c in _CASES if c.work and c.epi == L.EPI_ATOMIC]


@pytest.mark.parametrize("case", _SLAB, ids=[c.id for c in _SLAB])
def test_workspace_reduction_is_ordered(case):
    """Two runs are bitwise equal to each other (and each within the bar of float64)."""
    a, _ = _run(case)
    b, _ = _run(case)
    assert torch.equal(_bits(a.dev), _bits(b.dev)), case.id
