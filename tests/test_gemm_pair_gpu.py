"""nr_gemm_f32_pair (two independent small GEMMs in one launch) against two calls of the existing
entry: the outputs must be BITWISE those of the two calls -- every unit of a paired problem runs the
arithmetic of its own launch, in the same order -- wherever those calls are themselves deterministic
(a store epilogue, or an atomic one with a single K split into a zeroed output).  Outputs are
NaN-prefilled and over-wide.  Which pairs share a launch is pinned without a GPU in
tests/test_gemm_pair_route_cpu.py.

Problem a is an input gradient dx = dY W (rows x D x NY: K-contiguous dY, MN-contiguous W, store),
problem b a weight gradient dW += dYᵀ x (NY x D x rows: MN-contiguous dY and x, atomic)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from newsrec_amd import _lib as L
from newsrec_amd import kernels as K

NAN = float("nan")


def _bits(t):
    return t.contiguous().view(torch.int32)


class Dgrad:
    """dx [rows, D] = dY [rows, NY] W [NY, D]"""

    def __init__(self, rows, D, NY, seed, w_kc=False):
        g = torch.Generator().manual_seed(seed)
        self.M, self.N, self.Kd = rows, D, NY
        self.dY = torch.randn(rows, NY, generator=g).cuda()
        W = torch.randn(NY, D, generator=g)
        # w_kc: W stored [D][NY] (K-contiguous, the forward's mode pair: not instantiated as a pair)
        self.W = (W.t().contiguous() if w_kc else W).cuda()
        self.b_layout = L.KCONTIG if w_kc else L.MNCONTIG
        self.kw = {}

    def out(self):
        return torch.full((self.M, self.N + 4), NAN, device="cuda")

    def ops(self):
        return K.operand(self.dY, L.KCONTIG), K.operand(self.W, self.b_layout)


class Wgrad:
    """dW [NY, D] += dYᵀ [NY, rows] x [rows, D], split_k K pieces added atomically"""

    def __init__(self, NY, D, rows, seed, split_k=1):
        g = torch.Generator().manual_seed(seed)
        self.M, self.N, self.Kd = NY, D, rows
        self.dY = torch.randn(rows, (NY + 3) // 4 * 4, generator=g).cuda()
        self.x = torch.randn(rows, D, generator=g).cuda()
        self.kw = dict(epilogue=L.EPI_ATOMIC, split_k=split_k)

    def out(self):
        c = torch.full((self.M, self.N + 4), NAN, device="cuda")
        c[:, :self.N] = 0.0
        return c

    def ops(self):
        return K.operand(self.dY, L.MNCONTIG), K.operand(self.x, L.MNCONTIG)


def _alone(p, prec, **kw):
    c = p.out()
    a, b = p.ops()
    K.gemm(p.M, p.N, p.Kd, a, b, c, ldc=c.stride(0), prec=prec, **p.kw, **kw)
    return c


def _desc(p, c, prec, **kw):
    a, b = p.ops()
    return K.gemm_desc(p.M, p.N, p.Kd, a, b, c, ldc=c.stride(0), prec=prec, **p.kw, **kw)


def _paired(p1, p2, prec):
    c1, c2 = p1.out(), p2.out()
    K.gemm_pair(_desc(p1, c1, prec), _desc(p2, c2, prec), c1)
    return c1, c2


def _check_pair(p1, p2, prec):
    want1, want2 = _alone(p1, prec), _alone(p2, prec)
    for first, second in ((p1, p2), (p2, p1)):   # either order of the two descriptions
        got = _paired(first, second, prec)
        torch.cuda.synchronize()
        got1, got2 = got if first is p1 else got[::-1]
        assert torch.equal(_bits(got1), _bits(want1))
        assert torch.equal(_bits(got2), _bits(want2))
    for p, w in ((p1, want1), (p2, want2)):      # and the reference calls did compute something
        assert not torch.isnan(w[:, :p.N]).any() and torch.isnan(w[:, p.N:]).all()
        assert w[:, :p.N].abs().max() > 0


PRECS = [L.GEMM_BF16X6, L.GEMM_F32]   # both take small problems to the exact-f32 64 x 64 kernel


@pytest.mark.parametrize("prec", PRECS)
def test_pair_base_shapes(prec):
    """rows = 96, D = 64, NY = 96: 2 + 2 units, each problem ragged in its row tiles."""
    _check_pair(Dgrad(96, 64, 96, 1), Wgrad(96, 64, 96, 2), prec)


@pytest.mark.parametrize("prec", PRECS)
def test_pair_odd_tile_counts(prec):
    """M = 70 rows: a ragged second row tile in the input gradient, and in the weight gradient (whose
    MN-contiguous dY then has padded rows of 72)."""
    _check_pair(Dgrad(70, 64, 96, 3), Wgrad(96, 64, 96, 4), prec)
    _check_pair(Dgrad(96, 64, 96, 5), Wgrad(70, 64, 96, 6), prec)
    _check_pair(Dgrad(70, 200, 160, 7), Wgrad(70, 136, 64, 8), prec)   # 2 x 4 and 2 x 3 tiles, ragged columns


def test_pair_single_unit():
    _check_pair(Dgrad(64, 64, 32, 9), Wgrad(96, 64, 96, 10), L.GEMM_BF16X6)
    _check_pair(Dgrad(96, 64, 96, 11), Wgrad(64, 64, 32, 12), L.GEMM_BF16X6)
    _check_pair(Dgrad(64, 64, 32, 13), Wgrad(64, 64, 32, 14), L.GEMM_BF16X6)


def test_pair_more_units_than_resident_slots():
    """1728 x 1216 x 32 is 27 x 19 = 513 units, one more than 256 CUs x 2 resident workgroups: the launch is
    capped and each problem strides over its own share (its partner, one unit, keeps one workgroup)."""
    _check_pair(Dgrad(1728, 1216, 32, 15), Wgrad(64, 64, 32, 16), L.GEMM_BF16X6)


def test_pair_split_k_weight_gradient():
    """The step's form: the weight gradient's K in three pieces added atomically.  The three fp32
    partial sums of an element meet in any order, in the pair as in the call alone, so the comparison is
    not bitwise: each element is a sum of 3 partials of magnitude <= S = sum_k |a_k b_k| <= K max|a| max|b|,
    and two orders of adding three fp32 numbers differ by at most 2 roundings of at most S: 2 * 2^-24 * S
    (bound used: 4 * 2^-24 * K * max|a| * max|b|)."""
    p1, p2 = Dgrad(96, 64, 96, 17), Wgrad(96, 64, 96, 18, split_k=3)
    want1, want2 = _alone(p1, L.GEMM_BF16X6), _alone(p2, L.GEMM_BF16X6)
    got1, got2 = _paired(p1, p2, L.GEMM_BF16X6)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got1), _bits(want1))
    bound = 4 * 2.0 ** -24 * p2.Kd * p2.dY.abs().max().item() * p2.x.abs().max().item()
    err = (got2[:, :p2.N] - want2[:, :p2.N]).abs().max().item()
    print("split-K pair vs alone: max err %.3g, bound %.3g" % (err, bound))
    assert err <= bound
    assert torch.isnan(got2[:, p2.N:]).all()


def test_pair_falls_back_for_another_mode_pair():
    """A forward-mode first problem (both operands K-contiguous) is not instantiated as a pair: the two
    problems run one after the other, with the same results and return code."""
    _check_pair(Dgrad(96, 64, 96, 19, w_kc=True), Wgrad(96, 64, 96, 20), L.GEMM_BF16X6)


def test_pair_falls_back_with_a_cu_cap():
    """max_cus set on one problem: the dynamic form (128 x 128 tiles) for it, no pairing."""
    p1, p2 = Dgrad(200, 136, 96, 21), Wgrad(96, 64, 96, 22)
    c = p1.out()
    a, b = p1.ops()
    K.gemm_dyn(p1.M, p1.N, p1.Kd, a, b, c, ldc=c.stride(0), prec=L.GEMM_BF16X6, max_cus=64)
    want2 = _alone(p2, L.GEMM_BF16X6)
    c1, c2 = p1.out(), p2.out()
    K.gemm_pair(_desc(p1, c1, L.GEMM_BF16X6, max_cus=64), _desc(p2, c2, L.GEMM_BF16X6), c1)
    torch.cuda.synchronize()
    assert torch.equal(_bits(c1), _bits(c)) and torch.equal(_bits(c2), _bits(want2))
    assert not torch.isnan(c1[:, :p1.N]).any()


def test_pair_refuses_aliasing():
    """An output overlapping the other problem's operand or output: NR_EINVAL(201), nothing launched."""
    p1, p2 = Dgrad(96, 64, 96, 23), Wgrad(96, 64, 96, 24)
    c1, c2 = p1.out(), p2.out()
    x_before = p2.x.clone()
    d1 = K.gemm_desc(p1.M, p1.N, p1.Kd, *p1.ops(), p2.x, ldc=p2.x.stride(0), prec=L.GEMM_BF16X6)   # dx over x
    with pytest.raises(L.HipError, match="invalid argument 201"):
        K.gemm_pair(d1, _desc(p2, c2, L.GEMM_BF16X6), c2)
    with pytest.raises(L.HipError, match="invalid argument 201"):                                    # one output
        K.gemm_pair(_desc(p1, c1, L.GEMM_BF16X6), K.gemm_desc(p2.M, p2.N, p2.Kd, *p2.ops(), c1, ldc=c1.stride(0),
                                                              prec=L.GEMM_BF16X6, **p2.kw), c1)
    torch.cuda.synchronize()
    assert torch.equal(p2.x, x_before) and torch.isnan(c1).all() and torch.isnan(c2[:, p2.N:]).all()
    assert (c2[:, :p2.N] == 0).all()


def test_pair_reports_which_problem_is_invalid():
    p1, p2 = Dgrad(96, 64, 96, 25), Wgrad(96, 64, 96, 26)
    c1, c2 = p1.out(), p2.out()
    bad = K.gemm_desc(p2.M, p2.N, p2.Kd, *p2.ops(), c2, ldc=c2.stride(0), prec=7)   # nr_gemm_f32_ws: argument 12
    with pytest.raises(L.HipError, match="invalid argument 112"):
        K.gemm_pair(_desc(p1, c1, L.GEMM_BF16X6), bad, c1)
    with pytest.raises(L.HipError, match="invalid argument 12$"):
        K.gemm_pair(bad, _desc(p1, c1, L.GEMM_BF16X6), c1)
    torch.cuda.synchronize()
    assert torch.isnan(c1).all()
