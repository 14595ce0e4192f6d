"""What tests/test_gemm_map_kernels_gpu.py stands on, checked without a GPU.

References: the float64 forms of tests/gemm_map_util.py against float64 autograd to 1e-12 on small
inputs -- F.embedding + F.linear for the gathered forward and, with padding_idx, its backward for the
scatter with a pad row; F.conv1d(padding=1) forward, input gradient (scattered through the taps) and
weight gradient for the three CONV3 problems, with the permutations of test_gemm_conv3.

Inputs: the scatter-store ids are distinct, the scatter ids reach at most 4 (GATHER) / 12 (CONV3)
contributions per destination element (counted with the reference's own index_add_ of ones), no live
id names a NaN, guard or absent row, the poison and guard rows are named only at and past the device
extent, and every stored operand holds NaN exactly where gemm_map_util says.

Routes: every case of the table goes through the extended argument mode of
tests/gemm_route_dump.cpp (built as tests/test_gemm_route_cpu.py builds it) and must land on the
family, tile, planes, operand modes, accumulator layout, epilogue, K splits and workspace use its row
names.  A routing change that moves a case to another kernel fails here, not on the GPU."""
import os
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

import gemm_map_util as U
from newsrec_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "gemm_route_dump.cpp")
F64 = torch.float64


def _close(got, want, name):
    scale = max(want.abs().max().item(), 1.0)
    err = (got - want).abs().max().item()
    assert err <= 1e-12 * scale, "%s: err %.3e of max %.3e" % (name, err, scale)


# ---- references against autograd

def test_gather_and_its_scatter_vs_embedding():
    g = torch.Generator().manual_seed(1)
    v, e, t, n = 13, 6, 22, 5
    tab = torch.randn(v, e, generator=g, dtype=F64).requires_grad_()
    w, bias, dy = (torch.randn(n, e, generator=g, dtype=F64), torch.randn(n, generator=g, dtype=F64),
                   torch.randn(t, n, generator=g, dtype=F64))
    ids = torch.randint(0, v - 1, (t,), generator=g)
    ids[::4] = 0
    y = F.linear(F.embedding(ids, tab, padding_idx=0), w, bias)
    _close(tab.detach()[ids] @ w.t() + bias, y.detach(), "gather forward")
    y.backward(dy)
    got = U.scatter_sum(dy @ w, "gather", ids, 1, 1, v)
    _close(got, tab.grad, "scatter with a pad row")
    assert (got[0] == 0).all() and (got[v - 1] == 0).all() and (ids == 0).sum() >= 5


@pytest.mark.parametrize("seq", [5, 1])
def test_conv3_forms_vs_conv1d(seq):
    g = torch.Generator().manual_seed(2)
    v, e, titles, h = 11, 4, 6, 7
    t = titles * seq
    tab = torch.randn(v, e, generator=g, dtype=F64)
    ids = torch.randint(1, v, (t,), generator=g)
    w = torch.randn(h, e, 3, generator=g, dtype=F64).requires_grad_()
    bias, dc = torch.randn(h, generator=g, dtype=F64), torch.randn(t, h, generator=g, dtype=F64)
    x = tab[ids].view(titles, seq, e).transpose(1, 2).clone().requires_grad_()      # [n, E, L]
    out = F.conv1d(x, w, bias, padding=1).transpose(1, 2).reshape(-1, h)
    wr = w.detach().permute(0, 2, 1).reshape(h, 3 * e)                               # [H][j E + e]
    cols = U.conv_cols(tab[ids], seq)
    _close(cols @ wr.t() + bias, out.detach(), "conv forward")
    out.backward(dc)
    # input gradient, scattered through the taps into the table (token ids with a pad row)
    sids = ids.clone()
    sids[::3] = 0
    want = torch.zeros(v, e, dtype=F64).index_add_(0, sids, x.grad.transpose(1, 2).reshape(-1, e))
    want[0] = 0
    _close(U.scatter_sum(dc @ wr, "conv3", sids, seq, e, v), want, "conv scatter")
    _close(dc.t() @ cols, w.grad.permute(0, 2, 1).reshape(h, 3 * e), "conv weight gradient")


# ---- the inputs' properties

def test_scatter_ids_and_contribution_caps():
    ids = U.scatter_ids(U.T)
    live = ids[ids != 0]
    assert (ids == 0).sum() == 10 and live.min() == 1 and live.max() == 53 < 54 <= U.V_SCATTER - 2
    occ = torch.bincount(live, minlength=U.V_SCATTER)[1:54]
    assert occ.min() >= 2 and occ.max() <= 4        # repeats everywhere
    ones = torch.ones(U.T, 72, dtype=F64)
    cg = U.scatter_sum(ones, "gather", ids, 1, 1, U.V_SCATTER)
    cc = U.scatter_sum(ones, "conv3", ids, U.SEQ, 24, U.V_SCATTER)
    assert 2 <= cg.max() <= 4 and cg.max() < cc.max() <= 12
    for counts in (cg, cc):   # the pad row, the absent rows and the guard row get nothing
        assert (counts[0] == 0).all() and (counts[54:] == 0).all() and (counts[1:54] > 0).all()
    # what wanted() multiplies the bar by: the count times the splits
    sc = [c for c in U.all_cases() if c.epi == L.EPI_SCATTER]
    assert {U.wanted(c)[3] for c in sc if U.problem(c).cmap == "gather"} == {int(cg.max()) * s for s in (1, 2)}
    assert all(U.wanted(c)[3] <= 12 * c.splits for c in sc)


def test_store_ids_are_distinct_and_guarded():
    for n, live, v in ((160, None, 201), (160, 100, 201), (1800, 1600, 2001)):
        ids, rows = U.store_ids(n, live)
        m = n if live is None else live
        head = ids[:m]
        named = head[head != 0]
        assert rows == v and (head == 0).sum() == (m + 15) // 16
        assert named.numel() == named.unique().numel() and named.min() >= 1 and named.max() <= v - 2
        assert (ids[m:] == v - 1).all() and not (head == v - 1).any()


def test_load_ids_and_tables():
    for n, live in ((160, None), (160, 100), (2048, 1600), (1800, 1600)):
        ids = U.load_ids(n, live)
        m = n if live is None else live
        assert ids[:m].min() >= 1 and ids[:m].max() <= U.V_LOAD - 2 and (ids[m:] == U.V_LOAD - 1).all()
    t = U.table(U._seed("t"), 64, 68)
    assert torch.isnan(t[0]).all() and torch.isnan(t[-1]).all() and torch.isnan(t[:, 64:]).all()
    assert torch.isfinite(t[1:-1, :64]).all()


def test_every_case_holds_nan_where_nothing_may_be_read():
    """Per case: the padding columns of both stored operands, the rows of a plain operand past the
    device extent and table rows 0 and V - 1 are NaN; the logical operands and the reference are finite;
    the ids past the extent name the poison / guard row and no earlier id does."""
    for c in U.all_cases():
        p = U.problem(c)
        for op, extent in ((p.A, c.m_dev if p.A.layout == "kc" else c.k_dev),
                           (p.B, c.k_dev if p.B.layout == "mn" else None)):
            assert torch.isnan(op.store[:, op.cols:]).all() and op.store.shape[1] >= U.round4(op.cols), c.id
            if op.map == "plain":
                live = op.store.shape[0] if extent is None else extent
                assert torch.isfinite(op.store[:live, :op.cols]).all() and torch.isnan(op.store[live:]).all(), c.id
            else:
                assert torch.isnan(op.store[0]).all() and torch.isnan(op.store[-1]).all(), c.id
                live = op.ids.numel() if extent is None else extent
                assert op.ids[:live].min() >= 1 and op.ids[:live].max() <= U.V_LOAD - 2, c.id
                assert (op.ids[live:] == U.V_LOAD - 1).all(), c.id
        if p.A.layout == "mn" and c.M % 4:   # the columns [M, round4(M)) the loaders read and discard
            assert p.A.store.shape[1] >= U.round4(c.M) and torch.isnan(p.A.store[:, c.M:U.round4(c.M)]).all(), c.id
        assert torch.isfinite(p.a[:p.m_live, :p.k_live]).all() and torch.isfinite(p.b[:p.k_live]).all(), c.id
        want, touched, bar, contrib = U.wanted(c)
        assert torch.isfinite(want[touched]).all() and touched.any() and 0 < bar < 2e-2 and contrib >= 1, c.id
        if p.cids is not None:
            assert p.cids.max() < p.v and p.cids.min() >= 0
            if c.epi in U.STORES:
                assert not touched[0].any() and not touched[p.v - 1].any(), c.id
                if c.epi == L.EPI_SCATTER_ZEROED:   # named rows zero on entry, the rest is not
                    fill = U.entry_fill(c)
                    assert (fill[touched] == 0).all() and (fill[~touched] != 0).all(), c.id


def test_conv_taps_outside_the_title_are_zero_not_row_zero():
    """The reference replaces a tap outside the title by zero: with row 0 NaN a kernel that multiplied
    the loaded row by a mask instead would give NaN."""
    c = next(c for c in U.all_cases() if c.problem == "conv_fwd")
    p = U.problem(c)
    cols = p.a.view(-1, U.SEQ, 3, c.seg)
    assert (cols[:, 0, 0] == 0).all() and (cols[:, U.SEQ - 1, 2] == 0).all() and torch.isfinite(cols).all()
    assert (cols[:, 1:, 0] != 0).all() and (cols[:, :, 1] != 0).all() and torch.isnan(p.A.store[0]).all()


def test_table_covers_every_family_and_problem():
    cases = U.all_cases()
    assert len({c.id for c in cases}) == len(cases)
    fams = {c.family for c in cases}
    assert fams == {"f32_64", "f32_128", "split_128_3", "split_128_1", "big_3", "big_1", "generic"}
    eight = {"gather_fwd", "conv_fwd", "scatter_gather", "scatter_conv3", "scatter_store", "wgrad_plain",
             "wgrad_gather", "wgrad_conv3"}
    for f in fams - {"big_3", "big_1"}:
        assert {c.problem for c in cases if c.family == f} >= eight, f
    assert {c.problem for c in cases if c.family == "generic"} >= {"mn_gather_a", "kc_gather_b", "kc_conv3_b", "mn_conv3_a"}
    assert any(c.seq == 1 and c.family == "generic" for c in cases) and any(c.seq == 1 and c.family == "f32_64" for c in cases)


# ---- routes

@pytest.fixture(scope="module")
def route_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/gemm_route_dump.cpp"
    exe = str(tmp_path_factory.mktemp("map_route") / "gemm_route_dump")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True, capture_output=True, text=True)
    return exe


def _route(exe, argv):
    r = subprocess.run([exe] + argv, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (argv, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == 1
    return U.parse_route(lines[0])


@pytest.mark.parametrize("family", ["f32_64", "f32_128", "split_128_3", "split_128_1", "big_3", "big_1", "generic"])
def test_cases_route_where_they_say(route_exe, family):
    for c in U.all_cases():
        if c.family != family:
            continue
        got = _route(route_exe, U.route_argv(c))
        want = U.route_fields(c)
        assert {f: got.get(f) for f in want} == want, (c.id, got)
        assert got["name"] == c.id and got["prec"] == c.prec


def test_routes_the_table_relies_on(route_exe):
    """The exceptions the table is built around: a CONV3 weight gradient of seg 64 is not eligible for
    the 128-tile kernels (generic in the static form, NR_EINVAL(7) in the dynamic one); the big gathered
    forward without a device M stays on the 128 x 128 kernel; a scatter over one-token titles and
    NR_EPI_SCATTER_STORE at an ineligible K run the generic kernel, the latter as a store."""
    base = ["160", "192", "160", "mn", "160", "mn", "68", str(L.EPI_ATOMIC)]
    tail = ["bmap=conv3", "bseg=64", "seq=5", "split=2"]
    assert _route(route_exe, ["w"] + base + ["static", "bf16"] + tail)["family"] == "generic"
    got = _route(route_exe, ["w"] + base + ["dyn", "bf16x6"] + tail)
    assert (got["family"], got["einval"]) == ("not_eligible", "7")
    got = _route(route_exe, ["g", "1800", "1024", "512", "kc", "516", "kc", "516", "0", "dyn", "bf16x6", "amap=gather"])
    assert (got["family"], got["tile"]) == ("split_128", "128x128")
    got = _route(route_exe, ["s", "160", "70", "155", "kc", "160", "mn", "72", str(L.EPI_SCATTER_STORE), "static", "f32",
                             "cmap=gather"])
    assert (got["family"], got["epi"]) == ("generic", str(L.EPI_SCATTER_STORE))
    got = _route(route_exe, ["z", "160", "70", "155", "kc", "160", "mn", "72", str(L.EPI_SCATTER_ZEROED), "static", "f32",
                             "cmap=gather"])
    assert (got["family"], got["epi"]) == ("generic", str(L.EPI_SCATTER))


def test_argument_mode_keys(route_exe):
    """Without key=value tokens the line is the plain problem's, as before; every malformed token is
    refused with the usage line and exit status 2."""
    head = ["x", "160", "72", "160", "kc", "164", "mn", "72", str(L.EPI_SCATTER), "static", "f32"]
    plain = _route(route_exe, head)
    assert _route(route_exe, head + ["amap=plain", "bmap=plain", "cmap=gather", "seq=30", "split=1", "work=0"]) == plain
    assert _route(route_exe, head + ["split=2"])["splits"] == "2"
    for bad in (["amap"], ["amap="], ["=gather"], ["amap=scatter"], ["cmap=plain"], ["aseg=0"], ["bseg=x"],
                ["seq=0"], ["split=0"], ["work=2"], ["tile=64"], ["split=2x"], ["amap=gather", "nonsense"]):
        r = subprocess.run([route_exe] + head + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stdout == "" and r.stderr.startswith("usage:"), bad
