"""What tests/test_gemm_epi_kernels_gpu.py stands on, checked without a GPU.

References: the closed forms of tests/gemm_epi_util.py against float64 autograd to 1e-12 -- F.gelu
(exact erf form) and its gradient, tanh, ReLU's forward and, for the gate of NR_EPI_ACCUM_GATE, ReLU's
backward (torch's relu passes no gradient at 0, like `aux > 0`) -- on small random inputs that
include +0.0 and -0.0; a NaN bias must not reach a bias-free epilogue's reference either.

Routes: every case of the family table goes through tests/gemm_route_dump.cpp's argument mode (built
as tests/test_gemm_route_cpu.py builds it: g++, warnings as errors, address and undefined-behaviour
sanitizers) and must land on the kernel family, tile and bf16 planes the table names, for every
epilogue, B layout and width.  A routing change that moves a case to another kernel fails here."""
import math
import os
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

import gemm_epi_util as U
from newsrec_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "gemm_route_dump.cpp")
F64 = torch.float64


def _close(got, want, name):
    scale = max(want.abs().max().item(), 1.0)
    err = (got - want).abs().max().item()
    assert err <= 1e-12 * scale, "%s: err %.3e of max %.3e" % (name, err, scale)


def _small(seed=0, m=9, n=7):
    g = torch.Generator().manual_seed(seed)
    pre = torch.randn(m, n, generator=g, dtype=F64) * 2
    bias = torch.randn(n, generator=g, dtype=F64)
    c0 = torch.randn(m, n, generator=g, dtype=F64)
    aux = torch.randn(m, n, generator=g, dtype=F64) * 2
    pre[0, 0] = 0.0
    pre[1, 1] = -bias[1]        # pre + bias == 0
    aux[0, 0], aux[0, 1] = 0.0, -0.0
    return pre, bias, c0, aux


def test_store_forms_vs_torch():
    pre, bias, c0, _ = _small(1)
    _close(U.reference(L.EPI_STORE, pre, bias)[0], pre + bias, "store")
    _close(U.reference(L.EPI_STORE_RELU, pre, bias)[0], F.relu(pre + bias), "relu")
    _close(U.reference(L.EPI_STORE_TANH, pre, bias)[0], torch.tanh(pre + bias), "tanh")
    _close(U.reference(L.EPI_ACCUM, pre, bias, c0=c0)[0], torch.add(c0, pre + bias), "accum")
    for epi in (L.EPI_STORE, L.EPI_STORE_RELU, L.EPI_STORE_TANH):   # no bias: zeros
        _close(U.reference(epi, pre, None)[0], U.reference(epi, pre, torch.zeros_like(bias))[0], "no bias")
    assert U.reference(L.EPI_STORE_RELU, pre, bias)[0][1, 1] == 0.0


def test_gelu_forms_vs_autograd():
    pre, bias, _, aux = _small(2)
    c, x = U.reference(L.EPI_STORE_GELU, pre, bias)
    _close(x, pre + bias, "store_gelu aux")
    _close(c, F.gelu(pre + bias), "store_gelu C")            # approximate='none': the erf form
    a = aux.clone().requires_grad_()
    F.gelu(a).backward(pre)                                   # dL/da = pre * gelu'(a)
    _close(U.reference(L.EPI_GELU_GRAD, pre, aux=aux)[0], a.grad, "gelu_grad")
    z = torch.zeros(1, dtype=F64)
    assert U.gelu_grad(z).item() == 0.5 and U.gelu(z).item() == 0.0
    _close(U.normal_pdf(z), torch.tensor([1.0 / math.sqrt(2.0 * math.pi)], dtype=F64), "pdf(0)")


def test_gate_vs_relu_backward():
    """C = (C0 + pre) * relu'(aux): autograd of relu(aux) with the upstream gradient C0 + pre."""
    pre, _, c0, aux = _small(3)
    a = aux.clone().requires_grad_()
    F.relu(a).backward(c0 + pre)
    got = U.reference(L.EPI_ACCUM_GATE, pre, None, c0=c0, aux=aux)[0]
    _close(got, a.grad, "accum_gate")
    assert got[0, 0] == 0.0 and got[0, 1] == 0.0              # +0.0 and -0.0 close the gate
    assert (got[aux > 0] != 0).all() and (got[aux < 0] == 0).all()


def test_bias_free_references_ignore_bias():
    pre, bias, c0, aux = _small(4)
    nan = torch.full_like(bias, float("nan"))
    for epi in (L.EPI_ACCUM_GATE, L.EPI_GELU_GRAD):
        got = U.reference(epi, pre, nan, c0=c0, aux=aux)[0]
        assert torch.isfinite(got).all()
        assert torch.equal(got, U.reference(epi, pre, None, c0=c0, aux=aux)[0])
    assert {e for e in U.EPI_NAME if e not in U.READS_BIAS} == {L.EPI_ACCUM_GATE, L.EPI_GELU_GRAD}


def test_case_inputs():
    """The gate matrix holds +0.0, -0.0 and both signs; a narrower case is a slice of the wider one's
    product; the bf16 product is over the rounded operands."""
    d = U.inputs(U.SMALL)
    gate = d["aux_gate"]
    bits = gate.view(torch.int32)
    assert (bits == 0).sum() > 100 and (bits == -2 ** 31).sum() > 100
    assert (gate > 0).sum() > 100 and (gate < 0).sum() > 100
    p = U.product(U.SMALL, 0)
    assert p.dtype == F64 and p.shape == (70, 52) and U.product(U.SMALL, 3) is p
    assert torch.equal(p, d["a"].double() @ d["b"].double())
    p1 = U.product(U.SMALL, 1)
    assert torch.equal(p1, d["a"].bfloat16().double() @ d["b"].bfloat16().double()) and not torch.equal(p1, p)
    assert torch.equal(U.product(U.MID, 0, k=64), U.inputs(U.MID)["a"][:, :64].double() @ U.inputs(U.MID)["b"][:64].double())
    c, x, bar_c, bar_x = U.wanted(U.KERNEL["big_3-mdev"], L.EPI_STORE_GELU, 1026)
    assert c.shape == (1600, 1026) and x.shape == c.shape and 0 < bar_x < bar_c < 1e-3
    for s in (U.SMALL, U.MID, U.BIG):   # both widths of a row: one float4-able, one not
        assert s.n_vec % 4 == 0 and s.n_scalar % 4 != 0 and s.ldb_mn >= (max(s.n_vec, s.n_scalar) + 3) // 4 * 4


@pytest.fixture(scope="module")
def route_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/gemm_route_dump.cpp"
    exe = str(tmp_path_factory.mktemp("epi_route") / "gemm_route_dump")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True, capture_output=True, text=True)
    return exe


def _route(exe, argv):
    r = subprocess.run([exe] + argv, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (argv, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == 1
    return U.parse_route(lines[0])


@pytest.mark.parametrize("kernel", U.KERNELS, ids=[k.id for k in U.KERNELS])
def test_table_rows_route_where_they_say(route_exe, kernel):
    for name, epi in U.EPILOGUES:
        for lay in U.layouts(kernel.shape):
            for n in U.widths(kernel.shape):
                got = _route(route_exe, U.route_argv(kernel, epi, lay, n, name=kernel.id))
                want = U.route_fields(kernel, epi, lay)
                assert {f: got.get(f) for f in want} == want, (kernel.id, name, lay, n, got)
                assert got["name"] == kernel.id and got["prec"] == kernel.prec


def test_device_k_case_routes(route_exe):
    """The device-K cases (bound K = 96, dynamic form) are the table's dyn rows themselves; the K == 0
    case (static form) runs the generic kernel in every arithmetic."""
    for prec in ("f32", "bf16x6", "bf16"):
        got = _route(route_exe, ["k0", "70", "50", "0", "kc", "72", "kc", "72", str(L.EPI_ACCUM), "static", prec])
        assert got["family"] == "generic" and got["tile"] == "64x64"


def test_pair_case_routes(route_exe):
    """Both problems of the pair case on the exact-f32 64 x 64 kernel, in the instantiated mode pair."""
    dx = _route(route_exe, ["dx", "96", "64", "96", "kc", "96", "mn", "64", str(L.EPI_ACCUM), "static", "bf16x6"])
    dw = _route(route_exe, ["dw", "96", "64", "96", "mn", "96", "mn", "64", str(L.EPI_ATOMIC), "static", "bf16x6"])
    assert (dx["family"], dx["modes"], dx["tr"]) == ("f32_64", "0,3", "1")
    assert (dw["family"], dw["modes"], dw["tr"]) == ("f32_64", "3,3", "0")


def test_argument_mode_refuses_malformed_lines(route_exe):
    for argv in (["x"], ["x", "70", "50", "70", "kc", "72", "kc", "72", "0", "static"],
                 ["x", "70", "50", "70", "kk", "72", "kc", "72", "0", "static", "f32"],
                 ["x", "70", "50", "70", "kc", "72", "kc", "72", "11", "static", "f32"],
                 ["x", "70", "5o", "70", "kc", "72", "kc", "72", "0", "static", "f32"],
                 ["x", "70", "50", "70", "kc", "72", "kc", "72", "0", "static", "fp32"]):
        r = subprocess.run([route_exe] + argv, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stdout == "" and r.stderr.startswith("usage:"), argv
