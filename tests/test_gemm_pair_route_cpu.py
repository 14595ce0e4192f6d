"""Which problem pairs nr_gemm_f32_pair runs as ONE launch (csrc/gemm_route.h: gemm_pair_order,
gemm_pair_alias) and how that launch's workgroups are shared (pair_grids), pinned without a GPU.

tests/gemm_pair_dump.cpp -- stand-alone, only the route header -- prints the decision for the MHA user
encoder's backward at the bench shapes (dx = dY W beside dW += dYᵀ x) and for one pair per way of
leaving it, and the workgroup split for unit counts around the 512 resident slots.  Built here with
g++ under the address and undefined-behaviour sanitizers and run as a child process.

EXPECTED was worked out by hand from the rules, not recorded from the program:
families -- 2 = exact-f32 64 x 64 (under 400 tiles of 128 x 128, static form), 4 = 128 x 128 bf16 planes
(the dynamic form, bf16, or >= 400 tiles), 5 = 256-row tiles (a re-split split-K weight gradient in the
dynamic form), 1 = generic (ld % 4 != 0).  order -- 1: one launch as given, 2: one launch, the
descriptions swapped, 0: two launches.  alias -- an output overlaps the other problem's output or
operand bytes (large_partner: its 243 MB dY spans the partner's output).
grids -- ga workgroups of the first problem at 0, gb of the second at off = ga rounded up to 8 (the
XCDs); capped at the slots, shared in proportion to the units, when off + gb would exceed them:
513 + 1 units -> 512 * 1 / 514 = 0 -> 1 workgroup for b, 511 -> 504 (a multiple of 8) for a."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "gemm_pair_dump.cpp")

EXPECTED = """\
user_bwd: families=2,2 alias=0 order=1
user_bwd_swapped: families=2,2 alias=0 order=2
two_dgrads: families=2,2 alias=1 order=0
two_dgrads_apart: families=2,2 alias=0 order=0
forward_modes: families=2,2 alias=0 order=0
gathered_wgrad: families=2,2 alias=0 order=0
cu_cap: families=4,2 alias=0 order=0
device_extent: families=2,5 alias=0 order=0
large_partner: families=4,2 alias=1 order=0
bf16_partner: families=4,2 alias=0 order=0
f32_partner: families=2,2 alias=0 order=1
generic_partner: families=1,2 alias=0 order=0
alias_operand: families=2,2 alias=1 order=0
alias_operand_2: families=2,2 alias=1 order=0
alias_output: families=2,2 alias=1 order=0
adjacent_outputs: families=2,2 alias=0 order=1
grids ua=150 ub=324 slots=512: ga=150 off=152 gb=324
grids ua=2 ub=2 slots=512: ga=2 off=8 gb=2
grids ua=1 ub=1 slots=512: ga=1 off=8 gb=1
grids ua=513 ub=1 slots=512: ga=504 off=504 gb=1
grids ua=1 ub=513 slots=512: ga=1 off=8 gb=511
grids ua=300 ub=300 slots=512: ga=256 off=256 gb=256
grids ua=504 ub=8 slots=512: ga=504 off=504 gb=8
grids ua=505 ub=8 slots=512: ga=505 off=512 gb=7
grids ua=1000 ub=3000 slots=512: ga=128 off=128 gb=384
grids ua=3 ub=5 slots=2: ga=1 off=8 gb=1
grids ua=7 ub=9 slots=0: ga=7 off=8 gb=9
"""


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/gemm_pair_dump.cpp"
    exe = str(tmp_path_factory.mktemp("pair") / "gemm_pair_dump")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr == ""   # no sanitizer report
    return r.stdout.splitlines()


def test_pairing_decisions_and_grids(dumped):
    want = EXPECTED.splitlines()
    assert len(dumped) == len(want)
    for got, exp in zip(dumped, want):
        assert got == exp


def test_only_the_step_pair_shares_a_launch(dumped):
    paired = [l.split(":")[0] for l in dumped if not l.startswith("grids") and not l.endswith("order=0")]
    assert paired == ["user_bwd", "user_bwd_swapped", "f32_partner", "adjacent_outputs"]


def test_every_problem_keeps_a_workgroup_and_its_xcd_alignment(dumped):
    for l in dumped:
        if l.startswith("grids"):
            f = dict(kv.split("=") for kv in l.replace(":", "").split()[1:])
            ga, off, gb, ua, ub = (int(f[k]) for k in ("ga", "off", "gb", "ua", "ub"))
            assert 1 <= ga <= ua and 1 <= gb <= ub and off % 8 == 0 and ga <= off < ga + 8
