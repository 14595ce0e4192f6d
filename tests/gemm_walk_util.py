"""Shared by tests/test_gemm_walk_gpu.py and tests/test_gemm_route_cpu.py: the cases that make one
workgroup of a fast GEMM kernel walk several units (csrc/gemm_walk.h, the walk gemm_fast_body and
gemm_split_kernel share; the big kernel's own unit loop), each with its line of arguments for
tests/gemm_route_dump.cpp, so that the kernel a case means is pinned without a GPU.  Shapes, inputs and bars are gemm_epi_util's.

A positive max_cus caps the persistent grid at that many CUs' worth of resident workgroups
(capped_slots): two workgroups per CU on the 128 x 128 kernels, one on the 256 x 256 kernel."""
import collections

import gemm_epi_util as U
from newsrec_amd import _lib as L

# 3 x 2 tiles of 128 (2 x 2 live under m_dev = 200): max_cus = 1 -> two workgroups walk six units
WALK = U.Shape("walk", 384, 96, 256, None, 96, 96, 256, 200)
# the big kernel's split-K: 2 x 1 tiles of 256, K = 3 x 512
WALK_BIG_K = U.Shape("walk_big_k", 512, 1536, 256, None, 512, None, 256, 300)
# 34 x 34 = 1156 tiles of 64 against at most 1024 resident workgroups (256 CUs x 4)
WALK_64 = U.Shape("walk_64", 2176, 64, 2176, None, 64, 64, None, None)

Case = collections.namedtuple("Case", "id kernel n a_layout b_layout epi split_k max_cus k_dev")


def _k(kid, family, tile, planes, form, prec, shape):
    return U.Kernel(kid, family, tile, planes, form, prec, shape)


# store epilogue, the whole K: C must not depend on the grid
STORE_CASES = [
    Case("f32_128", _k("walk-f32_128", "f32_128", 128, 0, "dyn", "f32", WALK), 256, "kc", "kc",
         L.EPI_STORE, 1, 1, None),
    Case("split_128_3", _k("walk-split_128_3", "split_128", 128, 3, "dyn", "bf16x6", WALK), 256, "kc", "kc",
         L.EPI_STORE, 1, 1, None),
    # gemm_epi_util.BIG: 7 live tile rows x 4 = 28 units on one workgroup
    Case("big_3", U.KERNEL["big_3-mdev"], 1024, "kc", "kc", L.EPI_STORE, 1, 1, None),
]

# NR_EPI_ATOMIC, split_k = 3, k_dev = 32: splits 1 and 2 are empty on the device.  The 128 x 128
# kernels walk 4 live tiles x 3 splits on two workgroups.  The big kernel is re-split to one unit per CU
# it may use (gemm_route.h: want = max_cus / tiles, at least 512 k each), so it never has more units than
# workgroups: max_cus = 6 gives 2 tiles x 3 splits on six workgroups, four of which find an empty split.
ATOMIC_CASES = [
    Case("f32_128", _k("walk-f32_128-mdev", "f32_128", 128, 0, "mdev", "f32", WALK), 256, "kc", "mn", L.EPI_ATOMIC, 3,
         1, 32),
    Case("split_128_3", _k("walk-split_128_3-mdev", "split_128", 128, 3, "mdev", "bf16x6", WALK), 256, "kc", "mn",
         L.EPI_ATOMIC, 3, 1, 32),
    Case("big_3", _k("walk-big_3-mdev", "big", 256, 3, "mdev", "bf16x6", WALK_BIG_K), 256, "mn", "mn", L.EPI_ATOMIC, 3,
         6, 32),
]

# static form: more units than resident workgroups, so some walk two
STATIC_CASE = Case("f32_64", _k("walk-f32_64", "f32_64", 64, 0, "static", "f32", WALK_64), 2176, "kc", "kc",
                   L.EPI_STORE, 1, 0, None)

ALL_CASES = STORE_CASES + ATOMIC_CASES + [STATIC_CASE]


def round4(n):
    return (n + 3) // 4 * 4


def lda(case):
    s = case.kernel.shape
    return s.lda if case.a_layout == "kc" else round4(s.M)


def ldb(case):
    s = case.kernel.shape
    return s.ldb_kc if case.b_layout == "kc" else s.ldb_mn


def route_argv(case):
    s = case.kernel.shape
    argv = [case.kernel.id, str(s.M), str(case.n), str(s.K), case.a_layout, str(lda(case)), case.b_layout,
            str(ldb(case)), str(case.epi), case.kernel.form, case.kernel.prec]
    if case.split_k > 1:
        argv.append("split=%d" % case.split_k)
    if case.max_cus:
        argv.append("cus=%d" % case.max_cus)
    return argv


def route_fields(case):
    k = case.kernel
    mode = {"kc": 0, "mn": 3}
    return {"family": k.family, "tile": "%dx%d" % (k.tile, k.tile), "planes": str(k.planes),
            "modes": "%d,%d" % (mode[case.a_layout], mode[case.b_layout]), "epi": str(case.epi),
            "splits": str(case.split_k), "slab": "0", "tail": "0"}
