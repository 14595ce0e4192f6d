// Prints, for a table of problem pairs, whether nr_gemm_f32_pair runs them as one launch
// (csrc/gemm_route.h: gemm_pair_order, gemm_pair_alias) and how the launch's workgroups are shared
// (pair_grids).  Stand-alone and HIP-free, in the style of gemm_route_dump.cpp:
// tests/test_gemm_pair_route_cpu.py builds it with g++ under the address and undefined-behaviour
// sanitizers, runs it and compares the lines.
#include <stdio.h>

#include "../news-recommendation-mind_amd/csrc/gemm_route.h"

using namespace nrfast;

namespace {

// a 16 MB arena of addresses that are never read: every matrix of a problem at an offset of its own
float* at(int64_t mb) { return reinterpret_cast<float*>(0x10000000 + mb * (1 << 20)); }

enum { KC = NR_KCONTIG, MN = NR_MNCONTIG };

struct Prob {
  int64_t M, N, K;
  int la, lb;          // operand layouts
  int64_t lda, ldb;
  int epi, split_k, prec;
  const int32_t* m_dev;
  int max_cus;
  float *a, *b, *c;    // data addresses
  int64_t ldc;
  int map_b;
};

// the MHA user encoder's backward at the bench shapes: dx = dY W, dW += dYᵀ x (dY at 0 MB, 7.4 MB)
Prob dgrad() { return Prob{1600, 384, 1152, KC, MN, 1152, 384, NR_EPI_STORE, 1, NR_GEMM_BF16X6, nullptr, 0, at(0), at(8), at(10), 384, NR_ROWS_PLAIN}; }
Prob wgrad() { return Prob{1152, 384, 1600, MN, MN, 1152, 384, NR_EPI_ATOMIC, 3, NR_GEMM_BF16X6, nullptr, 0, at(0), at(13), at(16), 384, NR_ROWS_PLAIN}; }

void dump(const char* name, const Prob& x, const Prob& y) {
  static const int64_t rows[4] = {0, 1, 2, 3};
  const Prob* ps[2] = {&x, &y};
  nr_operand ops[2][2];
  GemmProblem gp[2];
  GemmRoute gr[2];
  GemmOut go[2];
  for (int i = 0; i < 2; ++i) {
    const Prob& p = *ps[i];
    ops[i][0] = nr_operand{p.a, p.lda, nullptr, NR_ROWS_PLAIN, 1, 1, p.la};
    ops[i][1] = nr_operand{p.b, p.ldb, p.map_b == NR_ROWS_PLAIN ? nullptr : rows, p.map_b, 1, 1, p.lb};
    const bool dyn = p.m_dev || p.max_cus;
    gp[i] = GemmProblem{p.M, p.N, p.K, &ops[i][0], &ops[i][1], nullptr, p.epi, p.split_k, p.prec, dyn, p.m_dev != nullptr,
                        p.max_cus, nullptr, 0, false};
    gr[i] = gemm_route(gp[i], 0);
    go[i] = GemmOut{p.c, p.ldc, nullptr};
  }
  printf("%s: families=%d,%d alias=%d order=%d\n", name, gr[0].family, gr[1].family,
         (int)gemm_pair_alias(gp[0], go[0], gp[1], go[1]), gemm_pair_order(gp[0], gr[0], go[0], gp[1], gr[1], go[1]));
}

void grids(int64_t ua, int64_t ub, int slots) {
  int ga, off, gb;
  pair_grids(ua, ub, slots, ga, off, gb);
  printf("grids ua=%lld ub=%lld slots=%d: ga=%d off=%d gb=%d\n", (long long)ua, (long long)ub, slots, ga, off, gb);
}

}  // namespace

int main() {
  static const int32_t MDEV = 0;
  Prob p;
  dump("user_bwd", dgrad(), wgrad());
  dump("user_bwd_swapped", wgrad(), dgrad());
  dump("two_dgrads", dgrad(), dgrad());                         // (both write at(10): alias, and not a mode pair)
  p = dgrad(); p.c = at(20);
  dump("two_dgrads_apart", dgrad(), p);                         // not an instantiated mode pair
  p = dgrad(); p.lb = KC; p.ldb = 1152;
  dump("forward_modes", p, wgrad());                            // K-contiguous W: the forward's kernel
  p = wgrad(); p.map_b = NR_ROWS_GATHER;
  dump("gathered_wgrad", dgrad(), p);                           // MN_GATHER B: instantiated alone, not as a pair
  p = dgrad(); p.max_cus = 64;
  dump("cu_cap", p, wgrad());
  p = wgrad(); p.m_dev = &MDEV;
  dump("device_extent", dgrad(), p);
  p = dgrad(); p.M = 52800;                                     // 128 x 128 tiles: another family
  dump("large_partner", p, wgrad());
  p = dgrad(); p.prec = NR_GEMM_BF16;                           // bf16 has no 64 x 64 kernel
  dump("bf16_partner", p, wgrad());
  p = dgrad(); p.prec = NR_GEMM_F32;
  dump("f32_partner", p, wgrad());
  p = dgrad(); p.lda = 1150; p.a = at(1);                       // ld % 4: the generic kernel
  dump("generic_partner", p, wgrad());
  p = dgrad(); p.c = at(13);                                    // dx over the weight gradient's x
  dump("alias_operand", p, wgrad());
  p = wgrad(); p.c = at(9);                                     // dW inside the input gradient's W (1.7 MB at 8 MB)
  dump("alias_operand_2", dgrad(), p);
  p = wgrad(); p.c = at(10);                                    // one output
  dump("alias_output", dgrad(), p);
  p = dgrad(); p.c = reinterpret_cast<float*>(reinterpret_cast<char*>(at(16)) + 1152 * 384 * 4);
  dump("adjacent_outputs", p, wgrad());                         // dx right behind dW: no overlap

  grids(150, 324, 512);    // the step: 152 + 324 workgroups
  grids(2, 2, 512);
  grids(1, 1, 512);
  grids(513, 1, 512);      // capped: b keeps one workgroup, a 504 (a multiple of 8)
  grids(1, 513, 512);
  grids(300, 300, 512);
  grids(504, 8, 512);      // fits exactly
  grids(505, 8, 512);      // 512 + 8 > 512: capped
  grids(1000, 3000, 512);
  grids(3, 5, 2);          // fewer slots than problems' minimum: one workgroup each
  grids(7, 9, 0);          // slots unknown: uncapped
  return 0;
}
