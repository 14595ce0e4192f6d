// The exact-f32 fast GEMM kernel (persistent, two-deep pipelined) and its launchers, included by
// gemm_fast.hip (128x128 tiles + the entry point) and gemm_fast64.hip (64x64 tiles) so the
// instantiations compile in parallel.
#pragma once
#include "gemm_fast_common.h"

namespace nrfast {


// Persistent GEMM: a grid of (resident blocks) walks the units with stride gridDim.x, and the
// k-loop runs over the flattened (unit, k-tile) sequence.  Two-deep pipeline per block: while
// the MFMAs consume k-tile P from LDS, tile P+1 sits in registers and is written to the other
// LDS buffer after the first quarter of P's MFMAs, and the global loads of P+2 are issued right
// behind that write — so a load has a whole iteration to land, the LDS write never waits, and
// each iteration ends in a bare barrier.  Unit boundaries are invisible to the pipeline: the
// next unit's first tiles load during the current unit's last ones, and the finished unit's
// epilogue stores go out behind them.  A grid of `units` blocks is the plain one-tile-per-block
// kernel.
// The body takes its place in the grid as arguments (`bid` of `G` workgroups, the LDS images from the
// caller), so that one launch can run two problems side by side (gemm_fast_pair_kernel): each problem
// sees a grid of its own and walks its units in the order it has alone.
template <int BM, int BN, int AM, int BMODE, bool TR>
__device__ __forceinline__ void gemm_fast_body(Args g, const int bid, const int G,
                                               float (*As)[Loader<BM, AM>::LDS_FLOATS],
                                               float (*Bs)[Loader<BN, BMODE>::LDS_FLOATS]) {
  using LA = Loader<BM, AM>;
  using LB = Loader<BN, BMODE>;
  constexpr bool IDX_AHEAD = AM == MN_GATHER || BMODE == MN_GATHER;

  clamp_extents(g);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, c = lane & 31;
  const int gn = (int)((g.N + BN - 1) / BN);
  const int ntiles = (int)((g.M + BM - 1) / BM) * gn;
  const int units = ntiles * g.splits;
#define NR_WALK_PART 1   // the unit walk: cp (or return), advance, peek_k
#include "gemm_walk.h"

  constexpr int TI = BM / 64, TJ = BN / 64;
  const int wm = (w >> 1) * (BM / 2), wn = (w & 1) * (BN / 2);
  f32x16 acc[TI][TJ];
  zero_acc(acc);

  // prologue: P0 -> LDS[0], P1 -> registers
  LA la;
  LB lb;
#define NR_WALK_PART 2   // the load position: lp, step_load; P0's loads issued
#include "gemm_walk.h"
  la.store(As[0], tid);
  lb.store(Bs[0], tid);
  bool staged = step_load();   // registers hold the position after cp
  __syncthreads();

  bool pending = false;
  int64_t pm0 = 0, pn0 = 0;
  int buf = 0;
  for (;;) {
    if (pending) {   // previous unit's output, behind this unit's first loads
      epilogue_any<TR, TI, TJ>(g, acc, pm0, pn0, wm, wn, h, c);
      zero_acc(acc);
      pending = false;
    }
    const float* a_s = As[buf];
    const float* b_s = Bs[buf];
    const bool had_staged = staged;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float4 a[TI], b[TJ];
#pragma unroll
      for (int i = 0; i < TI; ++i) a[i] = la.frag(a_s, wm + 32 * i + c, h, q);
#pragma unroll
      for (int j = 0; j < TJ; ++j) b[j] = lb.frag(b_s, wn + 32 * j + c, h, q);
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
          acc[i][j] = TR ? __builtin_amdgcn_mfma_f32_32x32x2f32(b[j].x, a[i].x, acc[i][j], 0, 0, 0)
                         : __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].x, b[j].x, acc[i][j], 0, 0, 0);
          acc[i][j] = TR ? __builtin_amdgcn_mfma_f32_32x32x2f32(b[j].y, a[i].y, acc[i][j], 0, 0, 0)
                         : __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].y, b[j].y, acc[i][j], 0, 0, 0);
          acc[i][j] = TR ? __builtin_amdgcn_mfma_f32_32x32x2f32(b[j].z, a[i].z, acc[i][j], 0, 0, 0)
                         : __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].z, b[j].z, acc[i][j], 0, 0, 0);
          acc[i][j] = TR ? __builtin_amdgcn_mfma_f32_32x32x2f32(b[j].w, a[i].w, acc[i][j], 0, 0, 0)
                         : __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].w, b[j].w, acc[i][j], 0, 0, 0);
        }
      if (q == 0 && had_staged) {   // publish P+1 (its buffer's readers passed the last barrier)
        la.store(As[buf ^ 1], tid);
        lb.store(Bs[buf ^ 1], tid);
        staged = step_load();       // and start P+2
      }
    }
    __syncthreads();
    buf ^= 1;
    const int old = cp.id;
    const int64_t om0 = cp.u.m0, on0 = cp.u.n0;
    if (!had_staged) break;         // cp was the block's last position
    advance(cp);
    if (cp.id != old) {
      pending = true;
      pm0 = om0;
      pn0 = on0;
    }
  }
  epilogue_any<TR, TI, TJ>(g, acc, cp.u.m0, cp.u.n0, wm, wn, h, c);
}

template <int BM, int BN, int AM, int BMODE, bool TR>
__global__ __launch_bounds__(256, 2) void gemm_fast_kernel(Args g) {
  __shared__ __attribute__((aligned(16))) float As[2][Loader<BM, AM>::LDS_FLOATS];
  __shared__ __attribute__((aligned(16))) float Bs[2][Loader<BN, BMODE>::LDS_FLOATS];
  gemm_fast_body<BM, BN, AM, BMODE, TR>(g, (int)blockIdx.x, (int)gridDim.x, As, Bs);
}

template <int BM, int BN>
int launch_modes(const Args& g, const GemmRoute& r, hipStream_t s) {
#define NR_KERN(A_, B_, TR_) gemm_fast_kernel<BM, BN, A_, B_, TR_>
#define NR_ROW(A_, B_, TR_) NR_LAUNCH_ROW(256, BM, BN, A_, B_, TR_)
  NR_MODES_KC(NR_ROW) NR_MODES_MN(NR_ROW)
#undef NR_ROW
#undef NR_KERN
  return NR_EINVAL(7);
}

}  // namespace nrfast
