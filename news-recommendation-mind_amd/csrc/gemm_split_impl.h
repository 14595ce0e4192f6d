// bf16 matrix-core GEMM kernels (NR_GEMM_BF16X6: NP = 3 planes, six products; NR_GEMM_BF16: NP = 1,
// one product), included by the gemm_split_*.hip translation units so the instantiations compile in
// parallel.  Shared code: gemm_fast_common.h.
#pragma once
#include <type_traits>

#include "gemm_fast_common.h"

namespace nrfast {

// bf16x6 form of gemm_fast_kernel (128x128 tiles, the same persistent two-deep pipeline and
// epilogues): the loaders split each fp32 element into three bf16 planes as they publish a
// k-tile to LDS (K-contiguous operands as loaded, MN-contiguous ones through a 4x4 register
// transpose), and each 16-deep k-step runs six v_mfma_f32_32x32x16_bf16 per 32x32 output tile,
// smallest terms first.  The accumulators have the f32 MFMA's C/D layout, so the epilogues are
// shared.  One LDS image (60 KiB) so two workgroups share a CU: tile P+1 waits in registers while
// P computes, is published between two barriers, and P+2's loads go out right behind it.
// NP = 1 (bf16 arithmetic): the same pipeline with one plane per operand and one MFMA per
// 32x32 tile and k-step (fp32 operands rounded to bf16 on the way to LDS, fp32 accumulation).
template <int AM, int BMODE, bool TR, int NP>
__global__ __launch_bounds__(256, 2) void gemm_split_kernel(Args g) {
  using LA = typename std::conditional<is_kc(AM), Loader<128, AM>, MNBlk<AM>>::type;
  using LB = typename std::conditional<is_kc(BMODE), Loader<128, BMODE>, MNBlk<BMODE>>::type;
  constexpr int BM = 128, BN = 128;
  __shared__ __attribute__((aligned(16))) uint16_t As[NP * SPL];
  __shared__ __attribute__((aligned(16))) uint16_t Bs[NP * SPL];
  constexpr bool IDX_AHEAD = AM == MN_GATHER || BMODE == MN_GATHER;

  clamp_extents(g);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, c = lane & 31;
  const int gn = (int)((g.N + BN - 1) / BN);
  const int ntiles = (int)((g.M + BM - 1) / BM) * gn;
  const int units = ntiles * g.splits;
  const int G = gridDim.x;
  const unsigned bid = blockIdx.x;
#define NR_WALK_PART 1   // the unit walk: cp (or return), advance, peek_k
#include "gemm_walk.h"

  constexpr int TI = 2, TJ = 2;
  const int wm = (w >> 1) * (BM / 2), wn = (w & 1) * (BN / 2);
  f32x16 acc[TI][TJ];
  zero_acc(acc);

  LA la;
  LB lb;
#define NR_WALK_PART 2   // the load position: lp, step_load; P0's loads issued
#include "gemm_walk.h"
  la.template store_split<NP>(As, tid);
  lb.template store_split<NP>(Bs, tid);
  bool staged = step_load();
  __syncthreads();

  bool pending = false;
  int64_t pm0 = 0, pn0 = 0;
  for (;;) {
    if (pending) {
      epilogue_any<TR, TI, TJ>(g, acc, pm0, pn0, wm, wn, h, c);
      zero_acc(acc);
      pending = false;
    }
    const uint16_t* a_s = As;
    const uint16_t* b_s = Bs;
    const bool had_staged = staged;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 a[TI][NP], b[TJ][NP];
      const int ko = 16 * s + 8 * h;
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int p = 0; p < NP; ++p)
          a[i][p] = *reinterpret_cast<const bf16x8*>(a_s + p * SPL + (wm + 32 * i + c) * SROW + ko);
#pragma unroll
      for (int j = 0; j < TJ; ++j)
#pragma unroll
        for (int p = 0; p < NP; ++p)
          b[j][p] = *reinterpret_cast<const bf16x8*>(b_s + p * SPL + (wn + 32 * j + c) * SROW + ko);
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) mfma_planes<NP, TR>(acc[i][j], a[i], b[j]);
    }
    __syncthreads();                // every wave is done reading P
    const int old = cp.id;
    const int64_t om0 = cp.u.m0, on0 = cp.u.n0;
    if (!had_staged) break;
    la.template store_split<NP>(As, tid);   // publish P+1 (its loads landed during P's MFMAs)
    lb.template store_split<NP>(Bs, tid);
    staged = step_load();           // and start P+2
    __syncthreads();
    advance(cp);
    if (cp.id != old) {
      pending = true;
      pm0 = om0;
      pn0 = on0;
    }
  }
  epilogue_any<TR, TI, TJ>(g, acc, cp.u.m0, cp.u.n0, wm, wn, h, c);
}

#define NR_KERN(A_, B_, TR_) gemm_split_kernel<A_, B_, TR_, NP>
#define NR_ROW(A_, B_, TR_) NR_LAUNCH_ROW(256, 128, 128, A_, B_, TR_)
// K-contiguous A operand (projections, dgrads)
template <int NP>
int launch_split_kc(const Args& g, const GemmRoute& r, hipStream_t s) {
  NR_MODES_KC(NR_ROW)
  return NR_EINVAL(7);
}

// MN-contiguous A operand (weight gradients)
template <int NP>
int launch_split_mn(const Args& g, const GemmRoute& r, hipStream_t s) {
  // the rows of NR_MODES_MN, in the order this unit has always instantiated them
  NR_ROW(MN_PLAIN, MN_GATHER, false)
  NR_ROW(MN_PLAIN, MN_PLAIN, false)
  NR_ROW(MN_PLAIN, MN_CONV3, false)
  return NR_EINVAL(7);
}
#undef NR_ROW
#undef NR_KERN

}  // namespace nrfast
