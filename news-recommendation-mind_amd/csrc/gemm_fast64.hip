// 64x64-tile instantiations of the exact-f32 fast GEMM (small problems), a translation unit of
// their own so they compile in parallel with the 128x128 ones.
#include "gemm_fast_impl.h"

namespace nrfast {

int launch_modes64(const Args& g, const GemmRoute& r, hipStream_t s) {
  return launch_modes<64, 64>(g, r, s);
}

// Two independent problems in one launch: workgroups [0, ga) run problem a as a grid of ga, workgroups
// [off, off + gb) problem b as a grid of gb; those of [ga, off) (off = ga rounded up to the 8 XCDs, so
// that b's virtual ids keep their XCD: decode_unit) leave at once.  No workgroup waits for another.
struct PairArgs {
  Args a, b;
  int ga, off, gb;
};

constexpr int pair_max(int x, int y) { return x > y ? x : y; }

template <int BM, int BN, int AM1, int BMODE1, bool TR1, int AM2, int BMODE2, bool TR2>
__global__ __launch_bounds__(256, 2) void gemm_fast_pair_kernel(PairArgs p) {
  using LA1 = Loader<BM, AM1>;
  using LB1 = Loader<BN, BMODE1>;
  using LA2 = Loader<BM, AM2>;
  using LB2 = Loader<BN, BMODE2>;
  __shared__ __attribute__((aligned(16))) float lds[pair_max(2 * (LA1::LDS_FLOATS + LB1::LDS_FLOATS),
                                                             2 * (LA2::LDS_FLOATS + LB2::LDS_FLOATS))];
  static_assert(LA1::LDS_FLOATS % 4 == 0 && LA2::LDS_FLOATS % 4 == 0, "the B images stay 16-B aligned");
  const int b = (int)blockIdx.x;
  if (b < p.off) {
    if (b >= p.ga) return;
    gemm_fast_body<BM, BN, AM1, BMODE1, TR1>(p.a, b, p.ga, reinterpret_cast<float(*)[LA1::LDS_FLOATS]>(lds),
                                             reinterpret_cast<float(*)[LB1::LDS_FLOATS]>(lds + 2 * LA1::LDS_FLOATS));
  } else {
    gemm_fast_body<BM, BN, AM2, BMODE2, TR2>(p.b, b - p.off, p.gb, reinterpret_cast<float(*)[LA2::LDS_FLOATS]>(lds),
                                             reinterpret_cast<float(*)[LB2::LDS_FLOATS]>(lds + 2 * LA2::LDS_FLOATS));
  }
}

// The one instantiated pair (gemm_route.h pair_modes): a = an input gradient dx = dY W (K-contiguous
// dY, MN-contiguous W, transposed accumulators), b = a weight gradient dW += dYᵀ x (both operands
// MN-contiguous, C-major accumulators).  The caller (nr_gemm_fast_pair) has checked gemm_pair_order.
int launch_pair64(const Args& a, const Args& b, hipStream_t s) {
  auto kern = gemm_fast_pair_kernel<64, 64, KC_PLAIN, MN_PLAIN, true, MN_PLAIN, MN_PLAIN, false>;
  const int64_t ua = ((a.M + 63) / 64) * ((a.N + 63) / 64) * a.splits;
  const int64_t ub = ((b.M + 63) / 64) * ((b.N + 63) / 64) * b.splits;
  if (ua <= 0 || ub <= 0 || ua > 0x3fffffff || ub > 0x3fffffff) return NR_EINVAL(0);
  PairArgs p;
  p.a = a;
  p.b = b;
  pair_grids(ua, ub, resident_slots<256>(kern), p.ga, p.off, p.gb);
  hipLaunchKernelGGL(kern, dim3((unsigned)(p.off + p.gb)), dim3(256), 0, s, p);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

}  // namespace nrfast
