// Large-tile bf16 GEMM instantiations: NP = 3 (bf16x6), BN = 128 (gemm_big_impl.h).
#include "gemm_big_impl.h"

namespace nrfast {

int launch_big_3_128(const Args& g, const GemmRoute& r, hipStream_t s) {
  return launch_big_modes<3, 128>(g, r, s);
}

}  // namespace nrfast
