// bf16x6 launches with a K-contiguous A operand (projections, dgrads).
#include "gemm_split_impl.h"

namespace nrfast {

int launch_split_kc3(const Args& g, const GemmRoute& r, hipStream_t s) {
  return launch_split_kc<3>(g, r, s);
}

}  // namespace nrfast
