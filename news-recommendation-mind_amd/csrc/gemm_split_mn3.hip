// bf16x6 launches with a MN-contiguous A operand (weight gradients).
#include "gemm_split_impl.h"

namespace nrfast {

int launch_split_mn3(const Args& g, const GemmRoute& r, hipStream_t s) {
  return launch_split_mn<3>(g, r, s);
}

}  // namespace nrfast
