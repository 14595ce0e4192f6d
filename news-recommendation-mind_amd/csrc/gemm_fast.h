// Internal: the validated GEMM call and the launcher of its fast-kernel routes (not part of the C ABI).
#pragma once
#include "gemm_route.h"

// One validated call: what gemm_route looks at plus the pointers only a launch needs.
struct GemmCall {
  nrfast::GemmProblem p;
  float* C;
  int64_t ldc;
  const float* bias;
  int64_t pad_row;
  const int32_t *m_dev, *k_dev;
  float *work, *colsum;
  int32_t* colsum_folded;
  hipStream_t stream;
};

// CUs of the current device (0 when there is none)
int nr_gemm_device_cus();
// Launches a GEMM_F32_64 / F32_128 / SPLIT_128 / BIG route, and the reductions it asks for.
int nr_gemm_fast(const GemmCall& c, const nrfast::GemmRoute& r);
// Launches two GEMM_F32_64 routes as one kernel: (a, b) in the order of nrfast::pair_modes.
int nr_gemm_fast_pair(const GemmCall& a, const nrfast::GemmRoute& ra, const GemmCall& b, const nrfast::GemmRoute& rb);
