// Internal: the validated GEMM call and the launcher of its fast-kernel routes (not part of the C ABI).
#pragma once
#include "gemm_route.h"

// One validated call: what gemm_route looks at (split_k at least 1 there), the caller's description
// for the pointers only a launch needs, and the stream.
struct GemmCall {
  nrfast::GemmProblem p;
  nr_gemm_desc d;
  hipStream_t stream;
};

// CUs of the current device (0 when there is none)
int nr_gemm_device_cus();
// Launches a GEMM_F32_64 / F32_128 / SPLIT_128 / BIG route, and the reductions it asks for.
int nr_gemm_fast(const GemmCall& c, const nrfast::GemmRoute& r);
// Launches two GEMM_F32_64 routes as one kernel: (a, b) in the order of nrfast::pair_modes.
int nr_gemm_fast_pair(const GemmCall& a, const nrfast::GemmRoute& ra, const GemmCall& b, const nrfast::GemmRoute& rb);
