// Fast path of nr_gemm_f32: the same contraction as gemm_f32.hip with every operand mode a
// compile-time parameter, branch-free loads and per-tile row pointers hoisted out of the
// k-loop (gather / conv3 token rows are constant along k), so the loop body is loads, LDS
// stores and MFMAs only.
//
// LDS images, by operand layout:
//   K-contiguous operand (rows = M/N index, k contiguous in memory): [row][k], stride 36
//     floats — a 16-B ds_write per float4 and ONE ds_read_b128 per 4 MFMA k-steps; the
//     32-row lane groups of a b128 read hit 16 distinct 16-B slots (36/4 = 9 is odd).
//   MN-contiguous operand (rows = k): [k][row], stride R+4 — a 16-B store per float4 and
//     four ds_read_b32 per 4 k-steps (lanes read consecutive rows: conflict-free).
// MFMA k-step s (0..15) of a 32-deep tile reads k = 16*half + s in BOTH operands (the sum over
// k is order-free), which is what makes the b128 fragment read possible.
//
// Requirements (checked by gemm_route, gemm_route.h; else the generic kernel runs): data 16-B aligned,
// ld % 4 == 0, MN-contiguous operands with ld >= round4(M or N) (reads stay inside padded
// rows), conv3 seg % 32 == 0 and seg % BN == 0 where the taps run along N.
#include <stdlib.h>

#include "gemm_fast.h"

#include "gemm_fast_impl.h"

namespace nrfast {

// Split-K slabs -> C: C[m][n] += sum over the valid splits of slab[s][m][n], in split order
// (deterministic).  The valid split count and row count follow the GEMM kernel's own reading of
// the device-resident K / M (a split whose k range starts past the device K wrote nothing).
__global__ __launch_bounds__(256) void splitk_reduce_kernel(float* __restrict__ C, int64_t ldc,
                                                            const float* __restrict__ slab, int64_t ld,
                                                            int64_t stride, int splits, int64_t M, int64_t N,
                                                            int64_t K, int64_t kchunk, const int32_t* mdyn,
                                                            const int32_t* kdyn, int vec, float* __restrict__ colsum) {
  const int64_t m_eff = mdyn ? clamp_extent(M, *mdyn) : M;
  if (kdyn) {   // as clamp_extents does in the GEMM kernel
    K = clamp_extent(K, *kdyn);
    kchunk = k_chunk(K, splits);
  }
  const int64_t nk = k_chunks(K, kchunk);
  const int ns = nk < splits ? (int)nk : splits;
  const int64_t n4 = (N + 3) / 4, total = m_eff * n4;
  if (colsum) {   // the fused bias gradient: per-split column sums after the partial tiles
    const float* cs = slab + (int64_t)splits * stride;
    const int64_t mh = stride / ld;
    for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < m_eff; m += (int64_t)gridDim.x * 256) {
      float a = colsum[m];
      for (int sp = 0; sp < ns; ++sp) a += cs[sp * mh + m];
      colsum[m] = a;
    }
  }
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t m = i / n4, n = 4 * (i - m * n4);
    const float* s = slab + m * ld + n;
    float* c = C + m * ldc + n;
    if (vec && n + 3 < N) {
      float4 a = *reinterpret_cast<const float4*>(c);
#pragma unroll 4
      for (int sp = 0; sp < ns; ++sp) {
        const float4 x = *reinterpret_cast<const float4*>(s + sp * stride);
        a.x += x.x; a.y += x.y; a.z += x.z; a.w += x.w;
      }
      *reinterpret_cast<float4*>(c) = a;
    } else {
      for (int e = 0; e < 4 && n + e < N; ++e) {
        float a = c[e];
        for (int sp = 0; sp < ns; ++sp) a += s[sp * stride + e];
        c[e] = a;
      }
    }
  }
}

// The big kernel's stream-K tail through its workspace (tail_slab_tr): every tail tile's pieces added
// in piece order (deterministic) and stored to the tile's distinct destination rows (rows[m]; pad_row
// and rows past the device-resident M skipped), the plan read from the header the GEMM wrote.
__global__ __launch_bounds__(256) void tail_reduce_kernel(float* __restrict__ C, int64_t ldc,
                                                          const float* __restrict__ ws, const int64_t* __restrict__ rows,
                                                          int64_t pad_row, int64_t M, const int32_t* mdyn, int64_t N,
                                                          int vec) {
  const int* hd = reinterpret_cast<const int*>(ws);
  const int full = hd[0], rem = hd[1], pieces = hd[2], gn = hd[3];
  if (pieces <= 1 || rem <= 0 || gn <= 0) return;
  const int64_t m_eff = mdyn ? clamp_extent(M, *mdyn) : M;
  const float* part = ws + TAIL_WS_HDR;
  const int64_t total = (int64_t)rem * 256 * 64;   // float4 of the rem tail tiles
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int t = (int)(e >> 14), w = (int)(e & 16383), r = w >> 6, c4 = w & 63;
    const int tile = full + t;
    const int64_t m = (int64_t)(tile / gn) * 256 + r, n = (int64_t)(tile % gn) * 256 + 4 * c4;
    if (m >= m_eff || n >= N) continue;
    const int64_t tok = rows[m];
    if (tok == pad_row) continue;
    const float* s = part + (int64_t)t * 65536 + r * 256 + 4 * c4;
    float4 a = *reinterpret_cast<const float4*>(s);
    for (int q = 1; q < pieces; ++q) {
      const float4 x = *reinterpret_cast<const float4*>(s + (int64_t)q * rem * 65536);
      a.x += x.x; a.y += x.y; a.z += x.z; a.w += x.w;
    }
    float* c = C + tok * ldc + n;
    if (vec && n + 3 < N) {
      *reinterpret_cast<float4*>(c) = a;
    } else {
      const float v[4] = {a.x, a.y, a.z, a.w};
      for (int u = 0; u < 4 && n + u < N; ++u) c[u] = v[u];
    }
  }
}

}  // namespace nrfast

// Elements of nr_gemm_f32_ws' split-K workspace that serve any shape: one round of 256 x 256
// partial tiles over the device's CUs (the big kernel re-splits a split-K contraction to one unit
// per CU), plus row padding and the per-split column sums.
extern "C" int64_t nr_gemm_splitk_workspace(void) {
  const int cus = nrfast::device_cus();
  return (int64_t)(cus > 0 ? cus : 256) * 256 * 261;
}


int nr_gemm_device_cus() { return nrfast::device_cus(); }

namespace {
// the kernel arguments of a routed call
nrfast::Args make_args(const GemmCall& c, const nrfast::GemmRoute& r) {
  using namespace nrfast;
  const GemmProblem& p = c.p;
  const nr_operand *A = p.A, *B = p.B, *cr = p.c_rows;
  Args g;
  g.M = p.M; g.N = p.N; g.K = p.K;
  g.A = Op{A->data, A->ld, A->rows, A->seq_len, A->seg};
  g.B = Op{B->data, B->ld, B->rows, B->seq_len, B->seg};
  g.Cm = Op{cr ? cr->data : nullptr, cr ? cr->ld : 0, cr ? cr->rows : nullptr,
            cr ? (cr->map == NR_ROWS_CONV3 ? cr->seq_len : 1) : 1, cr ? cr->seg : 1};
  g.C = c.d.C; g.ldc = c.d.ldc; g.bias = c.d.bias; g.epi = r.epi; g.pad_row = c.d.pad_row;
  g.mdyn = c.d.m_dev; g.kdyn = c.d.k_dev; g.max_cus = p.max_cus > 0 ? p.max_cus : 0;
  g.splits = r.splits; g.kchunk = r.kchunk; g.tail = r.tail;
  {
    bool v = p.N % 4 == 0 && c.d.ldc % 4 == 0 && aligned16(c.d.C) && (!c.d.bias || aligned16(c.d.bias));
    if (r.epi == NR_EPI_ACCUM_GATE || r.epi == NR_EPI_STORE_GELU || r.epi == NR_EPI_GELU_GRAD)
      v = v && cr && cr->ld % 4 == 0 && aligned16(cr->data);
    g.vec = v ? 1 : 0;
  }
  const int64_t sld = (p.N + 3) & ~int64_t(3);
  if (r.tail_ws) {
    g.slab = c.d.work;
    g.tail_cap = r.tail_cap;
  }
  if (r.slab) {
    g.slab = c.d.work;
    g.slab_ld = sld;
    g.slab_stride = p.M * sld;
    g.colsum = r.fold ? c.d.colsum : nullptr;
  }
  return g;
}
}  // namespace

int nr_gemm_fast_pair(const GemmCall& a, const nrfast::GemmRoute& ra, const GemmCall& b, const nrfast::GemmRoute& rb) {
  if (ra.family != nrfast::GEMM_F32_64 || rb.family != nrfast::GEMM_F32_64 || !nrfast::pair_modes(ra, rb))
    return NR_EINVAL(7);
  return nrfast::launch_pair64(make_args(a, ra), make_args(b, rb), a.stream);
}

int nr_gemm_fast(const GemmCall& c, const nrfast::GemmRoute& r) {
  using namespace nrfast;
  const GemmProblem& p = c.p;
  const Args g = make_args(c, r);
  const int64_t sld = (p.N + 3) & ~int64_t(3);
  int rc;
  switch (r.family) {
    case GEMM_F32_64: return launch_modes64(g, r, c.stream);
    case GEMM_F32_128: return launch_modes<128, 128>(g, r, c.stream);
    case GEMM_SPLIT_128:
      if (is_kc(r.am)) return r.planes == 1 ? launch_split_kc1(g, r, c.stream) : launch_split_kc3(g, r, c.stream);
      return r.planes == 1 ? launch_split_mn1(g, r, c.stream) : launch_split_mn3(g, r, c.stream);
    case GEMM_BIG:
      rc = r.bn == 256 ? (r.planes == 1 ? launch_big_1_256(g, r, c.stream) : launch_big_3_256(g, r, c.stream))
                       : (r.planes == 1 ? launch_big_1_128(g, r, c.stream) : launch_big_3_128(g, r, c.stream));
      break;
    default: return NR_EINVAL(7);
  }
  if (rc != NR_OK) return rc;
  if (r.tail_ws) {
    hipLaunchKernelGGL(tail_reduce_kernel, dim3(1024), dim3(256), 0, c.stream, c.d.C, c.d.ldc, c.d.work, g.Cm.idx,
                       g.pad_row, p.M, c.d.m_dev, p.N, g.vec);
    NR_LAUNCH_CHECK();
  }
  if (r.slab) {
    int64_t blocks = (p.M * ((p.N + 3) / 4) + 255) / 256;
    blocks = blocks > 2048 ? 2048 : (blocks < 1 ? 1 : blocks);
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, c.stream, c.d.C, c.d.ldc, c.d.work, sld,
                       g.slab_stride, r.splits, p.M, p.N, p.K, r.kchunk, c.d.m_dev, c.d.k_dev, g.vec, g.colsum);
    NR_LAUNCH_CHECK();
    if (r.fold && c.d.colsum_folded) *c.d.colsum_folded = 1;
  }
  return NR_OK;
}
