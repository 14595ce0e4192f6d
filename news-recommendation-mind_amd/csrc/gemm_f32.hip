// fp32 GEMM on the CDNA4 f32-input matrix cores (v_mfma_f32_32x32x2_f32: exact f32,
// 64 FLOP/clk/SIMD, the same rate as the f32 VALU but with one VGPR per operand per lane).
//
// It carries every dense contraction of the news / user towers:
//   * the MHA key/value projections   (models/Modules/Attention.py:107-108, :125-127)
//   * the k=3 Conv1d of the CNN encoder as a GEMM with K = 3E  (models/Encoders/CNN.py:12-17,41)
//   * their backward dgrad / wgrad     (autograd of the above)
// The word-embedding gather (models/Embeddings/BERT.py:39) is FUSED into the operand loader:
// an operand row can be a token id's row of the [V, E] table (GATHER), or the three
// neighbouring tokens of a k=3 convolution with zero padding at the title ends (CONV3), so the
// [T, 768] embedding activations are never written to HBM.  The dgrad epilogue scatters
// straight back into the dense [V, E] table gradient with no-return f32 atomics, skipping the
// padding row (nn.Embedding padding_idx=0).
//
// Tile: BM x BN x 32, 256 threads = 4 waves in 2x2, each wave (BM/2) x (BN/2) of 32x32 MFMA
// tiles.  Operands are register-staged into a double-buffered LDS image laid out [k][m]
// (m contiguous) so each lane's fragment is one ds_read_b32 per k-pair; the next tile's global
// loads are issued before the current tile's MFMAs.  Blocks are remapped XCD-aware so that the
// column tiles of one row panel run on the same XCD and share its L2.
#include "common.h"
#include "../../include/newsrec_hip.h"
#include "gemm_fast.h"
#include <stdlib.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

struct Op {
  const float* base;
  int64_t ld;
  const int64_t* idx;
  int map;
  int L;
  int seg;
  int vec;   // rows 16-B aligned: float4 loads; else scalar loads
};

__device__ __forceinline__ const float* row_ptr(const Op& d, int64_t r, int j) {
  if (d.map == NR_ROWS_PLAIN) return d.base + r * d.ld;
  if (d.map == NR_ROWS_GATHER) return d.base + d.idx[r] * d.ld;
  // CONV3: row r = (news n, position t); tap j reads position t + j - 1 (zero outside)
  int64_t n = r / d.L;
  int t2 = (int)(r - n * d.L) + j - 1;
  if (t2 < 0 || t2 >= d.L) return nullptr;
  return d.base + d.idx[n * d.L + t2] * d.ld;
}

struct Args {
  int64_t M, N, K;
  Op A, B, Cm;
  float* C;
  int64_t ldc;
  const float* bias;
  int epi;
  int64_t pad_row;
  int64_t kchunk;
};

// Loads one operand tile (R rows of the M/N side x 32 k) into registers.
// KC = true : element (r, k) stored at row_ptr(r)[k]  (k contiguous)
// KC = false: element (r, k) stored at row_ptr(k)[r]  (r contiguous)
template <int R, bool KC>
struct Tile {
  static constexpr int BK = 32;
  static constexpr int NV = R / 32;                 // float4 per thread
  static constexpr int S = KC ? R + 1 : R + 4;      // LDS row stride ([k][r] image)
  float4 v[NV];

  __device__ __forceinline__ void load(const Op& d, int64_t r0, int64_t rlim, int64_t k0,
                                       int64_t K, int tid) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int f = tid + 256 * i;
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (KC) {
        const int r = f >> 3, kq = f & 7;
        const int64_t row = r0 + r, k = k0 + 4 * kq;
        const int j = d.map == NR_ROWS_CONV3 ? (int)(k0 / d.seg) : 0;
        if (row < rlim && k < K) {
          const float* p = row_ptr(d, row, j);
          if (p) {
            p += k - (int64_t)j * d.seg;
            if (k + 3 < K && d.vec) {
              x = *reinterpret_cast<const float4*>(p);
            } else if (k + 3 < K) {
              x.x = p[0]; x.y = p[1]; x.z = p[2]; x.w = p[3];
            } else {
              x.x = p[0];
              if (k + 1 < K) x.y = p[1];
              if (k + 2 < K) x.z = p[2];
            }
          }
        }
      } else {
        constexpr int CPR = R / 4;                    // float4 per k-row
        const int kr = f / CPR, c4 = f % CPR;
        const int64_t k = k0 + kr, col = r0 + 4 * c4;
        const int j = d.map == NR_ROWS_CONV3 ? (int)(r0 / d.seg) : 0;
        if (k < K && col < rlim) {
          const float* p = row_ptr(d, k, j);
          if (p) {
            p += col - (int64_t)j * d.seg;
            if (col + 3 < rlim && d.vec) {
              x = *reinterpret_cast<const float4*>(p);
            } else if (col + 3 < rlim) {
              x.x = p[0]; x.y = p[1]; x.z = p[2]; x.w = p[3];
            } else {
              x.x = p[0];
              if (col + 1 < rlim) x.y = p[1];
              if (col + 2 < rlim) x.z = p[2];
            }
          }
        }
      }
      v[i] = x;
    }
  }

  __device__ __forceinline__ void store(float* lds, int tid) const {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int f = tid + 256 * i;
      if (KC) {
        const int r = f >> 3, kq = f & 7;
        lds[(4 * kq + 0) * S + r] = v[i].x;
        lds[(4 * kq + 1) * S + r] = v[i].y;
        lds[(4 * kq + 2) * S + r] = v[i].z;
        lds[(4 * kq + 3) * S + r] = v[i].w;
      } else {
        constexpr int CPR = R / 4;
        const int kr = f / CPR, c4 = f % CPR;
        *reinterpret_cast<float4*>(&lds[kr * S + 4 * c4]) = v[i];
      }
    }
  }
};

template <int BM, int BN, bool AK, bool BKC>
__global__ __launch_bounds__(256, 2) void gemm_f32_kernel(Args g) {
  constexpr int BK = 32;
  using TA = Tile<BM, AK>;
  using TB = Tile<BN, BKC>;
  __shared__ __attribute__((aligned(16))) float As[2][BK * TA::S];
  __shared__ __attribute__((aligned(16))) float Bs[2][BK * TB::S];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t gm = (g.M + BM - 1) / BM, gn = (g.N + BN - 1) / BN;
  const int nwg = (int)(gm * gn);
  const int id = blockIdx.x;
  // bijective XCD remap: blocks id, id+8, ... share an XCD; give them consecutive tiles
  const int xcd = id & 7, q = nwg >> 3, rr = nwg & 7;
  const int wg = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (id >> 3);
  const int64_t m0 = (wg / gn) * BM, n0 = (wg % gn) * BN;

  const int64_t kbeg = (int64_t)blockIdx.y * g.kchunk;
  const int64_t kend = kbeg + g.kchunk < g.K ? kbeg + g.kchunk : g.K;
  const int nt = kend > kbeg ? (int)((kend - kbeg + BK - 1) / BK) : 0;

  constexpr int TI = BM / 64, TJ = BN / 64;
  const int wm = (w >> 1) * (BM / 2), wn = (w & 1) * (BN / 2);
  f32x16 acc[TI][TJ];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  TA ta;
  TB tb;
  if (nt > 0) {
    ta.load(g.A, m0, g.M, kbeg, g.K, tid);
    tb.load(g.B, n0, g.N, kbeg, g.K, tid);
    ta.store(As[0], tid);
    tb.store(Bs[0], tid);
  }
  __syncthreads();

  for (int t = 0; t < nt; ++t) {
    const int buf = t & 1;
    if (t + 1 < nt) {
      ta.load(g.A, m0, g.M, kbeg + (int64_t)(t + 1) * BK, g.K, tid);
      tb.load(g.B, n0, g.N, kbeg + (int64_t)(t + 1) * BK, g.K, tid);
    }
    const float* a_s = As[buf];
    const float* b_s = Bs[buf];
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk) {
      const int kr = 2 * kk + (lane >> 5);
      float a[TI], b[TJ];
#pragma unroll
      for (int i = 0; i < TI; ++i) a[i] = a_s[kr * TA::S + wm + 32 * i + (lane & 31)];
#pragma unroll
      for (int j = 0; j < TJ; ++j) b[j] = b_s[kr * TB::S + wn + 32 * j + (lane & 31)];
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (t + 1 < nt) {
      ta.store(As[buf ^ 1], tid);
      tb.store(Bs[buf ^ 1], tid);
    }
    __syncthreads();
  }

  // epilogue: 32x32 C/D map — col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
      const int64_t col = n0 + wn + 32 * j + (lane & 31);
      if (col >= g.N) continue;
      const float bcol = (g.bias && (g.epi == NR_EPI_STORE || g.epi == NR_EPI_STORE_RELU ||
                                     g.epi == NR_EPI_STORE_TANH || g.epi == NR_EPI_ACCUM ||
                                     g.epi == NR_EPI_STORE_GELU)) ? g.bias[col] : 0.f;
      int sj = 0;
      int64_t scol = col;
      if (g.epi == NR_EPI_SCATTER && g.Cm.map == NR_ROWS_CONV3) {
        sj = (int)(col / g.Cm.seg);
        scol = col - (int64_t)sj * g.Cm.seg;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t row = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row >= g.M) continue;
        const float v = acc[i][j][r];
        if (g.epi == NR_EPI_STORE) {
          g.C[row * g.ldc + col] = v + bcol;
        } else if (g.epi == NR_EPI_STORE_RELU) {
          g.C[row * g.ldc + col] = fmaxf(v + bcol, 0.f);
        } else if (g.epi == NR_EPI_STORE_TANH) {
          g.C[row * g.ldc + col] = tanhf(v + bcol);
        } else if (g.epi == NR_EPI_ACCUM_GATE) {
          const int64_t o = row * g.ldc + col;
          g.C[o] = g.Cm.base[row * g.Cm.ld + col] > 0.f ? g.C[o] + v : 0.f;
        } else if (g.epi == NR_EPI_ACCUM) {
          g.C[row * g.ldc + col] += v + bcol;
        } else if (g.epi == NR_EPI_STORE_GELU) {
          const float x = v + bcol;
          const_cast<float*>(g.Cm.base)[row * g.Cm.ld + col] = x;
          g.C[row * g.ldc + col] = nr_gelu(x);
        } else if (g.epi == NR_EPI_GELU_GRAD) {
          g.C[row * g.ldc + col] = v * nr_gelu_grad(g.Cm.base[row * g.Cm.ld + col]);
        } else if (g.epi == NR_EPI_ATOMIC) {
          atomicAdd(&g.C[row * g.ldc + col], v);
        } else {  // NR_EPI_SCATTER, NR_EPI_SCATTER_STORE (GATHER rows only: gemm_prepare)
          int64_t tok;
          if (g.Cm.map == NR_ROWS_GATHER) {
            tok = g.Cm.idx[row];
          } else if (g.Cm.map == NR_ROWS_CONV3) {
            const int64_t n = row / g.Cm.L;
            const int t2 = (int)(row - n * g.Cm.L) + sj - 1;
            if (t2 < 0 || t2 >= g.Cm.L) continue;
            tok = g.Cm.idx[n * g.Cm.L + t2];
          } else {
            tok = row;
          }
          if (tok == g.pad_row) continue;
          if (g.epi == NR_EPI_SCATTER_STORE) {
            g.C[tok * g.ldc + scol] = v;   // distinct rows, one split: this workgroup owns the element
          } else {
            atomicAdd(&g.C[tok * g.ldc + scol], v);
          }
        }
      }
    }
}

Op to_op(const nr_operand* o) {
  Op d;
  d.base = o ? o->data : nullptr;
  d.ld = o ? o->ld : 0;
  d.idx = o ? o->rows : nullptr;
  d.map = o ? o->map : NR_ROWS_PLAIN;
  d.L = o ? o->seq_len : 1;
  d.seg = o ? o->seg : 1;
  d.vec = o && (o->ld % 4 == 0) && ((reinterpret_cast<uintptr_t>(o->data) & 15) == 0);
  return d;
}

template <int BM, int BN, bool AK, bool BKC>
int launch(const Args& g, int splits, hipStream_t s) {
  const int64_t gm = (g.M + BM - 1) / BM, gn = (g.N + BN - 1) / BN;
  dim3 grid((unsigned)(gm * gn), (unsigned)splits);
  hipLaunchKernelGGL((gemm_f32_kernel<BM, BN, AK, BKC>), grid, dim3(256), 0, s, g);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

template <int BM, int BN>
int launch_kc(const Args& g, int ak, int bk, int splits, hipStream_t s) {
  if (ak && bk) return launch<BM, BN, true, true>(g, splits, s);
  if (ak && !bk) return launch<BM, BN, true, false>(g, splits, s);
  if (!ak && bk) return launch<BM, BN, false, true>(g, splits, s);
  return launch<BM, BN, false, false>(g, splits, s);
}

// the generic kernel: any alignment; NR_EPI_SCATTER_STORE as plain stores, NR_EPI_SCATTER_ZEROED (rows
// zero on entry) as the same sums via NR_EPI_SCATTER's atomics (gemm_route)
int launch_generic(const GemmCall& c, const nrfast::GemmRoute& r) {
  const nrfast::GemmProblem& p = c.p;
  Args g;
  g.M = p.M; g.N = p.N; g.K = p.K;
  g.A = to_op(p.A); g.B = to_op(p.B); g.Cm = to_op(p.c_rows);
  g.C = c.d.C; g.ldc = c.d.ldc; g.bias = c.d.bias; g.epi = r.epi; g.pad_row = c.d.pad_row;
  g.kchunk = r.kchunk;
  const int ak = p.A->layout == NR_KCONTIG, bk = p.B->layout == NR_KCONTIG;
  if (r.bm == 128 && r.bn == 128) return launch_kc<128, 128>(g, ak, bk, r.splits, c.stream);
  if (r.bm == 128 && r.bn == 64) return launch_kc<128, 64>(g, ak, bk, r.splits, c.stream);
  if (r.bm == 64 && r.bn == 128) return launch_kc<64, 128>(g, ak, bk, r.splits, c.stream);
  return launch_kc<64, 64>(g, ak, bk, r.splits, c.stream);
}

// The one path behind the five exported entries: gemm_prepare validates and routes (gemm_route.h) a
// described call (`run` false: a valid call with nothing to do), gemm_launch runs the route;
// nr_gemm_f32_pair prepares two calls before it launches either.
// `dyn`: the dynamic form -- device-resident extents and / or a CU cap, fast kernels only; the static
// form also takes unaligned operands (generic kernel) and small tiles.
int gemm_prepare(bool dyn, const nr_gemm_desc& d, hipStream_t stream, GemmCall& c, nrfast::GemmRoute& r, bool& run) {
  const nr_operand *A = d.A, *B = d.B, *c_rows = d.c_rows;
  const int32_t epilogue = d.epilogue;
  run = false;
  if (d.work_elems < 0 || (d.work_elems > 0 && !d.work)) return NR_EINVAL(16);
  if (d.colsum_folded) *d.colsum_folded = 0;
  if (d.colsum && !d.colsum_folded) return NR_EINVAL(17);
  if (dyn && d.max_cus < 0) return NR_EINVAL(15);
  // the device K of the dynamic form must be a multiple of 32, so its bound must be one
  if (d.M < 0 || d.N < 0 || d.K < 0 || (dyn && d.K % 32)) return NR_EINVAL(0);
  // (the two forms have always reported a bad prec under different argument numbers)
  if (d.prec != NR_GEMM_F32 && d.prec != NR_GEMM_BF16X6 && d.prec != NR_GEMM_BF16) return NR_EINVAL(dyn ? 14 : 12);
  if (epilogue < NR_EPI_STORE || epilogue > NR_EPI_SCATTER_ZEROED) return NR_EINVAL(3);
  if (!A || !B || !d.C || !A->data || !B->data) return NR_EINVAL(1);
  // gathered tables must be float4-addressable; the dynamic form has the fast kernels only, which
  // need that of every operand
  if (((dyn || A->map != NR_ROWS_PLAIN) && (A->ld & 3)) || ((dyn || B->map != NR_ROWS_PLAIN) && (B->ld & 3)))
    return NR_EINVAL(2);
  if (epilogue == NR_EPI_SCATTER && (!c_rows || (c_rows->map != NR_ROWS_PLAIN && !c_rows->rows)))
    return NR_EINVAL(4);
  if ((epilogue == NR_EPI_ACCUM_GATE || epilogue == NR_EPI_STORE_GELU || epilogue == NR_EPI_GELU_GRAD) &&
      (!c_rows || !c_rows->data))
    return NR_EINVAL(4);
  const bool no_store_rows = (epilogue == NR_EPI_SCATTER_STORE || epilogue == NR_EPI_SCATTER_ZEROED) &&
                             (!c_rows || c_rows->map != NR_ROWS_GATHER || !c_rows->rows);
  // the dynamic form checks the scatter-store rows here, the static form only once it has work to
  // do (after the split_k check and the empty-problem return)
  if (dyn && no_store_rows) return NR_EINVAL(4);
  const int32_t split_k = d.split_k < 1 ? 1 : d.split_k;
  if (split_k > 1 && epilogue != NR_EPI_ATOMIC && epilogue != NR_EPI_SCATTER) return NR_EINVAL(5);
  // K == 0: the dynamic form leaves C alone, the static form runs the generic kernel's epilogue on
  // zero accumulators (C = bias for a store epilogue)
  if (d.M == 0 || d.N == 0 || (dyn && d.K == 0)) return NR_OK;
  if (no_store_rows) return NR_EINVAL(4);

  c = GemmCall{{d.M, d.N, d.K, A, B, c_rows, epilogue, split_k, d.prec, dyn, d.m_dev != nullptr, d.max_cus, d.work,
                d.work_elems, d.colsum != nullptr},
               d, stream};
  // the CU count matters to a route only where it sizes a workspace's use
  r = nrfast::gemm_route(c.p, d.work ? nr_gemm_device_cus() : 0);
  if (r.family == nrfast::GEMM_NOT_ELIGIBLE) return NR_EINVAL(r.einval);
  run = true;
  return NR_OK;
}

int gemm_launch(const GemmCall& c, const nrfast::GemmRoute& r) {
  return r.family == nrfast::GEMM_GENERIC ? launch_generic(c, r) : nr_gemm_fast(c, r);
}

// nr_gemm_f32_ws reads a description's form off it: m_dev, k_dev NULL and max_cus 0 is the static form
bool desc_dyn(const nr_gemm_desc& d) { return d.m_dev || d.k_dev || d.max_cus != 0; }

int gemm_run(bool dyn, const nr_gemm_desc& d, hipStream_t stream) {
  GemmCall c;
  nrfast::GemmRoute r;
  bool run;
  const int rc = gemm_prepare(dyn, d, stream, c, r, run);
  return rc != NR_OK || !run ? rc : gemm_launch(c, r);
}

}  // namespace

extern "C" int nr_gemm_f32(int64_t M, int64_t N, int64_t K, const nr_operand* A,
                           const nr_operand* B, float* C, int64_t ldc, const float* bias,
                           int32_t epilogue, const nr_operand* c_rows, int64_t pad_row,
                           int32_t split_k, int32_t prec, hipStream_t stream) {
  return gemm_run(false, nr_gemm_desc{M, N, K, A, B, C, ldc, bias, epilogue, c_rows, pad_row, split_k, nullptr, nullptr,
                                      prec, 0, nullptr, 0, nullptr, nullptr},
                  stream);
}

extern "C" int nr_gemm_f32_ws(int64_t M, int64_t N, int64_t K, const nr_operand* A, const nr_operand* B, float* C,
                              int64_t ldc, const float* bias, int32_t epilogue, const nr_operand* c_rows,
                              int64_t pad_row, int32_t split_k, const int32_t* m_dev, const int32_t* k_dev,
                              int32_t prec, int32_t max_cus, float* work, int64_t work_elems, float* colsum,
                              int32_t* colsum_folded, hipStream_t stream) {
  const nr_gemm_desc d{M, N, K, A, B, C, ldc, bias, epilogue, c_rows, pad_row, split_k, m_dev, k_dev,
                       prec, max_cus, work, work_elems, colsum, colsum_folded};
  return gemm_run(desc_dyn(d), d, stream);
}

// Two independent problems: one launch where gemm_pair_order (gemm_route.h) allows it, else the two
// calls of nr_gemm_f32_ws one after the other.  Both are validated before either launches.
extern "C" int nr_gemm_f32_pair(const nr_gemm_desc* p1, const nr_gemm_desc* p2, hipStream_t stream) {
  if (!p1 || !p2) return NR_EINVAL(200);
  GemmCall c1, c2;
  nrfast::GemmRoute r1, r2;
  bool run1, run2;
  int rc = gemm_prepare(desc_dyn(*p1), *p1, stream, c1, r1, run1);
  if (rc != NR_OK) return rc;
  rc = gemm_prepare(desc_dyn(*p2), *p2, stream, c2, r2, run2);
  if (rc != NR_OK) return rc <= -1000 ? rc - 100 : rc;   // NR_EINVAL(100 + n): problem 2's argument n
  if (run1 && run2) {
    const nrfast::GemmOut o1{c1.d.C, c1.d.ldc, c1.d.bias}, o2{c2.d.C, c2.d.ldc, c2.d.bias};
    if (nrfast::gemm_pair_alias(c1.p, o1, c2.p, o2)) return NR_EINVAL(201);
    const int order = nrfast::gemm_pair_order(c1.p, r1, o1, c2.p, r2, o2);
    if (order == 1) return nr_gemm_fast_pair(c1, r1, c2, r2);
    if (order == 2) return nr_gemm_fast_pair(c2, r2, c1, r1);
  }
  if (run1 && (rc = gemm_launch(c1, r1)) != NR_OK) return rc;
  return run2 ? gemm_launch(c2, r2) : NR_OK;
}

// Device-resident extents: M and K are upper bounds (grid sizing); the kernel reads the actual
// values from m_dev / k_dev (either may be null).  Fast-path operand shapes only (K-contiguous
// or MN-contiguous rows, 16-B aligned, ld % 4 == 0); the device K must be a multiple of 32.
extern "C" int nr_gemm_f32_dyn(int64_t M, int64_t N, int64_t K, const nr_operand* A, const nr_operand* B,
                               float* C, int64_t ldc, const float* bias, int32_t epilogue,
                               const nr_operand* c_rows, int64_t pad_row, int32_t split_k, const int32_t* m_dev,
                               const int32_t* k_dev, int32_t prec, hipStream_t stream) {
  return gemm_run(true, nr_gemm_desc{M, N, K, A, B, C, ldc, bias, epilogue, c_rows, pad_row, split_k, m_dev, k_dev, prec,
                                     0, nullptr, 0, nullptr, nullptr},
                  stream);
}

extern "C" int nr_gemm_f32_dyn_cus(int64_t M, int64_t N, int64_t K, const nr_operand* A, const nr_operand* B,
                                   float* C, int64_t ldc, const float* bias, int32_t epilogue,
                                   const nr_operand* c_rows, int64_t pad_row, int32_t split_k, const int32_t* m_dev,
                                   const int32_t* k_dev, int32_t prec, int32_t max_cus, hipStream_t stream) {
  return gemm_run(true, nr_gemm_desc{M, N, K, A, B, C, ldc, bias, epilogue, c_rows, pad_row, split_k, m_dev, k_dev, prec,
                                     max_cus, nullptr, 0, nullptr, nullptr},
                  stream);
}
