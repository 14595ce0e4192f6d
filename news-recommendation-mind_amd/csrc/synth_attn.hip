// Dense-synthesizer attention core of the reference's `-b synthesizer` PLM tower
// (models/Modules/Synthesizer.py BertSelfAttention): the scores come from a two-layer MLP over each token
// of the value projection hv, not from q . k; no mask, no heads, no scale, no dropout on the probabilities:
//   z1  = hv W1^T + b1,  a1 = max(z1, 0)        [L x L] per title, W1 [L][D]
//   a2  = a1 W2^T + b2                          W2 [L][L]
//   P   = softmax_j(a2)                         over all L positions
//   ctx = P hv
// and its backward from the saved a1 and P (the weight gradients are summed over titles by the GEMMs that
// consume the stored dA1 / dA2, not here).
//
// The layout is sha_attn.hip's: one workgroup (4 waves) owns one title of L <= 64 tokens and walks the
// model width D in chunks of 64 columns staged in LDS with 16-B coalesced loads, so the LDS footprint does
// not grow with D: three [LR][68] matrices forward (52 KB at L = 64, 26 KB at L = 30), four backward
// (70 KB / 35 KB; the request crosses 64 KB between L = 60 and 61), several titles per CU at L = 30.
// sha_attn.hip's header gives the argument for f32 VALU fma chains over the MFMA at this intensity; it
// holds here unchanged (4 L^2 D + 2 L^3 flop forward against 2 L D floats of HBM traffic per title).  Both
// thread tilings are the ones of that file:
//   [L x L] = X Y^T over a chunk: thread (ti, tj) of 16 x 16 holds the 4 x 4 results (ti + 16 a, tj + 16 b)
//   [L x 64] = M X  over the rows of X: thread (ti, tj) holds rows ti + 16 a of the float4 column group tj
// The kernels are instantiated per NA = ceil(L / 16) in 1..4, the a and b ranges a title uses: at L = 30 a
// thread holds 2 x 2 accumulators in 62 / 74 VGPRs, and LDS, not registers, sets the titles per CU (6 / 4).
// W1 is re-read by every title (L2 hits: L D floats, the size of one title).  The small operands (w2, b1,
// b2, a1, probs, da1, da2: rows of L floats, 120 B at L = 30) are touched with 4-B accesses only.
// The softmax is fp32 with the row maximum subtracted, one wave per row.  No atomics: every output element
// has one writer and a fixed summation order, so two calls give the same bits.
#include "common.h"
#include "../../include/newsrec_hip.h"

namespace {

constexpr int SYN_THREADS = 256;
constexpr int SYN_DC = 64;          // columns per chunk
constexpr int SYN_LD = SYN_DC + 4;  // LDS row stride (floats) of a chunk and of an [L][L] matrix
constexpr int SYN_MAX_L = 64;
constexpr int SYN_MAX_D = 1024;

struct SynArgs {
  const float* hv; int64_t ldh;
  const float* w1; int64_t ldw1; const float* b1;
  const float* w2; const float* b2;
  int L; int D;
  float* a1; int64_t lda;
  float* probs;
  float* ctx; int64_t ldc;
  const float* dctx; int64_t ldd;
  float* da1; float* da2;
  float* dhv; int64_t lddh;
};

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

__device__ __forceinline__ void fma4(float4& acc, float s, const float4& x) {
  acc.x = fmaf(s, x.x, acc.x); acc.y = fmaf(s, x.y, acc.y);
  acc.z = fmaf(s, x.z, acc.z); acc.w = fmaf(s, x.w, acc.w);
}

// Stage columns [c0, c0 + 64) of L rows (ld apart) in dst [LR][SYN_LD]; rows >= L and columns >= D are zero.
__device__ __forceinline__ void syn_load_chunk(float* dst, const float* src, int64_t ld, int L, int LR, int c0,
                                               int D, int tid) {
  for (int idx = tid; idx < LR * (SYN_DC / 4); idx += SYN_THREADS) {
    const int r = idx >> 4, c = 4 * (idx & 15);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < L && c0 + c < D) v = ld4(src + (int64_t)r * ld + c0 + c);
    st4(dst + r * SYN_LD + c, v);
  }
}

// Stage the contiguous [L][L] matrix w2 (4-B aligned) in dst [LR][SYN_LD], all 64 columns written; rows and
// columns >= L are zero.
__device__ __forceinline__ void syn_load_w2(float* dst, const float* w2, int L, int LR, int tid) {
  for (int idx = tid; idx < LR * SYN_DC; idx += SYN_THREADS) {
    const int r = idx >> 6, c = idx & 63;
    dst[r * SYN_LD + c] = r < L && c < L ? w2[r * L + c] : 0.f;
  }
}

// acc[a][b] += sum_c X[ti + 16 a][c] Y[tj + 16 b][c] over columns [0, nc), nc % 4 == 0; rows past LR - 1
// are clamped (their results are never stored).  NA = ceil(L / 16) is a template argument: the tile loops
// carry no branch and a title of L <= 32 holds 2 x 2 accumulators, not 4 x 4.
template <int NA>
__device__ __forceinline__ void syn_dot_chunk(const float* X, const float* Y, int ti, int tj, int LR, int nc,
                                              float (&acc)[NA][NA]) {
  int xr[NA], yr[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    xr[a] = min(ti + 16 * a, LR - 1) * SYN_LD;
    yr[a] = min(tj + 16 * a, LR - 1) * SYN_LD;
  }
#pragma unroll 2
  for (int c = 0; c < nc; c += 4) {
    float4 x[NA], y[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      x[a] = ld4(X + xr[a] + c);
      y[a] = ld4(Y + yr[a] + c);
    }
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
      for (int b = 0; b < NA; ++b) {
        float s = acc[a][b];
        s = fmaf(x[a].x, y[b].x, s); s = fmaf(x[a].y, y[b].y, s);
        s = fmaf(x[a].z, y[b].z, s); s = fmaf(x[a].w, y[b].w, s);
        acc[a][b] = s;
      }
  }
}

// acc[a] += sum_j M[ti + 16 a][j] X[j][4 tj .. 4 tj + 3] over j in [0, LR): M's columns and X's rows in
// [L, LR) are zero.
template <int NA>
__device__ __forceinline__ void syn_mm_chunk(const float* M, const float* X, int ti, int tj, int LR,
                                             float4 (&acc)[NA]) {
  int mr[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) mr[a] = min(ti + 16 * a, LR - 1) * SYN_LD;
#pragma unroll 2
  for (int j = 0; j < LR; j += 4) {
    const float4 x0 = ld4(X + (j + 0) * SYN_LD + 4 * tj);
    const float4 x1 = ld4(X + (j + 1) * SYN_LD + 4 * tj);
    const float4 x2 = ld4(X + (j + 2) * SYN_LD + 4 * tj);
    const float4 x3 = ld4(X + (j + 3) * SYN_LD + 4 * tj);
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      const float4 m = ld4(M + mr[a] + j);
      fma4(acc[a], m.x, x0); fma4(acc[a], m.y, x1); fma4(acc[a], m.z, x2); fma4(acc[a], m.w, x3);
    }
  }
}

template <int NA>
__device__ __forceinline__ void syn_zero(float4 (&acc)[NA]) {
#pragma unroll
  for (int a = 0; a < NA; ++a) acc[a] = make_float4(0.f, 0.f, 0.f, 0.f);
}

template <int NA>
__device__ __forceinline__ void syn_zero(float (&acc)[NA][NA]) {
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int b = 0; b < NA; ++b) acc[a][b] = 0.f;
}

// Rows ti + 16 a < L of the column group tj of chunk c0 -> out (ld apart), columns < D only.
template <int NA>
__device__ __forceinline__ void syn_store_chunk(float* out, int64_t ld, const float4 (&acc)[NA], int ti, int tj,
                                                int L, int c0, int D) {
  const int c = c0 + 4 * tj;
  if (c >= D) return;
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    const int i = ti + 16 * a;
    if (i < L) st4(out + (int64_t)i * ld + c, acc[a]);
  }
}

template <int NA>
__global__ __launch_bounds__(SYN_THREADS) void synth_attn_fwd_kernel(SynArgs g) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int L = g.L, D = g.D;
  const int LR = (L + 3) & ~3;
  float* xa = sm;                      // hv chunk, then a1, then hv chunk again
  float* xb = xa + LR * SYN_LD;        // W1 chunk, then W2
  float* ps = xb + LR * SYN_LD;        // a2, then P
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ti = tid >> 4, tj = tid & 15;
  const int64_t s = blockIdx.x;
  const float* hv = g.hv + s * L * g.ldh;

  // z1 = hv W1^T
  float acc[NA][NA];
  syn_zero(acc);
  for (int c0 = 0; c0 < D; c0 += SYN_DC) {
    syn_load_chunk(xa, hv, g.ldh, L, LR, c0, D, tid);
    syn_load_chunk(xb, g.w1, g.ldw1, L, LR, c0, D, tid);
    __syncthreads();
    syn_dot_chunk(xa, xb, ti, tj, LR, SYN_DC, acc);
    __syncthreads();
  }
  // a1 = max(z1 + b1, 0) -> global and xa [LR][LR] (zero outside L x L); W2 -> xb
  float* a1 = g.a1 + s * L * g.lda;
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int b = 0; b < NA; ++b) {
      const int i = ti + 16 * a, j = tj + 16 * b;
      if (i < LR && j < LR) {
        float v = 0.f;
        if (i < L && j < L) {
          v = fmaxf(acc[a][b] + g.b1[j], 0.f);
          a1[(int64_t)i * g.lda + j] = v;
        }
        xa[i * SYN_LD + j] = v;
      }
    }
  syn_load_w2(xb, g.w2, L, LR, tid);
  __syncthreads();
  // a2 = a1 W2^T + b2
  syn_zero(acc);
  syn_dot_chunk(xa, xb, ti, tj, LR, LR, acc);
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int b = 0; b < NA; ++b) {
      const int i = ti + 16 * a, j = tj + 16 * b;
      if (i < L && j < L) ps[i * SYN_LD + j] = acc[a][b] + g.b2[j];
    }
  __syncthreads();
  // the first hv chunk of the second walk travels while the softmax runs
  syn_load_chunk(xa, hv, g.ldh, L, LR, 0, D, tid);
  const bool valid = lane < L;
  for (int i = wave; i < L; i += SYN_THREADS / 64) {
    const float x = valid ? ps[i * SYN_LD + lane] : -INFINITY;
    const float m = nr_wave_max(x);
    const float e = valid ? expf(x - m) : 0.f;
    const float sum = nr_wave_sum(e);
    const float p = valid ? e / sum : 0.f;
    if (valid) g.probs[((int64_t)s * L + i) * L + lane] = p;
    if (lane < LR) ps[i * SYN_LD + lane] = p;
  }
  __syncthreads();
  float* ctx = g.ctx + s * L * g.ldc;
  for (int c0 = 0; c0 < D; c0 += SYN_DC) {
    if (c0) {
      syn_load_chunk(xa, hv, g.ldh, L, LR, c0, D, tid);
      __syncthreads();
    }
    float4 o[NA];
    syn_zero(o);
    syn_mm_chunk(ps, xa, ti, tj, LR, o);
    syn_store_chunk(ctx, g.ldc, o, ti, tj, L, c0, D);
    __syncthreads();
  }
}

template <int NA>
__global__ __launch_bounds__(SYN_THREADS) void synth_attn_bwd_kernel(SynArgs g) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int L = g.L, D = g.D;
  const int LR = (L + 3) & ~3;
  const int MS = LR * SYN_LD;
  float* xa = sm;                // dctx chunk
  float* xb = xa + MS;           // hv chunk, then W2 [j][m], then W1 chunk
  float* ds = xb + MS;           // dP, then dA2 [i][j], then dA1 [i][m]
  float* pt = ds + MS;           // P^T [key][query]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ti = tid >> 4, tj = tid & 15;
  const int64_t s = blockIdx.x;
  const float* hv = g.hv + s * L * g.ldh;
  const float* dctx = g.dctx + s * L * g.ldd;

  // dP = dctx hv^T
  float acc[NA][NA];
  syn_zero(acc);
  for (int c0 = 0; c0 < D; c0 += SYN_DC) {
    syn_load_chunk(xa, dctx, g.ldd, L, LR, c0, D, tid);
    syn_load_chunk(xb, hv, g.ldh, L, LR, c0, D, tid);
    __syncthreads();
    syn_dot_chunk(xa, xb, ti, tj, LR, SYN_DC, acc);
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int b = 0; b < NA; ++b) {
      const int i = ti + 16 * a, j = tj + 16 * b;
      if (i < L && j < L) ds[i * SYN_LD + j] = acc[a][b];
    }
  syn_load_w2(xb, g.w2, L, LR, tid);
  __syncthreads();
  // per row: dA2 = P (dP - sum_j dP P); rows and columns in [L, LR) are zero
  for (int i = wave; i < LR; i += SYN_THREADS / 64) {
    const bool in = i < L && lane < L;
    const int64_t elem = ((int64_t)s * L + i) * L + lane;
    const float p = in ? g.probs[elem] : 0.f;
    const float dp = in ? ds[i * SYN_LD + lane] : 0.f;
    const float r = nr_wave_sum(dp * p);
    const float d = p * (dp - r);
    if (in) g.da2[((int64_t)s * L + i) * g.lda + lane] = d;
    if (lane < LR) {
      ds[i * SYN_LD + lane] = d;
      pt[lane * SYN_LD + i] = p;
    }
  }
  __syncthreads();
  // dA1 = (dA2 W2) gated by the stored a1 > 0 -> global and, once every thread has read dA2, over it
  {
    float4 o[NA];
    syn_zero(o);
    syn_mm_chunk(ds, xb, ti, tj, LR, o);
    const float* a1 = g.a1 + s * L * g.lda;
    float* da1 = g.da1 + s * L * g.lda;
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      const int i = ti + 16 * a;
      float v[4] = {o[a].x, o[a].y, o[a].z, o[a].w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int m = 4 * tj + k;
        if (i < L && m < L) {
          v[k] = a1[(int64_t)i * g.lda + m] > 0.f ? v[k] : 0.f;
          da1[(int64_t)i * g.lda + m] = v[k];
        } else {
          v[k] = 0.f;
        }
      }
      o[a] = make_float4(v[0], v[1], v[2], v[3]);
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      const int i = ti + 16 * a;
      if (i < LR) st4(ds + i * SYN_LD + 4 * tj, o[a]);
    }
  }
  __syncthreads();
  // dhv = P^T dctx + dA1 W1
  float* dhv = g.dhv + s * L * g.lddh;
  for (int c0 = 0; c0 < D; c0 += SYN_DC) {
    syn_load_chunk(xa, dctx, g.ldd, L, LR, c0, D, tid);
    syn_load_chunk(xb, g.w1, g.ldw1, L, LR, c0, D, tid);
    __syncthreads();
    float4 o[NA];
    syn_zero(o);
    syn_mm_chunk(pt, xa, ti, tj, LR, o);
    syn_mm_chunk(ds, xb, ti, tj, LR, o);
    syn_store_chunk(dhv, g.lddh, o, ti, tj, L, c0, D);
    __syncthreads();
  }
}

bool syn_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool syn_al4(const void* p) { return ((uintptr_t)p & 3) == 0; }

bool syn_sizes_ok(int64_t nseq, int32_t L, int32_t D, int64_t ldh, int64_t ldw1, int64_t lda) {
  return nseq >= 0 && nseq <= 0x7fffffff && L >= 1 && L <= SYN_MAX_L && D >= 4 && D <= SYN_MAX_D && D % 4 == 0 &&
         ldh % 4 == 0 && ldh >= D && ldw1 % 4 == 0 && ldw1 >= D && lda >= L;
}

template <typename Kern>
int syn_launch_one(Kern kern, int64_t nseq, size_t smem, hipStream_t stream, const SynArgs& g) {
  if (smem > 64 * 1024 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess)
    return -(int)hipGetLastError();
  hipLaunchKernelGGL(kern, dim3((unsigned)nseq), dim3(SYN_THREADS), smem, stream, g);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

size_t syn_smem(int L, int mats) { return (size_t)mats * ((L + 3) & ~3) * SYN_LD * sizeof(float); }

// The instantiation for NA = ceil(L / 16) 16-row thread tiles.
template <bool FWD>
int syn_launch(int64_t nseq, hipStream_t stream, const SynArgs& g) {
  const size_t smem = syn_smem(g.L, FWD ? 3 : 4);
#define SYN_CASE(NA)                                                                                  \
  case NA:                                                                                            \
    return FWD ? syn_launch_one(synth_attn_fwd_kernel<NA>, nseq, smem, stream, g)                     \
               : syn_launch_one(synth_attn_bwd_kernel<NA>, nseq, smem, stream, g)
  switch ((g.L + 15) >> 4) {
    SYN_CASE(1);
    SYN_CASE(2);
    SYN_CASE(3);
    default: break;
  }
  return FWD ? syn_launch_one(synth_attn_fwd_kernel<4>, nseq, smem, stream, g)
             : syn_launch_one(synth_attn_bwd_kernel<4>, nseq, smem, stream, g);
#undef SYN_CASE
}

}  // namespace

extern "C" int nr_synth_attn_fwd(const float* hv, int64_t ldh, const float* w1, int64_t ldw1, const float* b1,
                                 const float* w2, const float* b2, int64_t nseq, int32_t L, int32_t D, float* a1,
                                 int64_t lda, float* probs, float* ctx, int64_t ldc, hipStream_t stream) {
  if (!syn_sizes_ok(nseq, L, D, ldh, ldw1, lda) || ldc % 4 || ldc < D) return NR_EINVAL(0);
  if (!hv || !w1 || !b1 || !w2 || !b2 || !a1 || !probs || !ctx) return NR_EINVAL(1);
  if (!syn_al16(hv) || !syn_al16(w1) || !syn_al16(ctx) || !syn_al4(b1) || !syn_al4(w2) || !syn_al4(b2) ||
      !syn_al4(a1) || !syn_al4(probs))
    return NR_EINVAL(0);
  if (nseq == 0) return NR_OK;
  SynArgs g{};
  g.hv = hv; g.ldh = ldh; g.w1 = w1; g.ldw1 = ldw1; g.b1 = b1; g.w2 = w2; g.b2 = b2; g.L = L; g.D = D;
  g.a1 = a1; g.lda = lda; g.probs = probs; g.ctx = ctx; g.ldc = ldc;
  return syn_launch<true>(nseq, stream, g);
}

extern "C" int nr_synth_attn_bwd(const float* hv, int64_t ldh, const float* w1, int64_t ldw1, const float* w2,
                                 const float* a1, int64_t lda, const float* probs, const float* dctx, int64_t ldd,
                                 int64_t nseq, int32_t L, int32_t D, float* da1, float* da2, float* dhv,
                                 int64_t lddh, hipStream_t stream) {
  if (!syn_sizes_ok(nseq, L, D, ldh, ldw1, lda) || ldd % 4 || ldd < D || lddh % 4 || lddh < D) return NR_EINVAL(0);
  if (!hv || !w1 || !w2 || !a1 || !probs || !dctx || !da1 || !da2 || !dhv) return NR_EINVAL(1);
  if (!syn_al16(hv) || !syn_al16(w1) || !syn_al16(dctx) || !syn_al16(dhv) || !syn_al4(w2) || !syn_al4(a1) ||
      !syn_al4(probs) || !syn_al4(da1) || !syn_al4(da2))
    return NR_EINVAL(0);
  if (nseq == 0) return NR_OK;
  SynArgs g{};
  g.hv = hv; g.ldh = ldh; g.w1 = w1; g.ldw1 = ldw1; g.w2 = w2; g.L = L; g.D = D;
  g.a1 = const_cast<float*>(a1); g.lda = lda; g.probs = const_cast<float*>(probs); g.dctx = dctx; g.ldd = ldd;
  g.da1 = da1; g.da2 = da2; g.dhv = dhv; g.lddh = lddh;
  return syn_launch<false>(nseq, stream, g);
}
