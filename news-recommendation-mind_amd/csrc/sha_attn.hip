// Single-head self-attention core of the reference's one-layer BERT news encoder, Transformer_Encoder
// (models/Modules/OneLayerBert.py BertSelfAttention: ONE head as wide as the model, scale 1/sqrt(H),
// XSoftmax with the key-only mask [N, 1, L], Dropout on the probabilities):
//   P   = XSoftmax_j(scale * q_i . k_j, m_j)     masked keys exactly 0, a title with no token all zero
//   ctx = (P * keep / (1 - p)) v
// and its backward from the saved P.
//
// One workgroup (4 waves) owns one title of L <= 64 tokens and walks the model width D in chunks of 64
// columns: a chunk of q, k (forward) or dctx, v / k, q, dctx (backward) is staged in LDS with 16-B
// coalesced loads, so qkv is read once per pass and the LDS footprint does not grow with D (52 KB
// forward, 104 KB backward at L = 64; 24 / 49 KB at L = 30, several titles per CU).
//
// Arithmetic: f32 VALU fma chains (every product rounded once).  The f32 MFMA has the same peak rate
// as the packed VALU fma on gfx950, and the core's 2.4 GFLOP at the train shape is ~15 us at that rate
// against >= 80 us of HBM traffic, so the matrix unit would buy nothing here; the VALU form keeps one
// conflict-free ds_read_b128 layout for all seven products:
//   [L x L] = X Y^T over a chunk: thread (ti, tj) of 16 x 16 holds the 4 x 4 results (ti + 16 a, tj + 16 b)
//   [L x 64] = M X  over the keys: thread (ti, tj) holds rows ti + 16 a of the float4 column group tj
// The softmax, the row sums and the dropout are fp32, one wave per query row.  No atomics: every
// output element has one writer and a fixed summation order, so two calls give the same bits.
#include "common.h"
#include "../../include/newsrec_hip.h"

namespace {

constexpr int SHA_THREADS = 256;
constexpr int SHA_DC = 64;          // columns per chunk
constexpr int SHA_LD = SHA_DC + 4;  // LDS row stride (floats) of a chunk and of an [L][L] matrix
constexpr int SHA_MAX_L = 64;
constexpr int SHA_MAX_D = 1024;

struct ShaArgs {
  const float* qkv; int64_t ldq; int64_t koff; int64_t voff;
  const void* mask; int mask_dtype;
  int L; int D; float scale;
  float pscale; uint32_t thresh; uint32_t key; const uint64_t* rng; uint64_t offset;
  float* ctx; int64_t ldc;
  float* probs;
  const float* dctx; int64_t ldd;
  float* dqkv; int64_t lddq;
};

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

__device__ __forceinline__ void fma4(float4& acc, float s, const float4& x) {
  acc.x = fmaf(s, x.x, acc.x); acc.y = fmaf(s, x.y, acc.y);
  acc.z = fmaf(s, x.z, acc.z); acc.w = fmaf(s, x.w, acc.w);
}

// Stage columns [c0, c0 + 64) of L rows (ld apart) in dst [LR][SHA_LD]; rows >= L and columns >= D are zero.
__device__ __forceinline__ void sha_load_chunk(float* dst, const float* src, int64_t ld, int L, int LR, int c0,
                                               int D, int tid) {
  for (int idx = tid; idx < LR * (SHA_DC / 4); idx += SHA_THREADS) {
    const int r = idx >> 4, c = 4 * (idx & 15);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < L && c0 + c < D) v = ld4(src + (int64_t)r * ld + c0 + c);
    st4(dst + r * SHA_LD + c, v);
  }
}

// acc[a][b] += sum_c X[ti + 16 a][c] Y[tj + 16 b][c] over the chunk's 64 columns; rows past LR - 1 are
// clamped (their results are never stored).
__device__ __forceinline__ void sha_dot_chunk(const float* X, const float* Y, int ti, int tj, int na, int LR,
                                              float (&acc)[4][4]) {
  int xr[4], yr[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    xr[a] = min(ti + 16 * a, LR - 1) * SHA_LD;
    yr[a] = min(tj + 16 * a, LR - 1) * SHA_LD;
  }
#pragma unroll 1
  for (int c = 0; c < SHA_DC; c += 4) {
    float4 x[4], y[4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
      if (a < na) {   // uniform
        x[a] = ld4(X + xr[a] + c);
        y[a] = ld4(Y + yr[a] + c);
      }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (a < na && b < na) {
          float s = acc[a][b];
          s = fmaf(x[a].x, y[b].x, s); s = fmaf(x[a].y, y[b].y, s);
          s = fmaf(x[a].z, y[b].z, s); s = fmaf(x[a].w, y[b].w, s);
          acc[a][b] = s;
        }
  }
}

// acc[a] = sum_j M[ti + 16 a][j] X[j][4 tj .. 4 tj + 3] over j in [0, LR): M's columns and X's rows in
// [L, LR) are zero.
__device__ __forceinline__ void sha_mm_chunk(const float* M, const float* X, int ti, int tj, int na, int LR,
                                             float4 (&acc)[4]) {
  int mr[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    mr[a] = min(ti + 16 * a, LR - 1) * SHA_LD;
    acc[a] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll 1
  for (int j = 0; j < LR; j += 4) {
    const float4 x0 = ld4(X + (j + 0) * SHA_LD + 4 * tj);
    const float4 x1 = ld4(X + (j + 1) * SHA_LD + 4 * tj);
    const float4 x2 = ld4(X + (j + 2) * SHA_LD + 4 * tj);
    const float4 x3 = ld4(X + (j + 3) * SHA_LD + 4 * tj);
#pragma unroll
    for (int a = 0; a < 4; ++a)
      if (a < na) {   // uniform
        const float4 m = ld4(M + mr[a] + j);
        fma4(acc[a], m.x, x0); fma4(acc[a], m.y, x1); fma4(acc[a], m.z, x2); fma4(acc[a], m.w, x3);
      }
  }
}

// Rows ti + 16 a < L of the column group tj of chunk c0 -> out (ld apart), columns < D only.
__device__ __forceinline__ void sha_store_chunk(float* out, int64_t ld, const float4 (&acc)[4], int ti, int tj,
                                                int na, int L, int c0, int D) {
  const int c = c0 + 4 * tj;
  if (c >= D) return;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = ti + 16 * a;
    if (a < na && i < L) st4(out + (int64_t)i * ld + c, acc[a]);
  }
}

__device__ __forceinline__ uint32_t sha_key(const ShaArgs& g) {
  return g.rng ? nr_dropout_key(g.rng[0], g.rng[1] + g.offset) : g.key;
}

__global__ __launch_bounds__(SHA_THREADS) void sha_attn_fwd_kernel(ShaArgs g) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int L = g.L, D = g.D;
  const int LR = (L + 3) & ~3;
  const int na = (L + 15) >> 4;
  float* xa = sm;                      // q chunk, then v chunk
  float* xb = xa + LR * SHA_LD;        // k chunk
  float* ps = xb + LR * SHA_LD;        // scores, then the dropped probabilities
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ti = tid >> 4, tj = tid & 15;
  const int64_t s = blockIdx.x;
  const float* q = g.qkv + s * L * g.ldq;
  const uint32_t key = sha_key(g);

  float acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
  for (int c0 = 0; c0 < D; c0 += SHA_DC) {
    sha_load_chunk(xa, q, g.ldq, L, LR, c0, D, tid);
    sha_load_chunk(xb, q + g.koff, g.ldq, L, LR, c0, D, tid);
    __syncthreads();
    sha_dot_chunk(xa, xb, ti, tj, na, LR, acc);
    __syncthreads();
  }
  // the first v chunk travels while the softmax runs
  sha_load_chunk(xa, q + g.voff, g.ldq, L, LR, 0, D, tid);
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int i = ti + 16 * a, j = tj + 16 * b;
      if (a < na && b < na && i < L && j < L) ps[i * SHA_LD + j] = acc[a][b] * g.scale;
    }
  __syncthreads();
  const bool valid = lane < L && nr_mask_at(g.mask, g.mask_dtype, s * L + lane);
  for (int i = wave; i < L; i += SHA_THREADS / 64) {
    const float x = valid ? ps[i * SHA_LD + lane] : -INFINITY;
    const float m = nr_wave_max(x);
    const float e = valid ? expf(x - m) : 0.f;
    const float sum = nr_wave_sum(e);
    const float p = valid ? e / sum : 0.f;
    const uint64_t elem = ((uint64_t)s * L + i) * L + lane;
    if (lane < L) g.probs[elem] = p;
    if (lane < LR) ps[i * SHA_LD + lane] = nr_dropout_keep(key, (uint32_t)elem, g.thresh) ? p * g.pscale : 0.f;
  }
  __syncthreads();
  float* ctx = g.ctx + s * L * g.ldc;
  for (int c0 = 0; c0 < D; c0 += SHA_DC) {
    if (c0) {
      sha_load_chunk(xa, q + g.voff, g.ldq, L, LR, c0, D, tid);
      __syncthreads();
    }
    float4 o[4];
    sha_mm_chunk(ps, xa, ti, tj, na, LR, o);
    sha_store_chunk(ctx, g.ldc, o, ti, tj, na, L, c0, D);
    __syncthreads();
  }
}

__global__ __launch_bounds__(SHA_THREADS) void sha_attn_bwd_kernel(ShaArgs g) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int L = g.L, D = g.D;
  const int LR = (L + 3) & ~3;
  const int na = (L + 15) >> 4;
  const int MS = LR * SHA_LD;
  float* xa = sm;                // dctx chunk
  float* xb = xa + MS;           // v chunk, then k chunk
  float* xc = xb + MS;           // q chunk
  float* ds = xc + MS;           // dPd, then scale * dS [query][key]
  float* dst = ds + MS;          // scale * dS^T [key][query]
  float* pdt = dst + MS;         // (P * keep / (1 - p))^T [key][query]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ti = tid >> 4, tj = tid & 15;
  const int64_t s = blockIdx.x;
  const float* q = g.qkv + s * L * g.ldq;
  const float* dctx = g.dctx + s * L * g.ldd;
  const uint32_t key = sha_key(g);

  // dPd = dctx v^T
  float acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
  for (int c0 = 0; c0 < D; c0 += SHA_DC) {
    sha_load_chunk(xa, dctx, g.ldd, L, LR, c0, D, tid);
    sha_load_chunk(xb, q + g.voff, g.ldq, L, LR, c0, D, tid);
    __syncthreads();
    sha_dot_chunk(xa, xb, ti, tj, na, LR, acc);
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int i = ti + 16 * a, j = tj + 16 * b;
      if (a < na && b < na && i < L && j < L) ds[i * SHA_LD + j] = acc[a][b];
    }
  __syncthreads();
  // per query row: g = dPd * keep / (1 - p), dS = P (g - sum_j g P); rows and columns in [L, LR) are zero
  for (int i = wave; i < LR; i += SHA_THREADS / 64) {
    const bool in = i < L && lane < L;
    const uint64_t elem = ((uint64_t)s * L + i) * L + lane;
    const float p = in ? g.probs[elem] : 0.f;
    const bool keep = nr_dropout_keep(key, (uint32_t)elem, g.thresh);
    const float gg = in && keep ? ds[i * SHA_LD + lane] * g.pscale : 0.f;
    const float r = nr_wave_sum(gg * p);
    const float d = p * (gg - r) * g.scale;
    const float pd = keep ? p * g.pscale : 0.f;
    if (lane < LR) {
      if (i < L) ds[i * SHA_LD + lane] = d;
      dst[lane * SHA_LD + i] = d;
      pdt[lane * SHA_LD + i] = pd;
    }
  }
  __syncthreads();
  float* dq = g.dqkv + s * L * g.lddq;
  for (int c0 = 0; c0 < D; c0 += SHA_DC) {
    sha_load_chunk(xa, dctx, g.ldd, L, LR, c0, D, tid);
    sha_load_chunk(xb, q + g.koff, g.ldq, L, LR, c0, D, tid);
    sha_load_chunk(xc, q, g.ldq, L, LR, c0, D, tid);
    __syncthreads();
    float4 o[4];
    sha_mm_chunk(ds, xb, ti, tj, na, LR, o);      // dQ = scale dS k
    sha_store_chunk(dq, g.lddq, o, ti, tj, na, L, c0, D);
    sha_mm_chunk(dst, xc, ti, tj, na, LR, o);     // dK = scale dS^T q
    sha_store_chunk(dq + g.koff, g.lddq, o, ti, tj, na, L, c0, D);
    sha_mm_chunk(pdt, xa, ti, tj, na, LR, o);     // dV = Pd^T dctx
    sha_store_chunk(dq + g.voff, g.lddq, o, ti, tj, na, L, c0, D);
    __syncthreads();
  }
}

bool sha_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The shared argument checks -> NR_OK or the invalid-argument code.
int sha_setup(ShaArgs& g, const float* qkv, int64_t ldq, int64_t koff, int64_t voff, const void* mask,
              int32_t mask_dtype, int64_t nseq, int32_t L, int32_t D, float scale, float p_drop, uint64_t seed,
              uint64_t offset, const uint64_t* rng, const float* probs) {
  if (nseq < 0 || nseq > 0x7fffffff || L < 1 || L > SHA_MAX_L || D < 4 || D > SHA_MAX_D || D % 4 || koff % 4 ||
      voff % 4 || koff < D || voff < koff + D || ldq % 4 || ldq < voff + D || !(p_drop >= 0.f && p_drop < 1.f) ||
      mask_dtype < NR_MASK_U8 || mask_dtype > NR_MASK_F32)
    return NR_EINVAL(0);
  if (!qkv || !mask || !probs) return NR_EINVAL(1);
  if (!sha_aligned(qkv)) return NR_EINVAL(0);
  g.qkv = qkv; g.ldq = ldq; g.koff = koff; g.voff = voff; g.mask = mask; g.mask_dtype = mask_dtype;
  g.L = L; g.D = D; g.scale = scale;
  g.pscale = p_drop > 0.f ? 1.f / (1.f - p_drop) : 1.f;
  g.thresh = nr_dropout_threshold(p_drop);
  g.key = nr_dropout_key(seed, offset); g.rng = rng; g.offset = offset;
  return NR_OK;
}

template <typename Kern>
int sha_launch(Kern kern, int64_t nseq, size_t smem, hipStream_t stream, const ShaArgs& g) {
  if (smem > 64 * 1024 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess)
    return -(int)hipGetLastError();
  hipLaunchKernelGGL(kern, dim3((unsigned)nseq), dim3(SHA_THREADS), smem, stream, g);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

size_t sha_smem(int L, int mats) { return (size_t)mats * ((L + 3) & ~3) * SHA_LD * sizeof(float); }

}  // namespace

extern "C" int nr_sha_attn_fwd(const float* qkv, int64_t ldq, int64_t koff, int64_t voff, const void* mask,
                               int32_t mask_dtype, int64_t nseq, int32_t L, int32_t D, float scale, float p_drop,
                               uint64_t seed, uint64_t offset, const uint64_t* rng, float* ctx, int64_t ldc,
                               float* probs, hipStream_t stream) {
  ShaArgs g{};
  const int rc = sha_setup(g, qkv, ldq, koff, voff, mask, mask_dtype, nseq, L, D, scale, p_drop, seed, offset, rng,
                           probs);
  if (rc != NR_OK) return rc;
  if (ldc % 4 || ldc < D) return NR_EINVAL(0);
  if (!ctx) return NR_EINVAL(1);
  if (!sha_aligned(ctx)) return NR_EINVAL(0);
  if (nseq == 0) return NR_OK;
  g.ctx = ctx; g.ldc = ldc; g.probs = probs;
  return sha_launch(sha_attn_fwd_kernel, nseq, sha_smem(L, 3), stream, g);
}

extern "C" int nr_sha_attn_bwd(const float* qkv, int64_t ldq, int64_t koff, int64_t voff, const void* mask,
                               int32_t mask_dtype, int64_t nseq, int32_t L, int32_t D, float scale, float p_drop,
                               uint64_t seed, uint64_t offset, const uint64_t* rng, const float* probs,
                               const float* dctx, int64_t ldd, float* dqkv, int64_t lddq, hipStream_t stream) {
  ShaArgs g{};
  const int rc = sha_setup(g, qkv, ldq, koff, voff, mask, mask_dtype, nseq, L, D, scale, p_drop, seed, offset, rng,
                           probs);
  if (rc != NR_OK) return rc;
  if (ldd % 4 || ldd < D || lddq % 4 || lddq < voff + D) return NR_EINVAL(0);
  if (!dctx || !dqkv) return NR_EINVAL(1);
  if (!sha_aligned(dctx) || !sha_aligned(dqkv)) return NR_EINVAL(0);
  if (nseq == 0) return NR_OK;
  g.probs = const_cast<float*>(probs); g.dctx = dctx; g.ldd = ldd; g.dqkv = dqkv; g.lddq = lddq;
  return sha_launch(sha_attn_bwd_kernel, nseq, sha_smem(L, 6), stream, g);
}
