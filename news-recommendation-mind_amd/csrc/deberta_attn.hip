// Disentangled self-attention core of the `-b deberta` PLM tower (transformers' DebertaModel with
// relative_attention and pos_att_type = c2p | p2c: DisentangledSelfAttention).  Per (title s, head h) of
// L <= 64 tokens and 64 dims, with the shared relative-position projections pk, pq [2L][64 per head] and
// delta(i, j) = i - j + L in [1, 2L - 1]:
//   S[i][j] = scale * (q_i . k_j + q_i . pk[delta(i, j)] + k_j . pq[delta(i, j)])
//   P[i]    = softmax of S[i] over the keys with mask 1 (exactly 0 elsewhere) for a query with mask 1,
//             1 / L at every key for a query with mask 0 (the library's masked_fill(finfo.min) arithmetic)
//   ctx     = (P * keep / (1 - p)) v
// and its backward from the saved P, including dpk and dpq summed over all titles.
//
// One workgroup (4 waves) holds one (title, head) in LDS as [rows][68] f32 tiles (16-B coalesced loads,
// ds_read_b128 in the products).  Of the 2L position rows a query touches only L, so the two position terms
// cost one q k^T each and the L x 2L products are never formed: thread (ti, tj) of 16 x 16 holds the 4 x 4
// scores of queries ti + 16 a and of the MIRRORED keys L - 1 - (tj + 16 b), for which
// delta = ti + tj + 1 + 16 (a + b): the 16 scores share 7 position rows, so a 4-column step costs 4 + 4 + 7
// b128 reads for 128 fma (content + one position term), no worse than the plain 4 + 4 for 64.
//
// LDS: q, k, pk, pq and v of one (title, head) at L = 64 are 5 x 17 + 2 x 17 KB; they are not all alive at
// once, so the position tile is staged twice (pk, then pq over it) and v / the later operands reuse dead
// tiles.  Forward: q|v, k, scores, one position tile = (3 LR + 2 L) x 272 B (85 KB at L = 64, 41.4 KB at
// L = 30: three workgroups per CU).  Backward: two operand tiles, dS, dS^T, the skewed dS and one position
// tile = (4 LR + 4 L) x 272 B (136 KB at L = 64: one resident workgroup; 65.9 KB at L = 30: two).
//
// Backward reduction: dpk / dpq are sums over titles.  Workgroup (g, h) of G x heads walks the titles
// g, g + G, ... of head h and keeps its [2L][64] partial sums in registers (rows ti + 16 a of the float4
// column group tj); they come from the skewed matrix sk[delta][i] = dS[i][i + L - delta] (zero outside the
// title) in one walk over i: dpk[delta] += sk[delta][i] q_i, dpq[delta] += sk[delta][i] k_(i + L - delta).
// The partials go to the caller's
// workspace and a second kernel adds the G of them in ascending g.  G = min(nseq, max(1, 512 / heads))
// depends on the arguments only: no atomics, a fixed summation order, two calls give the same bits.
//
// Arithmetic: f32 VALU fma chains, every product rounded once (sha_attn.hip's header gives the argument
// against the MFMA at this intensity); fp32 softmax with the row maximum subtracted, one wave per row.
#include "common.h"
#include "../../include/newsrec_hip.h"

namespace {

constexpr int DEB_THREADS = 256;
constexpr int DEB_D = 64;             // head width
constexpr int DEB_LD = DEB_D + 4;     // LDS row stride (floats)
constexpr int DEB_MAX_L = 64;
constexpr int DEB_MAX_HEADS = 1024;
constexpr int DEB_WALKERS = 512;      // workgroups the backward aims for (2 per CU)
constexpr size_t DEB_MAX_LDS = 160 * 1024;

struct DebArgs {
  const float* qkv; int64_t ldq; int64_t hstride; int64_t qoff; int64_t koff; int64_t voff;
  const float* pk; const float* pq; int64_t ldp;
  const void* mask; int mask_dtype;
  int nseq; int L; int heads; float scale;
  float pscale; uint32_t thresh; uint32_t key; const uint64_t* rng; uint64_t offset;
  float* probs;
  float* ctx; int64_t ldc;
  const float* dctx; int64_t ldd;
  float* dqkv; int64_t lddq;
  float* dpk; float* dpq; int64_t lddp;
  float* work; int G;
};

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

__device__ __forceinline__ void fma4(float4& acc, float s, const float4& x) {
  acc.x = fmaf(s, x.x, acc.x); acc.y = fmaf(s, x.y, acc.y);
  acc.z = fmaf(s, x.z, acc.z); acc.w = fmaf(s, x.w, acc.w);
}

__device__ __forceinline__ float dot4(const float4& x, const float4& y, float s) {
  s = fmaf(x.x, y.x, s); s = fmaf(x.y, y.y, s);
  s = fmaf(x.z, y.z, s); s = fmaf(x.w, y.w, s);
  return s;
}

// Stage 64 columns of `rows` rows (ld apart) in dst [rows_pad][DEB_LD]; rows in [rows, rows_pad) are zero.
__device__ __forceinline__ void deb_load(float* dst, const float* src, int64_t ld, int rows, int rows_pad, int tid) {
  for (int idx = tid; idx < rows_pad * (DEB_D / 4); idx += DEB_THREADS) {
    const int r = idx >> 4, c = 4 * (idx & 15);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < rows) v = ld4(src + (int64_t)r * ld + c);
    st4(dst + r * DEB_LD + c, v);
  }
}

template <int N>
__device__ __forceinline__ void deb_zero(float4 (&acc)[N]) {
#pragma unroll
  for (int a = 0; a < N; ++a) acc[a] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// acc[a] += sum_t M[ti + 16 a][t] X[t][4 tj .. 4 tj + 3] over t in [0, LR): M's columns and X's rows in
// [L, LR) are zero; M's rows are clamped to mrows - 1 (those results are never stored).
template <int N>
__device__ __forceinline__ void deb_mm(const float* M, int mrows, const float* X, int ti, int tj, int LR,
                                       float4 (&acc)[N]) {
  int mr[N];
#pragma unroll
  for (int a = 0; a < N; ++a) mr[a] = min(ti + 16 * a, mrows - 1) * DEB_LD;
#pragma unroll 2
  for (int t = 0; t < LR; t += 4) {
    const float4 x0 = ld4(X + (t + 0) * DEB_LD + 4 * tj);
    const float4 x1 = ld4(X + (t + 1) * DEB_LD + 4 * tj);
    const float4 x2 = ld4(X + (t + 2) * DEB_LD + 4 * tj);
    const float4 x3 = ld4(X + (t + 3) * DEB_LD + 4 * tj);
#pragma unroll
    for (int a = 0; a < N; ++a) {
      const float4 m = ld4(M + mr[a] + t);
      fma4(acc[a], m.x, x0); fma4(acc[a], m.y, x1); fma4(acc[a], m.z, x2); fma4(acc[a], m.w, x3);
    }
  }
}

// The skewed matrix's two products in one walk over the queries t: with d = min(ti + 16 a, 2L - 1) a position
// row and sk[d][t] = dS[t][t + L - d],
//   accq[a] += sum_t sk[d][t] Q[t]            (dpk: the query of the pair, shared by every a)
//   acck[a] += sum_t sk[d][t] Kk[t + L - d]   (dpq: the KEY of the pair, a row of its own per a)
// sk is zero wherever t + L - d is no key of the title or t >= L, so the key row is clamped into the tile.
template <int N>
__device__ __forceinline__ void deb_mm_skew(const float* SK, const float* Q, const float* Kk, int ti, int tj, int L,
                                            int LR, float4 (&accq)[N], float4 (&acck)[N]) {
  int d[N];
#pragma unroll
  for (int a = 0; a < N; ++a) d[a] = min(ti + 16 * a, 2 * L - 1);
#pragma unroll 1
  for (int t = 0; t < LR; t += 4) {
    float4 x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = ld4(Q + (t + u) * DEB_LD + 4 * tj);
#pragma unroll
    for (int a = 0; a < N; ++a) {
      const float4 m = ld4(SK + d[a] * DEB_LD + t);
      const float mv[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        fma4(accq[a], mv[u], x[u]);
        const int j = min(max(t + u + L - d[a], 0), LR - 1);
        fma4(acck[a], mv[u], ld4(Kk + j * DEB_LD + 4 * tj));
      }
    }
  }
}

// The position product: acc[a] += sum_t M[r][t] PP[delta][4 tj .. 4 tj + 3] with r = ti + 16 a and
// delta = r - t + L (QUERY_ROWS: M = dS, r a query, t a key) or t - r + L (M = dS^T, r a key, t a query).
// PP holds 2L initialised rows; delta is clamped into them where r or t lies in the padding, and there M
// is zero or the result is never stored.
template <int N, bool QUERY_ROWS>
__device__ __forceinline__ void deb_mm_pos(const float* M, const float* PP, int ti, int tj, int L, int LR,
                                           float4 (&acc)[N]) {
  int r[N];
#pragma unroll
  for (int a = 0; a < N; ++a) r[a] = min(ti + 16 * a, LR - 1);
  const int top = 2 * L - 1;
#pragma unroll 1
  for (int t = 0; t < LR; t += 4) {
#pragma unroll
    for (int a = 0; a < N; ++a) {
      const float4 m = ld4(M + r[a] * DEB_LD + t);
      const float mv[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int d = QUERY_ROWS ? r[a] - (t + u) + L : (t + u) - r[a] + L;
        fma4(acc[a], mv[u], ld4(PP + min(max(d, 0), top) * DEB_LD + 4 * tj));
      }
    }
  }
}

// Rows ti + 16 a < rows of the float4 column group tj -> out (ld apart).
template <int N>
__device__ __forceinline__ void deb_store(float* out, int64_t ld, const float4 (&acc)[N], int ti, int tj, int rows) {
#pragma unroll
  for (int a = 0; a < N; ++a) {
    const int i = ti + 16 * a;
    if (i < rows) st4(out + (int64_t)i * ld + 4 * tj, acc[a]);
  }
}

__device__ __forceinline__ uint32_t deb_key(const DebArgs& g) {
  return g.rng ? nr_dropout_key(g.rng[0], g.rng[1] + g.offset) : g.key;
}

// One workgroup per (title, head).  NA = ceil(L / 16): the 16-row thread tiles a title uses.
template <int NA>
__global__ __launch_bounds__(DEB_THREADS) void deb_attn_fwd_kernel(DebArgs g) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int L = g.L, P2 = 2 * L;
  const int LR = (L + 3) & ~3;
  float* xa = sm;                    // q, then v
  float* xb = xa + LR * DEB_LD;      // k
  float* ps = xb + LR * DEB_LD;      // scores, then the dropped probabilities
  float* pp = ps + LR * DEB_LD;      // pk, then pq  [2L][DEB_LD]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ti = tid >> 4, tj = tid & 15;
  const int64_t s = blockIdx.x / g.heads;
  const int h = blockIdx.x % g.heads;
  const float* base = g.qkv + s * L * g.ldq + h * g.hstride;
  const uint32_t key = deb_key(g);

  deb_load(xa, base + g.qoff, g.ldq, L, LR, tid);
  deb_load(xb, base + g.koff, g.ldq, L, LR, tid);
  deb_load(pp, g.pk + DEB_D * h, g.ldp, P2, P2, tid);
  __syncthreads();
  // query rows ti + 16 a, mirrored key rows L - 1 - (tj + 16 b), position rows ti + tj + 1 + 16 (a + b)
  int xr[NA], yr[NA], pr[2 * NA - 1];
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    xr[a] = min(ti + 16 * a, LR - 1) * DEB_LD;
    yr[a] = max(L - 1 - tj - 16 * a, 0) * DEB_LD;
  }
#pragma unroll
  for (int n = 0; n < 2 * NA - 1; ++n) pr[n] = min(ti + tj + 1 + 16 * n, P2 - 1) * DEB_LD;
  float acc[NA][NA];
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int b = 0; b < NA; ++b) acc[a][b] = 0.f;
  // q . k + q . pk[delta]
#pragma unroll 2
  for (int c = 0; c < DEB_D; c += 4) {
    float4 x[NA], y[NA], p[2 * NA - 1];
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      x[a] = ld4(xa + xr[a] + c);
      y[a] = ld4(xb + yr[a] + c);
    }
#pragma unroll
    for (int n = 0; n < 2 * NA - 1; ++n) p[n] = ld4(pp + pr[n] + c);
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
      for (int b = 0; b < NA; ++b) acc[a][b] = dot4(x[a], p[a + b], dot4(x[a], y[b], acc[a][b]));
  }
  __syncthreads();
  deb_load(pp, g.pq + DEB_D * h, g.ldp, P2, P2, tid);
  deb_load(xa, base + g.voff, g.ldq, L, LR, tid);
  __syncthreads();
  // + k . pq[delta]
#pragma unroll 2
  for (int c = 0; c < DEB_D; c += 4) {
    float4 y[NA], p[2 * NA - 1];
#pragma unroll
    for (int a = 0; a < NA; ++a) y[a] = ld4(xb + yr[a] + c);
#pragma unroll
    for (int n = 0; n < 2 * NA - 1; ++n) p[n] = ld4(pp + pr[n] + c);
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
      for (int b = 0; b < NA; ++b) acc[a][b] = dot4(y[b], p[a + b], acc[a][b]);
  }
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int b = 0; b < NA; ++b) {
      const int i = ti + 16 * a, j = L - 1 - tj - 16 * b;
      if (i < L && j >= 0) ps[i * DEB_LD + j] = acc[a][b] * g.scale;
    }
  __syncthreads();
  const bool valid = lane < L && nr_mask_at(g.mask, g.mask_dtype, s * L + lane);
  const float uniform = 1.f / (float)L;
  for (int i = wave; i < L; i += DEB_THREADS / 64) {
    const bool qi = nr_mask_at(g.mask, g.mask_dtype, s * L + i);   // wave-uniform
    const float x = valid ? ps[i * DEB_LD + lane] : -INFINITY;
    const float m = nr_wave_max(x);
    const float e = valid ? expf(x - m) : 0.f;
    const float sum = nr_wave_sum(e);
    float p = valid ? e / sum : 0.f;
    if (!qi) p = lane < L ? uniform : 0.f;
    const uint64_t elem = (((uint64_t)s * g.heads + h) * L + i) * L + lane;
    if (lane < L) g.probs[elem] = p;
    if (lane < LR) ps[i * DEB_LD + lane] = nr_dropout_keep(key, (uint32_t)elem, g.thresh) ? p * g.pscale : 0.f;
  }
  __syncthreads();
  float4 o[NA];
  deb_zero(o);
  deb_mm(ps, LR, xa, ti, tj, LR, o);
  deb_store(g.ctx + s * L * g.ldc + DEB_D * h, g.ldc, o, ti, tj, L);
}

// Workgroup (gi, h) = blockIdx.x / heads, % heads walks the titles gi, gi + G, ... of head h.
template <int NA>
__global__ __launch_bounds__(DEB_THREADS) void deb_attn_bwd_kernel(DebArgs g) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int L = g.L, P2 = 2 * L;
  const int LR = (L + 3) & ~3;
  const int MS = LR * DEB_LD;
  float* xa = sm;                    // dctx, then k
  float* xb = xa + MS;               // v, then (P * keep / (1 - p))^T [key][query], then q
  float* ds = xb + MS;               // dPd, then scale * dS [query][key]
  float* dst = ds + MS;              // scale * dS^T [key][query]
  float* sk = dst + MS;              // sk[delta][i] = scale * dS[i][i + L - delta]  [2L][DEB_LD]
  float* pp = sk + P2 * DEB_LD;      // pk, then pq  [2L][DEB_LD]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ti = tid >> 4, tj = tid & 15;
  const int h = blockIdx.x % g.heads;
  const int gi = blockIdx.x / g.heads;
  const uint32_t key = deb_key(g);

  // the entries of sk no (i, j) of a title maps to stay zero for the whole walk; the others are rewritten
  // by every title
  for (int idx = tid; idx < P2 * DEB_LD; idx += DEB_THREADS) sk[idx] = 0.f;
  float4 apk[2 * NA], apq[2 * NA];
  deb_zero(apk);
  deb_zero(apq);

  for (int64_t s = gi; s < g.nseq; s += g.G) {
    const float* base = g.qkv + s * L * g.ldq + h * g.hstride;
    float* dbase = g.dqkv + s * L * g.lddq + h * g.hstride;
    deb_load(xa, g.dctx + s * L * g.ldd + DEB_D * h, g.ldd, L, LR, tid);
    deb_load(xb, base + g.voff, g.ldq, L, LR, tid);
    deb_load(pp, g.pk + DEB_D * h, g.ldp, P2, P2, tid);
    __syncthreads();
    {  // dPd = dctx v^T
      int xr[NA], yr[NA];
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        xr[a] = min(ti + 16 * a, LR - 1) * DEB_LD;
        yr[a] = min(tj + 16 * a, LR - 1) * DEB_LD;
      }
      float acc[NA][NA];
#pragma unroll
      for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int b = 0; b < NA; ++b) acc[a][b] = 0.f;
#pragma unroll 2
      for (int c = 0; c < DEB_D; c += 4) {
        float4 x[NA], y[NA];
#pragma unroll
        for (int a = 0; a < NA; ++a) {
          x[a] = ld4(xa + xr[a] + c);
          y[a] = ld4(xb + yr[a] + c);
        }
#pragma unroll
        for (int a = 0; a < NA; ++a)
#pragma unroll
          for (int b = 0; b < NA; ++b) acc[a][b] = dot4(x[a], y[b], acc[a][b]);
      }
#pragma unroll
      for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int b = 0; b < NA; ++b) {
          const int i = ti + 16 * a, j = tj + 16 * b;
          if (i < L && j < L) ds[i * DEB_LD + j] = acc[a][b];
        }
    }
    __syncthreads();
    // per query row: g = dPd * keep / (1 - p), dS = P (g - sum_j g P), zero for a query with mask 0 (its
    // probabilities are constants); rows and columns in [L, LR) are zero
    for (int i = wave; i < LR; i += DEB_THREADS / 64) {
      const bool in = i < L && lane < L;
      const bool qi = i < L && nr_mask_at(g.mask, g.mask_dtype, s * L + i);   // wave-uniform
      const uint64_t elem = (((uint64_t)s * g.heads + h) * L + i) * L + lane;
      const float p = in ? g.probs[elem] : 0.f;
      const bool keep = nr_dropout_keep(key, (uint32_t)elem, g.thresh);
      const float gg = in && keep ? ds[i * DEB_LD + lane] * g.pscale : 0.f;
      const float r = nr_wave_sum(gg * p);
      const float d = qi ? p * (gg - r) * g.scale : 0.f;
      const float pd = keep ? p * g.pscale : 0.f;
      if (lane < LR) {
        ds[i * DEB_LD + lane] = d;
        dst[lane * DEB_LD + i] = d;
        xb[lane * DEB_LD + i] = pd;
      }
      if (in) sk[(i + L - lane) * DEB_LD + i] = d;
    }
    __syncthreads();
    float4 o[NA];
    deb_zero(o);
    deb_mm(xb, LR, xa, ti, tj, LR, o);                 // dV = Pd^T dctx
    deb_store(dbase + g.voff, g.lddq, o, ti, tj, L);
    __syncthreads();
    deb_load(xa, base + g.koff, g.ldq, L, LR, tid);
    deb_load(xb, base + g.qoff, g.ldq, L, LR, tid);
    __syncthreads();
    deb_zero(o);
    deb_mm(ds, LR, xa, ti, tj, LR, o);                 // dQ = dS k + sum_j dS[i][j] pk[delta(i, j)]
    deb_mm_pos<NA, true>(ds, pp, ti, tj, L, LR, o);
    deb_store(dbase + g.qoff, g.lddq, o, ti, tj, L);
    deb_zero(o);
    deb_mm(dst, LR, xb, ti, tj, LR, o);                // dK = dS^T q + sum_i dS[i][j] pq[delta(i, j)]
    deb_mm_skew(sk, xb, xa, ti, tj, L, LR, apk, apq);  // dpk[d] += sk[d] q, dpq[d] += sum_i sk[d][i] k[i + L - d]
    __syncthreads();
    deb_load(pp, g.pq + DEB_D * h, g.ldp, P2, P2, tid);
    __syncthreads();
    deb_mm_pos<NA, false>(dst, pp, ti, tj, L, LR, o);
    deb_store(dbase + g.koff, g.lddq, o, ti, tj, L);
    __syncthreads();
  }
  float* part = g.work + ((int64_t)gi * g.heads + h) * 2 * P2 * DEB_D;
  deb_store(part, DEB_D, apk, ti, tj, P2);
  deb_store(part + P2 * DEB_D, DEB_D, apq, ti, tj, P2);
}

// dpk / dpq [2L][64 heads] = the G partials of each head added in ascending g; row 0 (no (i, j) maps to it)
// is stored as 0.
__global__ __launch_bounds__(DEB_THREADS) void deb_attn_reduce_kernel(DebArgs g) {
  const int P2 = 2 * g.L;
  const int64_t idx = (int64_t)blockIdx.x * DEB_THREADS + threadIdx.x;
  const int64_t total = (int64_t)2 * P2 * g.heads * (DEB_D / 4);
  if (idx >= total) return;
  const int c = 4 * (int)(idx % (DEB_D / 4));
  const int h = (int)((idx / (DEB_D / 4)) % g.heads);
  const int d = (int)((idx / ((DEB_D / 4) * g.heads)) % P2);
  const int w = (int)(idx / ((int64_t)(DEB_D / 4) * g.heads * P2));
  float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
  if (d > 0)
    for (int gi = 0; gi < g.G; ++gi) {
      const float4 v = ld4(g.work + ((((int64_t)gi * g.heads + h) * 2 + w) * P2 + d) * DEB_D + c);
      sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
    }
  st4((w ? g.dpq : g.dpk) + (int64_t)d * g.lddp + DEB_D * h + c, sum);
}

bool deb_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

bool deb_shape_ok(int64_t nseq, int32_t L, int32_t heads) {
  return nseq >= 0 && L >= 1 && L <= DEB_MAX_L && heads >= 1 && heads <= DEB_MAX_HEADS &&
         nseq * heads <= 0x7fffffff;
}

int deb_walkers(int64_t nseq, int32_t heads) {
  const int64_t cap = DEB_WALKERS / heads > 1 ? DEB_WALKERS / heads : 1;
  return (int)(nseq < cap ? nseq : cap);
}

int64_t deb_work_bytes(int64_t nseq, int32_t L, int32_t heads) {
  return (int64_t)deb_walkers(nseq, heads) * heads * 2 * (2 * L) * DEB_D * (int64_t)sizeof(float);
}

bool deb_far(int64_t a, int64_t b) { return a - b >= DEB_D || b - a >= DEB_D; }

// A [rows][ld] matrix with `heads` blocks of 64 columns at q / k / v's places.
bool deb_layout_ok(int64_t ld, int64_t hstride, int64_t qoff, int64_t koff, int64_t voff, int32_t heads) {
  if (ld % 4 || ld < DEB_D || ld > 0x7fffffff || hstride % 4 || hstride < DEB_D || hstride > ld || qoff % 4 ||
      koff % 4 || voff % 4 || qoff < 0 || koff < 0 || voff < 0)
    return false;
  if (!deb_far(qoff, koff) || !deb_far(qoff, voff) || !deb_far(koff, voff)) return false;
  const int64_t top = qoff > koff ? (qoff > voff ? qoff : voff) : (koff > voff ? koff : voff);
  return (heads - 1) * hstride + top + DEB_D <= ld;
}

// The shared argument checks -> NR_OK or the invalid-argument code.
int deb_setup(DebArgs& g, const float* qkv, int64_t ldq, int64_t hstride, int64_t qoff, int64_t koff, int64_t voff,
              const float* pk, const float* pq, int64_t ldp, const void* mask, int32_t mask_dtype, int64_t nseq,
              int32_t L, int32_t heads, float scale, float p_drop, uint64_t seed, uint64_t offset,
              const uint64_t* rng, const float* probs) {
  if (!deb_shape_ok(nseq, L, heads) || !deb_layout_ok(ldq, hstride, qoff, koff, voff, heads) || ldp % 4 ||
      ldp < (int64_t)DEB_D * heads || !(p_drop >= 0.f && p_drop < 1.f) || mask_dtype < NR_MASK_U8 ||
      mask_dtype > NR_MASK_F32)
    return NR_EINVAL(0);
  if (!qkv || !pk || !pq || !mask || !probs) return NR_EINVAL(1);
  if (!deb_al16(qkv) || !deb_al16(pk) || !deb_al16(pq) || ((uintptr_t)probs & 3)) return NR_EINVAL(0);
  g.qkv = qkv; g.ldq = ldq; g.hstride = hstride; g.qoff = qoff; g.koff = koff; g.voff = voff;
  g.pk = pk; g.pq = pq; g.ldp = ldp; g.mask = mask; g.mask_dtype = mask_dtype;
  g.nseq = (int)nseq; g.L = L; g.heads = heads; g.scale = scale;
  g.pscale = p_drop > 0.f ? 1.f / (1.f - p_drop) : 1.f;
  g.thresh = nr_dropout_threshold(p_drop);
  g.key = nr_dropout_key(seed, offset); g.rng = rng; g.offset = offset;
  g.probs = const_cast<float*>(probs);
  return NR_OK;
}

template <typename Kern>
int deb_launch_one(Kern kern, unsigned blocks, size_t smem, hipStream_t stream, const DebArgs& g) {
  if (smem > 64 * 1024 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess)
    return -(int)hipGetLastError();
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(DEB_THREADS), smem, stream, g);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

// LDS bytes of the forward (3 [LR] tiles + one [2L] tile) and the backward (4 + 2).
size_t deb_smem(int L, bool fwd) {
  const size_t LR = (L + 3) & ~3;
  return ((fwd ? 3 : 4) * LR + (fwd ? 2 : 4) * (size_t)L) * DEB_LD * sizeof(float);
}

// What the kernels are compiled for: DEB_THREADS threads (their launch bound) and at most DEB_MAX_LDS of LDS.
bool deb_launchable(int threads, size_t smem) { return threads <= DEB_THREADS && smem <= DEB_MAX_LDS; }

// The instantiation for NA = ceil(L / 16) 16-row thread tiles.
template <bool FWD>
int deb_launch(unsigned blocks, hipStream_t stream, const DebArgs& g) {
  const size_t smem = deb_smem(g.L, FWD);
#define DEB_CASE(NA)                                                                                    \
  case NA:                                                                                              \
    return FWD ? deb_launch_one(deb_attn_fwd_kernel<NA>, blocks, smem, stream, g)                       \
               : deb_launch_one(deb_attn_bwd_kernel<NA>, blocks, smem, stream, g)
  switch ((g.L + 15) >> 4) {
    DEB_CASE(1);
    DEB_CASE(2);
    DEB_CASE(3);
    default: break;
  }
  return FWD ? deb_launch_one(deb_attn_fwd_kernel<4>, blocks, smem, stream, g)
             : deb_launch_one(deb_attn_bwd_kernel<4>, blocks, smem, stream, g);
#undef DEB_CASE
}

}  // namespace

extern "C" int64_t nr_deb_attn_bwd_workspace(int64_t nseq, int32_t L, int32_t heads) {
  if (!deb_shape_ok(nseq, L, heads)) return NR_EINVAL(0);
  return deb_work_bytes(nseq, L, heads);
}

extern "C" int nr_deb_attn_fwd(const float* qkv, int64_t ldq, int64_t hstride, int64_t qoff, int64_t koff,
                               int64_t voff, const float* pk, const float* pq, int64_t ldp, const void* mask,
                               int32_t mask_dtype, int64_t nseq, int32_t L, int32_t heads, float scale, float p_drop,
                               uint64_t seed, uint64_t offset, const uint64_t* rng, float* probs, float* ctx,
                               int64_t ldc, hipStream_t stream) {
  DebArgs g{};
  if (ldc % 4 || ldc < (int64_t)DEB_D * heads) return NR_EINVAL(0);
  const int rc = deb_setup(g, qkv, ldq, hstride, qoff, koff, voff, pk, pq, ldp, mask, mask_dtype, nseq, L, heads,
                           scale, p_drop, seed, offset, rng, probs);
  if (rc != NR_OK) return rc;
  if (!ctx) return NR_EINVAL(1);
  if (!deb_al16(ctx) || !deb_launchable(DEB_THREADS, deb_smem(L, true))) return NR_EINVAL(0);
  if (nseq == 0) return NR_OK;
  g.ctx = ctx; g.ldc = ldc;
  return deb_launch<true>((unsigned)(nseq * heads), stream, g);
}

extern "C" int nr_deb_attn_bwd(const float* qkv, int64_t ldq, int64_t hstride, int64_t qoff, int64_t koff,
                               int64_t voff, const float* pk, const float* pq, int64_t ldp, const void* mask,
                               int32_t mask_dtype, int64_t nseq, int32_t L, int32_t heads, float scale, float p_drop,
                               uint64_t seed, uint64_t offset, const uint64_t* rng, const float* probs,
                               const float* dctx, int64_t ldd, float* dqkv, int64_t lddq, float* dpk, float* dpq,
                               int64_t lddp, float* work, int64_t work_bytes, hipStream_t stream) {
  DebArgs g{};
  if (ldd % 4 || ldd < (int64_t)DEB_D * heads || !deb_layout_ok(lddq, hstride, qoff, koff, voff, heads) ||
      lddp % 4 || lddp < (int64_t)DEB_D * heads)
    return NR_EINVAL(0);
  const int rc = deb_setup(g, qkv, ldq, hstride, qoff, koff, voff, pk, pq, ldp, mask, mask_dtype, nseq, L, heads,
                           scale, p_drop, seed, offset, rng, probs);
  if (rc != NR_OK) return rc;
  if (work_bytes < deb_work_bytes(nseq, L, heads)) return NR_EINVAL(0);
  if (!dctx || !dqkv || !dpk || !dpq || (!work && nseq > 0)) return NR_EINVAL(1);
  if (!deb_al16(dctx) || !deb_al16(dqkv) || !deb_al16(dpk) || !deb_al16(dpq) || !deb_al16(work) ||
      !deb_launchable(DEB_THREADS, deb_smem(L, false)))
    return NR_EINVAL(0);
  if (nseq == 0) return NR_OK;
  g.dctx = dctx; g.ldd = ldd; g.dqkv = dqkv; g.lddq = lddq; g.dpk = dpk; g.dpq = dpq; g.lddp = lddp;
  g.work = work; g.G = deb_walkers(nseq, heads);
  const int rc2 = deb_launch<false>((unsigned)(g.G * heads), stream, g);
  if (rc2 != NR_OK) return rc2;
  const int64_t total = (int64_t)2 * 2 * L * heads * (DEB_D / 4);
  hipLaunchKernelGGL(deb_attn_reduce_kernel, dim3((unsigned)((total + DEB_THREADS - 1) / DEB_THREADS)),
                     dim3(DEB_THREADS), 0, stream, g);
  NR_LAUNCH_CHECK();
  return NR_OK;
}
