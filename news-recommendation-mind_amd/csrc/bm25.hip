// Sparse (BM25) recall (`--mode recall -rt s`, utils/Manager.py:52,117-119): the token-level inverted index
// of utils/utils.py:219-246 (construct_inverted_index over BM25_token, :287-342) built on the device, its
// per-news view, and the exact top-K search over that view (the reference builds the index and leaves the
// search out).  The definition, quirks included, is in include/newsrec_hip.h.
//
// Build.  nr_bm25_count: one lane per corpus row (rows staged in LDS) adds the row's term frequencies to
//   df and counts its postings per token -- integer atomics, exact.  The host forms idf from df (math.log:
//   the reference's bits).  nr_bm25_build: a one-workgroup scan turns the posting counts into offsets; the
//   rows scatter one 64-bit key per posting into the token's range of a scratch buffer (slot = an atomic
//   cursor: arbitrary); one workgroup per token then finds the key of rank P by a radix select over the
//   range (five 8-bit digits, LDS histograms), collects the keys at or above it and ranks them by counting.
//   Within a token idf is constant and tf (k + 1) / (tf + k) rises with tf, so the list order (score
//   descending, row ascending) is the order of
//     key = (idf > 0 ? tf : idf < 0 ? 63 - tf : 0) << 40 | (2^31 - 1 - row) << 8 | tf
//   -- distinct per posting, so the P best are a set that no arrival order changes.  The score is formed
//   from the key's tf at the end: ((idf * tf) * (k + 1)) / (tf + k) in fp64, two multiplies and a divide.
// View.  nr_bm25_forward: one lane per posting finds its token's first column in its row and stores the
//   score (rounded once to fp32) there and the column's bit in the row's keep word.
// Query.  bm25_topk_kernel: grid = (16-user tiles) x (n_slices ranges of 64-news tiles).  A workgroup holds
//   its users' query-token bitmaps in LDS, per wave and word-major ([wave][word][4 users]: the four users of
//   a wave are one 16-byte read, and the lanes' random words fall on all banks) and their exclude ids,
//   streams the tiles' tok / fwd rows through LDS (the next tile's rows and keep words are loaded into
//   registers before the current tile is summed), and lane j of wave w sums news j of the tile for users
//   4w .. 4w+3 over the kept columns in ascending order.  Selection as in topk.hip: 64-bit
//   entries (score key << 32 | 2^31 - 1 - id), a per-user buffer that only its wave touches, ranked by
//   counting when it would overflow; bm25_merge_kernel ranks the slices' sorted lists.  No float atomics;
//   the result does not depend on n_slices.
#include "common.h"
#include "../../include/newsrec_hip.h"

#include <math.h>

namespace {

constexpr int NT = 256;          // threads of the select, forward, query and merge kernels
constexpr int CR = 128;          // corpus rows per workgroup of the count / scatter kernels (one per lane)
constexpr int SCAN_NT = 1024;
constexpr int QU = 16;           // users per query workgroup
constexpr int UW = QU / 4;       // ... per wave
constexpr int QN = 64;           // news per query tile (one per lane)
constexpr int MAX_SLICES = 64;
constexpr int N_CU = 256;
constexpr int LDS_BYTES = 160 * 1024;
constexpr int64_t EMPTY = INT64_MIN;

extern __shared__ __attribute__((aligned(16))) unsigned char bm25_smem[];

struct Special { int a, b, c; };

__device__ __forceinline__ bool in_range(int t, int V) { return (unsigned)t < (unsigned)V; }
__device__ __forceinline__ bool indexable(int t, int V, Special sp) {
  return in_range(t, V) && t != sp.a && t != sp.b && t != sp.c;
}

// rows r0 .. r0 + CR - 1 of tok into S[CR][LS]; rows past R are not read (their lanes return early)
__device__ __forceinline__ void stage_rows(int* S, const int32_t* __restrict__ tok, int64_t ldt, int64_t r0, int64_t R,
                                           int L, int LS, int nrows, int tid, int nthreads) {
  for (int i = tid; i < nrows * L; i += nthreads) {
    const int r = i / L, l = i - r * L;
    if (r0 + r < R) S[r * LS + l] = tok[(r0 + r) * ldt + l];
  }
}

// ------------------------------------------------------------------------------------------------ build
__global__ __launch_bounds__(CR) void bm25_count_kernel(const int32_t* __restrict__ tok, int64_t ldt, int64_t R, int L,
                                                        int V, Special sp, unsigned long long* __restrict__ df,
                                                        int32_t* __restrict__ n_post, int32_t* status) {
  int* S = reinterpret_cast<int*>(bm25_smem);
  const int LS = L | 1, tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * CR;
  stage_rows(S, tok, ldt, r0, R, L, LS, CR, tid, CR);
  __syncthreads();
  if (r0 + tid >= R) return;
  const int* row = S + tid * LS;
  bool bad = false;
  for (int l = 0; l < L; ++l) {
    const int t = row[l];
    if (!in_range(t, V)) {
      bad = true;
      continue;
    }
    bool first_any = true, first_body = l >= 1;      // first in the row / first in columns 1 ..
    for (int j = 0; j < l; ++j)
      if (row[j] == t) {
        first_any = false;
        if (j >= 1) first_body = false;
      }
    if (first_any && t != sp.a && t != sp.b && t != sp.c) atomicAdd(&n_post[t], 1);
    if (first_body) {
      int tf = 0;
      for (int j = l; j < L; ++j) tf += row[j] == t;
      atomicAdd(&df[t], (unsigned long long)tf);
    }
  }
  if (bad) atomicOr(status, NR_BM25_BAD_TOKEN);
}

// off[t] = the postings of the tokens below t, off[V] = all of them (one workgroup)
__global__ __launch_bounds__(SCAN_NT) void bm25_scan_kernel(const int32_t* __restrict__ n_post, int V,
                                                            int64_t* __restrict__ off) {
  __shared__ int64_t part[SCAN_NT];
  const int tid = threadIdx.x, per = (V + SCAN_NT - 1) / SCAN_NT;
  const int b = min(tid * per, V), e = min(b + per, V);
  int64_t s = 0;
  for (int i = b; i < e; ++i) s += max(n_post[i], 0);
  part[tid] = s;
  __syncthreads();
  for (int d = 1; d < SCAN_NT; d <<= 1) {
    const int64_t v = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int64_t run = part[tid] - s;
  for (int i = b; i < e; ++i) {
    off[i] = run;
    run += max(n_post[i], 0);
  }
  if (tid == SCAN_NT - 1) off[V] = part[tid];
}

__global__ __launch_bounds__(CR) void bm25_scatter_kernel(const int32_t* __restrict__ tok, int64_t ldt, int64_t R, int L,
                                                          int V, Special sp, const double* __restrict__ idf,
                                                          const int32_t* __restrict__ n_post,
                                                          const int64_t* __restrict__ off, int32_t* __restrict__ cursor,
                                                          int64_t* __restrict__ ent, int64_t cap) {
  int* S = reinterpret_cast<int*>(bm25_smem);
  const int LS = L | 1, tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * CR;
  stage_rows(S, tok, ldt, r0, R, L, LS, CR, tid, CR);
  __syncthreads();
  const int64_t n = r0 + tid;
  if (n >= R) return;
  const int* row = S + tid * LS;
  for (int l = 0; l < L; ++l) {
    const int t = row[l];
    if (!indexable(t, V, sp)) continue;
    bool first = true;
    for (int j = 0; j < l; ++j) first &= row[j] != t;
    if (!first) continue;
    int tf = 0;
    for (int j = 1; j < L; ++j) tf += row[j] == t;
    const double w = idf[t];
    const int rk = w > 0.0 ? tf : w < 0.0 ? 63 - tf : 0;
    const int64_t key = ((int64_t)rk << 40) | ((int64_t)(0x7FFFFFFF - (int)n) << 8) | (int64_t)tf;
    // (a count that does not belong to this corpus must not send a store outside the token's range)
    const int c = atomicAdd(&cursor[t], 1);
    const int64_t pos = off[t] + c;
    if (c < n_post[t] && pos < cap) ent[pos] = key;
  }
}

// One workgroup per token: its list, best first, padded with (R, +0.0).
__global__ __launch_bounds__(NT) void bm25_select_kernel(const int64_t* __restrict__ ent, int64_t cap,
                                                         const int64_t* __restrict__ off,
                                                         const int32_t* __restrict__ cursor,
                                                         const int32_t* __restrict__ n_post,
                                                         const double* __restrict__ idf, int64_t R, int P, int k,
                                                         int32_t* __restrict__ post_ids,
                                                         double* __restrict__ post_scores) {
  __shared__ int64_t sel[NR_BM25_MAX_POSTINGS];
  __shared__ int hist[256];
  __shared__ int n_sel, remaining;
  __shared__ int64_t prefix;
  const int t = blockIdx.x, tid = threadIdx.x;
  const int64_t o = off[t];
  int64_t c64 = min(cursor[t], n_post[t]);
  if (c64 > cap - o) c64 = cap - o;
  const int c = c64 > 0 ? (int)c64 : 0;
  const int64_t* base = ent + o;
  const int m = min(c, P);
  if (tid == 0) {
    n_sel = 0;
    remaining = P;
    prefix = 0;
  }
  __syncthreads();
  if (c > P) {
    // the key >> 8 of rank P - 1 (keys >> 8 are distinct), digit by digit from the top
    for (int shift = 40; shift >= 8; shift -= 8) {
      hist[tid] = 0;
      __syncthreads();
      const int64_t pre = prefix;
      for (int i = tid; i < c; i += NT) {
        const int64_t e = base[i];
        if ((e >> (shift + 8)) == pre) atomicAdd(&hist[(int)(e >> shift) & 255], 1);
      }
      __syncthreads();
      if (tid == 0) {
        int above = 0, d = 255;
        while (d > 0 && above + hist[d] < remaining) above += hist[d--];
        remaining -= above;
        prefix = (pre << 8) | d;
      }
      __syncthreads();
    }
  }
  const int64_t thr = prefix;                     // 0 when the whole range is taken
  for (int i = tid; i < c; i += NT) {
    const int64_t e = base[i];
    if ((e >> 8) >= thr) {
      const int slot = atomicAdd(&n_sel, 1);      // where it lands does not matter: ranked below
      if (slot < m) sel[slot] = e;
    }
  }
  __syncthreads();
  const int have = min(n_sel, m);
  const double w = idf[t];
  for (int i = tid; i < have; i += NT) {
    const int64_t e = sel[i];
    int rank = 0;
    for (int j = 0; j < have; ++j) rank += sel[j] > e;
    const int tf = (int)(e & 255);
    post_ids[(int64_t)t * P + rank] = 0x7FFFFFFF - (int)((e >> 8) & 0x7FFFFFFF);
    post_scores[(int64_t)t * P + rank] = ((w * (double)tf) * (double)(k + 1)) / (double)(tf + k);
  }
  for (int i = have + tid; i < P; i += NT) {
    post_ids[(int64_t)t * P + i] = (int32_t)R;
    post_scores[(int64_t)t * P + i] = 0.0;
  }
}

__global__ __launch_bounds__(NT) void bm25_forward_kernel(const int32_t* __restrict__ tok, int64_t ldt, int64_t R, int L,
                                                          int64_t VP, int P, const int32_t* __restrict__ post_ids,
                                                          const double* __restrict__ post_scores,
                                                          float* __restrict__ fwd, int64_t ldf,
                                                          unsigned long long* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= VP) return;
  const int64_t n = post_ids[i];
  if (n < 0 || n >= R) return;
  const int t = (int)(i / P);
  const int32_t* row = tok + n * ldt;
  for (int l = 0; l < L; ++l)
    if (row[l] == t) {
      fwd[n * ldf + l] = (float)post_scores[i];
      atomicOr(&keep[n], 1ull << l);
      break;
    }
}

// ------------------------------------------------------------------------------------------------ query
__device__ __forceinline__ int64_t entry_pack(float s, int id) {
  int b = __float_as_int(s);
  if (b == (int)0x80000000) b = 0;                       // -0.0 ties with +0.0
  const int key = b >= 0 ? b : b ^ 0x7FFFFFFF;           // signed order of key == order of the floats
  return (int64_t)(((uint64_t)(uint32_t)key << 32) | (uint32_t)(0x7FFFFFFF - id));
}
__device__ __forceinline__ float entry_score(int64_t e) {
  const int key = (int)(e >> 32);
  return e == EMPTY ? -INFINITY : __int_as_float(key >= 0 ? key : key ^ 0x7FFFFFFF);
}
__device__ __forceinline__ int64_t entry_id(int64_t e) {
  return e == EMPTY ? -1 : (int64_t)(0x7FFFFFFF - (int)(uint32_t)e);
}

// LDS written by some lanes of a wave and read by others: order the accesses for the compiler (the
// hardware runs one wave's LDS instructions in order)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Ranks the cnt (<= 192, wave-uniform) distinct entries of the buffer at 64-bit word `off` of the LDS
// array by counting and stores those of rank < K at their rank: buf[0 .. min(cnt, K)) sorted, best first.
// -> buf[K - 1] (the new threshold when cnt >= K).
__device__ __attribute__((noinline)) int64_t wave_compact(int off, int cnt, int K, int lane) {
  int64_t* buf = reinterpret_cast<int64_t*>(bm25_smem) + off;
  wave_lds_sync();
  int64_t e[3];
  int rk[3] = {0, 0, 0};
#pragma unroll
  for (int i = 0; i < 3; ++i) e[i] = 64 * i + lane < cnt ? buf[64 * i + lane] : EMPTY;
  for (int j = 0; j < cnt; ++j) {
    const int64_t x = buf[j];
#pragma unroll
    for (int i = 0; i < 3; ++i) rk[i] += x > e[i];
  }
  wave_lds_sync();
#pragma unroll
  for (int i = 0; i < 3; ++i)
    if (64 * i + lane < cnt && rk[i] < K) buf[rk[i]] = e[i];
  wave_lds_sync();
  return buf[K - 1];
}

typedef uint32_t bm_words __attribute__((ext_vector_type(UW)));     // a wave's users' words: one LDS read
constexpr int SE = QN * NR_BM25_MAX_L / NT;                         // elements of a tile a thread stages, at most

__global__ __launch_bounds__(NT) void bm25_topk_kernel(const int32_t* __restrict__ qtok, int64_t ldq, int64_t U, int Tq,
                                                       const int32_t* __restrict__ tok, int64_t ldt,
                                                       const float* __restrict__ fwd, int64_t ldf,
                                                       const unsigned long long* __restrict__ keep, int64_t R, int L,
                                                       int V, Special sp, int K, int C, int64_t first_row,
                                                       const uint8_t* __restrict__ row_mask,
                                                       const int64_t* __restrict__ exclude, int E, int n_slices,
                                                       int64_t* __restrict__ top_ids, float* __restrict__ top_scores,
                                                       int64_t* __restrict__ ws) {
  const int words = (V + 31) >> 5, nL = QN * L;
  int64_t* lists = reinterpret_cast<int64_t*>(bm25_smem);            // [QU][C]
  uint32_t* bm = reinterpret_cast<uint32_t*>(lists + QU * C);        // [4 waves][words][UW]
  uint32_t* xbits = bm + (size_t)words * QU;                         // [QU][2]
  int* tokS = reinterpret_cast<int*>(xbits + QU * 2);                // [QN][L]
  float* fwdS = reinterpret_cast<float*>(tokS + nL);                 // [QN][L]
  int* exS = reinterpret_cast<int*>(fwdS + nL);                      // [QU][E]: exclude ids, -1 = none

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t u0 = (int64_t)blockIdx.x * QU;
  const int slice = blockIdx.y;
  const int64_t n_tiles = (R + QN - 1) / QN;
  const int64_t t_begin = slice * n_tiles / n_slices, t_end = (slice + 1) * n_tiles / n_slices;

  for (int i = tid; i < QU * C; i += NT) lists[i] = EMPTY;
  for (int i = tid; i < words * QU; i += NT) bm[i] = 0u;
  __syncthreads();
  for (int ul = 0; ul < QU && u0 + ul < U; ++ul) {
    const int32_t* q = qtok + (u0 + ul) * ldq;
    for (int i = tid; i < Tq; i += NT) {
      const int t = q[i];
      if (indexable(t, V, sp)) atomicOr(&bm[((ul / UW) * words + (t >> 5)) * UW + ul % UW], 1u << (t & 31));
    }
  }
  for (int i = tid; i < QU * E; i += NT) {
    const int64_t u = u0 + i / E;
    const int64_t v = u < U ? exclude[u * E + i % E] : -1;
    exS[i] = v >= 0 && v < R ? (int)v : -1;
  }
  __syncthreads();

  // candidate buffers of this wave's users: entries held and the entry a newcomer has to beat
  int cnt[UW];
  int64_t thr[UW];
  bool uval[UW];
#pragma unroll
  for (int r = 0; r < UW; ++r) {
    cnt[r] = 0;
    thr[r] = EMPTY;
    uval[r] = u0 + UW * w + r < U;
  }
  const unsigned long long lmask = L >= 64 ? ~0ull : (1ull << L) - 1ull;
  const unsigned long long below = (1ull << lane) - 1ull;
  uint32_t* xb = xbits + 2 * UW * w;                                  // this wave's users
  const uint32_t* bmw = bm + (size_t)w * words * UW;

  // a tile's rows and keep words, global memory -> registers (one tile ahead of the sums)
  const bool contig = ldt == L && ldf == L;
  int rt[SE];
  float rf[SE];
  unsigned long long kp_next = 0ull;
  auto gload = [&](int64_t tile) {
    const int64_t n0 = tile * QN;
#pragma unroll
    for (int j = 0; j < SE; ++j) {
      const int i = tid + NT * j;
      rt[j] = 0;
      rf[j] = 0.f;
      if (i < nL) {
        int64_t gt, gf;
        bool ok;
        if (contig) {
          gt = gf = n0 * L + i;
          ok = gt < R * L;
        } else {
          const int r = i / L, l = i - r * L;
          gt = (n0 + r) * ldt + l;
          gf = (n0 + r) * ldf + l;
          ok = n0 + r < R;
        }
        if (ok) {
          rt[j] = tok[gt];
          rf[j] = fwd[gf];
        }
      }
    }
    const int64_t n = n0 + lane;
    kp_next = 0ull;
    if (n < R && n >= first_row && (!row_mask || row_mask[n] != 0)) kp_next = keep[n] & lmask;
  };

  if (t_begin < t_end) gload(t_begin);
  for (int64_t tile = t_begin; tile < t_end; ++tile) {
    const int64_t n0 = tile * QN, n = n0 + lane;
    __syncthreads();                                                  // the previous tile's reads are done
#pragma unroll
    for (int j = 0; j < SE; ++j) {
      const int i = tid + NT * j;
      if (i < nL) {
        tokS[i] = rt[j];
        fwdS[i] = rf[j];
      }
    }
    unsigned long long kp = kp_next;
    // the exclude ids of this wave's users that fall into the tile, one bit per news
    if (E > 0) {
      if (lane < 2 * UW) xb[lane] = 0u;
      wave_lds_sync();
      for (int i = lane; i < UW * E; i += 64) {
        const int64_t d = (int64_t)exS[UW * w * E + i] - n0;
        if (d >= 0 && d < QN) atomicOr(&xb[(i / E) * 2 + (int)(d >> 5)], 1u << (int)(d & 31));
      }
      wave_lds_sync();
    }
    __syncthreads();
    if (tile + 1 < t_end) gload(tile + 1);
    // this lane's news against the wave's users, kept columns in ascending order
    float s[UW];
#pragma unroll
    for (int r = 0; r < UW; ++r) s[r] = 0.f;
    unsigned hit = 0u;
    while (kp) {
      const int l = __builtin_ctzll(kp);
      kp &= kp - 1ull;
      const int t = tokS[lane * L + l];
      if (!in_range(t, V)) continue;
      const bm_words b = *reinterpret_cast<const bm_words*>(bmw + (t >> 5) * UW);
      const float f = fwdS[lane * L + l];
      const unsigned bit = 1u << (t & 31);
#pragma unroll
      for (int r = 0; r < UW; ++r)
        if (b[r] & bit) {
          s[r] += f;
          hit |= 1u << r;
        }
    }
#pragma unroll
    for (int r = 0; r < UW; ++r) {
      const bool excl = E > 0 && ((xb[r * 2 + (lane >> 5)] >> (lane & 31)) & 1u);
      const bool cand = ((hit >> r) & 1u) && uval[r] && !excl;
      const int64_t c = entry_pack(s[r], (int)n);
      bool pass = cand && c > thr[r];
      unsigned long long m = __ballot(pass);
      if (m) {
        int hits = __popcll(m);
        if (cnt[r] + hits > C) {
          // (overflow: cnt > C - 64 >= K, so the K-th entry exists and K + hits fits afterwards)
          thr[r] = wave_compact((UW * w + r) * C, cnt[r], K, lane);
          cnt[r] = K;
          pass = cand && c > thr[r];
          m = __ballot(pass);
          hits = __popcll(m);
        }
        if (pass) lists[(UW * w + r) * C + cnt[r] + __popcll(m & below)] = c;
        cnt[r] += hits;
      }
    }
  }

  // sort what each user holds (the K best in front), then each wave writes its own users' lists
#pragma unroll
  for (int r = 0; r < UW; ++r)
    if (cnt[r] > 0) wave_compact((UW * w + r) * C, cnt[r], K, lane);
  wave_lds_sync();
  for (int ul = UW * w; ul < UW * w + UW; ++ul) {
    const int64_t u = u0 + ul;
    if (u >= U) break;
    for (int p = lane; p < K; p += 64) {
      const int64_t e = lists[ul * C + p];
      if (n_slices == 1) {
        top_ids[u * K + p] = entry_id(e);
        top_scores[u * K + p] = entry_score(e);
      } else {
        ws[(u * n_slices + slice) * K + p] = e;
      }
    }
  }
}

// One workgroup per user: rank of an entry = its position in its own list + the entries of the other
// lists that beat it (real entries are distinct; empty slots tie and cover the ranks after the last one).
__global__ __launch_bounds__(NT) void bm25_merge_kernel(const int64_t* __restrict__ ws, int K, int n_slices,
                                                        int64_t* __restrict__ top_ids,
                                                        float* __restrict__ top_scores) {
  int64_t* Ls = reinterpret_cast<int64_t*>(bm25_smem);              // [n_slices][K]
  const int64_t u = blockIdx.x;
  const int total = n_slices * K;
  for (int i = threadIdx.x; i < total; i += NT) Ls[i] = ws[u * total + i];
  __syncthreads();
  for (int i = threadIdx.x; i < total; i += NT) {
    const int a = i / K;
    const int64_t e = Ls[i];
    int rank = i - a * K;
    for (int b = 0; b < n_slices && rank < K; ++b) {
      if (b == a) continue;
      const int64_t* lb = Ls + b * K;
      int lo = 0, hi = K;                                           // first position with lb[pos] <= e
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (lb[mid] > e) lo = mid + 1;
        else hi = mid;
      }
      rank += lo;
    }
    if (rank < K) {
      top_ids[u * K + rank] = entry_id(e);
      top_scores[u * K + rank] = entry_score(e);
    }
  }
}

// ------------------------------------------------------------------------------------------------ host
// entries of a user's candidate buffer: whole waves of lanes, at least K + 64 (a tile appends up to 64)
int buf_entries(int K) { return K <= 64 ? 128 : 192; }

size_t rows_lds(int L) { return (size_t)CR * (L | 1) * sizeof(int); }

size_t topk_lds(int K, int V, int L, int E) {
  return (size_t)QU * buf_entries(K) * sizeof(int64_t) + (size_t)((V + 31) / 32) * QU * 4 + QU * 2 * 4 +
         (size_t)2 * QN * L * 4 + (size_t)QU * E * 4;
}

// enough slices for two workgroups per CU
int auto_slices(int64_t U, int64_t R) {
  const int64_t user_tiles = (U + QU - 1) / QU, n_tiles = (R + QN - 1) / QN;
  int64_t s = user_tiles > 0 ? (2 * N_CU + user_tiles - 1) / user_tiles : 1;
  if (s > MAX_SLICES) s = MAX_SLICES;
  if (s > n_tiles) s = n_tiles;
  return s < 1 ? 1 : (int)s;
}

bool corpus_ok(int64_t R, int32_t L, int32_t V) {
  return R >= 0 && R <= 0x7FFFFFFF && L >= 1 && L <= NR_BM25_MAX_L && V >= 1 && (R + CR - 1) / CR <= 0x7FFFFFFF;
}

int64_t build_ws_bytes(int64_t R, int32_t L, int32_t V) {
  return ((int64_t)V + 1) * 8 + R * L * 8 + ((int64_t)V * 4 + 7) / 8 * 8;
}

// nt against the kernel's own launch bound (asked of the runtime once per kernel: `bound` is the caller's
// cache slot), and the dynamic LDS limit raised when the launch needs more than 64 KB
template <typename Kern>
int launch_fits(Kern kern, int nt, size_t lds, int* bound) {
  if (lds > (size_t)LDS_BYTES) return 0;
  if (*bound == 0) {
    hipFuncAttributes attr;
    if (hipFuncGetAttributes(&attr, (const void*)kern) != hipSuccess) return 0;
    *bound = attr.maxThreadsPerBlock;
  }
  if (*bound < nt) return 0;
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return 0;
  return 1;
}

#define NR_HIP_CHECK(call)                       \
  do {                                           \
    hipError_t e__ = (call);                     \
    if (e__ != hipSuccess) return -(int)e__;     \
  } while (0)

}  // namespace

extern "C" int nr_bm25_count(const int32_t* tok, int64_t ldt, int64_t R, int32_t L, int32_t V, int32_t special0,
                             int32_t special1, int32_t special2, int64_t* df, int32_t* n_post, int32_t* status,
                             hipStream_t stream) {
  if (!corpus_ok(R, L, V)) return NR_EINVAL(0);
  if (!df || !n_post || !status || (R > 0 && !tok)) return NR_EINVAL(1);
  if (ldt < L) return NR_EINVAL(4);
  static int bound;
  if (!launch_fits(bm25_count_kernel, CR, rows_lds(L), &bound)) return NR_EINVAL(7);
  NR_HIP_CHECK(hipMemsetAsync(df, 0, (size_t)V * 8, stream));
  NR_HIP_CHECK(hipMemsetAsync(n_post, 0, (size_t)V * 4, stream));
  if (R == 0) return NR_OK;
  hipLaunchKernelGGL(bm25_count_kernel, dim3((unsigned)((R + CR - 1) / CR)), dim3(CR), rows_lds(L), stream, tok, ldt,
                     R, (int)L, (int)V, Special{special0, special1, special2}, (unsigned long long*)df, n_post,
                     status);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

extern "C" int64_t nr_bm25_build_workspace(int64_t R, int32_t L, int32_t V) {
  return corpus_ok(R, L, V) ? build_ws_bytes(R, L, V) : 0;
}

extern "C" int nr_bm25_build(const int32_t* tok, int64_t ldt, int64_t R, int32_t L, int32_t V, int32_t P, int32_t k,
                             int32_t special0, int32_t special1, int32_t special2, const double* idf,
                             const int32_t* n_post, int32_t* post_ids, double* post_scores, void* workspace,
                             int64_t workspace_bytes, hipStream_t stream) {
  if (!corpus_ok(R, L, V) || k < 1 || workspace_bytes < 0) return NR_EINVAL(0);
  if (!idf || !n_post || !post_ids || !post_scores || (R > 0 && !tok)) return NR_EINVAL(1);
  if (P < 1 || P > NR_BM25_MAX_POSTINGS) return NR_EINVAL(2);
  if (ldt < L) return NR_EINVAL(4);
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < build_ws_bytes(R, L, V)) return NR_EINVAL(6);
  static int bounds[3];
  if (!launch_fits(bm25_scan_kernel, SCAN_NT, 0, &bounds[0]) ||
      !launch_fits(bm25_scatter_kernel, CR, rows_lds(L), &bounds[1]) ||
      !launch_fits(bm25_select_kernel, NT, 0, &bounds[2]))
    return NR_EINVAL(7);
  int64_t* off = (int64_t*)workspace;
  int64_t* ent = off + V + 1;
  const int64_t cap = R * L;
  int32_t* cursor = (int32_t*)(ent + cap);
  const Special sp{special0, special1, special2};
  NR_HIP_CHECK(hipMemsetAsync(cursor, 0, (size_t)V * 4, stream));
  hipLaunchKernelGGL(bm25_scan_kernel, dim3(1), dim3(SCAN_NT), 0, stream, n_post, (int)V, off);
  NR_LAUNCH_CHECK();
  if (R > 0) {
    hipLaunchKernelGGL(bm25_scatter_kernel, dim3((unsigned)((R + CR - 1) / CR)), dim3(CR), rows_lds(L), stream, tok,
                       ldt, R, (int)L, (int)V, sp, idf, n_post, (const int64_t*)off, cursor, ent, cap);
    NR_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(bm25_select_kernel, dim3((unsigned)V), dim3(NT), 0, stream, (const int64_t*)ent, cap,
                     (const int64_t*)off, (const int32_t*)cursor, n_post, idf, R, (int)P, (int)k, post_ids,
                     post_scores);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

extern "C" int nr_bm25_forward(const int32_t* tok, int64_t ldt, int64_t R, int32_t L, int32_t V, int32_t P,
                               const int32_t* post_ids, const double* post_scores, float* fwd, int64_t ldf,
                               uint64_t* keep, hipStream_t stream) {
  if (!corpus_ok(R, L, V)) return NR_EINVAL(0);
  if (!post_ids || !post_scores || (R > 0 && (!tok || !fwd || !keep))) return NR_EINVAL(1);
  if (P < 1 || P > NR_BM25_MAX_POSTINGS) return NR_EINVAL(2);
  if (ldt < L || ldf < L) return NR_EINVAL(4);
  if (R == 0) return NR_OK;
  static int bound;
  if (!launch_fits(bm25_forward_kernel, NT, 0, &bound)) return NR_EINVAL(7);
  NR_HIP_CHECK(hipMemset2DAsync(fwd, (size_t)ldf * 4, 0, (size_t)L * 4, (size_t)R, stream));
  NR_HIP_CHECK(hipMemsetAsync(keep, 0, (size_t)R * 8, stream));
  const int64_t VP = (int64_t)V * P;
  hipLaunchKernelGGL(bm25_forward_kernel, dim3((unsigned)((VP + NT - 1) / NT)), dim3(NT), 0, stream, tok, ldt, R,
                     (int)L, VP, (int)P, post_ids, post_scores, fwd, ldf, (unsigned long long*)keep);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

extern "C" int64_t nr_bm25_topk_workspace(int64_t U, int64_t R, int32_t K, int32_t n_slices) {
  if (U < 0 || R < 0 || R > 0x7FFFFFFF || K < 1 || K > NR_TOPK_MAX_K || n_slices < 0 || n_slices > MAX_SLICES ||
      (U + QU - 1) / QU > 0x7FFFFFFF)
    return 0;
  const int ns = n_slices ? n_slices : auto_slices(U, R);
  return U * ns * K * (int64_t)sizeof(int64_t);
}

extern "C" int nr_bm25_topk(const int32_t* qtok, int64_t ldq, int64_t U, int32_t Tq, const int32_t* tok, int64_t ldt,
                            const float* fwd, int64_t ldf, const uint64_t* keep, int64_t R, int32_t L, int32_t V,
                            int32_t special0, int32_t special1, int32_t special2, int32_t K, int64_t first_row,
                            const uint8_t* row_mask, const int64_t* exclude, int32_t E, int32_t n_slices,
                            int64_t* top_ids, float* top_scores, void* workspace, int64_t workspace_bytes,
                            hipStream_t stream) {
  if (U < 0 || Tq < 0 || !corpus_ok(R, L, V) || E < 0 || first_row < 0 || n_slices < 0 || workspace_bytes < 0)
    return NR_EINVAL(0);
  if (K < 1 || K > NR_TOPK_MAX_K) return NR_EINVAL(2);
  if (E > NR_TOPK_MAX_EXCLUDE) return NR_EINVAL(3);
  if (ldt < L || ldf < L || ldq < Tq) return NR_EINVAL(4);
  if (n_slices > MAX_SLICES || (U + QU - 1) / QU > 0x7FFFFFFF) return NR_EINVAL(5);
  if (U == 0) return NR_OK;
  if (!top_ids || !top_scores || (Tq > 0 && !qtok) || (R > 0 && (!tok || !fwd || !keep))) return NR_EINVAL(1);
  if (!exclude) E = 0;
  const int ns = n_slices ? n_slices : auto_slices(U, R);
  if (ns > 1) {
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < U * ns * K * (int64_t)sizeof(int64_t))
      return NR_EINVAL(6);
  }
  const size_t lds1 = topk_lds(K, V, L, E);
  const size_t lds2 = (size_t)ns * K * sizeof(int64_t);
  static int bounds[2];
  if (!launch_fits(bm25_topk_kernel, NT, lds1, &bounds[0]) ||
      (ns > 1 && !launch_fits(bm25_merge_kernel, NT, lds2, &bounds[1])))
    return NR_EINVAL(7);
  hipLaunchKernelGGL(bm25_topk_kernel, dim3((unsigned)((U + QU - 1) / QU), (unsigned)ns), dim3(NT), lds1, stream, qtok,
                     ldq, U, (int)Tq, tok, ldt, fwd, ldf, (const unsigned long long*)keep, R, (int)L, (int)V,
                     Special{special0, special1, special2}, (int)K, buf_entries(K), first_row, row_mask, exclude,
                     (int)E, ns, top_ids, top_scores, (int64_t*)workspace);
  NR_LAUNCH_CHECK();
  if (ns > 1) {
    hipLaunchKernelGGL(bm25_merge_kernel, dim3((unsigned)U), dim3(NT), lds2, stream, (const int64_t*)workspace, (int)K,
                       ns, top_ids, top_scores);
    NR_LAUNCH_CHECK();
  }
  return NR_OK;
}
