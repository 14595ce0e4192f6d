// Exact full-corpus top-K retrieval (dense recall, utils/Manager.py:45,52,117-119; the reference leaves
// the search to an external ANN index): for every user the K best rows of the whole news table under
//   s[i][j] = (fmaf chain over k = 0 .. H-1 of user[i][k] * table[j][k], from 0.f) * (1 / sqrt(H))
// ordered by (score descending, row id ascending), without the [U, N] score matrix ever reaching HBM.
//
// Scores come from v_mfma_f32_16x16x4_f32 with the k-tiles accumulated in ascending order: bit for bit
// the k-ordered fmaf chain, so the value -- and with it the top-K boundary -- does not depend on the
// tiling or the launch geometry.  Rows past H are zero in LDS (fma(0, 0, acc) == acc).
//
// Phase 1 (topk_slice_kernel): grid = (64-user tiles) x (n_slices contiguous ranges of 128-news tiles).
//   A workgroup streams its slice through LDS in 32-wide k chunks; wave w owns users 16w .. 16w+15 of the
//   tile and all 128 news of a tile (eight 16x16 accumulators), and it alone touches those users'
//   candidate buffers, so the selection needs no workgroup barrier.  An entry is 64 bits
//   (order-preserving score key << 32 | 0x7FFFFFFF - id): signed compare IS (score desc, id asc), a total
//   order with no equal real entries, so the K best of a set do not depend on the order of arrival.
//   Per user: a buffer of C >= K + 32 entries, a count and a threshold.  Per accumulator register one
//   ballot tests the entries against the thresholds; the lanes that pass append in parallel (slot = count
//   + passing lanes below); a buffer that would overflow is first ranked by counting (every lane holds
//   up to three entries and compares them with all), which leaves its K best sorted in front and raises
//   the threshold to the K-th.  Where an append lands in the buffer never reaches the result: only the
//   set does.  The user's exclude ids that fall into the tile are a 128-bit map built per tile.
// Phase 2 (topk_merge_kernel): one workgroup per user ranks every entry of its n_slices sorted lists by
//   position + binary searches in the other lists, and writes the entries of rank < K.
// No float atomics: the output is a pure function of the inputs.
#include "common.h"
#include "../../include/newsrec_hip.h"

#include <math.h>

namespace {

constexpr int TU = 64;          // users per workgroup (16 per wave)
constexpr int TN = 128;         // news per tile
constexpr int KC = 32;          // k per LDS chunk
constexpr int LDK = KC + 2;     // LDS row stride: rows 2 banks apart, the 16 rows x 2 k of a half wave on 32 banks
constexpr int NT = 256;         // threads per workgroup (the launch bound of both kernels)
constexpr int MAX_SLICES = 64;
constexpr int N_CU = 256;
constexpr int LDS_BYTES = 160 * 1024;
constexpr int STAGE_BYTES = (TU + TN) * LDK * 4;    // the operand chunks
constexpr int XBITS_BYTES = TU * 4 * 4;             // per user 128 exclude bits of the current tile
constexpr int64_t EMPTY = INT64_MIN; // an unused list slot: below every real entry

// all LDS of both kernels (dynamic): one array, also reached from wave_compact
extern __shared__ __attribute__((aligned(16))) unsigned char topk_smem[];

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

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
// -> buf[K - 1] (the new threshold when cnt >= K).  Called from 32 unrolled places, rarely: kept out of line.
__device__ __attribute__((noinline)) int64_t wave_compact(int off, int cnt, int K, int lane) {
  int64_t* buf = reinterpret_cast<int64_t*>(topk_smem) + off;
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

template <bool VEC>
__device__ __forceinline__ f32x4 load4(const float* row, int k, int H, bool valid) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (!valid) return v;
  if (VEC) {
    if (k < H) v = *reinterpret_cast<const f32x4*>(row + k);      // H % 4 == 0: all four or none
  } else {
    if (k < H) v[0] = row[k];
    if (k + 1 < H) v[1] = row[k + 1];
    if (k + 2 < H) v[2] = row[k + 2];
    if (k + 3 < H) v[3] = row[k + 3];
  }
  return v;
}

__device__ __forceinline__ void store4(float* dst, f32x4 v) {     // 8-byte aligned (LDK even)
  reinterpret_cast<f32x2*>(dst)[0] = f32x2{v[0], v[1]};
  reinterpret_cast<f32x2*>(dst)[1] = f32x2{v[2], v[3]};
}

// VEC: 16-byte loads (H, ldt, ldu multiples of 4 and 16-byte aligned bases), else guarded scalar loads.
template <bool VEC>
__global__ __launch_bounds__(NT) void topk_slice_kernel(const float* __restrict__ table, int64_t ldt, int64_t N,
                                                        const float* __restrict__ user, int64_t ldu, int64_t U,
                                                        int H, int K, int C, int64_t first_row,
                                                        const uint8_t* __restrict__ row_mask,
                                                        const int64_t* __restrict__ exclude, int E, int n_slices,
                                                        float scale, int64_t* __restrict__ top_ids,
                                                        float* __restrict__ top_scores, int64_t* __restrict__ ws,
                                                        int32_t* status) {
  float* Us = reinterpret_cast<float*>(topk_smem);                  // [TU][LDK]
  float* Ns = Us + TU * LDK;                                        // [TN][LDK]
  int64_t* lists = reinterpret_cast<int64_t*>(Ns + TN * LDK);       // [TU][C]
  uint32_t* xbits = reinterpret_cast<uint32_t*>(lists + TU * C);    // [TU][4]

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t u0 = (int64_t)blockIdx.x * TU;
  const int slice = blockIdx.y;
  const int64_t n_tiles = (N + TN - 1) / TN;
  const int64_t t_begin = slice * n_tiles / n_slices, t_end = (slice + 1) * n_tiles / n_slices;
  const int nkc = (H + KC - 1) / KC;

  for (int i = tid; i < TU * C; i += NT) lists[i] = EMPTY;
  __syncthreads();

  // staging: thread -> float4 kq of rows r0 + 32 i
  const int kq = tid & 7, r0 = tid >> 3;
  f32x4 ru[2], rn[4];
  auto gload = [&](int64_t tile, int kc) {
    const int k = kc * KC + kq * 4;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t r = u0 + r0 + 32 * i;
      ru[i] = load4<VEC>(user + r * ldu, k, H, r < U);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t r = tile * TN + r0 + 32 * i;
      rn[i] = load4<VEC>(table + r * ldt, k, H, r < N);
    }
  };

  f32x4 acc[8];
#pragma unroll
  for (int n = 0; n < 8; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};

  // acc[n][r] = user 16 w + 4 fq + r (A rows), news tile * TN + 16 n + fr (B columns)
  const int fr = lane & 15, fq = lane >> 4;
  const float* a_ptr = Us + (16 * w + fr) * LDK + fq;
  const float* b_ptr = Ns + fr * LDK + fq;
  uint32_t* xb = xbits + 64 * w;                                    // this wave's 16 users
  const unsigned long long gmask = 0xFFFFull << (16 * fq);          // the lanes that share my users
  const unsigned long long below = gmask & ((1ull << lane) - 1ull);

  // candidate buffers of my four users: entries held and the entry a newcomer has to beat (the same in
  // all 16 lanes of a group)
  int cnt[4];
  int64_t thr[4];
  bool uval[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    cnt[r] = 0;
    thr[r] = EMPTY;
    uval[r] = u0 + 16 * w + 4 * fq + r < U;
  }
  bool bad = false;

  if (t_begin < t_end) gload(t_begin, 0);
  for (int64_t tile = t_begin; tile < t_end; ++tile) {
    const int64_t j0 = tile * TN;
    // eligibility of this lane's news column of each accumulator
    unsigned elig = 0;
    if (row_mask) {
      uint8_t mb[8];
#pragma unroll
      for (int n = 0; n < 8; ++n) {
        const int64_t j = j0 + 16 * n + fr;
        mb[n] = row_mask[j < N ? j : N - 1];
      }
#pragma unroll
      for (int n = 0; n < 8; ++n) {
        const int64_t j = j0 + 16 * n + fr;
        elig |= (unsigned)(j < N && j >= first_row && mb[n] != 0) << n;
      }
    } else {
#pragma unroll
      for (int n = 0; n < 8; ++n) {
        const int64_t j = j0 + 16 * n + fr;
        elig |= (unsigned)(j < N && j >= first_row) << n;
      }
    }
    // the exclude ids of this wave's users that fall into the tile, one bit per news
    if (E > 0) {
      xb[lane] = 0u;
      wave_lds_sync();
      for (int i = lane; i < 16 * E; i += 64) {
        const int ul = i / E;
        const int64_t u = u0 + 16 * w + ul;
        if (u < U) {
          const int64_t d = exclude[u * E + (i - ul * E)] - j0;
          if (d >= 0 && d < TN) atomicOr(&xb[ul * 4 + (int)(d >> 5)], 1u << (int)(d & 31));
        }
      }
      wave_lds_sync();
    }
    for (int kc = 0; kc < nkc; ++kc) {
      __syncthreads();                       // the previous chunk's fragment reads are done
#pragma unroll
      for (int i = 0; i < 2; ++i) store4(Us + (r0 + 32 * i) * LDK + kq * 4, ru[i]);
#pragma unroll
      for (int i = 0; i < 4; ++i) store4(Ns + (r0 + 32 * i) * LDK + kq * 4, rn[i]);
      __syncthreads();
      if (kc + 1 < nkc) gload(tile, kc + 1);
      else if (tile + 1 < t_end) gload(tile + 1, 0);
#pragma unroll
      for (int kk = 0; kk < KC; kk += 4) {
        const float a = a_ptr[kk];
#pragma unroll
        for (int n = 0; n < 8; ++n)
          acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b_ptr[16 * n * LDK + kk], acc[n], 0, 0, 0);
      }
    }
    // selection
    uint32_t xw[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int q = 0; q < 4; ++q) xw[r][q] = E > 0 ? xb[(4 * fq + r) * 4 + q] : 0u;
#pragma unroll
    for (int n = 0; n < 8; ++n) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float s = acc[n][r] * scale;
        const bool cand = ((elig >> n) & 1u) && uval[r] && !((xw[r][n >> 1] >> ((n & 1) * 16 + fr)) & 1u);
        bad |= cand && !(fabsf(s) <= 3.402823466e38f);
        const int64_t c = entry_pack(s, (int)j0 + 16 * n + fr);
        bool pass = cand && c > thr[r];
        unsigned long long m = __ballot(pass);
        if (m) {
          int hits = __popcll(m & gmask);
          const unsigned long long ov = __ballot(cnt[r] + hits > C);
          if (ov) {
            // (overflow: cnt > C - 16 >= K + 16, so the K-th entry exists and K + hits fits afterwards)
            for (int g = 0; g < 4; ++g) {
              if (!((ov >> (16 * g)) & 1ull)) continue;
              const int cg = __shfl(cnt[r], 16 * g, 64);
              const int64_t t = wave_compact(STAGE_BYTES / 8 + (16 * w + 4 * g + r) * C, cg, K, lane);
              if (fq == g) {
                cnt[r] = K;
                thr[r] = t;
              }
            }
            pass = cand && c > thr[r];
            m = __ballot(pass);
            hits = __popcll(m & gmask);
          }
          if (pass) lists[(16 * w + 4 * fq + r) * C + cnt[r] + __popcll(m & below)] = c;
          cnt[r] += hits;
        }
      }
      acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  if (__ballot(bad) && lane == 0) atomicOr(status, NR_TOPK_NONFINITE);

  // sort what each user holds (the K best in front), then each wave writes its own users' lists
#pragma unroll
  for (int r = 0; r < 4; ++r)
    for (int g = 0; g < 4; ++g) {
      const int cg = __shfl(cnt[r], 16 * g, 64);
      if (cg > 0) wave_compact(STAGE_BYTES / 8 + (16 * w + 4 * g + r) * C, cg, K, lane);
    }
  for (int ul = 16 * w; ul < 16 * w + 16; ++ul) {
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
// lists that beat it.  Real entries are distinct (disjoint slices), so ranks below the number of real
// entries are a permutation; empty slots tie and land, several at a time with the same bytes, on the
// ranks after the last real entry, covering them up to K - 1.
__global__ __launch_bounds__(NT) void topk_merge_kernel(const int64_t* __restrict__ ws, int K, int n_slices,
                                                        int64_t* __restrict__ top_ids,
                                                        float* __restrict__ top_scores) {
  int64_t* L = reinterpret_cast<int64_t*>(topk_smem);               // [n_slices][K]
  const int64_t u = blockIdx.x;
  const int total = n_slices * K;
  for (int i = threadIdx.x; i < total; i += NT) L[i] = ws[u * total + i];
  __syncthreads();
  for (int i = threadIdx.x; i < total; i += NT) {
    const int a = i / K;
    const int64_t e = L[i];
    int rank = i - a * K;
    for (int b = 0; b < n_slices && rank < K; ++b) {
      if (b == a) continue;
      const int64_t* lb = L + b * K;
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

// entries of a user's candidate buffer: whole waves of lanes, at least K + 32
int buf_entries(int K) { return K <= 32 ? 64 : K <= 96 ? 128 : 192; }

size_t slice_lds(int K) { return (size_t)STAGE_BYTES + (size_t)TU * buf_entries(K) * sizeof(int64_t) + XBITS_BYTES; }

// enough slices for every CU to hold the workgroups its LDS admits (two at most)
int auto_slices(int64_t U, int64_t N, int K) {
  const int64_t user_tiles = (U + TU - 1) / TU, n_tiles = (N + TN - 1) / TN;
  const int64_t target = N_CU * (LDS_BYTES / slice_lds(K) >= 2 ? 2 : 1);
  int64_t s = user_tiles > 0 ? (target + user_tiles - 1) / user_tiles : 1;
  if (s > MAX_SLICES) s = MAX_SLICES;
  if (s > n_tiles) s = n_tiles;
  return s < 1 ? 1 : (int)s;
}

bool sizes_ok(int64_t U, int64_t N, int32_t K, int32_t n_slices) {
  return U >= 0 && N >= 0 && N <= 0x7FFFFFFF && K >= 1 && K <= NR_TOPK_MAX_K && n_slices >= 0 &&
         n_slices <= MAX_SLICES && (U + TU - 1) / TU <= 0x7FFFFFFF;
}

// NT against the kernel's own launch bound (asked of the runtime once per kernel: `bound` is the
// caller's cache slot), and the dynamic LDS limit raised when the launch needs more than 64 KB
template <typename Kern>
int launch_fits(Kern kern, size_t lds, int* bound) {
  if (*bound == 0) {
    hipFuncAttributes attr;
    if (hipFuncGetAttributes(&attr, (const void*)kern) != hipSuccess) return 0;
    *bound = attr.maxThreadsPerBlock;
  }
  if (*bound < NT) return 0;
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return 0;
  return 1;
}

}  // namespace

extern "C" int64_t nr_topk_workspace(int64_t U, int64_t N, int32_t K, int32_t n_slices) {
  if (!sizes_ok(U, N, K, n_slices)) return 0;
  const int ns = n_slices ? n_slices : auto_slices(U, N, K);
  return U * ns * K * (int64_t)sizeof(int64_t);
}

extern "C" int nr_topk_news(const float* table, int64_t ldt, int64_t N, const float* user, int64_t ldu, int64_t U,
                            int32_t H, int32_t K, int64_t first_row, const uint8_t* row_mask,
                            const int64_t* exclude, int32_t E, int32_t n_slices, int64_t* top_ids,
                            float* top_scores, void* workspace, int64_t workspace_bytes, int32_t* status,
                            hipStream_t stream) {
  if (U < 0 || N < 0 || N > 0x7FFFFFFF || H < 1 || E < 0 || first_row < 0 || n_slices < 0 || workspace_bytes < 0)
    return NR_EINVAL(0);
  if (K < 1 || K > NR_TOPK_MAX_K) return NR_EINVAL(2);
  if (E > NR_TOPK_MAX_EXCLUDE) return NR_EINVAL(3);
  if (ldt < H || ldu < H) return NR_EINVAL(4);
  if (n_slices > MAX_SLICES || (U + TU - 1) / TU > 0x7FFFFFFF) return NR_EINVAL(5);
  if (U == 0) return NR_OK;
  if (!user || !top_ids || !top_scores || !status || (N > 0 && !table)) return NR_EINVAL(1);
  if (!exclude) E = 0;
  const int ns = n_slices ? n_slices : auto_slices(U, N, K);
  if (ns > 1) {
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < U * ns * K * (int64_t)sizeof(int64_t))
      return NR_EINVAL(6);
  }
  const bool vec = H % 4 == 0 && ldt % 4 == 0 && ldu % 4 == 0 && ((uintptr_t)table & 15) == 0 &&
                   ((uintptr_t)user & 15) == 0;
  const size_t lds1 = slice_lds(K);
  const size_t lds2 = (size_t)ns * K * sizeof(int64_t);
  auto kern = vec ? topk_slice_kernel<true> : topk_slice_kernel<false>;
  static int bounds[3];
  if (!launch_fits(kern, lds1, &bounds[vec]) || (ns > 1 && !launch_fits(topk_merge_kernel, lds2, &bounds[2])))
    return NR_EINVAL(7);
  const float scale = 1.0f / sqrtf((float)H);
  hipLaunchKernelGGL(kern, dim3((unsigned)((U + TU - 1) / TU), (unsigned)ns), dim3(NT), lds1, stream, table, ldt, N,
                     user, ldu, U, (int)H, (int)K, buf_entries(K), first_row, row_mask, exclude, (int)E, ns, scale, top_ids,
                     top_scores, (int64_t*)workspace, status);
  NR_LAUNCH_CHECK();
  if (ns > 1) {
    hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)U), dim3(NT), lds2, stream, (const int64_t*)workspace,
                       (int)K, ns, top_ids, top_scores);
    NR_LAUNCH_CHECK();
  }
  return NR_OK;
}
