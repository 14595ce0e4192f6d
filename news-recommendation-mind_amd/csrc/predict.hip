// MIND prediction.txt on the device: the tail of Manager.test (utils/Manager.py:842-850),
//   for pred in preds:
//       rank_list = ss.rankdata(1 - np.asarray(pred), method="ordinal")
//       f.write(str(index) + " [" + ",".join(str(i) for i in rank_list) + "]" + "\n"); index += 1
// over a packed ragged score vector, in two launches around a prefix sum of the line lengths:
//   nr_rank_ordinal       rank[c] of every candidate inside its impression and line_len[g], the
//                         exact byte count of impression g's line
//   nr_format_prediction  the ASCII text, line g at text + line_off[g]
//
// Ranks: pred holds Python floats (fp32 scores widened to double), so the sort key is the DOUBLE
// 1.0 - (double)p.  That map is not injective on fp32: every p below 2^-54 rounds to the key 1.0 and
// neighbouring small p share keys up to 2^-29 or so, and rankdata's ordinal method orders equal keys
// by position.  Hence key_i = 1.0 - (double)preds[i] and
//   rank_i = 1 + #{ j : key_j < key_i or (key_j == key_i and j < i) },
// all in f64; "descending fp32 score" gives other ranks.
//
// One WAVE per impression in both kernels, as metrics_kernel (MIND impressions average ~37
// candidates, the largest have ~300): lane l owns candidates l, l + 64, ...
#include "common.h"
#include "../../include/newsrec_hip.h"

namespace {

// decimal digits of v (str(v) without a sign)
__device__ __forceinline__ int digits_u32(uint32_t v) {
  return 1 + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) +
         (v >= 10000000u) + (v >= 100000000u) + (v >= 1000000000u);
}

// (compares against powers of ten: a 64-bit division is a long instruction sequence here)
__device__ __forceinline__ int digits_u64(uint64_t v) {
  int d = 1;
  for (uint64_t p = 10ull; d < 20 && v >= p; p *= 10ull) ++d;
  return d;
}

// the hd = digits_u64(v) decimal digits of v to b[0 .. hd), dividing in 32 bits once v fits
__device__ __forceinline__ void put_u64(uint8_t* b, int hd, uint64_t v) {
  int k = hd;
  while (v > 0xFFFFFFFFull) { b[--k] = (uint8_t)('0' + (int)(v % 10ull)); v /= 10ull; }
  uint32_t w = (uint32_t)v;
  while (k > 0) { b[--k] = (uint8_t)('0' + (int)(w % 10u)); w /= 10u; }
}

__device__ __forceinline__ int wave_sum_i32(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The O(n^2) count reads the group's scores straight from global memory at wave-uniform
// addresses (one broadcast load per j, L1/L2 resident), as metrics_kernel does.  The cap bounds the
// run time of one wave; the host entry enforces it on the caller's max_group, and a group that is
// larger all the same (or has a negative size) is flagged and left unranked, never ranked wrongly.
__global__ __launch_bounds__(256) void rank_ordinal_kernel(const float* preds, const int64_t* grp_off, int64_t G,
                                                           int64_t first_line, int32_t* rank, int64_t* line_len,
                                                           int32_t* status) {
  const int lane = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (g >= G) return;
  const int64_t o0 = grp_off[g];
  const int64_t n64 = grp_off[g + 1] - o0;
  if (n64 < 0 || n64 > NR_RANK_MAX_GROUP) {
    if (lane == 0) {
      atomicOr(status, NR_RANK_GROUP_TOO_LARGE);
      line_len[g] = 0;
    }
    return;
  }
  const int n = (int)n64;
  const float* P = preds + o0;
  int dsum = 0;       // digits of this lane's ranks
  bool nan = false;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    const bool live = i < n;
    const float pi = live ? P[i] : 0.f;
    const double ki = 1.0 - (double)pi;
    int r = 0;
    for (int j = 0; j < n; ++j) {
      const double kj = 1.0 - (double)P[j];
      r += (kj < ki) | ((kj == ki) & (j < i));
    }
    if (!live) continue;
    nan |= pi != pi;
    rank[o0 + i] = r + 1;
    dsum += digits_u32((uint32_t)(r + 1));
  }
  if (nan) atomicOr(status, NR_RANK_NAN);
  dsum = wave_sum_i32(dsum);
  // str(line) + " [" + digits and n - 1 commas + "]\n"
  if (lane == 0)
    line_len[g] = (int64_t)digits_u64((uint64_t)(first_line + g)) + 4 + (int64_t)dsum + (n > 0 ? n - 1 : 0);
}

// Bytes of LDS per wave of format_kernel: one segment is the line's head (at most 20 digits and
// " ["), 64 ranks of at most 10 digits and a separator each, the closing "]\n" of an empty line, and up
// to 3 bytes in front that put the segment at its global address modulo 4.
constexpr int FMT_SEG = 768;
static_assert(3 + 22 + 64 * 11 + 2 <= FMT_SEG, "segment buffer");

// LDS written by some lanes of a wave, read by others: order the accesses for the compiler (the
// hardware runs one wave's LDS instructions in order)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A line is assembled in segments of 64 candidates: each lane's bytes (its rank's digits and one
// separator, "," or the closing "]") start at the wave prefix sum of digits + 1; the segment is
// built in LDS at the byte phase of its global address and leaves as aligned dwords, with byte
// stores only for the partial dwords at its two ends.  Nothing is stored at or past text_bytes.
__global__ __launch_bounds__(256) void format_kernel(const int32_t* rank, const int64_t* grp_off,
                                                     const int64_t* line_off, int64_t G, int64_t first_line,
                                                     uint8_t* text, int64_t text_bytes) {
  __shared__ __attribute__((aligned(16))) uint8_t s_seg[4][FMT_SEG];
  const int lane = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (g >= G) return;
  uint8_t* seg = s_seg[threadIdx.x >> 6];
  const int64_t o0 = grp_off[g];
  const int64_t n = grp_off[g + 1] - o0;
  int64_t gpos = line_off[g];        // byte offset in text of the next segment
  if (gpos < 0) return;
  int64_t i0 = 0;
  do {
    const int mis = (int)((uintptr_t)(text + gpos) & 3);
    uint8_t* b = seg + mis;
    int len = 0;
    if (i0 == 0) {
      const uint64_t v = (uint64_t)(first_line + g);
      const int hd = digits_u64(v);
      if (lane == 0) {
        put_u64(b, hd, v);
        b[hd] = ' ';
        b[hd + 1] = '[';
      }
      len = hd + 2;
    }
    const int64_t i = i0 + lane;
    const bool live = i < n;
    uint32_t r = live ? (uint32_t)rank[o0 + i] : 0u;
    const int d = live ? digits_u32(r) : 0;
    int incl = live ? d + 1 : 0;
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(incl, o, 64);
      if (lane >= o) incl += y;
    }
    const int total = __shfl(incl, 63, 64);
    if (live) {
      uint8_t* p = b + len + incl - (d + 1);
      for (int k = d - 1; k >= 0; --k) { p[k] = (uint8_t)('0' + (int)(r % 10u)); r /= 10u; }
      p[d] = i == n - 1 ? ']' : ',';
    }
    len += total;
    if (i0 + 64 >= n) {
      if (lane == 0) {
        if (n == 0) b[len] = ']';
        b[len + (n == 0)] = '\n';
      }
      len += 1 + (n == 0);
    }
    wave_lds_sync();
    // LDS byte k of the segment <-> global byte base[k]; k in [first, end)
    const int64_t room = text_bytes - gpos;
    const int first = mis;
    const int end = mis + (int)(room < (int64_t)len ? (room > 0 ? room : 0) : (int64_t)len);
    uint8_t* base = text + gpos - mis;
    const int ds = (first + 3) >> 2, de = end >> 2;
    if (ds <= de) {
      if (lane < ds * 4 - first) base[first + lane] = seg[first + lane];
      for (int w = ds + lane; w < de; w += 64)
        reinterpret_cast<uint32_t*>(base)[w] = reinterpret_cast<const uint32_t*>(seg)[w];
      if (lane < end - de * 4) base[de * 4 + lane] = seg[de * 4 + lane];
    } else if (lane < end - first) {
      base[first + lane] = seg[first + lane];
    }
    wave_lds_sync();
    gpos += len;
    i0 += 64;
  } while (i0 < n);
}

}  // namespace

extern "C" int nr_rank_ordinal(const float* preds, const int64_t* grp_off, int64_t G, int64_t first_line,
                               int64_t max_group, int32_t* rank, int64_t* line_len, int32_t* status,
                               hipStream_t stream) {
  if (G < 0 || first_line < 0 || max_group < 0) return NR_EINVAL(0);
  // (an empty array has no address to give: line_len with G == 0, preds / rank with no candidates)
  if (!grp_off || !status || (G > 0 && !line_len) || (max_group > 0 && (!preds || !rank))) return NR_EINVAL(1);
  if (max_group > NR_RANK_MAX_GROUP) return NR_EINVAL(2);
  if (G == 0) return NR_OK;
  if ((G + 3) / 4 > 0x7FFFFFFF) return NR_EINVAL(3);
  hipLaunchKernelGGL(rank_ordinal_kernel, dim3((unsigned)((G + 3) / 4)), dim3(256), 0, stream, preds, grp_off, G,
                     first_line, rank, line_len, status);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

extern "C" int nr_format_prediction(const int32_t* rank, const int64_t* grp_off, const int64_t* line_off, int64_t G,
                                    int64_t first_line, uint8_t* text, int64_t text_bytes, hipStream_t stream) {
  if (G < 0 || first_line < 0 || text_bytes < 0) return NR_EINVAL(0);
  if (!grp_off || !line_off || (G > 0 && !text)) return NR_EINVAL(1);
  if (G == 0) return NR_OK;
  if ((G + 3) / 4 > 0x7FFFFFFF) return NR_EINVAL(2);
  // the shortest line is "N []\n"
  if (text_bytes / 5 < G) return NR_EINVAL(3);
  hipLaunchKernelGGL(format_kernel, dim3((unsigned)((G + 3) / 4)), dim3(256), 0, stream, rank, grp_off, line_off, G,
                     first_line, text, text_bytes);
  NR_LAUNCH_CHECK();
  return NR_OK;
}
