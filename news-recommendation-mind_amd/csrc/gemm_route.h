// Routing of the GEMM entry points: which kernel a call runs on, with which tile, split and
// workspace use.  gemm_route() is a pure host function -- no HIP here, so it compiles with a plain
// C++ compiler and is tested without a GPU (tests/gemm_route_dump.cpp); gemm_f32.hip validates the
// arguments and launches what the route says (generic kernel there, the fast ones in gemm_fast.hip).
#pragma once
#include <stdint.h>

#include "../../include/newsrec_hip.h"

namespace nrfast {

// operand modes of the fast kernels (compile-time parameters there)
enum { KC_PLAIN = 0, KC_GATHER = 1, KC_CONV3 = 2, MN_PLAIN = 3, MN_GATHER = 4, MN_CONV3 = 5 };

// Instantiated (A mode, B mode, transposed accumulators) combinations: transposed accumulators
// (float4 stores) for the store epilogues, C-major for the atomic ones.  The exact-f32 and the
// 128 x 128 split kernels have NR_MODES_KC + NR_MODES_MN, the 256 x BN kernel NR_MODES_BIG.
#define NR_MODES_KC(X)                                                      \
  X(KC_GATHER, KC_PLAIN, true)  /* fused gather + projection (fwd) */       \
  X(KC_CONV3, KC_PLAIN, true)   /* conv as K = 3E GEMM (fwd) */             \
  X(KC_PLAIN, KC_PLAIN, true)   /* plain y = x Wᵀ */                        \
  X(KC_PLAIN, MN_PLAIN, true)   /* dgrad dx = dy W */                       \
  X(KC_PLAIN, MN_PLAIN, false)  /* dgrad scattered into the word-table gradient */
#define NR_MODES_MN(X)                                                      \
  X(MN_PLAIN, MN_GATHER, false) /* wgrad dW = dyᵀ table[ids] */             \
  X(MN_PLAIN, MN_CONV3, false)  /* conv wgrad */                            \
  X(MN_PLAIN, MN_PLAIN, false)  /* wgrad dW = dyᵀ x */
#define NR_MODES_BIG(X)                                                     \
  X(KC_GATHER, KC_PLAIN, true)  /* gathered projection (fwd) */             \
  X(KC_PLAIN, KC_PLAIN, true)   /* y = x Wᵀ */                              \
  X(KC_PLAIN, MN_PLAIN, true)   /* dgrad (store / scatter-store epilogues) */ \
  X(MN_PLAIN, MN_GATHER, false) /* wgrad over gathered rows */              \
  X(MN_PLAIN, MN_PLAIN, false)  /* wgrad */
#define NR_MODE_HIT(A_, B_, TR_) if (am == A_ && bm == B_ && tr == TR_) return true;
inline bool fast_modes(int am, int bm, bool tr) {
  NR_MODES_KC(NR_MODE_HIT) NR_MODES_MN(NR_MODE_HIT) return false;
}
inline bool big_modes(int am, int bm, bool tr) { NR_MODES_BIG(NR_MODE_HIT) return false; }
#undef NR_MODE_HIT

enum GemmFamily {
  GEMM_NOT_ELIGIBLE,   // GemmRoute::einval says which NR_EINVAL the entry returns
  GEMM_GENERIC,        // gemm_f32_kernel, bm x bn of 64 / 128 (static form only)
  GEMM_F32_64,         // gemm_fast_kernel<64, 64>
  GEMM_F32_128,        // gemm_fast_kernel<128, 128>
  GEMM_SPLIT_128,      // gemm_split_kernel (128 x 128, bf16 planes)
  GEMM_BIG             // gemm_big_kernel (256 x bn, bf16 planes)
};

// What routing looks at.  `dyn`: the dynamic form (nr_gemm_f32_dyn / _dyn_cus, nr_gemm_f32_ws with
// m_dev, k_dev or max_cus); the operands' data pointers count by their alignment only.
struct GemmProblem {
  int64_t M, N, K;
  const nr_operand *A, *B, *c_rows;
  int32_t epilogue, split_k, prec;   // split_k >= 1
  bool dyn, m_dyn;                   // m_dyn: M is device-resident (m_dev)
  int32_t max_cus;
  const float* work;                 // workspace (null: none), its elements, and whether the
  int64_t work_elems;                // caller wants the bias-gradient column sums
  bool colsum;
};

struct GemmRoute {
  int family = GEMM_NOT_ELIGIBLE;
  int einval = 7;
  int bm = 0, bn = 0;       // tile
  int planes = 0;           // bf16 planes per operand: 3 = bf16x6, 1 = bf16, 0 = exact f32
  int am = 0, bmode = 0;    // operand modes
  bool tr = false;          // transposed accumulators (else C-major)
  int epi = 0;              // the epilogue the kernel runs
  int splits = 1;           // K splits and their length, after any re-split
  int64_t kchunk = 32;
  bool slab = false;        // split-K partial tiles through the workspace + splitk_reduce_kernel
  bool fold = false;        // ... with the bias-gradient column sums folded in
  int tail = 0;             // stream-K tail: max K pieces of the last partial round's tiles (0 = off)
  bool tail_ws = false;     // ... through the workspace + tail_reduce_kernel (else atomics),
  int tail_cap = 0;         // which holds this many partial tiles
};

// The two rules the host and the kernels must read alike (the kernels and the reduce kernels re-derive
// them from device-resident extents): callable from both under hipcc, plain functions under g++.
#ifdef __HIPCC__
#define NR_HD __host__ __device__
#else
#define NR_HD
#endif

// Length of one split of K cut `splits` ways: whole 32-deep k-tiles, never 0.
NR_HD inline int64_t k_chunk(int64_t K, int64_t splits) {
  const int64_t kc = (K + splits - 1) / splits;
  return kc > 0 ? (kc + 31) / 32 * 32 : 32;
}
// Splits of length kchunk that hold some of K (a split that starts at or past K is empty).
NR_HD inline int64_t k_chunks(int64_t K, int64_t kchunk) { return (K + kchunk - 1) / kchunk; }
// A device-resident extent under its host bound: [0, bound].
NR_HD inline int64_t clamp_extent(int64_t bound, int64_t dev_value) {
  return dev_value < bound ? (dev_value > 0 ? dev_value : 0) : bound;
}

// K split `want` ways in 32-deep k-tiles: the chunk per split and the splits that are not empty.
struct KSplit {
  int64_t kchunk;
  int splits;
};
inline KSplit k_split(int64_t K, int64_t want) {
  const int64_t kc = k_chunk(K, want);
  const int s = (int)k_chunks(K, kc);
  return {kc, s > 0 ? s : 1};
}

inline int operand_mode(const nr_operand* o) {
  const int m = o->map == NR_ROWS_PLAIN ? 0 : o->map == NR_ROWS_GATHER ? 1 : 2;
  return (o->layout == NR_KCONTIG ? KC_PLAIN : MN_PLAIN) + m;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Floats before the big kernel's tail partial tiles in its NR_EPI_SCATTER_ZEROED workspace (ints
// {full, rem, pieces, gn} of the launch's stream-K tail, padded to 256 B; gemm_big_impl.h tail_slab_tr)
constexpr int TAIL_WS_HDR = 64;

// Large-tile (256 x BN) bf16 kernel choice: 0 = stay on the 128x128 kernel; 256 x 256 tiles unless
// their units fill the 256 CUs clearly worse ("round efficiency" = units / (256 * rounds), times the useful fraction
// of padded columns) than the 128x128 kernel's at two workgroups per CU.
// Split-K callers (atomic epilogues) are re-split for the chosen tile, so they always fill the chip.
inline double round_eff(int64_t units, int64_t slots) {
  if (units <= 0) return 0.0;
  const int64_t rounds = (units + slots - 1) / slots;
  return (double)units / (double)(rounds * slots);
}

inline int big_bn(int64_t M, int64_t N, int64_t K, int splits, bool resplit, bool m_dyn, int kmin) {
  if (N < 128) return 0;
  // a short contraction (K < kmin) does not amortise the per-unit pipeline fill
  if (!resplit && K < kmin) return 0;
  const int64_t gm = (M + 255) / 256;
  if (!resplit && gm * splits < 8) return 0;
  if (resplit) return (N % 256 == 0 || N >= 1024) ? 256 : 128;
  // padded-N MFMA work counts against a tile width too; measured on the step's shapes, the
  // 256 x 256 core is ~15 % faster per unit of work than the 128 x 128 kernel, 256 x 128 is not
  const double e256 = round_eff(gm * ((N + 255) / 256) * splits, 256) * (double)N / (double)((N + 255) / 256 * 256);
  const double e_old = round_eff(((M + 127) / 128) * ((N + 127) / 128) * splits, 512) * (double)N /
                       (double)((N + 127) / 128 * 128);
  // device-resident M (distinct-row counts): the host M is only a bound and the persistent grid
  // absorbs the actual count -- the big tiles for wide N, else the round efficiencies at the bound
  // (the CNN tap projection, N = 480: 141 -> see DESIGN §4.1)
  if (m_dyn) return (N >= 1024 || e256 >= 0.87 * e_old) ? 256 : 0;
  return e256 >= 0.87 * e_old ? 256 : 0;
}

inline int pick_tile(int64_t n) {  // 64 or 128: least padding, ties -> 128
  const int64_t p64 = (n + 63) / 64 * 64, p128 = (n + 127) / 128 * 128;
  return p128 <= p64 ? 128 : 64;
}

// The fast kernels' route at t x t tiles (t = 64: exact f32 only), or false when the operands are
// not eligible for them: data 16-B aligned, ld % 4 == 0, K a positive multiple of 32, MN-contiguous
// operands with ld >= round4(M or N) (reads stay inside padded rows), conv3 seg % 32 == 0 and
// seg % t == 0 where the taps run along N, and an instantiated mode combination.
inline bool fast_route(const GemmProblem& p, int t, int cus, GemmRoute& r) {
  const nr_operand *A = p.A, *B = p.B, *cr = p.c_rows;
  const int64_t M = p.M, N = p.N, K = p.K;
  auto aligned = [](const nr_operand* o) { return o->ld % 4 == 0 && aligned16(o->data); };
  if (K <= 0 || K % 32 || !aligned(A) || !aligned(B)) return false;
  const int am = operand_mode(A), bmode = operand_mode(B);
  if (am == KC_CONV3 && A->seg % 32) return false;
  if (am == MN_GATHER || am == MN_CONV3 || (am == MN_PLAIN && A->ld < ((M + 3) & ~3LL))) return false;
  if (bmode == KC_GATHER || bmode == KC_CONV3) return false;
  if ((bmode == MN_PLAIN || bmode == MN_GATHER) && B->ld < ((N + 3) & ~3LL)) return false;
  if (bmode == MN_CONV3 && (B->seg % t || B->seg % 4)) return false;
  // NR_EPI_SCATTER_ZEROED = NR_EPI_SCATTER_STORE whose destination rows are zero on entry: the big
  // kernel may then split the K of its last partial round of tiles (atomic adds of the pieces)
  const bool zeroed = p.epilogue == NR_EPI_SCATTER_ZEROED;
  const int epi = zeroed ? NR_EPI_SCATTER_STORE : p.epilogue;
  if (epi == NR_EPI_SCATTER && cr && (cr->map == NR_ROWS_PLAIN || (cr->map == NR_ROWS_CONV3 && cr->seq_len == 1)))
    return false;
  if (epi == NR_EPI_SCATTER_STORE && (!cr || cr->map != NR_ROWS_GATHER || !cr->rows)) return false;
  const bool atomic_epi = epi == NR_EPI_ATOMIC || epi == NR_EPI_SCATTER;
  const KSplit ks = k_split(K, p.split_k);
  r = GemmRoute();
  r.bm = r.bn = t;
  r.am = am; r.bmode = bmode; r.tr = !atomic_epi; r.epi = epi;
  r.splits = ks.splits; r.kchunk = ks.kchunk;
  if (t == 128 && p.prec != NR_GEMM_F32) {
    r.planes = p.prec == NR_GEMM_BF16 ? 1 : 3;
    const bool resplit = p.split_k > 1 && atomic_epi;
    // shortest contraction the big kernel takes: 512 (32 k-tiles of MFMAs per unit fill), in bf16 too
    // (A/B: the CNN table dgrad, K = 480, ran 94 us on the 128x128 kernel and 114 us on the big one)
    // (re-measured in round 4 on the k-contiguous CNN dgrad, bf16: 59 us here, 95 us with kmin = 480,
    // profiles/r04_h_gemm_ab.json)
    const int kmin = 512;
    // the stream-K tail through the workspace (bf16x6, below) makes the big kernel pay for contractions
    // down to 256 too: the CNN table dgrad (K = 480) left the 128 x 128 kernel with it
    const bool ws_tail = zeroed && p.prec == NR_GEMM_BF16X6 && p.work != nullptr;
    const bool tailed = zeroed && ks.splits == 1 && K >= (ws_tail ? 256 : kmin) && N >= 256;
    // bf16 split-K (atomic) launches take the big kernel too: its fewer, larger units halve the operand
    // re-reads and keep three k-tiles of loads in flight (CNN conv weight gradient 200 -> 138 us)
    // (the bf16x6 big kernel runs its k-loop two 16-deep k-tiles per iteration with no branch: every
    // unit's k range is a multiple of 32, as k chunks are and eligibility makes K)
    const int BN = tailed ? 256 : big_bn(M, N, K, ks.splits, resplit, p.m_dyn, kmin);
    if (BN && big_modes(am, bmode, r.tr)) {
      r.family = GEMM_BIG;
      r.bm = 256; r.bn = BN;
      r.tail = tailed ? 16 : 0;
      if (resplit) {
        // re-split for 256 x BN tiles: one wave of units over the CUs it may use (all 256 of the
        // MI355X unless the caller caps them), >= 512 k per split
        const int64_t tiles = ((M + 255) / 256) * ((N + BN - 1) / BN);
        int64_t want = (p.max_cus > 0 ? p.max_cus : 256) / (tiles > 0 ? tiles : 1);
        if (want > K / 512) want = K / 512;
        if (want > 64) want = 64;
        if (want < 1) want = 1;
        const KSplit rs = k_split(K, want);
        r.splits = rs.splits; r.kchunk = rs.kchunk;
      }
      // split-K partial tiles through a workspace (plain stores + one reduction launch) when the caller
      // gave one: a round of 256 fp32 atomic tiles costs ~50 us at the chip's ~1.3 TB/s atomic rate
      const int64_t sld = (N + 3) & ~int64_t(3);
      r.slab = epi == NR_EPI_ATOMIC && r.splits > 1 && p.work && aligned16(p.work) &&
               p.work_elems >= (int64_t)r.splits * M * sld + (p.colsum ? (int64_t)r.splits * M : 0);
      r.fold = r.slab && p.colsum && am == MN_PLAIN;
      // the stream-K tail's pieces through the workspace too (tail_slab_tr / tail_reduce_kernel): one
      // 256 x 256 partial tile per tail unit; the kernel's plan keeps the pieces within the tiles the
      // workspace holds (Args::tail_cap), so a grid of more than one workgroup per CU cannot overrun it
      // (bf16x6: one 147 KB workgroup per CU; the bf16 kernel keeps the atomic tail)
      const int64_t cap_tiles = p.work_elems > TAIL_WS_HDR ? (p.work_elems - TAIL_WS_HDR) / 65536 : 0;
      r.tail_ws = tailed && ws_tail && cus > 0 && cap_tiles >= cus && aligned16(p.work);
      if (r.tail_ws) r.tail_cap = (int)(cap_tiles < 0x7fffffff ? cap_tiles : 0x7fffffff);
      return true;
    }
    // the split kernel's conv wgrad needs whole 128-column tap tiles (t == 128 here: seg % t above)
    if (fast_modes(am, bmode, r.tr)) { r.family = GEMM_SPLIT_128; return true; }
    return false;
  }
  r.family = t == 128 ? GEMM_F32_128 : GEMM_F32_64;
  return fast_modes(am, bmode, r.tr);
}

// What runs for a validated call with M, N > 0 (and K > 0 in the dynamic form).
inline GemmRoute gemm_route(const GemmProblem& p, int cus) {
  GemmRoute r;
  const KSplit ks = k_split(p.K, p.split_k);
  // dynamic form: 128 x 128 tiles and up, fast kernels only.  Static form: bf16x6 and f32 take 64x64
  // tiles for small problems (< 400 tiles of 128x128), which only the exact-f32 kernel has (they are
  // latency-bound, and 128x128 tiles would leave most CUs idle); larger ones take 128x128 tiles
  // (bf16x6: the split kernels; f32: the exact-f32 128x128 kernel).  bf16: every eligible shape runs
  // on the bf16 kernel (one product per tile is cheap).
  const int64_t t128 = ((p.M + 127) / 128) * ((p.N + 127) / 128) * ks.splits;
  const int64_t small_min = 400;
  const int t = (p.dyn || p.prec == NR_GEMM_BF16 || t128 >= small_min) ? 128 : 64;
  if (fast_route(p, t, cus, r)) return r;
  r = GemmRoute();
  if (p.dyn) return r;   // einval 7: not eligible for the fast kernels
  // generic kernel: any alignment.  NR_EPI_SCATTER_STORE stores (split_k > 1 is refused for it, so one
  // workgroup produces each element); NR_EPI_SCATTER_ZEROED, whose rows are zero on entry, runs as the
  // same sums via NR_EPI_SCATTER's atomics
  const nr_operand *A = p.A, *B = p.B;
  r.epi = p.epilogue == NR_EPI_SCATTER_ZEROED ? (int)NR_EPI_SCATTER : p.epilogue;
  r.am = operand_mode(A); r.bmode = operand_mode(B);
  r.splits = ks.splits; r.kchunk = ks.kchunk;
  int bm = pick_tile(p.M), bn = pick_tile(p.N);
  // small problems: prefer 64x64 tiles to fill the 256 CUs
  if ((int64_t)((p.M + bm - 1) / bm) * ((p.N + bn - 1) / bn) * ks.splits < 512) { bm = 64; bn = 64; }
  // CONV3 operands need a tap-uniform tile: seg must be a multiple of the tile extent
  // along the axis that carries the taps (k for K-contiguous, m/n otherwise)
  const bool ak = A->layout == NR_KCONTIG, bk = B->layout == NR_KCONTIG;
  r.einval = 6;
  if (A->map == NR_ROWS_CONV3 && ak && (A->seg % 32)) return r;
  if (B->map == NR_ROWS_CONV3 && bk && (B->seg % 32)) return r;
  if (A->map == NR_ROWS_CONV3 && !ak && (A->seg % bm)) bm = 64;
  if (B->map == NR_ROWS_CONV3 && !bk && (B->seg % bn)) bn = 64;
  r.einval = 7;
  if ((A->map == NR_ROWS_CONV3 && !ak && (A->seg % bm)) || (B->map == NR_ROWS_CONV3 && !bk && (B->seg % bn)))
    return r;
  r.family = GEMM_GENERIC;
  r.bm = bm; r.bn = bn;
  return r;
}

// ---- two independent problems in one launch (nr_gemm_f32_pair)

// Where a problem's result goes (not part of routing: GemmProblem has no output).
struct GemmOut {
  const float* C;
  int64_t ldc;
  const float* bias;
};

// Bytes [lo, hi) of a stored matrix of `rows` x `cols` floats, rows `ld` apart (empty: lo == hi == 0).
struct ByteSpan {
  uintptr_t lo, hi;
};
inline ByteSpan span_of(const float* p, int64_t rows, int64_t ld, int64_t cols) {
  if (!p || rows <= 0 || cols <= 0) return {0, 0};
  const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
  return {lo, lo + (uintptr_t)(((rows - 1) * ld + cols) * (int64_t)sizeof(float))};
}
inline bool spans_overlap(ByteSpan a, ByteSpan b) { return a.lo < b.hi && b.lo < a.hi; }

// The stored bytes an operand reads: a plain one's [extent x K] (K-contiguous) or [K x extent]
// (MN-contiguous) matrix; a gathered / conv3 one's table has no height known here -- its first row.
inline ByteSpan operand_span(const nr_operand* o, int64_t extent, int64_t K) {
  if (!o) return {0, 0};
  const bool kc = o->layout == NR_KCONTIG;
  const int64_t rows = o->map != NR_ROWS_PLAIN ? 1 : (kc ? extent : K);
  return span_of(o->data, rows, o->ld, kc ? K : extent);
}

// Does either problem's output ([M x N] at C, rows ldc apart) overlap what the other problem reads
// (A, B, the auxiliary matrix of the gate / GELU epilogues, bias) or writes?  Such problems are not
// independent: nr_gemm_f32_pair refuses them.
inline bool gemm_pair_alias(const GemmProblem& p1, const GemmOut& o1, const GemmProblem& p2, const GemmOut& o2) {
  const ByteSpan c1 = span_of(o1.C, p1.M, o1.ldc, p1.N), c2 = span_of(o2.C, p2.M, o2.ldc, p2.N);
  if (spans_overlap(c1, c2)) return true;
  auto reads = [](const GemmProblem& p, const GemmOut& o, ByteSpan c) {
    const bool aux = p.c_rows && p.c_rows->data && p.c_rows->map == NR_ROWS_PLAIN;
    return spans_overlap(c, operand_span(p.A, p.M, p.K)) || spans_overlap(c, operand_span(p.B, p.N, p.K)) ||
           spans_overlap(c, span_of(o.bias, 1, p.N, p.N)) ||
           (aux && spans_overlap(c, span_of(p.c_rows->data, p.M, p.c_rows->ld, p.N)));
  };
  return reads(p2, o2, c1) || reads(p1, o1, c2);
}

// The pairs gemm_fast64.hip instantiates, as (first, second): an input gradient dx = dY W (K-contiguous
// x MN-contiguous, transposed accumulators) beside a weight gradient dW += dYᵀ x (MN x MN, C-major).
inline bool pair_modes(const GemmRoute& a, const GemmRoute& b) {
  return a.am == KC_PLAIN && a.bmode == MN_PLAIN && a.tr && b.am == MN_PLAIN && b.bmode == MN_PLAIN && !b.tr;
}

// Can two validated, routed problems share one launch?  0: no (they run one after the other); 1: yes, as
// (p1, p2); 2: yes, as (p2, p1).  Both on the exact-f32 64 x 64 kernel in an instantiated mode pair,
// static form (no device extents), no CU cap, outputs that alias nothing of the other problem.
inline int gemm_pair_order(const GemmProblem& p1, const GemmRoute& r1, const GemmOut& o1, const GemmProblem& p2,
                           const GemmRoute& r2, const GemmOut& o2) {
  if (r1.family != GEMM_F32_64 || r2.family != GEMM_F32_64) return 0;
  if (p1.dyn || p2.dyn || p1.max_cus != 0 || p2.max_cus != 0) return 0;
  if (gemm_pair_alias(p1, o1, p2, o2)) return 0;
  if (pair_modes(r1, r2)) return 1;
  if (pair_modes(r2, r1)) return 2;
  return 0;
}


// Workgroups of the pair launch for problems of ua and ub units on `slots` resident workgroups: each
// problem its units when both fit, else the slots shared in proportion to the units (at least one
// each); a's share is a multiple of 8 where it can be, so that no slot goes to an idle workgroup.
inline void pair_grids(int64_t ua, int64_t ub, int slots, int& ga, int& off, int& gb) {
  const int64_t pad = (ua + 7) / 8 * 8;
  if (slots <= 0 || pad + ub <= slots) {
    ga = (int)ua; off = (int)pad; gb = (int)ub;
    return;
  }
  int64_t sb = slots * ub / (ua + ub);
  if (sb < 1) sb = 1;
  if (sb > ub) sb = ub;
  int64_t sa = slots - sb;
  if (sa > ua) sa = ua;
  if (sa >= 8 && sa < ua) sa &= ~int64_t(7);
  if (sa < 1) sa = 1;
  ga = (int)sa; off = (int)((sa + 7) / 8 * 8); gb = (int)sb;
}

}  // namespace nrfast
