// Prints the GEMM route (csrc/gemm_route.h) of a table of problems on a 256-CU device, one line per
// problem.  Stand-alone and HIP-free: tests/test_gemm_route_cpu.py builds it with g++ (address and
// undefined-behaviour sanitizers on), runs it and compares the lines with the recorded table.
// With arguments it prints the route of the one problem they describe (dump_argv below):
// tests/test_gemm_epi_ref_cpu.py and tests/test_gemm_map_ref_cpu.py pin the kernels of the epilogue
// and row-map tests' case tables that way.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../news-recommendation-mind_amd/csrc/gemm_route.h"

using namespace nrfast;

namespace {

const float* const DATA = reinterpret_cast<const float*>(0x10000);      // 16-B aligned, never read
const float* const WORK = reinterpret_cast<const float*>(0x20000);
const int64_t* const ROWS = reinterpret_cast<const int64_t*>(0x30000);
const int64_t WORK_ELEMS = 256LL * 256 * 261;   // nr_gemm_splitk_workspace() at 256 CUs

enum { KC = NR_KCONTIG, MN = NR_MNCONTIG };
enum { PLAIN = NR_ROWS_PLAIN, GATHER = NR_ROWS_GATHER, CONV3 = NR_ROWS_CONV3 };
enum { STATIC = 0, DYN = 1, MDEV = 2 };   // form: static, dynamic, dynamic with a device-resident M

struct Side {
  int layout, map;
  int64_t ld;
  int seg;
  int misalign;   // bytes added to the data pointer
};

struct Row {
  const char* name;
  int64_t M, N, K;
  Side A, B;
  int epi, split_k, form, max_cus;
  int work;   // workspace: 0 none, 1 nr_gemm_splitk_workspace(), 2 too small for a round of tail tiles
  bool colsum;
  int cmap = GATHER, cseg = 1;   // the scatter epilogues' destination row map
  int seq = 30;                  // tokens per title of every CONV3 map
};

nr_operand operand(const Side& s, int seq) {
  nr_operand o;
  o.data = reinterpret_cast<const float*>(reinterpret_cast<const char*>(DATA) + s.misalign);
  o.ld = s.ld;
  o.rows = s.map == PLAIN ? nullptr : ROWS;
  o.map = s.map;
  o.seq_len = s.map == CONV3 ? seq : 1;
  o.seg = s.seg;
  o.layout = s.layout;
  return o;
}

const char* family_name(int f) {
  static const char* const names[] = {"not_eligible", "generic", "f32_64", "f32_128", "split_128", "big"};
  return names[f];
}

void dump(const Row& w, int prec, const char* prec_name) {
  const nr_operand a = operand(w.A, w.seq), b = operand(w.B, w.seq);
  // c_rows: the destination row map of the scatter epilogues, the aux matrix of the GELU ones
  const nr_operand rows = operand(Side{KC, w.cmap, w.N, w.cseg, 0}, w.seq), aux = operand(Side{KC, PLAIN, w.N, 1, 0}, w.seq);
  const bool scatter = w.epi == NR_EPI_SCATTER || w.epi == NR_EPI_SCATTER_STORE || w.epi == NR_EPI_SCATTER_ZEROED;
  const bool gelu = w.epi == NR_EPI_STORE_GELU || w.epi == NR_EPI_GELU_GRAD;
  GemmProblem p{w.M, w.N, w.K, &a, &b, scatter ? &rows : gelu ? &aux : nullptr, w.epi, w.split_k, prec, w.form != STATIC,
                w.form == MDEV, w.max_cus, w.work ? WORK : nullptr,
                w.work == 1 ? WORK_ELEMS : w.work == 2 ? 100 * 65536 : 0, w.colsum};
  const GemmRoute r = gemm_route(p, 256);
  printf("%s %s: %s", w.name, prec_name, family_name(r.family));
  if (r.family == GEMM_NOT_ELIGIBLE) {
    printf(" einval=%d\n", r.einval);
    return;
  }
  printf(" tile=%dx%d planes=%d modes=%d,%d tr=%d epi=%d splits=%d kchunk=%lld slab=%d fold=%d tail=%d tail_ws=%d "
         "tail_cap=%d\n", r.bm, r.bn, r.planes, r.am, r.bmode, (int)r.tr, r.epi, r.splits, (long long)r.kchunk,
         (int)r.slab, (int)r.fold, r.tail, (int)r.tail_ws, r.tail_cap);
}

// operands: K-contiguous [rows][k] (ld = the row length), MN-contiguous [k][rows]
Side kc(int64_t ld, int map = PLAIN, int seg = 1) { return Side{KC, map, ld, seg, 0}; }
Side mn(int64_t ld, int map = PLAIN, int seg = 1) { return Side{MN, map, ld, seg, 0}; }

const int E = 768, U = 24576, T = 20832;   // tools/gemm_ab.py: table width, distinct-row bound, BERT tokens
const int STORE = NR_EPI_STORE, ATOMIC = NR_EPI_ATOMIC, ZEROED = NR_EPI_SCATTER_ZEROED;

// the split_k the step passes for a weight gradient (functions._split_k)
int split_k(int64_t m, int64_t n, int64_t k) {
  const int64_t tiles = ((m + 127) / 128) * ((n + 127) / 128);
  int64_t s = 512 / (tiles > 0 ? tiles : 1);
  if (s > k / 512) s = k / 512;
  if (s > 64) s = 64;
  return (int)(s < 1 ? 1 : s);
}

const Row ROWS_TABLE[] = {
    // ---- the step's shapes (tools/gemm_ab.py), each in bf16x6 and bf16
    {"nrms_proj_fwd", 23872, 1152, E, kc(E, GATHER), kc(E), STORE, 1, MDEV, 0, 0, false},   // the traced anchor
    {"nrms_proj_fwd_bound", U, 1152, E, kc(E, GATHER), kc(E), STORE, 1, DYN, 0, 0, false},
    {"nrms_proj_dgrad", U, E, 1152, kc(1152), mn(E), STORE, 1, DYN, 0, 0, false},
    {"nrms_dgrad_table", 52800, E, 1152, kc(1152), mn(E), ZEROED, 1, MDEV, 0, 0, false},
    {"nrms_dgrad_table_ws", 52800, E, 1152, kc(1152), mn(E), ZEROED, 1, MDEV, 0, 1, false},
    {"nrms_dgrad_table_kc_ws", 52800, E, 1152, kc(1152), kc(1152), ZEROED, 1, MDEV, 0, 1, false},
    {"nrms_dgrad_table_store", 52800, E, 1152, kc(1152), mn(E), NR_EPI_SCATTER_STORE, 1, MDEV, 0, 0, false},
    {"nrms_proj_wgrad", 1152, E, U, mn(1152), mn(E, GATHER), ATOMIC, split_k(1152, E, U), DYN, 0, 0, false},
    {"nrms_proj_wgrad_ws", 1152, E, U, mn(1152), mn(E, GATHER), ATOMIC, split_k(1152, E, U), DYN, 0, 1, false},
    {"nrms_proj_wgrad_cus", 1152, E, U, mn(1152), mn(E, GATHER), ATOMIC, split_k(1152, E, U), DYN, 192, 0, false},
    {"bert_qkv", T, 2304, E, kc(E), kc(E), STORE, 1, STATIC, 0, 0, false},
    {"bert_ffn1_gelu", T, 3072, E, kc(E), kc(E), NR_EPI_STORE_GELU, 1, STATIC, 0, 0, false},
    {"bert_ffn2", T, E, 3072, kc(3072), kc(3072), STORE, 1, STATIC, 0, 0, false},
    {"bert_ffn2_dgrad", T, 3072, E, kc(E), mn(3072), STORE, 1, STATIC, 0, 0, false},
    {"bert_qkv_dgrad", T, E, 2304, kc(2304), mn(E), STORE, 1, STATIC, 0, 0, false},
    {"bert_ffn1_wgrad", 3072, E, T, mn(3072), mn(E), ATOMIC, split_k(3072, E, T), STATIC, 0, 0, false},
    {"bert_ffn1_wgrad_cs", 3072, E, T, mn(3072), mn(E), ATOMIC, split_k(3072, E, T), STATIC, 0, 1, true},
    {"bert_ffn2_wgrad_cs", E, 3072, T, mn(E), mn(3072), ATOMIC, split_k(E, 3072, T), STATIC, 0, 1, true},
    {"bert_qkv_wgrad_cs", 2304, E, T, mn(2304), mn(E), ATOMIC, split_k(2304, E, T), STATIC, 0, 1, true},
    {"cnn_tap_proj", U, 480, E, kc(E, GATHER), kc(E), STORE, 1, DYN, 0, 0, false},
    {"cnn_tap_proj_mdev", U, 480, E, kc(E, GATHER), kc(E), STORE, 1, MDEV, 0, 0, false},
    {"cnn_table_dgrad", U, E, 480, kc(480), mn(E), ZEROED, 1, MDEV, 0, 0, false},
    {"cnn_table_dgrad_kc", U, E, 480, kc(480), kc(480), ZEROED, 1, MDEV, 0, 0, false},
    {"cnn_table_dgrad_ws", U, E, 480, kc(480), mn(E), ZEROED, 1, MDEV, 0, 1, false},
    {"cnn_conv_wgrad", 480, E, U, mn(480), mn(E, GATHER), ATOMIC, split_k(480, E, U), DYN, 0, 0, false},
    {"cnn_conv_wgrad_ws", 480, E, U, mn(480), mn(E, GATHER), ATOMIC, split_k(480, E, U), DYN, 0, 1, false},
    {"user_fwd", 1600, E, 384, kc(384), kc(384), STORE, 1, STATIC, 0, 0, false},
    {"user_wgrad_cs", E, 384, 1600, mn(E), mn(384), ATOMIC, split_k(E, 384, 1600), STATIC, 0, 1, true},
    // ---- the shapes the GEMM GPU tests name: N = 1152 / 520 / 768 / 1100 / 1200, K = 480 / 544 / 992
    {"test_split_plain_kk", 1000, 520, 768, kc(768), kc(768), STORE, 1, DYN, 0, 0, false},
    {"test_split_plain_km", 1000, 520, 768, kc(768), mn(520), STORE, 1, DYN, 0, 0, false},
    {"test_split_plain_mm", 1000, 520, 768, mn(1000), mn(520), ATOMIC, 3, DYN, 0, 0, false},
    {"test_split_plain_static", 1000, 520, 768, kc(768), kc(768), STORE, 1, STATIC, 0, 0, false},
    {"test_gather_n1152", 2016, 1152, 768, kc(768, GATHER), kc(768), STORE, 1, DYN, 0, 0, false},
    {"test_big_n1100", 4000, 1100, 768, kc(768, GATHER), kc(768), STORE, 1, DYN, 0, 0, false},
    {"test_big_n1100_mdev", 4000, 1100, 768, kc(768, GATHER), kc(768), STORE, 1, MDEV, 0, 0, false},
    {"test_big_n1200", 4000, 1200, 768, kc(768, GATHER), kc(768), STORE, 1, DYN, 0, 0, false},
    {"test_big_n768_mdev", 4000, 768, 1152, kc(1152), mn(768), ZEROED, 1, MDEV, 0, 0, false},
    {"test_k480", 4000, 768, 480, kc(480), mn(768), ZEROED, 1, MDEV, 0, 0, false},
    {"test_k544", 4000, 768, 544, kc(544), mn(768), ZEROED, 1, MDEV, 0, 0, false},
    {"test_k544_ws", 4000, 768, 544, kc(544), mn(768), ZEROED, 1, MDEV, 0, 1, false},
    {"test_k992_wgrad", 1152, 768, 992, mn(1152), mn(768, GATHER), ATOMIC, 9, DYN, 0, 0, false},
    {"test_k992_wgrad_ws", 1152, 768, 992, mn(1152), mn(768, GATHER), ATOMIC, 9, DYN, 0, 1, false},
    // ---- the other families and the workspace decisions
    {"small_static", 200, 136, 96, kc(96), kc(96), STORE, 1, STATIC, 0, 0, false},          // < 400 tiles: 64x64
    {"small_dyn", 200, 136, 96, kc(96), kc(96), STORE, 1, MDEV, 0, 0, false},
    {"unaligned_static", 3000, 1152, 768, Side{KC, PLAIN, 768, 1, 4}, kc(768), STORE, 1, STATIC, 0, 0, false},
    {"unaligned_dyn", 3000, 1152, 768, Side{KC, PLAIN, 768, 1, 4}, kc(768), STORE, 1, DYN, 0, 0, false},
    {"odd_ld_static", 300, 200, 70, kc(70), kc(70), STORE, 1, STATIC, 0, 0, false},
    {"k_zero_static", 64, 64, 0, kc(32), kc(32), STORE, 1, STATIC, 0, 0, false},
    {"conv3_fwd", 24000, 400, 2304, kc(E, CONV3, E), kc(2304), NR_EPI_STORE_RELU, 1, STATIC, 0, 0, false},
    {"conv3_wgrad", 512, 2304, 24000, mn(512), mn(E, CONV3, E), ATOMIC, 8, STATIC, 0, 0, false},
    {"conv3_wgrad_seg_96", 512, 288, 24000, mn(512), mn(96, CONV3, 96), ATOMIC, 8, STATIC, 0, 0, false},
    {"conv3_kc_seg_20", 64, 64, 96, kc(32, CONV3, 20), kc(96), STORE, 1, STATIC, 0, 0, false},
    {"conv3_mn_seg_20", 64, 64, 96, mn(64, CONV3, 20), kc(96), STORE, 1, STATIC, 0, 0, false},
    {"zeroed_small_ws", 52800, E, 1152, kc(1152), mn(E), ZEROED, 1, MDEV, 0, 2, false},
    {"splitk_small_ws", 1152, E, U, mn(1152), mn(E), ATOMIC, 10, STATIC, 0, 2, false},
    {"splitk_atomic", 1152, E, U, mn(1152), mn(E), ATOMIC, 10, STATIC, 0, 0, false},
    {"splitk_slab", 1152, E, U, mn(1152), mn(E), ATOMIC, 10, STATIC, 0, 1, false},
    {"splitk_slab_fold", 1152, E, U, mn(1152), mn(E), ATOMIC, 10, STATIC, 0, 1, true},
    {"splitk_slab_gather_colsum", 1152, E, U, mn(1152), mn(E, GATHER), ATOMIC, 10, DYN, 0, 1, true},
    {"splitk_scatter", 8000, E, 2304, kc(2304), mn(E), NR_EPI_SCATTER, 4, STATIC, 0, 0, false},
};

// Argument mode: the route of one problem,
//   NAME M N K A_LAYOUT A_LD B_LAYOUT B_LD EPILOGUE FORM PREC [KEY=VALUE ...]
// with layouts kc | mn, the epilogue's number (enum nr_epilogue), FORM static | dyn | mdev and PREC
// f32 | bf16x6 | bf16; one line in the table's format.  Without KEY=VALUE tokens the operands are plain,
// split_k is 1 and there is no workspace.  The keys: amap / bmap = plain | gather | conv3 (the operands'
// row maps) with aseg / bseg (CONV3: columns per tap); cmap = gather | conv3 with cseg (the scatter
// epilogues' destination map); seq (tokens per title of every CONV3 map, default 30); split (split_k);
// work = 0 | 1 (nr_gemm_splitk_workspace() floats of workspace); cus (max_cus of the dynamic forms).
// Anything else: usage on stderr, exit 2.
int pick(const char* s, const char* const* names, int n) {
  for (int i = 0; i < n; ++i)
    if (!strcmp(s, names[i])) return i;
  return -1;
}

bool number(const char* s, int64_t lo, int64_t hi, int64_t& v) {
  char* end = nullptr;
  const long long x = strtoll(s, &end, 10);
  if (end == s || *end || x < lo || x > hi) return false;
  v = x;
  return true;
}

// KEY=VALUE tokens of the argument mode into the row; false for an unknown key or a bad value
bool key_values(char** kv, int n, Row& w) {
  static const char* const maps[] = {"plain", "gather", "conv3"};   // enum nr_rows_map follows this order
  for (int i = 0; i < n; ++i) {
    const char* eq = strchr(kv[i], '=');
    if (!eq || eq == kv[i]) return false;
    const size_t kl = (size_t)(eq - kv[i]);
    const char* val = eq + 1;
    auto is = [&](const char* k) { return strlen(k) == kl && !strncmp(kv[i], k, kl); };
    int64_t v = 0;
    const int m = pick(val, maps, 3);
    if (is("amap") && m >= 0) w.A.map = m;
    else if (is("bmap") && m >= 0) w.B.map = m;
    else if (is("cmap") && m >= 1) w.cmap = m;
    else if (is("aseg") && number(val, 1, 1 << 30, v)) w.A.seg = (int)v;
    else if (is("bseg") && number(val, 1, 1 << 30, v)) w.B.seg = (int)v;
    else if (is("cseg") && number(val, 1, 1 << 30, v)) w.cseg = (int)v;
    else if (is("seq") && number(val, 1, 1 << 30, v)) w.seq = (int)v;
    else if (is("split") && number(val, 1, 1 << 30, v)) w.split_k = (int)v;
    else if (is("work") && number(val, 0, 1, v)) w.work = (int)v;
    else if (is("cus") && number(val, 0, 1 << 20, v)) w.max_cus = (int)v;
    else return false;
  }
  return true;
}

int dump_argv(char** a, int extra) {
  static const char* const layouts[] = {"kc", "mn"};
  static const char* const forms[] = {"static", "dyn", "mdev"};
  static const char* const precs[] = {"f32", "bf16x6", "bf16"};
  int64_t M, N, K, lda, ldb, epi;
  const int la = pick(a[4], layouts, 2), lb = pick(a[6], layouts, 2), form = pick(a[9], forms, 3);
  const int prec = pick(a[10], precs, 3);
  const int64_t big = int64_t(1) << 40;
  if (!number(a[1], 1, big, M) || !number(a[2], 1, big, N) || !number(a[3], 0, big, K) || la < 0 ||
      !number(a[5], 1, big, lda) || lb < 0 || !number(a[7], 1, big, ldb) ||
      !number(a[8], NR_EPI_STORE, NR_EPI_SCATTER_ZEROED, epi) || form < 0 || prec < 0)
    return 2;
  Row w{a[0], M, N, K, Side{la, PLAIN, lda, 1, 0}, Side{lb, PLAIN, ldb, 1, 0}, (int)epi, 1, form, 0, 0, false};
  if (!key_values(a + 11, extra, w)) return 2;
  dump(w, prec, precs[prec]);   // enum nr_gemm_precision follows the order of precs
  return 0;
}

// The one argument `ksplit`: the K-split rule the host and the kernels share, one line per (K, want):
//   K want k_chunk(K, want) k_split(K, want).kchunk k_split(K, want).splits k_chunk(K, that .splits)
int dump_ksplit() {
  const int64_t Ks[] = {32, 64, 96, 480, 1152, 20832};
  for (int64_t K : Ks)
    for (int64_t want = 1; want <= 64; ++want) {
      const KSplit ks = k_split(K, want);
      printf("%lld %lld %lld %lld %d %lld\n", (long long)K, (long long)want, (long long)k_chunk(K, want),
             (long long)ks.kchunk, ks.splits, (long long)k_chunk(K, ks.splits));
    }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "ksplit")) return dump_ksplit();
  if (argc > 1) {
    const int rc = argc >= 12 ? dump_argv(argv + 1, argc - 12) : 2;
    if (rc)
      fprintf(stderr, "usage: %s [NAME M N K kc|mn A_LD kc|mn B_LD EPILOGUE static|dyn|mdev f32|bf16x6|bf16 "
              "[amap=|bmap=plain|gather|conv3 aseg= bseg= cmap=gather|conv3 cseg= seq= split= work=0|1]]\n", argv[0]);
    return rc;
  }
  for (const Row& w : ROWS_TABLE) {
    dump(w, NR_GEMM_BF16X6, "bf16x6");
    dump(w, NR_GEMM_BF16, "bf16");
  }
  for (const Row& w : ROWS_TABLE)   // exact f32: 64 x 64 below 400 tiles, else 128 x 128
    if (!strcmp(w.name, "small_static") || !strcmp(w.name, "bert_qkv")) dump(w, NR_GEMM_F32, "f32");
  return 0;
}
