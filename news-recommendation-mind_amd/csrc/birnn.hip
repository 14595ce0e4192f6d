// Bidirectional-LSTM news (title) encoder, RNN_Encoder (models/Encoders/RNN.py:5-33): the sequential
// part of nn.LSTM(E, H, batch_first=True, bidirectional=True) over nseq titles of L tokens, h0 = c0 = 0,
// all L steps run (no packing), with the reference's two outputs
//   tok[n, t]  = 1/2 (h->_t + h<-_t)          (out.view(.., L, 2, H).mean(-2))
//   news[n]    = 1/2 (h->_{L-1} + h<-_0)      (h_n.mean(0))
//
// The input projections x W_ih^T + b_ih of both directions are one GEMM before this kernel.  Here a
// workgroup (8 waves) owns a TILE of 16 sequences of ONE direction, so W_hh is read once per step per
// tile rather than per sequence, and the step's [4H x H] . [H x 16] product runs on
// v_mfma_f32_16x16x4_f32 (exact f32: every product rounded once, as an fmaf chain):
//   forward   A = W_hh rows, re-ordered so that a 16-row tile holds the i,f,g,o rows of 4 hidden units
//             (row 4*ul + gate): the 4 accumulator registers of a lane are then the four gates of ONE
//             (unit, sequence) pair and the cell update needs no exchange.  B = h [k][16 seq] in LDS.
//   backward  A = W_hh^T tiles of 16 hidden units, contraction index 4*unit + gate, B = the gate
//             gradients [4*unit + gate][16 seq] in LDS; the result dh_{t-1} goes back through LDS.
// Both A operands are packed by the caller in lane order (one coalesced 256-B load per MFMA) and are
// streamed from L2 every step.
//
// No atomics anywhere: the two directions write separate state, and the 1/2 (-> + <-) outputs are
// formed by a second kernel inside nr_birnn_fwd, so two calls give the same bits.
#include "common.h"
#include "../../include/newsrec_hip.h"

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int BIRNN_THREADS = 512;   // 8 waves
constexpr int BIRNN_WAVES = BIRNN_THREADS / 64;
constexpr int BIRNN_TILE = 16;       // sequences per workgroup
constexpr int BIRNN_MAX_H = 256;

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + __expf(-x)); }

struct BiArgs {
  const float* gx; int64_t ldgx;
  const float* whh;            // fwd: [2][UT][UT][64]; bwd: [2][RT][4*UT][64]
  const float* bhh;            // [2][4H] or NULL
  int64_t nseq; int L; int H;
  float* gates;                // [2][ntile][L][UT][5][64]
  float* hprev; int64_t ldh;   // [2][nseq*L][ldh]
  float* hlast;                // [2][nseq][H]
  float* news; int64_t ldn;
  float* tok; int64_t ldt;
  const float* dnews; int64_t lddn;
  const float* dtok; int64_t lddt;
  float* dg; int64_t lddg;
};

// The step product of one wave: NTL row tiles (tile wave + 8 i of `ntiles`) against the [4 KS][16] LDS
// operand `bs`, A streamed from the lane-order pack `wp` ([tile][KS][64], + lane applied).  The A
// operands are fetched KC k-steps ahead of the MFMAs that use them (two register chunks).
template <int NTL, int KC>
struct BiChunk { float a[KC][NTL]; };

template <int NTL, int KC>
__device__ __forceinline__ void bi_load(BiChunk<NTL, KC>& c, const float* wp, int wave, int ntiles, int KS, int ks0) {
#pragma unroll
  for (int kk = 0; kk < KC; ++kk) {
#pragma unroll
    for (int i = 0; i < NTL; ++i) {
      const int T = wave + BIRNN_WAVES * i, ks = ks0 + kk;
      c.a[kk][i] = (T < ntiles && ks < KS) ? wp[((int64_t)T * KS + ks) * 64] : 0.f;
    }
  }
}

template <int NTL, int KC, int NCH>
__device__ __forceinline__ void bi_mma(const BiChunk<NTL, KC>& c, const float* bs, int q, int s, int wave, int ntiles,
                                       int KS, int ks0, f32x4 (&acc)[NTL][NCH]) {
#pragma unroll
  for (int kk = 0; kk < KC; ++kk) {
    const int ks = ks0 + kk;
    if (ks < KS) {   // uniform
      const float b = bs[(4 * ks + q) * 16 + s];
#pragma unroll
      for (int i = 0; i < NTL; ++i)
        if (wave + BIRNN_WAVES * i < ntiles)   // wave-uniform
          acc[i][kk % NCH] = __builtin_amdgcn_mfma_f32_16x16x4f32(c.a[kk][i], b, acc[i][kk % NCH], 0, 0, 0);
    }
  }
}

// -> acc[i] = row tile (wave + 8 i)'s [16 x 16] product.  A wave with fewer than 3 tiles keeps two
// accumulator chains per tile (even / odd k-steps); with more, the tiles themselves are independent.
template <int NTL>
__device__ __forceinline__ void bi_product(const float* wp, const float* bs, int q, int s, int wave, int ntiles,
                                           int KS, f32x4 (&out)[NTL]) {
  // k-steps per register chunk (KC * NTL operands each, two chunks): as deep as the registers of the
  // kernels that use this width allow without spilling
  constexpr int KC = NTL <= 2 ? 16 : NTL == 3 ? 8 : NTL <= 5 ? 4 : NTL <= 7 ? 2 : 1;
  constexpr int NCH = NTL >= 3 ? 1 : 2;
  f32x4 acc[NTL][NCH];
#pragma unroll
  for (int i = 0; i < NTL; ++i)
#pragma unroll
    for (int c = 0; c < NCH; ++c) acc[i][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  BiChunk<NTL, KC> c0, c1;
  bi_load(c0, wp, wave, ntiles, KS, 0);
  for (int ks0 = 0; ks0 < KS; ks0 += 2 * KC) {
    bi_load(c1, wp, wave, ntiles, KS, ks0 + KC);
    bi_mma<NTL, KC, NCH>(c0, bs, q, s, wave, ntiles, KS, ks0, acc);
    bi_load(c0, wp, wave, ntiles, KS, ks0 + 2 * KC);
    bi_mma<NTL, KC, NCH>(c1, bs, q, s, wave, ntiles, KS, ks0 + KC, acc);
  }
#pragma unroll
  for (int i = 0; i < NTL; ++i) out[i] = NCH == 2 ? acc[i][0] + acc[i][NCH - 1] : acc[i][0];
}

// NT = unit tiles (4 hidden units each) per wave: UT = ceil(H / 4) <= 8 * NT
template <int NT>
__global__ __launch_bounds__(BIRNN_THREADS) void birnn_fwd_kernel(BiArgs g) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int H = g.H, L = g.L;
  const int UT = (H + 3) / 4;          // unit tiles == k-steps of the forward product
  const int HK = 4 * UT;               // rows of the h tile
  float* hbuf = sm;                    // [2][HK][16]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: the per-tile branches stay uniform
  const int s = lane & 15, q = lane >> 4;
  const int dir = blockIdx.y;
  const int64_t tile = blockIdx.x;
  const int64_t ntile = gridDim.x;
  const int64_t seq = tile * BIRNN_TILE + s;
  const bool vs = seq < g.nseq;
  const float* wp = g.whh + (int64_t)dir * UT * UT * 64 + lane;
  float* hp_out = g.hprev + (int64_t)dir * g.nseq * L * g.ldh;
  float* hl_out = g.hlast + (int64_t)dir * g.nseq * H;

  for (int i = tid; i < HK * 16; i += BIRNN_THREADS) hbuf[i] = 0.f;
  float c[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) c[i] = 0.f;
  __syncthreads();

  for (int t = 0; t < L; ++t) {
    const int tt = dir ? L - 1 - t : t;
    const int64_t row = seq * L + tt;
    const float* hc = hbuf + (t & 1) * HK * 16;
    float* hn = hbuf + ((t & 1) ^ 1) * HK * 16;
    // this step's input projections (+ b_hh, a cached re-read): issued before the product, consumed after it
    float x[NT][4];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int u = 4 * (wave + BIRNN_WAVES * i) + q;
      const bool ok = vs && u < H;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int col = dir * 4 * H + k * H + u;
        x[i][k] = ok ? g.gx[row * g.ldgx + col] + (g.bhh ? g.bhh[col] : 0.f) : 0.f;
      }
    }
    f32x4 acc[NT];
    bi_product<NT>(wp, hc, q, s, wave, UT, UT, acc);
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int T = wave + BIRNN_WAVES * i;
      if (T >= UT) continue;
      const int u = 4 * T + q;
      const bool ok = vs && u < H;
      const float hp = hc[u * 16 + s];
      float ig = 0.f, fg = 0.f, gg = 0.f, og = 0.f, cn = 0.f, hv = 0.f;
      const float cp = c[i];
      if (ok) {
        ig = sigm(x[i][0] + acc[i][0]);
        fg = sigm(x[i][1] + acc[i][1]);
        gg = tanhf(x[i][2] + acc[i][2]);
        og = sigm(x[i][3] + acc[i][3]);
        cn = fmaf(fg, cp, ig * gg);
        hv = og * tanhf(cn);
        hp_out[row * g.ldh + u] = hp;
        if (t == L - 1) hl_out[seq * H + u] = hv;
      }
      float* gs = g.gates + ((((int64_t)dir * ntile + tile) * L + tt) * UT + T) * 5 * 64 + lane;
      gs[0] = ig; gs[64] = fg; gs[128] = gg; gs[192] = og; gs[256] = ok ? cp : 0.f;
      c[i] = cn;
      hn[u * 16 + s] = hv;
    }
    __syncthreads();
  }
}

// tok / news = 1/2 (forward direction + reverse direction), from the saved state: h->_t is hprev-> of
// step t + 1 (hlast-> at t = L - 1), h<-_t is hprev<- of token t - 1 (hlast<- at t = 0)
__global__ __launch_bounds__(256) void birnn_combine_kernel(BiArgs g) {
  const int H = g.H, L = g.L;
  const int64_t T = g.nseq * L;
  const int64_t n_news = g.nseq * H;
  const int64_t total = n_news + (g.tok ? T * H : 0);
  const float* hp0 = g.hprev;
  const float* hp1 = g.hprev + T * g.ldh;
  const float* hl0 = g.hlast;
  const float* hl1 = g.hlast + n_news;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    if (i < n_news) {
      const int64_t n = i / H;
      const int u = (int)(i - n * H);
      g.news[n * g.ldn + u] = 0.5f * (hl0[i] + hl1[i]);
    } else {
      const int64_t j = i - n_news;
      const int64_t row = j / H;
      const int u = (int)(j - row * H);
      const int64_t n = row / L;
      const int t = (int)(row - n * L);
      const float a = t < L - 1 ? hp0[(row + 1) * g.ldh + u] : hl0[n * H + u];
      const float b = t > 0 ? hp1[(row - 1) * g.ldh + u] : hl1[n * H + u];
      g.tok[row * g.ldt + u] = 0.5f * (a + b);
    }
  }
}

// NT as the forward; NR = row tiles (16 hidden units each) of W_hh^T per wave: RT = ceil(H / 16) <= 8 * NR
template <int NT, int NR>
__global__ __launch_bounds__(BIRNN_THREADS) void birnn_bwd_kernel(BiArgs g) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int H = g.H, L = g.L;
  const int UT = (H + 3) / 4;
  const int KS = 4 * UT;               // k-steps of the backward product (contraction 4*unit + gate)
  const int RT = (H + 15) / 16;
  float* dgs = sm;                     // [16 * UT][16]   gate gradients, row 4*unit + gate
  float* dhs = sm + 16 * UT * 16;      // [16 * RT][16]   dh from the recurrent path
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: the per-tile branches stay uniform
  const int s = lane & 15, q = lane >> 4;
  const int dir = blockIdx.y;
  const int64_t tile = blockIdx.x;
  const int64_t ntile = gridDim.x;
  const int64_t seq = tile * BIRNN_TILE + s;
  const bool vs = seq < g.nseq;
  const float* wp = g.whh + (int64_t)dir * RT * KS * 64 + lane;

  for (int i = tid; i < 16 * RT * 16; i += BIRNN_THREADS) dhs[i] = 0.f;
  float dc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) dc[i] = 0.f;
  __syncthreads();

  for (int t = L - 1; t >= 0; --t) {
    const int tt = dir ? L - 1 - t : t;
    const int64_t row = seq * L + tt;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int T = wave + BIRNN_WAVES * i;
      if (T >= UT) continue;
      const int u = 4 * T + q;
      const bool ok = vs && u < H;
      const float* gs = g.gates + ((((int64_t)dir * ntile + tile) * L + tt) * UT + T) * 5 * 64 + lane;
      const float ig = gs[0], fg = gs[64], gg = gs[128], og = gs[192], cp = gs[256];
      float di = 0.f, df = 0.f, dgg = 0.f, dog = 0.f, dcn = 0.f;
      if (ok) {
        float dh = dhs[u * 16 + s];
        if (g.dtok) dh = fmaf(0.5f, g.dtok[row * g.lddt + u], dh);
        if (g.dnews && t == L - 1) dh = fmaf(0.5f, g.dnews[seq * g.lddn + u], dh);
        const float cc = fmaf(fg, cp, ig * gg);
        const float tc = tanhf(cc);
        const float dcc = dc[i] + dh * og * (1.f - tc * tc);
        di = dcc * gg * ig * (1.f - ig);
        df = dcc * cp * fg * (1.f - fg);
        dgg = dcc * ig * (1.f - gg * gg);
        dog = dh * tc * og * (1.f - og);
        dcn = dcc * fg;
        float* o = g.dg + row * g.lddg + dir * 4 * H + u;
        o[0] = di; o[H] = df; o[2 * H] = dgg; o[3 * H] = dog;
      }
      dc[i] = dcn;
      float* d = dgs + (4 * u) * 16 + s;
      d[0] = di; d[16] = df; d[32] = dgg; d[48] = dog;
    }
    if (t == 0) break;                 // dh of the zero initial state is nobody's gradient
    __syncthreads();
    f32x4 acc[NR];
    bi_product<NR>(wp, dgs, q, s, wave, RT, KS, acc);
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int R = wave + BIRNN_WAVES * j;
      if (R < RT) {
#pragma unroll
        for (int r = 0; r < 4; ++r) dhs[(16 * R + 4 * q + r) * 16 + s] = acc[j][r];
      }
    }
    __syncthreads();
  }
}

size_t birnn_fwd_smem(int H) { return (size_t)2 * 4 * ((H + 3) / 4) * 16 * sizeof(float); }
size_t birnn_bwd_smem(int H) { return (size_t)(16 * ((H + 3) / 4) + 16 * ((H + 15) / 16)) * 16 * sizeof(float); }

template <typename Kern>
int birnn_launch(Kern kern, dim3 grid, size_t smem, hipStream_t stream, const BiArgs& g) {
  if (smem > 64 * 1024 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess)
    return -(int)hipGetLastError();
  hipLaunchKernelGGL(kern, grid, dim3(BIRNN_THREADS), smem, stream, g);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

}  // namespace

extern "C" int nr_birnn_fwd(const float* gx, int64_t ldgx, const float* whh_fwd, const float* bhh, int64_t nseq,
                            int32_t L, int32_t H, float* gates, float* hprev, int64_t ldh, float* hlast,
                            float* news, int64_t ldn, float* tok, int64_t ldt, hipStream_t stream) {
  const int64_t ntile = (nseq + BIRNN_TILE - 1) / BIRNN_TILE;
  if (nseq < 0 || L < 1 || H < 1 || H > BIRNN_MAX_H || ldgx < 8 * (int64_t)H || ldh < H || ldn < H ||
      (tok && ldt < H) || ntile > 0x7fffffff)
    return NR_EINVAL(0);
  if (!gx || !whh_fwd || !gates || !hprev || !hlast || !news) return NR_EINVAL(1);
  if (nseq == 0) return NR_OK;
  BiArgs g{};
  g.gx = gx; g.ldgx = ldgx; g.whh = whh_fwd; g.bhh = bhh; g.nseq = nseq; g.L = L; g.H = H; g.gates = gates;
  g.hprev = hprev; g.ldh = ldh; g.hlast = hlast; g.news = news; g.ldn = ldn; g.tok = tok; g.ldt = ldt;
  const dim3 grid((unsigned)ntile, 2);
  const size_t smem = birnn_fwd_smem(H);
  const int NT = ((H + 3) / 4 + BIRNN_WAVES - 1) / BIRNN_WAVES;   // 1 .. 8 for H <= 256
  int rc;
  switch (NT) {
    case 1: rc = birnn_launch(birnn_fwd_kernel<1>, grid, smem, stream, g); break;
    case 2: rc = birnn_launch(birnn_fwd_kernel<2>, grid, smem, stream, g); break;
    case 3: rc = birnn_launch(birnn_fwd_kernel<3>, grid, smem, stream, g); break;
    case 4: rc = birnn_launch(birnn_fwd_kernel<4>, grid, smem, stream, g); break;
    case 5: rc = birnn_launch(birnn_fwd_kernel<5>, grid, smem, stream, g); break;
    case 6: rc = birnn_launch(birnn_fwd_kernel<6>, grid, smem, stream, g); break;
    case 7: rc = birnn_launch(birnn_fwd_kernel<7>, grid, smem, stream, g); break;
    case 8: rc = birnn_launch(birnn_fwd_kernel<8>, grid, smem, stream, g); break;
    default: return NR_EINVAL(0);
  }
  if (rc != NR_OK) return rc;
  const int64_t total = nseq * H + (tok ? nseq * L * H : 0);
  const unsigned blocks = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(birnn_combine_kernel, dim3(blocks), dim3(256), 0, stream, g);
  NR_LAUNCH_CHECK();
  return NR_OK;
}

extern "C" int nr_birnn_bwd(const float* whh_bwd, const float* gates, int64_t nseq, int32_t L, int32_t H,
                            const float* dnews, int64_t lddn, const float* dtok, int64_t lddt, float* dg,
                            int64_t lddg, hipStream_t stream) {
  const int64_t ntile = (nseq + BIRNN_TILE - 1) / BIRNN_TILE;
  if (nseq < 0 || L < 1 || H < 1 || H > BIRNN_MAX_H || lddg < 8 * (int64_t)H || (dnews && lddn < H) ||
      (dtok && lddt < H) || ntile > 0x7fffffff)
    return NR_EINVAL(0);
  if (!whh_bwd || !gates || !dg || (!dnews && !dtok)) return NR_EINVAL(1);
  if (nseq == 0) return NR_OK;
  BiArgs g{};
  g.whh = whh_bwd; g.gates = const_cast<float*>(gates); g.nseq = nseq; g.L = L; g.H = H; g.dnews = dnews;
  g.lddn = lddn; g.dtok = dtok; g.lddt = lddt; g.dg = dg; g.lddg = lddg;
  const dim3 grid((unsigned)ntile, 2);
  const size_t smem = birnn_bwd_smem(H);
  const int NT = ((H + 3) / 4 + BIRNN_WAVES - 1) / BIRNN_WAVES;
  switch (NT) {   // RT = ceil(H / 16) <= 8 exactly when NT <= 4
    case 1: return birnn_launch(birnn_bwd_kernel<1, 1>, grid, smem, stream, g);
    case 2: return birnn_launch(birnn_bwd_kernel<2, 1>, grid, smem, stream, g);
    case 3: return birnn_launch(birnn_bwd_kernel<3, 1>, grid, smem, stream, g);
    case 4: return birnn_launch(birnn_bwd_kernel<4, 1>, grid, smem, stream, g);
    case 5: return birnn_launch(birnn_bwd_kernel<5, 2>, grid, smem, stream, g);
    case 6: return birnn_launch(birnn_bwd_kernel<6, 2>, grid, smem, stream, g);
    case 7: return birnn_launch(birnn_bwd_kernel<7, 2>, grid, smem, stream, g);
    case 8: return birnn_launch(birnn_bwd_kernel<8, 2>, grid, smem, stream, g);
    default: return NR_EINVAL(0);
  }
}
