// EQTransformer: training step of the three decoder stacks and their heads, trunk frozen (vp_eqt_dec_train_*).
//
// The trunk is the inference plan of an internal Net up to the launch that reads `decoder.in`; what follows it is new:
//
//   forward    a_i = relu(conv_i(up2(a_{i-1})) + b_i), i = 0 .. 6        dec_conv_kernel<FWD>   (fp32 MFMA 16x16x4)
//   heads      z = conv11(a_6) + b, p = sigmoid(z), gz_h = dL/dz         dec_head_kernel        (vector ALU, 89 terms)
//   loss       0.05 BCE(det) + 0.40 BCE(P) + 0.55 BCE(S) in float64      bce_launch (bce.hip)
//   d input    ga_6 = conv11^T(gz_h); gu = conv_i^T(gz_i), ga_{i-1}[j] = gu[2j] + gu[2j+1], gz_{i-1} = ga_{i-1} (a_{i-1} > 0)
//                                                                        dec_head_dgrad_kernel, dec_conv_kernel<DGRAD>
//   d weight   gW[co][ci][k] = sum_b sum_t gz[co][t] u[ci][t + k - pad], gb = sum gz
//                                                                        dec_wgrad_kernel + dec_fold_kernel
//   update     torch.optim.Adam                                          OptimState::update (train_optim.hip)
//
// The weights, their gradient and Adam's state are the OptimState both trainers hold (train_optim.h); device memory is owned
// DevArrays.  The seven stages are stated once, in StageTable: launches, tensor sizes and offsets all follow from its rows.
//
// Every tensor is a dense row block [3 decoders][B][C][L]; the x2 nearest up-sample and the crop of stage 2 (376 -> 375)
// exist only as the index `s >> 1`, `s < Lout` of the operand load into LDS.  No atomics: a weight gradient is summed per
// workgroup over a fixed list of (window, time chunk) units and the workgroups' partial blocks are folded in index order, so
// two runs from the same state give the same bits.
//
// Scope VP_EQT_TRAIN_PICK_BRANCHES adds the two pick branches in front of the P and S decoders (train_eqt_pick.hip): their
// training forward writes sets 1 and 2 of decoder.in, stage 0's input gradient (dec_conv_kernel<DGRAD> without the ReLU gate:
// decoder.in is no ReLU output) feeds their adjoints, and their eighteen tensors join the weight blob.  Scope
// VP_EQT_TRAIN_DECODERS runs the launches above and nothing else.
#include <cmath>
#include <memory>

#include "api_handle.h"
#include "batchgen.h"
#include "bce.h"
#include "net.h"
#include "train_eqt_pick.h"
#include "train_optim.h"

namespace vp {
namespace {

// ---- the stages ----------------------------------------------------------------------------------------------------------
// One row per stage, in order: input channels, output channels, taps, and the samples per workgroup of its forward and of its
// input-gradient launch (stage 4 runs 256 forward and 128 backward), and whether its input is a ReLU output (decoder.in is
// not; stage 0's input gradient is formed for the pick branches alone).
template <int CI_, int CO_, int K_, int TN_FWD_, int TN_DGRAD_, bool RELU_IN_ = true>
struct StageCfg {
  static constexpr int CI = CI_, CO = CO_, K = K_, TN_FWD = TN_FWD_, TN_DGRAD = TN_DGRAD_;
  static constexpr bool RELU_IN = RELU_IN_;
};
template <class... S>
struct StageList {
  static constexpr int N = sizeof...(S);
  static constexpr int CI[N] = {S::CI...}, CO[N] = {S::CO...}, K[N] = {S::K...};
  // f(row i), the row as a value of its StageCfg type
  template <class F>
  static void at(int i, F&& f) {
    int n = 0;
    ((n++ == i ? f(S{}) : void()), ...);
  }
};
// clang-format off
using StageTable = StageList<
    StageCfg<16, 64,  3, 128, 128, false>,
    StageCfg<64, 64,  5, 128, 128>,
    StageCfg<64, 32,  5, 128, 128>,
    StageCfg<32, 32,  7, 128, 128>,
    StageCfg<32, 16,  7, 256, 128>,
    StageCfg<16, 16,  9, 256, 256>,
    StageCfg<16,  8, 11, 256, 256>>;
// clang-format on
constexpr int NSTAGE = StageTable::N, NSET = 3, T_OUT = 6000, HK = 11, HC = 8, DIN0 = 47;
constexpr auto &kCi = StageTable::CI, &kCo = StageTable::CO, &kK = StageTable::K;
constexpr int kDin[NSTAGE] = {47, 94, 188, 375, 750, 1500, 3000};  // samples in / out: x2, stage 2 cropped (376 -> 375)
constexpr int kDout[NSTAGE] = {94, 188, 375, 750, 1500, 3000, 6000};
static_assert(kCi[0] == 16 && kCo[NSTAGE - 1] == HC && kDin[0] == DIN0 && kDout[NSTAGE - 1] == T_OUT, "decoder.in is [16][47], the head reads [8][6000]");
const char* const kDecPrefix[NSET] = {"decoder_d", "pick_decoders.0", "pick_decoders.1"};
const char* const kHeadPrefix[NSET] = {"conv_d", "pick_convs.0", "pick_convs.1"};

// ---- forward conv / input-gradient conv on the fp32 matrix cores ---------------------------------------------------------
// D[m][n] = sum over (tap k, reduction channel c) of A[m][(k, c)] * rows[c][col(n) + k], v_mfma_f32_16x16x4_f32: lane l feeds
// A[l & 15][l >> 4] and B[l >> 4][l & 15] and holds D[4 (l >> 4) + r][l & 15], r = 0 .. 3.
//   FWD    m = output channel, c = input channel, rows = the up-sampled input u[c][s] = x[c][s >> 1] (0 outside [0, Lout)),
//          A = W[m][c][k]; the accumulator starts at the bias: one chain of CR K + 1 terms.
//   DGRAD  m = input channel of the conv, c = its output channel, rows = gz[c][s] (0 outside [0, Lout)), A = W[c][m][K-1-k]:
//          gu[m][s]; the n-tiles come in pairs that hold gu[2j] and gu[2j+1] of the same j in the same lane, so the up-sample's
//          adjoint is one addition in registers (a chain of CR K terms and one pair sum); gu[Lout] of the cropped stage does
//          not exist and is left out of the pair.  RELU_IN = false (stage 0): the input is no ReLU output, ga is the result
//          and there is no gz.
struct ConvTArgs {
  const float* src;  // [3 B][CR][Ls]
  const float* w;    // the trainer's weight blob
  int w_off[NSET], b_off[NSET];
  float* dst;        // FWD: a_i [3 B][CM][Lout]; DGRAD: ga_{i-1} [3 B][CM][Lprev]
  float* dst2;       // DGRAD: gz_{i-1}
  const float* act;  // DGRAD: a_{i-1}
  int B, Ls, Lout, Lprev;
};

template <int CR, int K, int TN>
struct ConvTile {
  static constexpr int W = TN + K - 1;
  static constexpr int S = (W + 31) / 32 * 32 + 16;  // row stride = 16 mod 32: the four rows of a B fragment in four bank groups
};

template <bool DGRAD, int CR, int CM, int K, int TN, bool RELU_IN = true>
__global__ __launch_bounds__(256) void dec_conv_kernel(const ConvTArgs a) {
  constexpr int MT = (CM + 15) / 16, NG = 4 / MT, NTW = TN / 16 / NG, CB = CR / 4, STEPS = CB * K, PAD = K / 2;
  constexpr int S = ConvTile<CR, K, TN>::S, W = ConvTile<CR, K, TN>::W;
  static_assert(MT == 1 || MT == 2 || MT == 4, "m-tiles per workgroup");
  static_assert(CR % 4 == 0 && TN % (16 * NG) == 0 && (!DGRAD || NTW % 2 == 0), "tile shape");
  __shared__ float rows[CR * S];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int win = blockIdx.y, set = win / a.B, t0 = blockIdx.x * TN;
  const int mt = wave % MT, ng = wave / MT, lm = lane & 15, lk = lane >> 4;

  {  // operand rows: samples [t0 - PAD, t0 - PAD + W) of the (virtual) row, zero outside [0, Lout)
    const float* src = a.src + (long)win * CR * a.Ls;
    for (int idx = tid; idx < CR * S; idx += 256) {
      const int c = idx / S, j = idx - c * S, s = t0 - PAD + j;
      float v = 0.f;
      if (j < W && s >= 0 && s < a.Lout) v = src[(long)c * a.Ls + (DGRAD ? s : (s >> 1))];
      rows[idx] = v;
    }
  }
  float af[STEPS];  // this wave's A fragments, one per (tap, channel block)
  {
    const float* w = a.w + a.w_off[set];
    const int m = mt * 16 + lm;
#pragma unroll
    for (int st = 0; st < STEPS; ++st) {
      const int k = st / CB, c = (st % CB) * 4 + lk;
      float v = 0.f;
      if (m < CM) v = DGRAD ? w[((long)c * CM + m) * K + (K - 1 - k)] : w[((long)m * CR + c) * K + k];
      af[st] = v;
    }
  }
  f32x4 acc[NTW];
#pragma unroll
  for (int j = 0; j < NTW; ++j) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = mt * 16 + 4 * lk + r;
      acc[j][r] = (!DGRAD && m < CM) ? a.w[a.b_off[set] + m] : 0.f;
    }
  }
  __syncthreads();
  int col[NTW];
#pragma unroll
  for (int j = 0; j < NTW; ++j) {
    const int nt = ng * NTW + j;
    col[j] = DGRAD ? 2 * ((nt >> 1) * 16 + lm) + (nt & 1) : nt * 16 + lm;
  }
#pragma unroll
  for (int st = 0; st < STEPS; ++st) {
    const int k = st / CB, c = (st % CB) * 4 + lk;
    const float* row = rows + c * S + k;
#pragma unroll
    for (int j = 0; j < NTW; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[st], row[col[j]], acc[j], 0, 0, 0);
  }
  if (!DGRAD) {
    float* dst = a.dst + (long)win * CM * a.Lout;
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
      const int t = t0 + col[j];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = mt * 16 + 4 * lk + r;
        const float v = acc[j][r];
        if (m < CM && t < a.Lout) dst[(long)m * a.Lout + t] = v < 0.f ? 0.f : v;
      }
    }
  } else {
    const long base = (long)win * CM * a.Lprev;
#pragma unroll
    for (int p = 0; p < NTW / 2; ++p) {
      const int s = t0 + col[2 * p], jo = s >> 1;  // s even: gu[s] in tile 2p, gu[s + 1] in tile 2p + 1
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = mt * 16 + 4 * lk + r;
        if (m < CM && s < a.Lout) {
          const float g = (s + 1 < a.Lout) ? acc[2 * p][r] + acc[2 * p + 1][r] : acc[2 * p][r];
          const long o = base + (long)m * a.Lprev + jo;
          a.dst[o] = g;
          if constexpr (RELU_IN) a.dst2[o] = a.act[o] > 0.f ? g : 0.f;
        }
      }
    }
  }
}

// ---- weight and bias gradient on the fp32 matrix cores ---------------------------------------------------------------------
// Per tap k: D_k[co][ci] = sum_t gz[co][t] u[ci][t + k - pad]  (A[m][kk] = gz[co0 + m][t + kk], B[kk][n] = u[ci0 + n][t + kk + k - pad]);
// the bias gradient is one more tile per m-tile whose B fragment is 1 in column 0.  Workgroup g of a decoder walks the units
// (window b, chunk of TC samples) g, g + NBLK, ... in that order and keeps the sums in registers; its block of CO CI K + CO
// sums goes to partial[set][g].  NBLK <= 256 per decoder: 768 workgroups, three per CU; 1024 per decoder for the small blocks
// (stages 0 and 3-6, the head) measured slower, 5.90 against 5.46 ms for the step's weight gradients at B = 256.
constexpr int WG_TC = 64;
constexpr int wgrad_max_blocks(size_t) { return 256; }

struct WgradArgs {
  const float* gz;   // [3 B][CO][Lout]
  const float* src;  // [3 B][CI][Ls]
  float* partial;    // [3][nblk][CO CI K + CO]
  int B, Ls, Lout, nchunks, nblk;
};

template <int CO, int CI, int K, bool UP>
__global__ __launch_bounds__(256) void dec_wgrad_kernel(const WgradArgs a) {
  constexpr int MT = (CO + 15) / 16, CIT = (CI + 15) / 16, NT_MAIN = MT * CIT * K, NT = NT_MAIN + MT, NTQ = (NT + 3) / 4;
  constexpr int PAD = K / 2, S2 = WG_TC + 4, W1 = WG_TC + K - 1, S1 = (W1 + 27) / 32 * 32 + 4;  // strides = 4 mod 32
  static_assert(S1 >= W1, "operand row");
  constexpr int PSZ = CO * CI * K + CO;
  __shared__ float gzs[MT * 16 * S2];
  __shared__ float us[CIT * 16 * S1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lm = lane & 15, lk = lane >> 4;
  const int g = blockIdx.x, set = blockIdx.y;
  int aoff[NTQ], boff[NTQ], kind[NTQ];  // kind: 0 tap tile, 1 bias tile, 2 none
  f32x4 acc[NTQ];
#pragma unroll
  for (int j = 0; j < NTQ; ++j) {
    const int q = wave + 4 * j;
    acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (q < NT_MAIN) {
      const int mt = q / (CIT * K), rem = q - mt * (CIT * K), cit = rem / K, k = rem - cit * K;
      kind[j] = 0, aoff[j] = (mt * 16 + lm) * S2 + lk, boff[j] = (cit * 16 + lm) * S1 + lk + k;
    } else if (q < NT) {
      kind[j] = 1, aoff[j] = ((q - NT_MAIN) * 16 + lm) * S2 + lk, boff[j] = 0;
    } else {
      kind[j] = 2, aoff[j] = boff[j] = 0;
    }
  }
  const float one0 = lm == 0 ? 1.f : 0.f;
  const int units = a.B * a.nchunks;
  for (int u = g; u < units; u += a.nblk) {
    const int b = u / a.nchunks, t0 = (u - b * a.nchunks) * WG_TC;
    const long win = (long)set * a.B + b;
    __syncthreads();  // the previous unit's fragments have been read
    for (int idx = tid; idx < MT * 16 * S2; idx += 256) {
      const int c = idx / S2, j = idx - c * S2, t = t0 + j;
      gzs[idx] = (c < CO && j < WG_TC && t < a.Lout) ? a.gz[(win * CO + c) * a.Lout + t] : 0.f;
    }
    for (int idx = tid; idx < CIT * 16 * S1; idx += 256) {
      const int c = idx / S1, j = idx - c * S1, s = t0 - PAD + j;
      us[idx] = (c < CI && j < W1 && s >= 0 && s < a.Lout) ? a.src[(win * CI + c) * a.Ls + (UP ? (s >> 1) : s)] : 0.f;
    }
    __syncthreads();
#pragma unroll 4
    for (int tt = 0; tt < WG_TC; tt += 4) {
#pragma unroll
      for (int j = 0; j < NTQ; ++j) {
        if (kind[j] == 2) continue;  // (wave-uniform)
        const float av = gzs[aoff[j] + tt];
        const float bv = kind[j] == 0 ? us[boff[j] + tt] : one0;
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[j], 0, 0, 0);
      }
    }
  }
  float* out = a.partial + ((long)set * a.nblk + g) * PSZ;
#pragma unroll
  for (int j = 0; j < NTQ; ++j) {
    const int q = wave + 4 * j;
    if (q < NT_MAIN) {
      const int mt = q / (CIT * K), rem = q - mt * (CIT * K), cit = rem / K, k = rem - cit * K;
      const int ci = cit * 16 + lm;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = mt * 16 + 4 * lk + r;
        if (co < CO && ci < CI) out[((long)co * CI + ci) * K + k] = acc[j][r];
      }
    } else if (q < NT && lm == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = (q - NT_MAIN) * 16 + 4 * lk + r;
        if (co < CO) out[CO * CI * K + co] = acc[j][r];
      }
    }
  }
}

// grad[...] = partial[set][0] + partial[set][1] + ... in that order; the first n_w sums are the weight, the rest the bias
struct FoldArgs {
  const float* partial;
  float* grad;
  int w_off[NSET], b_off[NSET];
  int nblk, n_w, psz;
};
__global__ __launch_bounds__(256) void dec_fold_kernel(const FoldArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x, set = blockIdx.y;
  if (i >= a.psz) return;
  const float* p = a.partial + (long)set * a.nblk * a.psz + i;
  float s = p[0];
  for (int g = 1; g < a.nblk; ++g) s += p[(long)g * a.psz];
  a.grad[i < a.n_w ? a.w_off[set] + i : a.b_off[set] + (i - a.n_w)] = s;
}

// ---- heads -----------------------------------------------------------------------------------------------------------------
// z = b + sum_ci sum_k W[ci][k] a6[ci][t + k - 5] (one fmaf chain, ci-major: 88 products on the bias), p = 1 / (1 + exp(-z)).
// Gradient as torch takes it, every step rounded to fp32: BCELoss backward (p - y) / max((1 - p) p, 1e-12) * w_h, / (B T) for
// the mean, then sigmoid backward * (1 - p) * p.
struct HeadArgs {
  const float* a6;   // [3 B][8][T]
  const float* w;
  int w_off[NSET], b_off[NSET];
  const float* y;    // (B, 3, T): rows detection, P, S
  float* logit;      // [3 B][T]
  float* p;          // (B, 3, T)
  float* gz;         // [3 B][T]
  float* ga6;        // [3 B][8][T] (dgrad)
  float* gz6;
  float lw[NSET], numel;
  int B;
};
__global__ __launch_bounds__(256) void dec_head_kernel(const HeadArgs a) {
  __shared__ float rows[HC][256 + HK - 1];
  __shared__ float wh[HC * HK];
  const int tid = threadIdx.x, win = blockIdx.y, set = win / a.B, b = win - set * a.B, t0 = blockIdx.x * 256;
  const float* src = a.a6 + (long)win * HC * T_OUT;
  for (int idx = tid; idx < HC * (256 + HK - 1); idx += 256) {
    const int c = idx / (256 + HK - 1), j = idx - c * (256 + HK - 1), s = t0 - HK / 2 + j;
    rows[c][j] = (s >= 0 && s < T_OUT) ? src[(long)c * T_OUT + s] : 0.f;
  }
  if (tid < HC * HK) wh[tid] = a.w[a.w_off[set] + tid];
  __syncthreads();
  const int t = t0 + tid;
  if (t >= T_OUT) return;
  float z = a.w[a.b_off[set]];
#pragma unroll
  for (int c = 0; c < HC; ++c)
#pragma unroll
    for (int k = 0; k < HK; ++k) z = fmaf(wh[c * HK + k], rows[c][tid + k], z);
  const float p = 1.f / (1.f + expf(-z));
  const long o = (long)win * T_OUT + t, od = ((long)b * NSET + set) * T_OUT + t;
  const float y = a.y[od];
  const float q = (1.f - p) * p;
  float g = (p - y) / fmaxf(q, 1e-12f) * a.lw[set];
  g = g / a.numel;
  g = g * (1.f - p) * p;
  a.logit[o] = z;
  a.p[od] = p;
  a.gz[o] = g;
}

// ga6[ci][s] = sum_k gz_h[s - k + 5] W[ci][k] (11 terms, k ascending), gz6 = ga6 (a6 > 0)
__global__ __launch_bounds__(256) void dec_head_dgrad_kernel(const HeadArgs a) {
  const int win = blockIdx.y, set = win / a.B, s = blockIdx.x * 256 + threadIdx.x;
  if (s >= T_OUT) return;
  const float* gz = a.gz + (long)win * T_OUT;
  const float* w = a.w + a.w_off[set];
  float g[HK];
#pragma unroll
  for (int k = 0; k < HK; ++k) {
    const int t = s - k + HK / 2;
    g[k] = (t >= 0 && t < T_OUT) ? gz[t] : 0.f;
  }
#pragma unroll
  for (int c = 0; c < HC; ++c) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < HK; ++k) v = fmaf(g[k], w[c * HK + k], v);
    const long o = ((long)win * HC + c) * T_OUT + s;
    a.ga6[o] = v;
    a.gz6[o] = a.a6[o] > 0.f ? v : 0.f;
  }
}

// decoder.in of the trunk's plan (haloed rows) -> the trainer's dense [3 B][16][47]
__global__ __launch_bounds__(256) void dec_copy_in_kernel(const float* __restrict__ src, int ls, long ws, float* __restrict__ dst, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long win = i / (16 * DIN0);
  const int rem = (int)(i - win * 16 * DIN0), c = rem / DIN0, j = rem - c * DIN0;
  dst[i] = src[win * ws + (long)c * ls + HALO + j];
}

// ---- the trainer -------------------------------------------------------------------------------------------------------------
struct DecParam {
  std::string name;
  size_t size, off_full, off;  // offset in the model's flat blob / in the trainer's
};

bool scope_ok(int scope) { return scope == VP_EQT_TRAIN_DECODERS || scope == VP_EQT_TRAIN_PICK_BRANCHES; }

// the scope's tensors in the flat blob's order: the 48 of the decoders and heads, with the pick branches' 18 in scope 1
std::vector<DecParam> dec_params(int scope = VP_EQT_TRAIN_DECODERS) {
  std::vector<DecParam> out;
  const ParamDesc* t;
  const int n = param_table(VP_MODEL_EQTRANSFORMER, &t);
  size_t full = 0, off = 0;
  for (int i = 0; i < n; ++i) {
    const std::string nm = t[i].name;
    bool mine = false;
    for (int d = 0; d < NSET; ++d)
      mine = mine || nm.rfind(std::string(kDecPrefix[d]) + ".", 0) == 0 || nm.rfind(std::string(kHeadPrefix[d]) + ".", 0) == 0;
    if (scope == VP_EQT_TRAIN_PICK_BRANCHES)
      for (int k = 0; k < PickDims::NBR; ++k)
        mine = mine || nm.rfind(std::string(kPickLstmPrefix[k]) + ".", 0) == 0 || nm.rfind(std::string(kPickAttPrefix[k]) + ".", 0) == 0;
    if (mine) {
      out.push_back({nm, t[i].size, full, off});
      off += t[i].size;
    }
    full += t[i].size;
  }
  return out;
}

struct DecTensor {
  std::string name;
  float* p;
  int sets, C, L;
};

struct DecTrainer {
  int device = 0, max_batch = 0, launches = 0, scope = VP_EQT_TRAIN_DECODERS;
  std::unique_ptr<PickState> pick;  // scope VP_EQT_TRAIN_PICK_BRANCHES
  hipStream_t stream = nullptr;
  Net net;
  int trunk_steps = 0, t_dec_in = -1;
  std::vector<DecParam> params;
  size_t n_params = 0;
  int w_off[NSTAGE + 1][NSET], b_off[NSTAGE + 1][NSET];  // [7] = the head
  OptimState opt;  // (no EMA: selector 4 of a read is refused)
  DevArray<float> din, a[NSTAGE], ga[NSTAGE], gz[NSTAGE], logit, gzh, pred, x_dev, y_dev, partial;
  DevArray<double> loss_dev;  // [0] the batch loss, [1 ..] per window
  std::vector<DecTensor> tensors;
  StagingRing rows_ring;
  bool timing = false;
  hipEvent_t ev[6] = {};
  ~DecTrainer() {  // (the device arrays free themselves, behind the wait for the stream)
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    if (pick) pick->release_events();
    if (stream) (void)hipStreamDestroy(stream);
    net.release();
  }
};

#define DTL(...)                     \
  do {                               \
    ++tr.launches;                   \
    hipLaunchKernelGGL(__VA_ARGS__); \
  } while (0)

int wgrad_blocks(int B, int Lout, size_t psz) { return std::min(B * ((Lout + WG_TC - 1) / WG_TC), wgrad_max_blocks(psz)); }

template <int CR, int CM, int K, int TN>
void launch_fwd(DecTrainer& tr, int i, int B) {
  ConvTArgs a{};
  a.src = i == 0 ? tr.din.p : tr.a[i - 1].p;
  a.w = tr.opt.w.p;
  for (int d = 0; d < NSET; ++d) a.w_off[d] = tr.w_off[i][d], a.b_off[d] = tr.b_off[i][d];
  a.dst = tr.a[i].p;
  a.B = B, a.Ls = kDin[i], a.Lout = kDout[i], a.Lprev = kDin[i];
  DTL((dec_conv_kernel<false, CR, CM, K, TN>), dim3((kDout[i] + TN - 1) / TN, NSET * B), dim3(256), 0, tr.stream, a);
}

// stage i's input gradient: gz_i -> ga_{i-1}, gz_{i-1}; stage 0's (RELU_IN = false), for the sets 1 and 2 alone: gz_0 -> pick.gv
template <int CR, int CM, int K, int TN, bool RELU_IN>
void launch_dgrad(DecTrainer& tr, int i, int B) {
  ConvTArgs a{};
  a.w = tr.opt.w.p;
  a.B = B, a.Ls = kDout[i], a.Lout = kDout[i], a.Lprev = kDin[i];
  if constexpr (RELU_IN) {
    a.src = tr.gz[i].p;
    for (int d = 0; d < NSET; ++d) a.w_off[d] = tr.w_off[i][d], a.b_off[d] = tr.b_off[i][d];
    a.dst = tr.ga[i - 1].p;
    a.dst2 = tr.gz[i - 1].p;
    a.act = tr.a[i - 1].p;
    DTL((dec_conv_kernel<true, CR, CM, K, TN>), dim3((kDout[i] + TN - 1) / TN, NSET * B), dim3(256), 0, tr.stream, a);
  } else {
    a.src = tr.gz[i].p + (long)B * CR * kDout[i];  // behind set 0
    for (int k = 0; k < PickDims::NBR; ++k) a.w_off[k] = tr.w_off[i][1 + k], a.b_off[k] = tr.b_off[i][1 + k];
    a.dst = tr.pick->gv.p;
    DTL((dec_conv_kernel<true, CR, CM, K, TN, false>), dim3((kDout[i] + TN - 1) / TN, PickDims::NBR * B), dim3(256), 0, tr.stream, a);
  }
}

template <int CO, int CI, int K, bool UP>
void launch_wgrad(DecTrainer& tr, int i, const float* gz, const float* src, int Ls, int Lout, int B) {
  WgradArgs a{};
  a.gz = gz, a.src = src, a.partial = tr.partial.p;
  a.B = B, a.Ls = Ls, a.Lout = Lout, a.nchunks = (Lout + WG_TC - 1) / WG_TC, a.nblk = wgrad_blocks(B, Lout, (size_t)CO * CI * K + CO);
  DTL((dec_wgrad_kernel<CO, CI, K, UP>), dim3(a.nblk, NSET), dim3(256), 0, tr.stream, a);
  FoldArgs f{};
  f.partial = tr.partial.p, f.grad = tr.opt.grad.p;
  for (int d = 0; d < NSET; ++d) f.w_off[d] = tr.w_off[i][d], f.b_off[d] = tr.b_off[i][d];
  f.nblk = a.nblk, f.n_w = CO * CI * K, f.psz = CO * CI * K + CO;
  DTL(dec_fold_kernel, dim3((f.psz + 255) / 256, NSET), dim3(256), 0, tr.stream, f);
}

// the launches of stage i, instantiated from its row of the table
void forward_stage(DecTrainer& tr, int i, int B) {
  StageTable::at(i, [&](auto s) { launch_fwd<s.CI, s.CO, s.K, s.TN_FWD>(tr, i, B); });
}
void dgrad_stage(DecTrainer& tr, int i, int B) {  // CR = the conv's output channels, CM = its input channels
  StageTable::at(i, [&](auto s) { launch_dgrad<s.CO, s.CI, s.K, s.TN_DGRAD, s.RELU_IN>(tr, i, B); });
}
void wgrad_stage(DecTrainer& tr, int i, int B) {
  const float* src = i == 0 ? tr.din.p : tr.a[i - 1].p;
  StageTable::at(i, [&](auto s) { launch_wgrad<s.CO, s.CI, s.K, true>(tr, i, tr.gz[i].p, src, kDin[i], kDout[i], B); });
}

int build(DecTrainer& tr, const float* weights, size_t n_floats, const vp_config& cfg) {
  ParamView pv;
  VP_REQUIRE(build_param_view(VP_MODEL_EQTRANSFORMER, weights, n_floats, &pv), "vp_eqt_dec_train_create: weight blob does not match the table");
  tr.net.model_kind = VP_MODEL_EQTRANSFORMER;
  tr.net.cfg = cfg;
  tr.net.cfg.max_batch = tr.max_batch;
  tr.net.max_batch = tr.max_batch;
  int rc = plan_eqt(tr.net, pv);
  if (rc == VP_OK) rc = tr.net.finalize_layout();
  if (rc != VP_OK) return rc;
  // the trunk: every launch in front of the first one that reads decoder.in
  tr.trunk_steps = -1;
  for (size_t i = 0; i < tr.net.steps.size() && tr.trunk_steps < 0; ++i) {
    const std::string& nm = tr.net.steps[i].name;
    if (nm.rfind("decoder.", 0) == 0 || nm.rfind("fused.dec03", 0) == 0) tr.trunk_steps = (int)i;
  }
  for (size_t i = 0; i < tr.net.tensors.size(); ++i)
    if (tr.net.tensors[i].name == "decoder.in") tr.t_dec_in = (int)i;
  VP_REQUIRE(tr.trunk_steps > 0 && tr.t_dec_in >= 0, "vp_eqt_dec_train_create: the plan has no decoder.in");
  if ((rc = tr.net.upload()) != VP_OK) return rc;

  tr.params = dec_params(tr.scope);
  tr.n_params = 0;
  for (const DecParam& p : tr.params) tr.n_params += p.size;
  for (const DecParam& p : tr.params) {
    int set = -1, stage = -1;
    bool picks = false;
    for (int k = 0; tr.pick && k < PickDims::NBR; ++k)
      for (int sg = 0; sg < PK_NSEG; ++sg)
        if (p.name == std::string(sg < PK_WX ? kPickLstmPrefix[k] : kPickAttPrefix[k]) + "." + kPickSegName[sg]) {
          VP_REQUIRE(p.size == (size_t)kPickSegSize[sg], "vp_eqt_dec_train_create: %s has %zu floats", p.name.c_str(), p.size);
          tr.pick->off[k][sg] = (int)p.off, picks = true;
        }
    if (picks) continue;
    for (int d = 0; d < NSET; ++d) {
      const std::string dp = std::string(kDecPrefix[d]) + ".convs.", hp = std::string(kHeadPrefix[d]) + ".";
      if (p.name.rfind(dp, 0) == 0) set = d, stage = p.name[dp.size()] - '0';
      if (p.name.rfind(hp, 0) == 0) set = d, stage = NSTAGE;
    }
    VP_REQUIRE(set >= 0 && stage >= 0 && stage <= NSTAGE, "vp_eqt_dec_train_create: unexpected tensor %s", p.name.c_str());
    const bool is_w = p.name.size() > 7 && p.name.compare(p.name.size() - 7, 7, ".weight") == 0;
    (is_w ? tr.w_off : tr.b_off)[stage][set] = (int)p.off;
  }
  std::vector<float> host(tr.n_params);
  for (const DecParam& p : tr.params) memcpy(host.data() + p.off, weights + p.off_full, p.size * sizeof(float));
  int r = tr.opt.alloc(tr.n_params);
  if (r != VP_OK) return r;
  VP_HIP(hipMemcpy(tr.opt.w.p, host.data(), tr.n_params * sizeof(float), hipMemcpyHostToDevice));
  std::fill(host.begin(), host.end(), 1.f);
  VP_HIP(hipMemcpy(tr.opt.mask.p, host.data(), tr.n_params * sizeof(float), hipMemcpyHostToDevice));

  auto rows = [&](DevArray<float>& b, const std::string& name, int sets, int C, int L) -> int {
    VP_HIP(b.alloc((size_t)sets * tr.max_batch * C * L, true));
    tr.tensors.push_back({name, b.p, sets, C, L});
    return VP_OK;
  };
  if ((r = rows(tr.din, "decoder.in", NSET, 16, kDin[0])) != VP_OK) return r;
  if (tr.pick) {
    tr.tensors.push_back({"pick.x", tr.din.p, 1, 16, kDin[0]});  // set 0 of decoder.in: the bottleneck the branches read
    const int pr = tr.pick->alloc(tr.max_batch, [&](const std::string& name, float* p, int sets, int C, int L) {
      tr.tensors.push_back({name, p, sets, C, L});
    });
    if (pr != VP_OK) return pr;
  }
  for (int i = 0; i < NSTAGE; ++i)
    if ((r = rows(tr.a[i], "a" + std::to_string(i), NSET, kCo[i], kDout[i])) != VP_OK) return r;
  if ((r = rows(tr.logit, "logits", NSET, 1, T_OUT)) != VP_OK) return r;
  if ((r = rows(tr.pred, "p", 1, NSET, T_OUT)) != VP_OK) return r;
  if ((r = rows(tr.gzh, "gz_head", NSET, 1, T_OUT)) != VP_OK) return r;
  for (int i = NSTAGE - 1; i >= 0; --i) {
    if ((r = rows(tr.ga[i], "ga" + std::to_string(i), NSET, kCo[i], kDout[i])) != VP_OK) return r;
    if ((r = rows(tr.gz[i], "gz" + std::to_string(i), NSET, kCo[i], kDout[i])) != VP_OK) return r;
  }
  VP_HIP(tr.x_dev.alloc((size_t)tr.max_batch * 3 * T_OUT));
  VP_HIP(tr.y_dev.alloc((size_t)tr.max_batch * 3 * T_OUT));
  VP_HIP(tr.loss_dev.alloc((size_t)1 + tr.max_batch, true));
  size_t partial = (size_t)wgrad_max_blocks(HC * HK + 1) * (HC * HK + 1);  // the largest [nblk][block] of any launch
  for (int i = 0; i < NSTAGE; ++i) {
    const size_t psz = (size_t)kCo[i] * kCi[i] * kK[i] + kCo[i];
    partial = std::max(partial, wgrad_max_blocks(psz) * psz);
  }
  VP_HIP(tr.partial.alloc((size_t)NSET * partial));
  VP_HIP(hipStreamCreateWithFlags(&tr.stream, hipStreamNonBlocking));
  for (auto& e : tr.ev) VP_HIP(hipEventCreate(&e));
  return VP_OK;
}

int run_step(DecTrainer& tr, const float* x_dev, const float* y_dev, int B, const double* lw, float lr, int update, double* loss) {
  hipStream_t s = tr.stream;
  Net& net = tr.net;
  tr.launches = 0;
  if (tr.timing) (void)hipEventRecord(tr.ev[0], s);
  {  // the frozen trunk, as vp_forward(preprocess = 0) runs it
    const Tensor& in = net.tensors[net.input];
    PreArgs pa{};
    pa.src = x_dev, pa.dense = 1, pa.T = net.in_samples, pa.preprocess = 0;
    pa.norm = net.cfg.norm, pa.per_comp = net.cfg.norm_amp_per_comp, pa.taper = net.cfg.taper_samples, pa.norm_eps = net.cfg.norm_eps;
    pa.dst = in.p, pa.lsd = in.ls, pa.wsd = (long)in.win_stride();
    pa.flags = net.win_flags ? net.win_flags->d : nullptr;
    launch_gather_normalize(pa, B, s);
    ++tr.launches;
    for (int i = 0; i < tr.trunk_steps; ++i) {
      const int rc = net.steps[i].run(net, B, s);
      if (rc != 0) return rc;
      ++tr.launches;
    }
    const Tensor& di = net.tensors[tr.t_dec_in];
    const long n = (long)NSET * B * 16 * kDin[0];
    DTL(dec_copy_in_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, di.p, di.ls, (long)di.win_stride(), tr.din.p, n);
  }
  if (tr.timing) (void)hipEventRecord(tr.ev[1], s);
  PickState* const pk = tr.pick.get();
  const bool pk_timing = pk && tr.timing && pk->ev[0];
  if (pk) {  // sets 1 and 2 of decoder.in: the branches' training forward on set 0, under this step's dropout masks
    if (pk_timing) (void)hipEventRecord(pk->ev[0], s);
    pick_forward(*pk, tr.opt.w.p, tr.din.p, tr.din.p, B, s, tr.launches);
    ++pk->step;  // (every step, update or not: two steps never share a mask)
    if (pk_timing) (void)hipEventRecord(pk->ev[1], s);
  }
  for (int i = 0; i < NSTAGE; ++i) forward_stage(tr, i, B);
  HeadArgs h{};
  h.a6 = tr.a[6].p, h.w = tr.opt.w.p, h.y = y_dev, h.logit = tr.logit.p, h.p = tr.pred.p, h.gz = tr.gzh.p, h.ga6 = tr.ga[6].p, h.gz6 = tr.gz[6].p;
  for (int d = 0; d < NSET; ++d) h.w_off[d] = tr.w_off[NSTAGE][d], h.b_off[d] = tr.b_off[NSTAGE][d], h.lw[d] = (float)lw[d];
  h.numel = (float)((double)B * T_OUT);
  h.B = B;
  const dim3 hgrid((T_OUT + 255) / 256, NSET * B);
  DTL(dec_head_kernel, hgrid, dim3(256), 0, s, h);
  {
    const int rc = bce_launch(tr.pred.p, y_dev, B, NSET, T_OUT, lw, nullptr, tr.loss_dev.p + 1, tr.loss_dev.p, s);
    if (rc != VP_OK) return rc;
  }
  if (tr.timing) (void)hipEventRecord(tr.ev[2], s);
  DTL(dec_head_dgrad_kernel, hgrid, dim3(256), 0, s, h);
  for (int i = NSTAGE - 1; i >= 1; --i) dgrad_stage(tr, i, B);
  if (pk) {
    if (pk_timing) (void)hipEventRecord(pk->ev[2], s);
    dgrad_stage(tr, 0, B);
    pick_backward(*pk, tr.opt.w.p, B, s, tr.launches);
    if (pk_timing) (void)hipEventRecord(pk->ev[3], s);
  }
  if (tr.timing) (void)hipEventRecord(tr.ev[3], s);
  launch_wgrad<1, HC, HK, false>(tr, NSTAGE, tr.gzh.p, tr.a[6].p, T_OUT, T_OUT, B);
  for (int i = NSTAGE - 1; i >= 0; --i) wgrad_stage(tr, i, B);
  if (pk) {
    if (pk_timing) (void)hipEventRecord(pk->ev[4], s);
    pick_wgrad(*pk, tr.din.p, tr.opt.grad.p, B, s, tr.launches);
    if (pk_timing) (void)hipEventRecord(pk->ev[5], s);
  }
  if (tr.timing) (void)hipEventRecord(tr.ev[4], s);
  if (update) tr.opt.update(s, lr, tr.launches);
  if (tr.timing) (void)hipEventRecord(tr.ev[5], s);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("vp_eqt_dec_train_step: kernel launch failed: %s", hipGetErrorString(e));
    return VP_ERR_HIP;
  }
  if (loss) {
    VP_HIP(hipMemcpyAsync(loss, tr.loss_dev.p, sizeof(double), hipMemcpyDeviceToHost, s));
    VP_HIP(hipStreamSynchronize(s));
  }
  return VP_OK;
}

int check_step(const DecTrainer& tr, const char* who, int B, const double* lw, float lr) {
  VP_REQUIRE(B >= 1 && B <= tr.max_batch, "%s: batch %d outside [1, %d]", who, B, tr.max_batch);
  VP_REQUIRE(lw != nullptr, "%s: loss_weights is null", who);
  VP_REQUIRE(std::isfinite(lw[0]) && std::isfinite(lw[1]) && std::isfinite(lw[2]), "%s: loss weights %g, %g, %g are not finite", who,
             lw[0], lw[1], lw[2]);
  VP_REQUIRE(std::isfinite(lr), "%s: learning rate %g is not finite", who, (double)lr);
  return VP_OK;
}

int step_bank(DecTrainer& tr, const Bank& bk, BatchRows rows, int B, float sigma, int norm, const int* label_rows, float det_fixed_window,
              const double* lw, float lr, int update, double* loss) {
  const char* who = rows.aug ? "vp_eqt_dec_train_step_bank_aug" : "vp_eqt_dec_train_step_bank";
  int rc = check_step(tr, who, B, lw, lr);
  if (rc != VP_OK) return rc;
  VP_REQUIRE(bk.device == tr.device, "%s: bank on device %d, trainer on device %d", who, bk.device, tr.device);
  BatchSpec spec;
  spec.T = T_OUT, spec.sigma = sigma, spec.norm = norm, spec.labels = LABEL_DET, spec.label_rows = label_rows;
  spec.det_fixed_window = det_fixed_window;
  if ((rc = bank_check(bk, spec, rows, B)) != VP_OK) return rc;
  VP_HIP(hipSetDevice(tr.device));
  if ((rc = tr.rows_ring.acquire(rows.bytes(B), (size_t)tr.max_batch * sizeof(vp_aug_row))) != VP_OK) return rc;
  const void* rd = tr.rows_ring.stage({{rows.p, rows.bytes(B)}}, tr.stream);
  if (!rd) return VP_ERR_HIP;
  if ((rc = bank_launch(bk, spec, rows.at(rd), B, tr.x_dev.p, tr.y_dev.p, tr.stream)) != VP_OK) return rc;
  if ((rc = tr.rows_ring.retire(tr.stream)) != VP_OK) return rc;
  return run_step(tr, tr.x_dev.p, tr.y_dev.p, B, lw, lr, update, loss);
}

}  // namespace
}  // namespace vp

using namespace vp;

extern "C" {

int vp_eqt_dec_train_param_count(void) { return (int)dec_params().size(); }
const char* vp_eqt_dec_train_param_name(int index) {
  static const std::vector<DecParam> table = dec_params();
  return (index >= 0 && index < (int)table.size()) ? table[index].name.c_str() : nullptr;
}
size_t vp_eqt_dec_train_param_size(int index) {
  static const std::vector<DecParam> table = dec_params();
  return (index >= 0 && index < (int)table.size()) ? table[index].size : 0;
}

int vp_eqt_dec_train_scope_param_count(int scope) { return scope_ok(scope) ? (int)dec_params(scope).size() : 0; }
const char* vp_eqt_dec_train_scope_param_name(int scope, int index) {
  static const std::vector<DecParam> table[2] = {dec_params(VP_EQT_TRAIN_DECODERS), dec_params(VP_EQT_TRAIN_PICK_BRANCHES)};
  return (scope_ok(scope) && index >= 0 && index < (int)table[scope].size()) ? table[scope][index].name.c_str() : nullptr;
}
size_t vp_eqt_dec_train_scope_param_size(int scope, int index) {
  static const std::vector<DecParam> table[2] = {dec_params(VP_EQT_TRAIN_DECODERS), dec_params(VP_EQT_TRAIN_PICK_BRANCHES)};
  return (scope_ok(scope) && index >= 0 && index < (int)table[scope].size()) ? table[scope][index].size : 0;
}
size_t vp_eqt_dec_train_scope_weight_count(int scope) {
  size_t n = 0;
  if (scope_ok(scope))
    for (const DecParam& p : dec_params(scope)) n += p.size;
  return n;
}

// what both constructors run; `who` is the entry that was called
static int create_trainer(const char* who, int device_id, const float* weights, size_t n_floats, const vp_config* cfg, int max_batch,
                          int scope, float drop_rate, uint64_t seed, vp_eqt_dec_trainer** out) {
  VP_REQUIRE(out && weights, "%s: null argument", who);
  VP_REQUIRE(scope_ok(scope), "%s: scope %d is neither VP_EQT_TRAIN_DECODERS nor VP_EQT_TRAIN_PICK_BRANCHES", who, scope);
  VP_REQUIRE(drop_rate >= 0.f && drop_rate < 1.f, "%s: drop_rate %g outside [0, 1)", who, (double)drop_rate);
  VP_REQUIRE(max_batch > 0 && max_batch <= 65535 / NSET, "%s: max_batch %d outside [1, %d]", who, max_batch, 65535 / NSET);
  if (n_floats == vp_weight_count(VP_MODEL_PHASENET)) {
    set_error("%s: a PhaseNet blob (%zu floats); PhaseNet trains through vp_train_create", who, n_floats);
    return VP_ERR_UNSUPPORTED;
  }
  VP_REQUIRE(n_floats == vp_weight_count(VP_MODEL_EQTRANSFORMER), "%s: expected %zu weight floats, got %zu", who,
             vp_weight_count(VP_MODEL_EQTRANSFORMER), n_floats);
  vp_config c;
  if (cfg) {
    c = *cfg;
  } else {
    vp_default_config(VP_MODEL_EQTRANSFORMER, &c);
  }
  for (int v : c.reserved) VP_REQUIRE(v == 0, "%s: vp_config.reserved must be zero", who);
  VP_HIP(hipSetDevice(device_id));
  auto tr = std::make_unique<DecTrainer>();
  tr->device = device_id;
  tr->max_batch = max_batch;
  tr->scope = scope;
  if (scope == VP_EQT_TRAIN_PICK_BRANCHES) {
    tr->pick = std::make_unique<PickState>();
    tr->pick->drop_rate = drop_rate, tr->pick->scale = 1.f / (1.f - drop_rate), tr->pick->seed = seed;
  }
  const int rc = build(*tr, weights, n_floats, c);
  if (rc != VP_OK) return rc;
  *out = reinterpret_cast<vp_eqt_dec_trainer*>(tr.release());
  return VP_OK;
}

int vp_eqt_dec_train_create(int device_id, const float* weights, size_t n_floats, const vp_config* cfg, int max_batch,
                            vp_eqt_dec_trainer** out) {
  return create_trainer("vp_eqt_dec_train_create", device_id, weights, n_floats, cfg, max_batch, VP_EQT_TRAIN_DECODERS, 0.f, 0, out);
}

int vp_eqt_dec_train_create_scope(int device_id, const float* weights, size_t n_floats, const vp_config* cfg, int max_batch, int scope,
                                  float drop_rate, uint64_t seed, vp_eqt_dec_trainer** out) {
  return create_trainer("vp_eqt_dec_train_create_scope", device_id, weights, n_floats, cfg, max_batch, scope, drop_rate, seed, out);
}

int vp_eqt_dec_train_destroy(vp_eqt_dec_trainer* h) {
  delete reinterpret_cast<DecTrainer*>(h);
  return VP_OK;
}

int vp_eqt_dec_train_set_hyper(vp_eqt_dec_trainer* h, float beta1, float beta2, float adam_eps) {
  VP_REQUIRE(h, "vp_eqt_dec_train_set_hyper: null handle");
  if (const int rc = check_hyper("vp_eqt_dec_train_set_hyper", beta1, beta2, adam_eps); rc != VP_OK) return rc;
  OptimState& opt = reinterpret_cast<DecTrainer*>(h)->opt;
  opt.beta1 = beta1, opt.beta2 = beta2, opt.adam_eps = adam_eps;
  return VP_OK;
}

int vp_eqt_dec_train_step(vp_eqt_dec_trainer* h, const float* x, const float* y, int mem, int B, const double* loss_weights, float lr,
                          int update, double* loss) {
  VP_REQUIRE(h && x && y, "vp_eqt_dec_train_step: null argument");
  VP_REQUIRE(mem == VP_MEM_HOST || mem == VP_MEM_DEVICE, "vp_eqt_dec_train_step: mem %d is neither VP_MEM_HOST nor VP_MEM_DEVICE", mem);
  DecTrainer& tr = *reinterpret_cast<DecTrainer*>(h);
  const int rc = check_step(tr, "vp_eqt_dec_train_step", B, loss_weights, lr);
  if (rc != VP_OK) return rc;
  VP_HIP(hipSetDevice(tr.device));
  const float *xd = x, *yd = y;
  if (mem == VP_MEM_HOST) {
    const size_t n = (size_t)B * 3 * T_OUT * sizeof(float);
    VP_HIP(hipMemcpyAsync(tr.x_dev.p, x, n, hipMemcpyHostToDevice, tr.stream));
    VP_HIP(hipMemcpyAsync(tr.y_dev.p, y, n, hipMemcpyHostToDevice, tr.stream));
    xd = tr.x_dev.p, yd = tr.y_dev.p;
  }
  return run_step(tr, xd, yd, B, loss_weights, lr, update, loss);
}

int vp_eqt_dec_train_step_bank(vp_eqt_dec_trainer* h, vp_bank* bank, const vp_plan_row* rows, int B, float sigma, int norm,
                               const int* label_rows, float det_fixed_window, const double* loss_weights, float lr, int update,
                               double* loss) {
  VP_REQUIRE(h && bank, "vp_eqt_dec_train_step_bank: null argument");
  return step_bank(*reinterpret_cast<DecTrainer*>(h), *reinterpret_cast<const Bank*>(bank), rows, B, sigma, norm, label_rows,
                   det_fixed_window, loss_weights, lr, update, loss);
}

int vp_eqt_dec_train_step_bank_aug(vp_eqt_dec_trainer* h, vp_bank* bank, const vp_aug_row* rows, int B, float sigma, int norm,
                                   const int* label_rows, float det_fixed_window, const double* loss_weights, float lr, int update,
                                   double* loss) {
  VP_REQUIRE(h && bank, "vp_eqt_dec_train_step_bank_aug: null argument");
  return step_bank(*reinterpret_cast<DecTrainer*>(h), *reinterpret_cast<const Bank*>(bank), rows, B, sigma, norm, label_rows,
                   det_fixed_window, loss_weights, lr, update, loss);
}

int vp_eqt_dec_train_synchronize(vp_eqt_dec_trainer* h) {
  VP_REQUIRE(h, "vp_eqt_dec_train_synchronize: null handle");
  DecTrainer& tr = *reinterpret_cast<DecTrainer*>(h);
  VP_HIP(hipSetDevice(tr.device));
  VP_HIP(hipStreamSynchronize(tr.stream));
  return VP_OK;
}

size_t vp_eqt_dec_train_weight_count(void) {
  size_t n = 0;
  for (const DecParam& p : dec_params()) n += p.size;
  return n;
}

int vp_eqt_dec_train_read(vp_eqt_dec_trainer* h, int which, float* out, size_t n_floats) {
  VP_REQUIRE(h && out, "vp_eqt_dec_train_read: null argument");
  DecTrainer& tr = *reinterpret_cast<DecTrainer*>(h);
  return tr.opt.read("vp_eqt_dec_train_read", tr.device, tr.stream, 3, which, out, n_floats);
}

int vp_eqt_dec_train_write_weights(vp_eqt_dec_trainer* h, const float* weights, size_t n_floats) {
  VP_REQUIRE(h && weights, "vp_eqt_dec_train_write_weights: null argument");
  DecTrainer& tr = *reinterpret_cast<DecTrainer*>(h);
  return tr.opt.write("vp_eqt_dec_train_write_weights", tr.device, tr.stream, weights, n_floats);
}

int vp_eqt_dec_train_tensor_count(const vp_eqt_dec_trainer* h) {
  return h ? (int)reinterpret_cast<const DecTrainer*>(h)->tensors.size() : VP_ERR_INVALID;
}
int vp_eqt_dec_train_tensor_info(const vp_eqt_dec_trainer* h, int index, const char** name, int* sets, int* channels, int* length) {
  VP_REQUIRE(h, "vp_eqt_dec_train_tensor_info: null handle");
  const DecTrainer& tr = *reinterpret_cast<const DecTrainer*>(h);
  VP_REQUIRE(index >= 0 && index < (int)tr.tensors.size(), "vp_eqt_dec_train_tensor_info: bad index");
  const DecTensor& t = tr.tensors[index];
  if (name) *name = t.name.c_str();
  if (sets) *sets = t.sets;
  if (channels) *channels = t.C;
  if (length) *length = t.L;
  return VP_OK;
}
int vp_eqt_dec_train_tensor_read(vp_eqt_dec_trainer* h, int index, int B, float* out) {
  VP_REQUIRE(h && out, "vp_eqt_dec_train_tensor_read: null argument");
  DecTrainer& tr = *reinterpret_cast<DecTrainer*>(h);
  VP_REQUIRE(index >= 0 && index < (int)tr.tensors.size() && B > 0 && B <= tr.max_batch, "vp_eqt_dec_train_tensor_read: bad argument");
  const DecTensor& t = tr.tensors[index];
  VP_HIP(hipSetDevice(tr.device));
  VP_HIP(hipStreamSynchronize(tr.stream));
  VP_HIP(hipMemcpy(out, t.p, (size_t)t.sets * B * t.C * t.L * sizeof(float), hipMemcpyDeviceToHost));
  return VP_OK;
}

int vp_eqt_dec_train_scope(const vp_eqt_dec_trainer* h) { return h ? reinterpret_cast<const DecTrainer*>(h)->scope : VP_ERR_INVALID; }
int vp_eqt_dec_train_launch_count(const vp_eqt_dec_trainer* h) { return h ? reinterpret_cast<const DecTrainer*>(h)->launches : 0; }
void* vp_eqt_dec_train_stream(const vp_eqt_dec_trainer* h) { return h ? reinterpret_cast<const DecTrainer*>(h)->stream : nullptr; }

int vp_eqt_dec_train_set_timing(vp_eqt_dec_trainer* h, int on) {
  VP_REQUIRE(h, "vp_eqt_dec_train_set_timing: null handle");
  DecTrainer& tr = *reinterpret_cast<DecTrainer*>(h);
  if (on && tr.pick && !tr.pick->ev[0]) {
    VP_HIP(hipSetDevice(tr.device));
    for (auto& e : tr.pick->ev) VP_HIP(hipEventCreate(&e));
  }
  tr.timing = on != 0;
  return VP_OK;
}
int vp_eqt_dec_train_pick_ms(vp_eqt_dec_trainer* h, float* ms) {
  VP_REQUIRE(h && ms, "vp_eqt_dec_train_pick_ms: null argument");
  DecTrainer& tr = *reinterpret_cast<DecTrainer*>(h);
  VP_REQUIRE(tr.pick, "vp_eqt_dec_train_pick_ms: the trainer's scope is VP_EQT_TRAIN_DECODERS");
  VP_REQUIRE(tr.timing && tr.pick->ev[0], "vp_eqt_dec_train_pick_ms: timing is off (vp_eqt_dec_train_set_timing)");
  VP_HIP(hipSetDevice(tr.device));
  VP_HIP(hipStreamSynchronize(tr.stream));
  for (int i = 0; i < 3; ++i) VP_HIP(hipEventElapsedTime(&ms[i], tr.pick->ev[2 * i], tr.pick->ev[2 * i + 1]));
  return VP_OK;
}
int vp_eqt_dec_train_phase_ms(vp_eqt_dec_trainer* h, float* ms) {
  VP_REQUIRE(h && ms, "vp_eqt_dec_train_phase_ms: null argument");
  DecTrainer& tr = *reinterpret_cast<DecTrainer*>(h);
  VP_REQUIRE(tr.timing, "vp_eqt_dec_train_phase_ms: timing is off (vp_eqt_dec_train_set_timing)");
  VP_HIP(hipSetDevice(tr.device));
  VP_HIP(hipStreamSynchronize(tr.stream));
  for (int i = 0; i < 5; ++i) VP_HIP(hipEventElapsedTime(&ms[i], tr.ev[i], tr.ev[i + 1]));
  return VP_OK;
}

}  // extern "C"
