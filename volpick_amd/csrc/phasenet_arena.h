// PhaseNet forward: what its kernel sources (phasenet_tiled.hip, phasenet_window.hip) and the planner
// (phasenet_fused.hip) share -- image strides, the LDS arena of the 13 core layers, the LDS / global row stores, the
// kernels' argument blocks and the launch functions through which the planner reaches the kernels of the other two files.
#pragma once
#include "conv_lds.h"
#include "conv_valu.h"
#include "net.h"

namespace vp {

constexpr int T0 = 3001, T1 = 751, T2 = 188, T3 = 47, T4 = 12;
constexpr int IB = 4;  // column of logical sample 0 in every LDS image

constexpr int img_stride(int L) { return ((4 + L + 20 - 16 + 31) / 32) * 32 + 16; }
constexpr int S1_ = img_stride(T1), S2_ = img_stride(T2), S3_ = img_stride(T3), S4_ = img_stride(T4);
static_assert(S1_ == 784 && S2_ == 240 && S3_ == 80 && S4_ == 48, "image strides");

template <int C, int S, int L, int B = IB>
__device__ __forceinline__ void zero_halo(float* img, int tid, int nth) {
  constexpr int RW = S - L;
  for (int i = tid; i < C * RW; i += nth) {
    const int c = i / RW, k = i - c * RW;
    img[c * S + (k < B ? k : L + k)] = 0.f;
  }
}

template <int S, int B>
struct RangeStore {  // LDS image store, valid t in [0, L)
  float* img;
  int L;
  __device__ __forceinline__ void operator()(int co, int t, float v) const {
    if ((unsigned)t < (unsigned)L) img[co * S + B + t] = v;
  }
  __device__ __forceinline__ bool all_valid(int t0, int t1) const { return t0 >= 0 && t1 < L; }
  __device__ __forceinline__ void unchecked(int co, int t, float v) const { img[co * S + B + t] = v; }
};

// The images written by the four-phase transposed convs of the core keep sample 0 at column TB = 5: with OUT_OFF = -1
// a lane's four consecutive outputs 4c - 1 .. 4c + 2 then start on a 16-byte boundary and leave as one ds_write_b128.
constexpr int TB = 5;
template <int S, int B>
struct RangeStoreS : RangeStore<S, B> {};
template <int S, int B>
struct RangeStoreV : RangeStore<S, B> {
  __device__ __forceinline__ void vec4(int co, int t, f32x4 v) const { *reinterpret_cast<f32x4*>(this->img + co * S + B + t) = v; }
};

struct GlobalRowStore {  // haloed activation tensor row store with a valid range
  float* p;              // window base + HALO
  int ls, L, t_add;      // global t = t_local + t_add
  __device__ __forceinline__ void operator()(int co, int t, float v) const {
    const int tg = t + t_add;
    if (t >= 0 && tg >= 0 && tg < L) p[(long)co * ls + tg] = v;
  }
  __device__ __forceinline__ bool all_valid(int t0, int t1) const { return t0 >= 0 && t0 + t_add >= 0 && t1 + t_add < L; }
  __device__ __forceinline__ void unchecked(int co, int t, float v) const { p[(long)co * ls + t + t_add] = v; }
};

// The 13 core layers (levels 1-4 down, up0 .. up2): one 1024-thread workgroup (16 waves) per window.
using C_d1same = LdsLayer<8, 0, 16, 1, 7, 1, -3, 0, 6, 1>;
using C_d1down = LdsLayer<16, 0, 16, 1, 7, 4, -2, 0, 3, 1>;
using C_d2same = LdsLayer<16, 0, 32, 1, 7, 1, -3, 0, 3, 1>;
using C_d2down = LdsLayer<32, 0, 32, 1, 7, 4, -1, 0, 1, 1>;
using C_d3same = LdsLayer<32, 0, 64, 1, 7, 1, -3, 0, 3, 1>;
using C_d3down = LdsLayer<64, 0, 64, 1, 7, 4, -2, 0, 1, 1>;
using C_d4same = LdsLayer<64, 0, 128, 1, 7, 1, -3, 0, 1, 1>;
using C_u0T = LdsLayer<128, 0, 64, 4, 2, 1, -1, -1, 1, 1>;
using C_u0same = LdsLayer<64, 64, 64, 1, 7, 1, -3, 0, 3, 1>;
using C_u1T = LdsLayer<64, 0, 32, 4, 2, 1, -1, -1, 3, 1>;
using C_u1same = LdsLayer<32, 32, 32, 1, 7, 1, -3, 0, 6, 1>;
using C_u2T = LdsLayer<32, 0, 16, 4, 2, 1, -1, -1, 3, 1>;
using C_u2same = LdsLayer<16, 16, 16, 1, 7, 1, -3, 0, 6, 1>;

// layers with at least this many n-tiles per item read their B fragments tap by tap instead of double-buffering a
// whole channel block of them (register budget of a 1024-thread workgroup: 128 per wave)
constexpr int BDB_MAX_NB = 6;

// LDS arena (floats); lifetimes in the header comment of pn_core_kernel
constexpr int A_SKIP1 = 0;                       // 16 x 784
constexpr int A_SKIP2 = A_SKIP1 + 16 * S1_;      // 32 x 240
constexpr int A_Q = A_SKIP2 + 32 * S2_;          // scratch region Q
constexpr int A_SKIP3 = A_Q;                     // 64 x 80
constexpr int A_R = A_Q + 64 * S3_;
constexpr int A_D0 = A_R;                        // 8 x 784
constexpr int A_D1 = A_R;                        // 16 x 240
constexpr int A_D2 = A_R;                        // 32 x 80
constexpr int A_D3 = A_R;                        // 64 x 48
constexpr int A_BOT = A_R + 64 * S4_;            // 128 x 48
constexpr int A_U0T = A_BOT + 128 * S4_;         // 64 x 80
constexpr int A_U0S = A_R;                       // 64 x 80
constexpr int A_U1T = A_U0S + 64 * S3_;          // 32 x 240
constexpr int A_U1S = A_Q;                       // 32 x 240
constexpr int A_U2T = A_U1S + 32 * S2_;          // 16 x 784
constexpr int CORE_LDS_FLOATS = A_U2T + 16 * S1_;
static_assert(A_U0T + 64 * S3_ <= CORE_LDS_FLOATS && A_U1T + 32 * S2_ <= CORE_LDS_FLOATS, "arena overflow");
static_assert(CORE_LDS_FLOATS * 4 <= 160 * 1024, "core arena must fit the 160 KiB LDS");

struct CoreArgs {
  const float* d0;  // [B][8][ls]   (down0.down)
  int ls_d0;
  long ws_d0;
  float* u2s;       // [B][16][ls]  (up2.same)
  int ls_u2s;
  long ws_u2s;
  const float* af[13];
  const float* bs[13];
  // optional debug dumps of every intermediate (null = off): order skip1,d1,skip2,d2,skip3,d3,bottom,u0T,u0s,u1T,u1s,u2T
  float* dbg[12];
  int dbg_ls[12];
  long dbg_ws[12];
  unsigned long long* clk;  // optional [B][32]: [0..14] shader-clock stamps (start, load, 13 layers), [16],[17] 100 MHz wall clock
  int warm;                 // 1: the first workgroup of each XCD pre-touches the weights (pn_core_kernel: every launch -- the
                            // level-0 launches of the three-launch plan run in between; pn_window_kernel: a plan's first launch)
};

// ---- the time-tiled level-0 kernels of the three-launch plans (phasenet_tiled.hip) ----
constexpr int TT = 512;                   // level-0 samples per tile
constexpr int N_TILES = (T0 + TT - 1) / TT;     // 6
constexpr int VT = 1024, VS = VT + 8;           // lanes x 4 samples; image row stride (local l at column l + 4)
constexpr int VD_TS = 1008, VD_TILES = (T0 + VD_TS - 1) / VD_TS;  // down0: local 0 <-> global VD_TS * tile - 8
constexpr int VU_TS = 1016, VU_TILES = (T0 + VU_TS - 1) / VU_TS;  // up3:   local 0 <-> global VU_TS * tile - 4

struct Down0Args {
  const float* x;   // [B][3][ls] normalised input
  int ls_x;
  long ws_x;
  float* skip0;     // [B][8][ls]  (down0.same)
  int ls_s;
  long ws_s;
  float* d0;        // [B][8][ls]  (down0.down)
  int ls_d;
  long ws_d;
  float* h0_dbg;    // optional [B][8][ls] (inc)
  int ls_h;
  long ws_h;
  const float *af_inc, *bs_inc, *af_same, *bs_same, *af_down, *bs_down;
};

struct Up3Args {
  const float* u2s;    // [B][16][ls] (up2.same)
  int ls_u;
  long ws_u;
  const float* skip0;  // [B][8][ls]
  int ls_s;
  long ws_s;
  float* y;            // dense [B][3][T0]
  float* ut_dbg;       // optional [B][8][ls] (up3.convT)
  int ls_t;
  long ws_t;
  const float *af_t, *bs_t, *af_same, *bs_same;
  const float* w_out;  // [3][8]
  const float* b_out;  // [3]
  unsigned long long* clk;  // optional debug stamps (tile 2 of each window): slots 18..23 of the core's [B][32] block
};

struct Down0VArgs {
  Down0Args t;  // tensors as in the MFMA form (af_* / bs_* unused)
  const f32x2 *w_inc, *b_inc, *w_same, *b_same, *w_down, *b_down;  // [cin][7][4] channel pairs, [4] bias pairs
  int n_windows;
};

struct Up3VArgs {
  Up3Args t;  // tensors as in the MFMA form
  const f32x2 *w_t, *b_t, *w_same, *b_same;  // up3.convT [16][7][4], up3.same [16][7][4] (skip channels first)
  int n_windows;
};

// relu + zero outside the signal, channel pair c of acc -> two float4 rows
template <int NC>
__device__ __forceinline__ void valu_finish(const f32x2 (&acc)[NC][4], int c, int tg, f32x4* lo, f32x4* hi) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const bool in = (unsigned)(tg + r) < (unsigned)T0;
    (*lo)[r] = in ? fmaxf(acc[c][r].x, 0.f) : 0.f;
    (*hi)[r] = in ? fmaxf(acc[c][r].y, 0.f) : 0.f;
  }
}
template <int NC>
__device__ __forceinline__ void valu_bias(f32x2 (&acc)[NC][4], const f32x2* b) {
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[c][r] = as_weights(b)[c];
}

// ---- the whole network in one launch (phasenet_window.hip) ----
constexpr int W0_S = 3024;                 // level-0 image row stride: sample t at column t + 4, t in [-4, 3020); == 16 mod 32
constexpr int D0T_TILES = 6, U3T_TILES = 12;  // tiles of the time-tiled level-0 down / up path
constexpr bool q4_layer_index(int i) { return (i >= 1 && i <= 9) || i == 11; }  // d1down .. up0.same, and the two register-resident two-tap layers
// the layers a DUMP instance of pn_window_kernel writes out (WindowArgs::dbg), in the order of WD_NAMES
enum WinDump { WD_INC, WD_D0DOWN, WD_D1SAME, WD_D1DOWN, WD_D2SAME, WD_D2DOWN, WD_D3SAME, WD_D3DOWN, WD_D4SAME, WD_U0T, WD_U0SAME,
               WD_U1T, WD_U1SAME, WD_U2T, WD_U2SAME, WD_U3T, WD_U3SAME, WD_LOGITS, WD_COUNT };
const char* const WD_NAMES[WD_COUNT] = {"inc",        "down0.down", "down1.same", "down1.down", "down2.same", "down2.down",
                                        "down3.same", "down3.down", "down4.same", "up0.convT",  "up0.same",   "up1.convT",
                                        "up1.same",   "up2.convT",  "up2.same",   "up3.convT",  "up3.same",   "logits"};
struct WindowArgs {
  CoreArgs c;       // d0 / u2s unused (they live in LDS)
  const float* af4[13];  // weights of the core layers regrouped for 16-byte loads (conv_lds_q4), null where unused
  const uint4* af3[6];   // down3.same .. up0.same, up1.same as three-piece bf16 operands (conv_b3.h); every af3* is null in the Fp32Core form
  int af3_lines[6];      // their sizes in 128-byte lines (L2 warm-up)
  const uint4* af3_u2[2];  // up2.same's operand per input half (skip 1 | up2.convT), 16-channel K-steps (B3Steps<16, 7>)
  const uint4* af3_uT[2];  // up1.convT / up2.convT, rows (phase, channel)
  const uint4* af3_d12[2]; // down1.same (B3Steps<8, 7>), down2.same (B3Steps<16, 7>)
  const uint4* af3_inc;    // Default form only: inc, rows (phase, channel), ONE K-step of eight taps x four channels (three + a zero one)
  const uint4* af3_d0s;    // Default form only: down0.same, rows (phase, channel), two K-steps of four taps x eight channels (B3Steps<8, 8>)
  const float *bs_inc8, *bs_d0s;  // their biases [8] (BatchNorm folded)
  const uint4* af3_u3t;    // Default form only: up3.convT, rows (phase, channel), ONE K-step of two taps x 16 channels (B3Steps<16, 2>), two m-tiles
  const uint4* af3_u3s;    // Default form only: up3.same, rows (phase, channel), four K-steps of two taps x 16 channels (skip 0 | up3.convT) (B3Steps<16, 8>)
  const float *bs_u3t, *bs_u3s;  // their biases [8]
  const float* x;   // [B][3][ls] normalised input
  int ls_x;
  long ws_x;
  float* skip0;     // [B][8][ls] (down0.same): written in the down phase, read back in the up phase
  int ls_s;
  long ws_s;
  float* y;         // dense [B][3][T0]
  const f32x2 *w_inc, *b_inc, *w_same, *b_same, *w_up, *b_up;  // VALU weights: [cin][7][4] channel pairs, [4] bias pairs
  const float *af_down, *bs_down, *af_t, *bs_t;                // MFMA fragments of down0.down and up3.convT
  const float *w_out, *b_out;                                  // 1x1 output conv
  PreArgs pre;                                                 // has_pre: the kernel cuts and normalises its window itself
  int has_pre;                                                 // (annotate_batch_pre, as gather_normalize_kernel); else it reads x
  // DUMP instances only (plan_flags[1] & 4, tests/test_gpu_layers_f64.py): every layer's output, as the epilogue computed it in fp32,
  // into the haloed debug tensors of the layer plan (down0.same needs none: it is the skip tensor).  Last in the struct, so that the
  // kernel arguments of the default instances keep their offsets.
  float* dbg[WD_COUNT];
  int dbg_ls[WD_COUNT];
  long dbg_ws[WD_COUNT];
};

// The forms of pn_window_kernel (plan_flags[5] = 0 | 8 | 3).
enum class PnForm {
  Default,     // every layer but the strided convs on the bf16 matrix cores with exact three-piece operands, level 0 time-tiled
  Level0Valu,  // level 0 on the vector ALUs (and the fp32 MFMA): the rounding reference of the tiled level-0 layers
  Fp32Core,    // that, and every core layer on the fp32 MFMA: the reference of the bf16-piece layers
};

// Launches, one per kernel family; pn_register_* enter the kernels into Net::extra_kernels (dynamic LDS attribute).
void pn_launch_down0(const Down0Args& a, int B, hipStream_t s);
void pn_launch_down0v(const Down0VArgs& a, int B, hipStream_t s);
void pn_launch_core(const CoreArgs& a, int B, hipStream_t s);
void pn_launch_up3(const Up3Args& a, int B, bool persistent, hipStream_t s);  // persistent: two workgroups per window walk the tiles
void pn_launch_up3v(const Up3VArgs& a, int B, hipStream_t s);
void pn_register_tiled(Net& net);
void pn_launch_window(PnForm form, bool dump, const WindowArgs& a, int B, hipStream_t s);  // dump: the DUMP instance (Default only)
void pn_register_window(Net& net, bool dump);

}  // namespace vp
