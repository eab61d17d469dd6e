// PhaseNet forward in three launches: the plans that came before the one-launch kernel (phasenet_window.hip), kept as
// references -- of tests/test_gpu_phasenet.py::test_fused_equals_layerwise_bitwise (plan_flags[5] = 1: all MFMA,
// bit-identical to the layer plan), of the debug-dump plans (plan_flags[1] & 1) and of the A/B forms plan_flags[5] = 1 | 2.
//
//   pn_down0v_kernel / pn_down0_kernel   inc -> down0.same -> down0.down, time-tiled (stride-1 convs on the VALU /
//                    all MFMA); only the skip tensor (down0.same) and the 751-sample down0.down rows go to memory.
//   pn_core_kernel   ONE workgroup per window: levels 1-4 down and up0..up2 (13 layers, 71 % of the
//                    model's FLOPs) run back to back out of a 158 KB LDS arena.
//   pn_up3v_kernel / pn_up3p_kernel      up3.convT -> concat(skip0) -> up3.same -> 1x1 conv + softmax, time-tiled.
//
// The MFMA layers are conv_lds<> (conv_lds.h): LDS image -> MFMA -> LDS image; the 8-channel stride-1 layers of
// level 0 are direct convolutions on the VALU (conv_valu.h).  Coordinates inside a tiled kernel are local to the
// tile; ImageStore writes explicit zeros where the global position falls outside the signal so that the next layer
// sees the reference's zero padding.
#include "phasenet_arena.h"

namespace vp {

namespace {

template <int C, int S, int B = IB>
__device__ void dump_image(const float* img, int L, float* dst, int ls, long ws, int win, int tid, int nth) {
  if (!dst) return;
  float* d = dst + (long)win * ws + HALO;
  for (int i = tid; i < C * L; i += nth) {
    const int c = i / L, t = i - c * L;
    d[(long)c * ls + t] = img[c * S + B + t];
  }
}

__global__ __launch_bounds__(1024) void pn_core_kernel(const CoreArgs a) {
  extern __shared__ float4 lds_raw[];
  float* lds = reinterpret_cast<float*>(lds_raw);
  // (the wave index as a scalar: item loops, block indices and the epilogues' "whole block in range" tests become
  // scalar code instead of per-lane predicates)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), win = blockIdx.x;
  constexpr int NTH = 1024, NWV = 16;
  int stamp = 0;
  if (a.clk && tid == 0) a.clk[(long)win * 32 + 16] = wall_clock64();  // 100 MHz constant clock
#define CORE_STAMP()                                                              \
  if (a.clk && tid == 0) a.clk[(long)win * 32 + stamp] = __builtin_readcyclecounter(); \
  ++stamp;
  CORE_STAMP()

  // The first workgroup of each XCD (consecutive workgroups go to consecutive XCDs) touches one word of every
  // 128-byte line of the 1.06 MB of packed weights: kernels of the other contexts have pushed them out of L2 since
  // the last launch, and the layer chain below would otherwise meet the misses one channel block at a time.
  if (win < 8 && a.warm) {
    float sink = 0.f;
#define CORE_WARM(IDX, LAYER)                                                                          \
  for (int l = tid; l < LAYER::MT * LAYER::CB * LAYER::TAPS * 2; l += NTH) sink += a.af[IDX][l * 32];
    CORE_WARM(0, C_d1same) CORE_WARM(1, C_d1down) CORE_WARM(2, C_d2same) CORE_WARM(3, C_d2down) CORE_WARM(4, C_d3same)
    CORE_WARM(5, C_d3down) CORE_WARM(6, C_d4same) CORE_WARM(7, C_u0T) CORE_WARM(8, C_u0same) CORE_WARM(9, C_u1T)
    CORE_WARM(10, C_u1same) CORE_WARM(11, C_u2T) CORE_WARM(12, C_u2same)
#undef CORE_WARM
    if (sink == 1.2345678e-30f) a.u2s[0] = sink;  // never true: keeps the loads alive
  }

  // ---- load down0.down (8 x 751) -------------------------------------------------------
  {
    const float* src = a.d0 + (long)win * a.ws_d0 + HALO;
    float* img = lds + A_D0;
    for (int i = tid; i < 8 * T1; i += NTH) {
      const int c = i / T1, t = i - c * T1;
      img[c * S1_ + IB + t] = src[(long)c * a.ls_d0 + t];
    }
    zero_halo<8, S1_, T1>(img, tid, NTH);
  }
  __syncthreads();
  CORE_STAMP()

#define CORE_LAYER(IDX, LAYER, IN1, SI1, IN2, SI2, B2, OUT, SO, OB, STORE, CO, COLS, LOUT, DBG)                    \
  {                                                                                                                \
    STORE<SO, OB> st{{lds + (OUT), (LOUT)}};                                                                      \
    zero_halo<CO, SO, LOUT, OB>(lds + (OUT), tid, NTH);                                                          \
    conv_lds<LAYER, SI1, IB, SI2, B2, false, (LAYER::NB < BDB_MAX_NB)>(lds + (IN1), lds + (IN2), a.af[IDX], a.bs[IDX], (COLS), st, wave, NWV, lane); \
    __syncthreads();                                                                                               \
    CORE_STAMP()                                                                                                   \
    if (a.dbg[DBG]) dump_image<CO, SO, OB>(lds + (OUT), (LOUT), a.dbg[DBG], a.dbg_ls[DBG], a.dbg_ws[DBG], win, tid, NTH); \
  }
#define CORE_LAYER_AREG(IDX, LAYER, IN1, SI1, OUT, SO, OB, STORE, CO, COLS, LOUT, WMT, WFIRST, WSTEP, DBG)                    \
  {                                                                                                                \
    STORE<SO, OB> st{{lds + (OUT), (LOUT)}};                                                                      \
    zero_halo<CO, SO, LOUT, OB>(lds + (OUT), tid, NTH);                                                          \
    if ((WMT) < LAYER::MT && (WFIRST) < ((((COLS) + 15) >> 4) + LAYER::NB - 1) / LAYER::NB) {                    \
      float ar[LAYER::CB * LAYER::TAPS], br[4];                                                                    \
      load_areg<LAYER>(a.af[IDX], (WMT), lane, ar);                                                                \
      load_biasreg<LAYER>(a.bs[IDX], (WMT), lane, br);                                                             \
      conv_lds_areg<LAYER, SI1, IB, SI1, IB>(lds + (IN1), lds + (IN1), ar, br, (WMT), (COLS), st, (WFIRST), (WSTEP), lane); \
    }                                                                                                              \
    __syncthreads();                                                                                               \
    CORE_STAMP()                                                                                                   \
    if (a.dbg[DBG]) dump_image<CO, SO, OB>(lds + (OUT), (LOUT), a.dbg[DBG], a.dbg_ls[DBG], a.dbg_ws[DBG], win, tid, NTH); \
  }
  //          idx layer      in1      S    in2      S    b2  out      S    ob  store        C    cols     Lout dbg
  CORE_LAYER(0, C_d1same, A_D0, S1_, A_D0, S1_, IB, A_SKIP1, S1_, IB, RangeStoreS, 16, T1, T1, 0)
  CORE_LAYER(1, C_d1down, A_SKIP1, S1_, A_SKIP1, S1_, IB, A_D1, S2_, IB, RangeStoreS, 16, T2, T2, 1)
  CORE_LAYER(2, C_d2same, A_D1, S2_, A_D1, S2_, IB, A_SKIP2, S2_, IB, RangeStoreS, 32, T2, T2, 2)
  CORE_LAYER(3, C_d2down, A_SKIP2, S2_, A_SKIP2, S2_, IB, A_D2, S3_, IB, RangeStoreS, 32, T3, T3, 3)
  CORE_LAYER(4, C_d3same, A_D2, S3_, A_D2, S3_, IB, A_SKIP3, S3_, IB, RangeStoreS, 64, T3, T3, 4)
  CORE_LAYER(5, C_d3down, A_SKIP3, S3_, A_SKIP3, S3_, IB, A_D3, S4_, IB, RangeStoreS, 64, T4, T4, 5)
  CORE_LAYER(6, C_d4same, A_D3, S4_, A_D3, S4_, IB, A_BOT, S4_, IB, RangeStoreS, 128, T4, T4, 6)
  CORE_LAYER(7, C_u0T, A_BOT, S4_, A_BOT, S4_, IB, A_U0T, S3_, TB, RangeStoreV, 64, T4 + 1, T3, 7)
  CORE_LAYER(8, C_u0same, A_SKIP3, S3_, A_U0T, S3_, TB, A_U0S, S3_, IB, RangeStoreS, 64, T3, T3, 8)
  // Two-tap layers with few items: the wave's whole A operand (16-32 fragments) is fetched up front — two fragments per
  // channel block in flight (the double buffer of conv_lds) left these layers waiting on L2 at every block.
  CORE_LAYER_AREG(9, C_u1T, A_U0S, S3_, A_U1T, S2_, TB, RangeStoreV, 32, T3 + 1, T2, wave, 0, 1, 9)        // 8 m-tiles x 1 block
  CORE_LAYER(10, C_u1same, A_SKIP2, S2_, A_U1T, S2_, TB, A_U1S, S2_, IB, RangeStoreS, 32, T2, T2, 10)
  CORE_LAYER_AREG(11, C_u2T, A_U1S, S2_, A_U2T, S1_, TB, RangeStoreV, 16, T2 + 1, T1, wave & 3, wave >> 2, 4, 11)  // 4 m-tiles x 4 blocks
#undef CORE_LAYER_AREG
#undef CORE_LAYER
  {
    GlobalRowStore st{a.u2s + (long)win * a.ws_u2s + HALO, a.ls_u2s, T1, 0};
    conv_lds<C_u2same, S1_, IB, S1_, TB, false, (C_u2same::NB < BDB_MAX_NB)>(lds + A_SKIP1, lds + A_U2T, a.af[12], a.bs[12], T1, st, wave, NWV, lane);
  }
  __syncthreads();
  CORE_STAMP()
  if (a.clk && tid == 0) a.clk[(long)win * 32 + 17] = wall_clock64();
#undef CORE_STAMP
}

// ---------------------------------------------------------------------------------------------
// Level-0 down path, time-tiled: inc -> down0.same -> down0.down.
// Local coordinate l <-> global level-0 sample (t0 - 12) + l, t0 = tile * TT.
// ---------------------------------------------------------------------------------------------
constexpr int D0_S = 560;                 // image stride (== 16 mod 32), covers local [-4, 556)
using D_inc = LdsLayer<3, 0, 8, 2, 8, 2, -3, 0, 5, 1>;
using D_same = LdsLayer<8, 0, 8, 2, 8, 2, -3, 0, 5, 1>;
using D_down = LdsLayer<8, 0, 8, 2, 11, 8, 9, 0, 1, 1>;  // reads skip0 local 8n + tap + 9 (= global 8(c0+n) + tap - 3)
constexpr int D0_X = 0, D0_H = 4 * D0_S, D0_K = 12 * D0_S, D0_LDS_FLOATS = 20 * D0_S;

__global__ __launch_bounds__(256) void pn_down0_kernel(const Down0Args a) {
  extern __shared__ float4 lds_raw[];
  float* lds = reinterpret_cast<float*>(lds_raw);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x, win = blockIdx.y;
  const int t0 = tile * TT, o = t0 - 12;
  constexpr int NTH = 256, NWV = 4;

  // x image: local [-4, TT + 24) as float4s; physical index = HALO + o - 4 + 4q = t0 - 8 + 4q
  {
    const float* src = a.x + (long)win * a.ws_x;
    constexpr int NQ = (TT + 28) / 4;  // 135 float4 per row
    for (int i = tid; i < 3 * NQ; i += NTH) {
      const int c = i / NQ, q = i - c * NQ;
      const int p = t0 - 8 + 4 * q;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (p >= 0 && p + 3 < a.ls_x) v = *reinterpret_cast<const float4*>(src + (long)c * a.ls_x + p);
      *reinterpret_cast<float4*>(lds + D0_X + c * D0_S + 4 * q) = v;
    }
    for (int i = tid; i < D0_S / 4; i += NTH)  // 4th (padding) channel must be true zeros
      *reinterpret_cast<float4*>(lds + D0_X + 3 * D0_S + 4 * i) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();
  const int sig_lo = -o, sig_hi = T0 - o;
  {
    ImageStore<D0_S, IB> st{lds + D0_H, 0, TT + 16, sig_lo, sig_hi};
    conv_lds<D_inc, D0_S, IB, D0_S, IB, false>(lds + D0_X, lds + D0_X, a.af_inc, a.bs_inc, (TT + 16) / 2, st, wave, NWV, lane);
  }
  __syncthreads();
  if (a.h0_dbg) {
    float* d = a.h0_dbg + (long)win * a.ws_h + HALO;
    for (int i = tid; i < 8 * TT; i += NTH) {
      const int c = i / TT, l = 12 + (i - c * TT);
      if (o + l < T0) d[(long)c * a.ls_h + o + l] = lds[D0_H + c * D0_S + IB + l];
    }
  }
  {
    ImageStore<D0_S, IB> st{lds + D0_K, 0, TT + 16, sig_lo, sig_hi};
    conv_lds<D_same, D0_S, IB, D0_S, IB, false>(lds + D0_H, lds + D0_H, a.af_same, a.bs_same, (TT + 16) / 2, st, wave, NWV, lane);
  }
  __syncthreads();
  {  // skip tensor rows [t0, t0 + TT) -> memory, 16-byte coalesced (local 12 <-> column 16)
    float* d = a.skip0 + (long)win * a.ws_s + HALO + t0;
    for (int i = tid; i < 8 * (TT / 4); i += NTH) {
      const int c = i / (TT / 4), q = i - c * (TT / 4);
      const int t = t0 + 4 * q;
      if (t < T0) {
        float4 v = *reinterpret_cast<const float4*>(lds + D0_K + c * D0_S + IB + 12 + 4 * q);  // zeros beyond the signal
        *reinterpret_cast<float4*>(d + (long)c * a.ls_s + 4 * q) = v;
      }
    }
  }
  {
    GlobalRowStore st{a.d0 + (long)win * a.ws_d + HALO, a.ls_d, T1, tile * (TT / 4)};
    conv_lds<D_down, D0_S, IB, D0_S, IB, false>(lds + D0_K, lds + D0_K, a.af_down, a.bs_down, TT / 8, st, wave, NWV, lane);
  }
}

// ---------------------------------------------------------------------------------------------
// Level-0 up path, time-tiled: up3.convT -> cat(skip0, .) -> up3.same -> 1x1 conv + softmax.
// Level-1 local n <-> global (t0/4 - 4) + n; level-0 local l <-> global (t0 - 16) + l.
// ---------------------------------------------------------------------------------------------
constexpr int U_S1 = 176;                 // u2s image stride: local1 [-4, 172)
constexpr int U_S0 = 592;                 // level-0 image stride: local0 [-4, 588)
constexpr int U_SO = 516;                 // staged up3.same tile
using U_T = LdsLayer<16, 0, 8, 4, 2, 1, -1, -2, 5, 1>;
using U_same = LdsLayer<8, 8, 8, 2, 8, 2, 13, 0, 4, 1>;  // out local'' 2n+p <-> level-0 local 16 + 2n + p
constexpr int U_U2S = 0, U_SKIP = 16 * U_S1, U_UT = U_SKIP + 8 * U_S0, U_OUT = U_UT + 8 * U_S0;
constexpr int UP3_LDS_FLOATS = U_OUT + 8 * U_SO;

__global__ __launch_bounds__(256) void pn_up3_kernel(const Up3Args a) {
  extern __shared__ float4 lds_raw[];
  float* lds = reinterpret_cast<float*>(lds_raw);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x, win = blockIdx.y;
  const int t0 = tile * TT, o1 = t0 / 4 - 4, o0 = t0 - 16;
  constexpr int NTH = 256, NWV = 4;
  int stamp = 18;
#define UP3_STAMP()                                                                                   \
  if (a.clk && tid == 0 && tile == 2) a.clk[(long)win * 32 + stamp] = __builtin_readcyclecounter(); \
  ++stamp;
  UP3_STAMP()

  {  // up2.same rows: local1 [0, 144); physical = HALO + o1 + 4q
    const float* src = a.u2s + (long)win * a.ws_u + HALO + o1;
    for (int i = tid; i < 16 * 36; i += NTH) {
      const int c = i / 36, q = i - c * 36;
      *reinterpret_cast<float4*>(lds + U_U2S + c * U_S1 + IB + 4 * q) =
          *reinterpret_cast<const float4*>(src + (long)c * a.ls_u + 4 * q);
    }
    if (tid < 16) *reinterpret_cast<float4*>(lds + U_U2S + tid * U_S1) = make_float4(0.f, 0.f, 0.f, 0.f);  // local1 -4..-1
  }
  {  // skip rows: local0 [12, 532); physical = HALO + o0 + 12 + 4q = t0 + 4 + 4q
    const float* src = a.skip0 + (long)win * a.ws_s + HALO + o0 + 12;
    for (int i = tid; i < 8 * 130; i += NTH) {
      const int c = i / 130, q = i - c * 130;
      *reinterpret_cast<float4*>(lds + U_SKIP + c * U_S0 + IB + 12 + 4 * q) =
          *reinterpret_cast<const float4*>(src + (long)c * a.ls_s + 4 * q);
    }
  }
  __syncthreads();
  UP3_STAMP()
  {
    ImageStore<U_S0, IB> st{lds + U_UT, 0, U_S0 - IB, -o0, T0 - o0};
    conv_lds<U_T, U_S1, IB, U_S1, IB, false>(lds + U_U2S, lds + U_U2S, a.af_t, a.bs_t, 144, st, wave, NWV, lane);
  }
  __syncthreads();
  UP3_STAMP()
  if (a.ut_dbg) {
    float* d = a.ut_dbg + (long)win * a.ws_t + HALO;
    for (int i = tid; i < 8 * TT; i += NTH) {
      const int c = i / TT, l = 16 + (i - c * TT);
      if (o0 + l < T0) d[(long)c * a.ls_t + o0 + l] = lds[U_UT + c * U_S0 + IB + l];
    }
  }
  {
    ImageStore<U_SO, 0> st{lds + U_OUT, 0, TT, 0, TT};
    conv_lds<U_same, U_S0, IB, U_S0, IB, false>(lds + U_SKIP, lds + U_UT, a.af_same, a.bs_same, TT / 2, st, wave, NWV, lane);
  }
  __syncthreads();
  UP3_STAMP()
  {  // 1x1 conv (8 -> 3) + softmax over channels, dense output
    float w[3][8], bb[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      bb[c] = a.b_out[c];
#pragma unroll
      for (int k = 0; k < 8; ++k) w[c][k] = a.w_out[c * 8 + k];
    }
    float* y = a.y + (long)win * 3 * T0;
    for (int l = tid; l < TT; l += NTH) {
      const int t = t0 + l;
      if (t < T0) {
        float z[3] = {bb[0], bb[1], bb[2]};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float v = lds[U_OUT + k * U_SO + l];
#pragma unroll
          for (int c = 0; c < 3; ++c) z[c] = fmaf(w[c][k], v, z[c]);
        }
        const float mx = fmaxf(z[0], fmaxf(z[1], z[2]));
        const float e0 = __expf(z[0] - mx), e1 = __expf(z[1] - mx), e2 = __expf(z[2] - mx);
        const float inv = 1.f / (e0 + e1 + e2);
        y[t] = e0 * inv;
        y[T0 + t] = e1 * inv;
        y[2 * T0 + t] = e2 * inv;
      }
    }
  }
  __syncthreads();
  UP3_STAMP()
#undef UP3_STAMP
}

// ---------------------------------------------------------------------------------------------
// Persistent forms of the two tiled kernels.  One workgroup walks TPS consecutive tiles of a window:
// the A fragments of its waves' m-tiles are loaded ONCE into registers (the layers here have K of
// only 8-32 steps, so an exposed L2 round trip per tile costs as much as the MFMAs), and the next
// tile's input rows are fetched into registers while the current tile computes.
// ---------------------------------------------------------------------------------------------
constexpr int NSPLIT_U = 2, TPS_U = (N_TILES + NSPLIT_U - 1) / NSPLIT_U;  // up3:   66 KB LDS -> 2 workgroups / CU

// (pn_down0p_kernel, the persistent form of the level-0 down kernel -- plan_flags[3] = 2, measured 4-15 % slower than one workgroup
// per tile -- was removed in round 6.)

__global__ __launch_bounds__(256) void pn_up3p_kernel(const Up3Args a) {
  extern __shared__ float4 lds_raw[];
  float* lds = reinterpret_cast<float*>(lds_raw);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int win = blockIdx.y;
  const int tile_lo = blockIdx.x * TPS_U, tile_hi = (tile_lo + TPS_U < N_TILES) ? tile_lo + TPS_U : N_TILES;
  constexpr int NTH = 256;
  float aT[U_T::CB * U_T::TAPS], aS[U_same::CB * U_same::TAPS], bT[4], bS[4];
  const int mtT = wave & 1;  // up3.convT: M = 32 -> two m-tiles; waves (0,2) take m-tile 0, (1,3) m-tile 1
  load_areg<U_T>(a.af_t, mtT, lane, aT);
  load_biasreg<U_T>(a.bs_t, mtT, lane, bT);
  load_areg<U_same>(a.af_same, 0, lane, aS);
  load_biasreg<U_same>(a.bs_same, 0, lane, bS);
  float w[3][8], bb[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    bb[c] = a.b_out[c];
#pragma unroll
    for (int k = 0; k < 8; ++k) w[c][k] = a.w_out[c * 8 + k];
  }
  if (tid < 16) *reinterpret_cast<float4*>(lds + U_U2S + tid * U_S1) = make_float4(0.f, 0.f, 0.f, 0.f);  // local1 -4..-1

  const float* usrc = a.u2s + (long)win * a.ws_u + HALO;
  const float* ssrc = a.skip0 + (long)win * a.ws_s + HALO;
  float4 pu[3], ps[5];  // 16 x 36 = 576 and 8 x 130 = 1040 float4
  auto fetch = [&](int tile) __attribute__((always_inline)) {
    const int o1 = tile * (TT / 4) - 4, o0 = tile * TT - 16;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int i = tid + k * NTH;
      pu[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (i < 16 * 36) {
        const int c = i / 36, q = i - c * 36;
        pu[k] = *reinterpret_cast<const float4*>(usrc + o1 + (long)c * a.ls_u + 4 * q);
      }
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int i = tid + k * NTH;
      ps[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (i < 8 * 130) {
        const int c = i / 130, q = i - c * 130;
        ps[k] = *reinterpret_cast<const float4*>(ssrc + o0 + 12 + (long)c * a.ls_s + 4 * q);
      }
    }
  };
  fetch(tile_lo);
  for (int tile = tile_lo; tile < tile_hi; ++tile) {
    const int t0 = tile * TT, o0 = t0 - 16;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int i = tid + k * NTH;
      if (i < 16 * 36) {
        const int c = i / 36, q = i - c * 36;
        *reinterpret_cast<float4*>(lds + U_U2S + c * U_S1 + IB + 4 * q) = pu[k];
      }
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int i = tid + k * NTH;
      if (i < 8 * 130) {
        const int c = i / 130, q = i - c * 130;
        *reinterpret_cast<float4*>(lds + U_SKIP + c * U_S0 + IB + 12 + 4 * q) = ps[k];
      }
    }
    __syncthreads();
    if (tile + 1 < tile_hi) fetch(tile + 1);
    {
      ImageStore<U_S0, IB> st{lds + U_UT, 0, U_S0 - IB, -o0, T0 - o0};
      conv_lds_areg<U_T, U_S1, IB, U_S1, IB>(lds + U_U2S, lds + U_U2S, aT, bT, mtT, 144, st, wave >> 1, 2, lane);
    }
    __syncthreads();
    {
      ImageStore<U_SO, 0> st{lds + U_OUT, 0, TT, 0, TT};
      conv_lds_areg<U_same, U_S0, IB, U_S0, IB>(lds + U_SKIP, lds + U_UT, aS, bS, 0, TT / 2, st, wave, 4, lane);
    }
    __syncthreads();
    float* y = a.y + (long)win * 3 * T0;
    for (int l = tid; l < TT; l += NTH) {  // 1x1 conv (8 -> 3) + softmax over channels
      const int t = t0 + l;
      if (t < T0) {
        float z[3] = {bb[0], bb[1], bb[2]};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float v = lds[U_OUT + k * U_SO + l];
#pragma unroll
          for (int c = 0; c < 3; ++c) z[c] = fmaf(w[c][k], v, z[c]);
        }
        const float mx = fmaxf(z[0], fmaxf(z[1], z[2]));
        const float e0 = __expf(z[0] - mx), e1 = __expf(z[1] - mx), e2 = __expf(z[2] - mx);
        const float inv = 1.f / (e0 + e1 + e2);
        y[t] = e0 * inv;
        y[T0 + t] = e1 * inv;
        y[2 * T0 + t] = e2 * inv;
      }
    }
    // the next iteration's first barrier orders this read of the staged tile before its rewrite
  }
}

// ---------------------------------------------------------------------------------------------
// VALU forms of the two level-0 kernels (conv_valu.h): direct convolution, four consecutive samples and all
// eight output channels per lane, 256 lanes = a 1024-sample span per workgroup.  Layer chains shrink the valid
// span by 3 samples per side per k7 layer, so consecutive tiles advance by 1008 (down path) / 1016 (up path).
// ---------------------------------------------------------------------------------------------
constexpr int VU_SX = 272;                      // up2.same image row stride (258 level-1 samples per tile; == 16 mod 32)
// 50 KB and 50 KB of LDS: the three tiles of a window are resident on one CU together (256 windows on 256 CUs = one round)
constexpr int VD_LDS_FLOATS = 12 * VS + 64, VU_LDS_FLOATS = 8 * VS + 16 * VU_SX + 64;  // + margin for masked MFMA columns
// the strided and the transposed conv of the two kernels stay on the MFMA (weights used once per output sample:
// on the VALU they are bound by scalar-load latency, measured 15 k cycles for 448 packed FMAs per lane)
using VD_down = LdsLayer<4, 4, 8, 2, 11, 8, 5, 0, 1, 1>;   // out n' = 2n + p reads local 8n + tap + 5; channels 0-3 / 4-7 in two images
using VU_T = LdsLayer<16, 0, 8, 4, 2, 1, -1, -2, 5, 1>;    // out local 4m + p - 2 reads level-1 local m + tap - 1
struct TileRowStore {  // haloed activation row store of one tile: local t in [0, t_hi), global t + t_add in [0, L)
  float* p;
  int ls, L, t_add, t_hi;
  __device__ __forceinline__ void operator()(int co, int t, float v) const {
    if ((unsigned)t < (unsigned)t_hi && t + t_add < L) p[(long)co * ls + t + t_add] = v;
  }
  __device__ __forceinline__ bool all_valid(int t0, int t1) const { return t0 >= 0 && t1 < t_hi && t1 + t_add < L; }
  __device__ __forceinline__ void unchecked(int co, int t, float v) const { p[(long)co * ls + t + t_add] = v; }
};
constexpr int VX_Q = VS / 4;                    // float4 per image row
static_assert(VD_TILES == 3 && VU_TILES == 3, "three tiles per window");

__global__ __launch_bounds__(256) void pn_down0v_kernel(const Down0VArgs a) {
  extern __shared__ float4 lds_raw[];
  float* lds = reinterpret_cast<float*>(lds_raw);
  float *X = lds, *H = lds + 4 * VS;  // X: 3 input rows, later rows 0-3 of down0.same; H: inc, later rows 4-7 of down0.same
  const int tid = threadIdx.x;
  // Workgroup -> (window, tile): consecutive workgroups go to consecutive XCDs, and the core kernel runs window w on
  // XCD w % 8 — with this mapping the rows a window hands from kernel to kernel stay in one XCD's L2.
  int win, tile;
  {
    const int id = blockIdx.x, B = a.n_windows;
    if ((B & 7) == 0) {
      const int slot = id >> 3;
      win = (slot / 3) * 8 + (id & 7);
      tile = slot % 3;
    } else {
      win = id / 3;
      tile = id % 3;
    }
  }
  const int g0 = VD_TS * tile - 8;  // global sample of local 0
  {  // x image: local [-4, 1028); physical index of local -4 + 4q = HALO + g0 - 4 + 4q (16-byte aligned)
    const float* src = a.t.x + (long)win * a.t.ws_x;
    for (int i = tid; i < 3 * VX_Q; i += 256) {
      const int c = i / VX_Q, q = i - c * VX_Q;
      const int p = HALO + g0 - 4 + 4 * q;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (p >= 0 && p + 3 < a.t.ls_x) v = *reinterpret_cast<const float4*>(src + (long)c * a.t.ls_x + p);
      *reinterpret_cast<float4*>(X + c * VS + 4 * q) = v;
    }
  }
  __syncthreads();
  const int t0 = 4 * tid, tg = g0 + t0;
  const bool own = t0 >= 8 && t0 < 8 + VD_TS && tg < T0;  // samples this tile hands to memory
  f32x2 acc[4][4];
  {  // inc: Conv1d(3, 8, 7, same, bias) + BN + ReLU
    valu_bias(acc, a.b_inc);
    valu_conv7_r4<3, VS>(X, as_weights(a.w_inc), t0, acc);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      f32x4 lo, hi;
      valu_finish(acc, c, tg, &lo, &hi);
      *reinterpret_cast<f32x4*>(H + (2 * c) * VS + 4 + t0) = lo;
      *reinterpret_cast<f32x4*>(H + (2 * c + 1) * VS + 4 + t0) = hi;
      if (a.t.h0_dbg && own) {
        float* d = a.t.h0_dbg + (long)win * a.t.ws_h + HALO + tg;
        *reinterpret_cast<f32x4*>(d + (long)(2 * c) * a.t.ls_h) = lo;
        *reinterpret_cast<f32x4*>(d + (long)(2 * c + 1) * a.t.ls_h) = hi;
      }
    }
  }
  __syncthreads();
  {  // down0.same: Conv1d(8, 8, 7, same) + BN + ReLU -> skip tensor + image for the strided conv.  Two passes of four
     // output channels: the skip rows of the first pass drain to memory under the FMAs of the second (in one pass the
     // whole 25 MB of a launch left the chip in one burst after the last FMA, with nothing to hide it).
    float* d = a.t.skip0 + (long)win * a.t.ws_s + HALO + tg;
    f32x2 acc2[2][4];
    f32x4 lo[2], hi[2];
    valu_bias(acc2, a.b_same);
    valu_conv7_r4<8, VS, 2, 0>(H, as_weights(a.w_same), t0, acc2);
#pragma unroll
    for (int c = 0; c < 2; ++c) {  // rows 0-3 take the place of the x image (its last reader finished two barriers ago)
      valu_finish(acc2, c, tg, &lo[c], &hi[c]);
      *reinterpret_cast<f32x4*>(X + (2 * c) * VS + 4 + t0) = lo[c];
      *reinterpret_cast<f32x4*>(X + (2 * c + 1) * VS + 4 + t0) = hi[c];
      if (own) {  // the float4 holding sample T0 - 1 also rewrites up to three zeros of the row's right margin
        __builtin_nontemporal_store(lo[c], reinterpret_cast<f32x4*>(d + (long)(2 * c) * a.t.ls_s));
        __builtin_nontemporal_store(hi[c], reinterpret_cast<f32x4*>(d + (long)(2 * c + 1) * a.t.ls_s));
      }
    }
    valu_bias(acc2, a.b_same + 2);
    valu_conv7_r4<8, VS, 2, 2>(H, as_weights(a.w_same), t0, acc2);
    lds_barrier();  // every lane has read its inc window: rows 4-7 overwrite the first rows of that image
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      valu_finish(acc2, c, tg, &lo[c], &hi[c]);
      *reinterpret_cast<f32x4*>(H + (2 * c) * VS + 4 + t0) = lo[c];
      *reinterpret_cast<f32x4*>(H + (2 * c + 1) * VS + 4 + t0) = hi[c];
    }
    lds_barrier();
    if (own) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        __builtin_nontemporal_store(lo[c], reinterpret_cast<f32x4*>(d + (long)(4 + 2 * c) * a.t.ls_s));
        __builtin_nontemporal_store(hi[c], reinterpret_cast<f32x4*>(d + (long)(5 + 2 * c) * a.t.ls_s));
      }
    }
  }
  {  // down0.down: Conv1d(8, 8, 7, stride 4, pad 3) + BN + ReLU on the MFMA; output n = 252 * tile + n' reads local 4 n' + 5 + k
    TileRowStore st{a.t.d0 + (long)win * a.t.ws_d + HALO, a.t.ls_d, T1, (VD_TS / 4) * tile, VD_TS / 4};
    conv_lds<VD_down, VS, 4, VS, 4, false>(X, H, a.t.af_down, a.t.bs_down, VD_TS / 8, st, tid >> 6, 4, tid & 63);
  }
}

__global__ __launch_bounds__(256) void pn_up3v_kernel(const Up3VArgs a) {
  extern __shared__ float4 lds_raw[];
  float* lds = reinterpret_cast<float*>(lds_raw);
  float *A = lds, *U = lds + 8 * VS;  // A: skip rows, later the up3.convT rows; U: up2.same rows
  const int tid = threadIdx.x;
  // Workgroup -> (window, tile): consecutive workgroups go to consecutive XCDs, and the core kernel runs window w on
  // XCD w % 8 — with this mapping the rows a window hands from kernel to kernel stay in one XCD's L2.
  int win, tile;
  {
    const int id = blockIdx.x, B = a.n_windows;
    if ((B & 7) == 0) {
      const int slot = id >> 3;
      win = (slot / 3) * 8 + (id & 7);
      tile = slot % 3;
    } else {
      win = id / 3;
      tile = id % 3;
    }
  }
  const int g0 = VU_TS * tile - 4;  // global sample of local 0
  int stamp = 18;  // debug clock stamps of tile 1 (slots 18..25 of the core's [B][32] block)
#define UP3V_STAMP()                                                                                  \
  if (a.t.clk && tid == 0 && tile == 1) a.t.clk[(long)win * 32 + stamp] = __builtin_readcyclecounter(); \
  ++stamp;
  UP3V_STAMP()
  if (a.t.clk && tid == 0 && tile == 1) a.t.clk[(long)win * 32 + 26] = wall_clock64();
  const int lane = tid & 63, wave = tid >> 6;
  // skip rows: local [-4, 1028); physical index HALO + g0 - 4 + 4q = VU_TS * tile + 4q
  constexpr int NSK = (8 * VX_Q + 255) / 256;
  float4 sk[NSK];
  {
    const float* src = a.t.skip0 + (long)win * a.t.ws_s + VU_TS * tile;
#pragma unroll
    for (int k = 0; k < NSK; ++k) {
      const int i = tid + k * 256, c = i / VX_Q, q = i - c * VX_Q;
      sk[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (i < 8 * VX_Q && VU_TS * tile + 4 * q + 3 < a.t.ls_s) sk[k] = *reinterpret_cast<const float4*>(src + (long)c * a.t.ls_s + 4 * q);
    }
  }
  // up2.same rows: U[ci][j] = x[ci][(g0 >> 2) - 1 + j], j in [0, 258); physical index HALO + 254 tile - 2 + j >= 6.
  // Fetched into registers behind the skip rows and written to their image after the skip half of up3.same
  // (first use: the transposed conv): they stay in flight across the first barrier.
  constexpr int NU = (16 * 258 + 255) / 256;
  float u[NU];
  {
    const float* us = a.t.u2s + (long)win * a.t.ws_u + HALO + (VU_TS / 4) * tile - 2;
#pragma unroll
    for (int k = 0; k < NU; ++k) {
      const int i = tid + k * 256, c = i / 258, j = i - c * 258;
      u[k] = (i < 16 * 258) ? us[(long)c * a.t.ls_u + j] : 0.f;
    }
  }
  // A fragments of the transposed conv (M = 32: waves 0, 2 take m-tile 0, waves 1, 3 m-tile 1), resident in registers
  float aT[VU_T::CB * VU_T::TAPS], bT[4];
  load_areg<VU_T>(a.t.af_t, wave & 1, lane, aT);
  load_biasreg<VU_T>(a.t.bs_t, wave & 1, lane, bT);
#pragma unroll
  for (int k = 0; k < NSK; ++k) {
    const int i = tid + k * 256, c = i / VX_Q, q = i - c * VX_Q;
    if (i < 8 * VX_Q) *reinterpret_cast<float4*>(A + c * VS + 4 * q) = sk[k];
  }
  lds_barrier();  // not __syncthreads(): the up2.same rows and the A fragments are still in flight
  UP3V_STAMP()
  const int t0 = 4 * tid, tg = g0 + t0;
  const bool own = t0 >= 4 && t0 < 4 + VU_TS && tg < T0;
  f32x2 acc[4][4];
  // up3.same on cat([skip0, up3.convT]): the skip half first, then the convT rows take the skip image's place
  valu_bias(acc, a.b_same);
  valu_conv7_r4<8, VS>(A, as_weights(a.w_same), t0, acc);
  UP3V_STAMP()
#pragma unroll
  for (int k = 0; k < NU; ++k) {
    const int i = tid + k * 256, c = i / 258, j = i - c * 258;
    if (i < 16 * 258) U[c * VU_SX + j] = u[k];
  }
  __syncthreads();
  UP3V_STAMP()
  {  // up3.convT: ConvTranspose1d(16, 8, 7, stride 4) + BN + ReLU, crop [1:-2] and centre crop (t = o - 2), on the MFMA
    ImageStore<VS, 4> st{A, 0, VT, -g0, T0 - g0};
    conv_lds_areg<VU_T, VU_SX, 1, VU_SX, 1>(U, U, aT, bT, wave & 1, VT / 4 + 1, st, wave >> 1, 2, lane);
  }
  UP3V_STAMP()
  __syncthreads();
  if (a.t.ut_dbg && own) {
    float* d = a.t.ut_dbg + (long)win * a.t.ws_t + HALO + tg;
#pragma unroll
    for (int c = 0; c < 8; ++c) *reinterpret_cast<f32x4*>(d + (long)c * a.t.ls_t) = *reinterpret_cast<const f32x4*>(A + c * VS + 4 + t0);
  }
  UP3V_STAMP()
  valu_conv7_r4<8, VS>(A, as_weights(a.w_same + 8 * 28), t0, acc);
  UP3V_STAMP()
  if (own) {  // BN + ReLU -> Conv1d(8, 3, 1) -> softmax over channels
    float z[3][4];
#pragma unroll
    for (int o = 0; o < 3; ++o)
#pragma unroll
      for (int r = 0; r < 4; ++r) z[o][r] = as_scalars(a.t.b_out)[o];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v0 = fmaxf(acc[c][r].x, 0.f), v1 = fmaxf(acc[c][r].y, 0.f);
#pragma unroll
        for (int o = 0; o < 3; ++o)
          z[o][r] = fmaf(as_scalars(a.t.w_out)[o * 8 + 2 * c + 1], v1, fmaf(as_scalars(a.t.w_out)[o * 8 + 2 * c], v0, z[o][r]));
      }
    f32x4 y0, y1, y2;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float mx = fmaxf(z[0][r], fmaxf(z[1][r], z[2][r]));
      const float e0 = __expf(z[0][r] - mx), e1 = __expf(z[1][r] - mx), e2 = __expf(z[2][r] - mx);
      const float inv = 1.f / (e0 + e1 + e2);
      y0[r] = e0 * inv, y1[r] = e1 * inv, y2[r] = e2 * inv;
    }
    float* y = a.t.y + (long)win * 3 * T0 + tg;
    if (tg + 3 < T0) {  // dense rows of odd length: 4-byte aligned vector stores
      *reinterpret_cast<f32x4u*>(y) = y0;
      *reinterpret_cast<f32x4u*>(y + T0) = y1;
      *reinterpret_cast<f32x4u*>(y + 2 * T0) = y2;
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (tg + r < T0) y[r] = y0[r], y[T0 + r] = y1[r], y[2 * T0 + r] = y2[r];
    }
  }
  UP3V_STAMP()
  if (a.t.clk && tid == 0 && tile == 1) a.t.clk[(long)win * 32 + 27] = wall_clock64();
#undef UP3V_STAMP
}
}  // namespace

void pn_launch_down0(const Down0Args& a, int B, hipStream_t s) {
  hipLaunchKernelGGL(pn_down0_kernel, dim3(N_TILES, B), dim3(256), D0_LDS_FLOATS * sizeof(float), s, a);
}
void pn_launch_down0v(const Down0VArgs& a, int B, hipStream_t s) {
  hipLaunchKernelGGL(pn_down0v_kernel, dim3(VD_TILES * B), dim3(256), VD_LDS_FLOATS * sizeof(float), s, a);
}
void pn_launch_core(const CoreArgs& a, int B, hipStream_t s) {
  hipLaunchKernelGGL(pn_core_kernel, dim3(B), dim3(1024), CORE_LDS_FLOATS * sizeof(float), s, a);
}
void pn_launch_up3(const Up3Args& a, int B, bool persistent, hipStream_t s) {
  if (persistent) hipLaunchKernelGGL(pn_up3p_kernel, dim3(NSPLIT_U, B), dim3(256), UP3_LDS_FLOATS * sizeof(float), s, a);
  else hipLaunchKernelGGL(pn_up3_kernel, dim3(N_TILES, B), dim3(256), UP3_LDS_FLOATS * sizeof(float), s, a);
}
void pn_launch_up3v(const Up3VArgs& a, int B, hipStream_t s) {
  hipLaunchKernelGGL(pn_up3v_kernel, dim3(VU_TILES * B), dim3(256), VU_LDS_FLOATS * sizeof(float), s, a);
}
void pn_register_tiled(Net& net) {
  net.extra_kernels.push_back({reinterpret_cast<const void*>(&pn_core_kernel), CORE_LDS_FLOATS * sizeof(float)});
  net.extra_kernels.push_back({reinterpret_cast<const void*>(&pn_down0_kernel), D0_LDS_FLOATS * sizeof(float)});
  net.extra_kernels.push_back({reinterpret_cast<const void*>(&pn_up3_kernel), UP3_LDS_FLOATS * sizeof(float)});
  net.extra_kernels.push_back({reinterpret_cast<const void*>(&pn_up3p_kernel), UP3_LDS_FLOATS * sizeof(float)});
  net.extra_kernels.push_back({reinterpret_cast<const void*>(&pn_down0v_kernel), VD_LDS_FLOATS * sizeof(float)});
  net.extra_kernels.push_back({reinterpret_cast<const void*>(&pn_up3v_kernel), VU_LDS_FLOATS * sizeof(float)});
}

}  // namespace vp
