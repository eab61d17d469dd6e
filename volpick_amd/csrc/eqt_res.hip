// EQTransformer ResCNN stack as ONE launch: seven residual blocks (14 convs 64->64, k 3/2, length 47)
// run back to back inside one workgroup per window with the residual stream, the BN-ReLU'd conv
// input and the mid activation in LDS (60 KB); only the packed weights stream in from L2.
// Same arithmetic and the same packed A-fragments as the 14 conv_mfma_kernel launches it replaces
// (plan flag plan_flags[0] = 1 keeps those for A/B timing and the layer-by-layer parity test).
#include <type_traits>

#include "conv_b3.h"
#include "eqt_kernels.h"
#include "net.h"

namespace vp {

namespace {

constexpr int RT = EQT_T;   // 47
constexpr int RS = 80;      // image stride (== 16 mod 32): logical 0 at column 4, 29 zero columns to the right
constexpr int RB = 4;
using R_k3 = LdsLayer<64, 0, 64, 1, 3, 1, -1, 0, 3, 1>;   // conv1: (BN folded) + ReLU
using R_k2 = LdsLayer<64, 0, 64, 1, 2, 1, 0, 0, 3, 1>;
using R_k3n = LdsLayer<64, 0, 64, 1, 3, 1, -1, 0, 3, 0>;  // conv2: no activation, residual epilogue
using R_k2n = LdsLayer<64, 0, 64, 1, 2, 1, 0, 0, 3, 0>;

struct ResArgs {
  const float* x0;    // encoder output [B][64][ls]
  const float* act0;  // relu(bn1_0(x0)) [B][64][ls]
  int ls_x, ls_a;
  long ws_x, ws_a;
  float* out;         // [B][64][ls]
  int ls_out;
  long ws_out;
  const float* af1[7];  // af1 / af2: A operands regrouped for 16-byte loads (regroup_afrag4)
  const float* bs1[7];
  const float* af2[7];
  const float* bs2[7];
  const float* s_next[7];  // BN scale/shift of the NEXT block's norm1 (block 6: unused)
  const float* b_next[7];
};

struct MidStore {  // conv1 epilogue -> mid image
  float* img;
  __device__ __forceinline__ void operator()(int co, int t, float v) const {
    if ((unsigned)t < (unsigned)RT) img[co * RS + RB + t] = v;
  }
  __device__ __forceinline__ bool all_valid(int t0, int t1) const { return t0 >= 0 && t1 < RT; }
  __device__ __forceinline__ void unchecked(int co, int t, float v) const { img[co * RS + RB + t] = v; }
};

struct ResStore {  // conv2 epilogue: x += v (in place); act = relu(s*x + b) for the next block's conv1
  float* x;
  float* act;
  const float* s;
  const float* b;
  bool last;
  __device__ __forceinline__ void unchecked(int co, int t, float v) const {
    const float o = v + x[co * RS + RB + t];
    x[co * RS + RB + t] = o;
    if (!last) act[co * RS + RB + t] = fmaxf(fmaf(s[co], o, b[co]), 0.f);
  }
  __device__ __forceinline__ void operator()(int co, int t, float v) const {
    if ((unsigned)t < (unsigned)RT) unchecked(co, t, v);
  }
  __device__ __forceinline__ bool all_valid(int t0, int t1) const { return t0 >= 0 && t1 < RT; }
};

__global__ __launch_bounds__(256) void eqt_res_kernel(const ResArgs a) {
  __shared__ __attribute__((aligned(16))) float X[64 * RS];
  __shared__ __attribute__((aligned(16))) float ACT[64 * RS];
  __shared__ __attribute__((aligned(16))) float MID[64 * RS];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), win = blockIdx.x;
  // The 14 convs are a chain of short K loops over 690 KB of weights that the kernels before this one have pushed
  // out of L2: every workgroup would wait out the same HBM round trips, one channel block after the other
  // (91 us in the pipeline against 52 us on warm weights).  The first eight workgroups -- one per XCD, since
  // consecutive workgroups go to consecutive XCDs -- therefore touch one word of every 128-byte line of all
  // weights up front; the misses overlap instead of queueing, and everybody else finds the lines in L2.
  if (win < 8) {
    constexpr int kers_pf[7] = {3, 3, 3, 3, 2, 3, 2};
    float sink = 0.f;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      const int lines = 64 * 64 * kers_pf[i] / 32;
      for (int l = tid; l < lines; l += 256) sink += a.af1[i][l * 32] + a.af2[i][l * 32];
    }
    if (sink == 1.2345678e-30f) a.out[0] = sink;  // never true: keeps the loads alive
  }
  {
    const float* x0 = a.x0 + (long)win * a.ws_x + HALO;
    const float* a0 = a.act0 + (long)win * a.ws_a + HALO;
    for (int i = tid; i < 64 * RS; i += 256) {
      const int c = i / RS, col = i - c * RS, t = col - RB;
      const bool in = (unsigned)t < (unsigned)RT;
      X[i] = in ? x0[(long)c * a.ls_x + t] : 0.f;
      ACT[i] = in ? a0[(long)c * a.ls_a + t] : 0.f;  // halo columns stay zero for the whole kernel
      MID[i] = 0.f;
    }
  }
  __syncthreads();
  // The 14 convs as a straight line: every wave keeps one m-tile, its A operand (48 / 32 fragments per lane, 16-byte
  // loads) sits in registers and is requested one whole conv ahead, so no K loop waits for L2 (streamed block by block
  // inside the loop, conv_lds_q4, every conv opened with an exposed round trip: 46.6 us for 14 x 4.6 k cycles of MFMA).
#define RES_STORE1 MidStore st{MID};
#define RES_STORE2(I) ResStore st{X, ACT, a.s_next[I], a.b_next[I], (I) == 6};
#define RES_LOAD(NAME, LT, AF, BS)                     \
  float NAME[LT::CB * LT::TAPS], NAME##_b[4];          \
  load_areg4<LT>(AF, wave, lane, NAME);                \
  load_biasreg<LT>(BS, wave, lane, NAME##_b);
#define RES_RUN(NAME, LT, SRC, STORE)                                                            \
  {                                                                                              \
    STORE conv_lds_areg<LT, RS, RB, RS, RB>(SRC, SRC, NAME, NAME##_b, wave, RT, st, 0, 1, lane); \
  }                                                                                              \
  __syncthreads();
  // kernel sizes of the seven blocks: 3 3 3 3 2 3 2
  RES_LOAD(w0a, R_k3, a.af1[0], a.bs1[0])
  RES_LOAD(w0b, R_k3n, a.af2[0], a.bs2[0])
  RES_RUN(w0a, R_k3, ACT, RES_STORE1)
  RES_LOAD(w1a, R_k3, a.af1[1], a.bs1[1])
  RES_RUN(w0b, R_k3n, MID, RES_STORE2(0))
  RES_LOAD(w1b, R_k3n, a.af2[1], a.bs2[1])
  RES_RUN(w1a, R_k3, ACT, RES_STORE1)
  RES_LOAD(w2a, R_k3, a.af1[2], a.bs1[2])
  RES_RUN(w1b, R_k3n, MID, RES_STORE2(1))
  RES_LOAD(w2b, R_k3n, a.af2[2], a.bs2[2])
  RES_RUN(w2a, R_k3, ACT, RES_STORE1)
  RES_LOAD(w3a, R_k3, a.af1[3], a.bs1[3])
  RES_RUN(w2b, R_k3n, MID, RES_STORE2(2))
  RES_LOAD(w3b, R_k3n, a.af2[3], a.bs2[3])
  RES_RUN(w3a, R_k3, ACT, RES_STORE1)
  RES_LOAD(w4a, R_k2, a.af1[4], a.bs1[4])
  RES_RUN(w3b, R_k3n, MID, RES_STORE2(3))
  RES_LOAD(w4b, R_k2n, a.af2[4], a.bs2[4])
  RES_RUN(w4a, R_k2, ACT, RES_STORE1)
  RES_LOAD(w5a, R_k3, a.af1[5], a.bs1[5])
  RES_RUN(w4b, R_k2n, MID, RES_STORE2(4))
  RES_LOAD(w5b, R_k3n, a.af2[5], a.bs2[5])
  RES_RUN(w5a, R_k3, ACT, RES_STORE1)
  RES_LOAD(w6a, R_k2, a.af1[6], a.bs1[6])
  RES_RUN(w5b, R_k3n, MID, RES_STORE2(5))
  RES_LOAD(w6b, R_k2n, a.af2[6], a.bs2[6])
  RES_RUN(w6a, R_k2, ACT, RES_STORE1)
  RES_RUN(w6b, R_k2n, MID, RES_STORE2(6))
#undef RES_RUN
#undef RES_LOAD
#undef RES_STORE2
#undef RES_STORE1
  float* out = a.out + (long)win * a.ws_out + HALO;
  for (int i = tid; i < 64 * RT; i += 256) {
    const int c = i / RT, t = i - c * RT;
    out[(long)c * a.ls_out + t] = X[c * RS + RB + t];
  }
}



// ---- the same stack on the bf16 matrix cores, with EXACT three-piece operands (conv_b3.h: the form, its split, piece store and
// product group) ----
// The sums agree with the fp32-MFMA kernel above to fp32 rounding, at 6 / 16 of its matrix time.  (Activations cut to two pieces
// would need five products and move the probabilities by up to 4e-5, tools/split_bf16_study.py: not done -- parity first.)
// The residual stream stays fp32.  The A operand: [m-tile][tap * 2 + channel half][piece][lane][8], 72 / 48 registers per conv
// and lane, requested one conv ahead.
// Piece images are chunk planes (conv_b3.h: B3Chunk), 64 columns: a fragment piece = one ds_read_b128, 16 lanes reading 256
// consecutive bytes, the planes 1 KB apart -- conflict-free.
// (As [column][64 + 8 channels] the reads ran 2-way conflicted, and the four waves of a window read the SAME fragments:
// 36 KB per K-step at 128 B/clk = the 288 cycles of the step's MFMAs, one wave per SIMD to hide nothing behind:
// 3.9 k cycles per k = 3 conv for 1.7 k of MFMA issue, tools stamps of a diagnostic build.)
constexpr int R3_NC = 64;                    // columns: logical t at column t + 1
using R3Q = B3Chunk<64, R3_NC>;
constexpr int R3_XS = 49;                    // fp32 residual rows

struct Res3Args {
  const float* x0;
  const float* act0;
  int ls_x, ls_a;
  long ws_x, ws_a;
  float* out;
  int ls_out;
  long ws_out;
  const uint4* af1[7];  // bf16 pieces of the A operand (file comment)
  const float* bs1[7];
  const uint4* af2[7];
  const float* bs2[7];
  const float* s_next[7];
  const float* b_next[7];
  long af_bytes_k3, af_bytes_k2;  // size of one conv's operand (L2 warm-up)
  int warm;                       // 0: no pre-touch of the weights (plan flag plan_flags[4] = 1)
  int n_windows;                  // the last workgroup of a batch clamps its windows to it
  unsigned long long* clk;        // debug (plan_flags[1] & 2): shader-clock stamps of workgroup 0 (tools/res3_clock.py)
};
// The DUMP instance of eqt_res3t_kernel (plan_flags[1] & 4, tests/test_gpu_layers_f64.py) writes, per block i, the fp32 values its
// epilogues computed -- dbg[3 i] conv1's output relu(conv1 + b) (BatchNorm folded), dbg[3 i + 1] conv2's increment acc + b before the
// residual add, dbg[3 i + 2] the block's output -- into haloed [64][47] tensors of one row and window stride.  A struct of its own:
// a longer Res3Args would move the hidden kernel arguments of the default instances.
struct Res3DumpArgs : Res3Args {
  float* dbg[21];
  int dbg_ls;
  long dbg_ws;
};

// four consecutive channels ch .. ch + 3 (ch a multiple of four) of one column
__device__ __forceinline__ void store3(bf16_t* img, const int col, const int ch, const float (&v)[4]) {
  b3c_store4<64, R3_NC>(img, col, ch >> 2, v);
}

// R3_EXP (timing probes of tools/, never in the product build; results are WRONG with any of them):
//   1 = every conv reuses block 0's operands (no weight stream after the first request), 2 = no MFMAs, 4 = no piece stores,
//   8 = the fragments of a conv's first two K-steps stand in for all of them (no fragment reads inside the K loop)
#ifndef R3_EXP
#define R3_EXP 0
#endif
#ifndef R3_CLOCK
#define R3_CLOCK 0
#endif
template <int TAPS>
struct Res3A {
  uint4 q[TAPS * 2][3];
  float bias[4], sn[4], bn[4];  // this lane's four output channels: conv bias; scale / shift of the next block's BatchNorm (conv2)
  // everything a conv needs from memory, requested together one conv ahead
  __device__ __forceinline__ void load(const uint4* af, const float* b, const float* s, const float* sh, const int mt, const int lane) {
    const uint4* p = af + (long)mt * (TAPS * 2 * 3 * 64) + lane;
#pragma unroll
    for (int st = 0; st < TAPS * 2; ++st)
#pragma unroll
      for (int pc = 0; pc < 3; ++pc) {
        if (R3_EXP & 1) q[st][pc] = make_uint4(0x3c003c00u + lane, 0x3c003c00u + st, 0x3c003c00u + pc, 0x3c003c00u);  // no memory
        else q[st][pc] = p[(st * 3 + pc) * 64];
      }
    const int co = mt * 16 + 4 * (lane >> 4);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      bias[r] = b[co + r];
      sn[r] = s ? s[co + r] : 0.f;
      bn[r] = sh ? sh[co + r] : 0.f;
    }
  }
  // the same request in PARTS fragments k = 0 .. TAPS * 6 - 1 (the per-channel vectors ride with part 0), spread over
  // the K loop of the conv before
  static constexpr int PARTS = TAPS * 2 * 3;
  __device__ __forceinline__ void load_part(const uint4* af, const float* b, const float* s, const float* sh, const int mt, const int lane,
                                            const int k) {
    if (R3_EXP & 1) q[k / 3][k % 3] = make_uint4(0x3c003c00u + lane, 0x3c003c00u + k, 0x3c003c00u, 0x3c003c00u);  // no memory
    else q[k / 3][k % 3] = af[(long)mt * (TAPS * 2 * 3 * 64) + lane + k * 64];
    if (k == 0) {  // one 16-byte load per vector (the arrays are hipMalloc'ed, co is a multiple of four); s / sh are null for conv1 and
                   // for the last block: uniform branches around the two loads
      const int co = mt * 16 + 4 * (lane >> 4);
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 vb = *reinterpret_cast<const float4*>(b + co);
      const float4 vs = s ? *reinterpret_cast<const float4*>(s + co) : z;
      const float4 vh = sh ? *reinterpret_cast<const float4*>(sh + co) : z;
      bias[0] = vb.x, bias[1] = vb.y, bias[2] = vb.z, bias[3] = vb.w;
      sn[0] = vs.x, sn[1] = vs.y, sn[2] = vs.z, sn[3] = vs.w;
      bn[0] = vh.x, bn[1] = vh.y, bn[2] = vh.z, bn[3] = vh.w;
    }
  }
};

// acc[j] (j = n-tile) of m-tile `mt` for all 48 columns: IN_OFF = -1 (k = 3) or 0 (k = 2); src = three-piece image
template <int TAPS, int NL = 0, class NextPart = int>
__device__ __forceinline__ void res3_mac(const bf16_t* src, const Res3A<TAPS>& A, f32x4 (&acc)[3], const int lane, NextPart next_part = 0) {
  constexpr int IN_OFF = (TAPS == 3) ? -1 : 0;
  const int g = lane >> 4, n = lane & 15;
#pragma unroll
  for (int j = 0; j < 3; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bf16_t* bp = src + g * R3Q::CHS + (n + IN_OFF + 1) * 8;  // chunk g (channels 8 g ..), column of logical t = n + IN_OFF
  uint4 bA[3][3], bB[3][3];  // [n-tile][piece], two sets: the reads of step s + 1 are issued before the MFMAs of step s
  auto load_b = [&](uint4 (&b)[3][3], const int s) {
    const int tap = s >> 1, ks = s & 1;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int pc = 0; pc < 3; ++pc)
        b[j][pc] = *reinterpret_cast<const uint4*>(bp + pc * R3Q::PS + (j * 16 + tap) * 8 + ks * 4 * R3Q::CHS);
  };
  load_b(bA, 0);
  if (R3_EXP & 8) load_b(bB, 1);
#pragma unroll
  for (int s = 0; s < TAPS * 2; ++s) {
    if (s + 1 < TAPS * 2 && !(R3_EXP & 8)) {
      if (s & 1) load_b(bA, s + 1); else load_b(bB, s + 1);
    }
    if constexpr (NL > 0) {  // the next operand in parts, between the K-steps
#pragma unroll
      for (int k = s * NL / (TAPS * 2); k < (s + 1) * NL / (TAPS * 2); ++k) next_part(k);
    }
    __builtin_amdgcn_sched_barrier(0);
    {
      // b3_mac6's products, the three n-tiles interleaved: consecutive MFMAs never share an accumulator
#pragma unroll
      for (int t = 0; t < 6; ++t)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const uint4(&b)[3] = (s & 1) ? bB[j] : bA[j];
          const uint4 w = A.q[s][b3_product(t).w], x = b[b3_product(t).x];
          if (R3_EXP & 2) {
            acc[j][0] += __uint_as_float(w.x ^ x.x);  // keeps the operands alive
          } else
          acc[j] = b3_mfma(acc[j], w, x);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// One window per 256-thread workgroup, four waves, wave = m-tile (16 output channels) with all three n-tiles: the one-window
// reference of eqt_res3t_kernel (plan_flags[7] bit 9; the tests hold the default to it bit for bit).
__global__ __launch_bounds__(256) void eqt_res3_kernel(const Res3Args a) {
  __shared__ __attribute__((aligned(16))) float X_lds[64 * R3_XS];
  __shared__ __attribute__((aligned(16))) bf16_t ACT_lds[3 * R3Q::PS];
  __shared__ __attribute__((aligned(16))) bf16_t MID_lds[3 * R3Q::PS];
  // The images through pointers and the (redundant) mask on threadIdx.x: hipcc's code for this kernel depends on both spellings,
  // and these give the instruction stream the tests' reference has had since the kernel was written (tools/kernel_digest.py).
  float* X = X_lds;
  bf16_t* ACT = ACT_lds;
  bf16_t* MID = MID_lds;
  const int tid = threadIdx.x & 255, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int win = min((int)blockIdx.x, a.n_windows - 1);
  const int g = lane >> 4, n = lane & 15;
  // Debug stamps (tools/res3_clock.py) exist in -DR3_CLOCK=1 builds only: the kernel stands at 256 registers and the three
  // values a run-time switch keeps alive spilled 21 of them.
#if R3_CLOCK == 2  // inside the phases too: after the MFMAs are issued, after the epilogue, after the barrier
  unsigned long long* clk = (a.clk && tid == 0 && blockIdx.x == 0) ? a.clk : nullptr;
  int stamp = 0;
#define R3_STAMP() \
  if (clk) clk[stamp++] = __builtin_readcyclecounter();
#define R3_WSTAMP() R3_STAMP()
#elif R3_CLOCK
  unsigned long long* clk = (a.clk && threadIdx.x == 0 && blockIdx.x == 0) ? a.clk : nullptr;
  int stamp = 0;
#define R3_STAMP() \
  if (clk) clk[stamp++] = __builtin_readcyclecounter();
#define R3_WSTAMP()
#else
#define R3_STAMP()
#define R3_WSTAMP()
#endif
  R3_STAMP()
  // Prologue: EVERYTHING is requested before the first wait, the window's own rows first (loads return in order), then block
  // 0's first operand, then this workgroup's share of the L2 warm-up.  (Rounds 2-5 had three loops of load -> use, i.e. one
  // exposed memory latency per trip: 12 k cycles for the warm-up's seven trips, 12 k for the fifteen of x / act, of a 118 k-
  // cycle kernel -- tools/res3_clock.py.)
  constexpr int NXR = (64 * RT + 255) / 256, NAR = (16 * RT + 255) / 256;
  float xr[NXR], ar[NAR][4];
  {
    const float* x0 = a.x0 + (long)win * a.ws_x + HALO;
    const float* a0 = a.act0 + (long)win * a.ws_a + HALO;
#pragma unroll
    for (int k = 0; k < NXR; ++k) {
      const int i = tid + 256 * k, c = i / RT, t = i - c * RT;
      xr[k] = i < 64 * RT ? x0[(long)c * a.ls_x + t] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < NAR; ++k) {  // four channels of one column per item
      const int i = tid + 256 * k, cq = i / RT, t = i - cq * RT;
#pragma unroll
      for (int r = 0; r < 4; ++r) ar[k][r] = i < 16 * RT ? a0[(long)(4 * cq + r) * a.ls_a + t] : 0.f;
    }
  }
  Res3A<3> w1_0;
  w1_0.load(a.af1[0], a.bs1[0], nullptr, nullptr, wave, lane);
  unsigned wv[14] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};  // looked at behind the prologue's LDS stores, not here
  if (a.warm) {
    // The weights (1 MB) have left L2 since the last launch (the other kernels of the step move 0.3 GB): every XCD's L2 is
    // warmed up front, one word per 128-byte line (see eqt_res_kernel) -- by ALL workgroups of the XCD, each a slice of the
    // lines (consecutive workgroups go to consecutive XCDs): as the job of the first workgroup of each XCD, pulling 2 MB
    // through one CU made those eight workgroups, hence the launch, 4 us longer.
    const int nx = gridDim.x >= 8 ? gridDim.x >> 3 : 1, xw = (int)blockIdx.x >> 3;  // workgroups per XCD that take part; this one's index
    constexpr int kers_pf[7] = {3, 3, 3, 3, 2, 3, 2};
    if (xw < nx) {
      if ((long)nx * 256 * 128 >= a.af_bytes_k3) {  // one line per conv and thread at most: fourteen independent loads, no trip waits
#pragma unroll
        for (int i = 0; i < 7; ++i) {
          const int lines = (int)((kers_pf[i] == 3 ? a.af_bytes_k3 : a.af_bytes_k2) / 128);
          const int l = min(xw * 256 + tid, lines - 1);  // (beyond the conv's lines: its last line again, one request per wave)
          wv[2 * i] = reinterpret_cast<const unsigned*>(a.af1[i])[l * 32];
          wv[2 * i + 1] = reinterpret_cast<const unsigned*>(a.af2[i])[l * 32];
        }
      } else {
#pragma unroll
        for (int i = 0; i < 7; ++i) {
          const int lines = (int)((kers_pf[i] == 3 ? a.af_bytes_k3 : a.af_bytes_k2) / 128);
          for (int l = xw * 256 + tid; l < lines; l += nx * 256)
            wv[0] ^= reinterpret_cast<const unsigned*>(a.af1[i])[l * 32] ^ reinterpret_cast<const unsigned*>(a.af2[i])[l * 32];
        }
      }
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  R3_STAMP()
  for (int i = tid; i < 3 * R3Q::PS / 8; i += 256) {  // zero halo columns (and everything else once)
    reinterpret_cast<uint4*>(ACT)[i] = make_uint4(0u, 0u, 0u, 0u);
    reinterpret_cast<uint4*>(MID)[i] = make_uint4(0u, 0u, 0u, 0u);
  }
  __syncthreads();
  R3_STAMP()
#pragma unroll
  for (int k = 0; k < NXR; ++k) {
    const int i = tid + 256 * k, c = i / RT, t = i - c * RT;
    if (i < 64 * RT) X[c * R3_XS + t] = xr[k];
  }
#pragma unroll
  for (int k = 0; k < NAR; ++k) {
    const int i = tid + 256 * k, cq = i / RT, t = i - cq * RT;
    if (i < 16 * RT) store3(ACT, t + 1, 4 * cq, ar[k]);
  }
  {
    unsigned sink = 0u;
#pragma unroll
    for (int i = 0; i < 14; ++i) sink ^= wv[i];
    if (sink == 0x12345678u && a.ls_x == -1) a.out[0] = __uint_as_float(sink);  // never true: keeps the warm-up loads alive
  }
  __syncthreads();
  R3_STAMP()
  const int co = wave * 16 + 4 * g;  // this lane's four output channels
  f32x4 acc[3];
  // conv1: MID = relu(conv(ACT) + b) (BatchNorm folded); conv2: X += conv(MID) + b, ACT = relu(s X + b') for the next block
  auto conv1_epilogue = [&](const float (&bv)[4]) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int t = j * 16 + n;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = (t < RT) ? fmaxf(acc[j][r] + bv[r], 0.f) : 0.f;
      if (R3_EXP & 4) {
        if (v[0] + v[1] + v[2] + v[3] == 1234.5f) MID[t] = 1;
      } else
      store3(MID, t + 1, co, v);
    }
  };
  auto conv2_epilogue = [&](const float (&bv)[4], const float (&sv)[4], const float (&ov)[4], const bool last) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int t = j * 16 + n;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float o = 0.f;
        if (t < RT) {
          o = acc[j][r] + bv[r] + X[(co + r) * R3_XS + t];
          X[(co + r) * R3_XS + t] = o;
        }
        v[r] = (t < RT) ? fmaxf(fmaf(sv[r], o, ov[r]), 0.f) : 0.f;
      }
      if (R3_EXP & 4) {
        if (v[0] + v[1] + v[2] + v[3] == 1234.5f) ACT[t] = 1;
      } else
      if (!last) store3(ACT, t + 1, co, v);
    }
  };
#define R3_W(I, TAPS) ((R3_EXP & 1) ? ((TAPS) == 3 ? 0 : 4) : (I))
#define R3_BLOCK(I, TAPS, TN, W1NEXT)                                                             \
  {                                                                                               \
    Res3A<TAPS> w2;                                                                               \
    res3_mac<TAPS, TAPS * 6>(ACT, w1_##I, acc, lane, [&](const int k) {                           \
      w2.load_part(a.af2[I], a.bs2[I], (I) == 6 ? nullptr : a.s_next[I], (I) == 6 ? nullptr : a.b_next[I], wave, lane, k); \
    });                                                                                           \
    R3_WSTAMP()                                                                                   \
    conv1_epilogue(w1_##I.bias);                                                                  \
    R3_WSTAMP()                                                                                   \
    __syncthreads();                                                                              \
    R3_STAMP()                                                                                    \
    res3_mac<TAPS, TN * 6>(MID, w2, acc, lane, [&](const int k) { W1NEXT });                      \
    R3_WSTAMP()                                                                                   \
    conv2_epilogue(w2.bias, w2.sn, w2.bn, (I) == 6);                                              \
    R3_WSTAMP()                                                                                   \
    __syncthreads();                                                                              \
    R3_STAMP()                                                                                    \
  }
  Res3A<3> w1_1;
  R3_BLOCK(0, 3, 3, w1_1.load_part(a.af1[1], a.bs1[1], nullptr, nullptr, wave, lane, k);)
  Res3A<3> w1_2;
  R3_BLOCK(1, 3, 3, w1_2.load_part(a.af1[2], a.bs1[2], nullptr, nullptr, wave, lane, k);)
  Res3A<3> w1_3;
  R3_BLOCK(2, 3, 3, w1_3.load_part(a.af1[3], a.bs1[3], nullptr, nullptr, wave, lane, k);)
  Res3A<2> w1_4;
  R3_BLOCK(3, 3, 2, w1_4.load_part(a.af1[4], a.bs1[4], nullptr, nullptr, wave, lane, k);)
  Res3A<3> w1_5;
  R3_BLOCK(4, 2, 3, w1_5.load_part(a.af1[5], a.bs1[5], nullptr, nullptr, wave, lane, k);)
  Res3A<2> w1_6;
  R3_BLOCK(5, 3, 2, w1_6.load_part(a.af1[6], a.bs1[6], nullptr, nullptr, wave, lane, k);)
  R3_BLOCK(6, 2, 0, (void)k;)
#undef R3_BLOCK
  float* out = a.out + (long)win * a.ws_out + HALO;
  for (int i = tid; i < 64 * RT; i += 256) {
    const int c = i / RT, t = i - c * RT;
    out[(long)c * a.ls_out + t] = X[c * R3_XS + t];
  }
  R3_STAMP()
#undef R3_STAMP
#undef R3_WSTAMP
}

// ---- THREE windows per workgroup, eight waves (round 6) ----------------------------------------------------------------------------
// Where eqt_res3_kernel with two windows per workgroup (two teams of four waves) spent its conv phases (tools/res3_clock.py
// waves, profiles/r06_g_*): 6.8 k cycles per k = 3 conv for 3.5 k of matrix time per SIMD -- the same 6 k with the MFMAs taken
// out, the same with the fragment reads taken out, 4.3 k with the WEIGHT STREAM taken out.  Wave w of either team requests the same 18 KB operand of m-tile w (144 KB per conv and CU, 21
// 1-KB requests per wave), and those requests stood in program order in front of the conv's MFMAs: a wave issues in order, the
// texture path takes ~25 cycles per request.  Three steps from there, each measured:
//   (1) the requests in PARTS between the K-steps of the conv before (Res3A::load_part; now the form of eqt_res3_kernel too):
//       107 k -> 94 k cycles per launch;
//   (2) a wave taking its m-tile for BOTH windows of a workgroup (four waves, half the traffic, the residual rows in registers, a
//       tile's epilogue among the next tile's MFMAs): 90 k -- but ONE wave per SIMD: everything that is not an MFMA lengthens its
//       K-steps (tools/micro/mfma_slot_probe.hip: 253 cycles per twelve MFMAs with six fragment reads and twelve vector
//       instructions beside them, 183 with a second wave on the SIMD).  Built, measured (+1.2 % windows/s), replaced by
//   (3) this kernel: two waves per SIMD AND a shared stream -- wave = (m-tile, half), the nine n-tiles of THREE windows split 5 + 4
//       over the halves (the two waves of an m-tile sit on one SIMD, which has nine n-tiles whichever wave issues them), two
//       requests of each operand per three windows, on 86 CUs instead of 128.  147 KB of LDS (no residual rows there).  Tiles one
//       after the other, one accumulator each (a chain into one accumulator issues as fast as alternating ones: tools/micro/
//       mfma_chain_probe.hip); a tile's epilogue in two slices among the MFMAs of the next tile's first two K-steps.
//       101 k cycles per THREE windows (33.8 k per window against 53.4 k), matrix pipes 63 % busy (profiles/r06_g_sq_*).
// The L2 warm-up of rounds 2-5 is gone (8 k cycles of prologue; the parts are requested a whole conv ahead of their use).
// Same products in the same order into every accumulator, same epilogue arithmetic: bit-identical to eqt_res3_kernel.
// DUMP instances: one block's epilogue values (Res3DumpArgs::dbg) for this lane's four channels at sample t of tile q (window q / 3)
template <bool ON, class Args>
struct Res3Dump {
  static constexpr bool on = ON;
  const Args& a;
  const int* win;
  int blk, co;
  __device__ __forceinline__ void operator()(const int q, const int what, const int t, const float (&v)[4]) const {
    if constexpr (ON) {
      if (t < RT) {
        float* p = a.dbg[3 * blk + what] + (long)win[q / 3] * a.dbg_ws + HALO + (long)co * a.dbg_ls + t;
#pragma unroll
        for (int r = 0; r < 4; ++r) p[(long)r * a.dbg_ls] = v[r];
      }
    }
  }
};
template <int TAPS, int TN, bool CONV2, bool LAST, int NT, int Q0, class NextPart, class Stamp, class Dump>
__device__ __forceinline__ void res3t_conv(const bf16_t* src_all, bf16_t* dst_all, const Res3A<TAPS>& A, float (&X)[NT][4],
                                           NextPart next_part, const int lane, const int co, Stamp stamp, const Dump& dump) {
    constexpr int IN_OFF = (TAPS == 3) ? -1 : 0, STEPS = TAPS * 2, SLOTS = NT * STEPS, AHEAD = 2, NBUF = AHEAD + 1;  // (read-ahead 3 / 4: 104 / 108 k cycles against 101 k)
  constexpr int NL = TN * 2 * 3;  // fragments of the next conv's operand
  const int g = lane >> 4, n = lane & 15;
  const bf16_t* bp = src_all + g * R3Q::CHS + (n + IN_OFF + 1) * 8;
  uint4 b[NBUF][3];  // [slot % NBUF][piece]
  auto load_b = [&](const int i) {
    const int u = i / STEPS, s = i - u * STEPS, tap = s >> 1, ks = s & 1, q = Q0 + u, h = q / 3, j = q - 3 * h;
#pragma unroll
    for (int pc = 0; pc < 3; ++pc)
      b[i % NBUF][pc] = *reinterpret_cast<const uint4*>(bp + h * 3 * R3Q::PS + pc * R3Q::PS + (j * 16 + tap) * 8 + ks * 4 * R3Q::CHS);
  };
  auto values = [&](const int u, const f32x4 acc, float (&v)[4]) {
    const int q = Q0 + u, j = q % 3, t = j * 16 + n;
    if (!CONV2) {
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = (t < RT) ? fmaxf(acc[r] + A.bias[r], 0.f) : 0.f;
      dump(q, 0, t, v);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float o = 0.f;
        if (t < RT) {
          o = acc[r] + A.bias[r] + X[u][r];
          X[u][r] = o;
        }
        v[r] = (t < RT) ? fmaxf(fmaf(A.sn[r], o, A.bn[r]), 0.f) : 0.f;
      }
      if constexpr (Dump::on) {  // the increment is the first sum of o's: the same fp32 value
        float d[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) d[r] = acc[r] + A.bias[r];
        dump(q, 1, t, d);
        dump(q, 2, t, X[u]);
      }
    }
  };
  auto pieces = [&](const int u, const float (&v)[4]) {
    const int q = Q0 + u, h = q / 3, j = q - 3 * h, t = j * 16 + n;
    if (!(CONV2 && LAST)) store3(dst_all + h * 3 * R3Q::PS, t + 1, co, v);
  };
#pragma unroll
  for (int i = 0; i < AHEAD; ++i) load_b(i);
  f32x4 prev = {0.f, 0.f, 0.f, 0.f};
  float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < NT; ++u) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
      const int i = u * STEPS + s;
      __builtin_amdgcn_sched_barrier(0);
      if (i + AHEAD < SLOTS) load_b(i + AHEAD);
      if (NL > 0) {
#pragma unroll
        for (int k = i * NL / SLOTS; k < (i + 1) * NL / SLOTS; ++k) next_part(k);
      }
      if (u > 0 && s == 0) values(u - 1, prev, v);  // the tile before: its epilogue among this tile's MFMAs
      if (u > 0 && s == 1) pieces(u - 1, v);
      acc = b3_mac6(A.q[s], b[i % NBUF], acc);
    }
    __builtin_amdgcn_sched_barrier(0);
    prev = acc;
  }
  stamp();
  values(NT - 1, prev, v);
  pieces(NT - 1, v);
  stamp();
}

template <int NT, int Q0, bool DUMP, class Args>
__device__ __forceinline__ void res3t_body(const Args& a, bf16_t* ACT, bf16_t* MID, const int (&win)[3], const int mt) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int g = lane >> 4, n = lane & 15, co = mt * 16 + 4 * g;  // this lane's four output channels, in every conv
#if R3_CLOCK
  unsigned long long* clk = (a.clk && (tid & 255) == 0 && blockIdx.x == 0) ? a.clk + (tid >> 8) * 128 : nullptr;  // wave 0 of either half
  int stamp = 0;
#define R3T_STAMP() \
  if (clk) clk[stamp++] = __builtin_readcyclecounter();
#else
#define R3T_STAMP()
#endif
  auto wstamp = [&]() {
#if R3_CLOCK == 2
    R3T_STAMP()
#endif
  };
  R3T_STAMP()
  // Prologue: everything requested before the first wait (as in eqt_res3_kernel): the residual rows of this wave's tiles straight
  // into the accumulator layout, the activation rows as (four channels x one column) items, block 0's operand.
  float X[NT][4];
#pragma unroll
  for (int u = 0; u < NT; ++u) {
    const int q = Q0 + u, h = q / 3, j = q - 3 * h;
    const float* x0 = a.x0 + (long)win[h] * a.ws_x + HALO;
#pragma unroll
    for (int r = 0; r < 4; ++r) X[u][r] = (j * 16 + n < RT) ? x0[(long)(co + r) * a.ls_x + j * 16 + n] : 0.f;
  }
  constexpr int NAR = (3 * 16 * RT + 511) / 512;
  float ar[NAR][4];
#pragma unroll
  for (int k = 0; k < NAR; ++k) {
    const int i = tid + 512 * k, h = i / (16 * RT), rem = i - h * (16 * RT), cq = rem / RT, t = rem - cq * RT;
    const float* a0 = a.act0 + (long)win[h < 3 ? h : 0] * a.ws_a + HALO;
#pragma unroll
    for (int r = 0; r < 4; ++r) ar[k][r] = i < 3 * 16 * RT ? a0[(long)(4 * cq + r) * a.ls_a + t] : 0.f;
  }
  Res3A<3> w1_0;
  w1_0.load(a.af1[0], a.bs1[0], nullptr, nullptr, mt, lane);
  __builtin_amdgcn_sched_barrier(0);
  R3T_STAMP()
  for (int i = tid; i < 3 * 3 * R3Q::PS / 8; i += 512) {  // zero halo columns (and everything else once)
    reinterpret_cast<uint4*>(ACT)[i] = make_uint4(0u, 0u, 0u, 0u);
    reinterpret_cast<uint4*>(MID)[i] = make_uint4(0u, 0u, 0u, 0u);
  }
  __syncthreads();
  R3T_STAMP()
#pragma unroll
  for (int k = 0; k < NAR; ++k) {
    const int i = tid + 512 * k, h = i / (16 * RT), rem = i - h * (16 * RT), cq = rem / RT, t = rem - cq * RT;
    if (i < 3 * 16 * RT) store3(ACT + h * 3 * R3Q::PS, t + 1, 4 * cq, ar[k]);
  }
  __syncthreads();
  R3T_STAMP()
  // conv1: MID = relu(conv(ACT) + b) (BatchNorm folded); conv2: X += conv(MID) + b, ACT = relu(s X + b') for the next block.
  // The operand of the conv after next is requested in parts between the K-steps of each conv.
#define R3T_BLOCK(I, TAPS, TN1, W1NEXT)                                                                                       \
  {                                                                                                                           \
    Res3A<TAPS> w2;                                                                                                           \
    const Res3Dump<DUMP, Args> dump{a, win, I, co};                                                                           \
    res3t_conv<TAPS, TAPS, false, false, NT, Q0>(ACT, MID, w1_##I, X, [&](const int k) {                                       \
      w2.load_part(a.af2[I], a.bs2[I], (I) == 6 ? nullptr : a.s_next[I], (I) == 6 ? nullptr : a.b_next[I], mt, lane, k);      \
    }, lane, co, wstamp, dump);                                                                                               \
    __syncthreads();                                                                                                          \
    R3T_STAMP()                                                                                                               \
    res3t_conv<TAPS, TN1, true, (I) == 6, NT, Q0>(MID, ACT, w2, X, [&](const int k) { W1NEXT }, lane, co, wstamp, dump);       \
    __syncthreads();                                                                                                          \
    R3T_STAMP()                                                                                                               \
  }
  Res3A<3> w1_1;
  R3T_BLOCK(0, 3, 3, w1_1.load_part(a.af1[1], a.bs1[1], nullptr, nullptr, mt, lane, k);)
  Res3A<3> w1_2;
  R3T_BLOCK(1, 3, 3, w1_2.load_part(a.af1[2], a.bs1[2], nullptr, nullptr, mt, lane, k);)
  Res3A<3> w1_3;
  R3T_BLOCK(2, 3, 3, w1_3.load_part(a.af1[3], a.bs1[3], nullptr, nullptr, mt, lane, k);)
  Res3A<2> w1_4;
  R3T_BLOCK(3, 3, 2, w1_4.load_part(a.af1[4], a.bs1[4], nullptr, nullptr, mt, lane, k);)
  Res3A<3> w1_5;
  R3T_BLOCK(4, 2, 3, w1_5.load_part(a.af1[5], a.bs1[5], nullptr, nullptr, mt, lane, k);)
  Res3A<2> w1_6;
  R3T_BLOCK(5, 3, 2, w1_6.load_part(a.af1[6], a.bs1[6], nullptr, nullptr, mt, lane, k);)
  R3T_BLOCK(6, 2, 0, (void)k;)
#undef R3T_BLOCK
#pragma unroll
  for (int u = 0; u < NT; ++u) {
    const int q = Q0 + u, h = q / 3, j = q - 3 * h;
    float* out = a.out + (long)win[h] * a.ws_out + HALO;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (j * 16 + n < RT) out[(long)(co + r) * a.ls_out + j * 16 + n] = X[u][r];
  }
  R3T_STAMP()
#undef R3T_STAMP
}

// DUMP (tests only, plan_flags[1] & 4): the same kernel writing every conv's epilogue values to Res3DumpArgs::dbg from registers
template <bool DUMP = false>
__global__ __launch_bounds__(512) void eqt_res3t_kernel(const std::conditional_t<DUMP, Res3DumpArgs, Res3Args> a) {
  __shared__ __attribute__((aligned(16))) bf16_t ACT[3 * 3 * R3Q::PS];  // [window of the workgroup][piece][chunk][column][8]
  __shared__ __attribute__((aligned(16))) bf16_t MID[3 * 3 * R3Q::PS];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int last = a.n_windows - 1;  // (a batch that is no multiple of three: the last window up to three times, identical stores)
  const int win[3] = {min((int)blockIdx.x * 3, last), min((int)blockIdx.x * 3 + 1, last), min((int)blockIdx.x * 3 + 2, last)};
  if (wave < 4) res3t_body<5, 0, DUMP>(a, ACT, MID, win, wave);  // (6 + 3 measured the same)
  else res3t_body<4, 5, DUMP>(a, ACT, MID, win, wave - 4);
}

// (eqt_res3k_kernel -- eight waves per window, K split over wave pairs with a partial-sum exchange through LDS; round 2's default,
// 31.5 us on 256 CUs against 44.5 us on 128 -- was removed in round 6: plan_flags[7] bit 12 is rejected.  So is bit 13, the
// two-window form of eqt_res3_kernel that eqt_res3t_kernel replaced.)

}  // namespace

// Replaces the steps "res0.conv1" .. "res6.conv2" of the layer plan by one fused step.
int plan_eqt_fuse_res(Net& net) {
  if (pf::eqt(net.cfg, pf::EQT_RES_KSPLIT)) {
    set_error("EQTransformer plan_flags[7] bit 12 (ResCNN kernel with K split over wave pairs): removed in round 6");
    return VP_ERR_UNSUPPORTED;
  }
  if (pf::eqt(net.cfg, pf::EQT_RES_TWO_REMOVED)) {
    set_error("EQTransformer plan_flags[7] bit 13 (ResCNN kernel with two windows per workgroup): removed; the default runs three "
              "windows per workgroup (eqt_res3t_kernel), bit 9 one");
    return VP_ERR_UNSUPPORTED;
  }
  FuseSite site;
  if (int rc = find_fuse_site(net, "fused ResCNN", "res0.conv1", 14, "res6.conv2", false, &site)) return rc;
  std::vector<std::string> names;
  for (int i = 0; i < 7; ++i)
    for (const char* conv : {".conv1", ".conv2"}) names.push_back("res" + std::to_string(i) + conv);
  ConvLayer* c[14];
  if (const int missing = find_convs(net, names, c); missing >= 0) {
    set_error("fused ResCNN: conv layer %d missing", missing / 2);
    return VP_ERR_INVALID;
  }
  std::vector<ConvLayer*> c1(7), c2(7);
  for (int i = 0; i < 7; ++i) c1[i] = c[2 * i], c2[i] = c[2 * i + 1];
  const int x0 = c2[0]->res, act0 = c1[0]->src1, out = c2[6]->dst;
  // every workgroup streams the 690 KB of weights out of L2: as 16-byte loads per lane (conv_lds_q4, micro_stream.hip)
  std::vector<HostBlob*> q1(7), q2(7);
  for (int i = 0; i < 7; ++i) {
    q1[i] = net.add_blob(regroup_afrag4(*c1[i]));
    q2[i] = net.add_blob(regroup_afrag4(*c2[i]));
  }
  // default: the 14 convs on the bf16 matrix cores with exact three-piece operands (eqt_res3_kernel); plan_flags[7] bit 4
  // keeps the fp32-MFMA kernel (A/B timing; the two agree to fp32 rounding, not bitwise)
  const bool bf3 = !pf::eqt(net.cfg, pf::EQT_RES_FP32);
  std::vector<HostBlob*> b1(7, nullptr), b2(7, nullptr);
  if (bf3)
    for (int i = 0; i < 7; ++i) {
      b1[i] = net.add_blob(res3_operand(c1[i]->afrag.h, c1[i]->g.taps));
      b2[i] = net.add_blob(res3_operand(c2[i]->afrag.h, c2[i]->g.taps));
    }
  // plan_flags[1] & 4 (plan_eqt checked that the plan is the default one): the DUMP instance and the tensors it writes
  const bool dumps = pf::layer_dumps(net.cfg);
  std::vector<int> dbg;
  if (dumps)
    for (int i = 0; i < 7; ++i)
      for (const char* what : {".mid", ".conv2", ".out"}) dbg.push_back(net.add_tensor("res." + std::to_string(i) + what, 64, EQT_T));
  Step st;
  st.name = "fused.rescnn (7 residual blocks)";
  st.flops_per_window = site.flops_per_window;
  {  // 4 m-tiles x 3 n-tiles per conv; K = 64 channels x taps: 16 x taps fp32 K-steps, or 2 x taps six-MFMA groups
    double taps = 0;
    for (int i = 0; i < 7; ++i) taps += c1[i]->g.taps + c2[i]->g.taps;
    if (bf3)
      st.set_issued(0.0, 12.0 * 2 * taps * 6 * 16384.0, 0.0);
    else
      st.set_issued(12.0 * 16 * taps * 2048.0, 0.0, 0.0);
  }
  // what ResArgs and Res3Args have in common, field for field
  auto bind_common = [=](auto& a, const Net& n) {
    bind(a.x0, a.ls_x, a.ws_x, n.tensors[x0]);
    bind(a.act0, a.ls_a, a.ws_a, n.tensors[act0]);
    bind(a.out, a.ls_out, a.ws_out, n.tensors[out]);
    for (int i = 0; i < 7; ++i) {
      a.bs1[i] = c1[i]->bias.d;
      a.bs2[i] = c2[i]->bias.d;
      a.s_next[i] = c2[i]->e1.d;
      a.b_next[i] = c2[i]->e2.d;
    }
  };
  if (bf3) {
    st.run = [=](Net& n, int B, hipStream_t s) -> int {
      Res3Args a{};
      bind_common(a, n);
      for (int i = 0; i < 7; ++i) {
        a.af1[i] = reinterpret_cast<const uint4*>(b1[i]->d);
        a.af2[i] = reinterpret_cast<const uint4*>(b2[i]->d);
      }
      a.af_bytes_k3 = 4L * 3 * 2 * 3 * 64 * 16;
      a.af_bytes_k2 = 4L * 2 * 2 * 3 * 64 * 16;
      a.warm = pf::warm(n.cfg);
      a.n_windows = B;
      a.clk = clock_words(n, ClockRegions(n.max_batch).conv);  // the conv launches' region: unused under the fused plan
      if (dumps) {
        Res3DumpArgs d{};
        static_cast<Res3Args&>(d) = a;
        d.dbg_ls = n.tensors[dbg[0]].ls;
        d.dbg_ws = (long)n.tensors[dbg[0]].win_stride();
        for (int i = 0; i < 21; ++i) {
          const Tensor& t = n.tensors[dbg[i]];
          if (t.ls != d.dbg_ls || (long)t.win_stride() != d.dbg_ws) {
            set_error("fused ResCNN dumps: tensor %s has a layout of its own", t.name.c_str());
            return VP_ERR_INVALID;
          }
          d.dbg[i] = t.p;
        }
        hipLaunchKernelGGL(eqt_res3t_kernel<true>, dim3((B + 2) / 3), dim3(512), 0, s, d);
      } else if (pf::eqt(n.cfg, pf::EQT_RES_ONE_WINDOW))  // bit 9: four waves per window, one window per workgroup
        hipLaunchKernelGGL(eqt_res3_kernel, dim3(B), dim3(256), 0, s, a);
      else  // eight waves per THREE windows
        hipLaunchKernelGGL(eqt_res3t_kernel<false>, dim3((B + 2) / 3), dim3(512), 0, s, a);
      return 0;
    };
  } else {
    st.run = [=](Net& n, int B, hipStream_t s) -> int {
      ResArgs a{};
      bind_common(a, n);
      for (int i = 0; i < 7; ++i) {
        a.af1[i] = q1[i]->d;
        a.af2[i] = q2[i]->d;
      }
      hipLaunchKernelGGL(eqt_res_kernel, dim3(B), dim3(256), 0, s, a);
      return 0;
    };
  }
  replace_steps(net, site, std::move(st));
  return VP_OK;
}

}  // namespace vp
