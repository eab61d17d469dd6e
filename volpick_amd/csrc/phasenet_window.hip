// PhaseNet forward in ONE launch (the default plan): pn_window_kernel, one 1024-thread workgroup per window, runs window cut +
// annotate_batch_pre, the level-0 down path, the 13 core layers and the level-0 up path back to back out of one 158 KB LDS
// arena.  Against the three launches of phasenet_tiled.hip: down0.down and up2.same never leave LDS (18 MB +
// 24 MB of traffic per 256 windows gone), the skip tensor of level 0 -- the only one that makes a round trip through memory --
// is written and read back by the SAME CU inside one kernel (no end-of-kernel L2 write-back and invalidate between producer
// and consumer: it is served from the XCD's L2), there are no tile halos to recompute, and the two memory-bound phases that
// every workgroup of a level-0 launch entered in lock step (all load, then all compute) shrink to one 36 KB read per window
// at the start.
//
// Three forms (PnForm, phasenet_arena.h): Default -- every conv layer but the three strided ones on the bf16 matrix cores with
// exact three-piece operands (conv_b3.h), level 0 time-tiled; Level0Valu -- level 0 on the vector ALUs (conv_valu.h) and the
// fp32 MFMA; Fp32Core -- that, and the core layers on the fp32 MFMA (conv_lds.h), as pn_core_kernel runs them.
#include "conv_b3.h"
#include "phasenet_arena.h"

namespace vp {

namespace {

constexpr int W0_Q = W0_S / 4;             // float4 per row = lanes that store into a row
constexpr int W_LANES = (T0 + 3) / 4;      // lanes that own signal samples (four each)
constexpr int W_WAVES = (W0_Q + 63) / 64;  // waves that run the VALU convs (the others only load, store and do MFMA items)
// down phase: inc (8 rows; down0.same later overwrites it in place) | x (3 rows)
constexpr int WD_H = 0, WD_X = 8 * W0_S;
static_assert(11 * W0_S <= CORE_LDS_FLOATS, "level-0 down images must fit the core arena");
static_assert(WD_X <= A_D0 && A_D0 + 8 * S1_ <= 11 * W0_S, "down0.down lands on the dead x rows");
// up phase: up2.same (16 x S1_) in the middle of the arena (dead while up2.same is computed), the eight level-0 rows
// (skip, then up3.convT) in two groups of four around it
constexpr int WU_U = A_SKIP2, WU_G0 = 0, WU_G1 = WU_U + 16 * S1_;
static_assert(WU_G0 + 4 * W0_S <= WU_U && WU_U + 16 * S1_ <= A_U2T && WU_G1 + 4 * W0_S <= CORE_LDS_FLOATS, "up-phase regions");
using W_down = LdsLayer<8, 0, 8, 2, 11, 8, -3, 0, 1, 1>;   // out n' = 2n + p reads sample 8n + tap - 3
using W_upT = LdsLayer<16, 0, 8, 4, 2, 1, -1, -2, 3, 1>;    // out sample 4m + p - 2 reads level-1 sample m + tap - 1

// DUMP: row c of debug tensor i for window win (sample 0 at index 0)
__device__ __forceinline__ float* win_dump_row(const WindowArgs& a, const int i, const int win, const int c) {
  return a.dbg[i] + (long)win * a.dbg_ws[i] + HALO + (long)c * a.dbg_ls[i];
}
// DUMP: samples [0, L) of a layer's output image out of LDS, C channels: fp32 [C][S] (sample t at column B + t), a three-piece
// image B3Image<C> or a chunk-plane piece image B3Chunk<C, NC> (sample t at column t + c0).  A piece image gives back the fp32
// value its epilogue split: hi + (mid + lo) is exact in that order (mid + lo is the residual of hi, 16 significant bits).
__device__ __forceinline__ float b3_join(const bf16_t* p, const int ps) {
  return from_bf16(p[0]) + (from_bf16(p[ps]) + from_bf16(p[2 * ps]));
}
template <int C, int S, int B>
__device__ void win_dump_f32(const WindowArgs& a, const int i, const float* img, const int L, const int win, const int tid, const int nth) {
  for (int k = tid; k < C * L; k += nth) {
    const int c = k / L, t = k - c * L;
    win_dump_row(a, i, win, c)[t] = img[c * S + B + t];
  }
}
template <int C>
__device__ void win_dump_b3(const WindowArgs& a, const int i, const B3Image<C> im, const int L, const int win, const int tid, const int nth) {
  for (int k = tid; k < C * L; k += nth) {
    const int c = k / L, t = k - c * L;
    win_dump_row(a, i, win, c)[t] = b3_join(im.img + (t + im.c0) * B3Image<C>::CS + c, im.ps);
  }
}
template <int C, int NC>
__device__ void win_dump_b3c(const WindowArgs& a, const int i, const bf16_t* img, const int c0, const int L, const int win, const int tid,
                             const int nth) {
  using Q = B3Chunk<C, NC>;
  for (int k = tid; k < C * L; k += nth) {
    const int c = k / L, t = k - c * L;
    win_dump_row(a, i, win, c)[t] = b3_join(img + (c >> 3) * Q::CHS + (t + c0) * 8 + (c & 7), Q::PS);
  }
}

struct SplitRowStore {  // up3.convT -> level-0 rows 0-3 (g0) and 4-7 (g1); zero outside the signal
  float *g0, *g1;
  __device__ __forceinline__ float* row(int co) const { return (co < 4) ? g0 + co * W0_S : g1 + (co - 4) * W0_S; }
  __device__ __forceinline__ void operator()(int co, int t, float v) const {
    if ((unsigned)t < (unsigned)(W0_S - 4)) row(co)[4 + t] = (t < T0) ? v : 0.f;
  }
  __device__ __forceinline__ bool all_valid(int t0, int t1) const { return t0 >= 0 && t1 < T0; }
  __device__ __forceinline__ void unchecked(int co, int t, float v) const { row(co)[4 + t] = v; }
  __device__ __forceinline__ void vec4(int co, int t, f32x4 v) const {  // OUT_OFF = -2: two 8-byte aligned halves
    float* d = row(co) + 4 + t;
    *reinterpret_cast<f32x2*>(d) = f32x2{v[0], v[1]};
    *reinterpret_cast<f32x2*>(d + 2) = f32x2{v[2], v[3]};
  }
};

// layers of the whole-network kernel that fetch their weights three channel blocks ahead (conv_lds ADEEP): the three
// up-path "same" convs (measured: up0.same 31.6 -> 30.4 k cycles, up1.same 29.3 -> 27.5 k, +1.7 % end to end; the
// down-path layers lose a little)
#define ADEEP_LAYER(LAYER) (LAYER::SN == 1 && LAYER::TAPS == 7 && LAYER::NB >= 3)
// layers of the whole-network kernel whose weights come as 16-byte loads (conv_lds_q4): the weight-heavy ones
// (the six-tile layers keep their dword path: 14 float4 of weights on top of 24 accumulators spill at 128 registers)
#define Q4_LAYER(LAYER) (LAYER::CB % 4 == 0 && LAYER::NB <= 3)
// B3: the five deepest layers (down3.same .. up0.same: 28 % of the kernel's cycles, 40 % of its fp32 MFMA issue) run on the
// bf16 matrix cores with exact three-piece operands (conv_b3.h); their images are the three-piece kind, placed in the
// same arena: down2.down's output / down3.down's output / up0.convT's output at A_R one after the other, the skip-3
// image at the end of the arena, the bottom image in the old skip-3 slot (A_Q), which then takes up0.same's fp32 output.
constexpr int B3_D2_NC = 54, B3_SK3_NC = 68, B3_D3_NC = 22, B3_BOT_NC = 18, B3_U0T_NC = 54;  // columns per image
constexpr int B3_D2_PS = B3_D2_NC * 40, B3_SK3_PS = B3_SK3_NC * 72, B3_D3_PS = B3_D3_NC * 72, B3_BOT_PS = B3_BOT_NC * 136,
              B3_U0T_PS = B3_U0T_NC * 72;                                                      // elements per piece
constexpr int B3_SK3_OFF = CORE_LDS_FLOATS * 2 - 3 * B3_SK3_PS;  // bf16 elements from the arena start
static_assert(B3_SK3_OFF % 8 == 0 && (A_R * 2) % 8 == 0 && (A_Q * 2) % 8 == 0, "16-byte aligned images");
static_assert(A_R * 2 + 3 * B3_U0T_PS <= B3_SK3_OFF && A_R * 2 + 3 * B3_D2_PS <= B3_SK3_OFF && 3 * B3_BOT_PS <= (A_R - A_Q) * 2,
              "three-piece images of the deep layers fit their slots");
// The other core layers run on the bf16 matrix cores too, all but the three strided convs (fp32 MFMA, piece-image epilogues):
// up1.same: its two inputs (skip 2, up1.convT's output: 32 channels x 188 each) do not fit the arena as piece images side by
// side, so it runs in two K halves over ONE 48 KB image at the end of the arena (up2.convT's output slot): up1.convT writes its
// output there as pieces, eight waves (m-tile x four blocks of three n-tiles) take its taps, the image is refilled from the fp32
// skip-2 rows, the same waves add the other half and store.
constexpr int B3_U1_NC = 200, B3_U1_PS = B3_U1_NC * 40;  // columns (sample t at column t + 3) / elements per piece
static_assert(A_U2T * 4 % 16 == 0 && A_U2T * 2 + 3 * B3_U1_PS <= CORE_LDS_FLOATS * 2 && B3_U1_NC >= 192 + 6, "up1.same piece image");
// up2.same the same way: its inputs are 16 channels x 751 each, 74 KB as a chunk-plane piece image, one at a time.  up2.convT
// writes pieces into it, the waves take that half (accumulators kept), the image is refilled from the fp32 skip-1 rows, the same
// waves add the other half and store into the skip-1 slot -- the up phase then finds up2.same at the start of the arena and
// its two groups of level-0 rows behind it.
// The two transposed convs in front of them: up0.same writes ITS output as pieces (21.6 KB in the old skip-3 slot; up0.convT's
// image sits 1.1 KB further up to make room), up1.convT reads them and writes up1.same's first image; up1.same writes its
// output as a chunk-plane piece image into the skip-2 slot (37 KB: it reaches 6.4 KB into the slot behind), up2.convT reads that
// and writes up2.same's first image, which therefore starts behind it and has 768 columns (the 48th n-tile of up2.same, whose
// outputs nobody keeps, then reads a few columns of the neighbouring plane).
constexpr int B3_U0S_NC = 50, B3_U0S_PS = B3_U0S_NC * 72;                    // up0.same's output: sample t at column t + 1
constexpr int B3_U0T_SHIFT = ((A_Q * 2 + 3 * B3_U0S_PS - A_R * 2 + 7) / 8) * 8;  // bf16 elements: up0.convT's image starts this much behind A_R
constexpr int B3_U1S_NC = 194;                                                // up1.same's output (chunk planes): sample t at column t + 1
constexpr int B3_U2_NC = 768, B3_U2_OFF = (A_SKIP2 * 4 + 3 * B3Chunk<32, B3_U1S_NC>::PS * 2 + 15) / 16 * 4;  // up2.same's image: columns (sample t at column t + 3) / float offset
static_assert(B3_U0T_SHIFT >= 0 && A_R * 2 + B3_U0T_SHIFT + 3 * B3_U0T_PS <= B3_SK3_OFF && (A_R * 2 + B3_U0T_SHIFT) % 8 == 0,
              "up0.convT's image between up0.same's output pieces and the skip-3 image");
static_assert(B3_U2_OFF * 4 + 3 * B3Chunk<16, B3_U2_NC>::PS * 2 <= CORE_LDS_FLOATS * 4 && B3_U2_NC >= 47 * 16 + 8 + 3 &&
                  B3_U1S_NC >= 192 + 2,
              "up1.same's output pieces and up2.same's image behind them fit the arena");
// down1.same and down2.same (8 / 16 input channels: K-steps of four / two taps): their inputs arrive as chunk-plane piece
// images written by the fp32-MFMA strided convs in front of them (down0.down: two phases per m-tile, two v_permlane16_swap
// bring four channels of one sample to a lane; down1.down: plain), their outputs are the fp32 skip rows.
constexpr int B3_D0_NC = 760, B3_D1_NC = 200;  // sample t at column t + 3
static_assert(A_D0 * 4 + 3 * B3Chunk<8, B3_D0_NC>::PS * 2 <= CORE_LDS_FLOATS * 4 && B3_D0_NC >= 47 * 16 + 7 && B3_D1_NC >= 192 + 7,
              "down0.down / down1.down as piece images");
// D0T (PnForm::Default): inc and down0.same on the bf16 matrix cores, TIME-TILED.  Neither layer's input exists in fp32 form: the
// normalised window goes from the registers it was read into straight into bf16 pieces that rest inside the rows down0.same fills
// later (pn_window_kernel), inc's epilogue writes PIECES into a 1040-column ring [piece][parity][column / 2][8 channels] (sample s at
// column s mod 1040; it keeps the previous tile, whose tail down0.same's taps reach back into), down0.same reads the ring and
// writes its fp32 rows (the image of the strided conv behind it and the skip tensor).  Both GEMMs are M = 16 rows (output phase,
// channel), columns = sample pairs: inc K = 8 taps x 4 channels = ONE K-step, down0.same K = 8 taps x 8 channels = two K-steps.
// Six tiles of 512 samples = sixteen n-tiles per layer; in phase j every wave runs one n-tile of inc on tile j and one of
// down0.same on tile j - 1, eight samples behind (it never needs a sample inc has not produced), one barrier per phase:
// 6 x 16 x (6 + 12) = 1,728 MFMAs in place of 1,792 packed FMAs per lane.  PnForm::Level0Valu keeps the VALU forms.
// (Round 4's slice-by-slice attempt converted inc's fp32 rows on the fly and lost to the packed FMAs.)
constexpr int D0T_TS = 512, D0T_RING = 1040, D0T_HPS = B3Chunk<8, D0T_RING>::PS;
constexpr int D0T_RED = CORE_LDS_FLOATS - 256;  // the reduction scratch of the normalisation (floats): behind the ring
static_assert(D0T_TILES * D0T_TS >= W0_S - 4 + 8 && D0T_RING >= 2 * D0T_TS + 11 + 4 && D0T_RING % 2 == 0 &&
                  WD_X * 4 + 3 * D0T_HPS * 2 <= D0T_RED * 4 && (9 * 16 + 8) <= 256,
              "level-0 tiles: the ring behind the eight fp32 rows, the scratch behind the ring, inside the arena");
// ... and the level-0 UP path on the bf16 matrix cores, time-tiled the same way.  up2.same writes its output as a piece
// image (16 channels x 751 samples, chunk planes, at the start of the arena); behind it a 528-column ring holds the 16 input
// channels of up3.same as pieces -- chunk 0 the skip tensor (read back from memory tile by tile and split), chunk 1 the output of
// up3.convT (bf16 MFMA: rows (phase, channel) = two m-tiles, K = two taps x 16 channels = ONE K-step; its epilogue writes pieces)
// -- as even / odd column planes.  Twelve tiles of 256 samples: in phase j waves 8-15 produce tile j (samples 256 j - 2 ..:
// one (m-tile, n-tile) of the transposed conv and one (sample, channel quad) of the skip tensor per lane), waves 0-7 run up3.same
// (rows (phase, channel), K = 8 taps x 16 channels = four K-steps) on tile j - 1, eight samples behind, and finish it in
// registers: the two lanes that hold a sample's eight channels exchange their halves of the 1 x 1 conv (v_permlane16_swap),
// softmax, store.  No fp32 level-0 row exists in the up path any more.
// The schedule inside a phase: a producer's MFMAs issue right behind the barrier from fragments of up2.same's (static) image
// that it fetched a phase ahead; the next fragments, the split and ring store of the skip quad (fetched from memory TWO tiles
// ahead) and the next skip fetch follow, the transposed conv's own epilogue and ring store come last.  A consumer requests the
// first K-step's fragments of tile j - 1, runs the epilogue of tile j - 2 (1 x 1 conv, swap, softmax, stores: it writes y only)
// while they are in flight, then its MFMAs; only the four BN + ReLU sums cross the barrier, and one drain epilogue behind the
// loop finishes the last tile.  Each role runs its own copy of the loop (thirteen barriers in each), so that neither holds the
// other's carried registers.  Same products, same sums, same order: y is bit for bit what the undeferred schedule stored.
constexpr int U3T_TS = 256, U3T_RING = 528, U3T_NCU = 768;
using U3T_QU = B3Chunk<16, U3T_NCU>;                      // up2.same's output: sample t at column t + 1
constexpr int U3T_PLN = U3T_RING / 2, U3T_MIR = 4;  // entries of a parity plane; its first four entries are repeated behind it, so
                                                    // that the four K-steps of a fragment (two columns apart) never wrap
constexpr int U3T_PL = (U3T_PLN + U3T_MIR) * 8, U3T_CH = 2 * U3T_PL, U3T_PS = 2 * U3T_CH;  // ring: bf16 per parity plane / chunk / piece
constexpr int U3T_RING_OFF = 3 * U3T_QU::PS;              // bf16 elements from the arena start: behind the U image
static_assert(U3T_TILES * U3T_TS >= T0 + 8 && U3T_TILES * U3T_TS < 6 * U3T_RING && U3T_RING >= 2 * U3T_TS + 11 + 4 && U3T_NCU >= T1 + 2 &&
                  (U3T_RING_OFF + 3 * U3T_PS) * 2 <= CORE_LDS_FLOATS * 4 && U3T_RING_OFF % 8 == 0,
              "level-0 up tiles: up2.same's piece image and the ring behind it fit the arena");
// ---- clock stamps: every switch of the probe builds is here ----------------------------------------------------------------
// WIN_STAMP(slot): thread 0 writes the shader clock into slot `slot` of its window's 32-slot block (WindowArgs::c.clk, null = off;
// tools/core_clock.py).  CORE_WIN_STAMP stamps the core layers, slots 2 ..; in a -DD0T_PROBE / -DU3T_PROBE build
// (tools/d0t_phase_probe.py, investigation only) the phases of the tiled level-0 down / up path take those slots instead.
#define WIN_STAMP(slot) \
  if (clk && tid == 0) clk[(long)win * 32 + (slot)] = __builtin_readcyclecounter();
#ifdef D0T_PROBE
constexpr bool D0T_PROBE_BUILD = true;
#else
constexpr bool D0T_PROBE_BUILD = false;
#endif
#ifdef U3T_PROBE
constexpr bool U3T_PROBE_BUILD = true;
#else
constexpr bool U3T_PROBE_BUILD = false;
#endif
#define CORE_WIN_STAMP(slot) \
  if constexpr (!D0T_PROBE_BUILD && !U3T_PROBE_BUILD) { WIN_STAMP(slot) }
#define D0T_PHASE_STAMP(j) \
  if constexpr (D0T_PROBE_BUILD) { WIN_STAMP(2 + (j)) }
#define U3T_PHASE_STAMP(j) \
  if constexpr (U3T_PROBE_BUILD) { WIN_STAMP(2 + (j)) }

// DUMP (tests only, plan_flags[1] & 4): the same kernel writing every layer's output to WindowArgs::dbg; each dump sits behind the
// barrier that closes its layer, or in the epilogue of a time-tiled level-0 layer, and adds nothing to the other instances.
template <PnForm F, bool DUMP = false>
// amdgpu_num_vgpr counts the VGPR half of the unified file on gfx90a+ (LLVM doubles it): 60 -> at most 120 registers per lane, so that
// four forward waves leave each SIMD the 32 registers the post-processing kernels need to run beside them (prepost.hip; the D0T
// form fits without scratch, its DUMP instance, tests only, spills 24 bytes per lane)
__global__ __launch_bounds__(1024) __attribute__((amdgpu_num_vgpr(60))) void pn_window_kernel(const WindowArgs a) {
  constexpr bool B3 = F != PnForm::Fp32Core;  // the core layers (all but the strided convs) on bf16 pieces
  constexpr bool D0T = F == PnForm::Default;  // level 0, down and up, time-tiled on the bf16 matrix cores
  static_assert(!DUMP || F == PnForm::Default, "DUMP instances exist for the default form only");
  // up phase: up2.same | level-0 rows 0-3 | level-0 rows 4-7
  constexpr int XU_U = B3 ? A_SKIP1 : WU_U, XU_G0 = B3 ? A_SKIP2 : WU_G0, XU_G1 = B3 ? A_SKIP2 + 4 * W0_S : WU_G1;
  static_assert(XU_G1 + 4 * W0_S <= CORE_LDS_FLOATS && XU_U + 16 * S1_ <= (B3 ? XU_G0 : A_U2T), "up-phase regions");
  extern __shared__ float4 lds_raw[];
  float* lds = reinterpret_cast<float*>(lds_raw);
  // (the wave index as a scalar: item loops, block indices and the epilogues' "whole block in range" tests become
  // scalar code instead of per-lane predicates)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), win = blockIdx.x;
  constexpr int NTH = 1024, NWV = 16;
  unsigned long long* clk = a.c.clk;
  if (clk && tid == 0) clk[(long)win * 32 + 16] = wall_clock64();
// DUMP: behind a layer's closing barrier, its output image goes out; the barrier behind it keeps the next layer's stores off it
#define WIN_DUMP(...)   \
  if constexpr (DUMP) { \
    __VA_ARGS__;        \
    __syncthreads();    \
  }
  WIN_STAMP(0)
  WIN_STAMP(18)
  // first workgroup of each XCD: touch one word per 128-byte line of the core weights (pn_core_kernel) -- on the FIRST launch of a
  // plan only (Net::warm_launches): from then on the weights are L2-resident from launch to launch (nothing but this kernel
  // runs on the chip), and pulling 2 MB through one CU's L1 made those eight workgroups, hence the launch, 9 us longer
  // (107.4 -> 97.8 us back to back, tools/ab_steps.py phasenet "0" "0,0,0,0,1")
  if (win < 8 && a.c.warm) {
    float sink = 0.f;
#define CORE_WARM(IDX, LAYER)                                                                          \
  for (int l = tid; l < LAYER::MT * LAYER::CB * LAYER::TAPS * 2; l += NTH) sink += a.c.af[IDX][l * 32];
    CORE_WARM(0, C_d1same) CORE_WARM(1, C_d1down) CORE_WARM(2, C_d2same) CORE_WARM(3, C_d2down)
    if constexpr (B3) {
#pragma unroll
      for (int i = 0; i < 6; ++i)
        for (int l = tid; l < a.af3_lines[i]; l += NTH) sink += __uint_as_float(reinterpret_cast<const unsigned*>(a.af3[i])[l * 32]);
    } else {
      CORE_WARM(4, C_d3same) CORE_WARM(5, C_d3down) CORE_WARM(6, C_d4same) CORE_WARM(7, C_u0T) CORE_WARM(8, C_u0same)
    }
    CORE_WARM(9, C_u1T) CORE_WARM(10, C_u1same) CORE_WARM(11, C_u2T) CORE_WARM(12, C_u2same)
#undef CORE_WARM
    if (sink == 1.2345678e-30f) a.y[0] = sink;  // never true: keeps the loads alive
  }
  // Waves without VALU work pull the weights of the NEXT VALU phase through the scalar cache (one dword per 64-byte
  // line): otherwise the twelve conv waves, in lock step, miss on every line together and each trip of the conv waits
  // out an L2 round trip (up3.same took 13.6 k cycles for its skip half and 8.5 k for the identical second half).
#define WIN_WARM_SCALAR(PTR, N_FLOATS)                                                      \
  {                                                                                         \
    float warm_ = 0.f;                                                                      \
    for (int l_ = 0; l_ < (N_FLOATS); l_ += 16) warm_ += as_scalars(reinterpret_cast<const float*>(PTR))[l_]; \
    asm volatile("" ::"s"(warm_));                                                          \
  }
  bool poisoned = false;                     // the window holds a NaN / Inf: its predictions are NaN (prepost.h)
  const int t0 = 4 * tid;                    // this lane's level-0 samples t0 .. t0 + 3 (VALU phases)
  const bool vconv = wave < W_WAVES;         // wave-uniform: runs the VALU convs
  const bool vstore = tid < W0_Q;            // lanes whose float4 lies inside an image row (751..755 store the zero margin)
  const bool own = tid < W_LANES;            // lanes holding signal samples

  // Round 6: every layer's first fragments are requested in front of the barrier BEFORE the layer (a layer's operand request
  // otherwise makes its trip to L2 with all sixteen waves waiting for it: 1.1 k cycles in front of down2.same, 2.9 k in front of
  // up0.convT -- tools/core_clock.py, profiles/r06_j_*)
  [[maybe_unused]] uint4 aw1[B3Steps<8, 7>::STEPS * 3];  // down1.same's operand
  // ================= level-0 down path: inc -> down0.same -> down0.down =================
  {
    float *H = lds + WD_H, *X = lds + WD_X;
    constexpr int MAXE = (T0 + NTH - 1) / NTH;
    float v[3][MAXE];  // the window: samples tid, tid + 1024, tid + 2048 of the three channels (D0T: the normalised ones, kept)
    // D0T: the A operands of inc and down0.same, the same 9 KB for every wave: fetched FIRST, so that their trip through the CU's
    // L1 (16 waves x 9 KB at 64 B per clock) passes under the window's trip from memory instead of in front of the first tile
    [[maybe_unused]] uint4 aI[3], aS[B3Steps<8, 8>::STEPS * 3];
    [[maybe_unused]] f32x4 bI, bS;
    if constexpr (D0T) {
#pragma unroll
      for (int pc = 0; pc < 3; ++pc) aI[pc] = a.af3_inc[pc * 64 + lane];
      b3_load_a<8, 8>(a.af3_d0s, 0, lane, aS);
#pragma unroll
      for (int r = 0; r < 4; ++r) bI[r] = a.bs_inc8[4 * ((lane >> 4) & 1) + r], bS[r] = a.bs_d0s[4 * ((lane >> 4) & 1) + r];
    }
    if (a.has_pre) {
      // SeisBench annotate_batch_pre inside the kernel, arithmetic and reduction order of gather_normalize_kernel
      // (prepost.hip): window cut from the stream, per-channel mean, peak / std amplitude, scale — the window is read
      // once into registers and the normalised rows go straight into the x image (no input tensor in memory).
      const PreArgs& p = a.pre;
      float* red = lds + (D0T ? D0T_RED : 11 * W0_S);  // [9][NWV] partials (sums, maxima, minima), then stat[3][2] (free arena space behind the x rows / the ring)
      float* stat = red + 9 * NWV;
      long start = p.dense ? 0 : (long)(p.first_window + win) * p.step;
      if (!p.dense && start > p.N - T0) start = p.N - T0;  // tail window flush with the end
      const float* src = p.src + (p.dense ? (long)win * 3 * T0 : start);
      long cs = p.dense ? T0 : p.N;
      if (p.table) {
        const long* e = p.table + 3 * (p.first_window + win);
        src = p.src + e[0] + e[2];
        cs = e[1];
      }
      float sum[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < MAXE; ++k) {
          const int t = tid + k * NTH;
          v[c][k] = t < T0 ? src[c * cs + t] : 0.f;
          sum[c] += v[c][k];
        }
      const bool one_pass = p.norm == VP_NORM_PEAK;  // uniform
      // norm = peak in ONE reduction round: max_k |v_k - mean| = max(vmax - mean, mean - vmin) bit for bit (rounding is
      // monotonic and symmetric), so the maxima and minima travel with the sums (two barriers and one reduction round
      // fewer in front of every window's first convolution; a NaN / Inf sample makes the mean non-finite: the window is
      // flagged and its predictions become NaN whatever the amplitude says)
      float vhi[3] = {-INFINITY, -INFINITY, -INFINITY}, vlo[3] = {INFINITY, INFINITY, INFINITY};
      if (one_pass) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int k = 0; k < MAXE; ++k)
            if (tid + k * NTH < T0) vhi[c] = fmaxf(vhi[c], v[c][k]), vlo[c] = fminf(vlo[c], v[c][k]);
      }
      wave_sum3(sum[0], sum[1], sum[2]);  // (the DPP tree of wave_sum, three rows interleaved by hand: prepost.h)
      if (one_pass) {
        float nlo[3] = {-vlo[0], -vlo[1], -vlo[2]};
        wave_max3(vhi[0], vhi[1], vhi[2]);
        wave_max3(nlo[0], nlo[1], nlo[2]);
        if (lane == 0)
          for (int c = 0; c < 3; ++c) red[(3 + c) * NWV + wave] = vhi[c], red[(6 + c) * NWV + wave] = -nlo[c];
      }
      if (lane == 0)
        for (int c = 0; c < 3; ++c) red[c * NWV + wave] = sum[c];
      WIN_STAMP(29)
      if constexpr (!D0T) {
        for (int i = tid; i < 3 * (W0_S - T0); i += NTH) {  // zero margins of the x rows: samples -4 .. -1 and T0 .. 3019
          const int c = i / (W0_S - T0), k = i - c * (W0_S - T0);
          X[c * W0_S + (k < 4 ? k : T0 + k)] = 0.f;
        }
      }
      __syncthreads();
      if (tid < 3) {
        float acc = 0.f;
        for (int i = 0; i < NWV; ++i) acc += red[tid * NWV + i];
        const float mu = acc / (float)T0;
        stat[tid * 2] = mu;
        if (one_pass) {
          float h = red[(3 + tid) * NWV], l = red[(6 + tid) * NWV];
          for (int i = 1; i < NWV; ++i) h = fmaxf(h, red[(3 + tid) * NWV + i]), l = fminf(l, red[(6 + tid) * NWV + i]);
          stat[tid * 2 + 1] = fmaxf(h - mu, mu - l);
        }
      }
      __syncthreads();
      WIN_STAMP(30)
      const float mean[3] = {stat[0], stat[2], stat[4]};
      if (!one_pass) {
      float m[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < MAXE; ++k) {
          const int t = tid + k * NTH;
          if (t < T0) {
            const float d = v[c][k] - mean[c];
            m[c] = fmaf(d, d, m[c]);  // as gather_normalize_kernel: not left to the compiler's contraction
          }
        }
      __syncthreads();
      for (int c = 0; c < 3; ++c) {
        const float r = wave_sum(m[c]);
        if (lane == 0) red[c * NWV + wave] = r;
      }
      __syncthreads();
      if (tid < 3) {
        const float* r = red + tid * NWV;
        float acc = r[0];
        for (int i = 1; i < NWV; ++i) acc = acc + r[i];
        stat[tid * 2 + 1] = acc;
      }
      __syncthreads();
      }
      for (int c = 0; c < 3; ++c) poisoned |= !isfinite(stat[2 * c]) || !isfinite(stat[2 * c + 1]);
      float amp[3];
      if (p.per_comp) {
        for (int c = 0; c < 3; ++c) amp[c] = (p.norm == VP_NORM_PEAK) ? stat[2 * c + 1] : sqrtf(stat[2 * c + 1] / (float)(T0 - 1));
      } else {
        const float g = (p.norm == VP_NORM_PEAK) ? fmaxf(stat[1], fmaxf(stat[3], stat[5]))
                                                 : sqrtf((stat[1] + stat[3] + stat[5]) / (float)(3 * T0 - 1));
        amp[0] = amp[1] = amp[2] = g;
      }
      const NormDiv den[3] = {norm_div_prepare(amp[0] + p.norm_eps), norm_div_prepare(amp[1] + p.norm_eps),
                              norm_div_prepare(amp[2] + p.norm_eps)};
      if (p.taper > 0) {  // (uniform; PhaseNet's default is no taper: the plain loop below then carries no branch per sample)
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int k = 0; k < MAXE; ++k) {
            const int t = tid + k * NTH;
            if (t < T0) {
              float o = norm_div(v[c][k] - mean[c], den[c]);
              const int e = (t < p.taper) ? t : ((T0 - 1 - t < p.taper) ? T0 - 1 - t : -1);
              if (e >= 0) o *= 0.5f * (1.f + cosf(3.14159265358979323846f * (1.f + (float)e / (float)(p.taper - 1))));
              if constexpr (D0T) v[c][k] = o;
              else X[c * W0_S + 4 + t] = o;
            }
          }
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int k = 0; k < MAXE; ++k) {
            const int t = tid + k * NTH;
            if constexpr (D0T) v[c][k] = norm_div(v[c][k] - mean[c], den[c]);
            else if (k + 1 < MAXE || t < T0) X[c * W0_S + 4 + t] = norm_div(v[c][k] - mean[c], den[c]);
          }
      }
    } else if constexpr (D0T) {  // the normalised rows of the input tensor, into the same registers
      const float* src = a.x + (long)win * a.ws_x + HALO;
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < MAXE; ++k) {
          const int t = tid + k * NTH;
          v[c][k] = t < T0 ? src[(long)c * a.ls_x + t] : 0.f;
        }
    } else {  // x rows: sample 4q - 4 .. 4q - 1 at float4 q; physical index HALO + 4q - 4 (16-byte aligned)
      const float* src = a.x + (long)win * a.ws_x;
      for (int i = tid; i < 3 * W0_Q; i += NTH) {
        const int c = i / W0_Q, q = i - c * W0_Q;
        const int p = 4 * q + HALO - 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p + 3 < a.ls_x) v = *reinterpret_cast<const float4*>(src + (long)c * a.ls_x + p);
        *reinterpret_cast<float4*>(X + c * W0_S + 4 * q) = v;
      }
    }
    if constexpr (!D0T) {
      if (tid < 8) *reinterpret_cast<float4*>(H + tid * W0_S) = make_float4(0.f, 0.f, 0.f, 0.f);  // samples -4 .. -1: left padding
    } else if (tid < 8) {  // (word 3 of rows 0-5 takes x's first sample below: zeroed behind the tile loop)
      H[tid * W0_S] = H[tid * W0_S + 1] = H[tid * W0_S + 2] = 0.f;
      if (tid >= 6) H[tid * W0_S + 3] = 0.f;
    }
    if constexpr (D0T) {
      bf16_t* const l16 = reinterpret_cast<bf16_t*>(lds);
      bf16_t* const HP = l16 + WD_X * 2;  // inc's output: the ring, behind the eight fp32 rows
      unsigned* const HU = reinterpret_cast<unsigned*>(H);
      const int g = lane >> 4, n = lane & 15, ph = g >> 1, quad = g & 1;  // GEMM rows 4 g .. 4 g + 3 = (phase ph, channels 4 quad ..)
      // The normalised window as bf16 pieces INSIDE the rows that down0.same fills later: piece pc of sample t rests in rows
      // 2 pc (channels 0, 1) and 2 pc + 1 (channel 2 and a zero) at word 3 + t -- one word below the place of down0.same's sample
      // t, which is written a tile (512 samples) behind inc's reads.  Stored once, straight from the registers the window was
      // read into: no fp32 x image, no per-tile copies.
#pragma unroll
      for (int k = 0; k < MAXE; ++k) {
        const int t = tid + k * NTH;
        if (k + 1 < MAXE || t < T0) {
          // three values: the short form of conv_b3.h's b3_split4 (a zero fourth, its residuals not computed), kept written out for
          // the instruction stream
          const float q0 = v[0][k], q1 = v[1][k], q2 = v[2][k];
          const unsigned h0 = pack_bf16x2(q0, q1), h1 = pack_bf16x2(q2, 0.f);
          const float r0 = q0 - bf16_lo(h0), r1 = q1 - bf16_hi(h0), r2 = q2 - bf16_lo(h1);
          const unsigned m0 = pack_bf16x2(r0, r1), m1 = pack_bf16x2(r2, 0.f);
          unsigned* const xp = HU + 3 + t;
          xp[0] = h0;
          xp[W0_S] = h1;
          xp[2 * W0_S] = m0;
          xp[3 * W0_S] = m1;
          xp[4 * W0_S] = pack_bf16x2(r0 - bf16_lo(m0), r1 - bf16_hi(m0));
          xp[5 * W0_S] = pack_bf16x2(r2 - bf16_lo(m1), 0.f);
        }
      }
      if (tid < 6 * (W0_S - 3 - T0)) {  // zeros behind the signal: words 3 + T0 .. of the six rows
        const int r = tid / (W0_S - 3 - T0), c = tid - r * (W0_S - 3 - T0);
        HU[r * W0_S + 3 + T0 + c] = 0u;
      }
      // the ring as two planes per piece, even columns | odd columns (sample s at column s mod 1040): the sixteen lanes of a
      // fragment step two columns at a time and so read consecutive 16-byte chunks of ONE plane
      auto ring_at = [](const int c) { return (c & 1) * (D0T_RING / 2 * 8) + (c >> 1) * 8; };
      if (tid < 48)  // ring columns 1024 .. 1039 <-> samples -16 .. -1: zeros
        *reinterpret_cast<uint4*>(HP + (tid >> 4) * D0T_HPS + ring_at(D0T_RING - 16 + (tid & 15))) = make_uint4(0u, 0u, 0u, 0u);
      // Every wave runs one n-tile (32 samples) of inc on tile j AND one of down0.same on tile j - 1 per phase: two independent
      // MFMA chains and epilogues per wave.  (Measured on the way here, tools/d0t_phase_probe.py: a phase costs the SUM of what
      // its waves issue -- scalar instructions and branches included, the CU has one scalar unit -- plus the latency of each
      // wave's one serial chain LDS read -> MFMAs -> epilogue -> barrier; thirteen phases of eight-wave roles with per-tile x
      // copies took 2.1 k cycles each, 870 of them the copies.)
      // the skip tensor leaves tile by tile, two phases behind down0.same (one 16-byte store per lane and phase: all 96 KB of a
      // window behind the last tile made every CU of the chip store at once, 5.3 k cycles)
      const int skip_ch = tid >> 7, skip_q = tid & 127;
      float* const skip_row = a.skip0 + (long)win * a.ws_s + HALO + (long)skip_ch * a.ls_s;
      auto store_skip_tile = [&](const int k) {  // samples 512 k - 8 + 4 q .. + 3
        const int ts = D0T_TS * k - 8 + 4 * skip_q;
        if (ts >= 0 && ts < T0)
          *reinterpret_cast<f32x4*>(skip_row + ts) = *reinterpret_cast<const f32x4*>(H + skip_ch * W0_S + 4 + ts);
      };
      WIN_STAMP(31)
      __syncthreads();
      WIN_STAMP(19)
      float aD[W_down::CB * W_down::TAPS], bD[4];
      int cinc = 32 * wave + 2 * n + ph;                    // inc: ring column of this lane's sample of tile j
      int csame = D0T_RING - 11 + 32 * wave + 2 * n + g;     // down0.same: ring column of tap g's sample for tile j - 1
      csame = csame >= D0T_RING ? csame - D0T_RING : csame;
      const unsigned* xq = HU + 32 * wave + 2 * n + 2 * g;   // inc: words 3 + (sample - 3 + tap), tap = 2 g, of tile 0
      float* hq = H + 4 * quad * W0_S + 4 - 8 + 32 * wave + 2 * n + ph;  // down0.same: this lane's sample of tile 0
#pragma unroll
      for (int j = 0; j <= D0T_TILES; ++j) {
        uint4 bi[3], bs[2][3];
        if (j < D0T_TILES) {
#pragma unroll
          for (int pc = 0; pc < 3; ++pc) {
            const uint2 lo = *reinterpret_cast<const uint2*>(xq + 2 * pc * W0_S), hi = *reinterpret_cast<const uint2*>(xq + (2 * pc + 1) * W0_S);
            bi[pc] = make_uint4(lo.x, lo.y, hi.x, hi.y);
          }
        }
        if (j > 0) {
          int c1 = csame + 4;
          c1 = c1 >= D0T_RING ? c1 - D0T_RING : c1;
#pragma unroll
          for (int pc = 0; pc < 3; ++pc) {
            bs[0][pc] = *reinterpret_cast<const uint4*>(HP + pc * D0T_HPS + ring_at(csame));
            bs[1][pc] = *reinterpret_cast<const uint4*>(HP + pc * D0T_HPS + ring_at(c1));
          }
        }
        if (j >= 2) store_skip_tile(j - 2);
        if (j == D0T_TILES) {  // the A operand of down0.down, into the registers inc's operand has left
          load_areg<W_down>(a.af_down, 0, lane, aD);
          load_biasreg<W_down>(a.bs_down, 0, lane, bD);
        }
        f32x4 ia = bI, sa = {0.f, 0.f, 0.f, 0.f}, sb = bS;
        if (j < D0T_TILES) {  // inc, n-tile `wave` of tile j: samples 512 j + 32 wave + 2 n + ph; smallest products first, bias as the accumulator input
          ia = b3_mac6(aI, bi, ia);
        }
        if (j > 0) {  // down0.same, n-tile `wave` of tile j - 1: samples 512 (j - 1) - 8 + 32 wave + 2 n + ph read inc's samples .. - 3 + tap, tap = g + 4 step
          sa = b3_mfma(sa, aS[2], bs[0][0]);  // one chain per K-step
          sb = b3_mfma(sb, aS[5], bs[1][0]);
          sa = b3_mfma(sa, aS[1], bs[0][1]);
          sb = b3_mfma(sb, aS[4], bs[1][1]);
          sa = b3_mfma(sa, aS[0], bs[0][2]);
          sb = b3_mfma(sb, aS[3], bs[1][2]);
          sa = b3_mfma(sa, aS[1], bs[0][0]);
          sb = b3_mfma(sb, aS[4], bs[1][0]);
          sa = b3_mfma(sa, aS[0], bs[0][1]);
          sb = b3_mfma(sb, aS[3], bs[1][1]);
          sa = b3_mfma(sa, aS[0], bs[0][0]);
          sb = b3_mfma(sb, aS[3], bs[1][0]);
        }
        if (j < D0T_TILES) {
          float o[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = fmaxf(ia[r], 0.f);
          if (D0T_TS * (j + 1) > T0) {  // (uniform) the tile that meets the end of the signal: zeros beyond it
            const int s = D0T_TS * j + 32 * wave + 2 * n + ph;
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = s < T0 ? o[r] : 0.f;
          }
          if constexpr (DUMP) {
            const int s = D0T_TS * j + 32 * wave + 2 * n + ph;
            if (s < T0) {
#pragma unroll
              for (int r = 0; r < 4; ++r) win_dump_row(a, WD_INC, win, 4 * quad + r)[s] = o[r];
            }
          }
          b3_store4(HP + ring_at(cinc), D0T_HPS, 0, 0, 4 * quad, o);
          cinc += D0T_TS;
          cinc = cinc >= D0T_RING ? cinc - D0T_RING : cinc;
          xq += D0T_TS;
        }
        if (j > 0) {
          float o[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = fmaxf(sa[r] + sb[r], 0.f);
          if (j == 1 || D0T_TS * j > T0) {  // (uniform) the tiles that meet the ends of the signal
            const int t = D0T_TS * (j - 1) - 8 + 32 * wave + 2 * n + ph;
            if ((unsigned)t < (unsigned)(W0_S - 4)) {
#pragma unroll
              for (int r = 0; r < 4; ++r) hq[r * W0_S] = t < T0 ? o[r] : 0.f;
            }
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) hq[r * W0_S] = o[r];
          }
          csame += D0T_TS;
          csame = csame >= D0T_RING ? csame - D0T_RING : csame;
          hq += D0T_TS;
        }
        lds_barrier();
        if (j == 0) { WIN_STAMP(20) }
        D0T_PHASE_STAMP(j)
      }
      // down0.same rests in H (fp32); the ring gives way to down0.down's piece image
      b3c_zero_rest<8, B3_D0_NC>(l16 + A_D0 * 2, 3, B3_D0_NC, tid, NTH);
      if (tid < 6) H[tid * W0_S + 3] = 0.f;  // word 3 = sample -1 of down0.same (padding): x's first sample rested there
      store_skip_tile(D0T_TILES - 1);
      lds_barrier();
      WIN_STAMP(21)
      const B3PairStoreC<8, B3_D0_NC> st{l16 + A_D0 * 2, 3, T1};
      conv_lds_areg<W_down, W0_S, 4, W0_S, 4>(H, H, aD, bD, 0, (T1 + 1) / 2, st, wave, NWV, lane);
    } else {
    WIN_STAMP(31)
    __syncthreads();
    WIN_STAMP(19)
    if (vconv) {  // inc: Conv1d(3, 8, 7, same, bias) + BN + ReLU
      f32x2 acc[4][4];
      valu_bias(acc, a.b_inc);
      valu_conv7_r4<3, W0_S>(X, as_weights(a.w_inc), t0, acc);
      if (vstore) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          f32x4 lo, hi;
          valu_finish(acc, c, t0, &lo, &hi);
          *reinterpret_cast<f32x4*>(H + (2 * c) * W0_S + 4 + t0) = lo;
          *reinterpret_cast<f32x4*>(H + (2 * c + 1) * W0_S + 4 + t0) = hi;
        }
      }
    } else {
      WIN_WARM_SCALAR(a.w_same, 8 * 7 * 8)
    }
    __syncthreads();
    WIN_STAMP(20)
    {  // down0.same: Conv1d(8, 8, 7, same) + BN + ReLU; the result overwrites inc in place (image of the strided conv)
       // and goes to memory as the skip tensor (it stays in this XCD's L2 for the up phase)
      float aD[W_down::CB * W_down::TAPS], bD[4];  // A fragments of down0.down: fetched under the FMAs of down0.same
      load_areg<W_down>(a.af_down, 0, lane, aD);
      load_biasreg<W_down>(a.bs_down, 0, lane, bD);
      f32x2 acc[4][4];
      if (vconv) {
        valu_bias(acc, a.b_same);
        valu_conv7_r4<8, W0_S>(H, as_weights(a.w_same), t0, acc);
      }
      lds_barrier();  // every lane has read its inc window
      f32x4 lo[4], hi[4];
      if (vconv) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          valu_finish(acc, c, t0, &lo[c], &hi[c]);
          if (vstore) {
            *reinterpret_cast<f32x4*>(H + (2 * c) * W0_S + 4 + t0) = lo[c];
            *reinterpret_cast<f32x4*>(H + (2 * c + 1) * W0_S + 4 + t0) = hi[c];
          }
        }
      }
      if constexpr (B3) {  // the x rows are dead: down0.down takes their place (B3: as a piece image)
        b3c_zero_rest<8, B3_D0_NC>(reinterpret_cast<bf16_t*>(lds) + A_D0 * 2, 3, B3_D0_NC, tid, NTH);
      } else {
        zero_halo<8, S1_, T1>(lds + A_D0, tid, NTH);
      }
      lds_barrier();
      if (own) {  // the float4 holding sample T0 - 1 also rewrites up to three zeros of the row's right margin
        float* d = a.skip0 + (long)win * a.ws_s + HALO + t0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          *reinterpret_cast<f32x4*>(d + (long)(2 * c) * a.ls_s) = lo[c];
          *reinterpret_cast<f32x4*>(d + (long)(2 * c + 1) * a.ls_s) = hi[c];
        }
      }
      WIN_STAMP(21)
      // down0.down: Conv1d(8, 8, 7, stride 4, pad 3) + BN + ReLU on the MFMA, straight into the core's input image
      if constexpr (B3) {
        const B3PairStoreC<8, B3_D0_NC> st{reinterpret_cast<bf16_t*>(lds) + A_D0 * 2, 3, T1};
        conv_lds_areg<W_down, W0_S, 4, W0_S, 4>(H, H, aD, bD, 0, (T1 + 1) / 2, st, wave, NWV, lane);
      } else {
        RangeStore<S1_, IB> st{lds + A_D0, T1};
        conv_lds_areg<W_down, W0_S, 4, W0_S, 4>(H, H, aD, bD, 0, (T1 + 1) / 2, st, wave, NWV, lane);
      }
    }
    }
    if constexpr (B3) {
      b3_load_a<8, 7>(a.af3_d12[0], 0, lane, aw1);
    }
    lds_barrier();  // not __syncthreads(): the skip rows drain to memory under the first core layers
    WIN_DUMP(win_dump_b3c<8, B3_D0_NC>(a, WD_D0DOWN, reinterpret_cast<const bf16_t*>(lds) + A_D0 * 2, 3, T1, win, tid, NTH))
    WIN_STAMP(22)
    WIN_STAMP(1)
  }

  // ================= levels 1-4 down, up0 .. up2 (pn_core_kernel) =================
  int stamp = 2;
#define CORE_LAYER(IDX, LAYER, IN1, SI1, IN2, SI2, B2, OUT, SO, OB, STORE, CO, COLS, LOUT)                         \
  {                                                                                                                \
    STORE<SO, OB> st{{lds + (OUT), (LOUT)}};                                                                      \
    zero_halo<CO, SO, LOUT, OB>(lds + (OUT), tid, NTH);                                                          \
    if constexpr (Q4_LAYER(LAYER)) {                                                                              \
      conv_lds_q4<LAYER, SI1, IB, SI2, B2>(lds + (IN1), lds + (IN2), a.af4[IDX], a.c.bs[IDX], (COLS), st, wave, NWV, lane); \
    } else {                                                                                                       \
      conv_lds<LAYER, SI1, IB, SI2, B2, false, (LAYER::NB < BDB_MAX_NB), ADEEP_LAYER(LAYER)>(lds + (IN1), lds + (IN2), a.c.af[IDX], a.c.bs[IDX], (COLS), st, wave, NWV, lane); \
    }                                                                                                              \
    __syncthreads();                                                                                               \
    CORE_WIN_STAMP(stamp)                                                                                               \
    ++stamp;                                                                                                       \
  }
#define CORE_LAYER_AREG(IDX, LAYER, IN1, SI1, OUT, SO, OB, STORE, CO, COLS, LOUT, WMT, WFIRST, WSTEP)                       \
  {                                                                                                                \
    STORE<SO, OB> st{{lds + (OUT), (LOUT)}};                                                                      \
    zero_halo<CO, SO, LOUT, OB>(lds + (OUT), tid, NTH);                                                          \
    if ((WMT) < LAYER::MT && (WFIRST) < ((((COLS) + 15) >> 4) + LAYER::NB - 1) / LAYER::NB) {                    \
      float ar[LAYER::CB * LAYER::TAPS], br[4];                                                                    \
      load_areg4<LAYER>(a.af4[IDX], (WMT), lane, ar);                                                              \
      load_biasreg<LAYER>(a.c.bs[IDX], (WMT), lane, br);                                                           \
      conv_lds_areg<LAYER, SI1, IB, SI1, IB>(lds + (IN1), lds + (IN1), ar, br, (WMT), (COLS), st, (WFIRST), (WSTEP), lane); \
    }                                                                                                              \
    __syncthreads();                                                                                               \
    CORE_WIN_STAMP(stamp)                                                                                               \
    ++stamp;                                                                                                       \
  }
  // the two fp32 strided layers' first superblock (seven 16-byte fragments per lane), requested a layer ahead as well
  // (conv_lds_q4_request): down1.down 5.6 -> 4.6 k cycles, down2.down 6.2 -> 5.5 k
  [[maybe_unused]] f32x4 qa_d1d[C_d1down::TAPS], qa_d2d[C_d2down::TAPS];
  if constexpr (B3) {
    bf16_t* const iD0 = reinterpret_cast<bf16_t*>(lds) + A_D0 * 2;  // written by down0.down
    bf16_t* const iD1 = reinterpret_cast<bf16_t*>(lds) + A_D1 * 2;
    const int g = lane >> 4, n = lane & 15;
    {  // down1.same: one m-tile, 47 n-tiles: three per wave
      zero_halo<16, S1_, T1, IB>(lds + A_SKIP1, tid, NTH);
      auto& aw = aw1;
      float biasv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) biasv[r] = a.c.bs[0][4 * g + r];
      const int colb = wave * 48;
      b3c_mac_tiles<8, B3_D0_NC, 7, 3>(b3c_lane_ptr<8, B3_D0_NC, 7>(iD0, colb, lane), aw, [&](const int j, const f32x4 acc) {
        const int t = colb + j * 16 + n;
        if (t < T1) {
#pragma unroll
          for (int r = 0; r < 4; ++r) lds[A_SKIP1 + (4 * g + r) * S1_ + IB + t] = fmaxf(acc[r] + biasv[r], 0.f);
        }
      });
      if constexpr (Q4_LAYER(C_d1down)) {
        conv_lds_q4_request<C_d1down>(a.af4[1], T2, wave, lane, qa_d1d);
        lds_barrier();
      } else {
        __syncthreads();
      }
      CORE_WIN_STAMP(stamp)
      ++stamp;
      WIN_DUMP(win_dump_f32<16, S1_, IB>(a, WD_D1SAME, lds + A_SKIP1, T1, win, tid, NTH))
    }
    [[maybe_unused]] uint4 aw2[B3Steps<16, 7>::STEPS * 3];  // down2.same's operand (requested a layer ahead, behind down1.down's MFMAs)
    {  // down1.down (fp32 MFMA, strided) -> piece image
      const B3BlockStoreC<16, B3_D1_NC> st{iD1, 3, T2};
      b3c_zero_rest<16, B3_D1_NC>(iD1, 3, 3 + 192, tid, NTH);
      if constexpr (Q4_LAYER(C_d1down)) {
        conv_lds_q4_requested<C_d1down, S1_, IB, S1_, IB>(lds + A_SKIP1, lds + A_SKIP1, a.af4[1], a.c.bs[1], T2, st, wave, NWV, lane, qa_d1d);
      } else {
        conv_lds<C_d1down, S1_, IB, S1_, IB, false, (C_d1down::NB < BDB_MAX_NB), ADEEP_LAYER(C_d1down)>(lds + A_SKIP1, lds + A_SKIP1, a.c.af[1], a.c.bs[1], T2, st, wave, NWV, lane);
      }
      if (wave < 8) b3_load_a<16, 7>(a.af3_d12[1], wave & 1, lane, aw2);  // travels under the barrier wait
      lds_barrier();  // not __syncthreads(): it would wait for the request just made
      CORE_WIN_STAMP(stamp)
      ++stamp;
      WIN_DUMP(win_dump_b3c<16, B3_D1_NC>(a, WD_D1DOWN, iD1, 3, T2, win, tid, NTH))
    }
    {  // down2.same: wave = (m-tile, block of three n-tiles), eight waves
      zero_halo<32, S2_, T2, IB>(lds + A_SKIP2, tid, NTH);
      if (wave < 8) {
        const int mt = wave & 1, colb = (wave >> 1) * 48;
        auto& aw = aw2;
        float biasv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) biasv[r] = a.c.bs[2][mt * 16 + 4 * g + r];
        b3c_mac_tiles<16, B3_D1_NC, 7, 3>(b3c_lane_ptr<16, B3_D1_NC, 7>(iD1, colb, lane), aw, [&](const int j, const f32x4 acc) {
          const int t = colb + j * 16 + n;
          if (t < T2) {
#pragma unroll
            for (int r = 0; r < 4; ++r) lds[A_SKIP2 + (mt * 16 + 4 * g + r) * S2_ + IB + t] = fmaxf(acc[r] + biasv[r], 0.f);
          }
        });
      }
      conv_lds_q4_request<C_d2down>(a.af4[3], T3, wave, lane, qa_d2d);  // (down2.down's conv_lds_q4 call sits in the B3 block below)
      lds_barrier();
      CORE_WIN_STAMP(stamp)
      ++stamp;
      WIN_DUMP(win_dump_f32<32, S2_, IB>(a, WD_D2SAME, lds + A_SKIP2, T2, win, tid, NTH))
    }
  } else {
  CORE_LAYER(0, C_d1same, A_D0, S1_, A_D0, S1_, IB, A_SKIP1, S1_, IB, RangeStoreS, 16, T1, T1)
  CORE_LAYER(1, C_d1down, A_SKIP1, S1_, A_SKIP1, S1_, IB, A_D1, S2_, IB, RangeStoreS, 16, T2, T2)
  CORE_LAYER(2, C_d2same, A_D1, S2_, A_D1, S2_, IB, A_SKIP2, S2_, IB, RangeStoreS, 32, T2, T2)
  }
  [[maybe_unused]] uint4 q_u1t[4][3];  // up1.convT's first fragments (requested under up0.same's closing barrier)
  [[maybe_unused]] uint4 q_u1s[4][3];  // up1.same's, either K half
  [[maybe_unused]] uint4 aT2[B3Steps<32, 2>::STEPS * 3];  // up2.convT's operand
  [[maybe_unused]] uint4 aw_u2[B3Steps<16, 7>::STEPS * 3];  // up2.same's first operand (the K half of up2.convT's channels)
  if constexpr (B3) {
    bf16_t* l16 = reinterpret_cast<bf16_t*>(lds);
    const B3Image<32> iD2{l16 + A_R * 2, B3_D2_PS, 3};
    const B3Image<64> iSK3{l16 + B3_SK3_OFF, B3_SK3_PS, 3}, iD3{l16 + A_R * 2, B3_D3_PS, 3}, iU0T{l16 + A_R * 2 + B3_U0T_SHIFT, B3_U0T_PS, 3};
    const B3Image<128> iBOT{l16 + A_Q * 2, B3_BOT_PS, 1};
#define B3_END          \
  lds_barrier(); /* not __syncthreads(): the next layer's first fragments are in flight */ \
  CORE_WIN_STAMP(stamp)      \
  ++stamp;
    // the first K-steps of every layer's first item are requested in front of the barrier BEFORE the layer
    // (conv_b3_request): a layer's first fragments otherwise make their trip to L2 with all sixteen waves waiting
    [[maybe_unused]] uint4 q_d3s[4][3], q_d3d[4][3], q_d4s[4][3], q_u0t[4][3], q_u0s[3][3];
    {  // down2.down (fp32 MFMA, strided) -> three-piece image
      B3BlockStore<32> st{{iD2.img, iD2.ps, iD2.c0, T3, B3_D2_NC}};
      st.zero_rest(3, 3 + 48, tid, NTH);
      conv_lds_q4_requested<C_d2down, S2_, IB, S2_, IB>(lds + A_SKIP2, lds + A_SKIP2, a.af4[3], a.c.bs[3], T3, st, wave, NWV, lane, qa_d2d);
      conv_b3_request<C_d3same>(a.af3[0], T3, wave, lane, q_d3s);
      B3_END
      WIN_DUMP(win_dump_b3<32>(a, WD_D2DOWN, iD2, T3, win, tid, NTH))
    }
    {  // down3.same
      B3Store<64> st{iSK3.img, iSK3.ps, iSK3.c0, T3, B3_SK3_NC};
      st.zero_rest(3, 3 + 48, tid, NTH);
      conv_b3_requested<C_d3same, false, 32, 32>(iD2, iD2, a.af3[0], a.c.bs[4], T3, st, wave, NWV, lane, q_d3s);
      conv_b3_request<C_d3down>(a.af3[1], T4, wave, lane, q_d3d);
      B3_END
      WIN_DUMP(win_dump_b3<64>(a, WD_D3SAME, iSK3, T3, win, tid, NTH))
    }
    {  // down3.down
      B3Store<64> st{iD3.img, iD3.ps, iD3.c0, T4, B3_D3_NC};
      st.zero_rest(3, 3 + 16, tid, NTH);
      conv_b3_requested<C_d3down, false, 64, 64>(iSK3, iSK3, a.af3[1], a.c.bs[5], T4, st, wave, NWV, lane, q_d3d);
      conv_b3_request<C_d4same>(a.af3[2], T4, wave, lane, q_d4s);
      B3_END
      WIN_DUMP(win_dump_b3<64>(a, WD_D3DOWN, iD3, T4, win, tid, NTH))
    }
    {  // down4.same
      B3Store<128> st{iBOT.img, iBOT.ps, iBOT.c0, T4, B3_BOT_NC};
      st.zero_rest(1, 1 + 16, tid, NTH);
      conv_b3_requested<C_d4same, false, 64, 64>(iD3, iD3, a.af3[2], a.c.bs[6], T4, st, wave, NWV, lane, q_d4s);
      conv_b3_request<C_u0T>(a.af3[3], T4 + 1, wave, lane, q_u0t);
      B3_END
      WIN_DUMP(win_dump_b3<128>(a, WD_D4SAME, iBOT, T4, win, tid, NTH))
    }
    {  // up0.convT: rows ordered (phase, channel); samples 4 c + phase - 1, columns c in [0, 16)
      B3Store<64> st{iU0T.img, iU0T.ps, iU0T.c0, T3, B3_U0T_NC};
      st.zero_rest(2, B3_U0T_NC, tid, NTH);
      conv_b3_requested<C_u0T, true, 128, 128>(iBOT, iBOT, a.af3[3], a.c.bs[7], T4 + 1, st, wave, NWV, lane, q_u0t);
      conv_b3_request<C_u0same, 2>(a.af3[4], T3, wave, lane, q_u0s);
      B3_END
      WIN_DUMP(win_dump_b3<64>(a, WD_U0T, iU0T, T3, win, tid, NTH))
    }
    {  // up0.same: cat(skip 3, up0.convT) -> three-piece image for up1.convT
      B3Store<64> st{l16 + A_Q * 2, B3_U0S_PS, 1, T3, B3_U0S_NC};
      st.zero_rest(1, 1 + 48, tid, NTH);
      conv_b3_requested<C_u0same, false, 64, 64, decltype(st), 2>(iSK3, iU0T, a.af3[4], a.c.bs[8], T3, st, wave, NWV, lane, q_u0s);
      conv_b3_request<C_u1T>(a.af3_uT[0], T3 + 1, wave, lane, q_u1t);
      B3_END
      WIN_DUMP(win_dump_b3<64>(a, WD_U0SAME, B3Image<64>{l16 + A_Q * 2, B3_U0S_PS, 1}, T3, win, tid, NTH))
    }
#undef B3_END
  } else {
  CORE_LAYER(3, C_d2down, A_SKIP2, S2_, A_SKIP2, S2_, IB, A_D2, S3_, IB, RangeStoreS, 32, T3, T3)
  CORE_LAYER(4, C_d3same, A_D2, S3_, A_D2, S3_, IB, A_SKIP3, S3_, IB, RangeStoreS, 64, T3, T3)
  CORE_LAYER(5, C_d3down, A_SKIP3, S3_, A_SKIP3, S3_, IB, A_D3, S4_, IB, RangeStoreS, 64, T4, T4)
  CORE_LAYER(6, C_d4same, A_D3, S4_, A_D3, S4_, IB, A_BOT, S4_, IB, RangeStoreS, 128, T4, T4)
  CORE_LAYER(7, C_u0T, A_BOT, S4_, A_BOT, S4_, IB, A_U0T, S3_, TB, RangeStoreV, 64, T4 + 1, T3)
  CORE_LAYER(8, C_u0same, A_SKIP3, S3_, A_U0T, S3_, TB, A_U0S, S3_, IB, RangeStoreS, 64, T3, T3)
  }
  if constexpr (B3) {
    const B3Image<32> iP{reinterpret_cast<bf16_t*>(lds) + A_U2T * 2, B3_U1_PS, 3};
    {  // up1.convT on the bf16 matrix cores: rows (phase, channel), samples 4 c + phase - 1, columns c in [0, 48)
      const B3Image<64> iU0S{reinterpret_cast<bf16_t*>(lds) + A_Q * 2, B3_U0S_PS, 1};
      B3Store<32> st{iP.img, iP.ps, iP.c0, T2, B3_U1_NC};
      st.zero_rest(2, 2 + 192, tid, NTH);
      conv_b3_requested<C_u1T, true, 64, 64>(iU0S, iU0S, a.af3_uT[0], a.c.bs[9], T3 + 1, st, wave, NWV, lane, q_u1t);
      if (wave < 8) conv_b3_part_request<C_u1same, 1>(a.af3[5], wave & 1, lane, q_u1s);
      lds_barrier();
      CORE_WIN_STAMP(stamp)
      ++stamp;
      WIN_DUMP(win_dump_b3<32>(a, WD_U1T, iP, T2, win, tid, NTH))
    }
    {  // up1.same: K half of up1.convT's channels, then the half of skip 2
      bf16_t* const iU1S = reinterpret_cast<bf16_t*>(lds) + A_SKIP2 * 2;  // the output as chunk-plane pieces, in skip 2's slot (the
                                                                          // stores come after its rows have been turned into pieces)
      const int mt = wave & 1, colb = (wave >> 1) * 48;
      f32x4 acc[3] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      if (wave < 8) {
        conv_b3_part_requested<C_u1same, 1, 3>(iP, a.af3[5], mt, colb, lane, acc, q_u1s);
        conv_b3_part_request<C_u1same, 0>(a.af3[5], mt, lane, q_u1s);  // the second half's first taps: under the refill
      }
      lds_barrier();
      b3_from_f32<S2_, IB>(lds + A_SKIP2, iP, -3, B3_U1_NC - 3, tid, NTH);
      lds_barrier();
      if (wave >= 8) b3c_zero_rest<32, B3_U1S_NC>(iU1S, 1, 193, tid - 512, NTH - 512);
      if (wave < 8) {
        conv_b3_part_requested<C_u1same, 0, 3>(iP, a.af3[5], mt, colb, lane, acc, q_u1s);
        const int co0 = mt * 16 + 4 * (lane >> 4);
        float biasv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) biasv[r] = a.c.bs[10][co0 + r];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          float v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = C_u1same::RELU ? fmaxf(acc[j][r] + biasv[r], 0.f) : acc[j][r] + biasv[r];
          const int t = colb + j * 16 + (lane & 15);
          if (t >= T2) v[0] = v[1] = v[2] = v[3] = 0.f;
          b3c_store4<32, B3_U1S_NC>(iU1S, t + 1, co0 >> 2, v);
        }
      }
      b3_load_a<32, 2>(a.af3_uT[1], wave & 3, lane, aT2);
      lds_barrier();
      CORE_WIN_STAMP(stamp)
      ++stamp;
      WIN_DUMP(win_dump_b3c<32, B3_U1S_NC>(a, WD_U1SAME, iU1S, 1, T2, win, tid, NTH))
    }
  } else {
  CORE_LAYER_AREG(9, C_u1T, A_U0S, S3_, A_U1T, S2_, TB, RangeStoreV, 32, T3 + 1, T2, wave, 0, 1)        // 8 m-tiles x 1 block (pn_core_kernel)
  CORE_LAYER(10, C_u1same, A_SKIP2, S2_, A_U1T, S2_, TB, A_U1S, S2_, IB, RangeStoreS, 32, T2, T2)
  }
  [[maybe_unused]] bf16_t* const P2 = reinterpret_cast<bf16_t*>(lds) + B3_U2_OFF * 2;
  if constexpr (B3) {  // up2.convT on the bf16 matrix cores: wave = (phase m-tile, block of three n-tiles), samples 4 c + phase - 1
    const bf16_t* iU1S = reinterpret_cast<const bf16_t*>(lds) + A_SKIP2 * 2;
    b3c_zero_rest<16, B3_U2_NC>(P2, 3, 3 + T1, tid, NTH);
    const int mt = wave & 3, colb = (wave >> 2) * 48, g = lane >> 4, n = lane & 15;
    auto& aT = aT2;
    float biasv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) biasv[r] = a.c.bs[11][4 * g + r];
    b3c_mac_tiles<32, B3_U1S_NC, 2, 3>(b3c_lane_ptr<32, B3_U1S_NC, 2>(iU1S, colb, lane), aT, [&](const int j, const f32x4 acc) {
      const int t = 4 * (colb + j * 16 + n) + mt - 1;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = C_u2T::RELU ? fmaxf(acc[r] + biasv[r], 0.f) : acc[r] + biasv[r];
      if ((unsigned)t < (unsigned)T1) b3c_store4<16, B3_U2_NC>(P2, t + 3, g, v);
    });
    if constexpr (D0T) {
      b3_load_a<16, 7>(a.af3_u2[1], 0, lane, aw_u2);
    }
    if (D0T) lds_barrier();
    else __syncthreads();
    CORE_WIN_STAMP(stamp)
    ++stamp;
    WIN_DUMP(win_dump_b3c<16, B3_U2_NC>(a, WD_U2T, P2, 3, T1, win, tid, NTH))
  } else {
  CORE_LAYER_AREG(11, C_u2T, A_U1S, S2_, A_U2T, S1_, TB, RangeStoreV, 16, T2 + 1, T1, wave & 3, wave >> 2, 4)  // 4 m-tiles x 4 blocks
  }
#undef CORE_LAYER_AREG
  // up2.same has eight items: waves 0-7 run it, waves 8-15 meanwhile fetch the eight skip rows of the up phase into
  // registers (their LDS destination is still in use by this layer) and park them in LDS right after the barrier —
  // the read-back of the skip tensor costs the up phase nothing (it was 8 k cycles of exposed memory latency).
  constexpr int NSKQ = (8 * W0_Q + 511) / 512;
  // D0T: the operands of the up path (the consumer waves' 48 registers of up3.same, the producer waves' 12 of up3.convT, the
  // 1 x 1 head, the first skip quads) are requested under up2.same, behind every wave's last MFMA of it
  [[maybe_unused]] uint4 u3_aw[B3Steps<16, 8>::STEPS * 3];
  [[maybe_unused]] f32x4 u3_bv;
  [[maybe_unused]] float u3_w1[3][4], u3_b1[3], u3_sk[4] = {0.f, 0.f, 0.f, 0.f};
  [[maybe_unused]] const int u3_pl = tid - 512, u3_skq = u3_pl & 1, u3_sks = u3_pl >> 1;  // producer lane: skip channel quad, sample within the tile
  [[maybe_unused]] const float* const u3_src = a.skip0 + (long)win * a.ws_s + HALO + (long)(4 * u3_skq) * a.ls_s;
  [[maybe_unused]] auto u3_fetch_skip = [&](float (&d)[4], const int j, const bool edge) {  // samples 256 j - 2 + u3_sks of channels 4 u3_skq ..
    const int ts = U3T_TS * j - 2 + u3_sks;
#pragma unroll
    for (int r = 0; r < 4; ++r) d[r] = (!edge || (unsigned)ts < (unsigned)T0) ? u3_src[(long)r * a.ls_s + ts] : 0.f;
  };
  [[maybe_unused]] auto u3_load_operands = [&]() {
    const int q = (lane >> 4) & 1;
    if (wave >= 8) {
#pragma unroll
      for (int pc = 0; pc < 3; ++pc) u3_aw[pc] = a.af3_u3t[(long)(wave & 1) * (3 * 64) + pc * 64 + lane];
#pragma unroll
      for (int r = 0; r < 4; ++r) u3_bv[r] = a.bs_u3t[4 * q + r];
      u3_fetch_skip(u3_sk, 0, true);
    } else {
      b3_load_a<16, 8>(a.af3_u3s, 0, lane, u3_aw);
#pragma unroll
      for (int r = 0; r < 4; ++r) u3_bv[r] = a.bs_u3s[4 * q + r];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        u3_b1[c] = a.b_out[c];
#pragma unroll
        for (int r = 0; r < 4; ++r) u3_w1[c][r] = a.w_out[c * 8 + 4 * q + r];
      }
    }
  };
  {
    RangeStoreS<S1_, IB> st{{lds + XU_U, T1}};
    if constexpr (!B3) zero_halo<16, S1_, T1, IB>(lds + XU_U, tid, NTH);
    if constexpr (D0T) {
      // D0T: nobody fetches skip rows here, so ALL sixteen waves share up2.same: wave w takes n-tiles 3 w .. 3 w + 2 (the matrix
      // time per SIMD is the same; four waves per SIMD instead of two hide each other's fragment reads and epilogues)
      bf16_t* const UP = reinterpret_cast<bf16_t*>(lds);
      const bf16_t* bp = b3c_lane_ptr<16, B3_U2_NC, 7>(P2, wave * 48, lane);
      f32x4 acc[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      auto& aw = aw_u2;
      b3c_mac_tiles_acc<16, B3_U2_NC, 7, 3>(bp, aw, acc);
      b3_load_a<16, 7>(a.af3_u2[0], 0, lane, aw);  // on its way under the refill
      __syncthreads();
      b3c_from_f32<16, B3_U2_NC, S1_, IB>(lds + A_SKIP1, P2, 3, tid, NTH);
      __syncthreads();  // skip 1 rests in the image: its fp32 rows give way to up2.same's output (pieces, U3T_QU)
      if (tid < 3 * 2) *reinterpret_cast<uint4*>(UP + (tid >> 1) * U3T_QU::PS + (tid & 1) * U3T_QU::CHS) = make_uint4(0u, 0u, 0u, 0u);  // column 0 = sample -1
      b3c_mac_tiles_acc<16, B3_U2_NC, 7, 3>(bp, aw, acc);
      u3_load_operands();
      {
        const int co0 = 4 * (lane >> 4);
        float biasv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) biasv[r] = a.c.bs[12][co0 + r];
#pragma unroll
        for (int j = 0; j < 3; ++j) {  // pieces, sample t at column t + 1 (zeros behind the signal: columns 752 .. 767)
          const int t = wave * 48 + j * 16 + (lane & 15);
          float v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = t < T1 ? fmaxf(acc[j][r] + biasv[r], 0.f) : 0.f;
          if (t + 1 < U3T_NCU) b3c_store4<16, U3T_NCU>(UP, t + 1, co0 >> 2, v);
        }
      }
      __syncthreads();
      WIN_DUMP(win_dump_b3c<16, U3T_NCU>(a, WD_U2SAME, UP, 1, T1, win, tid, NTH))
    } else if (wave >= 8) {
      float4 skq[NSKQ];
      const float* src = a.skip0 + (long)win * a.ws_s;
#pragma unroll
      for (int k = 0; k < NSKQ; ++k) {
        const int i = tid - 512 + k * 512, c = i / W0_Q, q = i - c * W0_Q;
        const int p = 4 * q + HALO - 4;
        skq[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < 8 * W0_Q && p + 3 < a.ls_s) skq[k] = *reinterpret_cast<const float4*>(src + (long)c * a.ls_s + p);
      }
      WIN_WARM_SCALAR(a.w_up, 16 * 7 * 8)
      if constexpr (B3) {
        __syncthreads();  // waves 0-7 are through with up2.convT's pieces
        b3c_from_f32<16, B3_U2_NC, S1_, IB>(lds + A_SKIP1, P2, 3, tid, NTH);
        __syncthreads();  // skip 1 rests in the image: its fp32 rows give way to up2.same's output
        zero_halo<16, S1_, T1, IB>(lds + XU_U, tid - 512, NTH - 512);
      }
      __syncthreads();  // up2.same done: its inputs give way to the level-0 rows (0-3 -> G0, 4-7 -> G1)
#pragma unroll
      for (int k = 0; k < NSKQ; ++k) {
        const int i = tid - 512 + k * 512, c = i / W0_Q, q = i - c * W0_Q;
        if (i < 8 * W0_Q)
          *reinterpret_cast<float4*>(((c < 4) ? lds + XU_G0 + c * W0_S : lds + XU_G1 + (c - 4) * W0_S) + 4 * q) = skq[k];
      }
    } else if constexpr (B3) {
      // wave w: n-tiles 6 w .. 6 w + 5 (48 for the 47 that hold samples), K = 2 halves x 4 steps of two taps x 16 channels
      const bf16_t* bp = b3c_lane_ptr<16, B3_U2_NC, 7>(P2, wave * 96, lane);
      f32x4 acc[6];
#pragma unroll
      for (int j = 0; j < 6; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      uint4 aw[B3Steps<16, 7>::STEPS * 3];
      b3_load_a<16, 7>(a.af3_u2[1], 0, lane, aw);
      b3c_mac_tiles_acc<16, B3_U2_NC, 7, 6>(bp, aw, acc);
      b3_load_a<16, 7>(a.af3_u2[0], 0, lane, aw);  // on its way under the refill
      __syncthreads();
      b3c_from_f32<16, B3_U2_NC, S1_, IB>(lds + A_SKIP1, P2, 3, tid, NTH);
      __syncthreads();
      b3c_mac_tiles_acc<16, B3_U2_NC, 7, 6>(bp, aw, acc);
      {
        const int co0 = 4 * (lane >> 4);
        float biasv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) biasv[r] = a.c.bs[12][co0 + r];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          const int t = wave * 96 + j * 16 + (lane & 15);
#pragma unroll
          for (int r = 0; r < 4; ++r) st(co0 + r, t, C_u2same::RELU ? fmaxf(acc[j][r] + biasv[r], 0.f) : acc[j][r] + biasv[r]);
        }
      }
      __syncthreads();
    } else {
      conv_lds<C_u2same, S1_, IB, S1_, TB, false, (C_u2same::NB < BDB_MAX_NB), ADEEP_LAYER(C_u2same)>(lds + A_SKIP1, lds + A_U2T, a.c.af[12], a.c.bs[12], T1, st, wave, NWV, lane);
      __syncthreads();
    }
    CORE_WIN_STAMP(stamp)
    ++stamp;
  }
#undef CORE_LAYER

  // ================= level-0 up path: up3.convT -> cat(skip0, .) -> up3.same -> 1x1 -> softmax =================
  if constexpr (D0T) {
    bf16_t* const l16 = reinterpret_cast<bf16_t*>(lds);
    const bf16_t* const UP = l16;
    bf16_t* const RU = l16 + U3T_RING_OFF;
    const int g = lane >> 4, n = lane & 15, ph = g >> 1, quad = g & 1;
    auto ring_at = [](const int c) { return (c & 1) * U3T_PL + (c >> 1) * 8; };
    // a producer's store of four channels of one column, all three pieces (+ the mirror entry behind the plane for columns 0 .. 7)
    auto ring_store = [&](bf16_t* const chunk, const int col, const int q, const float (&v)[4]) {
      const B3Quad s = b3_split4(v);
      bf16_t* const p = chunk + ring_at(col) + 4 * q;
      b3_put4(p, U3T_PS, s);
      if (col < 2 * U3T_MIR) b3_put4(p + U3T_PLN * 8, U3T_PS, s);
    };
    WIN_STAMP(23)
    const bool producer = wave >= 8;  // (uniform)
    const int wv = wave & 7;
    auto& aw = u3_aw;  // requested under up2.same (above)
    const f32x4 bv = u3_bv;
    auto& w1 = u3_w1;
    auto& b1 = u3_b1;
    auto& sk = u3_sk;
    const int sk_q = u3_skq, sk_s = u3_sks;
    if (tid < 96) {  // ring columns 512 .. 527 <-> samples -16 .. -1 of both chunks: zeros
      int tz = tid;
      asm volatile("" : "+v"(tz));  // (opaque: otherwise 4 tid and tid & 1 of the kernel's first lines are kept for this, in scratch)
      const int cp = tz >> 4, c = U3T_RING - 16 + (tz & 15);  // cp = piece * 2 + chunk
      *reinterpret_cast<uint4*>(RU + (cp >> 1) * U3T_PS + (cp & 1) * U3T_CH + ring_at(c)) = make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    WIN_STAMP(24)
    // producer: transposed conv item (m-tile wv & 1 = phases 2 (wv & 1) + ph, n-tile wv >> 1 of the tile's 64 level-1 samples)
    const int mphase = 2 * (wv & 1) + ph;
    int ct = mphase - 2 + 4 * (16 * (wv >> 1) + n);   // sample of this lane's output in tile 0 (tile j: + 256 j), >= -2
    ct = ct < 0 ? ct + U3T_RING : ct;                 // its ring column
    int cs = sk_s - 2;                                // skip sample of tile 0
    cs = cs < 0 ? cs + U3T_RING : cs;
    const bf16_t* up = UP + quad * U3T_QU::CHS + (16 * (wv >> 1) + n + ph) * 8;  // U column m + tap (sample m + tap - 1), tap = ph, chunk quad
    // consumer: n-tile wv of tile j - 1: samples 256 (j - 1) - 8 + 32 wv + 2 n + ph read the ring's samples .. - 3 + tap, tap = 2 step + ph, chunk quad
    int cc = U3T_RING - 11 + 32 * wv + 2 * n + ph;
    cc = cc >= U3T_RING ? cc - U3T_RING : cc;
    float* const yrow = a.y + (long)win * 3 * T0;
    // consumer: a tile's epilogue from its four BN + ReLU sums h (this lane's channel quad of sample t): Conv1d(8, 3, 1) -- the
    // other four channels come from the lane 16 further (the other channel quad) -- softmax, store.  It writes y only.
    auto u3_finish = [&](const int jt, const float (&h)[4]) {
      float z[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        float zz = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) zz = fmaf(w1[k][r], h[r], zz);
        const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(zz), __float_as_uint(zz), false, false);
        z[k] = (__uint_as_float(sw[0]) + __uint_as_float(sw[1])) + b1[k];  // rows (0, 1) and (2, 3): the pair's sum in both
      }
      const int t = U3T_TS * jt - 8 + 32 * wv + 2 * n + ph;
      if constexpr (DUMP) {
        if ((unsigned)t < (unsigned)T0) {
#pragma unroll
          for (int r = 0; r < 4; ++r) win_dump_row(a, WD_U3SAME, win, 4 * quad + r)[t] = h[r];
          if (quad == 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) win_dump_row(a, WD_LOGITS, win, k)[t] = z[k];
          }
        }
      }
      const float mx = fmaxf(z[0], fmaxf(z[1], z[2]));
      const float e0 = __expf(z[0] - mx), e1 = __expf(z[1] - mx), e2 = __expf(z[2] - mx);
      const float inv = __builtin_amdgcn_rcpf(e0 + e1 + e2);  // (1 ulp; the IEEE division is ten instructions on this issue-bound path)
      float y0 = e0 * inv, y1 = e1 * inv, y2 = e2 * inv;
      if (poisoned) y0 = y1 = y2 = __builtin_nanf("");
      if (quad == 0 && (unsigned)t < (unsigned)T0) yrow[t] = y0, yrow[T0 + t] = y1, yrow[2 * T0 + t] = y2;
    };
    float u3_h[4] = {0.f, 0.f, 0.f, 0.f};  // consumer: the sums of the tile whose epilogue is still owed
    // producer: up2.same's image is complete and static, so tile j + 1's fragments are fetched during phase j; the skip quads are
    // fetched TWO tiles ahead, even tiles into sk, odd ones into sk2 (one phase does not cover their trip to L2 once the MFMAs
    // no longer wait for a fragment read in front of them)
    uint4 u3_pb[3];
    float u3_sk2[4] = {0.f, 0.f, 0.f, 0.f};
    if (producer) {
      u3_fetch_skip(u3_sk2, 1, false);
#pragma unroll
      for (int pc = 0; pc < 3; ++pc) u3_pb[pc] = *reinterpret_cast<const uint4*>(up + pc * U3T_QU::PS);
    }
    auto u3_produce = [&](const int j) {  // tile j: MFMAs first, then everything that does not depend on them, then their epilogue
      f32x4 acc = bv;
      acc = b3_mac6(aw, u3_pb, acc);
      up += (U3T_TS / 4) * 8;
      if (j + 1 < U3T_TILES) {
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) u3_pb[pc] = *reinterpret_cast<const uint4*>(up + pc * U3T_QU::PS);
      }
      // the skip quad fetched two phases ago -> pieces, chunk 0
      float(&skj)[4] = (j & 1) ? u3_sk2 : sk;
      ring_store(RU, cs, sk_q, skj);
      if (j + 2 < U3T_TILES) u3_fetch_skip(skj, j + 2, U3T_TS * (j + 3) > T0);
      float o[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = fmaxf(acc[r], 0.f);
      if (j == 0 || U3T_TS * (j + 1) > T0) {  // (uniform) the tiles that meet the ends of the signal
        const int s = U3T_TS * j + mphase - 2 + 4 * (16 * (wv >> 1) + n);
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (unsigned)s < (unsigned)T0 ? o[r] : 0.f;
      }
      if constexpr (DUMP) {
        const int s = U3T_TS * j + mphase - 2 + 4 * (16 * (wv >> 1) + n);
        if ((unsigned)s < (unsigned)T0) {
#pragma unroll
          for (int r = 0; r < 4; ++r) win_dump_row(a, WD_U3T, win, 4 * quad + r)[s] = o[r];
        }
      }
      ring_store(RU + U3T_CH, ct, quad, o);
      ct += U3T_TS, cs += U3T_TS;
      ct = ct >= U3T_RING ? ct - U3T_RING : ct;
      cs = cs >= U3T_RING ? cs - U3T_RING : cs;
    };
    // consumer, phase j: the first K-step's fragments of tile j - 1 are requested, tile j - 2's epilogue runs while they are in
    // flight, the MFMAs follow (the other K-steps' reads among them).  (Requesting two or more K-steps ahead of the epilogue
    // spills at 120 registers.)
    auto u3_consume = [&](const int j) {
      const bf16_t* const rp0 = RU + quad * U3T_CH + ring_at(cc);  // K-step st: two columns = one plane entry further (mirrored: no wrap)
      uint4 b[4][3];
#pragma unroll
      for (int pc = 0; pc < 3; ++pc) b[0][pc] = *reinterpret_cast<const uint4*>(rp0 + pc * U3T_PS);
      if (j > 1) u3_finish(j - 2, u3_h);
      f32x4 sa = {0.f, 0.f, 0.f, 0.f}, sb = bv;
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        if (st > 0) {
#pragma unroll
          for (int pc = 0; pc < 3; ++pc) b[st][pc] = *reinterpret_cast<const uint4*>(rp0 + st * 8 + pc * U3T_PS);
        }
        sa = b3_mfma(sa, aw[st * 3 + 2], b[st][0]);
        sb = b3_mfma(sb, aw[st * 3 + 1], b[st][0]);
        sa = b3_mfma(sa, aw[st * 3 + 1], b[st][1]);
        sb = b3_mfma(sb, aw[st * 3 + 0], b[st][1]);
        sa = b3_mfma(sa, aw[st * 3 + 0], b[st][2]);
        sb = b3_mfma(sb, aw[st * 3 + 0], b[st][0]);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) u3_h[r] = fmaxf(sa[r] + sb[r], 0.f);  // BN + ReLU: all that crosses the barrier
      cc += U3T_TS;
      cc = cc >= U3T_RING ? cc - U3T_RING : cc;
    };
    // One loop per role, the same thirteen barriers in each (the branch is wave-uniform): what a role carries from phase to
    // phase -- the producers' fetched fragments and skip quads, the consumers' owed sums and 1 x 1 head -- then costs the other
    // role no registers.  One loop with both roles in its body spills 41 registers with these prefetches.
    if (producer) {
#pragma unroll
      for (int j = 0; j <= U3T_TILES; ++j) {
        if (j < U3T_TILES) u3_produce(j);
        lds_barrier();
      }
    } else {
#pragma unroll
      for (int j = 0; j <= U3T_TILES; ++j) {
        if (j > 0) u3_consume(j);
        lds_barrier();
        U3T_PHASE_STAMP(j)
      }
      u3_finish(U3T_TILES - 1, u3_h);  // the last tile's epilogue
    }
    WIN_STAMP(28)
  } else {
    float *G0 = lds + XU_G0, *G1 = lds + XU_G1, *U = lds + XU_U;
    WIN_STAMP(23)
    __syncthreads();
    WIN_STAMP(24)
    float aT[W_upT::CB * W_upT::TAPS], bT[4];  // A fragments of up3.convT (waves alternate over its two m-tiles)
    load_areg<W_upT>(a.af_t, wave & 1, lane, aT);
    load_biasreg<W_upT>(a.bs_t, wave & 1, lane, bT);
    f32x2 acc[4][4];
    if (vconv) {  // up3.same on cat([skip0, up3.convT]): the skip half first, then the convT rows take the skip rows' place
      valu_bias(acc, a.b_up);
      valu_conv7_r4<4, W0_S>(G0, as_weights(a.w_up), t0, acc);
      valu_conv7_r4<4, W0_S>(G1, as_weights(a.w_up + 4 * 28), t0, acc);
    }
    __syncthreads();
    WIN_STAMP(25)
    {  // up3.convT: ConvTranspose1d(16, 8, 7, stride 4) + BN + ReLU, crop [1:-2] and centre crop (t = o - 2), on the MFMA
      SplitRowStore st{G0, G1};
      conv_lds_areg<W_upT, S1_, IB, S1_, IB>(U, U, aT, bT, wave & 1, T1 + 1, st, wave >> 1, NWV / 2, lane);
    }
    __syncthreads();
    WIN_STAMP(26)
    if (vconv) {
      valu_conv7_r4<4, W0_S>(G0, as_weights(a.w_up + 8 * 28), t0, acc);
      valu_conv7_r4<4, W0_S>(G1, as_weights(a.w_up + 12 * 28), t0, acc);
    }
    WIN_STAMP(27)
    if (own) {  // BN + ReLU -> Conv1d(8, 3, 1) -> softmax over channels
      float z[3][4];
#pragma unroll
      for (int o = 0; o < 3; ++o)
#pragma unroll
        for (int r = 0; r < 4; ++r) z[o][r] = as_scalars(a.b_out)[o];
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v0 = fmaxf(acc[c][r].x, 0.f), v1 = fmaxf(acc[c][r].y, 0.f);
#pragma unroll
          for (int o = 0; o < 3; ++o)
            z[o][r] = fmaf(as_scalars(a.w_out)[o * 8 + 2 * c + 1], v1, fmaf(as_scalars(a.w_out)[o * 8 + 2 * c], v0, z[o][r]));
        }
      f32x4 y0, y1, y2;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float mx = fmaxf(z[0][r], fmaxf(z[1][r], z[2][r]));
        const float e0 = __expf(z[0][r] - mx), e1 = __expf(z[1][r] - mx), e2 = __expf(z[2][r] - mx);
        const float inv = 1.f / (e0 + e1 + e2);
        y0[r] = e0 * inv, y1[r] = e1 * inv, y2[r] = e2 * inv;
        if (poisoned) y0[r] = y1[r] = y2[r] = __builtin_nanf("");
      }
      float* y = a.y + (long)win * 3 * T0 + t0;
      if (t0 + 3 < T0) {  // dense rows of odd length: 4-byte aligned vector stores
        *reinterpret_cast<f32x4u*>(y) = y0;
        *reinterpret_cast<f32x4u*>(y + T0) = y1;
        *reinterpret_cast<f32x4u*>(y + 2 * T0) = y2;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (t0 + r < T0) y[r] = y0[r], y[T0 + r] = y1[r], y[2 * T0 + r] = y2[r];
      }
    }
    WIN_STAMP(28)
  }
  if (clk && tid == 0) clk[(long)win * 32 + 17] = wall_clock64();
#undef WIN_STAMP
#undef CORE_WIN_STAMP
#undef D0T_PHASE_STAMP
#undef U3T_PHASE_STAMP
#undef WIN_DUMP
#undef WIN_WARM_SCALAR
}

}  // namespace

void pn_launch_window(PnForm form, bool dump, const WindowArgs& a, int B, hipStream_t s) {
  const dim3 grid(B), block(1024);
  const size_t lds = CORE_LDS_FLOATS * sizeof(float);
  if (dump) hipLaunchKernelGGL((pn_window_kernel<PnForm::Default, true>), grid, block, lds, s, a);
  else if (form == PnForm::Default) hipLaunchKernelGGL(pn_window_kernel<PnForm::Default>, grid, block, lds, s, a);
  else if (form == PnForm::Level0Valu) hipLaunchKernelGGL(pn_window_kernel<PnForm::Level0Valu>, grid, block, lds, s, a);
  else hipLaunchKernelGGL(pn_window_kernel<PnForm::Fp32Core>, grid, block, lds, s, a);
}
void pn_register_window(Net& net, bool dump) {
  const size_t lds = CORE_LDS_FLOATS * sizeof(float);
  net.extra_kernels.push_back({reinterpret_cast<const void*>(&pn_window_kernel<PnForm::Fp32Core>), lds});
  net.extra_kernels.push_back({reinterpret_cast<const void*>(&pn_window_kernel<PnForm::Level0Valu>), lds});
  net.extra_kernels.push_back({reinterpret_cast<const void*>(&pn_window_kernel<PnForm::Default>), lds});
  if (dump) net.extra_kernels.push_back({reinterpret_cast<const void*>(&pn_window_kernel<PnForm::Default, true>), lds});
}

}  // namespace vp
