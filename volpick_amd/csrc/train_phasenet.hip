// PhaseNet training step (BASELINE config 5): forward in training mode (batch
// statistics), vector cross entropy, backward, Adam -- the arithmetic of one
// PhaseNetLit.training_step + optimizer.step of the reference
// (the reference's volpick/model/models.py:34-51 loss, :160-164 shared_step/training_step,
// :177-185 Adam; the SeisBench PhaseNet module it wraps is restated in oracle/models.py).
//
// Layout: every layer keeps z (raw conv output), a = relu(bn(z)) and the gradients gz, ga as haloed
// [B][C][ls] rows.  Forward convs and input-gradient convs run on conv_mfma_kernel with fragments
// re-packed from the live weights every step (gather_pack_kernel, index maps built once with the
// inference packers); weight gradients on wgrad_kernel; Adam and its state in train_optim.hip; everything else in train_kernels.h.
// ConvTranspose outputs are kept at full length (4 L + 3): BatchNorm sees the samples the U-Net
// crops away, and they receive gradient through the batch statistics.
//
// This file, top to bottom: the table of the 18 layers (LayerTable: one row per layer, its three Cfg types), the plan
// built from it (build_plan: everything else follows from a row's kind and level), the Trainer and its device memory
// (DevArray, upload), the step as a sequence of phases (forward_backward) with the weight gradients' side queue
// (WgradQueue), and the C entry points.
#include <hip/hip_ext.h>

#include <cmath>
#include <memory>

#include "batchgen.h"
#include "conv_mfma.h"
#include "conv_train_b16.h"
#include "train_kernels.h"
#include "train_optim.h"

namespace vp {
namespace {

constexpr int T0 = 3001, T1 = 751, T2 = 188, T3 = 47, T4 = 12;
constexpr int NLAYER = 18;
constexpr int LEN[5] = {T0, T1, T2, T3, T4};  // samples, channels of a level
constexpr int CH[5] = {8, 16, 32, 64, 128};
constexpr int PADL[4] = {3, 2, 1, 2};          // left padding of the stride-4 conv that leaves a level

// ---- the layers ------------------------------------------------------------------------------------------------------
// A layer is a kind and a level.  SAME / DOWN: the stride-1 and the stride-4 conv of down_branch.<level>; CONVT / UP_SAME:
// the ConvTranspose up to <level> and the conv over concat(skip, up) there, up_branch.<3 - level>.
enum Kind { INC, SAME, DOWN, CONVT, UP_SAME };
// forward order: 0 inc, 1+2i down{i}.same, 2+2i down{i}.down (i<4), 9 down4.same, 10+2j up{j}.convT, 11+2j up{j}.same
constexpr int layer_index(Kind k, int lv) {
  return k == INC ? 0 : k == SAME ? (lv < 4 ? 1 + 2 * lv : 9) : k == DOWN ? 2 + 2 * lv : (k == CONVT ? 10 : 11) + 2 * (3 - lv);
}
constexpr int layer_cout(Kind k, int lv) { return k == INC ? 8 : CH[lv]; }
constexpr int layer_cin(Kind k, int lv) {
  return k == INC ? 3 : k == SAME ? (lv ? CH[lv - 1] : 8) : k == DOWN ? CH[lv] : k == CONVT ? CH[lv + 1] : 2 * CH[lv];
}

// One row of the table: where the layer stands and the Cfg types of its forward (F), input-gradient (G, void for the
// first layer) and weight-gradient (W) launches.  bind_layer checks every Cfg figure that kind and level decide.
template <int LI_, Kind KIND_, int LV_, class F_, class G_, class W_>
struct LayerCfg {
  static constexpr int LI = LI_, LV = LV_;
  static constexpr Kind KIND = KIND_;
  using F = F_;
  using G = G_;
  using W = W_;
};
template <class... R>
struct LayerList {};

//                    CIN1 CIN2 COUT P TAPS SN IN_OFF OUT_OFF WM WN NW    (BF = 1: rows stored as bf16, conv_mfma.h)
// (no activation: BatchNorm needs the raw output)
template <int BF, int... V>
using TC = ConvCfg<V..., 0, EPI_STORE, 0, 0, BF>;
//                     LO HI1 HI2 K S NWAVE TT [WB windows per item]
// (level-0 stride-1 layers, bf16 rows: 512-sample chunks -- half the barriers per byte; same-box 1.394 -> 1.384 ms per step)
constexpr int W0TT = 512;

// Input gradients: conv(k7, same) -> conv with the flipped, transposed kernel; conv(k7, s4, left pad p) ->
// ConvTranspose(k7, s4) of the same kernel, output shifted by -p; ConvTranspose(k7, s4) -> conv(k7, s4, no pad) of the
// same kernel over the full-length gradient.
// (No layer keeps the fp32 form for its matrix time any more: with two K-steps of fragments in flight up0.same and its input
// gradient -- 57 k weights per 48-column tile, six bytes each as pieces instead of four -- were 1-7 us slower on the bf16
// pipe; with six in flight they are even.)
// clang-format off
template <int BF>
using LayerTable = LayerList<
    LayerCfg<0, INC, 0,       TC<BF, 3, 0, 8, 2, 8, 2, -3, 0, 1, 4, 8>,      void,                                          WgradCfg<8, 3, 0, 7, 1, 8, BF ? W0TT : 256>>,
    LayerCfg<1, SAME, 0,      TC<BF, 8, 0, 8, 2, 8, 2, -3, 0, 1, 4, 8>,      TC<BF, 8, 0, 8, 2, 8, 2, -3, 0, 1, 4, 8>,      WgradCfg<8, 8, 0, 7, 1, 8, BF ? W0TT : 256>>,
    LayerCfg<2, DOWN, 0,      TC<BF, 8, 0, 8, 2, 11, 8, -3, 0, 1, 4, 2>,     TC<BF, 8, 0, 8, 4, 2, 1, -1, -3, 2, 2, 4>,     WgradCfg<8, 8, 0, 7, 4, 8, 256>>,
    LayerCfg<3, SAME, 1,      TC<BF, 8, 0, 16, 1, 7, 1, -3, 0, 1, 4, 4>,     TC<BF, 16, 0, 8, 2, 8, 2, -3, 0, 1, 4, 2>,     WgradCfg<16, 8, 0, 7, 1, 8, 256>>,
    LayerCfg<4, DOWN, 1,      TC<BF, 16, 0, 16, 1, 7, 4, -2, 0, 1, 4, 1>,    TC<BF, 16, 0, 16, 4, 2, 1, -1, -2, 4, 1, 4>,   WgradCfg<16, 16, 0, 7, 4, 8, 96>>,
    LayerCfg<5, SAME, 2,      TC<BF, 16, 0, 32, 1, 7, 1, -3, 0, 2, 2, 3>,    TC<BF, 32, 0, 16, 1, 7, 1, -3, 0, 1, 4, 3>,    WgradCfg<32, 16, 0, 7, 1, 8, 192>>,
    LayerCfg<6, DOWN, 2,      TC<BF, 32, 0, 32, 1, 7, 4, -1, 0, 2, 2, 1>,    TC<BF, 32, 0, 32, 4, 2, 1, -1, -1, 4, 1, 3>,   WgradCfg<32, 32, 0, 7, 4, 4, 48>>,
    LayerCfg<7, SAME, 3,      TC<BF, 32, 0, 64, 1, 7, 1, -3, 0, 4, 1, 3>,    TC<BF, 64, 0, 32, 1, 7, 1, -3, 0, 2, 2, 2>,    WgradCfg<64, 32, 0, 7, 1, 8, 48>>,
    LayerCfg<8, DOWN, 3,      TC<BF, 64, 0, 64, 1, 7, 4, -2, 0, 4, 1, 1>,    TC<BF, 64, 0, 64, 4, 2, 1, -1, -2, 4, 1, 1>,   WgradCfg<64, 64, 0, 7, 4, 16, 12, 2>>,
    LayerCfg<9, SAME, 4,      TC<BF, 64, 0, 128, 1, 7, 1, -3, 0, 4, 1, 1>,   TC<BF, 128, 0, 64, 1, 7, 1, -3, 0, 4, 1, 1>,   WgradCfg<128, 64, 0, 7, 1, 16, 12, 4>>,
    LayerCfg<10, CONVT, 3,    TC<BF, 128, 0, 64, 4, 2, 1, -1, 0, 4, 1, 1>,   TC<BF, 64, 0, 128, 1, 7, 4, 0, 0, 4, 1, 1>,    WgradCfg<128, 64, 0, 7, 4, 16, 12, 2>>,
    LayerCfg<11, UP_SAME, 3,  TC<BF, 64, 64, 64, 1, 7, 1, -3, 0, 4, 1, 3>,   TC<BF, 64, 0, 128, 1, 7, 1, -3, 0, 4, 1, 3>,   WgradCfg<64, 64, 64, 7, 1, 16, 48>>,
    LayerCfg<12, CONVT, 2,    TC<BF, 64, 0, 32, 4, 2, 1, -1, 0, 4, 1, 3>,    TC<BF, 32, 0, 64, 1, 7, 4, 0, 0, 4, 1, 3>,     WgradCfg<64, 32, 0, 7, 4, 8, 48>>,
    LayerCfg<13, UP_SAME, 2,  TC<BF, 32, 32, 32, 1, 7, 1, -3, 0, 2, 2, 3>,   TC<BF, 32, 0, 64, 1, 7, 1, -3, 0, 2, 2, 3>,    WgradCfg<32, 32, 32, 7, 1, 8, 96>>,
    LayerCfg<14, CONVT, 1,    TC<BF, 32, 0, 16, 4, 2, 1, -1, 0, 4, 1, 4>,    TC<BF, 16, 0, 32, 1, 7, 4, 0, 0, 2, 2, 3>,     WgradCfg<32, 16, 0, 7, 4, 8, 96>>,
    LayerCfg<15, UP_SAME, 1,  TC<BF, 16, 16, 16, 1, 7, 1, -3, 0, 1, 4, 4>,   TC<BF, 16, 0, 32, 1, 7, 1, -3, 0, 2, 2, 4>,    WgradCfg<16, 16, 16, 7, 1, 8, 256>>,
    LayerCfg<16, CONVT, 0,    TC<BF, 16, 0, 8, 4, 2, 1, -1, 0, 2, 2, 4>,     TC<BF, 8, 0, 16, 1, 7, 4, 0, 0, 1, 4, 4>,      WgradCfg<16, 8, 0, 7, 4, 8, 256>>,
    LayerCfg<17, UP_SAME, 0,  TC<BF, 8, 8, 8, 2, 8, 2, -3, 0, 1, 4, 8>,      TC<BF, 8, 0, 16, 1, 7, 1, -3, 0, 1, 4, 8>,     WgradCfg<8, 8, 8, 7, 1, 8, BF ? W0TT : 256>>>;
// clang-format on

struct ConvOp {
  bool used = false;
  ConvGeom g{};
  int (*launch)(const ConvArgs&, int, hipStream_t) = nullptr;
  // bf16 rows, filters of >= 7 taps: the bf16-MFMA form (conv_train_b16.h); its A operand is cut from the fp32 fragments
  int (*launch_b16)(const ConvArgs&, const uint4*, float*, int, hipStream_t) = nullptr;
  int tn = 0, cout = 0;  // columns per tile / output channels (the statistics a forward launch leaves: [cout][tiles x B][2])
  size_t a3_n = 0, a3_off = 0;  // uint4 words of the operand / its place in Trainer::frag3
  const void* kernel = nullptr;
  size_t lds_bytes = 0;
  int src1 = -1, src2 = -1, dst = -1;
  int cols = 0, l_out = 0;
  size_t frag_off = 0;
  long bias_off = -1;  // offset of a real bias in the weight blob, -1 = zeros
};

struct WgradOp {
  int (*launch)(const WgradArgs&, int, hipStream_t) = nullptr;
  const void* kernel[2] = {nullptr, nullptr};  // wgrad_bf16_kernel for an even / odd tap offset, and its dynamic LDS
  size_t lds_bytes = 0;
  int lo = -1, hi1 = -1, hi2 = -1;
  int Ln = 0, off = 0, TT = 0, WB = 1, out_n = 0;
  long grad_off = 0;
  size_t partial_off = 0;  // slice of the shared partial buffer (all layers are folded by one launch at the end)
};

struct BnOp {
  int z = -1, a = -1, gz = -1;
  int ga1 = -1, ga1_ch = 0, ga2 = -1, ga2_ch = 0;
  int C = 0, Lz = 0, La = 0, crop = 0;
  long gamma_off = 0, beta_off = 0, rm_off = 0, rv_off = 0;
  size_t stats_off = 0;
};

struct Layer {
  Kind kind = INC;
  int lv = 0;
  std::string name;
  ConvOp fwd, dgrad;
  BnOp bn;
  WgradOp wg;
};

template <class Cfg>
void set_conv(ConvOp* op) {
  op->used = true;
  op->g = Cfg::geom();
  op->launch = &launch_conv<Cfg>;
  op->kernel = reinterpret_cast<const void*>(&conv_mfma_kernel<Cfg>);
  op->lds_bytes = Cfg::LDS_FLOATS * sizeof(float);
  if constexpr (Cfg::BF16 && (Cfg::TAPS >= 7 || (Cfg::TAPS == 2 && Cfg::CB % 4 == 0))) {
    op->launch_b16 = &launch_conv_b16<Cfg>;
    op->a3_n = ConvB16<Cfg>::A_UINT4;
    op->tn = Cfg::TN;
    op->cout = Cfg::COUT;
  }
}

template <class Cfg, int BF>
void set_wgrad(WgradOp* op) {
  // bf16 rows: exact products on the bf16 matrix cores (wgrad_bf16_kernel).  (Round 4 kept the four deepest layers -- >= 4096
  // channel pairs, <= 48 samples per row -- on the fp32-MFMA kernel: with 256 partial rows per tensor their cost was the
  // 115-230 KB every workgroup writes.  With the rows capped by bytes (wg_rows_cap: 64 workgroups for 57 k weights) the fp32
  // form is bound by its matrix time on those few CUs: up0.same 99-118 us against 51 here; the step itself does not move.)
  if constexpr (BF != 0) {
    op->launch = &launch_wgrad_bf16<Cfg>;
    op->kernel[0] = reinterpret_cast<const void*>(&wgrad_bf16_kernel<Cfg, 0>);
    op->kernel[1] = reinterpret_cast<const void*>(&wgrad_bf16_kernel<Cfg, 1>);
    op->lds_bytes = (size_t)WgradB<Cfg>::LDS_ELEMS * 2;
  } else {
    op->launch = &launch_wgrad<Cfg>;
  }
  op->TT = Cfg::TT;
  op->WB = Cfg::WB;
  op->out_n = Cfg::OUT;
}

// The launchers of a row, and the check that its Cfg types are those of a layer of this kind at this level: channels,
// stride (SN = stride x P phases; a ConvTranspose as four phases of two taps) and, for the stride-4 conv, the padding.
template <class R, int BF>
void bind_layer(Layer* Ls) {
  using F = typename R::F;
  using G = typename R::G;
  using W = typename R::W;
  constexpr Kind K = R::KIND;
  constexpr int LV = R::LV, COUT = layer_cout(K, LV), CIN = layer_cin(K, LV), STRIDE = K == DOWN ? 4 : 1;
  static_assert(R::LI == layer_index(K, LV), "the row's index is not that of its kind and level");
  static_assert(F::COUT == COUT && F::CIN == CIN && (K != UP_SAME || F::CIN1 == COUT), "forward conv: channels");
  static_assert(K == CONVT ? F::P == 4 && F::TAPS == 2 && F::SN == 1 : F::SN == STRIDE * F::P, "forward conv: stride");
  Layer& L = Ls[R::LI];
  L.kind = K;
  L.lv = LV;
  set_conv<F>(&L.fwd);
  if constexpr (K != INC) {
    static_assert(G::CIN == COUT && G::COUT == CIN && G::CIN2 == 0, "input gradient: channels");
    static_assert(K == DOWN    ? G::P == 4 && G::TAPS == 2 && G::SN == 1 && G::OUT_OFF == -PADL[LV < 4 ? LV : 0]
                  : K == CONVT ? G::P == 1 && G::SN == 4
                               : G::SN == G::P,
                  "input gradient: stride");
    set_conv<G>(&L.dgrad);
  } else {
    static_assert(std::is_void<G>::value, "the first layer has no input gradient");
  }
  // ConvTranspose: lo = layer input, hi = gz
  static_assert(W::K == 7 && W::LO == (K == CONVT ? CIN : COUT) && W::HI == (K == CONVT ? COUT : CIN) && W::S == (K == CONVT ? 4 : STRIDE) &&
                    (K == UP_SAME ? W::HI1 == COUT : W::HI2 == 0),
                "weight gradient: channels, stride");
  set_wgrad<W, BF>(&L.wg);
}
template <int BF, class... R>
void bind_layers(LayerList<R...>, Layer* Ls) {
  static_assert(sizeof...(R) == NLAYER && ((1u << R::LI) | ...) == (1u << NLAYER) - 1, "one row per layer");
  (bind_layer<R, BF>(Ls), ...);
}

// dense (B, C, T) -> haloed rows
__global__ __launch_bounds__(256) void load_rows_kernel(const float* __restrict__ x, Rows r, int C, int T) {
  const int c = blockIdx.y, b = blockIdx.z;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < T) r.p[(long)b * r.ws + (long)c * r.ls + HALO + t] = x[((long)b * C + c) * T + t];
}
// the same into bf16 rows, an even-aligned pair per thread: grid (ceil(T / 512), C, B)
__global__ __launch_bounds__(256) void load_rows_bf16_kernel(const float* __restrict__ x, Rows r, int C, int T) {
  const int c = blockIdx.y, b = blockIdx.z;
  const int t = 2 * (blockIdx.x * 256 + threadIdx.x);
  if (t < T) {
    const float* xp = x + ((long)b * C + c) * T + t;
    Elem<bf16_t>::store2(r.row<bf16_t>(b, c) + t, xp[0], t + 1 < T ? xp[1] : 0.f);
  }
}

// What differs between fp32 and bf16 rows outside the convs, chosen once with the plan (the convs' and weight gradients'
// launchers come with the table's BF).  The BatchNorm passes come per crop of the ConvTranspose layers: 0, 1 or 2 samples.
using BnKernel = void (*)(BnArgs);
struct RowKernels {
  void (*load_rows)(const float*, Rows, int, int) = nullptr;
  int load_span = 0;  // samples per workgroup
  BnKernel bn_stats = nullptr, bn_apply[3] = {}, bn_bwd_partial[3] = {}, bn_bwd_apply[3] = {};
  void (*head)(HeadArgs2) = nullptr;
  int head_span = 0;
  void (*channel_sum)(Rows, int, int, int, double*) = nullptr;
};
template <class T>
RowKernels row_kernels() {
  RowKernels k;
  if constexpr (sizeof(T) == 2) {
    k.load_rows = load_rows_bf16_kernel, k.load_span = 512;
    k.head = head_fwd_bwd_pair_kernel<bf16_t, 4>, k.head_span = 1024;
  } else {
    k.load_rows = load_rows_kernel, k.load_span = 256;
    k.head = head_fwd_bwd_kernel, k.head_span = 256;
  }
  k.bn_stats = bnv_stats_partial_kernel<T>;
  k.bn_apply[0] = bnv_apply_kernel<T, 0>, k.bn_apply[1] = bnv_apply_kernel<T, 1>, k.bn_apply[2] = bnv_apply_kernel<T, 2>;
  k.bn_bwd_partial[0] = bnv_bwd_partial_kernel<T, 0>, k.bn_bwd_partial[1] = bnv_bwd_partial_kernel<T, 1>, k.bn_bwd_partial[2] = bnv_bwd_partial_kernel<T, 2>;
  k.bn_bwd_apply[0] = bnv_bwd_apply_kernel<T, 0>, k.bn_bwd_apply[1] = bnv_bwd_apply_kernel<T, 1>, k.bn_bwd_apply[2] = bnv_bwd_apply_kernel<T, 2>;
  k.channel_sum = channel_sum_partial_v_kernel<T>;
  return k;
}

}  // namespace

struct Trainer {
  int device = 0, max_batch = 0;
  int launches = 0;   // kernel launches of the step enqueued last (vp_train_launch_count)
  bool bf16 = false;  // activation / gradient rows stored as bfloat16 (weights, gradients, statistics, Adam: fp32)
  int esize = 4;      // bytes per row element
  RowKernels rk;
  hipStream_t stream = nullptr;
  // The weight gradients run on a stream of their own: wgrad of layer L needs gz of L and the activations below it, nothing
  // downstream needs its result before the fold at the end of the step, and the backward chain (BatchNorm backward -> input
  // gradient -> next layer's BatchNorm backward) is a string of short launches that leave most of the chip idle in the deep
  // layers.  Events order the two: ev_gz[L] (gz of L complete) -> wgrad of L; ev_wg (all weight gradients) -> fold + Adam.
  hipStream_t stream_wg = nullptr;
  hipEvent_t ev_gz[NLAYER] = {}, ev_wg = nullptr, ev_wg1 = nullptr;  // ev_wg1: every weight gradient but the first layer's
  std::vector<Tensor> tensors;
  std::vector<Layer> layers;
  std::map<std::string, long> poff;  // parameter name -> offset in the flat blob
  std::map<std::string, size_t> psize;
  size_t n_params = 0;
  // device memory
  DevArray<char> arena;  // activation / gradient tensors
  OptimState opt;        // weights, gradients, Adam state; the EMA is allocated by vp_train_set_ema
  // behind the last reader of a step's x / y (the head kernel), a ring over the steps in flight:
  // vp_train_wait_inputs_consumed (the latest), vp_train_inputs_consumed_upto (which steps are past it)
  static constexpr int EV_RING = 8;
  hipEvent_t ev_inputs[EV_RING] = {};
  long long ev_inputs_seq[EV_RING] = {-1, -1, -1, -1, -1, -1, -1, -1};
  long long seq = 0;  // steps enqueued so far
  DevArray<int> frag_idx;
  DevArray<float> frag;
  size_t frag_n = 0;
  DevArray<float> zeros;  // 256 zero floats (bias of bias-free convs)
  DevArray<float> stats;
  DevArray<double> bn_partial;
  DevArray<float> conv_stat;  // BatchNorm sums a forward bf16-MFMA conv leaves per workgroup (one layer at a time)
  DevArray<uint4> frag3;      // three-piece A operands of the bf16-MFMA convs, cut from `frag` every step
  ConvB16PackJobs b16_jobs{};
  int b16_blocks = 0;
  DevArray<float> wg_partial;
  DevArray<double> head_partial;
  DevArray<double> head_sums;   // [28] + loss at [28]
  DevArray<double> head_stage;  // [64][28]
  DevArray<float> x_dev, y_dev;  // staging for host inputs, and where vp_train_step_bank generates its batch
  RowRing plan_rows;             // vp_train_step_bank(_aug)'s rows: slot seq % EV_RING, free again at ev_inputs of that slot
                                 // (the bare ring, not a StagingRing: the step events below exist anyway and free the slots too)
  DevArray<float> p_dev;         // predictions of the last step
  float bn_eps = 1e-3f, bn_momentum = 0.1f, loss_eps = 1e-5f;
  int t_x = -1, t_ga_last = -1;
  std::vector<int> frag_idx_host;

  int add_tensor(const std::string& name, int C, int L) {
    Tensor t;
    t.name = name;
    t.C = C;
    t.L = L;
    // rows are walked in 8-sample vectors, a cropped operand one vector further (train_kernels.h load8_at)
    t.need = HALO + round_up(L, 8) + 16;
    tensors.push_back(t);
    return (int)tensors.size() - 1;
  }
  void need(int id, int phys) {
    if (id >= 0 && tensors[id].need < phys) tensors[id].need = phys;
  }
  Rows rows(int id, int ch = 0) const {
    const Tensor& t = tensors[id];  // (t.p is a byte address in disguise when the rows are bf16)
    return Rows{reinterpret_cast<float*>(reinterpret_cast<char*>(t.p) + (long)ch * t.ls * esize), t.ls, (long)t.win_stride()};
  }
  ~Trainer() {  // (the device arrays free themselves)
    if (stream) (void)hipStreamDestroy(stream);
    if (stream_wg) (void)hipStreamDestroy(stream_wg);
    for (hipEvent_t e : ev_gz)
      if (e) (void)hipEventDestroy(e);
    if (ev_wg) (void)hipEventDestroy(ev_wg);
    if (ev_wg1) (void)hipEventDestroy(ev_wg1);
    for (hipEvent_t e : ev_inputs)
      if (e) (void)hipEventDestroy(e);
  }
};

namespace {

// a launch of the step: counted for vp_train_launch_count
#define TRL(...)                     \
  do {                               \
    ++tr.launches;                   \
    hipLaunchKernelGGL(__VA_ARGS__); \
  } while (0)

// index map of one conv's packed fragments: pack "weights" whose values are their own flat index + 1
std::vector<int> to_index(const std::vector<float>& packed) {
  std::vector<int> out(packed.size());
  for (size_t i = 0; i < packed.size(); ++i) out[i] = (int)(packed[i] + 0.5f);
  return out;
}
std::vector<float> index_weights(long off, size_t n) {
  std::vector<float> w(n);
  for (size_t i = 0; i < n; ++i) w[i] = (float)(off + (long)i + 1);  // exact below 2^24
  return w;
}
// W[co][ci][K] -> W'[ci][co][K] with the taps reversed (input gradient of a stride-1 "same" conv)
std::vector<float> flip_transpose(const std::vector<float>& w, int cout, int cin, int K) {
  std::vector<float> o(w.size());
  for (int co = 0; co < cout; ++co)
    for (int ci = 0; ci < cin; ++ci)
      for (int k = 0; k < K; ++k) o[((size_t)ci * cout + co) * K + (K - 1 - k)] = w[((size_t)co * cin + ci) * K + k];
  return o;
}

void append_frag(Trainer& tr, ConvOp* op, const std::vector<float>& amat) {
  const std::vector<int> idx = to_index(pack_afrag(amat, op->g.M(), op->g.cinp(), op->g.taps));
  op->frag_off = tr.frag_idx_host.size();
  tr.frag_idx_host.insert(tr.frag_idx_host.end(), idx.begin(), idx.end());
}

// Everything of the plan that is not a Cfg type, from each layer's kind and level.
int build_plan(Trainer& tr) {
  const ParamDesc* table;
  const int np = param_table(VP_MODEL_PHASENET, &table);
  long off = 0;
  for (int i = 0; i < np; ++i) {
    tr.poff[table[i].name] = off;
    tr.psize[table[i].name] = table[i].size;
    off += (long)table[i].size;
  }
  tr.n_params = (size_t)off;
  tr.layers.resize(NLAYER);
  Layer* Ls = tr.layers.data();
  if (tr.bf16) {  // the one place the row type is asked for
    bind_layers<1>(LayerTable<1>{}, Ls);
    tr.rk = row_kernels<bf16_t>();
  } else {
    bind_layers<0>(LayerTable<0>{}, Ls);
    tr.rk = row_kernels<float>();
  }
  auto P = [&](const std::string& n) { return tr.poff.at(n); };

  // ---- names, BatchNorm, the tensors z, a, gz ---------------------------------------------
  std::string conv_name[NLAYER];  // the conv's parameters: inc, down_branch.<i>.0 / .2, up_branch.<j>.0 / .2 (its BatchNorm: .1 / .3)
  tr.t_x = tr.add_tensor("x", 3, T0);
  for (int li = 0; li < NLAYER; ++li) {
    Layer& L = Ls[li];
    const int lv = L.lv;
    const bool up = L.kind == CONVT || L.kind == UP_SAME, second = L.kind == DOWN || L.kind == UP_SAME;
    const std::string n = std::to_string(up ? 3 - lv : lv), branch = std::string(up ? "up" : "down") + "_branch." + n;
    L.name = L.kind == INC ? "inc" : (up ? "up" : "down") + n + (L.kind == DOWN ? ".down" : L.kind == CONVT ? ".convT" : ".same");
    conv_name[li] = L.kind == INC ? "inc" : branch + (second ? ".2" : ".0");
    const std::string bn = L.kind == INC ? "in_bn" : branch + (second ? ".3" : ".1");
    BnOp& b = L.bn;
    b.C = layer_cout(L.kind, lv);
    b.La = LEN[L.kind == DOWN ? lv + 1 : lv];                   // what the next layer reads
    b.Lz = L.kind == CONVT ? 4 * LEN[lv + 1] + 3 : b.La;          // (a ConvTranspose output stays at full length)
    b.crop = L.kind == CONVT ? 1 + ((b.Lz - 3) - b.La) / 2 : 0;  // x[:, :, 1:-2] then the centre crop to the skip length
    b.gamma_off = P(bn + ".weight");
    b.beta_off = P(bn + ".bias");
    b.rm_off = P(bn + ".running_mean");
    b.rv_off = P(bn + ".running_var");
    b.z = tr.add_tensor(L.name + ".z", b.C, b.Lz);
    b.a = tr.add_tensor(L.name + ".a", b.C, b.La);
    b.gz = tr.add_tensor(L.name + ".gz", b.C, b.Lz);
  }
  // ---- gradient-of-activation tensors -------------------------------------------------------
  int gcat[4], gskip[4];  // by level
  for (int lv = 3; lv >= 0; --lv) {
    gcat[lv] = tr.add_tensor("up" + std::to_string(3 - lv) + ".gcat", 2 * CH[lv], LEN[lv]);  // d(concat(skip, up)) of the up path's conv at lv
    gskip[lv] = tr.add_tensor("down" + std::to_string(lv) + ".gskip", CH[lv], LEN[lv]);      // from down{lv}.down
  }
  for (Layer& L : tr.layers) {
    BnOp& b = L.bn;
    if (L.kind == SAME && L.lv < 4) {  // skips: from the up path (first half of gcat) + from the strided conv below
      b.ga1 = gcat[L.lv];
      b.ga2 = gskip[L.lv];
    } else if (L.kind == CONVT) {  // convT outputs: second half of gcat
      b.ga1 = gcat[L.lv];
      b.ga1_ch = CH[L.lv];
    } else {  // a single producer: the input gradient of the next layer, or the head for the last
      b.ga1 = tr.add_tensor(L.name + ".ga", b.C, b.La);
    }
  }
  tr.t_ga_last = Ls[NLAYER - 1].bn.ga1;

  // ---- convolutions: forward, weight gradient, input gradient -------------------------------
  auto W = [&](int li) { return index_weights(P(conv_name[li] + ".weight"), tr.psize.at(conv_name[li] + ".weight")); };
  auto cols_of = [](const ConvOp& op) { return (op.l_out + op.g.P - 1) / op.g.P; };
  for (int li = 0; li < NLAYER; ++li) {
    Layer& L = Ls[li];
    const Kind k = L.kind;
    const int lv = L.lv, cin = layer_cin(k, lv), cout = layer_cout(k, lv);
    const int below = li ? Ls[li - 1].bn.a : tr.t_x;
    ConvOp& f = L.fwd;
    f.src1 = k == UP_SAME ? Ls[layer_index(SAME, lv)].bn.a : below;  // concat(skip, up)
    f.src2 = k == UP_SAME ? below : -1;
    f.dst = L.bn.z;
    f.l_out = L.bn.Lz;
    f.cols = cols_of(f);
    append_frag(tr, &f, k == CONVT ? amat_convT_k7s4(W(li).data(), cin, cout, f.g.cinp(), nullptr)
                                   : amat_conv(W(li).data(), cout, cin, 7, k == DOWN ? 4 : 1, f.g.P, f.g.cinp(), nullptr));
    if (k == INC) f.bias_off = P("inc.bias");
    WgradOp& g = L.wg;
    g.grad_off = P(conv_name[li] + ".weight");
    if (k == CONVT) {  // ConvTranspose: lo = layer input, hi = gz
      g.lo = f.src1, g.hi1 = L.bn.gz, g.Ln = LEN[lv + 1], g.off = 0;
    } else {
      g.lo = L.bn.gz, g.hi1 = f.src1, g.hi2 = f.src2, g.Ln = L.bn.Lz, g.off = k == DOWN ? -PADL[lv] : -3;
    }
  }
  // (fragments in the order they have always had: stride-1, stride-4, ConvTranspose)
  for (Kind pass : {SAME, DOWN, CONVT})
    for (int li = 1; li < NLAYER; ++li) {
      Layer& L = Ls[li];
      const Kind k = L.kind;
      if ((k == UP_SAME ? SAME : k) != pass) continue;
      const int lv = L.lv, cin = layer_cin(k, lv), cout = layer_cout(k, lv);
      ConvOp& d = L.dgrad;
      d.src1 = L.bn.gz;
      if (k == DOWN) {
        // dgrad of a stride-4 conv W[C][C][7] with left pad PADL: transposed conv of gz, output index shifted by -PADL
        d.dst = gskip[lv];
        d.l_out = LEN[lv];
        d.cols = (d.l_out - 1 + PADL[lv]) / 4 + 1;
        append_frag(tr, &d, amat_convT_k7s4(W(li).data(), cout, cout, d.g.cinp(), nullptr));
      } else if (k == CONVT) {
        // dgrad of ConvTranspose Wt[CIN][COUT][7]: stride-4 conv of the full-length gz (COUT channels) -> CIN channels
        d.dst = Ls[li - 1].bn.ga1;
        d.l_out = d.cols = LEN[lv + 1];
        append_frag(tr, &d, amat_conv(W(li).data(), cin, cout, 7, 4, 1, d.g.cinp(), nullptr));
      } else {
        // dgrad of a stride-1 conv W[COUT][CIN][7]: conv of gz (COUT channels) with the flipped transpose -> CIN channels
        d.dst = k == UP_SAME ? gcat[lv] : Ls[li - 1].bn.ga1;
        d.l_out = LEN[lv];
        d.cols = cols_of(d);
        append_frag(tr, &d, amat_conv(flip_transpose(W(li), cout, cin, 7).data(), cin, cout, 7, 1, d.g.P, d.g.cinp(), nullptr));
      }
    }

  for (Layer& L : tr.layers)
    for (ConvOp* op : {&L.fwd, &L.dgrad})
      if (op->used) {
        tr.need(op->src1, op->g.src_need(op->cols));
        tr.need(op->src2, op->g.src_need(op->cols));
      }
  size_t so = 0;
  for (Layer& L : tr.layers) {
    L.bn.stats_off = so;
    so += 4 * (size_t)L.bn.C;
  }
  return VP_OK;
}

// Partial results of a weight gradient: one row of out_n floats per workgroup, folded by sum_rows_multi_kernel.  With 256
// rows for every tensor of > 10 k weights the rows were 267 MB per step -- written by the weight-gradient launches, read
// again by the fold (68 us, on the step's critical path) -- for 1.1 MB of gradients: the rows are capped by their bytes.
int wg_rows_cap(int out_n) {
  constexpr long budget = 1L << 22;  // same-box sweep: 1.64 ms per step unbounded, 1.60 at 8 M floats, 1.57 at 4-6 M, 1.60 at 2-3 M
                                     // (below that the deep layers' launches have too few workgroups and end behind the main chain)
  int cap = out_n > 10000 ? 256 : 512;
  while (cap > 32 && (long)cap * out_n > budget) cap >>= 1;
  return cap;
}

int upload(Trainer& tr, const float* weights) {
  const int B = tr.max_batch;
  size_t total = 0;
  std::vector<size_t> toff(tr.tensors.size());
  for (size_t i = 0; i < tr.tensors.size(); ++i) {
    Tensor& t = tr.tensors[i];
    t.ls = round_up(t.need, tr.bf16 ? 8 : 4);  // rows start on 16-byte boundaries either way
    toff[i] = total;
    total += (size_t)t.C * t.ls * B;
    total = (total + 63) / 64 * 64;
  }
  VP_HIP(tr.arena.alloc(total * tr.esize, true));  // (a zero of either type)
  for (size_t i = 0; i < tr.tensors.size(); ++i) tr.tensors[i].p = reinterpret_cast<float*>(tr.arena.p + toff[i] * tr.esize);
  const size_t np = tr.n_params;
  if (const int rc = tr.opt.alloc(np); rc != VP_OK) return rc;
  VP_HIP(hipMemcpy(tr.opt.w, weights, np * sizeof(float), hipMemcpyHostToDevice));
  std::vector<float> mask(np, 1.f);
  for (auto& kv : tr.poff) {
    const std::string& n = kv.first;
    const bool running = n.size() > 12 && (n.rfind("running_mean") == n.size() - 12 || n.rfind("running_var") == n.size() - 11);
    if (running)
      for (size_t i = 0; i < tr.psize[n]; ++i) mask[kv.second + i] = 0.f;
  }
  VP_HIP(hipMemcpy(tr.opt.mask, mask.data(), np * sizeof(float), hipMemcpyHostToDevice));
  tr.frag_n = tr.frag_idx_host.size();
  VP_HIP(tr.frag_idx.alloc(tr.frag_n));
  VP_HIP(hipMemcpy(tr.frag_idx, tr.frag_idx_host.data(), tr.frag_n * sizeof(int), hipMemcpyHostToDevice));
  VP_HIP(tr.frag.alloc(tr.frag_n));
  {  // the bf16-MFMA convs' operands
    size_t n3 = 0;
    for (Layer& L : tr.layers)
      for (ConvOp* op : {&L.fwd, &L.dgrad})
        if (op->used && op->launch_b16) {
          op->a3_off = n3;
          n3 += op->a3_n;
        }
    if (n3) {
      size_t ns2 = 0;
      for (Layer& L : tr.layers)
        if (L.fwd.launch_b16) {
          const size_t need = (size_t)L.fwd.cout * ((L.fwd.cols + L.fwd.tn - 1) / L.fwd.tn) * tr.max_batch * 2;
          if (need > ns2) ns2 = need;
        }
      if (ns2) VP_HIP(tr.conv_stat.alloc(ns2));
      VP_HIP(tr.frag3.alloc(n3));
      for (Layer& L : tr.layers)
        for (ConvOp* op : {&L.fwd, &L.dgrad})
          if (op->used && op->launch_b16) {
            if (tr.b16_jobs.count >= MAX_B16_JOBS) return VP_ERR_UNSUPPORTED;
            ConvB16PackJob& jb = tr.b16_jobs.job[tr.b16_jobs.count++];
            const int cb = op->g.cinp() / 4, tpr = op->g.taps <= 2 ? 2 : 8, tg = tpr == 8 ? (op->g.taps + 7) / 8 : 1, mt = op->g.M() / 16;
            jb.frag = tr.frag + op->frag_off;
            jb.out = tr.frag3 + op->a3_off;
            jb.MT = mt;
            jb.CB = cb;
            jb.TAPS = op->g.taps;
            jb.TG = tg;
            jb.TPR = tpr;
            jb.first_block = tr.b16_blocks;
            tr.b16_blocks += (mt * (tpr == 8 ? cb * tg : cb / 4) + 3) / 4;
          }
    }
  }
  VP_HIP(tr.zeros.alloc(256, true));
  size_t ns = 0;
  for (Layer& L : tr.layers) ns += 4 * (size_t)L.bn.C;
  VP_HIP(tr.stats.alloc(ns, true));
  VP_HIP(tr.bn_partial.alloc((size_t)128 * 256 * 2));
  size_t wtot = 0;
  for (Layer& L : tr.layers) {
    L.wg.partial_off = wtot;
    wtot += (size_t)wg_rows_cap(L.wg.out_n) * (size_t)L.wg.out_n;  // what the launches can reach (512 rows each was 550 MB)
  }
  VP_HIP(tr.wg_partial.alloc(wtot));
  VP_HIP(tr.head_partial.alloc((size_t)((T0 + 255) / 256) * B * 28));
  VP_HIP(tr.head_sums.alloc(32, true));
  VP_HIP(tr.head_stage.alloc(64 * 28));
  for (DevArray<float>* a : {&tr.x_dev, &tr.y_dev, &tr.p_dev}) VP_HIP(a->alloc((size_t)B * 3 * T0));
  for (Layer& L : tr.layers) {  // dynamic LDS beyond the default, for this trainer's device
    for (ConvOp* op : {&L.fwd, &L.dgrad})
      if (op->used && op->lds_bytes > 48 * 1024)
        VP_HIP(hipFuncSetAttribute(op->kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)op->lds_bytes));
    for (const void* k : L.wg.kernel)
      if (k) VP_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.wg.lds_bytes));
  }
  // Non-blocking: a blocking stream synchronises implicitly with the legacy default stream, so every event a binder
  // records there for the step's inputs (volpick_amd/train.py: torch's current stream) serialised the step against its
  // predecessor on the device -- 2.75 instead of 1.72 ms per 512-window step (tools/train_probe.py).  The uploads above ran
  // on the default stream: they are complete before the first step can be enqueued.
  VP_HIP(hipDeviceSynchronize());
  // The weight gradients' stream gets the LOWEST priority, the main chain the default one: streams of different priority
  // never share a hardware queue (two default-priority streams created after other streams of the process had been
  // destroyed did: the step ran 1.96 instead of 1.56 ms, its two chains serialised -- tools/train_after_forward_probe.py),
  // and where both have workgroups waiting the chain the step's length hangs on goes first.
  {
    int pr_least = 0, pr_greatest = 0;
    VP_HIP(hipDeviceGetStreamPriorityRange(&pr_least, &pr_greatest));
    VP_HIP(hipStreamCreateWithFlags(&tr.stream, hipStreamNonBlocking));
    VP_HIP(hipStreamCreateWithPriority(&tr.stream_wg, hipStreamNonBlocking, pr_least));  // (main chain at the highest: the same)
  }
  // consumed by another stream of this device only: a device-scope release at the event is enough (the default release
  // to the system writes the L2 back: ~5 us in front of the stream's next launch, once per layer)
  const unsigned ev_dev = hipEventDisableTiming | hipEventReleaseToDevice;
  for (hipEvent_t& e : tr.ev_gz) VP_HIP(hipEventCreateWithFlags(&e, ev_dev));
  VP_HIP(hipEventCreateWithFlags(&tr.ev_wg, ev_dev));
  VP_HIP(hipEventCreateWithFlags(&tr.ev_wg1, ev_dev));
  for (hipEvent_t& e : tr.ev_inputs) VP_HIP(hipEventCreateWithFlags(&e, ev_dev));
  return VP_OK;
}

// The A/B switches of the bf16-MFMA convs, read once per process: VP_CONV_B16=0 = the fp32-MFMA convs, VP_CONV_STAT=0 =
// separate statistics launches.
struct ConvSwitches {
  bool b16, stat;
};
const ConvSwitches& conv_switches() {
  static const auto on = [](const char* name) { return !getenv(name) || atoi(getenv(name)) != 0; };
  static const ConvSwitches s{on("VP_CONV_B16"), on("VP_CONV_STAT")};
  return s;
}

// Returns the number of per-workgroup BatchNorm sums the launch left in tr.conv_stat (want_stat, bf16-MFMA form), else 0.
int run_conv(Trainer& tr, const ConvOp& op, int B, bool want_stat = false) {
  ++tr.launches;
  ConvArgs a{};
  const Tensor& s1 = tr.tensors[op.src1];
  a.src1 = s1.p;
  a.ls1 = s1.ls;
  a.ws1 = (long)s1.win_stride();
  if (op.src2 >= 0) {
    const Tensor& s2 = tr.tensors[op.src2];
    a.src2 = s2.p;
    a.ls2 = s2.ls;
    a.ws2 = (long)s2.win_stride();
  }
  const Tensor& d = tr.tensors[op.dst];
  a.dst = d.p;
  a.lsd = d.ls;
  a.wsd = (long)d.win_stride();
  a.dst_halo = HALO;
  a.afrag = tr.frag + op.frag_off;
  a.bias = op.bias_off >= 0 ? tr.opt.w + op.bias_off : tr.zeros.p;
  a.win_per_set = B;
  a.n_windows = B;
  a.l_out = op.l_out;
  a.l_dst = op.l_out;
  if (op.launch_b16 && tr.frag3 && conv_switches().b16) {
    const bool st = want_stat && conv_switches().stat && tr.conv_stat;
    op.launch_b16(a, tr.frag3 + op.a3_off, st ? tr.conv_stat.p : nullptr, op.cols, tr.stream);
    return st ? ((op.cols + op.tn - 1) / op.tn) * B : 0;
  }
  op.launch(a, op.cols, tr.stream);
  return 0;
}

BnArgs bn_args(Trainer& tr, const BnOp& b, int B) {
  BnArgs a{};
  a.z = tr.rows(b.z);
  a.a = tr.rows(b.a);
  a.gz = tr.rows(b.gz);
  a.ga1 = tr.rows(b.ga1, b.ga1_ch);
  a.ga2 = b.ga2 >= 0 ? tr.rows(b.ga2, b.ga2_ch) : Rows{nullptr, 0, 0};
  a.C = b.C;
  a.B = B;
  a.Lz = b.Lz;
  a.La = b.La;
  a.crop = b.crop;
  a.gamma = tr.opt.w + b.gamma_off;
  a.beta = tr.opt.w + b.beta_off;
  a.running_mean = tr.opt.w + b.rm_off;
  a.running_var = tr.opt.w + b.rv_off;
  a.stats = tr.stats + b.stats_off;
  a.partial = tr.bn_partial;
  {  // 64 >> sl2 rows per wave and trip, ~2 k workgroups per launch at most
    const int nv = (b.Lz + 7) / 8;
    a.sl2 = nv <= 2 ? 1 : nv <= 4 ? 2 : nv <= 8 ? 3 : nv <= 16 ? 4 : nv <= 32 ? 5 : 6;
    const int rows_per_block = 4 * (64 >> a.sl2);
    int gb = 2048 / b.C;
    if (gb > (B + rows_per_block - 1) / rows_per_block) gb = (B + rows_per_block - 1) / rows_per_block;
    a.GB = gb < 1 ? 1 : (gb > 256 ? 256 : gb);
  }
  a.g_gamma = tr.opt.grad + b.gamma_off;
  a.g_beta = tr.opt.grad + b.beta_off;
  a.eps = tr.bn_eps;
  a.momentum = tr.bn_momentum;
  return a;
}

// A BatchNorm pass: the crop of the ConvTranspose layers (0, 1 or 2 samples) selects the instantiation.  With `done` (which
// may point to a null event) the launch is hipExtLaunchKernel's, the event bound to the launch's own completion (its stop
// event): what another stream waits for is this kernel's end, without the marker packet a hipEventRecord puts into the
// queue (6-8 us in front of the next launch of this stream, eighteen times per step).
void launch_bn(Trainer& tr, const BnKernel (&by_crop)[3], const BnArgs& a, const hipEvent_t* done = nullptr) {
  const BnKernel kernel = by_crop[a.crop < 2 ? a.crop : 2];
  const dim3 grid(a.C, a.GB);
  if (done) {
    ++tr.launches;
    hipExtLaunchKernelGGL(kernel, grid, dim3(256), 0, tr.stream, nullptr, *done, 0, a);
  } else {
    TRL(kernel, grid, dim3(256), 0, tr.stream, a);
  }
}

// ---- the weight gradients' side queue --------------------------------------------------------------------------------
// fills the job of folding `rows` partial rows of a layer's weight gradient; returns the workgroups it takes
int fill_sum_job(SumJob& jb, Trainer& tr, const WgradOp& w, const float* partial, int rows, int first_block) {
  jb.partial = partial;
  jb.out = tr.opt.grad + w.grad_off;
  jb.rows = rows;
  jb.n = w.out_n;
  jb.first_block = first_block;
  jb.cq = sum_job_cq(rows);
  return (w.out_n + 4 * jb.cq - 1) / (4 * jb.cq);
}

// The backward pass hands every layer's weight gradient to add(); flush() sends what is held to the other stream behind an
// event of the main chain.
struct WgradQueue {
  // The partial rows of the weight gradients are folded by sum_rows_multi_kernel: those of the layers >= FOLD_EARLY each
  // right behind its weight gradient on that stream (where the stream still waits for the main chain between its
  // launches), the rest in one launch at the end of the step, in front of Adam, alone on the chip.
  // (same-box sweep of FOLD_EARLY: none 1.414 ms per step, 13: 1.389, 11: 1.405, 9: 1.411, 7: 1.418, 5: 1.436 -- the folds of
  // the deep layers' 15 MB rows take more from the main chain beside them than they save at the end)
  static constexpr int FOLD_EARLY = 13;
  // Layers whose gz gets an event for the weight-gradient stream; the layers between hand their launch to the next event.
  // An event costs the main chain ~5 us (the launch behind a kernel with a completion signal starts that much later):
  // every other layer above level 0, every layer of the last four (their weight gradients are the step's tail).
  static constexpr unsigned ev_mask = 0x2aaaf;
  // ev_wg1 is recorded behind layer 1's launch on the premise that it is the last of its flush, li == 0 flushes the rest, and the
  // first layer handled (NLAYER - 1) opens the chain: a retuned mask must keep those three bits
  static_assert((ev_mask & 3u) == 3u && ((ev_mask >> (NLAYER - 1)) & 1u), "ev_mask: layers 0, 1 and NLAYER - 1 carry an event");
  static_assert(NLAYER <= MAX_SUM_JOBS, "one sum job per layer");
  static bool has_event(int li) { return (ev_mask >> li) & 1; }

  Trainer& tr;
  const int B;
  struct {
    const WgradOp* w;
    WgradArgs g;
    int grid, li;
  } held[NLAYER];
  int n_held = 0;
  SumJobs jobs{}, jobs_last{};  // the folds left for the end of the step: layers 1 .. FOLD_EARLY - 1 | layer 0
  int blocks = 0, blocks_last = 0;

  void add(int li) {
    const WgradOp& w = tr.layers[li].wg;
    WgradArgs g{};
    g.lo = tr.rows(w.lo);
    g.hi1 = tr.rows(w.hi1);
    g.lim_hi1 = tr.tensors[w.hi1].ls - HALO;
    if (w.hi2 >= 0) {
      g.hi2 = tr.rows(w.hi2);
      g.lim_hi2 = tr.tensors[w.hi2].ls - HALO;
    }
    g.Ln = w.Ln;
    g.off = w.off;
    g.B = B;
    g.chunks = (w.Ln + w.TT - 1) / w.TT;
    g.partial = tr.wg_partial + w.partial_off;
    const int items = ((B + w.WB - 1) / w.WB) * g.chunks;
    const int cap = wg_rows_cap(w.out_n);  // one partial result per workgroup: fewer, longer-lived workgroups for the big weight tensors
    const int grid = items < cap ? items : cap;
    held[n_held++] = {&w, g, grid, li};
    if (li < FOLD_EARLY) {
      SumJobs& set = li == 0 ? jobs_last : jobs;
      int& nb = li == 0 ? blocks_last : blocks;
      nb += fill_sum_job(set.job[set.count], tr, w, g.partial, grid, nb);
      ++set.count;
    }
  }
  void flush(hipEvent_t gz_done) {
    (void)hipStreamWaitEvent(tr.stream_wg, gz_done, 0);
    for (int k = 0; k < n_held; ++k) {
      const WgradOp& w = *held[k].w;
      ++tr.launches;
      w.launch(held[k].g, held[k].grid, tr.stream_wg);
      if (held[k].li >= FOLD_EARLY) {
        SumJobs one{};
        one.count = 1;
        const int nb = fill_sum_job(one.job[0], tr, w, held[k].g.partial, held[k].grid, 0);
        ++tr.launches;
        hipLaunchKernelGGL(sum_rows_multi_kernel, dim3(nb), dim3(256), 0, tr.stream_wg, one);
      }
      if (held[k].li == 1) (void)hipEventRecord(tr.ev_wg1, tr.stream_wg);  // (layer 1 carries an event: its launch is out)
    }
    n_held = 0;
  }
};

// ---- the step, phase by phase ----------------------------------------------------------------------------------------
void pack_weights(Trainer& tr) {
  TRL(gather_pack_kernel, dim3((unsigned)((tr.frag_n + 255) / 256)), dim3(256), 0, tr.stream, tr.frag_idx, tr.opt.w, tr.frag,
      (long)tr.frag_n);
  if (tr.b16_blocks) TRL(conv_b16_pack_kernel, dim3(tr.b16_blocks), dim3(256), 0, tr.stream, tr.b16_jobs);
}

void load_input(Trainer& tr, const float* x_dev, int B) {
  TRL(tr.rk.load_rows, dim3((T0 + tr.rk.load_span - 1) / tr.rk.load_span, 3, B), dim3(256), 0, tr.stream, x_dev, tr.rows(tr.t_x), 3, T0);
}

void forward_layers(Trainer& tr, int B) {
  for (Layer& L : tr.layers) {
    const int n_stat = run_conv(tr, L.fwd, B, true);
    BnArgs a = bn_args(tr, L.bn, B);
    a.fpart = n_stat ? tr.conv_stat.p : nullptr;
    a.n_fpart = n_stat;
    if (!a.fpart) TRL(tr.rk.bn_stats, dim3(a.C, a.GB), dim3(256), 0, tr.stream, a);  // (else the conv launch left the sums)
    launch_bn(tr, tr.rk.bn_apply, a);
  }
}

void head_and_loss(Trainer& tr, const float* y_dev, int B) {
  hipStream_t s = tr.stream;
  HeadArgs2 h{};
  h.a = tr.rows(tr.layers[NLAYER - 1].bn.a);
  h.ga = tr.rows(tr.t_ga_last);
  h.y = y_dev;
  h.p = tr.p_dev;
  h.w = tr.opt.w + tr.poff.at("out.weight");
  h.b = tr.opt.w + tr.poff.at("out.bias");
  h.partial = tr.head_partial;
  h.B = B;
  h.T = T0;
  h.eps = tr.loss_eps;
  const int gx = (T0 + tr.rk.head_span - 1) / tr.rk.head_span;
  const int slot = (int)(tr.seq % Trainer::EV_RING);
  hipEvent_t ev_in = tr.ev_inputs[slot];
  tr.ev_inputs_seq[slot] = tr.seq++;
  // load_rows read x, this launch reads y: nothing behind its end (ev_inputs) touches the caller's buffers
  ++tr.launches;
  hipExtLaunchKernelGGL(tr.rk.head, dim3(gx, B), dim3(256), 0, s, nullptr, ev_in, 0, h);
  // two stages: 64 row groups, then the 64 group sums
  TRL((sum_rows_kernel<double, double>), dim3(1, 64), dim3(256), 0, s, tr.head_partial, gx * B, 28, tr.head_stage);
  TRL((sum_rows_kernel<double, double>), dim3(1, 1), dim3(256), 0, s, tr.head_stage, 64, 28, tr.head_sums);
  TRL(head_final_kernel, dim3(1), dim3(32), 0, s, tr.head_sums, tr.head_sums + 28, tr.opt.grad + tr.poff.at("out.bias"),
      tr.opt.grad + tr.poff.at("out.weight"));
}

void backward_layers(Trainer& tr, WgradQueue& wq, int B) {
  hipStream_t s = tr.stream;
  for (int li = NLAYER - 1; li >= 0; --li) {
    Layer& L = tr.layers[li];
    const BnArgs a = bn_args(tr, L.bn, B);
    const hipEvent_t gz_done = WgradQueue::has_event(li) ? tr.ev_gz[li] : nullptr;  // the event: gz of this layer is complete
    launch_bn(tr, tr.rk.bn_bwd_partial, a);
    launch_bn(tr, tr.rk.bn_bwd_apply, a, &gz_done);
    wq.add(li);
    if (gz_done) wq.flush(gz_done);
    if (li == 0) {  // conv bias of `inc`: sum of gz per channel (zero up to rounding: BatchNorm removes the mean)
      const int GB = B < 64 ? B : 64;
      TRL(tr.rk.channel_sum, dim3(8, GB), dim3(256), 0, s, tr.rows(L.bn.gz), B, T0, GB, tr.bn_partial);
      TRL((sum_rows_kernel<double, float>), dim3(1, 1), dim3(256), 0, s, tr.bn_partial, GB, 8, tr.opt.grad + tr.poff.at("inc.bias"));
    }
    if (L.dgrad.used) run_conv(tr, L.dgrad, B);
  }
}

void fold_and_update(Trainer& tr, const WgradQueue& wq, bool update, float lr) {
  hipStream_t s = tr.stream;
  // the fold of everything but the first layer's rows runs beside that layer's weight gradient, the step's last launch on
  // the other stream; its own few rows behind it
  (void)hipStreamWaitEvent(s, tr.ev_wg1, 0);
  TRL(sum_rows_multi_kernel, dim3(wq.blocks), dim3(256), 0, s, wq.jobs);
  (void)hipEventRecord(tr.ev_wg, tr.stream_wg);
  (void)hipStreamWaitEvent(s, tr.ev_wg, 0);  // every weight gradient's partial rows are written
  TRL(sum_rows_multi_kernel, dim3(wq.blocks_last), dim3(256), 0, s, wq.jobs_last);
  if (update) tr.opt.update(s, lr, tr.launches);
}

int forward_backward(Trainer& tr, const float* x_dev, const float* y_dev, int B, bool update, float lr) {
  tr.launches = 0;
  pack_weights(tr);
  load_input(tr, x_dev, B);
  forward_layers(tr, B);
  head_and_loss(tr, y_dev, B);
  WgradQueue wq{tr, B};
  backward_layers(tr, wq, B);
  fold_and_update(tr, wq, update, lr);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("training step: kernel launch failed: %s", hipGetErrorString(e));
    return VP_ERR_HIP;
  }
  return VP_OK;
}

int step_and_loss(Trainer& tr, const float* x_dev, const float* y_dev, int B, float lr, int update, double* loss) {
  const int rc = forward_backward(tr, x_dev, y_dev, B, update != 0, lr);
  if (rc != VP_OK) return rc;
  if (loss) {
    VP_HIP(hipMemcpyAsync(loss, tr.head_sums + 28, sizeof(double), hipMemcpyDeviceToHost, tr.stream));
    VP_HIP(hipStreamSynchronize(tr.stream));
  }
  return VP_OK;
}

// vp_train_step_bank(_aug): the batch of `rows` generated into the trainer's input buffers, then the step.
int step_bank(Trainer& tr, const Bank& bk, BatchRows rows, int B, float sigma, int norm, const int* label_rows, float lr,
              int update, double* loss) {
  VP_REQUIRE(B >= 2 && B <= tr.max_batch, "vp_train_step_bank: batch %d outside [2, %d]", B, tr.max_batch);
  VP_REQUIRE(bk.device == tr.device, "vp_train_step_bank: bank on device %d, trainer on device %d", bk.device, tr.device);
  static_assert(RowRing::N == Trainer::EV_RING, "one plan-row slot per step event");
  const BatchSpec spec{T0, sigma, norm, LABEL_PSN, label_rows};
  int rc = bank_check(bk, spec, rows, B);
  if (rc != VP_OK) return rc;
  VP_HIP(hipSetDevice(tr.device));
  if (!tr.plan_rows.cap) {  // once, for either kind of row: a regrowth would have to wait for every slot
    rc = tr.plan_rows.reserve((size_t)tr.max_batch * std::max(sizeof(vp_plan_row), sizeof(vp_aug_row)));
    if (rc != VP_OK) return rc;
  }
  // the step that used this slot last: its ev_inputs stands behind the head kernel, which runs after the generation kernel
  // that read the slot's device copy, which ran after the copy that read the host slot
  const int slot = (int)(tr.seq % Trainer::EV_RING);
  if (tr.ev_inputs_seq[slot] >= 0) VP_HIP(hipEventSynchronize(tr.ev_inputs[slot]));
  const void* rd = tr.plan_rows.stage(slot, {{rows.p, rows.bytes(B)}}, tr.stream);
  if (!rd) return VP_ERR_HIP;
  if ((rc = bank_launch(bk, spec, rows.at(rd), B, tr.x_dev, tr.y_dev, tr.stream)) != VP_OK) return rc;
  return step_and_loss(tr, tr.x_dev, tr.y_dev, B, lr, update, loss);
}

}  // namespace
}  // namespace vp

using namespace vp;

extern "C" {

int vp_train_create(int device_id, int model_kind, const float* weights, size_t n_floats, int max_batch,
                    vp_trainer** out) {
  return vp_train_create_dtype(device_id, model_kind, weights, n_floats, max_batch, VP_TRAIN_FP32, out);
}

int vp_train_dtype(const vp_trainer* h) {
  return h ? (reinterpret_cast<const Trainer*>(h)->bf16 ? VP_TRAIN_BF16 : VP_TRAIN_FP32) : VP_ERR_INVALID;
}

int vp_train_create_dtype(int device_id, int model_kind, const float* weights, size_t n_floats, int max_batch, int dtype,
                          vp_trainer** out) {
  VP_REQUIRE(out && weights && max_batch > 0, "vp_train_create: bad argument");
  VP_REQUIRE(dtype == VP_TRAIN_FP32 || dtype == VP_TRAIN_BF16, "vp_train_create: dtype %d is neither VP_TRAIN_FP32 nor VP_TRAIN_BF16", dtype);
  if (model_kind != VP_MODEL_PHASENET) {
    set_error("vp_train_create: only PhaseNet has a training step");
    return VP_ERR_UNSUPPORTED;
  }
  auto tr = std::make_unique<Trainer>();
  tr->device = device_id;
  tr->max_batch = max_batch;
  tr->bf16 = dtype == VP_TRAIN_BF16;
  tr->esize = tr->bf16 ? 2 : 4;
  int rc = build_plan(*tr);
  if (rc != VP_OK) return rc;
  VP_REQUIRE(n_floats == tr->n_params, "vp_train_create: expected %zu weights, got %zu", tr->n_params, n_floats);
  VP_HIP(hipSetDevice(device_id));
  rc = upload(*tr, weights);
  if (rc != VP_OK) return rc;
  *out = reinterpret_cast<vp_trainer*>(tr.release());
  return VP_OK;
}

int vp_train_destroy(vp_trainer* h) {
  delete reinterpret_cast<Trainer*>(h);
  return VP_OK;
}

int vp_train_set_hyper(vp_trainer* h, float beta1, float beta2, float adam_eps, float bn_momentum, float loss_eps) {
  VP_REQUIRE(h, "vp_train_set_hyper: null handle");
  // (nothing is stored before all five have passed)
  if (const int rc = check_hyper("vp_train_set_hyper", beta1, beta2, adam_eps); rc != VP_OK) return rc;
  VP_REQUIRE(bn_momentum > 0.f && bn_momentum <= 1.f, "vp_train_set_hyper: bn_momentum %g outside (0, 1]", (double)bn_momentum);
  VP_REQUIRE(loss_eps > 0.f && std::isfinite(loss_eps), "vp_train_set_hyper: loss_eps %g is not finite and positive", (double)loss_eps);
  Trainer& tr = *reinterpret_cast<Trainer*>(h);
  tr.opt.beta1 = beta1, tr.opt.beta2 = beta2, tr.opt.adam_eps = adam_eps;
  tr.bn_momentum = bn_momentum;
  tr.loss_eps = loss_eps;
  return VP_OK;
}

int vp_train_set_ema(vp_trainer* h, float decay) {
  VP_REQUIRE(h && decay >= 0.f && decay < 1.f, "vp_train_set_ema: bad argument");
  Trainer& tr = *reinterpret_cast<Trainer*>(h);
  VP_HIP(hipSetDevice(tr.device));
  VP_HIP(hipStreamSynchronize(tr.stream));
  if (!tr.opt.ema) VP_HIP(tr.opt.ema.alloc(tr.n_params));
  // starts at the current weights; on the trainer's (non-blocking) stream, so that the next step's Adam / EMA update is
  // ordered behind the copy (a null-stream device-to-device copy may return before it has run)
  VP_HIP(hipMemcpyAsync(tr.opt.ema, tr.opt.w, tr.n_params * sizeof(float), hipMemcpyDeviceToDevice, tr.stream));
  VP_HIP(hipStreamSynchronize(tr.stream));
  tr.opt.ema_decay = decay;
  return VP_OK;
}

int vp_train_step(vp_trainer* h, const float* x, const float* y, int mem, int B, float lr, int update, double* loss) {
  VP_REQUIRE(h && x && y, "vp_train_step: null argument");
  Trainer& tr = *reinterpret_cast<Trainer*>(h);
  VP_REQUIRE(B >= 2 && B <= tr.max_batch, "vp_train_step: batch %d outside [2, %d]", B, tr.max_batch);
  VP_HIP(hipSetDevice(tr.device));
  const float *xd = x, *yd = y;
  if (mem == VP_MEM_HOST) {
    const size_t n = (size_t)B * 3 * T0 * sizeof(float);
    VP_HIP(hipMemcpyAsync(tr.x_dev, x, n, hipMemcpyHostToDevice, tr.stream));
    VP_HIP(hipMemcpyAsync(tr.y_dev, y, n, hipMemcpyHostToDevice, tr.stream));
    xd = tr.x_dev;
    yd = tr.y_dev;
  }
  return step_and_loss(tr, xd, yd, B, lr, update, loss);
}

int vp_train_step_bank(vp_trainer* h, vp_bank* bank, const vp_plan_row* rows, int B, float sigma, int norm,
                       const int* label_rows, float lr, int update, double* loss) {
  VP_REQUIRE(h && bank, "vp_train_step_bank: null argument");
  return step_bank(*reinterpret_cast<Trainer*>(h), *reinterpret_cast<const Bank*>(bank), rows, B, sigma, norm,
                   label_rows, lr, update, loss);
}

int vp_train_step_bank_aug(vp_trainer* h, vp_bank* bank, const vp_aug_row* rows, int B, float sigma, int norm,
                           const int* label_rows, float lr, int update, double* loss) {
  VP_REQUIRE(h && bank, "vp_train_step_bank_aug: null argument");
  return step_bank(*reinterpret_cast<Trainer*>(h), *reinterpret_cast<const Bank*>(bank), rows, B, sigma, norm,
                   label_rows, lr, update, loss);
}

// Makes `stream` (a hipStream_t of the same device; NULL = the legacy default stream) wait until the latest vp_train_step
// has read its x / y for the last time: work enqueued on `stream` afterwards may overwrite or free them.  No host wait.
int vp_train_wait_inputs_consumed(vp_trainer* h, void* stream) {
  VP_REQUIRE(h, "vp_train_wait_inputs_consumed: null handle");
  Trainer& tr = *reinterpret_cast<Trainer*>(h);
  VP_HIP(hipSetDevice(tr.device));
  if (tr.seq > 0)
    VP_HIP(hipStreamWaitEvent(reinterpret_cast<hipStream_t>(stream), tr.ev_inputs[(tr.seq - 1) % Trainer::EV_RING], 0));
  return VP_OK;
}

// The highest step number (0 = the first vp_train_step of this trainer) whose reads of x / y have completed, -1 if none is
// known to have: a caller that keeps device batches alive for queued steps drops the ones up to it.  No host wait.
long long vp_train_inputs_consumed_upto(vp_trainer* h) {
  if (!h) return -1;
  Trainer& tr = *reinterpret_cast<Trainer*>(h);
  if (hipSetDevice(tr.device) != hipSuccess) return -1;
  long long best = -1;
  for (int i = 0; i < Trainer::EV_RING; ++i)
    if (tr.ev_inputs_seq[i] > best && hipEventQuery(tr.ev_inputs[i]) == hipSuccess) best = tr.ev_inputs_seq[i];
  (void)hipGetLastError();  // hipErrorNotReady of the pending ones is not an error
  return best;
}

// Steps enqueued on this trainer so far: the step a vp_train_step call just queued has the number (this - 1).
long long vp_train_steps_enqueued(const vp_trainer* h) { return h ? reinterpret_cast<const Trainer*>(h)->seq : 0; }

int vp_train_synchronize(vp_trainer* h) {
  VP_REQUIRE(h, "vp_train_synchronize: null handle");
  VP_HIP(hipStreamSynchronize(reinterpret_cast<Trainer*>(h)->stream));
  return VP_OK;
}

// which: 0 weights (incl. BN running statistics), 1 gradients of the last step, 2 Adam m, 3 Adam v, 4 EMA weights
int vp_train_read(vp_trainer* h, int which, float* out, size_t n_floats) {
  VP_REQUIRE(h && out, "vp_train_read: null argument");
  Trainer& tr = *reinterpret_cast<Trainer*>(h);
  return tr.opt.read("vp_train_read", tr.device, tr.stream, 4, which, out, n_floats);
}

int vp_train_write_weights(vp_trainer* h, const float* weights, size_t n_floats) {
  VP_REQUIRE(h && weights, "vp_train_write_weights: null argument");
  Trainer& tr = *reinterpret_cast<Trainer*>(h);
  VP_REQUIRE(n_floats == tr.n_params, "vp_train_write_weights: bad size");  // (this entry point's own wording)
  return tr.opt.write("vp_train_write_weights", tr.device, tr.stream, weights, n_floats);
}

// predictions (B, 3, 3001) of the last step's forward pass
int vp_train_predictions(vp_trainer* h, float* out, int B) {
  VP_REQUIRE(h && out, "vp_train_predictions: null argument");
  Trainer& tr = *reinterpret_cast<Trainer*>(h);
  VP_REQUIRE(B > 0 && B <= tr.max_batch, "vp_train_predictions: bad batch");
  VP_HIP(hipSetDevice(tr.device));
  VP_HIP(hipStreamSynchronize(tr.stream));
  VP_HIP(hipMemcpy(out, tr.p_dev, (size_t)B * 3 * T0 * sizeof(float), hipMemcpyDeviceToHost));
  return VP_OK;
}

int vp_train_tensor_count(const vp_trainer* h) {
  return h ? (int)reinterpret_cast<const Trainer*>(h)->tensors.size() : VP_ERR_INVALID;
}
int vp_train_tensor_info(const vp_trainer* h, int index, const char** name, int* channels, int* length) {
  VP_REQUIRE(h, "vp_train_tensor_info: null handle");
  const Trainer& tr = *reinterpret_cast<const Trainer*>(h);
  VP_REQUIRE(index >= 0 && index < (int)tr.tensors.size(), "vp_train_tensor_info: bad index");
  if (name) *name = tr.tensors[index].name.c_str();
  if (channels) *channels = tr.tensors[index].C;
  if (length) *length = tr.tensors[index].L;
  return VP_OK;
}
// dense (B, C, L) copy of an activation / gradient tensor of the last step (parity tests)
int vp_train_tensor_read(vp_trainer* h, int index, int B, float* out) {
  VP_REQUIRE(h && out, "vp_train_tensor_read: null argument");
  Trainer& tr = *reinterpret_cast<Trainer*>(h);
  VP_REQUIRE(index >= 0 && index < (int)tr.tensors.size() && B > 0 && B <= tr.max_batch, "vp_train_tensor_read: bad argument");
  const Tensor& t = tr.tensors[index];
  VP_HIP(hipSetDevice(tr.device));
  VP_HIP(hipStreamSynchronize(tr.stream));
  if (tr.bf16) {
    const size_t n = (size_t)B * t.C * t.L;
    std::vector<uint16_t> raw(n);
    VP_HIP(hipMemcpy2D(raw.data(), (size_t)t.L * 2, reinterpret_cast<const uint16_t*>(t.p) + HALO, (size_t)t.ls * 2, (size_t)t.L * 2,
                       (size_t)B * t.C, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) {
      const uint32_t u = (uint32_t)raw[i] << 16;
      memcpy(out + i, &u, 4);
    }
    return VP_OK;
  }
  VP_HIP(hipMemcpy2D(out, (size_t)t.L * sizeof(float), t.p + HALO, (size_t)t.ls * sizeof(float), (size_t)t.L * sizeof(float),
                     (size_t)B * t.C, hipMemcpyDeviceToHost));
  return VP_OK;
}
int vp_train_launch_count(const vp_trainer* h) { return h ? reinterpret_cast<const Trainer*>(h)->launches : 0; }

void* vp_train_stream(const vp_trainer* h) { return h ? reinterpret_cast<const Trainer*>(h)->stream : nullptr; }

}  // extern "C"
