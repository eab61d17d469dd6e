// EQTransformer bottleneck kernels (sequence length 47, 16 channels): BiLSTM blocks,
// additive-attention transformer blocks and the P/S pick branches (LSTM + banded attention).
// (The 8->1 sigmoid heads run in the epilogue of the last decoder conv, conv_mfma.h EPI_HEAD.)  SURVEY.md §8a row A5, Appendix A.4/B.2.
//
// These stages are latency-bound (47 sequential LSTM steps; 47x47x32 tanh per attention)
// and hold <2 % of the model's FLOPs, so they are plain VALU code: one workgroup per
// window, activations in LDS, wavefront shuffles / readlanes for the recurrent state and
// the softmax-style row reductions.
#pragma once
#include "vp_common.h"

namespace vp {

constexpr int EQT_T = 47;  // bottleneck sequence length (6000 / 2^7)
constexpr int EQT_H = 16;  // hidden size / channels

struct LstmWeights {  // one direction, torch layout, gate order i,f,g,o
  const float* w_ih;  // [64][CIN]
  const float* w_hh;  // [64][16]
  const float* b;     // [64] = b_ih + b_hh
};

struct BiLstmArgs {
  const float* src;  // [B][CIN][ls]
  int ls_src;
  long ws_src;
  float* dst;        // [B][16][ls]
  int ls_dst;
  long ws_dst;
  LstmWeights fwd, bwd;
  const float* wc;   // folded conv1x1+BN: [16][32]
  const float* bc;   // [16]
};

struct AttnWeights {
  const float* Wt;  // [16][32]
  const float* Wx;  // [16][32]
  const float* bh;  // [32]
  const float* Wa;  // [32]
};

struct TransformerArgs {
  const float* src;  // [B][16][ls]
  int ls_src;
  long ws_src;
  float* dst;        // [B][16][ls]
  int ls_dst;
  long ws_dst;
  float* up;         // optional: decoder input, decoder input rows [B][16][ls_up] (set 0)
  int ls_up;
  long ws_up;
  AttnWeights att;
  const float *g1, *b1, *g2, *b2;  // LayerNormalization gamma/beta [16]; contiguous: g1[0..64) = g1 | b1 | g2 | b2
  const float* w1;   // [128][16]
  const float* bb1;  // [128]
  const float* w2;   // [16][128]
  const float* bb2;  // [16]
  float attn_eps, ln_eps;
};

struct PickBranchArgs {
  const float* src;  // transformer output [B][16][ls]
  int ls_src;
  long ws_src;
  float* up;         // decoder input sets 1..2: [3B][16][ls_up]
  int ls_up;
  long ws_up;
  int B;
  LstmWeights lstm[2];
  AttnWeights att[2];
  float attn_eps;
  int width;         // band width (3)
};

// The three BiLSTM blocks, the two transformer blocks and the two pick branches of one window as ONE launch
// (eqt_mid4_kernel, eqt_mid4.hip): the six launches it replaces are a chain of latency-bound kernels (47 sequential LSTM steps
// four times over) that the three device contexts cannot hide behind each other's MFMA work — measured: with them removed
// from the pipeline a 256-window step takes 510 instead of 615 us.
struct MidArgs {
  BiLstmArgs lstm[3];     // lstm[0].src: ResCNN output (64 channels); the others chain through LDS
  TransformerArgs tr[2];
  PickBranchArgs pick;
  unsigned long long* clk;  // optional debug: 8 shader-clock stamps per window (start, after each of the six stages, end)
  int B;                    // windows (the last workgroup clamps its windows to it)
};
// default: teams of four waves, FOUR windows per 1024-thread workgroup (64 CUs for a batch of 256)
int launch_eqt_mid4(const MidArgs& a, int B, hipStream_t s);
// plan_flags[2] = 2: the same kernel with ONE window per 256-thread workgroup, the bit reference of the tests
int launch_eqt_mid4_one_window(const MidArgs& a, int B, hipStream_t s);
// The DUMP instance of eqt_mid4_kernel (plan_flags[1] & 4, tests/test_gpu_layers_f64.py) also writes the fp32 values every stage
// computed into haloed [C][47] debug tensors, index MD_* below (the order of the tensors plan_eqt adds for it).  A struct of its
// own: the kernel requests sizeof(its argument struct) of kernel arguments up front, so a longer MidArgs would change the
// default instances.
enum : int {
  MD_BI_H = 0,   // bilstm.{i}.h [32][47], i = 0..2: the recurrence outputs, forward units 0-15, backward 16-31
  MD_BI_C = 3,   // bilstm.{i}.c [32][47]: the cell states
  MD_TR = 6,     // transformer i (0: transformer_d0, 1: transformer_d): MD_TR + 5 i + MD_TR_*
  MD_PICK = 16,  // pick branch k: MD_PICK + 3 k + MD_PK_*
  MD_N = 22
};
enum : int {  // .p [47][47] attention weights, .att [16][47] a.x before the residual, .y1 [16][47] LN1's output,
  MD_TR_P,    // .ff1 [128][47] ReLU(Linear1), .ff2 [16][47] Linear2 (both K halves) before the residual
  MD_TR_ATT,
  MD_TR_Y1,
  MD_TR_FF1,
  MD_TR_FF2
};
enum : int { MD_PK_H, MD_PK_C, MD_PK_P };  // pick_lstms.{k}.h, .c [16][47], pick_attentions.{k}.p [47][47]
struct MidDumpArgs : MidArgs {
  float* dbg[MD_N];
  int dbg_ls[MD_N];
  long dbg_ws[MD_N];
};
int launch_eqt_mid4_dump(const MidDumpArgs& a, int B, hipStream_t s);

int launch_bilstm(const BiLstmArgs& a, int cin, int B, hipStream_t s);
int launch_transformer(const TransformerArgs& a, int B, hipStream_t s);
int launch_pick_branch(const PickBranchArgs& a, hipStream_t s);

}  // namespace vp
