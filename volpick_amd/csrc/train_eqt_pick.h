// The two pick branches of EQTransformer in training (train_eqt_pick.hip): what the decoder trainer (train_eqt_dec.hip) holds
// and launches when its scope is VP_EQT_TRAIN_PICK_BRANCHES.
#pragma once
#include <cstdint>
#include <functional>
#include <string>

#include "train_optim.h"

namespace vp {

// ---- the branch, stated once ---------------------------------------------------------------------------------------------
struct PickDims {
  static constexpr int NBR = 2;        // branches: P, S
  static constexpr int T = 47;         // time steps (the bottleneck's length)
  static constexpr int CIN = 16;       // channels of the bottleneck x
  static constexpr int H = 16;         // LSTM units
  static constexpr int G = 4 * H;      // gate rows, torch's order i, f, g, o
  static constexpr int U = 32;         // attention units
  static constexpr int BAND = 3;       // attention width: columns i - 1 <= j < i + 2
  static constexpr float ATT_EPS = 1e-5f;
};

// The nine tensors of a branch in the flat blob's order, with their sizes; a partial gradient block of one (branch, window)
// is these nine segments back to back.
enum PickSeg { PK_W_IH, PK_W_HH, PK_B_IH, PK_B_HH, PK_WX, PK_WT, PK_BH, PK_WA, PK_BA, PK_NSEG };
constexpr int kPickSegSize[PK_NSEG] = {PickDims::G * PickDims::CIN, PickDims::G* PickDims::H, PickDims::G, PickDims::G,
                                       PickDims::H * PickDims::U,   PickDims::H* PickDims::U, PickDims::U, PickDims::U, 1};
constexpr int pick_seg_start(int s) { return s == 0 ? 0 : pick_seg_start(s - 1) + kPickSegSize[s - 1]; }
constexpr int PICK_PSZ = pick_seg_start(PK_NSEG);  // 3265 floats per branch
const char* const kPickLstmPrefix[PickDims::NBR] = {"pick_lstms.0", "pick_lstms.1"};
const char* const kPickAttPrefix[PickDims::NBR] = {"pick_attentions.0", "pick_attentions.1"};
const char* const kPickSegName[PK_NSEG] = {"weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "Wx", "Wt", "bh", "Wa", "ba"};

// Every tensor is a dense block [2 branches][B][rows][47] (rows x 47 per window).
struct PickState {
  int max_batch = 0;
  int off[PickDims::NBR][PK_NSEG] = {};  // offsets in the trainer's weight (and gradient) blob
  float drop_rate = 0.f, scale = 1.f;    // scale = 1 / (1 - drop_rate), formed once in float
  uint64_t seed = 0, step = 0;           // step: training steps run so far, update or not
  DevArray<float> pre, act, c, h, mask, hd, v, q, k, e, a, argmax;  // forward
  DevArray<float> gv, ghd, gh, gc, gpre, gq, gk, gwa;               // backward
  DevArray<float> partial;                                          // [2][max_batch][PICK_PSZ]
  hipEvent_t ev[6] = {};  // forward, adjoints, weight gradients: begin / end of each; exist only once timing was switched on

  using AddTensor = std::function<void(const std::string& name, float* p, int sets, int channels, int length)>;
  int alloc(int max_batch, const AddTensor& add);
  void release_events();
};

// x: the bottleneck [B][16][47]; din: the decoders' input [3 B][16][47], whose sets 1 and 2 are written.
void pick_forward(PickState& ps, const float* w, const float* x, float* din, int B, hipStream_t s, int& launches);
// from ps.gv (the decoders' stage-0 input gradient of sets 1 and 2): the attention's, the dropout's and the LSTM's adjoints
void pick_backward(PickState& ps, const float* w, int B, hipStream_t s, int& launches);
// the eighteen weight gradients into `grad` (the trainer's gradient blob)
void pick_wgrad(PickState& ps, const float* x, float* grad, int B, hipStream_t s, int& launches);

}  // namespace vp
