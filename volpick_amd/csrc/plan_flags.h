// Names of vp_config::plan_flags: every index and every value or bit the library reads, both models.  The short form;
// include/volpick_hip.h documents what each selects.  All 0 = the default plan.  Nothing outside this header indexes
// plan_flags with a literal.
#pragma once
#include "volpick_hip.h"

namespace vp {
namespace pf {

enum Index {
  LAYERS = 0,   // 1: PhaseNet layer by layer / EQTransformer's 14 ResCNN conv launches
  DEBUG = 1,    // bits DBG_*
  MID = 2,      // EQTransformer's middle (BiLSTM, transformers, pick branches): MID_*; PhaseNet: 1 removed; EQTransformer: 3 removed
  TILES = 3,    // TILES_*
  WARM = 4,     // 1: no L2 warm-up of the weight streams
  PN_FORM = 5,  // PhaseNet: PN_*
  PRE = 6,      // who cuts and normalises the windows: PRE_*
  EQT = 7,      // EQTransformer's conv kernels: bits EQT_*
};

constexpr int ON = 1;  // [LAYERS], [WARM]

// [DEBUG]
constexpr int DBG_LDS_DUMPS = 1;    // PhaseNet's three-launch plan dumps its LDS intermediates
constexpr int DBG_CLOCK = 2;        // clock stamps (Net::debug_clock)
constexpr int DBG_LAYER_DUMPS = 4;  // the DUMP instances of the default kernels write every layer's output

// [MID]
constexpr int MID_PN_REMOVED = 1;    // PhaseNet: the hand-pipelined K loop
constexpr int MID_SIX_LAUNCHES = 1;  // EQTransformer: the layer launches of the middle
constexpr int MID_ONE_WINDOW = 2;    // eqt_mid4_kernel<1, false>: one window per workgroup, the bit reference of the default
constexpr int MID_EQT_REMOVED = 3;   // EQTransformer: two windows per workgroup in teams of eight waves

// [TILES]
constexpr int TILES_ALT = 1;          // PhaseNet: up3 with one workgroup per tile
constexpr int TILES_EQT_REMOVED = 1;  // EQTransformer's half-width decoder tiles
constexpr int TILES_PN_REMOVED = 2;   // PhaseNet's persistent level-0 down kernel
constexpr int TILES_PN_NO_GATE = 64;  // PhaseNet's one-launch plan without the gate between device contexts (api.hip ForwardGate)

// [PN_FORM]
constexpr int PN_DEFAULT = 0;      // one launch, the core on bf16 pieces
constexpr int PN_TILED_MFMA = 1;   // three launches, all MFMA (bit-identical to the layer plan)
constexpr int PN_TILED_VALU = 2;   // three launches, level 0 on the vector ALUs
constexpr int PN_FP32_CORE = 3;    // one launch, the core on the fp32 MFMA
constexpr int PN_LEVEL0_VALU = 8;  // one launch, level 0 on the vector ALUs
inline bool pn_form_removed(int f) { return f == 4 || f == 5 || f == 6 || f == 7 || f == 9; }

// [PRE]
constexpr int PRE_PN_GATHER = 1;  // PhaseNet's one-launch plan reads the tensor gather_normalize filled
constexpr int PRE_EQT_FRONT = 2;  // EQTransformer's fused front cuts its windows itself

// [EQT] bits 0-3: keep the layer launches; 4-8: the fp32-MFMA form of a fused kernel instead of its bf16-piece form
constexpr int EQT_TAIL_LAYERS = 1 << 0;       // decoder.4 / .5 / .6+heads
constexpr int EQT_DEC03_LAYERS = 1 << 1;      // decoder.0 .. .3 and the stage-2 edge
constexpr int EQT_FRONT_LAYERS = 1 << 2;      // encoder.0 .. .2
constexpr int EQT_ENC36_LAYERS = 1 << 3;      // encoder.3 .. .6
constexpr int EQT_RES_FP32 = 1 << 4;          // eqt_res_kernel
constexpr int EQT_DEC03_FP32 = 1 << 5;        // eqt_dec03_kernel<false>
constexpr int EQT_TAIL_FP32 = 1 << 6;         // eqt_tail_kernel
constexpr int EQT_ENC36_FP32 = 1 << 7;        // eqt_enc36_kernel
constexpr int EQT_FRONT_FP32 = 1 << 8;        // eqt_front_kernel<false, ..>
constexpr int EQT_RES_ONE_WINDOW = 1 << 9;    // eqt_res3_kernel
constexpr int EQT_TAIL_WHOLE_ROW = 1 << 10;   // the tail computes every tile whatever the caller blinds
constexpr int EQT_DEC03_EVEN = 1 << 11;       // stage 3's n-tiles 12 + 12 over a SIMD's two waves
constexpr int EQT_RES_KSPLIT = 1 << 12;       // removed in round 6, rejected
constexpr int EQT_RES_TWO_REMOVED = 1 << 13;  // eqt_res3_kernel with two windows per workgroup: removed, rejected

inline int get(const vp_config& c, Index i) { return c.plan_flags[i]; }
inline bool has(const vp_config& c, Index i, int bits) { return (c.plan_flags[i] & bits) != 0; }

inline bool layer_dumps(const vp_config& c) { return has(c, DEBUG, DBG_LAYER_DUMPS); }  // "dumps requested"
inline bool clock_stamps(const vp_config& c) { return has(c, DEBUG, DBG_CLOCK); }
inline bool warm(const vp_config& c) { return get(c, WARM) != ON; }
inline bool eqt(const vp_config& c, int bits) { return has(c, EQT, bits); }
inline bool eqt_tail_whole_row(const vp_config& c) { return eqt(c, EQT_TAIL_WHOLE_ROW); }
// EQTransformer's DUMP plan exists for the default kernels only: it refuses every [EQT] bit except whole-row
inline bool eqt_dumps_refuse(const vp_config& c) { return (get(c, EQT) & ~EQT_TAIL_WHOLE_ROW) != 0; }

}  // namespace pf
}  // namespace vp
