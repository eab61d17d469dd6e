// Host-only packing of fp32 weights into exact three-piece bfloat16 operands: no device code, no HIP runtime call
// (tests/bf16_pack_check.cpp links bf16_pack.cpp with the host compiler alone).
#pragma once
#include <cstdint>
#include <vector>

namespace vp {

// w as three bfloat16 pieces, each the round-to-nearest-even of what the ones before it left: hi + (mid + lo) == w in fp32
void bf16_split3(float w, uint16_t* hi, uint16_t* mid, uint16_t* lo);
// ResCNN (eqt_res.hip): fp32 MFMA-order fragments [mt][cb][tap][64] of a 64 -> 64 conv (pack_afrag) -> the three-piece operand
// [mt][tap * 2 + half][piece][64][8], two bf16 per float slot
std::vector<float> res3_operand(const std::vector<float>& afrag, int taps);
// Decoder tail (eqt_tail_b3.hip): the heads' weights w[decoder][8][11] -> the table [decoder][piece][entry][8 channels];
// entry e holds w[.][e - lead] for 0 <= e - lead <= 10, zero elsewhere.  Two bf16 per float slot
std::vector<float> head_table3(const std::vector<float>& w, int entries, int lead);

}  // namespace vp
