// Three-piece bfloat16 operands from fp32 weights (bf16_pack.h).  Host code only.
#include "bf16_pack.h"

#include <cstring>

namespace vp {

void bf16_split3(float w, uint16_t* hi, uint16_t* mid, uint16_t* lo) {
  auto rne = [](float x) -> uint16_t {
    uint32_t u;
    memcpy(&u, &x, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
  };
  auto widen = [](uint16_t h) -> float {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
  };
  *hi = rne(w);
  const float r1 = w - widen(*hi);
  *mid = rne(r1);
  *lo = rne(r1 - widen(*mid));
}

static std::vector<float> as_floats(const std::vector<uint16_t>& o) {
  std::vector<float> f(o.size() / 2);
  memcpy(f.data(), o.data(), o.size() * 2);
  return f;
}

std::vector<float> res3_operand(const std::vector<float>& af, int taps) {
  constexpr int CB = 16;
  std::vector<uint16_t> o((size_t)4 * taps * 2 * 3 * 64 * 8);
  for (int mt = 0; mt < 4; ++mt)
    for (int tap = 0; tap < taps; ++tap)
      for (int half = 0; half < 2; ++half)
        for (int l = 0; l < 64; ++l)
          for (int i = 0; i < 8; ++i) {
            const int ci = half * 32 + 8 * (l >> 4) + i, m = l & 15;
            const float w = af[(((size_t)mt * CB + ci / 4) * taps + tap) * 64 + (ci % 4) * 16 + m];
            const size_t base = ((((size_t)mt * taps * 2 + tap * 2 + half) * 3) * 64 + l) * 8 + i;
            bf16_split3(w, &o[base], &o[base + 64 * 8], &o[base + 2 * 64 * 8]);
          }
  return as_floats(o);
}

std::vector<float> head_table3(const std::vector<float>& w, int entries, int lead) {
  std::vector<uint16_t> ht((size_t)3 * 3 * entries * 8, 0);
  for (int d = 0; d < 3; ++d)
    for (int k = 0; k <= 10; ++k)
      for (int ci = 0; ci < 8; ++ci) {
        const size_t e = ((size_t)d * 3 * entries + (k + lead)) * 8 + ci;
        bf16_split3(w[(size_t)d * 88 + ci * 11 + k], &ht[e], &ht[e + (size_t)entries * 8], &ht[e + (size_t)2 * entries * 8]);
      }
  return as_floats(ht);
}

}  // namespace vp
