// Host-only check of the three-piece bfloat16 packers (volpick_amd/csrc/bf16_pack.cpp): res3_operand for both tap counts and
// the decoder tail's head table must give, byte for byte, what the inline splits they replaced gave.  Those are kept below
// as the reference, as they stood in the ResCNN and decoder-tail planners.  No HIP runtime, no device code:
//   c++ -O2 -std=c++17 -I volpick_amd/csrc tests/bf16_pack_check.cpp volpick_amd/csrc/bf16_pack.cpp -o bf16_pack_check
// (tests/test_bf16_pack_cpu.py builds and runs it; add -fsanitize=address,undefined for a sanitizer build.)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "bf16_pack.h"

namespace {

uint16_t rne(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
float widen(uint16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
float bits(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}

std::vector<float> as_floats(const std::vector<uint16_t>& o) {
  std::vector<float> f(o.size() / 2);
  memcpy(f.data(), o.data(), o.size() * 2);
  return f;
}

// the ResCNN planner's packing before bf16_split3
std::vector<float> ref_res3_operand(const std::vector<float>& af, int taps) {
  constexpr int CB = 16;
  std::vector<uint16_t> o((size_t)4 * taps * 2 * 3 * 64 * 8);
  for (int mt = 0; mt < 4; ++mt)
    for (int tap = 0; tap < taps; ++tap)
      for (int half = 0; half < 2; ++half)
        for (int l = 0; l < 64; ++l)
          for (int i = 0; i < 8; ++i) {
            const int ci = half * 32 + 8 * (l >> 4) + i, m = l & 15;
            const float w = af[(((size_t)mt * CB + ci / 4) * taps + tap) * 64 + (ci % 4) * 16 + m];
            const uint16_t h = rne(w);
            const float r1 = w - widen(h);
            const uint16_t md = rne(r1);
            const uint16_t lo = rne(r1 - widen(md));
            const size_t base = ((((size_t)mt * taps * 2 + tap * 2 + half) * 3) * 64 + l) * 8 + i;
            o[base] = h;
            o[base + 64 * 8] = md;
            o[base + 2 * 64 * 8] = lo;
          }
  return as_floats(o);
}

// the decoder-tail planner's head table before bf16_split3
std::vector<float> ref_head_table(const std::vector<float>& w, int HT_N) {
  std::vector<uint16_t> ht((size_t)3 * 3 * HT_N * 8, 0);
  for (int d = 0; d < 3; ++d)
    for (int k = 0; k <= 10; ++k)
      for (int ci = 0; ci < 8; ++ci) {
        const float wv = w[(size_t)d * 88 + ci * 11 + k];
        const uint16_t h = rne(wv);
        const float r1 = wv - widen(h);
        const uint16_t md = rne(r1);
        const uint16_t lo = rne(r1 - widen(md));
        const size_t e = ((size_t)d * 3 * HT_N + (k + 15)) * 8 + ci;
        ht[e] = h;
        ht[e + (size_t)HT_N * 8] = md;
        ht[e + (size_t)2 * HT_N * 8] = lo;
      }
  return as_floats(ht);
}

// A few hundred floats: zeros, subnormals, +-max, infinities and NaNs, values with exactly one, two and three non-zero
// pieces, ties of the rounding, and random bit patterns.
std::vector<float> pool() {
  std::vector<float> v;
  for (uint32_t u : {0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x007fffffu, 0x807fffffu, 0x00008000u, 0x00010000u,
                     0x00800000u, 0x7f7fffffu, 0xff7fffffu, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0x7f800001u, 0xffc12345u})
    v.push_back(bits(u));
  for (int e = 1; e < 255; e += 23) {
    const uint32_t ex = (uint32_t)e << 23;
    for (uint32_t sign : {0u, 0x80000000u}) {
      v.push_back(bits(sign | ex | 0x00400000u));  // one piece: 8 significant bits
      v.push_back(bits(sign | ex | 0x007f0000u));
      v.push_back(bits(sign | ex | 0x00408000u));  // two pieces; 0x8000: a tie of the first rounding
      v.push_back(bits(sign | ex | 0x0012ff00u));
      v.push_back(bits(sign | ex | 0x00018000u));
      v.push_back(bits(sign | ex | 0x00408080u));  // three pieces; 0x80: a tie of the second rounding
      v.push_back(bits(sign | ex | 0x007fffffu));
      v.push_back(bits(sign | ex | 0x002aaaabu));
    }
  }
  uint32_t s = 0x9e3779b9u;  // xorshift32
  while (v.size() < 512) {
    s ^= s << 13, s ^= s >> 17, s ^= s << 5;
    v.push_back(bits(s));
  }
  return v;
}

bool same_bytes(const std::vector<float>& a, const std::vector<float>& b, const char* what) {
  const bool ok = a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
  printf("%-28s %8zu bytes  %s\n", what, a.size() * sizeof(float), ok ? "identical" : "DIFFERENT");
  return ok;
}

}  // namespace

int main() {
  const std::vector<float> p = pool();
  {  // the pool holds every piece count, and away from overflow and underflow (where a piece rounds to infinity or loses
     // bits below bfloat16's smallest subnormal) the three pieces add up to the value again
    size_t inexact = 0, pieces[4] = {0, 0, 0, 0};
    for (float w : p) {
      uint16_t h, m, l;
      vp::bf16_split3(w, &h, &m, &l);
      uint32_t u;
      memcpy(&u, &w, 4);
      const uint32_t ex = (u >> 23) & 0xff;
      if (ex != 0xff) ++pieces[((h & 0x7fff) != 0) + ((m & 0x7fff) != 0) + ((l & 0x7fff) != 0)];
      if (ex >= 40 && ex <= 250) inexact += widen(h) + (widen(m) + widen(l)) != w;
    }
    printf("pool: %zu values; finite with 0 / 1 / 2 / 3 non-zero pieces: %zu / %zu / %zu / %zu; inexact: %zu\n", p.size(),
           pieces[0], pieces[1], pieces[2], pieces[3], inexact);
    if (inexact || !pieces[0] || !pieces[1] || !pieces[2] || !pieces[3]) return 1;
  }
  bool ok = true;
  for (int taps : {3, 2}) {
    std::vector<float> af((size_t)4 * 16 * taps * 64);
    for (size_t i = 0; i < af.size(); ++i) af[i] = p[(i * 7 + i / p.size()) % p.size()];  // every pool value, in every lane position
    ok &= same_bytes(vp::res3_operand(af, taps), ref_res3_operand(af, taps), taps == 3 ? "res3_operand, 3 taps" : "res3_operand, 2 taps");
  }
  for (int shift = 0; shift < 2; ++shift) {
    std::vector<float> w(3 * 88);
    for (size_t i = 0; i < w.size(); ++i) w[i] = p[(i + shift * w.size()) % p.size()];
    ok &= same_bytes(vp::head_table3(w, 43, 15), ref_head_table(w, 43), "head table");
  }
  return ok ? 0 : 1;
}
