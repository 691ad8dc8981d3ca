// Host-side Montgomery arithmetic over a scalar field (Fr), 8 x 32-bit limbs, on
// the constants of curve_consts.h: the few products the entry points need before
// a launch (domain points, the recovery's coset shift), never a hot path.
#pragma once
#include <stdint.h>

namespace kzgx {

// out = a b 2^-256 mod r (out may alias a or b)
template <class FR>
inline void fr_host_mmul(const uint32_t* a, const uint32_t* b, uint32_t* out) {
  uint32_t t[10] = {0};
  for (int i = 0; i < 8; i++) {
    uint64_t c = 0, s;
    for (int j = 0; j < 8; j++) {
      s = (uint64_t)a[j] * b[i] + t[j] + c;
      t[j] = (uint32_t)s;
      c = s >> 32;
    }
    s = (uint64_t)t[8] + c;
    t[8] = (uint32_t)s;
    t[9] = (uint32_t)(s >> 32);
    const uint32_t q = t[0] * FR::INV;
    c = ((uint64_t)q * FR::P[0] + t[0]) >> 32;
    for (int j = 1; j < 8; j++) {
      s = (uint64_t)q * FR::P[j] + t[j] + c;
      t[j - 1] = (uint32_t)s;
      c = s >> 32;
    }
    s = (uint64_t)t[8] + c;
    t[7] = (uint32_t)s;
    t[8] = t[9] + (uint32_t)(s >> 32);
  }
  bool ge = t[8] != 0;  // t < 2 r
  if (!ge) {
    int i = 7;
    while (i >= 0 && t[i] == FR::P[i]) i--;
    ge = i < 0 || t[i] > FR::P[i];
  }
  uint64_t borrow = 0;
  for (int i = 0; i < 8; i++) {
    const uint64_t d = (uint64_t)t[i] - (ge ? FR::P[i] : 0u) - borrow;
    out[i] = (uint32_t)d;
    borrow = (d >> 32) & 1;
  }
}

// out = a^-1 = a^(r - 2) for a Montgomery value a (inv(0) = 0); out may not alias a
template <class FR>
inline void fr_host_minv(const uint32_t* a, uint32_t* out) {
  for (int w = 0; w < 8; w++) out[w] = FR::ONE[w];
  for (int b = 255; b >= 0; b--) {
    fr_host_mmul<FR>(out, out, out);
    if ((FR::PM2[b >> 5] >> (b & 31)) & 1u) fr_host_mmul<FR>(out, a, out);
  }
}

}  // namespace kzgx
