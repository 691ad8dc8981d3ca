// The per-point tests shared by the batched validation (subgroup.hip) and the
// decompression of compressed points (codec.hip): canonical and on the curve,
// and membership in the order-r subgroup of G1 / G2.  subgroup.hip's header
// comment derives the tests; both kernels of a kind run the same chain.
#pragma once
#include "tower.hpp"

namespace kzgx {

// canonical and on the curve, k_g1_validate's test; a: the point in Montgomery form
template <class C>
KZGX_DEV bool g1_canonical_on_curve(const uint32_t* __restrict__ xy, Affine<C>& a) {
  using F = typename C::Fp29;
  constexpr int N = C::Fp::N;
  bool lt = true;
  for (int c = 0; c < 2; c++) {
    int cmp = 0;  // coordinate vs modulus, most significant word first
    for (int i = N - 1; i >= 0 && cmp == 0; i--) {
      const uint32_t w = xy[c * N + i], m = C::Fp::P[i];
      cmp = w < m ? -1 : (w > m ? 1 : 0);
    }
    lt = lt && cmp < 0;
  }
  const bool finite = affine_from_canonical<C>(xy, a);
  uint32_t bw[N];
  for (int i = 0; i < N; i++) bw[i] = i == 0 ? C::BSMALL : 0u;
  const F29<F> b = f29_to_mont<F>(f29_from_words<F, N>(bw));
  const F29<F> y2 = f29_sqr<F>(a.y);
  const F29<F> x3 = f29_mul<F>(f29_sqr<F>(a.x), a.x);
  const F29<F> d = f29_sub<F>(y2, f29_add<F>(x3, b), F::P4);  // < 6m
  return lt && finite && f29_is_zero<F>(d);
}

// [x^2]P == (beta x, -y) for a finite curve point P = a (Montgomery, < m): the
// membership test of a curve with a cofactor.  Wave-uniform: the exponent is a
// compile-time constant.  The caller hands a masked lane the generator.
template <class C>
KZGX_DEV bool g1_in_subgroup(const Affine<C>& a) {
  using F = typename C::Fp29;
  Xyzz<C> acc = xyzz_from_affine<C>(a);  // the top bit of x^2
  for (int b = C::X2_BITS - 2; b >= 0; b--) {
    acc = xyzz_dbl<C>(acc);
    if ((C::X2[b >> 6] >> (b & 63)) & 1ull) acc = xyzz_add_affine<C>(acc, a);
  }
  // X = beta x ZZ and Y + y ZZZ = 0, ZZ != 0
  const F29<F> bx = f29_mul<F>(f29_const<F>(C::BETA29), a.x);                       // < 2m
  const F29<F> dx = f29_sub<F>(acc.X, f29_mul<F>(bx, acc.ZZ), F::P2);               // < 10m
  const F29<F> dy = f29_add<F>(acc.Y, f29_mul<F>(a.y, acc.ZZZ));                    // < 6m
  return !xyzz_is_inf<C>(acc) && f29_is_zero<F>(dx) && f29_is_zero<F>(dy);
}

// [r]Q == O for a finite twist point Q, by the definition (g2_add_mixed is
// complete: a small-order point walks through O exactly)
template <class C>
KZGX_DEV bool g2_in_subgroup(const G2A<C>& q) {
  using FR = typename C::Fr;
  G2J<C> acc = g2_from_affine<C>(q);  // the top bit of r
  for (int b = FR::BITS - 2; b >= 0; b--) {
    acc = g2_dbl<C>(acc);
    if ((FR::P[b >> 5] >> (b & 31)) & 1u) acc = g2_add_mixed<C>(acc, q);
  }
  return g2_is_inf<C>(acc);
}

}  // namespace kzgx
