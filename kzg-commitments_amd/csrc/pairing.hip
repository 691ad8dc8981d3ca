// Verify path on gfx950: the G2 half of the setup, polyeval_G2 and the
// optimal ate pairing behind trusted_setup::verify_proof
// (reference src/trusted_setup.cpp:123-135 G2 SRS, :176-201 polyeval_G2,
// :230-254 verify_proof with miracl PAIR_ate + PAIR_fexp).
//
// Pairing: Miller loop on the twist in Jacobian coordinates with the line
// functions evaluated at P and placed as sparse Fp12 elements, then the
// exact final exponentiation f^((p^12 - 1)/r):
//   easy part   f^(p^6 - 1)(p^2 + 1)       (conjugate, inverse, Frobenius)
//   hard part   f^((p^4 - p^2 + 1)/r) through exact curve-parameter
//               chains with cyclotomic (Granger-Scott) squarings: BN254
//               via l0 + l1 p + l2 p^2 + p^3 in u (Scott et al.), BLS12-381
//               via K3 (x + p)(x^2 + p^2 - 1) + 1, K3 = (x - 1)^2 / 3.
// BN254 (miracl Nogami, u < 0, D-type twist): loop |6u + 2|, then
// conjugate (u < 0), then the two Frobenius lines l_{T, pi(Q)},
// l_{T + pi(Q), -pi^2(Q)}.  BLS12-381 (x < 0, M-type twist): loop |x|, then
// conjugate.  Line functions are computed up to factors in proper subfields
// (Fp2, Fp4), which the final exponentiation removes, so the value is the
// unique pairing value -- bit-exact with the oracle's definitional pairing
// (oracle/pairing_ref.py).
//
// One pairing per thread: a verify needs two, so this is latency-bound
// single-lane code by design; many pairings (batched verifies) fill waves.
#include <hip/hip_runtime.h>

#include <utility>

#include "pairing_common.hpp"
#include "kzgx_setup.hpp"

namespace kzgx {

// ---- Miller loop ----------------------------------------------------------------
// place the scaled line  w0 + w1 w + w3 w^3 (D-type) or
// (w0 + w1 w^-1 + w3 w^-3) w^3 (M-type) into Fp12
template <class C>
KZGX_DEV Fp12<C> line_to_f12(const Fp2<C>& w0, const Fp2<C>& w1, const Fp2<C>& w3) {
  using P = typename PairOf<C>::T;
  Fp12<C> l;
  l.c0 = f6_zero<C>();
  l.c1 = f6_zero<C>();
  if (P::D_TWIST) {
    l.c0.c0 = w0;  // w^0
    l.c1.c0 = w1;  // w^1
    l.c1.c1 = w3;  // w^3 = w v
  } else {
    l.c0.c0 = w3;  // w^0
    l.c0.c1 = w1;  // w^2 = v
    l.c1.c1 = w0;  // w^3
  }
  return l;
}

// tangent at T evaluated at P = (xp, yp), scaled by 2 Y Z^3; T <- 2T
template <class C>
KZGX_TW Fp12<C> line_dbl(G2J<C>& T, const F29<typename C::Fp29>& xp, const F29<typename C::Fp29>& yp) {
  const Fp2<C> A = f2_sqr<C>(T.X);
  const Fp2<C> B = f2_sqr<C>(T.Y);
  const Fp2<C> E = f2_add<C>(f2_dbl<C>(A), A);
  const Fp2<C> ZZ = f2_sqr<C>(T.Z);
  const Fp2<C> Z3 = f2_dbl<C>(f2_mul<C>(T.Y, T.Z));
  const Fp2<C> w0 = f2_mul_fp<C>(f2_mul<C>(Z3, ZZ), yp);
  const Fp2<C> w1 = f2_neg<C>(f2_mul_fp<C>(f2_mul<C>(E, ZZ), xp));
  const Fp2<C> w3 = f2_sub<C>(f2_mul<C>(E, T.X), f2_dbl<C>(B));
  T = g2_dbl<C>(T);
  return line_to_f12<C>(w0, w1, w3);
}

// line through T and q (affine) evaluated at P, scaled by 2 Z H; T <- T + q
template <class C>
KZGX_TW Fp12<C> line_add(G2J<C>& T, const G2A<C>& q, const F29<typename C::Fp29>& xp,
                         const F29<typename C::Fp29>& yp) {
  const Fp2<C> Z1Z1 = f2_sqr<C>(T.Z);
  const Fp2<C> U2 = f2_mul<C>(q.x, Z1Z1);
  const Fp2<C> S2 = f2_mul<C>(q.y, f2_mul<C>(T.Z, Z1Z1));
  const Fp2<C> H = f2_sub<C>(U2, T.X);
  const Fp2<C> rr = f2_dbl<C>(f2_sub<C>(S2, T.Y));
  const Fp2<C> Z3 = f2_dbl<C>(f2_mul<C>(T.Z, H));
  const Fp2<C> w0 = f2_mul_fp<C>(Z3, yp);
  const Fp2<C> w1 = f2_neg<C>(f2_mul_fp<C>(rr, xp));
  const Fp2<C> w3 = f2_sub<C>(f2_mul<C>(rr, q.x), f2_mul<C>(q.y, Z3));
  T = g2_add_mixed<C>(T, q);
  return line_to_f12<C>(w0, w1, w3);
}

template <class C>
KZGX_TW Fp12<C> miller_loop(const Affine<C>& p, const G2A<C>& q) {
  using P = typename PairOf<C>::T;
  Fp12<C> f = f12_one<C>();
  G2J<C> T = g2_from_affine<C>(q);
  for (int i = P::LOOP_BITS - 2; i >= 0; i--) {
    f = f12_sqr<C>(f);
    f = f12_mul<C>(f, line_dbl<C>(T, p.x, p.y));
    if ((P::LOOP[i >> 6] >> (i & 63)) & 1ull) f = f12_mul<C>(f, line_add<C>(T, q, p.x, p.y));
  }
  if (P::LOOP_NEG) {  // f_{-n} = 1/f_n up to a vertical line; 1/f == conj(f) after the final exponentiation
    f = f12_conj<C>(f);
    T.Y = f2_neg<C>(T.Y);
  }
  if (P::D_TWIST) {  // BN optimal ate: the two Frobenius lines
    const G2A<C> q1 = twist_frob<C>(q);
    G2A<C> q2 = twist_frob<C>(q1);
    q2.y = f2_neg<C>(q2.y);
    f = f12_mul<C>(f, line_add<C>(T, q1, p.x, p.y));
    f = f12_mul<C>(f, line_add<C>(T, q2, p.x, p.y));
  }
  return f;
}

// Granger-Scott squaring, valid in the cyclotomic subgroup (after the easy
// part): three Fp4 squarings, 6 Fp2 products instead of 18
template <class C>
KZGX_DEV void fp4_sqr(const Fp2<C>& a, const Fp2<C>& b, Fp2<C>& c0, Fp2<C>& c1) {
  // (a + b y)^2 with y^2 = xi: c0 = a^2 + xi b^2, c1 = 2 a b
  const Fp2<C> t = f2_mul<C>(a, b);
  c0 = f2_sub<C>(f2_sub<C>(f2_mul<C>(f2_add<C>(a, b), f2_add<C>(a, f2_mul_xi<C>(b))), t), f2_mul_xi<C>(t));
  c1 = f2_dbl<C>(t);
}
template <class C>
KZGX_TW Fp12<C> f12_cyclo_sqr(const Fp12<C>& f) {
  Fp2<C> z0 = f.c0.c0, z4 = f.c0.c1, z3 = f.c0.c2, z2 = f.c1.c0, z1 = f.c1.c1, z5 = f.c1.c2;
  Fp2<C> t0, t1, t2, t3, t4, t5;
  fp4_sqr<C>(z0, z1, t0, t1);
  fp4_sqr<C>(z2, z3, t2, t3);
  fp4_sqr<C>(z4, z5, t4, t5);
  z0 = f2_sub<C>(t0, z0);
  z0 = f2_add<C>(f2_dbl<C>(z0), t0);
  z1 = f2_add<C>(t1, z1);
  z1 = f2_add<C>(f2_dbl<C>(z1), t1);
  const Fp2<C> x5 = f2_mul_xi<C>(t5);
  z2 = f2_add<C>(x5, z2);
  z2 = f2_add<C>(f2_dbl<C>(z2), x5);
  z3 = f2_sub<C>(t4, z3);
  z3 = f2_add<C>(f2_dbl<C>(z3), t4);
  z4 = f2_sub<C>(t2, z4);
  z4 = f2_add<C>(f2_dbl<C>(z4), t2);
  z5 = f2_add<C>(t3, z5);
  z5 = f2_add<C>(f2_dbl<C>(z5), t3);
  Fp12<C> r;
  r.c0.c0 = z0;
  r.c0.c1 = z4;
  r.c0.c2 = z3;
  r.c1.c0 = z2;
  r.c1.c1 = z1;
  r.c1.c2 = z5;
  return r;
}

// f^e for f in the cyclotomic subgroup, e = (e[1]:e[0]) of `bits` bits
template <class C>
KZGX_TW Fp12<C> cyclo_pow(const Fp12<C>& f, uint64_t e0, uint64_t e1, int bits) {
  Fp12<C> acc = f;
  for (int i = bits - 2; i >= 0; i--) {
    acc = f12_cyclo_sqr<C>(acc);
    if (((i < 64 ? e0 >> i : e1 >> (i - 64)) & 1ull)) acc = f12_mul<C>(acc, f);
  }
  return acc;
}

// f^z for the curve parameter z (BN: u, BLS: x); z < 0 -> unitary inverse
template <class C>
KZGX_DEV Fp12<C> cyclo_pow_z(const Fp12<C>& f) {
  using P = typename PairOf<C>::T;
  constexpr int bits = 64 - __builtin_clzll(P::Z_ABS);
  const Fp12<C> r = cyclo_pow<C>(f, P::Z_ABS, 0, bits);
  return P::Z_NEG ? f12_conj<C>(r) : r;
}

// g^n for a small constant n >= 1 (cyclotomic g)
template <class C>
KZGX_DEV Fp12<C> cyclo_pow_small(const Fp12<C>& g, uint32_t n) {
  return cyclo_pow<C>(g, n, 0, 32 - __builtin_clz(n));
}

// exact final exponentiation f^((p^12 - 1)/r)
template <class C>
KZGX_TW Fp12<C> final_exp(const Fp12<C>& f) {
  using P = typename PairOf<C>::T;
  // easy part: f^(p^6 - 1) (p^2 + 1) -> cyclotomic subgroup
  Fp12<C> g = f12_mul<C>(f12_conj<C>(f), f12_inv<C>(f));
  g = f12_mul<C>(f12_frob<C>(f12_frob<C>(g)), g);
  if (P::IS_BN) {
    // (p^4 - p^2 + 1)/r = l0 + l1 p + l2 p^2 + p^3 (exact, Scott et al.):
    //   l2 = 6u^2 + 1, l1 = -36u^3 - 18u^2 - 12u + 1, l0 = -36u^3 - 30u^2 - 18u - 2
    const Fp12<C> a = cyclo_pow_z<C>(g);  // g^u
    const Fp12<C> b = cyclo_pow_z<C>(a);  // g^(u^2)
    const Fp12<C> c = cyclo_pow_z<C>(b);  // g^(u^3)
    const Fp12<C> c36 = cyclo_pow_small<C>(c, 36);
    const Fp12<C> g2 = f12_cyclo_sqr<C>(g);
    const Fp12<C> f0 = f12_conj<C>(f12_mul<C>(f12_mul<C>(c36, cyclo_pow_small<C>(b, 30)),
                                              f12_mul<C>(cyclo_pow_small<C>(a, 18), g2)));
    const Fp12<C> f1 =
        f12_mul<C>(f12_conj<C>(f12_mul<C>(c36, f12_mul<C>(cyclo_pow_small<C>(b, 18), cyclo_pow_small<C>(a, 12)))), g);
    const Fp12<C> f2 = f12_mul<C>(cyclo_pow_small<C>(b, 6), g);
    Fp12<C> r = f12_mul<C>(f0, f12_frob<C>(f1));
    r = f12_mul<C>(r, f12_frob<C>(f12_frob<C>(f2)));
    return f12_mul<C>(r, f12_frob<C>(f12_frob<C>(f12_frob<C>(g))));
  }
  // BLS12: (p^4 - p^2 + 1)/r = K3 (x + p)(x^2 + p^2 - 1) + 1, K3 = (x - 1)^2 / 3
  const Fp12<C> t = cyclo_pow<C>(g, P::K3[0], P::K3[1], P::K3_BITS);
  const Fp12<C> t2 = f12_mul<C>(cyclo_pow_z<C>(t), f12_frob<C>(t));  // t^(x + p)
  const Fp12<C> t3 = f12_mul<C>(f12_mul<C>(cyclo_pow_z<C>(cyclo_pow_z<C>(t2)), f12_frob<C>(f12_frob<C>(t2))),
                                f12_conj<C>(t2));  // t2^(x^2 + p^2 - 1)
  return f12_mul<C>(t3, g);
}

// thread per pairing: e(P_k, Q_k) for canonical affine inputs (all-zero or
// flagged = infinity -> 1), canonical Fp12 out in tower order
template <class C>
__global__ __launch_bounds__(64) void k_pairing(const uint32_t* __restrict__ g1, const uint32_t* __restrict__ g1_inf,
                                                const uint32_t* __restrict__ g2, const uint32_t* __restrict__ g2_inf,
                                                uint32_t count, uint32_t* __restrict__ out) {
  constexpr int N = C::Fp::N;
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  Affine<C> p;
  G2A<C> q;
  const bool pf = affine_from_canonical<C>(g1 + (size_t)k * 2 * N, p) && !(g1_inf && g1_inf[k]);
  const bool qf = g2_from_canon<C>(g2 + (size_t)k * 4 * N, q) && !(g2_inf && g2_inf[k]);
  Fp12<C> r = f12_one<C>();
  if (pf && qf) r = final_exp<C>(miller_loop<C>(p, q));
  f12_to_canon<C>(r, out + (size_t)k * 12 * N);
}

// ---- G2 SRS and polyeval_G2 ---------------------------------------------------------
// [tau^(start + i)] G2, thread per point (generate_elements_range,
// trusted_setup.cpp:123-135)
template <class C>
KZGX_TW G2J<C> g2_mul_words(const G2A<C>& q, const uint32_t (&e)[8]) {
  G2J<C> acc = g2_inf<C>();
  for (int b = 255; b >= 0; b--) {
    acc = g2_dbl<C>(acc);
    if ((e[b >> 5] >> (b & 31)) & 1u) acc = g2_add_mixed<C>(acc, q);
  }
  return acc;
}

template <class C>
__global__ __launch_bounds__(64) void k_gen_srs_g2(const uint32_t* __restrict__ tau_canon, uint64_t start,
                                                   uint32_t n, uint32_t* __restrict__ out) {
  using P = typename PairOf<C>::T;
  using FR = typename C::Fr;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fe<FR> tm = fe_to_mont<FR>(fe_load<FR>(tau_canon));
  const uint64_t ex = start + i;
  Fe<FR> e = fe_one<FR>();
  for (int b = 63; b >= 0; b--) {
    e = fe_sqr<FR>(e);
    if ((ex >> b) & 1ull) e = fe_mul<FR>(e, tm);
  }
  e = fe_from_mont<FR>(e);
  G2A<C> g;
  g.x = f2_const<C>(P::G2X);
  g.y = f2_const<C>(P::G2Y);
  uint32_t ew[8];
  for (int k = 0; k < 8; k++) ew[k] = e.v[k];
  G2A<C> a;
  const bool fin = g2_to_affine<C>(g2_mul_words<C>(g, ew), a);
  g2_to_canon<C>(a, fin, out + (size_t)i * 4 * C::Fp::N);
}

// term i: c_i [tau^i]G2 (canonical scalar words, SRS canonical affine), Jacobian out
template <class C>
__global__ __launch_bounds__(64) void k_g2_terms(const uint32_t* __restrict__ scalars, const uint32_t* __restrict__ srs2,
                                                 uint32_t n, G2J<C>* __restrict__ terms) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  G2A<C> q;
  const bool fin = g2_from_canon<C>(srs2 + (size_t)i * 4 * C::Fp::N, q);
  uint32_t e[8];
  for (int k = 0; k < 8; k++) e[k] = scalars[(size_t)i * 8 + k];
  terms[i] = fin ? g2_mul_words<C>(q, e) : g2_inf<C>();
}

// one workgroup of 64: strided partial sums, then lane 0 folds and normalizes
template <class C>
__global__ __launch_bounds__(64) void k_g2_sum(const G2J<C>* __restrict__ terms, uint32_t n, G2J<C>* __restrict__ part,
                                               uint32_t* __restrict__ out, uint32_t* __restrict__ out_inf) {
  const uint32_t t = threadIdx.x;
  G2J<C> acc = g2_inf<C>();
  for (uint32_t i = t; i < n; i += 64) acc = g2_add<C>(acc, terms[i]);
  part[t] = acc;
  __syncthreads();
  if (t != 0) return;
  for (uint32_t k = 1; k < 64; k++) acc = g2_add<C>(acc, part[k]);
  G2A<C> a;
  const bool fin = g2_to_affine<C>(acc, a);
  g2_to_canon<C>(a, fin, out);
  *out_inf = fin ? 0u : 1u;
}

// Windowed G2 MSM: tab[i][w] = 2^(B w) G2[i] (affine Montgomery, zeros for
// an infinite SRS point), so term i = sum_w d_(i,w) tab[i][w] with B-bit
// digits (B = G2_TAB_BITS): one thread per (term, window) runs at most B
// doublings and B additions instead of a 256-bit double-and-add, and the
// n 256/B partial points are folded 2:1 per pass, then by a one-workgroup
// tree.  Every lone-lane G2 operation is ~27 us, so B = 8 (a chain of ~12
// operations, one more fold level) beats round 5's B = 16 (~24) by ~0.3 ms.
constexpr int G2_TAB_W = G2_TAB_WINDOWS;

template <class C>
__global__ __launch_bounds__(64) void k_g2_tab(const uint32_t* __restrict__ srs2, uint32_t n,
                                               G2A<C>* __restrict__ tab) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  G2A<C> q;
  const bool fin = g2_from_canon<C>(srs2 + (size_t)i * 4 * C::Fp::N, q);
  G2J<C> b = g2_from_affine<C>(q);
  for (int w = 0; w < G2_TAB_W; w++) {
    G2A<C> a;
    if (!fin || !g2_to_affine<C>(b, a)) a.x = a.y = f2_zero<C>();
    tab[(size_t)i * G2_TAB_W + w] = a;
    if (w + 1 < G2_TAB_W)
      for (int k = 0; k < G2_TAB_BITS; k++) b = g2_dbl<C>(b);
  }
}

template <class C>
__global__ __launch_bounds__(64) void k_g2_terms_w(const uint32_t* __restrict__ scalars,
                                                   const uint32_t* __restrict__ srs2, const G2A<C>* __restrict__ tab,
                                                   uint32_t n, G2J<C>* __restrict__ terms) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * G2_TAB_W) return;
  const uint32_t i = t / G2_TAB_W, w = t % G2_TAB_W;
  const uint32_t d =
      (scalars[(size_t)i * 8 + ((G2_TAB_BITS * w) >> 5)] >> ((G2_TAB_BITS * w) & 31)) & ((1u << G2_TAB_BITS) - 1u);
  G2A<C> q;
  G2J<C> acc = g2_inf<C>();
  if (d != 0 && g2_from_canon<C>(srs2 + (size_t)i * 4 * C::Fp::N, q)) {
    const G2A<C> b = tab[t];
    for (int k = 31 - __builtin_clz(d); k >= 0; k--) {
      acc = g2_dbl<C>(acc);
      if ((d >> k) & 1u) acc = g2_add_mixed<C>(acc, b);
    }
  }
  terms[t] = acc;
}

// out[t] = sum of in[F t .. F t + F - 1] (bounded by count).  F = 2: a G2
// addition on a lone lane is ~35 us, so the fold runs as a tree of 2:1
// levels (depth log2 of the term count) -- round 5's 8:1 passes chained 7
// additions per pass (~260 us each; a 128-point multi-proof verify spent
// 1.56 ms in polyeval_G2, round 6 trace)
template <class C, uint32_t F>
__global__ __launch_bounds__(64) void k_g2_fold(const G2J<C>* __restrict__ in, uint32_t count,
                                                G2J<C>* __restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t * F >= count) return;
  G2J<C> acc = in[t * F];
  for (uint32_t k = t * F + 1; k < count && k < t * F + F; k++) acc = g2_add<C>(acc, in[k]);
  out[t] = acc;
}

// <= 64 points: one workgroup, LDS tree, lane 0 normalizes
template <class C>
__global__ __launch_bounds__(64) void k_g2_sum_tree(const G2J<C>* __restrict__ in, uint32_t count,
                                                    uint32_t* __restrict__ out, uint32_t* __restrict__ out_inf) {
  __shared__ G2J<C> part[64];
  const uint32_t t = threadIdx.x;
  part[t] = t < count ? in[t] : g2_inf<C>();
  __syncthreads();
  uint32_t s0 = 32;
  while (s0 > 1 && s0 >= count) s0 >>= 1;  // levels above the count hold only the identity
  for (uint32_t s = s0; s >= 1; s >>= 1) {
    if (t < s) part[t] = g2_add<C>(part[t], part[t + s]);
    __syncthreads();
  }
  if (t != 0) return;
  G2A<C> a;
  const bool fin = g2_to_affine<C>(part[0], a);
  g2_to_canon<C>(a, fin, out);
  *out_inf = fin ? 0u : 1u;
}

// ok[k] = 1 if point k is a valid (finite) G2 point: coordinates < m and on
// the twist y^2 = x^3 + b'
template <class C>
__global__ __launch_bounds__(64) void k_g2_validate(const uint32_t* __restrict__ xy, uint32_t count,
                                                    uint32_t* __restrict__ ok) {
  using P = typename PairOf<C>::T;
  constexpr int N = C::Fp::N;
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const uint32_t* w = xy + (size_t)k * 4 * N;
  bool lt = true;
  for (int c = 0; c < 4; c++) lt = lt && canon_lt_m<C>(w + c * N);
  G2A<C> q;
  const bool fin = g2_from_canon<C>(w, q);
  const Fp2<C> d = f2_sub<C>(f2_sqr<C>(q.y), f2_add<C>(f2_mul<C>(f2_sqr<C>(q.x), q.x), f2_const<C>(P::B2)));
  ok[k] = (lt && fin && f2_is_zero<C>(d)) ? 1u : 0u;
}

// out = a - b for canonical affine G1 points (the C - [I(tau)]G1 of
// verify_proof, trusted_setup.cpp:245-247)
template <class C>
__global__ __launch_bounds__(64) void k_g1_sub(const uint32_t* __restrict__ a, const uint32_t* __restrict__ a_inf,
                         const uint32_t* __restrict__ b, const uint32_t* __restrict__ b_inf, uint32_t* __restrict__ out,
                         uint32_t* __restrict__ out_inf) {
  // every lane of the one wave holds the same point: the conversion's
  // inversion runs wave-uniform (xyzz_to_canonical_lane), lane 0 stores
  constexpr int N = C::Fp::N;
  Xyzz<C> acc = xyzz_inf<C>();
  Affine<C> pa, pb;
  if (affine_from_canonical<C>(a, pa) && !(a_inf && *a_inf)) acc = xyzz_from_affine<C>(pa);
  if (affine_from_canonical<C>(b, pb) && !(b_inf && *b_inf)) acc = xyzz_add_affine<C>(acc, affine_neg<C>(pb));
  uint32_t wx[N], wy[N];
  const bool fin = xyzz_to_canonical_lane<C>(acc, wx, wy);
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int k = 0; k < N; k++) {
    out[k] = wx[k];
    out[N + k] = wy[k];
  }
  *out_inf = fin ? 0u : 1u;
}

// per-cell verification (kzgx_verify_cells_each): lane k writes
// out[k] = commits[commit_index[k]] - b[k], canonical affine with an infinity
// flag.  The commitment is gathered only when bad[k] == 0 (its index is then
// in range); a bad cell gets -b[k], and its verdict is forced to 0 afterwards.
// The additions are complete: equal operands give infinity, opposite ones the
// doubling.
template <class C>
__global__ __launch_bounds__(64) void k_cells_sub(const uint32_t* __restrict__ commits,
                                                  const uint32_t* __restrict__ commit_inf,
                                                  const uint32_t* __restrict__ commit_index,
                                                  const uint32_t* __restrict__ bad, const uint32_t* __restrict__ b,
                                                  const uint32_t* __restrict__ b_inf, uint32_t count,
                                                  uint32_t* __restrict__ out, uint32_t* __restrict__ out_inf) {
  constexpr int N = C::Fp::N;
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  Xyzz<C> acc = xyzz_inf<C>();
  Affine<C> pa, pb;
  if (!bad[k]) {
    const uint32_t c = commit_index[k];
    if (affine_from_canonical<C>(commits + (size_t)c * 2 * N, pa) && !(commit_inf && commit_inf[c]))
      acc = xyzz_from_affine<C>(pa);
  }
  if (affine_from_canonical<C>(b + (size_t)k * 2 * N, pb) && !b_inf[k])
    acc = xyzz_add_affine<C>(acc, affine_neg<C>(pb));
  Affine<C> d;
  const bool fin = xyzz_to_affine<C>(acc, d);
  affine_to_canonical<C>(out + (size_t)k * 2 * N, d, fin);
  out_inf[k] = fin ? 0u : 1u;
}

// ---- batched single-point verify -----------------------------------------------
// thread per opening: verify_proof with one point (x = z, y), i.e.
//   e(pi, [tau - z]G2) == e(C - [y]G1, G2)
//   <=> e(pi, [tau]G2) * e(-(C - [y]G1 + [z]pi), G2) == 1,
// one product of two Miller loops and ONE final exponentiation.  The
// boolean is that of the reference (trusted_setup.cpp:230-254 with
// I = y, Z = X - z).  G1[0] = G, G2[0] = G2, G2[1] = [tau]G2 from the setup.
template <class C>
__global__ __launch_bounds__(64) void k_verify_single(const uint32_t* __restrict__ commits,
                                                      const uint32_t* __restrict__ commit_inf,
                                                      const uint32_t* __restrict__ proofs,
                                                      const uint32_t* __restrict__ proof_inf,
                                                      const uint32_t* __restrict__ zs, const uint32_t* __restrict__ ys,
                                                      uint32_t count, const uint32_t* __restrict__ g1_0,
                                                      const uint32_t* __restrict__ g2_01, uint32_t* __restrict__ ok) {
  constexpr int N = C::Fp::N;
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  Affine<C> c, pi, g;
  const bool cf = affine_from_canonical<C>(commits + (size_t)k * 2 * N, c) && !(commit_inf && commit_inf[k]);
  const bool pf = affine_from_canonical<C>(proofs + (size_t)k * 2 * N, pi) && !(proof_inf && proof_inf[k]);
  const bool gf = affine_from_canonical<C>(g1_0, g);
  uint32_t zw[8], yw[8];
  for (int i = 0; i < 8; i++) {
    zw[i] = zs[(size_t)k * 8 + i];
    yw[i] = ys[(size_t)k * 8 + i];
  }
  // D = C - [y]G + [z]pi
  Xyzz<C> d = xyzz_inf<C>();
  if (gf) d = xyzz_neg<C>(g1_mul_words<C>(g, yw));
  if (cf) d = xyzz_add_affine<C>(d, c);
  if (pf) d = xyzz_add<C>(d, g1_mul_words<C>(pi, zw));
  Affine<C> dn;
  const bool df = xyzz_to_affine<C>(d, dn);
  G2A<C> g2, tg2;
  const bool g2f = g2_from_canon<C>(g2_01, g2);
  const bool tg2f = g2_from_canon<C>(g2_01 + 4 * N, tg2);
  Fp12<C> f = f12_one<C>();
  if (pf && tg2f) f = miller_loop<C>(pi, tg2);
  if (df && g2f) {
    dn = affine_neg<C>(dn);
    f = f12_mul<C>(f, miller_loop<C>(dn, g2));
  }
  const Fp12<C> e = final_exp<C>(f);
  uint32_t w[12 * N];
  f12_to_canon<C>(e, w);
  uint32_t bad = w[0] ^ 1u;  // == 1 in Fp12: coefficient 0 is 1, all others 0
  for (int i = 1; i < 12 * N; i++) bad |= w[i];
  ok[k] = bad == 0 ? 1u : 0u;
}

// ---- host side ----------------------------------------------------------------
template <class C>
static int pairing_impl(const uint32_t* g1, const uint32_t* g1_inf, const uint32_t* g2, const uint32_t* g2_inf,
                        size_t count, uint32_t* out, hipStream_t st) {
  hipLaunchKernelGGL(k_pairing<C>, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, st, g1, g1_inf, g2, g2_inf,
                     (uint32_t)count, out);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

int pairing_batch(Ctx* ctx, const uint32_t* d_g1, const uint32_t* d_g1_inf, const uint32_t* d_g2,
                  const uint32_t* d_g2_inf, size_t count, uint32_t* d_out, hipStream_t st) {
  if (count == 0) return KZGX_OK;
  return ctx->curve == KZGX_CURVE_BN254 ? pairing_impl<BN254G1>(d_g1, d_g1_inf, d_g2, d_g2_inf, count, d_out, st)
                                        : pairing_impl<BLS12381G1>(d_g1, d_g1_inf, d_g2, d_g2_inf, count, d_out, st);
}

int gen_srs_g2_points(Ctx* ctx, const uint32_t* d_tau, size_t start, size_t n, uint32_t* d_out, hipStream_t st) {
  dim3 blk(64), grd((unsigned)((n + 63) / 64));
  if (ctx->curve == KZGX_CURVE_BN254)
    hipLaunchKernelGGL(k_gen_srs_g2<BN254G1>, grd, blk, 0, st, d_tau, (uint64_t)start, (uint32_t)n, d_out);
  else
    hipLaunchKernelGGL(k_gen_srs_g2<BLS12381G1>, grd, blk, 0, st, d_tau, (uint64_t)start, (uint32_t)n, d_out);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

template <class C>
static int msm_g2_windowed(Ctx* ctx, const uint32_t* d_scalars, const uint32_t* d_srs2, const uint32_t* d_tab,
                           size_t n, uint32_t* d_out, uint32_t* d_out_inf, hipStream_t st) {
  const size_t m = n * G2_TAB_W;
  const size_t tb = (m + (m + 1) / 2 + 64) * sizeof(G2J<C>);  // terms, then the 2:1 ping-pong half
  KZGX_TRY(dev_alloc(ctx, &ctx->d_g2_ws, tb, &ctx->g2_ws_b));
  G2J<C>* a = (G2J<C>*)ctx->d_g2_ws;
  G2J<C>* b = a + m;
  {
    ProfScope p(ctx, st, "g2_terms");
    hipLaunchKernelGGL(k_g2_terms_w<C>, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, st, d_scalars, d_srs2,
                       (const G2A<C>*)d_tab, (uint32_t)n, a);
  }
  size_t cnt = m;
  while (cnt > 8) {
    const size_t nxt = (cnt + 1) / 2;
    hipLaunchKernelGGL((k_g2_fold<C, 2>), dim3((unsigned)((nxt + 63) / 64)), dim3(64), 0, st, a, (uint32_t)cnt, b);
    std::swap(a, b);
    cnt = nxt;
  }
  hipLaunchKernelGGL(k_g2_sum_tree<C>, dim3(1), dim3(64), 0, st, a, (uint32_t)cnt, d_out, d_out_inf);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

size_t g2_table_bytes(int curve, size_t n) {
  return n * G2_TAB_W * (curve == KZGX_CURVE_BN254 ? sizeof(G2A<BN254G1>) : sizeof(G2A<BLS12381G1>));
}

int g2_table_build(Ctx* ctx, const uint32_t* d_srs2, size_t n, uint32_t* d_tab, hipStream_t st) {
  dim3 blk(64), grd((unsigned)((n + 63) / 64));
  ProfScope p(ctx, st, "g2_table");
  if (ctx->curve == KZGX_CURVE_BN254)
    hipLaunchKernelGGL(k_g2_tab<BN254G1>, grd, blk, 0, st, d_srs2, (uint32_t)n, (G2A<BN254G1>*)d_tab);
  else
    hipLaunchKernelGGL(k_g2_tab<BLS12381G1>, grd, blk, 0, st, d_srs2, (uint32_t)n, (G2A<BLS12381G1>*)d_tab);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

template <class C>
static int msm_g2_impl(Ctx* ctx, const uint32_t* d_scalars, const uint32_t* d_srs2, size_t n, uint32_t* d_out,
                       uint32_t* d_out_inf, hipStream_t st) {
  const size_t tb = (n + 64) * sizeof(G2J<C>);
  KZGX_TRY(dev_alloc(ctx, &ctx->d_g2_ws, tb, &ctx->g2_ws_b));
  G2J<C>* terms = (G2J<C>*)ctx->d_g2_ws;
  G2J<C>* part = terms + n;
  {
    ProfScope p(ctx, st, "g2_terms");
    hipLaunchKernelGGL(k_g2_terms<C>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, d_scalars, d_srs2,
                       (uint32_t)n, terms);
  }
  hipLaunchKernelGGL(k_g2_sum<C>, dim3(1), dim3(64), 0, st, terms, (uint32_t)n, part, d_out, d_out_inf);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

// msm_g2_windowed's workspace for an n-point G2 MSM (setup time)
int g2_ws_reserve(Ctx* ctx, size_t n) {
  const size_t m = n * G2_TAB_W;
  const size_t gj = ctx->curve == KZGX_CURVE_BN254 ? sizeof(G2J<BN254G1>) : sizeof(G2J<BLS12381G1>);
  return dev_alloc(ctx, &ctx->d_g2_ws, (m + (m + 1) / 2 + 64) * gj, &ctx->g2_ws_b);
}

int msm_g2(Ctx* ctx, const uint32_t* d_scalars, const uint32_t* d_srs2, size_t n, uint32_t* d_out,
           uint32_t* d_out_inf, hipStream_t st, const uint32_t* d_tab) {
  if (n == 0) {  // ECP2_inf (trusted_setup.cpp:177-181)
    const size_t pb = 4 * (size_t)ctx->base_words() * 4;
    KZGX_TRY_HIP(hipMemsetAsync(d_out, 0, pb, st));
    const uint32_t one = 1;
    KZGX_TRY_HIP(hipMemcpyAsync(d_out_inf, &one, 4, hipMemcpyHostToDevice, st));
    KZGX_TRY_HIP(hipStreamSynchronize(st));
    return KZGX_OK;
  }
  if (d_tab)
    return ctx->curve == KZGX_CURVE_BN254
               ? msm_g2_windowed<BN254G1>(ctx, d_scalars, d_srs2, d_tab, n, d_out, d_out_inf, st)
               : msm_g2_windowed<BLS12381G1>(ctx, d_scalars, d_srs2, d_tab, n, d_out, d_out_inf, st);
  return ctx->curve == KZGX_CURVE_BN254 ? msm_g2_impl<BN254G1>(ctx, d_scalars, d_srs2, n, d_out, d_out_inf, st)
                                        : msm_g2_impl<BLS12381G1>(ctx, d_scalars, d_srs2, n, d_out, d_out_inf, st);
}

int g2_validate(Ctx* ctx, const uint32_t* d_xy, size_t count, uint32_t* d_ok, hipStream_t st) {
  if (count == 0) return KZGX_OK;
  dim3 blk(64), grd((unsigned)((count + 63) / 64));
  if (ctx->curve == KZGX_CURVE_BN254)
    hipLaunchKernelGGL(k_g2_validate<BN254G1>, grd, blk, 0, st, d_xy, (uint32_t)count, d_ok);
  else
    hipLaunchKernelGGL(k_g2_validate<BLS12381G1>, grd, blk, 0, st, d_xy, (uint32_t)count, d_ok);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

int verify_single_batch(Ctx* ctx, const uint32_t* d_commits, const uint32_t* d_commit_inf, const uint32_t* d_proofs,
                        const uint32_t* d_proof_inf, const uint32_t* d_z, const uint32_t* d_y, size_t count,
                        const uint32_t* d_g1_0, const uint32_t* d_g2_01, uint32_t* d_ok, hipStream_t st) {
  if (count == 0) return KZGX_OK;
  dim3 blk(64), grd((unsigned)((count + 63) / 64));
  ProfScope p(ctx, st, "verify_single");
  if (ctx->curve == KZGX_CURVE_BN254)
    hipLaunchKernelGGL(k_verify_single<BN254G1>, grd, blk, 0, st, d_commits, d_commit_inf, d_proofs, d_proof_inf, d_z,
                       d_y, (uint32_t)count, d_g1_0, d_g2_01, d_ok);
  else
    hipLaunchKernelGGL(k_verify_single<BLS12381G1>, grd, blk, 0, st, d_commits, d_commit_inf, d_proofs, d_proof_inf,
                       d_z, d_y, (uint32_t)count, d_g1_0, d_g2_01, d_ok);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

int cells_sub(Ctx* ctx, const uint32_t* d_commits, const uint32_t* d_commit_inf, const uint32_t* d_commit_index,
              const uint32_t* d_bad, const uint32_t* d_b, const uint32_t* d_b_inf, size_t count, uint32_t* d_out,
              uint32_t* d_out_inf, hipStream_t st) {
  if (count == 0) return KZGX_OK;
  dim3 blk(64), grd((unsigned)((count + 63) / 64));
  ProfScope p(ctx, st, "cells_sub");
  if (ctx->curve == KZGX_CURVE_BN254)
    hipLaunchKernelGGL(k_cells_sub<BN254G1>, grd, blk, 0, st, d_commits, d_commit_inf, d_commit_index, d_bad, d_b,
                       d_b_inf, (uint32_t)count, d_out, d_out_inf);
  else
    hipLaunchKernelGGL(k_cells_sub<BLS12381G1>, grd, blk, 0, st, d_commits, d_commit_inf, d_commit_index, d_bad, d_b,
                       d_b_inf, (uint32_t)count, d_out, d_out_inf);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

int g1_sub(Ctx* ctx, const uint32_t* d_a, const uint32_t* d_a_inf, const uint32_t* d_b, const uint32_t* d_b_inf,
           uint32_t* d_out, uint32_t* d_out_inf, hipStream_t st) {
  if (ctx->curve == KZGX_CURVE_BN254)
    hipLaunchKernelGGL(k_g1_sub<BN254G1>, dim3(1), dim3(64), 0, st, d_a, d_a_inf, d_b, d_b_inf, d_out, d_out_inf);
  else
    hipLaunchKernelGGL(k_g1_sub<BLS12381G1>, dim3(1), dim3(64), 0, st, d_a, d_a_inf, d_b, d_b_inf, d_out, d_out_inf);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

}  // namespace kzgx

namespace kzgx {
// device bring-up (kzgx_setup.hpp): one launch loads this code object
__global__ void k_warm_pairing() {}
int warm_pairing(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_pairing, dim3(1), dim3(64), 0, st);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}
}  // namespace kzgx
