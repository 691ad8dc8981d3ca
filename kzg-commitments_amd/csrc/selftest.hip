// Device harness for single field and point primitives (kzgx_debug_prim):
// one primitive of field29.hpp, field.hpp or curve.hpp per launch, on raw
// limbs handed in by the caller, so a test can feed non-canonical and
// unnormalized representatives at the documented bounds and compare every
// output limb with an exact integer model (oracle/field_model.py,
// tests/test_gpu_primitives.py).
//
// Tuple t runs on thread t of 64-thread blocks: every lane of a wave carries
// a different value.  The wave-uniform forms (f29_inv_uniform,
// f29_inv_uniform_raw, xyzz_to_affine_impl<C, true>) take one tuple per
// block, loaded by every lane, and `mode` chooses the active lanes of the
// call: 0 = all 64, 1 = lanes 0-3 (combine4), 2 = lane 0 (the sequential
// fallback).  Every form is named explicitly: this translation unit is built
// with the library's default flags and defines none of the form switches.
//
// This checks the source-level arithmetic as compiled here, not the code
// generated for each kernel that inlines these templates.
#include <hip/hip_runtime.h>

#include <utility>

#include "curve.hpp"
#include "kzgx_internal.hpp"

namespace kzgx {

// operation ids (oracle/field_model.py PRIM_OPS mirrors this list)
enum PrimOp : int {
  PRIM_MUL = 0,
  PRIM_MUL_LAT,
  PRIM_MUL_CHAIN,
  PRIM_SQR,
  PRIM_SQR_CHAIN,
  PRIM_MUL2,
  PRIM_MUL2_LAT,
  PRIM_MUL2_CHAIN,
  PRIM_MUL_X2,
  PRIM_SQR_X2,
  PRIM_SQR_X2_PAIR,
  PRIM_MUL_X3,
  PRIM_MUL2_MUL,
  PRIM_MUL2_X3,
  PRIM_ADD,
  PRIM_SUB_P2,
  PRIM_SUB_P4,
  PRIM_SUB_P6,
  PRIM_SUB_P8,
  PRIM_SUB_P10,
  PRIM_SUB_P16,
  PRIM_NEG_LAZY,
  PRIM_NEG8_LAZY,
  PRIM_ADD_2X_LAZY,
  PRIM_NORMALIZE,
  PRIM_CSUB_P,
  PRIM_CSUB_P2,
  PRIM_CSUB_P4,
  PRIM_CSUB_P6,
  PRIM_CSUB_P8,
  PRIM_CSUB_P10,
  PRIM_CSUB_P16,
  PRIM_REDUCE,
  PRIM_IS_ZERO_LT2M,
  PRIM_IS_ZERO,
  PRIM_TO_MONT,
  PRIM_FROM_MONT,
  PRIM_FROM_WORDS,
  PRIM_TO_WORDS,
  PRIM_INV,
  PRIM_INV_VT,
  PRIM_INV_UNIFORM,
  PRIM_INV_UNIFORM_RAW,
  // field.hpp on the scalar field, then the same nine on the base field
  PRIM_FR_ADD,
  PRIM_FR_SUB,
  PRIM_FR_NEG,
  PRIM_FR_DBL,
  PRIM_FR_MUL,
  PRIM_FR_SQR,
  PRIM_FR_TO_MONT,
  PRIM_FR_FROM_MONT,
  PRIM_FR_INV,
  PRIM_FP_ADD,
  PRIM_FP_SUB,
  PRIM_FP_NEG,
  PRIM_FP_DBL,
  PRIM_FP_MUL,
  PRIM_FP_SQR,
  PRIM_FP_TO_MONT,
  PRIM_FP_FROM_MONT,
  PRIM_FP_INV,
  // curve.hpp
  PRIM_PT_DBL_AFFINE,
  PRIM_PT_DBL,
  PRIM_PT_ADD_AFFINE_CLASSIC,
  PRIM_PT_ADD_AFFINE_NWAY,
  PRIM_PT_ADD,
  PRIM_PT_NEG,
  PRIM_PT_TO_AFFINE,
  PRIM_PT_TO_AFFINE_UNIFORM,
  PRIM_COUNT
};

// words per tuple: ni elements of unit iu in, no elements of unit ou (+ xo
// words) out; units: 0 = Fp29 limbs (L), 1 = Fp words (N), 2 = Fr words, 3 = one word
struct PrimShape {
  int iu, ni, ou, no, xo;
};
constexpr PrimShape prim_shape(int op) {
  switch (op) {
    case PRIM_MUL: case PRIM_MUL_LAT: case PRIM_MUL_CHAIN: case PRIM_ADD: case PRIM_SUB_P2: case PRIM_SUB_P4:
    case PRIM_SUB_P6: case PRIM_SUB_P8: case PRIM_SUB_P10: case PRIM_SUB_P16: case PRIM_ADD_2X_LAZY:
      return {0, 2, 0, 1, 0};
    case PRIM_MUL2: case PRIM_MUL2_LAT: case PRIM_MUL2_CHAIN:
      return {0, 4, 0, 1, 0};
    case PRIM_MUL_X2:
      return {0, 4, 0, 2, 0};
    case PRIM_SQR_X2: case PRIM_SQR_X2_PAIR:
      return {0, 2, 0, 2, 0};
    case PRIM_MUL_X3:
      return {0, 6, 0, 3, 0};
    case PRIM_MUL2_MUL:
      return {0, 6, 0, 2, 0};
    case PRIM_MUL2_X3:
      return {0, 8, 0, 3, 0};
    case PRIM_IS_ZERO_LT2M: case PRIM_IS_ZERO:
      return {0, 1, 3, 1, 0};
    case PRIM_FROM_WORDS:
      return {1, 1, 0, 1, 0};
    case PRIM_TO_WORDS:
      return {0, 1, 1, 1, 0};
    case PRIM_FR_ADD: case PRIM_FR_SUB: case PRIM_FR_MUL:
      return {2, 2, 2, 1, 0};
    case PRIM_FR_NEG: case PRIM_FR_DBL: case PRIM_FR_SQR: case PRIM_FR_TO_MONT: case PRIM_FR_FROM_MONT:
    case PRIM_FR_INV:
      return {2, 1, 2, 1, 0};
    case PRIM_FP_ADD: case PRIM_FP_SUB: case PRIM_FP_MUL:
      return {1, 2, 1, 1, 0};
    case PRIM_FP_NEG: case PRIM_FP_DBL: case PRIM_FP_SQR: case PRIM_FP_TO_MONT: case PRIM_FP_FROM_MONT:
    case PRIM_FP_INV:
      return {1, 1, 1, 1, 0};
    case PRIM_PT_DBL_AFFINE:
      return {0, 2, 0, 4, 0};
    case PRIM_PT_DBL: case PRIM_PT_NEG:
      return {0, 4, 0, 4, 0};
    case PRIM_PT_ADD_AFFINE_CLASSIC: case PRIM_PT_ADD_AFFINE_NWAY:
      return {0, 6, 0, 4, 0};
    case PRIM_PT_ADD:
      return {0, 8, 0, 4, 0};
    case PRIM_PT_TO_AFFINE: case PRIM_PT_TO_AFFINE_UNIFORM:
      return {0, 4, 0, 2, 1};
    default:  // one Fp29 element in, one out
      return {0, 1, 0, 1, 0};
  }
}
constexpr bool prim_uniform(int op) {
  return op == PRIM_INV_UNIFORM || op == PRIM_INV_UNIFORM_RAW || op == PRIM_PT_TO_AFFINE_UNIFORM;
}
template <class C>
constexpr int prim_unit(int u) {
  return u == 0 ? C::Fp29::L : u == 1 ? C::Fp::N : u == 2 ? C::Fr::N : 1;
}
template <class C>
constexpr int prim_in_words(int op) {
  return prim_shape(op).ni * prim_unit<C>(prim_shape(op).iu);
}
template <class C>
constexpr int prim_out_words(int op) {
  return prim_shape(op).no * prim_unit<C>(prim_shape(op).ou) + prim_shape(op).xo;
}

// the nine field.hpp operations, OP relative to the field's first id
template <class FP, int OP>
KZGX_DEV void prim_fe(const uint32_t* p, uint32_t* o) {
  constexpr int N = FP::N;
  Fe<FP> a, b, r;
#pragma unroll
  for (int i = 0; i < N; i++) a.v[i] = p[i];
  if constexpr (OP == 0 || OP == 1 || OP == 4) {
#pragma unroll
    for (int i = 0; i < N; i++) b.v[i] = p[N + i];
  }
  if constexpr (OP == 0) r = fe_add<FP>(a, b);
  else if constexpr (OP == 1) r = fe_sub<FP>(a, b);
  else if constexpr (OP == 2) r = fe_neg<FP>(a);
  else if constexpr (OP == 3) r = fe_dbl<FP>(a);
  else if constexpr (OP == 4) r = fe_mul<FP>(a, b);
  else if constexpr (OP == 5) r = fe_sqr<FP>(a);
  else if constexpr (OP == 6) r = fe_to_mont<FP>(a);
  else if constexpr (OP == 7) r = fe_from_mont<FP>(a);
  else r = fe_inv<FP>(a);
#pragma unroll
  for (int i = 0; i < N; i++) o[i] = r.v[i];
}

// lanes that make a wave-uniform call in `mode`
KZGX_DEV uint32_t prim_lanes(int mode) { return mode == 0 ? 64u : mode == 1 ? 4u : 1u; }

template <class C, int OP>
__global__ __launch_bounds__(64) void k_prim(const uint32_t* __restrict__ in, uint32_t count, int mode,
                                             uint32_t* __restrict__ out) {
  using F = typename C::Fp29;
  constexpr int L = F::L, N = C::Fp::N;
  const uint32_t t = prim_uniform(OP) ? blockIdx.x : blockIdx.x * 64 + threadIdx.x;
  if (t >= count) return;
  const uint32_t* p = in + (size_t)t * prim_in_words<C>(OP);
  uint32_t* o = out + (size_t)t * prim_out_words<C>(OP);
  auto A = [&](int k) { return f29_load<F>(p + k * L); };
  auto W = [&](int k, const F29<F>& x) { f29_store<F>(o + k * L, x); };
  auto PT = [&](int k) {  // raw XYZZ limbs: X, Y, ZZ, ZZZ from element k on
    Xyzz<C> r;
    r.X = A(k), r.Y = A(k + 1), r.ZZ = A(k + 2), r.ZZZ = A(k + 3);
    return r;
  };
  auto AF = [&](int k) {
    Affine<C> r;
    r.x = A(k), r.y = A(k + 1);
    return r;
  };
  auto WPT = [&](const Xyzz<C>& r) { W(0, r.X), W(1, r.Y), W(2, r.ZZ), W(3, r.ZZZ); };
  F29<F> r0, r1, r2;
  if constexpr (OP == PRIM_MUL) W(0, f29_mul<F>(A(0), A(1)));
  else if constexpr (OP == PRIM_MUL_LAT) W(0, f29_mul_lat<F>(A(0), A(1)));
  else if constexpr (OP == PRIM_MUL_CHAIN) W(0, f29_mul_chain<F>(A(0), A(1)));
  else if constexpr (OP == PRIM_SQR) W(0, f29_sqr<F>(A(0)));
  else if constexpr (OP == PRIM_SQR_CHAIN) W(0, f29_sqr_chain<F>(A(0)));
  else if constexpr (OP == PRIM_MUL2) W(0, f29_mul2<F>(A(0), A(1), A(2), A(3)));
  else if constexpr (OP == PRIM_MUL2_LAT) W(0, f29_mul2_lat<F>(A(0), A(1), A(2), A(3)));
  else if constexpr (OP == PRIM_MUL2_CHAIN) W(0, f29_mul2_chain<F>(A(0), A(1), A(2), A(3)));
  else if constexpr (OP == PRIM_MUL_X2) {
    f29_mul_x2<F>(A(0), A(1), A(2), A(3), r0, r1);
    W(0, r0), W(1, r1);
  } else if constexpr (OP == PRIM_SQR_X2) {
    f29_sqr_x2<F>(A(0), A(1), r0, r1);
    W(0, r0), W(1, r1);
  } else if constexpr (OP == PRIM_SQR_X2_PAIR) {
    f29_sqr_x2_pair<F>(A(0), A(1), r0, r1);
    W(0, r0), W(1, r1);
  } else if constexpr (OP == PRIM_MUL_X3) {
    f29_mul_x3<F>(A(0), A(1), A(2), A(3), A(4), A(5), r0, r1, r2);
    W(0, r0), W(1, r1), W(2, r2);
  } else if constexpr (OP == PRIM_MUL2_MUL) {
    f29_mul2_mul<F>(A(0), A(1), A(2), A(3), A(4), A(5), r0, r1);
    W(0, r0), W(1, r1);
  } else if constexpr (OP == PRIM_MUL2_X3) {
    f29_mul2_x3<F>(A(0), A(1), A(2), A(3), A(4), A(5), A(6), A(7), r0, r1, r2);
    W(0, r0), W(1, r1), W(2, r2);
  } else if constexpr (OP == PRIM_ADD) W(0, f29_add<F>(A(0), A(1)));
  else if constexpr (OP == PRIM_SUB_P2) W(0, f29_sub<F>(A(0), A(1), F::P2));
  else if constexpr (OP == PRIM_SUB_P4) W(0, f29_sub<F>(A(0), A(1), F::P4));
  else if constexpr (OP == PRIM_SUB_P6) W(0, f29_sub<F>(A(0), A(1), F::P6));
  else if constexpr (OP == PRIM_SUB_P8) W(0, f29_sub<F>(A(0), A(1), F::P8));
  else if constexpr (OP == PRIM_SUB_P10) W(0, f29_sub<F>(A(0), A(1), F::P10));
  else if constexpr (OP == PRIM_SUB_P16) W(0, f29_sub<F>(A(0), A(1), F::P16));
  else if constexpr (OP == PRIM_NEG_LAZY) W(0, f29_neg_lazy<F>(A(0)));
  else if constexpr (OP == PRIM_NEG8_LAZY) W(0, f29_neg8_lazy<F>(A(0)));
  else if constexpr (OP == PRIM_ADD_2X_LAZY) W(0, f29_add_2x_lazy<F>(A(0), A(1)));
  else if constexpr (OP == PRIM_NORMALIZE) W(0, f29_normalize<F>(A(0)));
  else if constexpr (OP == PRIM_CSUB_P) W(0, f29_csub<F>(A(0), F::P));
  else if constexpr (OP == PRIM_CSUB_P2) W(0, f29_csub<F>(A(0), F::P2));
  else if constexpr (OP == PRIM_CSUB_P4) W(0, f29_csub<F>(A(0), F::P4));
  else if constexpr (OP == PRIM_CSUB_P6) W(0, f29_csub<F>(A(0), F::P6));
  else if constexpr (OP == PRIM_CSUB_P8) W(0, f29_csub<F>(A(0), F::P8));
  else if constexpr (OP == PRIM_CSUB_P10) W(0, f29_csub<F>(A(0), F::P10));
  else if constexpr (OP == PRIM_CSUB_P16) W(0, f29_csub<F>(A(0), F::P16));
  else if constexpr (OP == PRIM_REDUCE) W(0, f29_reduce<F>(A(0)));
  else if constexpr (OP == PRIM_IS_ZERO_LT2M) o[0] = f29_is_zero_lt2m<F>(A(0)) ? 1u : 0u;
  else if constexpr (OP == PRIM_IS_ZERO) o[0] = f29_is_zero<F>(A(0)) ? 1u : 0u;
  else if constexpr (OP == PRIM_TO_MONT) W(0, f29_to_mont<F>(A(0)));
  else if constexpr (OP == PRIM_FROM_MONT) W(0, f29_from_mont<F>(A(0)));
  else if constexpr (OP == PRIM_FROM_WORDS) {
    uint32_t w[N];
#pragma unroll
    for (int i = 0; i < N; i++) w[i] = p[i];
    W(0, f29_from_words<F, N>(w));
  } else if constexpr (OP == PRIM_TO_WORDS) {
    uint32_t w[N];
    f29_to_words<F, N>(A(0), w);
#pragma unroll
    for (int i = 0; i < N; i++) o[i] = w[i];
  } else if constexpr (OP == PRIM_INV) W(0, f29_inv<F, N>(A(0), C::Fp::PM2));
  else if constexpr (OP == PRIM_INV_VT) W(0, f29_inv_vt<F, N>(A(0), C::Fp::P));
  else if constexpr (OP == PRIM_INV_UNIFORM || OP == PRIM_INV_UNIFORM_RAW) {
    const F29<F> a = A(0);
    if (threadIdx.x < prim_lanes(mode)) {
      if constexpr (OP == PRIM_INV_UNIFORM) r0 = f29_inv_uniform<F, N>(a, C::Fp::P);
      else r0 = f29_inv_uniform_raw<F, N>(a, C::Fp::P);
      if (threadIdx.x == 0) W(0, r0);
    }
  } else if constexpr (OP >= PRIM_FR_ADD && OP <= PRIM_FR_INV) prim_fe<typename C::Fr, OP - PRIM_FR_ADD>(p, o);
  else if constexpr (OP >= PRIM_FP_ADD && OP <= PRIM_FP_INV) prim_fe<typename C::Fp, OP - PRIM_FP_ADD>(p, o);
  else if constexpr (OP == PRIM_PT_DBL_AFFINE) WPT(xyzz_dbl_affine_impl<C>(AF(0)));
  else if constexpr (OP == PRIM_PT_DBL) WPT(xyzz_dbl_impl<C>(PT(0)));
  else if constexpr (OP == PRIM_PT_ADD_AFFINE_CLASSIC) WPT(xyzz_add_affine_classic<C>(PT(0), AF(4)));
  else if constexpr (OP == PRIM_PT_ADD_AFFINE_NWAY) WPT(xyzz_add_affine_nway<C>(PT(0), AF(4)));
  else if constexpr (OP == PRIM_PT_ADD) WPT(xyzz_add_impl<C>(PT(0), PT(4)));
  else if constexpr (OP == PRIM_PT_NEG) WPT(xyzz_neg<C>(PT(0)));
  else if constexpr (OP == PRIM_PT_TO_AFFINE) {
    Affine<C> a;
    const bool fin = xyzz_to_affine_impl<C, false>(PT(0), a);
    W(0, a.x), W(1, a.y);
    o[2 * L] = fin ? 1u : 0u;
  } else {
    static_assert(OP == PRIM_PT_TO_AFFINE_UNIFORM, "unhandled primitive");
    const Xyzz<C> q = PT(0);
    if (threadIdx.x < prim_lanes(mode)) {
      Affine<C> a;
      const bool fin = xyzz_to_affine_impl<C, true>(q, a);
      if (threadIdx.x == 0) {
        W(0, a.x), W(1, a.y);
        o[2 * L] = fin ? 1u : 0u;
      }
    }
  }
}

template <class C, int OP>
static void prim_launch(const uint32_t* d_in, uint32_t count, int mode, uint32_t* d_out, hipStream_t st) {
  const uint32_t blocks = prim_uniform(OP) ? count : (count + 63) / 64;
  hipLaunchKernelGGL((k_prim<C, OP>), dim3(blocks), dim3(64), 0, st, d_in, count, mode, d_out);
}

template <class C, int... OPS>
static void prim_dispatch(std::integer_sequence<int, OPS...>, int op, const uint32_t* d_in, uint32_t count, int mode,
                          uint32_t* d_out, hipStream_t st) {
  ((op == OPS ? prim_launch<C, OPS>(d_in, count, mode, d_out, st) : (void)0), ...);
}

// the most tuples of one call (the staging buffers stay a few MB)
constexpr size_t PRIM_MAX_COUNT = 1u << 16;

// one primitive on `count` tuples of raw limbs at host pointer `in`, results
// to host pointer `out` (kzgx_debug_prim, kzgx_api.hip)
int prim_selftest(int curve, int op, int mode, const uint32_t* in, size_t count, uint32_t* out, hipStream_t st) {
  if (!in || !out || op < 0 || op >= PRIM_COUNT || count == 0 || count > PRIM_MAX_COUNT) return KZGX_ERR_ARG;
  if (mode < 0 || mode > 2 || (mode != 0 && !prim_uniform(op))) return KZGX_ERR_ARG;
  if (curve != KZGX_CURVE_BN254 && curve != KZGX_CURVE_BLS12381) return KZGX_ERR_ARG;
  const bool bn = curve == KZGX_CURVE_BN254;
  const size_t in_b = count * (size_t)(bn ? prim_in_words<BN254G1>(op) : prim_in_words<BLS12381G1>(op)) * 4;
  const size_t out_b = count * (size_t)(bn ? prim_out_words<BN254G1>(op) : prim_out_words<BLS12381G1>(op)) * 4;
  uint32_t *d_in = nullptr, *d_out = nullptr;
  KZGX_TRY_HIP(hipMalloc((void**)&d_in, in_b));
  hipError_t e = hipMalloc((void**)&d_out, out_b);
  if (e == hipSuccess) e = hipMemcpyAsync(d_in, in, in_b, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(d_out, 0, out_b, st);
  if (e == hipSuccess) {
    constexpr auto ops = std::make_integer_sequence<int, PRIM_COUNT>{};
    if (bn) prim_dispatch<BN254G1>(ops, op, d_in, (uint32_t)count, mode, d_out, st);
    else prim_dispatch<BLS12381G1>(ops, op, d_in, (uint32_t)count, mode, d_out, st);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, out_b, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(d_in);
  (void)hipFree(d_out);
  return e == hipSuccess ? KZGX_OK : hip_fail(e);
}

}  // namespace kzgx
