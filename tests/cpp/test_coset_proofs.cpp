// C++ facade test of the coset (cell) openings (include/kzg.h):
// trusted_setup::create_coset_proofs and create_coset_proofs_from_evaluations
// on BLS12-381 with a fixed tau against ground truth from the C ABI on a
// context of its own with the same tau -- every proof against kzgx_prove_range
// over kzgx_coset_points, two cells through kzgx_verify_proof -- then the
// refusals, BN254's included.  Run by tests/test_gpu_cpp_coset_proofs.py; a
// non-zero exit status or a FAILED line is a failure.
//
// usage: test_coset_proofs <tau hex>
#include <kzg.h>

#include <cstdlib>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

static int failures = 0;

static void check_test(bool status, const std::string& name) {
  std::cout << (status ? "PASSED" : "FAILED") << " [" << name << "]" << std::endl;
  if (!status) failures++;
}

template <class F>
static bool throws_invalid(F f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  } catch (...) {
  }
  return false;
}

static kzg::Fr fr_from_hex(const std::string& h) {
  std::string s = h.rfind("0x", 0) == 0 ? h.substr(2) : h;
  std::vector<uint8_t> le;
  for (int i = (int)s.size(); i > 0; i -= 2) {
    std::string byte = s.substr(i >= 2 ? i - 2 : 0, i >= 2 ? 2 : 1);
    le.push_back((uint8_t)strtol(byte.c_str(), nullptr, 16));
  }
  return kzg::Fr::from_le_bytes(le.data(), le.size());
}

static size_t bitrev(size_t i, unsigned bits) {
  size_t r = 0;
  for (unsigned b = 0; b < bits; b++) r |= ((i >> b) & 1) << (bits - 1 - b);
  return r;
}

static bool same_points(std::vector<kzg::proof> a, std::vector<kzg::proof> b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++)
    if (!(a[i].get_curve_point() == b[i].get_curve_point())) return false;
  return true;
}

// canonical limbs of a facade point, as the C ABI takes them (6 + 6 on BLS12-381)
static std::vector<uint64_t> limbs(const kzg::G1& g) {
  std::vector<uint64_t> w(12);
  std::memcpy(&w[0], g.x.data(), 48);
  std::memcpy(&w[6], g.y.data(), 48);
  return w;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::cerr << "usage: test_coset_proofs <tau hex>" << std::endl;
    return 2;
  }
  kzg::init(KZGX_CURVE_BLS12381);
  const kzg::Fr tau = fr_from_hex(argv[1]);
  kzg::trusted_setup kzg(300, tau);
  const unsigned k = 6, kl = 3;
  const size_t n = (size_t)1 << k, l = (size_t)1 << kl;

  // the C ABI's own context on the same tau: 300 G1 points, l + 1 G2 points
  kzgx_ctx* c = nullptr;
  bool abi = kzgx_create(&c, KZGX_CURVE_BLS12381, 0) == KZGX_OK && kzgx_set_default_table(c, 0, 0) == KZGX_OK &&
             kzgx_gen_srs_g1(c, tau.v.data(), 0, 300) == KZGX_OK && kzgx_gen_srs_g2(c, tau.v.data(), 0, l + 1) == KZGX_OK;
  check_test(abi, "a C ABI context on the same tau");
  if (!abi) return 1;

  // a full-degree polynomial on the 64-point domain, and one of degree 40
  std::vector<kzg::Fr> c0, c1;
  for (long i = 0; i < 64; i++) c0.push_back(kzg::Fr(i * i * i + 5 * i - 11));
  for (long i = 0; i <= 40; i++) c1.push_back(kzg::Fr(-1000003 * i - 1));
  const kzg::poly p(c0), p1(c1);
  std::vector<uint64_t> coef(4 * n, 0), coef1(4 * n, 0);
  for (size_t i = 0; i < c0.size(); i++) std::memcpy(&coef[4 * i], c0[i].v.data(), 32);
  for (size_t i = 0; i < c1.size(); i++) std::memcpy(&coef1[4 * i], c1[i].v.data(), 32);
  const std::vector<kzg::Fr> ev = p.evaluate_domain(k), ev_br = p.evaluate_domain(k, true);

  // every facade proof against kzgx_prove_range over the coset's points
  auto against_range = [&](std::vector<kzg::proof> got, const std::vector<uint64_t>& cf, int flags) {
    const size_t R = (size_t)1 << (k - kl + ((flags & KZGX_PROVE_COSETS_EXTENDED) ? 1 : 0));
    if (got.size() != R) return false;
    std::vector<uint64_t> xs(4 * l), ref(12);
    for (size_t i = 0; i < R; i++) {
      int inf = 0;
      if (kzgx_coset_points(KZGX_CURVE_BLS12381, k, kl, flags, i, xs.data()) != KZGX_OK) return false;
      if (kzgx_prove_range(c, cf.data(), n, xs.data(), l, ref.data(), &inf) != KZGX_OK) return false;
      const kzg::G1& g = got[i].get_curve_point();
      if (g.inf != (inf != 0) || (!g.inf && limbs(g) != ref)) return false;
    }
    return true;
  };
  std::vector<kzg::proof> nat = kzg.create_coset_proofs(p, k, kl);
  std::vector<kzg::proof> ext = kzg.create_coset_proofs(p, k, kl, true);
  std::vector<kzg::proof> ext_br = kzg.create_coset_proofs(p, k, kl, true, true);
  check_test(nat.size() == 8 && ext.size() == 16, "n / l cosets, 2 n / l extended");
  check_test(against_range(nat, coef, 0), "create_coset_proofs == kzgx_prove_range per coset");
  check_test(against_range(ext, coef, KZGX_PROVE_COSETS_EXTENDED), "the same on the twice larger domain");
  check_test(against_range(ext_br, coef, KZGX_PROVE_COSETS_EXTENDED | KZGX_NTT_BITREV), "the same in cell order");
  bool perm_ok = ext_br.size() == 16;
  for (size_t i = 0; perm_ok && i < 16; i++) perm_ok = ext_br[bitrev(i, 4)].get_curve_point() == ext[i].get_curve_point();
  check_test(perm_ok, "bit-reversed order is the permutation of the natural one");
  bool even_ok = true;  // coset 2 i of the extended domain is coset i of the domain itself
  for (size_t i = 0; i < 8; i++) even_ok = even_ok && ext[2 * i].get_curve_point() == nat[i].get_curve_point();
  check_test(even_ok, "the extended domain's even cosets are the domain's own");
  check_test(same_points(kzg.create_coset_proofs_from_evaluations(ev, kl, true), ext), "the same from the values");
  check_test(same_points(kzg.create_coset_proofs_from_evaluations(ev_br, kl, true, true), ext_br),
             "bit-reversed values in, cell order out");
  check_test(against_range(kzg.create_coset_proofs(p1, k, kl, true), coef1, KZGX_PROVE_COSETS_EXTENDED),
             "a degree-40 polynomial on the 64-point domain");
  check_test(same_points(kzg.create_coset_proofs(p, k, 0), kzg.create_all_proofs(p, k)),
             "cosets of one point are the all-domain openings");

  // two cells through kzgx_verify_proof against the facade's commitment; a swapped pair of values fails
  kzg::commit cm = kzg.create_commit(p);
  const std::vector<uint64_t> cw = limbs(cm.get_curve_point());
  bool ver_ok = true, bad_ok = true;
  for (size_t cell : {(size_t)3, (size_t)14}) {
    std::vector<uint64_t> xs(4 * l), ys(4 * l);
    const int flags = KZGX_PROVE_COSETS_EXTENDED | KZGX_NTT_BITREV;
    int ok = 0;
    ver_ok = ver_ok && kzgx_coset_points(KZGX_CURVE_BLS12381, k, kl, flags, cell, xs.data()) == KZGX_OK &&
             kzgx_poly_eval(c, coef.data(), n, xs.data(), l, ys.data()) == KZGX_OK;
    const kzg::G1& g = ext_br[cell].get_curve_point();
    const std::vector<uint64_t> pw = limbs(g);
    ver_ok = ver_ok && kzgx_verify_proof(c, cw.data(), 0, pw.data(), g.inf, xs.data(), ys.data(), l, &ok) == KZGX_OK &&
             ok == 1;
    for (int w = 0; w < 4; w++) std::swap(ys[4 * 1 + w], ys[4 * 6 + w]);
    ok = 1;
    bad_ok = bad_ok && kzgx_verify_proof(c, cw.data(), 0, pw.data(), g.inf, xs.data(), ys.data(), l, &ok) == KZGX_OK &&
             ok == 0;
  }
  check_test(ver_ok, "two cells verify");
  check_test(bad_ok, "two swapped values do not");

  // no quotient: a polynomial of degree < l, and one coset that is the whole domain
  std::vector<kzg::proof> low = kzg.create_coset_proofs(kzg::poly({kzg::Fr(42), kzg::Fr(7)}), k, kl, true);
  bool low_ok = low.size() == 16;
  for (auto& q : low) low_ok = low_ok && q.get_curve_point().inf;
  check_test(low_ok, "degree below the coset size: every proof is infinite");
  std::vector<kzg::proof> whole = kzg.create_coset_proofs(p, k, k, true);
  check_test(whole.size() == 2 && whole[0].get_curve_point().inf && whole[1].get_curve_point().inf,
             "l = n: two infinite proofs on the extended domain");
  check_test(kzg.create_coset_proofs(p1, 8, 6, true).size() == 8, "the largest domain below size() = 300");

  // refusals
  check_test(throws_invalid([&] { kzg.create_coset_proofs(p, 5, 3); }), "64 coefficients on a 32-point domain");
  check_test(throws_invalid([&] { kzg.create_coset_proofs(p, 9, 3); }), "2^9 >= size() = 300");
  check_test(throws_invalid([&] { kzg.create_coset_proofs(p, k, k + 1); }), "a coset larger than the domain");
  check_test(throws_invalid([&] { kzg.create_coset_proofs(p, 22, 0); }), "no 2^23 domain for the 2^22-point products");
  check_test(throws_invalid([&] { kzg.create_coset_proofs(p, 22, 6, true); }), "no 2^23 domain to open on");
  check_test(throws_invalid([&] { kzg.create_coset_proofs_from_evaluations(std::vector<kzg::Fr>(12), 1); }),
             "12 values: not a power of two");
  check_test(throws_invalid([&] { kzg.create_coset_proofs_from_evaluations(std::vector<kzg::Fr>(512), 3); }),
             "2^9 values >= size()");
  kzgx_destroy(c);

  // BN254: r - 1 = 4 * odd, domains of at most 4 points
  kzg::init();
  kzg::trusted_setup bn(16);
  const kzg::poly q4({kzg::Fr(1), kzg::Fr(2), kzg::Fr(3), kzg::Fr(4)}), q2({kzg::Fr(5), kzg::Fr(6)});
  check_test(throws_invalid([&] { bn.create_coset_proofs(q4, 2, 0); }), "BN254: four single-point cosets refused");
  check_test(throws_invalid([&] { bn.create_coset_proofs(q4, 2, 1, true); }), "BN254: the 8-point domain refused");
  check_test(bn.create_coset_proofs(q4, 2, 1).size() == 2, "BN254: two cosets of two points work");
  check_test(same_points(bn.create_coset_proofs(q2, 1, 0), bn.create_all_proofs(q2, 1)), "BN254: two points work");

  if (failures) {
    std::cout << failures << " TESTS FAILED" << std::endl;
    return 1;
  }
  std::cout << "ALL TESTS PASSED" << std::endl;
  return 0;
}
