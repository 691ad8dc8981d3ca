// C++ facade test of the all-domain openings (include/kzg.h):
// trusted_setup::create_all_proofs and create_all_proofs_from_evaluations on
// BLS12-381 with a fixed tau against create_proofs_from_evaluations over the
// domain, every proof through verify_proofs, then the refusals, BN254's
// included.  Run by tests/test_gpu_cpp_all_proofs.py; a non-zero exit status
// or a FAILED line is a failure.
//
// usage: test_all_proofs <tau hex>
#include <kzg.h>

#include <cstdlib>
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

int main(int argc, char** argv) {
  if (argc < 2) {
    std::cerr << "usage: test_all_proofs <tau hex>" << std::endl;
    return 2;
  }
  kzg::init(KZGX_CURVE_BLS12381);
  const kzg::Fr tau = fr_from_hex(argv[1]);
  kzg::trusted_setup kzg(300, tau);
  const unsigned k = 6;
  const size_t n = (size_t)1 << k;

  // a full-degree polynomial on the 64-point domain, and one of degree 40
  std::vector<kzg::Fr> c0, c1;
  for (long i = 0; i < 64; i++) c0.push_back(kzg::Fr(i * i * i + 5 * i - 11));
  for (long i = 0; i <= 40; i++) c1.push_back(kzg::Fr(-1000003 * i - 1));
  const kzg::poly p(c0), p1(c1);
  check_test(p.degree() == 63 && p1.degree() == 40, "degrees");

  const std::vector<kzg::Fr> dom = kzg::poly({kzg::Fr(0), kzg::Fr(1)}).evaluate_domain(k);
  const std::vector<kzg::Fr> ev = p.evaluate_domain(k), ev_br = p.evaluate_domain(k, true), ev1 = p1.evaluate_domain(k);

  std::vector<kzg::proof> want = kzg.create_proofs_from_evaluations(ev, dom);
  std::vector<kzg::proof> all = kzg.create_all_proofs(p, k);
  check_test(all.size() == n, "one proof per domain point");
  check_test(same_points(all, want), "create_all_proofs == create_proofs_from_evaluations over the domain");
  check_test(same_points(kzg.create_all_proofs_from_evaluations(ev), want), "the same from the values");
  std::vector<kzg::proof> all_br = kzg.create_all_proofs(p, k, true);
  bool perm_ok = all_br.size() == n;
  for (size_t i = 0; perm_ok && i < n; i++) perm_ok = all_br[bitrev(i, k)].get_curve_point() == all[i].get_curve_point();
  check_test(perm_ok, "bit-reversed order is the permutation of the natural one");
  check_test(same_points(kzg.create_all_proofs_from_evaluations(ev_br, true), all_br), "bit-reversed values in, bit-reversed proofs out");
  check_test(same_points(kzg.create_all_proofs(p1, k), kzg.create_proofs_from_evaluations(ev1, dom)),
             "a degree-40 polynomial on the 64-point domain");

  // every proof verifies against the commitment, and a wrong value does not
  std::vector<kzg::commit> cs = kzg.create_commits_from_evaluations({ev});
  std::vector<kzg::commit> commits(n, cs[0]);
  std::vector<kzg::proof> proofs = all;
  std::vector<std::pair<kzg::Fr, kzg::Fr>> pts;
  for (size_t i = 0; i < n; i++) pts.push_back({dom[i], ev[i]});
  std::vector<bool> ok = kzg.verify_proofs(commits, proofs, pts);
  bool all_ok = ok.size() == n;
  for (size_t i = 0; all_ok && i < n; i++) all_ok = ok[i];
  check_test(all_ok, "every proof verifies");
  pts[7].second = ev[8];
  ok = kzg.verify_proofs(commits, proofs, pts);
  check_test(!ok[7] && ok[6] && ok[8], "a wrong value does not verify");

  // a constant: every quotient is zero
  std::vector<kzg::proof> cst = kzg.create_all_proofs(kzg::poly({kzg::Fr(42)}), 3);
  bool cst_ok = cst.size() == 8;
  for (auto& q : cst) cst_ok = cst_ok && q.get_curve_point().inf;
  check_test(cst_ok, "a constant's proofs are all infinite");
  check_test(kzg.create_all_proofs(p1, 8).size() == 256, "the largest domain below size() = 300");

  // refusals
  check_test(throws_invalid([&] { kzg.create_all_proofs(p, 5); }), "64 coefficients on a 32-point domain");
  check_test(throws_invalid([&] { kzg.create_all_proofs(p, 9); }), "2^9 >= size() = 300");
  check_test(throws_invalid([&] { kzg.create_all_proofs(p, 22); }), "no 2^23 domain for 2^22 points");
  check_test(throws_invalid([&] { kzg.create_all_proofs_from_evaluations(std::vector<kzg::Fr>(12)); }), "12 values: not a power of two");
  check_test(throws_invalid([&] { kzg.create_all_proofs_from_evaluations(std::vector<kzg::Fr>(512)); }), "2^9 values >= size()");

  // BN254: r - 1 = 4 * odd, so the size-2n domain exists for n <= 2 only
  kzg::init();
  kzg::trusted_setup bn(16);
  const kzg::poly q4({kzg::Fr(1), kzg::Fr(2), kzg::Fr(3), kzg::Fr(4)}), q2({kzg::Fr(5), kzg::Fr(6)});
  check_test(throws_invalid([&] { bn.create_all_proofs(q4, 2); }), "BN254: four points refused");
  check_test(throws_invalid([&] { bn.create_all_proofs_from_evaluations(std::vector<kzg::Fr>(4)); }), "BN254: four values refused");
  std::vector<kzg::proof> two = bn.create_all_proofs(q2, 1);
  std::vector<kzg::proof> two_want = bn.create_proofs(q2, {1, -1});
  check_test(same_points(two, two_want), "BN254: two points work");

  if (failures) {
    std::cout << failures << " TESTS FAILED" << std::endl;
    return 1;
  }
  std::cout << "ALL TESTS PASSED" << std::endl;
  return 0;
}
