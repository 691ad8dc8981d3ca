// C++ facade test of the evaluation-form extensions (include/kzg.h):
// kzg::domain_root, poly::from_evaluations, poly::evaluate_domain,
// trusted_setup::create_commits_from_evaluations and
// trusted_setup::create_proofs_from_evaluations on BLS12-381 with a fixed tau,
// then the BN254 refusals.  Run by tests/test_gpu_cpp_evals.py; a non-zero
// exit status or a FAILED line is a failure.
//
// usage: test_evals <tau hex>
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

int main(int argc, char** argv) {
  if (argc < 2) {
    std::cerr << "usage: test_evals <tau hex>" << std::endl;
    return 2;
  }
  kzg::init(KZGX_CURVE_BLS12381);
  const kzg::Fr tau = fr_from_hex(argv[1]);
  kzg::trusted_setup kzg(300, tau);
  const unsigned k = 8;
  const size_t n = (size_t)1 << k;

  check_test(kzg::domain_root(0) == kzg::Fr(1) && kzg::domain_root(1) == kzg::Fr(-1), "domain_root(0) = 1, domain_root(1) = -1");
  check_test(throws_invalid([] { kzg::domain_root(33); }), "domain_root(33) throws");

  // a degree-200 polynomial and two companions
  std::vector<kzg::Fr> c0, c1, c2;
  for (long i = 0; i <= 200; i++) {
    c0.push_back(kzg::Fr(i * i + 3 * i - 7));
    c1.push_back(kzg::Fr(1000003 * i + 1));
  }
  for (long i = 0; i < 256; i++) c2.push_back(kzg::Fr(-i - 1));
  const kzg::poly p(c0), p1(c1), p2(c2);
  check_test(p.degree() == 200 && p2.degree() == 255, "degrees");

  const std::vector<kzg::Fr> ev = p.evaluate_domain(k), ev_br = p.evaluate_domain(k, true);
  check_test(ev.size() == n && ev_br.size() == n, "evaluate_domain size");
  bool perm_ok = true;
  for (size_t i = 0; i < n; i++) perm_ok = perm_ok && ev_br[bitrev(i, k)] == ev[i];
  check_test(perm_ok, "bit-reversed order is the permutation of the natural one");
  check_test(kzg::poly::from_evaluations(ev).get_poly() == p.get_poly(), "from_evaluations(evaluate_domain) == p");
  check_test(kzg::poly::from_evaluations(ev_br, true).get_poly() == p.get_poly(), "the same, bit-reversed");
  check_test(kzg::poly::from_evaluations(p2.evaluate_domain(k)).get_poly() == p2.get_poly(), "full-degree round trip");
  const std::vector<kzg::Fr> cst = kzg::poly({kzg::Fr(42)}).evaluate_domain(4);
  bool cst_ok = cst.size() == 16;
  for (auto& v : cst) cst_ok = cst_ok && v == kzg::Fr(42);
  check_test(cst_ok, "a constant evaluates to itself everywhere");
  check_test(kzg::poly::from_evaluations(cst).degree() == 0, "and interpolates back, normalized");
  check_test(kzg::poly::from_evaluations(std::vector<kzg::Fr>(8)).degree() == -1, "zero values: the zero polynomial");

  // commits
  const std::vector<std::vector<kzg::Fr>> evs = {ev, p1.evaluate_domain(k), p2.evaluate_domain(k)};
  const std::vector<std::vector<kzg::Fr>> evs_br = {ev_br, p1.evaluate_domain(k, true), p2.evaluate_domain(k, true)};
  std::vector<kzg::poly> interp;
  for (auto& e : evs) interp.push_back(kzg::poly::from_evaluations(e));
  std::vector<kzg::commit> want = kzg.create_commits(interp), direct = kzg.create_commits({p, p1, p2});
  std::vector<kzg::commit> got = kzg.create_commits_from_evaluations(evs);
  std::vector<kzg::commit> got_br = kzg.create_commits_from_evaluations(evs_br, true);
  bool commits_ok = got.size() == 3 && got_br.size() == 3;
  for (size_t i = 0; commits_ok && i < 3; i++)
    commits_ok = got[i].get_curve_point() == want[i].get_curve_point() &&
                 got[i].get_curve_point() == direct[i].get_curve_point() &&
                 got_br[i].get_curve_point() == want[i].get_curve_point() && !got[i].get_curve_point().inf;
  check_test(commits_ok, "create_commits_from_evaluations == create_commits of the interpolants");
  check_test(kzg.create_commits_from_evaluations({}).empty(), "no vectors, no commits");

  // openings: the domain point w^5, w^0 = 1, and w_9^3 (outside the size-2^8 domain:
  // its value comes from the twice larger domain)
  const std::vector<kzg::Fr> ev9 = p.evaluate_domain(k + 1), dom = kzg::poly({kzg::Fr(0), kzg::Fr(1)}).evaluate_domain(k),
                             dom9 = kzg::poly({kzg::Fr(0), kzg::Fr(1)}).evaluate_domain(k + 1);
  check_test(dom[1] == kzg::domain_root(k) && dom9[1] == kzg::domain_root(k + 1) && dom9[10] == dom[5],
             "X on the domain is the domain");
  const std::vector<kzg::Fr> zs = {dom[5], kzg::Fr(1), dom9[3]};
  const std::vector<std::pair<kzg::Fr, kzg::Fr>> pts = {{zs[0], ev[5]}, {zs[1], ev[0]}, {zs[2], ev9[3]}};
  std::vector<kzg::proof> proofs = kzg.create_proofs_from_evaluations(ev, zs);
  std::vector<kzg::proof> proofs_br = kzg.create_proofs_from_evaluations(ev_br, zs, true);
  std::vector<kzg::commit> cs(3, got[0]);
  std::vector<bool> ok = kzg.verify_proofs(cs, proofs, pts);
  check_test(ok.size() == 3 && ok[0] && ok[1] && ok[2], "create_proofs_from_evaluations verifies");
  bool same = proofs_br.size() == 3;
  for (size_t i = 0; same && i < 3; i++) same = proofs_br[i].get_curve_point() == proofs[i].get_curve_point();
  check_test(same, "the same proofs from bit-reversed values");
  std::vector<kzg::proof> by_coeff = kzg.create_proofs(p, {1});
  check_test(by_coeff[0].get_curve_point() == proofs[1].get_curve_point(), "== create_proofs at z = 1");
  std::vector<std::pair<kzg::Fr, kzg::Fr>> bad = pts;
  bad[0].second = ev[6];
  ok = kzg.verify_proofs(cs, proofs, bad);
  check_test(!ok[0] && ok[1] && ok[2], "a wrong value does not verify");
  check_test(kzg.create_proofs_from_evaluations(ev, {}).empty(), "no points, no proofs");

  // refusals
  check_test(throws_invalid([] { kzg::poly::from_evaluations(std::vector<kzg::Fr>(6)); }), "6 values: not a power of two");
  check_test(throws_invalid([] { kzg::poly::from_evaluations({}); }), "no values");
  check_test(throws_invalid([&] { p.evaluate_domain(7); }), "degree 200 on a 128-point domain");
  check_test(throws_invalid([&] { p.evaluate_domain(23); }), "2^23 exceeds the curve's domain");
  check_test(throws_invalid([&] { kzg.create_commits_from_evaluations({std::vector<kzg::Fr>(512)}); }),
             "2^9 >= size() = 300");
  check_test(throws_invalid([&] { kzg.create_commits_from_evaluations({ev, std::vector<kzg::Fr>(128)}); }),
             "vectors of different sizes");
  check_test(throws_invalid([&] { kzg.create_commits_from_evaluations({std::vector<kzg::Fr>(12)}); }),
             "commits of 12 values");
  check_test(throws_invalid([&] { kzg.create_proofs_from_evaluations(std::vector<kzg::Fr>(512), zs); }),
             "proofs with 2^9 >= size()");

  // BN254: r - 1 = 4 * odd, no domain beyond four points
  kzg::init();
  check_test(throws_invalid([] { kzg::poly::from_evaluations(std::vector<kzg::Fr>(8)); }), "BN254: 8 values throw");
  check_test(throws_invalid([] { kzg::domain_root(3); }), "BN254: domain_root(3) throws");
  const std::vector<kzg::Fr> four = {kzg::Fr(1), kzg::Fr(2), kzg::Fr(3), kzg::Fr(4)};
  check_test(kzg::poly::from_evaluations(kzg::poly(four).evaluate_domain(2)).get_poly() == four, "BN254: n = 4 works");

  if (failures) {
    std::cout << failures << " TESTS FAILED" << std::endl;
    return 1;
  }
  std::cout << "ALL TESTS PASSED" << std::endl;
  return 0;
}
