// C++ facade test of the aggregation extensions (include/kzg.h):
// trusted_setup::verify_proofs_aggregated and trusted_setup::linear_combination
// on a degree-40 setup with a fixed tau.  Run by tests/test_gpu_cpp_aggregate.py;
// a non-zero exit status or a FAILED line is a failure.
//
// usage: test_verify_aggregated <curve 0|1> <tau hex>
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

static kzg::Fr fr_from_hex(const std::string& h) {
  std::string s = h.rfind("0x", 0) == 0 ? h.substr(2) : h;
  std::vector<uint8_t> le;
  for (int i = (int)s.size(); i > 0; i -= 2) {
    std::string byte = s.substr(i >= 2 ? i - 2 : 0, i >= 2 ? 2 : 1);
    le.push_back((uint8_t)strtol(byte.c_str(), nullptr, 16));
  }
  return kzg::Fr::from_le_bytes(le.data(), le.size());
}

template <class F>
static bool throws(F f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::cerr << "usage: test_verify_aggregated <curve> <tau hex>" << std::endl;
    return 2;
  }
  kzg::init(atoi(argv[1]));
  const kzg::Fr tau = fr_from_hex(argv[2]);
  kzg::trusted_setup kzg(41, tau);

  // 16 honest openings of two polynomials: P(i) = (signed char) text[i]
  const std::string text1 = "aggregated openings, one check";
  const std::string text2 = "A second blob of other bytes!";
  kzg::poly p1 = kzg::poly::from_blob(kzg::blob::from_string(text1));
  kzg::poly p2 = kzg::poly::from_blob(kzg::blob::from_string(text2));
  kzg::commit c1 = kzg.create_commit(p1), c2 = kzg.create_commit(p2);
  std::vector<long> at;
  for (long i = 0; i < 8; i++) at.push_back(2 * i + 1);
  std::vector<kzg::proof> pr1 = kzg.create_proofs(p1, at), pr2 = kzg.create_proofs(p2, at);
  std::vector<kzg::commit> commits;
  std::vector<kzg::proof> proofs;
  std::vector<std::pair<kzg::Fr, kzg::Fr>> points;
  for (size_t k = 0; k < at.size(); k++) {
    commits.push_back(c1);
    proofs.push_back(pr1[k]);
    points.push_back({kzg::Fr(at[k]), kzg::Fr((long)(signed char)text1[at[k]])});
    commits.push_back(c2);
    proofs.push_back(pr2[k]);
    points.push_back({kzg::Fr(at[k]), kzg::Fr((long)(signed char)text2[at[k]])});
  }
  check_test(commits.size() == 16, "16 openings");
  check_test(kzg.verify_proofs_aggregated(commits, proofs, points), "aggregated verify of honest openings");
  {
    std::vector<bool> each = kzg.verify_proofs(commits, proofs, points);
    bool all = true;
    for (bool b : each) all = all && b;
    check_test(all, "verify_proofs agrees on honest openings");
  }
  const size_t bad = 11;
  auto tampered = points;
  tampered[bad].second = kzg::Fr((long)(signed char)text2[at[bad / 2]] + 1);
  check_test(!kzg.verify_proofs_aggregated(commits, proofs, tampered), "aggregated verify refutes one flipped y");
  {
    std::vector<bool> each = kzg.verify_proofs(commits, proofs, tampered);
    bool named = each.size() == 16;
    for (size_t k = 0; named && k < each.size(); k++) named = each[k] == (k != bad);
    check_test(named, "verify_proofs names the flipped opening");
  }
  {
    std::vector<kzg::commit> none_c;
    std::vector<kzg::proof> none_p;
    std::vector<std::pair<kzg::Fr, kzg::Fr>> none_x;
    check_test(kzg.verify_proofs_aggregated(none_c, none_p, none_x), "empty batch is true");
  }

  // linear combination of commitments = commitment of the combined polynomial
  const long a = 3, b = 5;
  std::vector<long> q1 = {1, -2, 3, 0, 7}, q2 = {4, 5, -6};
  std::vector<kzg::Fr> f1, f2, comb;
  for (long v : q1) f1.push_back(kzg::Fr(v));
  for (long v : q2) f2.push_back(kzg::Fr(v));
  for (size_t i = 0; i < q1.size(); i++) comb.push_back(kzg::Fr(a * q1[i] + b * (i < q2.size() ? q2[i] : 0)));
  kzg::commit d1 = kzg.create_commit(kzg::poly(f1)), d2 = kzg.create_commit(kzg::poly(f2));
  kzg::commit dc = kzg.create_commit(kzg::poly(comb));
  kzg::G1 lc = kzg.linear_combination({d1.get_curve_point(), d2.get_curve_point()}, {kzg::Fr(a), kzg::Fr(b)});
  check_test(lc == dc.get_curve_point(), "linear_combination of commitments");
  check_test(!lc.inf, "linear_combination is finite");
  kzg::G1 zero = kzg.linear_combination({d1.get_curve_point(), d1.get_curve_point()}, {kzg::Fr(a), kzg::Fr(-a)});
  check_test(zero.inf, "a P - a P is infinity");
  check_test(kzg.linear_combination({}, {}).inf, "empty combination is infinity");

  // mismatched sizes throw, as verify_proofs does
  check_test(throws([&] { kzg.linear_combination({d1.get_curve_point()}, {kzg::Fr(a), kzg::Fr(b)}); }),
             "linear_combination size mismatch");
  {
    auto fewer = points;
    fewer.pop_back();
    check_test(throws([&] { kzg.verify_proofs_aggregated(commits, proofs, fewer); }),
               "verify_proofs_aggregated size mismatch (points)");
    auto fewer_p = proofs;
    fewer_p.pop_back();
    check_test(throws([&] { kzg.verify_proofs_aggregated(commits, fewer_p, points); }),
               "verify_proofs_aggregated size mismatch (proofs)");
  }
  std::cout << (failures ? "SOME TESTS FAILED" : "ALL TESTS PASSED") << std::endl;
  return failures ? 1 : 0;
}
