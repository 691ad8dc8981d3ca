// C++ facade test of the batch openings (include/kzg.h):
// trusted_setup::create_batch_proofs and trusted_setup::verify_batch_proofs on a
// degree-40 setup with a fixed tau.  Polynomials, points and gammas are small
// integers, so the folded polynomial F_g = sum gamma^j P_j and every value are
// computed here in plain integer arithmetic.  Run by
// tests/test_gpu_cpp_multi_open.py; a non-zero exit status or a FAILED line is a
// failure.
//
// usage: test_batch_open <curve 0|1> <tau hex>
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

using ipoly = std::vector<long>;

static long eval(const ipoly& P, long x) {
  long acc = 0;
  for (size_t i = P.size(); i-- > 0;) acc = acc * x + P[i];
  return acc;
}

static kzg::poly to_poly(const ipoly& P) {
  std::vector<kzg::Fr> f;
  for (long v : P) f.push_back(kzg::Fr(v));
  return kzg::poly(f);
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::cerr << "usage: test_batch_open <curve> <tau hex>" << std::endl;
    return 2;
  }
  kzg::init(atoi(argv[1]));
  const kzg::Fr tau = fr_from_hex(argv[2]);
  kzg::trusted_setup kzg(41, tau);

  // five polynomials of different lengths (zero-padded by the facade), one of them constant
  const std::vector<ipoly> ip = {{3, -1, 4, 1, -5, 9}, {2, 7, -1, 8}, {-2, 8, 1, -8, 2, 8, -4}, {5}, {0, 0, 1}};
  std::vector<kzg::poly> polys;
  for (auto& P : ip) polys.push_back(to_poly(P));
  std::vector<kzg::commit> commits = kzg.create_commits(polys);
  // three groups: four polynomials at z = 3 (one of them twice), two at z = -2, the constant alone at 4
  std::vector<kzg::batch_opening> groups = {{kzg::Fr(3), {0, 1, 2, 0, 4}}, {kzg::Fr(-2), {2, 1}}, {kzg::Fr(4), {3}}};
  const std::vector<long> zs = {3, -2, 4}, gam = {2, -3, 5};
  std::vector<kzg::Fr> gammas;
  for (long g : gam) gammas.push_back(kzg::Fr(g));

  std::vector<std::vector<kzg::Fr>> values;
  std::vector<kzg::proof> proofs = kzg.create_batch_proofs(polys, groups, gammas, &values);
  check_test(proofs.size() == 3 && values.size() == 3, "one proof and one value list per group");
  {
    bool right = values.size() == 3;
    for (size_t g = 0; right && g < 3; g++) {
      right = values[g].size() == groups[g].polys.size();
      for (size_t j = 0; right && j < values[g].size(); j++)
        right = values[g][j] == kzg::Fr(eval(ip[groups[g].polys[j]], zs[g]));
    }
    check_test(right, "values are the polynomials' own evaluations");
  }
  // proof g = the single opening of F_g = sum_j gamma^j P_j at z_g; its commitment = the same
  // combination of the commitments
  for (size_t g = 0; g < 3; g++) {
    ipoly F(8, 0);
    std::vector<kzg::G1> cs;
    std::vector<kzg::Fr> ws;
    long w = 1;
    for (uint32_t j : groups[g].polys) {
      for (size_t i = 0; i < ip[j].size(); i++) F[i] += w * ip[j][i];
      cs.push_back(commits[j].get_curve_point());
      ws.push_back(kzg::Fr(w));
      w *= gam[g];
    }
    kzg::poly pf = to_poly(F);
    std::vector<kzg::proof> single = kzg.create_proofs(pf, {zs[g]});
    check_test(single.size() == 1 && single[0].get_curve_point() == proofs[g].get_curve_point(),
               "proof " + std::to_string(g) + " is the opening of the folded polynomial");
    check_test(kzg.linear_combination(cs, ws) == kzg.create_commit(pf).get_curve_point(),
               "folded commitment " + std::to_string(g));
  }
  check_test(!proofs[0].get_curve_point().inf && !proofs[1].get_curve_point().inf, "proofs are finite");
  check_test(proofs[2].get_curve_point().inf, "a constant's proof is infinity");
  check_test(kzg.create_batch_proofs(polys, groups, gammas).size() == 3, "values_out is optional");

  check_test(kzg.verify_batch_proofs(commits, groups, gammas, values, proofs), "honest batch verifies");
  check_test(kzg.verify_batch_proofs(commits, groups, gammas, values, proofs, true), "honest batch verifies, checked");
  check_test(kzg.verify_batch_proofs(commits, groups, gammas, values, proofs, false),
             "honest batch verifies, curve check only");
  {
    auto bad = values;
    bad[0][3] = kzg::Fr(eval(ip[0], zs[0]) + 1);
    check_test(!kzg.verify_batch_proofs(commits, groups, gammas, bad, proofs), "one wrong value is refuted");
    check_test(!kzg.verify_batch_proofs(commits, groups, gammas, bad, proofs, true), "one wrong value is refuted, checked");
    auto swapped = proofs;
    std::swap(swapped[0], swapped[1]);
    check_test(!kzg.verify_batch_proofs(commits, groups, gammas, values, swapped), "swapped proofs are refuted");
    auto other = gammas;
    other[1] = kzg::Fr(7);
    check_test(!kzg.verify_batch_proofs(commits, groups, other, values, proofs), "another gamma is refuted");
    auto wrong_c = commits;
    wrong_c[1] = commits[2];
    check_test(!kzg.verify_batch_proofs(wrong_c, groups, gammas, values, proofs), "a wrong commitment is refuted");
  }
  {
    std::vector<kzg::batch_opening> none;
    std::vector<kzg::Fr> no_g;
    std::vector<std::vector<kzg::Fr>> no_v;
    std::vector<kzg::proof> no_p;
    check_test(kzg.create_batch_proofs(polys, none, no_g).empty(), "no groups: no proofs");
    check_test(kzg.verify_batch_proofs(commits, none, no_g, no_v, no_p), "no groups: true");
    // an empty group among others: its proof is infinity and the batch still verifies
    auto with_empty = groups;
    with_empty.insert(with_empty.begin() + 1, kzg::batch_opening{kzg::Fr(9), {}});
    auto g4 = gammas;
    g4.insert(g4.begin() + 1, kzg::Fr(11));
    std::vector<std::vector<kzg::Fr>> v4;
    std::vector<kzg::proof> p4 = kzg.create_batch_proofs(polys, with_empty, g4, &v4);
    check_test(p4.size() == 4 && p4[1].get_curve_point().inf && v4[1].empty() &&
                   p4[2].get_curve_point() == proofs[1].get_curve_point(),
               "an empty group gives infinity and moves nothing");
    check_test(kzg.verify_batch_proofs(commits, with_empty, g4, v4, p4, true), "batch with an empty group verifies");
  }

  // argument errors throw std::invalid_argument, as the neighbouring extensions do
  {
    auto fewer = gammas;
    fewer.pop_back();
    check_test(throws([&] { kzg.create_batch_proofs(polys, groups, fewer); }), "create: one gamma per group");
    check_test(throws([&] { kzg.verify_batch_proofs(commits, groups, fewer, values, proofs); }),
               "verify: one gamma per group");
    auto beyond = groups;
    beyond[1].polys.push_back(5);
    check_test(throws([&] { kzg.create_batch_proofs(polys, beyond, gammas); }), "create: index out of range");
    auto fewer_p = proofs;
    fewer_p.pop_back();
    check_test(throws([&] { kzg.verify_batch_proofs(commits, groups, gammas, values, fewer_p); }),
               "verify: one proof per group");
    auto fewer_v = values;
    fewer_v[0].pop_back();
    check_test(throws([&] { kzg.verify_batch_proofs(commits, groups, gammas, fewer_v, proofs); }),
               "verify: one value per opened commitment");
    std::vector<kzg::Fr> longp(43, kzg::Fr(1));
    std::vector<kzg::poly> too_long = {kzg::poly(longp)};
    std::vector<kzg::batch_opening> one = {{kzg::Fr(1), {0}}};
    check_test(throws([&] { kzg.create_batch_proofs(too_long, one, {kzg::Fr(2)}); }), "create: degree beyond the setup");
  }
  std::cout << (failures ? "SOME TESTS FAILED" : "ALL TESTS PASSED") << std::endl;
  return failures ? 1 : 0;
}
