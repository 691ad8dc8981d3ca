// C++ facade test of the Shplonk openings (include/kzg.h):
// trusted_setup::create_shplonk_proof and trusted_setup::verify_shplonk_proof on a
// degree-40 setup with a fixed tau.  Polynomials, points, gamma and z are small
// integers, so h = sum_s F_s div Z_s (exact integer division by the monic Z_s), the
// values and G = sum zeta_s w_k P_k - Z_T(z) h are computed here in plain integer
// arithmetic and committed through the facade's older entries.  Run by
// tests/test_gpu_cpp_shplonk.py; a non-zero exit status or a FAILED line is a
// failure.
//
// usage: test_shplonk <curve 0|1> <tau hex>
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

template <class E, class F>
static bool throws(F f) {
  try {
    f();
  } catch (const E&) {
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

// F div Z for monic Z, into q (added)
static void add_floor_div(ipoly F, const ipoly& Z, ipoly& q) {
  const size_t d = Z.size() - 1;
  for (size_t i = F.size(); i-- > d;) {
    const long c = F[i];
    q[i - d] += c;
    for (size_t j = 0; j <= d; j++) F[i - d + j] -= c * Z[j];
  }
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::cerr << "usage: test_shplonk <curve> <tau hex>" << std::endl;
    return 2;
  }
  kzg::init(atoi(argv[1]));
  const kzg::Fr tau = fr_from_hex(argv[2]);
  kzg::trusted_setup kzg(41, tau);

  // five polynomials of different lengths (zero-padded by the facade), one of them constant
  const std::vector<ipoly> ip = {{3, -1, 4, 1, -5, 9}, {2, 7, -1, 8}, {-2, 8, 1, -8, 2, 8, -4}, {5}, {0, 0, 1}};
  const size_t N = 7;
  std::vector<kzg::poly> polys;
  for (auto& P : ip) polys.push_back(to_poly(P));
  std::vector<kzg::commit> commits = kzg.create_commits(polys);
  // T: the value 2 at the indices 0 and 3.  Sets: three polynomials at {2}; two at {2, -1}; two at
  // {-1, 3, 2} (through index 3); none at {3}
  const std::vector<long> T = {2, -1, 3, 2};
  std::vector<kzg::Fr> points;
  for (long t : T) points.push_back(kzg::Fr(t));
  const std::vector<kzg::shplonk_set> sets = {{{0}, {0, 1, 3}}, {{0, 1}, {2, 0}}, {{1, 2, 3}, {4, 2}}, {{2}, {}}};
  const long gam = 2, zl = 5;
  const kzg::Fr gamma(gam), z(zl);

  int calls = 0;
  kzg::G1 seen;
  std::vector<std::vector<kzg::Fr>> values;
  kzg::shplonk_proof pr = kzg.create_shplonk_proof(
      polys, points, sets, gamma,
      [&](const kzg::proof& W) {
        calls++;
        kzg::proof w = W;  // get_curve_point is not const
        seen = w.get_curve_point();
        return z;
      },
      &values);
  check_test(calls == 1 && seen == pr.W.get_curve_point(), "the challenge is asked once, with W");
  {
    bool right = values.size() == sets.size();
    for (size_t s = 0; right && s < sets.size(); s++) {
      right = values[s].size() == sets[s].points.size() * sets[s].polys.size();
      for (size_t j = 0; right && j < sets[s].polys.size(); j++)
        for (size_t i = 0; right && i < sets[s].points.size(); i++)
          right = values[s][j * sets[s].points.size() + i] == kzg::Fr(eval(ip[sets[s].polys[j]], T[sets[s].points[i]]));
    }
    check_test(right, "values are the polynomials' own evaluations, claim by claim");
  }
  // the integer model: weights gamma^k over the global claim index
  ipoly h(N, 0), G(N, 0);
  long ZT = 1;
  for (long t : T) ZT *= zl - t;
  {
    long w = 1;
    for (auto& st : sets) {
      ipoly F(N, 0), Z = {1};
      long zeta = ZT;
      for (uint32_t i : st.points) {
        ipoly Z2(Z.size() + 1, 0);
        for (size_t a = 0; a < Z.size(); a++) {
          Z2[a + 1] += Z[a];
          Z2[a] -= Z[a] * T[i];
        }
        Z = Z2;
        zeta /= zl - T[i];
      }
      for (uint32_t j : st.polys) {
        for (size_t i = 0; i < ip[j].size(); i++) {
          F[i] += w * ip[j][i];
          G[i] += zeta * w * ip[j][i];
        }
        w *= gam;
      }
      add_floor_div(F, Z, h);
    }
    for (size_t i = 0; i < N; i++) G[i] -= ZT * h[i];
  }
  check_test(h[N - 1] == 0, "h has one coefficient less than the polynomials");
  check_test(kzg.create_commit(to_poly(h)).get_curve_point() == pr.W.get_curve_point(), "W commits to sum_s F_s div Z_s");
  {
    kzg::poly pg = to_poly(G);
    std::vector<kzg::proof> single = kzg.create_proofs(pg, {zl});
    check_test(single.size() == 1 && single[0].get_curve_point() == pr.Wp.get_curve_point(),
               "W' is the opening of G at z");
  }
  check_test(!pr.W.get_curve_point().inf && !pr.Wp.get_curve_point().inf, "both proof points are finite");
  {
    kzg::shplonk_proof again = kzg.create_shplonk_proof(polys, points, sets, gamma, [&](const kzg::proof&) { return z; });
    check_test(again.W.get_curve_point() == pr.W.get_curve_point() && again.Wp.get_curve_point() == pr.Wp.get_curve_point(),
               "values_out is optional; the proof is reproducible");
  }

  check_test(kzg.verify_shplonk_proof(commits, points, sets, gamma, values, z, pr), "honest proof verifies");
  check_test(kzg.verify_shplonk_proof(commits, points, sets, gamma, values, z, pr, true), "honest proof verifies, checked");
  check_test(kzg.verify_shplonk_proof(commits, points, sets, gamma, values, z, pr, false),
             "honest proof verifies, curve check only");
  {
    auto bad = values;
    bad[1][2] = kzg::Fr(eval(ip[0], T[0]) + 1);
    check_test(!kzg.verify_shplonk_proof(commits, points, sets, gamma, bad, z, pr), "one wrong value is refuted");
    check_test(!kzg.verify_shplonk_proof(commits, points, sets, gamma, bad, z, pr, true), "one wrong value is refuted, checked");
    kzg::shplonk_proof swapped{pr.Wp, pr.W};
    check_test(!kzg.verify_shplonk_proof(commits, points, sets, gamma, values, z, swapped), "swapped proof points are refuted");
    check_test(!kzg.verify_shplonk_proof(commits, points, sets, kzg::Fr(3), values, z, pr), "another gamma is refuted");
    check_test(!kzg.verify_shplonk_proof(commits, points, sets, gamma, values, kzg::Fr(6), pr), "another z is refuted");
    auto wrong_c = commits;
    wrong_c[1] = commits[2];
    check_test(!kzg.verify_shplonk_proof(wrong_c, points, sets, gamma, values, z, pr), "a wrong commitment is refuted");
    auto moved = sets;
    moved[1].points = {0, 2};  // set 1 now claims its values at {2, 3}
    check_test(!kzg.verify_shplonk_proof(commits, points, moved, gamma, values, z, pr), "another point set is refuted");
  }

  // argument errors throw std::invalid_argument, as the neighbouring extensions do
  {
    using inv = std::invalid_argument;
    auto chal = [&](const kzg::proof&) { return z; };
    auto beyond = sets;
    beyond[1].polys.push_back(5);
    check_test(throws<inv>([&] { kzg.create_shplonk_proof(polys, points, beyond, gamma, chal); }), "create: index out of range");
    check_test(throws<inv>([&] { kzg.verify_shplonk_proof(commits, points, beyond, gamma, values, z, pr); }),
               "verify: index out of range");
    auto far = sets;
    far[0].points = {4};
    check_test(throws<inv>([&] { kzg.create_shplonk_proof(polys, points, far, gamma, chal); }), "create: point index out of range");
    auto twice = sets;
    twice[1].points = {1, 1};
    check_test(throws<inv>([&] { kzg.create_shplonk_proof(polys, points, twice, gamma, chal); }), "create: an index twice in one set");
    auto empty = sets;
    empty[3].points.clear();
    check_test(throws<inv>([&] { kzg.create_shplonk_proof(polys, points, empty, gamma, chal); }), "create: a set without points");
    std::vector<kzg::shplonk_set> none;
    check_test(throws<inv>([&] { kzg.create_shplonk_proof(polys, points, none, gamma, chal); }), "create: no sets");
    auto fewer_v = values;
    fewer_v[0].pop_back();
    check_test(throws<inv>([&] { kzg.verify_shplonk_proof(commits, points, sets, gamma, fewer_v, z, pr); }),
               "verify: one value per opened commitment and point");
    std::vector<kzg::Fr> longp(43, kzg::Fr(1));
    std::vector<kzg::poly> too_long = {kzg::poly(longp)};
    std::vector<kzg::shplonk_set> one = {{{0}, {0}}};
    check_test(throws<inv>([&] { kzg.create_shplonk_proof(too_long, points, one, gamma, chal); }),
               "create: degree beyond the setup");
    // the same value at two indices of one set: no interpolant (std::domain_error, as create_proofs on repeated points)
    auto equal = sets;
    equal[1].points = {0, 3};
    check_test(throws<std::domain_error>([&] { kzg.create_shplonk_proof(polys, points, equal, gamma, chal); }),
               "create: equal values in one set");
    check_test(throws<std::domain_error>([&] { kzg.verify_shplonk_proof(commits, points, equal, gamma, values, z, pr); }),
               "verify: equal values in one set");
  }
  std::cout << (failures ? "SOME TESTS FAILED" : "ALL TESTS PASSED") << std::endl;
  return failures ? 1 : 0;
}
