// C++ facade test of the aggregated cell verification (include/kzg.h):
// trusted_setup::verify_coset_proofs on BLS12-381 with a fixed tau.  The cells
// come from create_coset_proofs_from_evaluations / create_coset_proofs and
// poly::evaluate_domain (paths with tests of their own): every honest batch
// must verify, a changed value, a wrong index and a swapped proof must not;
// then the checked overload, the std::invalid_argument cases and BN254's
// refusals.  Run by tests/test_gpu_cpp_verify_cells.py; a non-zero exit status
// or a FAILED line is a failure.
//
// usage: test_verify_cells <tau hex>
#include <kzg.h>

#include <cstdlib>
#include <iostream>
#include <stdexcept>
#include <string>
#include <utility>
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

using cells = std::vector<std::vector<kzg::Fr>>;

int main(int argc, char** argv) {
  if (argc < 2) {
    std::cerr << "usage: test_verify_cells <tau hex>" << std::endl;
    return 2;
  }
  kzg::init(KZGX_CURVE_BLS12381);
  const kzg::Fr tau = fr_from_hex(argv[1]);
  kzg::trusted_setup kzg(300, tau);
  const unsigned k = 6, kl = 3;
  const size_t l = (size_t)1 << kl, R = (size_t)1 << (k - kl + 1), D = R * l;

  // a full-degree polynomial on the 64-point domain, and one of degree 40
  std::vector<kzg::Fr> c0, c1;
  for (long i = 0; i < 64; i++) c0.push_back(kzg::Fr(i * i * i + 5 * i - 11));
  for (long i = 0; i <= 40; i++) c1.push_back(kzg::Fr(-1000003 * i - 1));
  const kzg::poly P[2] = {kzg::poly(c0), kzg::poly(c1)};
  std::vector<kzg::commit> commits = {kzg.create_commit(P[0]), kzg.create_commit(P[1])};

  // every cell of both polynomials in the data-availability layout: proofs from the bit-reversed
  // values on the size-n domain, a cell's values = a chunk of the bit-reversed size-2n evaluations
  std::vector<kzg::proof> proofs;
  std::vector<uint32_t> ci, idx;
  cells vals;
  for (uint32_t b = 0; b < 2; b++) {
    const std::vector<kzg::proof> pr = kzg.create_coset_proofs_from_evaluations(P[b].evaluate_domain(k, true), kl, true, true);
    const std::vector<kzg::Fr> ev = P[b].evaluate_domain(k + 1, true);
    for (size_t p = 0; p < R; p++) {
      proofs.push_back(pr[p]);
      ci.push_back(b);
      idx.push_back((uint32_t)p);
      vals.push_back(std::vector<kzg::Fr>(ev.begin() + p * l, ev.begin() + (p + 1) * l));
    }
  }
  check_test(proofs.size() == 2 * R && vals.size() == 2 * R && D == 128, "32 cells of two polynomials");
  check_test(kzg.verify_coset_proofs(commits, ci, idx, proofs, vals, k, true, true), "every cell verifies (cell order)");

  // the natural order: coset i holds w^(i + R j)
  {
    std::vector<kzg::proof> np = kzg.create_coset_proofs(P[0], k, kl, true);
    const std::vector<kzg::Fr> ev = P[0].evaluate_domain(k + 1);
    std::vector<uint32_t> nci(R, 0), nidx;
    cells nv;
    for (size_t i = 0; i < R; i++) {
      nidx.push_back((uint32_t)i);
      std::vector<kzg::Fr> y;
      for (size_t j = 0; j < l; j++) y.push_back(ev[i + R * j]);
      nv.push_back(y);
    }
    check_test(kzg.verify_coset_proofs(commits, nci, nidx, np, nv, k, true), "every cell verifies (natural order)");
    std::swap(nv[5][0], nv[5][1]);
    check_test(!kzg.verify_coset_proofs(commits, nci, nidx, np, nv, k, true), "natural order: two swapped values fail");
  }
  // the domain itself (not extended): its cosets are the extended domain's even ones
  {
    std::vector<kzg::proof> np = kzg.create_coset_proofs(P[1], k, kl);
    const std::vector<kzg::Fr> ev = P[1].evaluate_domain(k);
    std::vector<uint32_t> nci(R / 2, 1), nidx;
    cells nv;
    for (size_t i = 0; i < R / 2; i++) {
      nidx.push_back((uint32_t)i);
      std::vector<kzg::Fr> y;
      for (size_t j = 0; j < l; j++) y.push_back(ev[i + (R / 2) * j]);
      nv.push_back(y);
    }
    check_test(kzg.verify_coset_proofs(commits, nci, nidx, np, nv, k), "the cosets of the size-n domain verify");
  }

  // one tampering at a time
  {
    cells v = vals;
    v[19][4] = kzg::Fr(12345);
    check_test(!kzg.verify_coset_proofs(commits, ci, idx, proofs, v, k, true, true), "a changed value fails");
    std::vector<uint32_t> i2 = idx;
    i2[7] = 8;
    check_test(!kzg.verify_coset_proofs(commits, ci, i2, proofs, vals, k, true, true), "a wrong cell index fails");
    std::vector<uint32_t> c2 = ci;
    c2[30] = 0;
    check_test(!kzg.verify_coset_proofs(commits, c2, idx, proofs, vals, k, true, true), "a wrong commit index fails");
    std::vector<kzg::proof> p2 = proofs;
    std::swap(p2[2], p2[3]);
    check_test(!kzg.verify_coset_proofs(commits, ci, idx, p2, vals, k, true, true), "two swapped proofs fail");
    check_test(!kzg.verify_coset_proofs(commits, ci, idx, proofs, vals, k, true, false),
               "cell-order input read in natural order fails");
  }

  // the checked overload
  check_test(kzg.verify_coset_proofs(commits, ci, idx, proofs, vals, k, true, true, true), "checked, subgroup: true");
  check_test(kzg.verify_coset_proofs(commits, ci, idx, proofs, vals, k, true, true, false), "checked, curve only: true");
  {
    cells v = vals;
    v[0][0] = kzg::Fr(1);
    check_test(!kzg.verify_coset_proofs(commits, ci, idx, proofs, v, k, true, true, true), "checked: a changed value fails");
    kzg::G1 off = proofs[11].get_curve_point();
    off.y[0] ^= 1;  // not on the curve
    std::vector<kzg::proof> p2 = proofs;
    p2[11] = kzg::proof(off);
    check_test(!kzg.verify_coset_proofs(commits, ci, idx, p2, vals, k, true, true, true) &&
                   !kzg.verify_coset_proofs(commits, ci, idx, p2, vals, k, true, true, false),
               "checked: an off-curve proof fails under both settings");
  }

  // the empty batch, and a subset with one commitment never named
  {
    std::vector<uint32_t> e;
    std::vector<kzg::proof> ep;
    cells ev;
    check_test(kzg.verify_coset_proofs(commits, e, e, ep, ev, k, true, true), "an empty batch is true");
    std::vector<uint32_t> sc = {1, 1, 1}, si = {4, 9, 4};
    std::vector<kzg::proof> sp = {proofs[R + 4], proofs[R + 9], proofs[R + 4]};
    cells sv = {vals[R + 4], vals[R + 9], vals[R + 4]};
    check_test(kzg.verify_coset_proofs(commits, sc, si, sp, sv, k, true, true), "three cells, one twice, one commitment unused");
  }

  // refusals
  {
    std::vector<uint32_t> shortc(ci.begin(), ci.end() - 1);
    check_test(throws_invalid([&] { kzg.verify_coset_proofs(commits, shortc, idx, proofs, vals, k, true, true); }),
               "mismatched sizes");
    cells v = vals;
    v[3].pop_back();
    check_test(throws_invalid([&] { kzg.verify_coset_proofs(commits, ci, idx, proofs, v, k, true, true); }),
               "cells of different sizes");
    cells v6(vals.size(), std::vector<kzg::Fr>(6));
    check_test(throws_invalid([&] { kzg.verify_coset_proofs(commits, ci, idx, proofs, v6, k, true, true); }),
               "6 values: not a power of two");
    std::vector<uint32_t> c2 = ci, i2 = idx;
    c2[1] = 2;
    i2[1] = (uint32_t)R;
    check_test(throws_invalid([&] { kzg.verify_coset_proofs(commits, c2, idx, proofs, vals, k, true, true); }),
               "a commit index out of range");
    check_test(throws_invalid([&] { kzg.verify_coset_proofs(commits, ci, i2, proofs, vals, k, true, true); }),
               "a cell index out of range");
    check_test(throws_invalid([&] { kzg.verify_coset_proofs(commits, ci, idx, proofs, vals, 2, true, true); }),
               "a coset larger than the domain");
    check_test(throws_invalid([&] { kzg.verify_coset_proofs(commits, ci, idx, proofs, vals, 22, true, true); }),
               "no 2^23 domain to open on");
  }

  // BN254: r - 1 = 4 * odd, domains of at most 4 points
  kzg::init();
  kzg::trusted_setup bn(16);
  const kzg::poly q4({kzg::Fr(1), kzg::Fr(2), kzg::Fr(3), kzg::Fr(4)});
  {
    std::vector<kzg::commit> bc = {bn.create_commit(q4)};
    std::vector<kzg::proof> bp = bn.create_coset_proofs(q4, 2, 1);
    const std::vector<kzg::Fr> ev = q4.evaluate_domain(2);
    std::vector<uint32_t> bci = {0, 0}, bidx = {0, 1};
    cells bv = {{ev[0], ev[2]}, {ev[1], ev[3]}};
    check_test(bn.verify_coset_proofs(bc, bci, bidx, bp, bv, 2), "BN254: two cosets of two points verify");
    std::swap(bv[1][0], bv[1][1]);
    check_test(!bn.verify_coset_proofs(bc, bci, bidx, bp, bv, 2), "BN254: swapped values fail");
    std::swap(bv[1][0], bv[1][1]);
    check_test(throws_invalid([&] { bn.verify_coset_proofs(bc, bci, bidx, bp, bv, 2, true); }),
               "BN254: the 8-point domain refused");
    check_test(throws_invalid([&] { bn.verify_coset_proofs(bc, bci, bidx, bp, bv, 3); }),
               "BN254: the 8-point domain refused (log2n = 3)");
  }

  if (failures) {
    std::cout << failures << " TESTS FAILED" << std::endl;
    return 1;
  }
  std::cout << "ALL TESTS PASSED" << std::endl;
  return 0;
}
