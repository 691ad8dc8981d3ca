// C++ facade test of the per-cell verdicts (include/kzg.h):
// trusted_setup::verify_coset_proofs_each on BLS12-381 with a fixed tau.  The
// cells are made as in test_verify_cells.cpp (create_coset_proofs(_from_evaluations)
// and poly::evaluate_domain).  The expected vector is known from how each batch
// was tampered with: an honest batch is all true, a changed value, a wrong index
// or exchanged proofs make exactly the touched cells false, and two errors that
// cancel in no way still show as two.  Then the checked overload, an empty
// batch, the std::invalid_argument cases and BN254.  Run by
// tests/test_gpu_cpp_verify_cells_each.py; a non-zero exit status or a FAILED
// line is a failure.
//
// usage: test_verify_cells_each <tau hex>
#include <kzg.h>

#include <cstdlib>
#include <iostream>
#include <set>
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

// got has `size` verdicts, false exactly at the positions of `bad`
static bool false_exactly_at(const std::vector<bool>& got, size_t size, const std::set<size_t>& bad) {
  if (got.size() != size) return false;
  for (size_t k = 0; k < size; k++)
    if (got[k] != (bad.count(k) == 0)) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::cerr << "usage: test_verify_cells_each <tau hex>" << std::endl;
    return 2;
  }
  kzg::init(KZGX_CURVE_BLS12381);
  const kzg::Fr tau = fr_from_hex(argv[1]);
  kzg::trusted_setup kzg(300, tau);
  const unsigned k = 6, kl = 3;
  const size_t l = (size_t)1 << kl, R = (size_t)1 << (k - kl + 1), M = 2 * R;

  std::vector<kzg::Fr> c0, c1;
  for (long i = 0; i < 64; i++) c0.push_back(kzg::Fr(i * i * i + 5 * i - 11));
  for (long i = 0; i <= 40; i++) c1.push_back(kzg::Fr(-1000003 * i - 1));
  const kzg::poly P[2] = {kzg::poly(c0), kzg::poly(c1)};
  std::vector<kzg::commit> commits = {kzg.create_commit(P[0]), kzg.create_commit(P[1])};

  // every cell of both polynomials in the data-availability layout
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
  check_test(false_exactly_at(kzg.verify_coset_proofs_each(commits, ci, idx, proofs, vals, k, true, true), M, {}),
             "32 honest cells: all true (cell order)");

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
    check_test(false_exactly_at(kzg.verify_coset_proofs_each(commits, nci, nidx, np, nv, k, true), R, {}),
               "natural order: all true");
    std::swap(nv[5][0], nv[5][1]);
    check_test(false_exactly_at(kzg.verify_coset_proofs_each(commits, nci, nidx, np, nv, k, true), R, {5}),
               "natural order: two swapped values make cell 5 false");
  }

  // tamperings: exactly the touched cells are false
  {
    cells v = vals;
    v[19][4] = kzg::Fr(12345);
    check_test(false_exactly_at(kzg.verify_coset_proofs_each(commits, ci, idx, proofs, v, k, true, true), M, {19}),
               "a changed value: cell 19 only");
    v[0][0] = kzg::Fr(1);
    v[M - 1][l - 1] = kzg::Fr(2);
    check_test(false_exactly_at(kzg.verify_coset_proofs_each(commits, ci, idx, proofs, v, k, true, true), M,
                                {0, 19, M - 1}),
               "three changed values: the first, a middle and the last cell");
    std::vector<uint32_t> i2 = idx;
    i2[7] = 8;
    check_test(false_exactly_at(kzg.verify_coset_proofs_each(commits, ci, i2, proofs, vals, k, true, true), M, {7}),
               "a wrong cell index: cell 7 only");
    std::vector<uint32_t> c2 = ci;
    c2[30] = 0;
    check_test(false_exactly_at(kzg.verify_coset_proofs_each(commits, c2, idx, proofs, vals, k, true, true), M, {30}),
               "a wrong commit index: cell 30 only");
    std::vector<kzg::proof> p2 = proofs;
    std::swap(p2[2], p2[3]);
    check_test(false_exactly_at(kzg.verify_coset_proofs_each(commits, ci, idx, p2, vals, k, true, true), M, {2, 3}),
               "two exchanged proofs: cells 2 and 3");
    check_test(!kzg.verify_coset_proofs(commits, ci, idx, p2, vals, k, true, true),
               "the aggregate refuses the same batch");
  }

  // the checked overload
  check_test(false_exactly_at(kzg.verify_coset_proofs_each(commits, ci, idx, proofs, vals, k, true, true, true), M, {}),
             "checked, subgroup: all true");
  check_test(false_exactly_at(kzg.verify_coset_proofs_each(commits, ci, idx, proofs, vals, k, true, true, false), M, {}),
             "checked, curve only: all true");
  {
    cells v = vals;
    v[1][0] = kzg::Fr(1);
    kzg::G1 off = proofs[11].get_curve_point();
    off.y[0] ^= 1;  // not on the curve
    std::vector<kzg::proof> p2 = proofs;
    p2[11] = kzg::proof(off);
    check_test(false_exactly_at(kzg.verify_coset_proofs_each(commits, ci, idx, p2, v, k, true, true, true), M, {1, 11}) &&
                   false_exactly_at(kzg.verify_coset_proofs_each(commits, ci, idx, p2, v, k, true, true, false), M, {1, 11}),
               "checked: a changed value and an off-curve proof, each its own cell");
    kzg::G1 offc = commits[1].get_curve_point();
    offc.y[0] ^= 1;
    std::vector<kzg::commit> cm2 = {commits[0], kzg::commit(offc)};
    std::set<size_t> second;
    for (size_t q = R; q < M; q++) second.insert(q);
    check_test(false_exactly_at(kzg.verify_coset_proofs_each(cm2, ci, idx, proofs, vals, k, true, true, true), M, second),
               "checked: an off-curve commitment zeroes the cells that name it");
  }

  // the empty batch, and a subset with one commitment never named
  {
    std::vector<uint32_t> e;
    std::vector<kzg::proof> ep;
    cells ev;
    check_test(kzg.verify_coset_proofs_each(commits, e, e, ep, ev, k, true, true).empty(), "an empty batch: no verdicts");
    check_test(kzg.verify_coset_proofs_each(commits, e, e, ep, ev, k, true, true, true).empty(),
               "an empty batch, checked: no verdicts");
    std::vector<uint32_t> sc = {1, 1, 1}, si = {4, 9, 4};
    std::vector<kzg::proof> sp = {proofs[R + 4], proofs[R + 9], proofs[R + 5]};
    cells sv = {vals[R + 4], vals[R + 9], vals[R + 4]};
    check_test(false_exactly_at(kzg.verify_coset_proofs_each(commits, sc, si, sp, sv, k, true, true), 3, {2}),
               "three cells, one twice with another cell's proof");
  }

  // refusals
  {
    std::vector<uint32_t> shortc(ci.begin(), ci.end() - 1);
    check_test(throws_invalid([&] { kzg.verify_coset_proofs_each(commits, shortc, idx, proofs, vals, k, true, true); }),
               "mismatched sizes");
    cells v = vals;
    v[3].pop_back();
    check_test(throws_invalid([&] { kzg.verify_coset_proofs_each(commits, ci, idx, proofs, v, k, true, true); }),
               "cells of different sizes");
    cells v6(vals.size(), std::vector<kzg::Fr>(6));
    check_test(throws_invalid([&] { kzg.verify_coset_proofs_each(commits, ci, idx, proofs, v6, k, true, true); }),
               "6 values: not a power of two");
    std::vector<uint32_t> c2 = ci, i2 = idx;
    c2[1] = 2;
    i2[1] = (uint32_t)R;
    check_test(throws_invalid([&] { kzg.verify_coset_proofs_each(commits, c2, idx, proofs, vals, k, true, true); }),
               "a commit index out of range");
    check_test(throws_invalid([&] { kzg.verify_coset_proofs_each(commits, ci, i2, proofs, vals, k, true, true, true); }),
               "a cell index out of range (checked)");
    check_test(throws_invalid([&] { kzg.verify_coset_proofs_each(commits, ci, idx, proofs, vals, 2, true, true); }),
               "a coset larger than the domain");
    check_test(throws_invalid([&] { kzg.verify_coset_proofs_each(commits, ci, idx, proofs, vals, 22, true, true); }),
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
    check_test(false_exactly_at(bn.verify_coset_proofs_each(bc, bci, bidx, bp, bv, 2), 2, {}), "BN254: two cosets verify");
    std::swap(bv[1][0], bv[1][1]);
    check_test(false_exactly_at(bn.verify_coset_proofs_each(bc, bci, bidx, bp, bv, 2), 2, {1}),
               "BN254: swapped values make cell 1 false");
    check_test(throws_invalid([&] { bn.verify_coset_proofs_each(bc, bci, bidx, bp, bv, 3); }),
               "BN254: the 8-point domain refused");
  }

  if (failures) {
    std::cout << failures << " TESTS FAILED" << std::endl;
    return 1;
  }
  std::cout << "ALL TESTS PASSED" << std::endl;
  return 0;
}
