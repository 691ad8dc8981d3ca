// C++ facade test of cell recovery (include/kzg.h): trusted_setup::recover_cells
// and recover_cells_and_proofs on BLS12-381 with a fixed tau.  The cells of a
// polynomial come from the C ABI (kzgx_prove_cosets_batch on a context of its own
// with the same tau); the blob is recovered from half of them and compared with
// all of them and with create_coset_proofs; then the refusals.  Run by
// tests/test_gpu_cpp_recover_cells.py; a non-zero exit status or a FAILED line is
// a failure.
//
// usage: test_recover_cells <tau hex>
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

template <class E, class F>
static bool throws(F f) {
  try {
    f();
  } catch (const E&) {
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

static bool same_points(std::vector<kzg::proof> a, std::vector<kzg::proof> b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++)
    if (!(a[i].get_curve_point() == b[i].get_curve_point())) return false;
  return true;
}

static bool same_values(const std::vector<kzg::Fr>& a, const std::vector<uint64_t>& limbs) {
  if (4 * a.size() != limbs.size()) return false;
  for (size_t i = 0; i < a.size(); i++)
    if (std::memcmp(a[i].v.data(), &limbs[4 * i], 32) != 0) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::cerr << "usage: test_recover_cells <tau hex>" << std::endl;
    return 2;
  }
  kzg::init(KZGX_CURVE_BLS12381);
  const kzg::Fr tau = fr_from_hex(argv[1]);
  kzg::trusted_setup kzg(300, tau);
  const unsigned k = 6, kl = 3;
  const size_t n = (size_t)1 << k, l = (size_t)1 << kl, D = 2 * n, R = D / l;

  kzgx_ctx* c = nullptr;
  bool abi = kzgx_create(&c, KZGX_CURVE_BLS12381, 0) == KZGX_OK && kzgx_set_default_table(c, 0, 0) == KZGX_OK &&
             kzgx_gen_srs_g1(c, tau.v.data(), 0, 300) == KZGX_OK;
  check_test(abi, "a C ABI context on the same tau");
  if (!abi) return 1;

  std::vector<kzg::Fr> c0;
  for (long i = 0; i < 64; i++) c0.push_back(kzg::Fr(i * i * i + 5 * i - 11));
  const kzg::poly p(c0);
  std::vector<uint64_t> coef(4 * n, 0);
  for (size_t i = 0; i < c0.size(); i++) std::memcpy(&coef[4 * i], c0[i].v.data(), 32);

  for (int rev = 0; rev < 2; rev++) {
    const std::string tag = rev ? " (cell order)" : " (natural order)";
    const int flags = KZGX_PROVE_COSETS_EXTENDED | (rev ? KZGX_NTT_BITREV : 0);
    std::vector<uint64_t> xy(12 * R), y(4 * D);
    std::vector<int> inf(R);
    bool cells = kzgx_prove_cosets_batch(c, coef.data(), k, kl, 1, flags, xy.data(), inf.data(), y.data()) == KZGX_OK;
    check_test(cells, "the blob's cells from the C ABI" + tag);
    // half the cells, in a scrambled order: 5, 10, 15, 4, 9, 14, 3, 8
    std::vector<uint32_t> idx;
    std::vector<std::vector<kzg::Fr>> vals;
    auto add = [&](uint32_t i) {
      idx.push_back(i);
      std::vector<kzg::Fr> v(l);
      for (size_t j = 0; j < l; j++) std::memcpy(v[j].v.data(), &y[4 * (i * l + j)], 32);
      vals.push_back(v);
    };
    for (uint32_t t = 1; t <= R / 2; t++) add((5 * t) % R);
    check_test(same_values(kzg.recover_cells(idx, vals, k, rev != 0), y), "a blob from half its cells" + tag);
    auto both = kzg.recover_cells_and_proofs(idx, vals, k, rev != 0);
    check_test(same_values(both.first, y), "the same with the proofs" + tag);
    check_test(same_points(both.second, kzg.create_coset_proofs(p, k, kl, true, rev != 0)),
               "the recovered proofs == create_coset_proofs" + tag);
    // one cell more: still consistent; then one value off by one
    add(0);
    check_test(same_values(kzg.recover_cells(idx, vals, k, rev != 0), y), "nine cells" + tag);
    vals[2][1] = kzg::Fr(17);
    check_test(throws<std::domain_error>([&] { kzg.recover_cells(idx, vals, k, rev != 0); }),
               "nine cells with a changed value lie on no polynomial" + tag);
    check_test(throws<std::domain_error>([&] { kzg.recover_cells_and_proofs(idx, vals, k, rev != 0); }),
               "the same with the proofs" + tag);
    idx.pop_back();
    vals.pop_back();
    std::vector<kzg::Fr> got = kzg.recover_cells(idx, vals, k, rev != 0);  // eight cells: any values interpolate
    bool agree = got.size() == D && !same_values(got, y);
    for (size_t t = 0; agree && t < idx.size(); t++)
      for (size_t j = 0; j < l; j++) agree = agree && got[idx[t] * l + j].v == vals[t][j].v;
    check_test(agree, "eight cells with a changed value: another polynomial through them" + tag);
  }
  kzgx_destroy(c);

  // refusals
  std::vector<uint32_t> idx;
  std::vector<std::vector<kzg::Fr>> vals;
  for (uint32_t i = 0; i < R / 2; i++) {
    idx.push_back(i);
    vals.push_back(std::vector<kzg::Fr>(l, kzg::Fr(3)));
  }
  check_test(kzg.recover_cells(idx, vals, k).size() == D, "a constant blob");
  auto with = [&](auto change) {
    std::vector<uint32_t> i2 = idx;
    std::vector<std::vector<kzg::Fr>> v2 = vals;
    change(i2, v2);
    return throws<std::invalid_argument>([&] { kzg.recover_cells(i2, v2, k); });
  };
  using I = std::vector<uint32_t>;
  using V = std::vector<std::vector<kzg::Fr>>;
  check_test(with([&](I& i, V&) { i[3] = (uint32_t)R; }), "an index out of range");
  check_test(with([&](I& i, V&) { i[3] = i[4]; }), "a cell given twice");
  check_test(with([&](I& i, V& v) { i.pop_back(); v.pop_back(); }), "fewer than half the cells");
  check_test(with([&](I& i, V&) { i.pop_back(); }), "mismatched sizes");
  check_test(with([&](I&, V& v) { v[2].pop_back(); }), "cells of different sizes");
  check_test(with([&](I&, V& v) { for (auto& x : v) x.resize(6); }), "a cell size that is no power of two");
  check_test(with([&](I& i, V& v) { i.clear(); v.clear(); }), "no cells");
  check_test(throws<std::invalid_argument>([&] { kzg.recover_cells(idx, vals, 2); }), "a coset larger than the domain");
  check_test(throws<std::invalid_argument>([&] { kzg.recover_cells(idx, vals, 22); }), "no 2^23 domain");
  check_test(throws<std::invalid_argument>([&] { kzg.recover_cells(idx, vals, 16); }), "more than 4096 cells");
  check_test(throws<std::invalid_argument>([&] { kzg.recover_cells_and_proofs(idx, vals, 9); }), "2^9 >= size() = 300");

  if (failures) {
    std::cout << failures << " TESTS FAILED" << std::endl;
    return 1;
  }
  std::cout << "ALL TESTS PASSED" << std::endl;
  return 0;
}
