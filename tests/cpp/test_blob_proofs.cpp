// C++ facade test of the blob proofs (include/kzg.h): trusted_setup::create_blob_proofs,
// verify_blob_proofs and verify_blob_proofs_each on BLS12-381 with a fixed tau.  The
// expected records come from the C ABI's separate steps on a context of its own with the
// same tau -- kzgx_commit_evals_batch, kzgx_g1_compress_batch, the host helper
// kzgx_blob_challenge, kzgx_prove_evals_batch -- then tampered batches, then the
// refusals.  Run by tests/test_gpu_cpp_blob_proofs.py; a non-zero exit status or a FAILED
// line is a failure.
//
// usage: test_blob_proofs <tau hex>
#include <kzg.h>

#include <algorithm>
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

// r - 1, big-endian: the largest canonical element
static const uint8_t R_MINUS_1[32] = {0x73, 0xed, 0xa7, 0x53, 0x29, 0x9d, 0x7d, 0x48, 0x33, 0x39, 0xd8,
                                      0x08, 0x09, 0xa1, 0xd8, 0x05, 0x53, 0xbd, 0xa4, 0x02, 0xff, 0xfe,
                                      0x5b, 0xfe, 0xff, 0xff, 0xff, 0xff, 0x00, 0x00, 0x00, 0x00};

int main(int argc, char** argv) {
  if (argc < 2) {
    std::cerr << "usage: test_blob_proofs <tau hex>" << std::endl;
    return 2;
  }
  kzg::init(KZGX_CURVE_BLS12381);
  const kzg::Fr tau = fr_from_hex(argv[1]);
  kzg::trusted_setup kzg(300, tau);
  const unsigned k = 6;
  const size_t n = (size_t)1 << k, m = 3, bb = 32 * n;

  kzgx_ctx* c = nullptr;
  bool abi = kzgx_create(&c, KZGX_CURVE_BLS12381, 0) == KZGX_OK && kzgx_set_default_table(c, 0, 0) == KZGX_OK &&
             kzgx_gen_srs_g1(c, tau.v.data(), 0, 300) == KZGX_OK;
  check_test(abi, "a C ABI context on the same tau");
  if (!abi) return 1;

  // three blobs of big-endian elements (element 5 of blob 1 is r - 1), and the same as limbs
  std::vector<uint8_t> blobs(m * bb, 0);
  for (size_t b = 0; b < m; b++)
    for (size_t i = 0; i < n; i++) {
      uint8_t* e = &blobs[b * bb + 32 * i];
      const uint64_t v = 1000003 * (b + 1) + i * i * i + 7 * i;
      for (int j = 0; j < 8; j++) e[31 - j] = (uint8_t)(v >> (8 * j));
      e[3] = (uint8_t)(b + i);  // a high byte, still < r
    }
  std::memcpy(&blobs[bb + 32 * 5], R_MINUS_1, 32);
  std::vector<uint64_t> limbs(4 * m * n);
  for (size_t i = 0; i < m * n; i++)
    for (int w = 0; w < 4; w++) {
      uint64_t v = 0;
      for (int j = 0; j < 8; j++) v = (v << 8) | blobs[32 * i + 8 * (3 - w) + j];
      limbs[4 * i + w] = v;
    }

  for (int rev = 0; rev < 2; rev++) {
    const std::string tag = rev ? " (bit-reversed)" : " (natural order)";
    const int nflags = rev ? KZGX_NTT_BITREV : 0;
    // the separate steps
    std::vector<uint64_t> xy(12 * m), z(4 * m), y(4 * m);
    std::vector<int> inf(m);
    std::vector<uint8_t> crec(48 * m), prec(48 * m);
    bool steps = kzgx_commit_evals_batch(c, limbs.data(), k, m, nflags, xy.data(), inf.data()) == KZGX_OK &&
                 kzgx_g1_compress_batch(c, xy.data(), inf.data(), m, KZGX_ENC_ZCASH, crec.data()) == KZGX_OK;
    for (size_t b = 0; steps && b < m; b++) {
      int ok = 0;
      steps = kzgx_blob_challenge(KZGX_CURVE_BLS12381, &blobs[b * bb], k, KZGX_BLOB_BYTES, &crec[48 * b], &z[4 * b],
                                  &ok) == KZGX_OK && ok == 1;
    }
    steps = steps && kzgx_prove_evals_batch(c, limbs.data(), k, n, z.data(), m, nflags, xy.data(), inf.data(),
                                            y.data()) == KZGX_OK &&
            kzgx_g1_compress_batch(c, xy.data(), inf.data(), m, KZGX_ENC_ZCASH, prec.data()) == KZGX_OK;
    check_test(steps, "commit, compress, challenge, open, compress through the C ABI" + tag);

    auto made = kzg.create_blob_proofs(blobs, k, rev != 0);
    check_test(made.first == crec, "create_blob_proofs: the commitments" + tag);
    check_test(made.second == prec, "create_blob_proofs: the proofs" + tag);
    check_test(kzg.verify_blob_proofs(blobs, crec, prec, k, rev != 0), "verify_blob_proofs" + tag);
    check_test(kzg.verify_blob_proofs_each(blobs, crec, prec, k, rev != 0) == std::vector<bool>({true, true, true}),
               "verify_blob_proofs_each" + tag);
    check_test(!kzg.verify_blob_proofs(blobs, crec, prec, k, rev == 0), "the other order is another polynomial" + tag);

    std::vector<uint8_t> t = blobs;
    t[bb + 32 * 9 + 31] ^= 1;  // a value of blob 1
    check_test(!kzg.verify_blob_proofs(t, crec, prec, k, rev != 0), "a changed value" + tag);
    check_test(kzg.verify_blob_proofs_each(t, crec, prec, k, rev != 0) == std::vector<bool>({true, false, true}),
               "a changed value: that blob only" + tag);
    std::vector<uint8_t> sw = prec;  // proofs 0 and 2 swapped
    std::swap_ranges(sw.begin(), sw.begin() + 48, sw.begin() + 96);
    check_test(!kzg.verify_blob_proofs(blobs, crec, sw, k, rev != 0), "two swapped proofs" + tag);
    check_test(kzg.verify_blob_proofs_each(blobs, crec, sw, k, rev != 0) == std::vector<bool>({false, true, false}),
               "two swapped proofs: those two blobs" + tag);
    t = blobs;
    t[2 * bb + 32 * 5 + 0] = 0x80;  // an element >= r in blob 2
    check_test(!kzg.verify_blob_proofs(t, crec, prec, k, rev != 0), "a non-canonical element" + tag);
    check_test(kzg.verify_blob_proofs_each(t, crec, prec, k, rev != 0) == std::vector<bool>({true, true, false}),
               "a non-canonical element: that blob only" + tag);
    check_test(throws<std::invalid_argument>([&] { kzg.create_blob_proofs(t, k, rev != 0); }),
               "create_blob_proofs refuses a non-canonical element" + tag);
    std::vector<uint8_t> bad = crec;
    bad[0] &= 0x7f;  // the compression flag cleared: no record
    check_test(!kzg.verify_blob_proofs(blobs, bad, prec, k, rev != 0), "a malformed record" + tag);
    check_test(kzg.verify_blob_proofs_each(blobs, bad, prec, k, rev != 0) == std::vector<bool>({false, true, true}),
               "a malformed record: that blob only" + tag);
  }
  kzgx_destroy(c);

  // an empty batch, the refusals
  const std::vector<uint8_t> none;
  check_test(kzg.verify_blob_proofs(none, none, none, k), "no blobs: true");
  check_test(kzg.verify_blob_proofs_each(none, none, none, k).empty(), "no blobs: no verdicts");
  auto made = kzg.create_blob_proofs(blobs, k);
  std::vector<uint8_t> cut(blobs.begin(), blobs.end() - 1), few(made.first.begin(), made.first.end() - 48);
  check_test(throws<std::invalid_argument>([&] { kzg.create_blob_proofs(cut, k); }), "not a whole number of blobs");
  check_test(throws<std::invalid_argument>([&] { kzg.verify_blob_proofs(cut, made.first, made.second, k); }),
             "verify: not a whole number of blobs");
  check_test(throws<std::invalid_argument>([&] { kzg.verify_blob_proofs(blobs, few, made.second, k); }),
             "verify: fewer commitments than blobs");
  check_test(throws<std::invalid_argument>([&] { kzg.verify_blob_proofs_each(blobs, made.first, few, k); }),
             "verify each: fewer proofs than blobs");
  check_test(throws<std::invalid_argument>([&] { kzg.create_blob_proofs(blobs, 23); }), "no 2^23 domain");
  std::vector<uint8_t> wide(32 << 9, 0);
  for (size_t i = 0; i < 512; i++) wide[32 * i + 31] = (uint8_t)(3 * i + 1);
  check_test(throws<std::invalid_argument>([&] { kzg.create_blob_proofs(wide, 9); }), "2^9 > size() = 300");
  // the verifier needs G1[0] and G2[0..1] only: a blob wider than the setup verifies
  kzg::trusted_setup big(600, tau);
  auto pw = big.create_blob_proofs(wide, 9);
  check_test(kzg.verify_blob_proofs(wide, pw.first, pw.second, 9), "a blob of 512 elements on a 300-point setup");

  if (failures) {
    std::cout << failures << " TESTS FAILED" << std::endl;
    return 1;
  }
  std::cout << "ALL TESTS PASSED" << std::endl;
  return 0;
}
