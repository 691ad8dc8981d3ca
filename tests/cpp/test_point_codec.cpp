// C++ facade test of the compressed point encodings (include/kzg.h):
// commit / proof::serialize_compressed and deserialize_compressed_batch,
// trusted_setup::from_compressed and the verify_coset_proofs overload on packed
// records, on a 40-point setup with a fixed tau.  Run by
// tests/test_gpu_cpp_point_codec.py; a non-zero exit status or a FAILED line is
// a failure.
//
// usage: test_point_codec <curve 0|1> <tau hex> [<x hex> <y hex>]
//   x, y: a curve point outside the prime-order subgroup (BLS12-381 only), big-endian
#include <kzg.h>

#include <cstdio>
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

static kzg::Fr fr_from_hex(const std::string& h) {
  std::string s = h.rfind("0x", 0) == 0 ? h.substr(2) : h;
  std::vector<uint8_t> le;
  for (int i = (int)s.size(); i > 0; i -= 2) {
    std::string byte = s.substr(i >= 2 ? i - 2 : 0, i >= 2 ? 2 : 1);
    le.push_back((uint8_t)strtol(byte.c_str(), nullptr, 16));
  }
  return kzg::Fr::from_le_bytes(le.data(), le.size());
}

// big-endian hex -> little-endian 64-bit limbs
static std::array<uint64_t, 6> limbs_from_hex(const std::string& h) {
  std::string s = h.rfind("0x", 0) == 0 ? h.substr(2) : h;
  std::array<uint64_t, 6> out{};
  for (size_t k = 0; k < s.size() && k < 96; k++) {
    const char c = s[s.size() - 1 - k];
    const uint64_t d = (uint64_t)(c <= '9' ? c - '0' : (c | 0x20) - 'a' + 10);
    out[k / 16] |= d << (4 * (k % 16));
  }
  return out;
}

template <class E, class F>
static bool throws(F&& f) {
  try {
    f();
  } catch (const E&) {
    return true;
  } catch (...) {
  }
  return false;
}

static void append(std::vector<uint8_t>& to, const std::vector<uint8_t>& rec) {
  to.insert(to.end(), rec.begin(), rec.end());
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::cerr << "usage: test_point_codec <curve> <tau hex> [<x hex> <y hex>]" << std::endl;
    return 2;
  }
  const int curve = atoi(argv[1]);
  const bool bls = curve == KZGX_CURVE_BLS12381;
  kzg::init(curve);
  const kzg::Fr tau = fr_from_hex(argv[2]);
  kzg::trusted_setup kzg(40, tau);
  const size_t mb = bls ? 48 : 32;

  std::vector<kzg::poly> polys;
  for (long k = 0; k < 62; k++) polys.push_back(kzg::poly({kzg::Fr(k + 1), kzg::Fr(3 * k - 7), kzg::Fr(k * k + 2)}));
  std::vector<kzg::commit> made = kzg.create_commits(polys);

  std::vector<int> encs;
  if (bls) encs.push_back(KZGX_ENC_ZCASH);
  encs.push_back(KZGX_ENC_SEC1);
  for (int enc : encs) {
    const std::string tag = enc == KZGX_ENC_ZCASH ? " (zcash)" : " (sec1)";
    const size_t rb = kzgx_point_bytes(curve, 1, enc);
    check_test(rb == (enc == KZGX_ENC_ZCASH ? 48 : 1 + mb), "record length" + tag);
    std::vector<uint8_t> packed;
    bool shape = true;
    for (auto& c : made) {
      const std::vector<uint8_t> rec = c.serialize_compressed(enc);
      const std::vector<uint8_t> oct = c.serialize();  // u32 length, 0x04, x, y
      shape = shape && rec.size() == rb && oct.size() == 5 + 2 * mb;
      if (enc == KZGX_ENC_SEC1) {
        shape = shape && rec[0] == (2 | (oct[4 + 2 * mb] & 1)) && !std::memcmp(&rec[1], &oct[5], mb);
      } else {
        shape = shape && (rec[0] & 0xC0) == 0x80 && (rec[0] & 0x1F) == oct[5] && !std::memcmp(&rec[1], &oct[6], mb - 1);
      }
      append(packed, rec);
    }
    check_test(shape, "records carry the octet's x and the sign of its y" + tag);
    for (int sg = 0; sg < 2; sg++) {
      std::vector<bool> valid;
      std::vector<kzg::commit> back = kzg::commit::deserialize_compressed_batch(packed, enc, sg != 0, &valid);
      bool same = back.size() == 62 && valid.size() == 62;
      for (size_t k = 0; same && k < 62; k++)
        same = valid[k] && back[k].get_curve_point() == made[k].get_curve_point();
      check_test(same, std::string("62 records round-trip") + (sg ? ", check_subgroup" : "") + tag);
    }
    // a malformed head, an x without a root (x = 1 on both curves), the identity
    std::vector<uint8_t> bad = packed;
    const size_t i_head = 5, i_root = 33, i_inf = 40;
    bad[i_head * rb] = enc == KZGX_ENC_SEC1 ? 0x04 : (uint8_t)(bad[i_head * rb] & 0x7F);
    std::memset(&bad[i_root * rb], 0, rb);
    bad[i_root * rb] = enc == KZGX_ENC_SEC1 ? 0x03 : 0xA0;
    bad[(i_root + 1) * rb - 1] = 1;
    const std::vector<uint8_t> ident = kzg::commit(kzg::G1()).serialize_compressed(enc);
    check_test(ident.size() == rb && ident[0] == (enc == KZGX_ENC_SEC1 ? 0x00 : 0xC0), "the identity record" + tag);
    std::memcpy(&bad[i_inf * rb], ident.data(), rb);
    std::vector<bool> valid;
    std::vector<kzg::proof> pb = kzg::proof::deserialize_compressed_batch(bad, enc, true, &valid);
    bool marks = pb.size() == 62 && valid.size() == 62;
    for (size_t k = 0; marks && k < 62; k++) {
      const kzg::G1& g = pb[k].get_curve_point();
      if (k == i_head || k == i_root)
        marks = !valid[k] && g.inf;
      else if (k == i_inf)
        marks = valid[k] && g.inf;
      else
        marks = valid[k] && g == made[k].get_curve_point();
    }
    check_test(marks, "bad records decode to infinity with valid = false, their neighbours exactly" + tag);
    check_test(kzg::proof(pb[7].get_curve_point()).serialize_compressed(enc) ==
                   std::vector<uint8_t>(packed.begin() + 7 * rb, packed.begin() + 8 * rb),
               "proof::serialize_compressed" + tag);
    check_test(kzg::commit::deserialize_compressed_batch({}, enc).empty(), "empty batch" + tag);
    std::vector<uint8_t> ragged(packed.begin(), packed.begin() + 2 * rb + 1);
    check_test(throws<std::invalid_argument>([&] { kzg::commit::deserialize_compressed_batch(ragged, enc); }),
               "a ragged size throws" + tag);
  }
  check_test(throws<std::invalid_argument>([&] { made[0].serialize_compressed(7); }) &&
                 throws<std::invalid_argument>([&] { kzg::commit::deserialize_compressed_batch({}, 7); }),
             "an unknown encoding throws");
  // the existing octets keep their behaviour
  check_test(kzg::commit::deserialize(made[3].serialize()).get_curve_point() == made[3].get_curve_point(),
             "serialize / deserialize unchanged");

  if (!bls) {
    check_test(throws<std::invalid_argument>([&] { made[0].serialize_compressed(KZGX_ENC_ZCASH); }),
               "BN254 refuses the ZCash encoding");
    check_test(throws<std::invalid_argument>([&] {
                 kzg::trusted_setup::from_compressed(std::vector<uint8_t>(48, 0), std::vector<uint8_t>(96, 0));
               }),
               "BN254 refuses from_compressed");
  }

  // a curve point outside the prime-order subgroup (BLS12-381)
  if (argc >= 5) {
    kzg::G1 non;
    non.inf = false;
    non.x = limbs_from_hex(argv[3]);
    non.y = limbs_from_hex(argv[4]);
    for (int enc : encs) {
      std::vector<uint8_t> three = made[0].serialize_compressed(enc);
      append(three, kzg::commit(non).serialize_compressed(enc));
      append(three, made[1].serialize_compressed(enc));
      std::vector<bool> valid;
      std::vector<kzg::commit> lax = kzg::commit::deserialize_compressed_batch(three, enc, false, &valid);
      check_test(lax[1].get_curve_point() == non && valid[1], "non-member decodes without check_subgroup");
      std::vector<kzg::commit> strict = kzg::commit::deserialize_compressed_batch(three, enc, true, &valid);
      check_test(strict[1].get_curve_point().inf && !valid[1] && valid[0] && valid[2] &&
                     strict[0].get_curve_point() == made[0].get_curve_point() &&
                     strict[2].get_curve_point() == made[1].get_curve_point(),
                 "non-member is infinity under check_subgroup, its neighbours untouched");
    }
  }

  // a setup from its compressed export
  if (bls) {
    const std::vector<kzg::G1> g1 = kzg.g1_points();
    const std::vector<kzg::G2> g2 = kzg.g2_points();
    std::vector<uint8_t> b1, b2(96 * g2.size());
    for (const kzg::G1& g : g1) append(b1, kzg::commit(g).serialize_compressed(KZGX_ENC_ZCASH));
    std::vector<uint64_t> w(24 * g2.size());
    for (size_t k = 0; k < g2.size(); k++)
      for (int i = 0; i < 6; i++) {
        w[24 * k + i] = g2[k].x0[i];
        w[24 * k + 6 + i] = g2[k].x1[i];
        w[24 * k + 12 + i] = g2[k].y0[i];
        w[24 * k + 18 + i] = g2[k].y1[i];
      }
    kzgx_ctx* raw = nullptr;
    bool made_g2 = kzgx_create(&raw, curve, 0) == KZGX_OK &&
                   kzgx_g2_compress_batch(raw, w.data(), nullptr, g2.size(), b2.data()) == KZGX_OK;
    if (raw) kzgx_destroy(raw);
    check_test(made_g2 && g1.size() == 40 && g2.size() == 40 && b1.size() == 40 * 48, "compressed export of the setup");
    {
      kzg::trusted_setup again = kzg::trusted_setup::from_compressed(b1, b2);
      check_test(again.size() == 40 && again.g1_points() == g1 && again.g2_points() == g2,
                 "from_compressed reproduces the G1 and G2 points");
      check_test(again.check_setup(), "check_setup on the decompressed setup");
      kzg::poly p = kzg::poly::from_blob(kzg::blob::from_string("compressed setup"));
      kzg::commit c = again.create_commit(p);
      check_test(c.get_curve_point() == kzg.create_commit(p).get_curve_point(), "the decompressed setup commits alike");
    }
    {
      // fewer G2 than G1 points (a verifier's setup)
      std::vector<uint8_t> few(b2.begin(), b2.begin() + 5 * 96);
      kzg::trusted_setup v = kzg::trusted_setup::from_compressed(b1, few, false);
      check_test(v.size() == 40 && v.g2_points().size() == 5, "a setup with 40 G1 and 5 G2 points");
    }
    std::vector<uint8_t> bad1 = b1, bad2 = b2;
    std::memset(&bad1[7 * 48 + 1], 0, 47);
    bad1[7 * 48] = 0x80;
    bad1[8 * 48 - 1] = 1;  // x = 1: no root
    bad2[3 * 96] &= 0x7F;  // C = 0
    check_test(throws<std::runtime_error>([&] { kzg::trusted_setup::from_compressed(bad1, b2); }),
               "a bad G1 record throws runtime_error");
    check_test(throws<std::logic_error>([&] { kzg::trusted_setup::from_compressed(b1, bad2); }),
               "a bad G2 record throws logic_error");
    check_test(throws<std::invalid_argument>([&] {
                 kzg::trusted_setup::from_compressed(std::vector<uint8_t>(b1.begin(), b1.end() - 1), b2);
               }),
               "a ragged G1 array throws invalid_argument");
  }

  // cells from packed records
  {
    const unsigned k = bls ? 4 : 1, kl = bls ? 2 : 0;
    const size_t l = (size_t)1 << kl, R = (size_t)1 << (k - kl + 1);
    std::vector<kzg::Fr> co;
    for (long i = 0; i < (1l << k); i++) co.push_back(kzg::Fr(1000 + 37 * i * i));
    kzg::poly P(co);
    std::vector<kzg::commit> commits = {kzg.create_commit(P)};
    std::vector<kzg::proof> proofs = kzg.create_coset_proofs(P, k, kl, true, true);
    const std::vector<kzg::Fr> ev = P.evaluate_domain(k + 1, true);
    std::vector<uint32_t> ci(R, 0), idx;
    std::vector<std::vector<kzg::Fr>> vals;
    for (size_t p = 0; p < R; p++) {
      idx.push_back((uint32_t)p);
      vals.push_back(std::vector<kzg::Fr>(ev.begin() + p * l, ev.begin() + (p + 1) * l));
    }
    check_test(proofs.size() == R && kzg.verify_coset_proofs(commits, ci, idx, proofs, vals, k, true, true, true),
               "the cells verify on points");
    for (int enc : encs) {
      const std::string tag = enc == KZGX_ENC_ZCASH ? " (zcash)" : " (sec1)";
      const size_t rb = kzgx_point_bytes(curve, 1, enc);
      std::vector<uint8_t> cb = commits[0].serialize_compressed(enc), pb;
      for (auto& pr : proofs) append(pb, pr.serialize_compressed(enc));
      check_test(kzg.verify_coset_proofs(cb, ci, idx, pb, vals, k, true, true, enc) &&
                     kzg.verify_coset_proofs(cb, ci, idx, pb, vals, k, true, true, enc, false),
                 "the cells verify on packed records" + tag);
      auto v = vals;
      v[R - 1][0] = kzg::Fr(12345);
      check_test(!kzg.verify_coset_proofs(cb, ci, idx, pb, v, k, true, true, enc), "a changed value fails" + tag);
      std::vector<uint8_t> neg = pb;
      neg[1 * rb] ^= enc == KZGX_ENC_ZCASH ? 0x20 : 0x01;  // -proof_1: decodes, does not verify
      check_test(!kzg.verify_coset_proofs(cb, ci, idx, neg, vals, k, true, true, enc), "a flipped sign fails" + tag);
      std::vector<uint8_t> undec = pb;
      undec[2 * rb] = enc == KZGX_ENC_ZCASH ? (uint8_t)(undec[2 * rb] & 0x7F) : 0x04;
      check_test(!kzg.verify_coset_proofs(cb, ci, idx, undec, vals, k, true, true, enc),
                 "a record that does not decode fails" + tag);
      std::vector<uint8_t> ragged(pb.begin(), pb.end() - 1);
      check_test(throws<std::invalid_argument>([&] { kzg.verify_coset_proofs(cb, ci, idx, ragged, vals, k, true, true, enc); }),
                 "a ragged proof array throws" + tag);
      std::vector<uint32_t> i2 = idx;
      i2[0] = (uint32_t)R;
      check_test(throws<std::invalid_argument>([&] { kzg.verify_coset_proofs(cb, ci, i2, pb, vals, k, true, true, enc); }),
                 "an index out of range throws" + tag);
    }
    check_test(kzg.verify_coset_proofs(std::vector<uint8_t>(), {}, {}, std::vector<uint8_t>(), {}, k, true, true,
                                       KZGX_ENC_SEC1),
               "an empty batch is true");
  }

  std::cout << (failures ? "SOME TESTS FAILED" : "ALL TESTS PASSED") << std::endl;
  return failures ? 1 : 0;
}
