// C++ facade test of the batched point validation (include/kzg.h):
// commit::deserialize_batch / proof::deserialize_batch, the checked
// trusted_setup::verify_proofs_aggregated overload and trusted_setup::check_setup
// on a degree-40 setup with a fixed tau.  Run by tests/test_gpu_cpp_subgroup.py;
// a non-zero exit status or a FAILED line is a failure.
//
// usage: test_subgroup <curve 0|1> <tau hex> <setup file to write> [<x hex> <y hex>]
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

// big-endian hex -> mb bytes, left-padded with zeros
static std::vector<uint8_t> be_bytes(const std::string& h, size_t mb) {
  std::string s = h.rfind("0x", 0) == 0 ? h.substr(2) : h;
  if (s.size() % 2) s = "0" + s;
  std::vector<uint8_t> out(mb, 0);
  const size_t nb = s.size() / 2;
  for (size_t k = 0; k < nb && k < mb; k++)
    out[mb - 1 - k] = (uint8_t)strtol(s.substr(s.size() - 2 * (k + 1), 2).c_str(), nullptr, 16);
  return out;
}

int main(int argc, char** argv) {
  if (argc < 4) {
    std::cerr << "usage: test_subgroup <curve> <tau hex> <setup file> [<x hex> <y hex>]" << std::endl;
    return 2;
  }
  const int curve = atoi(argv[1]);
  kzg::init(curve);
  const kzg::Fr tau = fr_from_hex(argv[2]);
  const std::string path = argv[3];
  kzg::trusted_setup kzg(41, tau);

  // 62 commitments of small polynomials, serialized, and three octets that are no points
  std::vector<kzg::poly> polys;
  for (long k = 0; k < 62; k++) polys.push_back(kzg::poly({kzg::Fr(k + 1), kzg::Fr(3 * k - 7), kzg::Fr(k * k + 2)}));
  std::vector<kzg::commit> made = kzg.create_commits(polys);
  std::vector<std::vector<uint8_t>> bytes;
  for (auto& c : made) bytes.push_back(c.serialize());
  const size_t olen = bytes[0].size();  // 4 + 1 + 2 mb
  const size_t i_trunc = 5, i_off = 33, i_zero = 64;
  std::vector<uint8_t> trunc = bytes[1];
  trunc.resize(olen - 5);
  std::vector<uint8_t> off = bytes[2];
  off[olen - 1] ^= 1;  // y +- 1: off the curve
  std::vector<uint8_t> zero = bytes[3];
  std::memset(zero.data() + 5, 0, olen - 5);
  bytes.insert(bytes.begin() + i_trunc, trunc);
  bytes.insert(bytes.begin() + i_off, off);
  bytes.push_back(zero);
  check_test(bytes.size() == 65 && bytes[i_zero] == zero && bytes[i_off] == off && bytes[i_trunc] == trunc,
             "65 octets");

  std::vector<kzg::commit> single;
  for (auto& b : bytes) single.push_back(kzg::commit::deserialize(b));
  for (int sg = 0; sg < 2; sg++) {
    const std::string tag = sg ? " (check_subgroup)" : "";
    std::vector<bool> valid;
    std::vector<kzg::commit> batch = kzg::commit::deserialize_batch(bytes, sg != 0, &valid);
    bool same = batch.size() == 65 && valid.size() == 65;
    for (size_t k = 0; same && k < 65; k++) same = batch[k].get_curve_point() == single[k].get_curve_point();
    check_test(same, "deserialize_batch equals 65 deserialize calls" + tag);
    bool marks = valid.size() == 65;
    for (size_t k = 0; marks && k < 65; k++) marks = valid[k] == !(k == i_trunc || k == i_off || k == i_zero);
    check_test(marks, "valid marks exactly the three bad octets" + tag);
    check_test(batch[i_trunc].get_curve_point().inf && batch[i_off].get_curve_point().inf &&
                   batch[i_zero].get_curve_point().inf,
               "bad octets decode to infinity" + tag);
    std::vector<kzg::proof> pb = kzg::proof::deserialize_batch(bytes, sg != 0);
    bool psame = pb.size() == 65;
    for (size_t k = 0; psame && k < 65; k++)
      psame = pb[k].get_curve_point() == kzg::proof::deserialize(bytes[k]).get_curve_point();
    check_test(psame, "proof::deserialize_batch equals proof::deserialize" + tag);
  }
  check_test(kzg::commit::deserialize_batch({}).empty(), "empty batch");
  {
    bool finite = true;
    for (size_t k = 0; k < 65; k++)
      if (k != i_trunc && k != i_off && k != i_zero) finite = finite && !single[k].get_curve_point().inf;
    check_test(finite, "the 62 good octets decode to finite points");
  }

  // a curve point outside the prime-order subgroup (BLS12-381)
  if (argc >= 6) {
    const size_t mb = (olen - 5) / 2;
    std::vector<uint8_t> oct(olen, 0);
    const uint32_t len = (uint32_t)(1 + 2 * mb);
    std::memcpy(oct.data(), &len, 4);
    oct[4] = 0x04;
    const std::vector<uint8_t> xb = be_bytes(argv[4], mb), yb = be_bytes(argv[5], mb);
    std::memcpy(oct.data() + 5, xb.data(), mb);
    std::memcpy(oct.data() + 5 + mb, yb.data(), mb);
    std::vector<std::vector<uint8_t>> two = {bytes[0], oct, bytes[1]};
    const kzg::G1 plain = kzg::commit::deserialize(oct).get_curve_point();
    check_test(!plain.inf, "the non-member is on the curve (deserialize keeps it)");
    std::vector<bool> valid;
    std::vector<kzg::commit> lax = kzg::commit::deserialize_batch(two, false, &valid);
    check_test(lax[1].get_curve_point() == plain && !lax[1].get_curve_point().inf && valid[1],
               "non-member returned unchanged without check_subgroup");
    check_test(lax[1].serialize() == oct, "non-member round-trips");
    std::vector<kzg::commit> strict = kzg::commit::deserialize_batch(two, true, &valid);
    check_test(strict[1].get_curve_point().inf && !valid[1], "non-member is infinity, valid = false under check_subgroup");
    check_test(strict[0].get_curve_point() == single[0].get_curve_point() && valid[0] && valid[2] &&
                   strict[2].get_curve_point() == single[1].get_curve_point(),
               "its neighbours are untouched");
  }

  // the checked aggregate on honest openings
  {
    const std::string text = "checked aggregate of openings";
    kzg::poly p = kzg::poly::from_blob(kzg::blob::from_string(text));
    kzg::commit c = kzg.create_commit(p);
    std::vector<long> at;
    for (long i = 0; i < 12; i++) at.push_back(2 * i);
    std::vector<kzg::proof> pr = kzg.create_proofs(p, at);
    std::vector<kzg::commit> commits(at.size(), c);
    std::vector<std::pair<kzg::Fr, kzg::Fr>> points;
    for (size_t k = 0; k < at.size(); k++) points.push_back({kzg::Fr(at[k]), kzg::Fr((long)(signed char)text[at[k]])});
    check_test(kzg.verify_proofs_aggregated(commits, pr, points, true), "checked aggregate (subgroup) of honest openings");
    check_test(kzg.verify_proofs_aggregated(commits, pr, points, false), "checked aggregate (curve only)");
    check_test(kzg.verify_proofs_aggregated(commits, pr, points), "unchecked aggregate agrees");
    auto tampered = points;
    tampered[7].second = kzg::Fr((long)(signed char)text[at[7]] + 1);
    check_test(!kzg.verify_proofs_aggregated(commits, pr, tampered, true), "checked aggregate refutes one flipped y");
    std::vector<kzg::commit> none_c;
    std::vector<kzg::proof> none_p;
    std::vector<std::pair<kzg::Fr, kzg::Fr>> none_x;
    check_test(kzg.verify_proofs_aggregated(none_c, none_p, none_x, true), "empty checked batch is true");
    bool threw = false;
    try {
      tampered.pop_back();
      kzg.verify_proofs_aggregated(commits, pr, tampered, true);
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    check_test(threw, "checked aggregate size mismatch throws");
  }

  // the setup itself
  check_test(kzg.check_setup(), "check_setup on a generated setup");
  check_test(kzg.check_setup(false), "check_setup(false) on a generated setup");
  kzg.export_setup(path);
  {
    kzg::trusted_setup loaded(path);
    check_test(loaded.size() == kzg.size(), "setup reloaded from export_setup");
    check_test(loaded.check_setup(), "check_setup on the reloaded setup");
  }
  std::remove(path.c_str());
  std::cout << (failures ? "SOME TESTS FAILED" : "ALL TESTS PASSED") << std::endl;
  return failures ? 1 : 0;
}
