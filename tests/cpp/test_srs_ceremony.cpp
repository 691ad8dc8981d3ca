// C++ facade test of the setup ceremony (include/kzg.h):
// trusted_setup::contribute, verify_structure and verify_contribution on a
// degree-40 setup with a fixed tau and a fixed secret.  Run by
// tests/test_gpu_cpp_srs_ceremony.py; a non-zero exit status or a FAILED line
// is a failure.
//
// usage: test_srs_ceremony <curve 0|1> <tau hex> <s hex> <setup file to write>
#include <kzg.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>
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

int main(int argc, char** argv) {
  if (argc < 5) {
    std::cerr << "usage: test_srs_ceremony <curve> <tau hex> <s hex> <setup file>" << std::endl;
    return 2;
  }
  const int curve = atoi(argv[1]);
  kzg::init(curve);
  const kzg::Fr tau = fr_from_hex(argv[2]), s = fr_from_hex(argv[3]);
  const std::string path = argv[4];
  kzg::trusted_setup kzg(41, tau);

  check_test(kzg.check_setup() && kzg.verify_structure(), "a generated setup has the structure");
  const std::string text = "a setup nobody knows the secret of";
  kzg::poly p = kzg::poly::from_blob(kzg::blob::from_string(text));
  kzg::commit old_commit = kzg.create_commit(p);
  const kzg::G1 prev_tau = kzg.g1_points()[1];

  // one contribution
  const kzg::G2 witness = kzg.contribute(s);
  const kzg::G1 new_tau = kzg.g1_points()[1];
  check_test(!witness.inf && new_tau != prev_tau, "contribute moves [tau]G1 and returns a finite witness");
  check_test(kzg.check_setup() && kzg.verify_structure(), "contribute then verify_structure()");
  check_test(kzg.verify_structure(false), "verify_structure(false) as well");
  check_test(kzg::trusted_setup::verify_contribution(prev_tau, new_tau, witness), "verify_contribution");
  check_test(!kzg::trusted_setup::verify_contribution(new_tau, prev_tau, witness), "not with the two points exchanged");
  check_test(!kzg::trusted_setup::verify_contribution(prev_tau, new_tau, kzg.g2_points()[1]),
             "not with [tau s]G2 for a witness");
  check_test(!kzg::trusted_setup::verify_contribution(prev_tau, new_tau, kzg::G2()), "not with an infinite witness");
  {
    kzg::trusted_setup direct(41, fr_from_hex(argv[2]));  // the same contribution again: deterministic
    const kzg::G2 w2 = direct.contribute(s);
    check_test(w2 == witness && direct.g1_points() == kzg.g1_points() && direct.g2_points() == kzg.g2_points(),
               "the same secret on the same setup gives the same setup and witness");
  }

  // commit / prove / verify under the new tau
  {
    kzg::commit c = kzg.create_commit(p);
    check_test(c.get_curve_point() != old_commit.get_curve_point(), "commitments move with the setup");
    kzg::proof pr = kzg.create_proof(p, 3, 4);
    kzg::blob expected = kzg::blob::from_string(text.substr(3, 4), 3);
    check_test(kzg.verify_proof(c, pr, expected), "create_commit / create_proof / verify_proof under the new tau");
    check_test(!kzg.verify_proof(old_commit, pr, expected), "the old setup's commitment no longer verifies");
  }
  {
    bool threw = false;
    try {
      kzg.contribute(kzg::Fr(0));
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    check_test(threw && kzg.g1_points()[1] == new_tau, "contribute(0) throws and leaves the setup");
  }

  // a setup file with one point replaced by another point of the same file:
  // every point is still a valid subgroup point, the powers are not consecutive
  kzg.export_setup(path);
  {
    kzg::trusted_setup loaded(path);
    check_test(loaded.check_setup() && loaded.verify_structure(), "the exported setup reloads with the structure");
  }
  {
    std::ifstream in(path, std::ios::binary);
    std::vector<char> bytes((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    in.close();
    const size_t mb = curve == 0 ? 32 : 48, rec = 4 + 1 + 2 * mb;  // u32 length, 0x04, x, y
    std::copy(bytes.begin() + 8 + 3 * rec, bytes.begin() + 8 + 4 * rec, bytes.begin() + 8 + 5 * rec);  // G1[5] := G1[3]
    std::ofstream out(path, std::ios::binary | std::ios::trunc);
    out.write(bytes.data(), (std::streamsize)bytes.size());
    out.close();
    kzg::trusted_setup bad(path);
    check_test(bad.check_setup(), "check_setup passes a file with one G1 point replaced");
    check_test(!bad.verify_structure(false) && !bad.verify_structure(), "verify_structure() refutes it");
  }
  std::remove(path.c_str());
  std::cout << (failures ? "SOME TESTS FAILED" : "ALL TESTS PASSED") << std::endl;
  return failures ? 1 : 0;
}
