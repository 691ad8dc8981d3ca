"""GPU: the C++ facade's per-cell verdicts (trusted_setup::verify_coset_proofs_each and its checked
overload; include/kzg.h) driven by tests/cpp/test_verify_cells_each.cpp under kzg::init(BLS12-381) on a
300-point setup with the golden fixtures' tau: honest cells of two polynomials are all true, each
tampering makes exactly the touched cells false, an off-curve proof or commitment zeroes its own cells
in the checked form, an empty batch gives no verdicts; then the std::invalid_argument cases and BN254."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_verify_cells_each")
GOLD = os.path.join(ROOT, "tests", "golden")


def test_cpp_verify_cells_each():
    assert os.path.exists(BIN), "run __graft_entry__.build()"
    with open(os.path.join(GOLD, "BLS12381.json")) as f:
        tau = json.load(f)["tau"]
    res = subprocess.run([BIN, tau], capture_output=True, text=True, timeout=300)
    out = res.stdout.splitlines()
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert not [l for l in out if l.startswith("FAILED")]
    assert len([l for l in out if l.startswith("PASSED")]) == 26
    assert out[-1] == "ALL TESTS PASSED"
