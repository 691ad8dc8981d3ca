"""GPU: the C++ facade's setup ceremony (trusted_setup::contribute,
verify_structure, verify_contribution; include/kzg.h) driven by
tests/cpp/test_srs_ceremony.cpp on a degree-40 setup with the golden fixtures'
tau and a fixed secret: contribute then verify_structure() and
verify_contribution hold, commit / prove / verify round-trips under the new tau,
and a setup file with one point replaced passes check_setup and fails
verify_structure()."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_srs_ceremony")
GOLD = os.path.join(ROOT, "tests", "golden")
SECRET = "2b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da56a784d9045190cfe"  # < r on both curves


@pytest.mark.parametrize("curve_id,name", [(0, "BN254"), (1, "BLS12381")])
def test_cpp_srs_ceremony(curve_id, name, tmp_path):
    assert os.path.exists(BIN), "run __graft_entry__.build()"
    with open(os.path.join(GOLD, name + ".json")) as f:
        tau = json.load(f)["tau"]
    args = [BIN, str(curve_id), tau, SECRET, str(tmp_path / "setup.bin")]
    res = subprocess.run(args, capture_output=True, text=True, timeout=300)
    out = res.stdout.splitlines()
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert not [l for l in out if l.startswith("FAILED")]
    assert len([l for l in out if l.startswith("PASSED")]) == 16
    assert out[-1] == "ALL TESTS PASSED"
