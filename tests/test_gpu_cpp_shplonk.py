"""GPU: the C++ facade's Shplonk openings (create_shplonk_proof, verify_shplonk_proof;
include/kzg.h) driven by tests/cpp/test_shplonk.cpp on a degree-40 setup with the golden
fixtures' tau."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_shplonk")
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.mark.parametrize("curve_id,name", [(0, "BN254"), (1, "BLS12381")])
def test_cpp_shplonk_openings(curve_id, name):
    assert os.path.exists(BIN), "run __graft_entry__.build()"
    with open(os.path.join(GOLD, name + ".json")) as f:
        tau = json.load(f)["tau"]
    res = subprocess.run([BIN, str(curve_id), tau], capture_output=True, text=True, timeout=300)
    out = res.stdout.splitlines()
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert not [l for l in out if l.startswith("FAILED")]
    assert len([l for l in out if l.startswith("PASSED")]) == 27
    assert out[-1] == "ALL TESTS PASSED"
