"""GPU: the C++ facade's blob proofs (trusted_setup::create_blob_proofs / verify_blob_proofs /
verify_blob_proofs_each; include/kzg.h) driven by tests/cpp/test_blob_proofs.cpp under
kzg::init(BLS12-381) on a 300-point setup with the golden fixtures' tau -- the records against the
C ABI's separate steps, tampered batches in both orders, then the throws."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_blob_proofs")
GOLD = os.path.join(ROOT, "tests", "golden")


def test_cpp_blob_proofs():
    assert os.path.exists(BIN), "run __graft_entry__.build()"
    with open(os.path.join(GOLD, "BLS12381.json")) as f:
        tau = json.load(f)["tau"]
    res = subprocess.run([BIN, tau], capture_output=True, text=True, timeout=300)
    out = res.stdout.splitlines()
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert not [l for l in out if l.startswith("FAILED")]
    assert len([l for l in out if l.startswith("PASSED")]) == 40
    assert out[-1] == "ALL TESTS PASSED"
