"""GPU: the C++ facade's coset openings (trusted_setup::create_coset_proofs /
create_coset_proofs_from_evaluations; include/kzg.h) driven by
tests/cpp/test_coset_proofs.cpp under kzg::init(BLS12-381) on a 300-point setup with
the golden fixtures' tau -- every proof against kzgx_prove_range on a C ABI context of
the driver's own, two cells through kzgx_verify_proof -- then the refusals, BN254's included."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_coset_proofs")
GOLD = os.path.join(ROOT, "tests", "golden")


def test_cpp_coset_proofs():
    assert os.path.exists(BIN), "run __graft_entry__.build()"
    with open(os.path.join(GOLD, "BLS12381.json")) as f:
        tau = json.load(f)["tau"]
    res = subprocess.run([BIN, tau], capture_output=True, text=True, timeout=300)
    out = res.stdout.splitlines()
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert not [l for l in out if l.startswith("FAILED")]
    assert len([l for l in out if l.startswith("PASSED")]) == 27
    assert out[-1] == "ALL TESTS PASSED"
