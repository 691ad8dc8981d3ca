"""GPU: the C++ facade's cell recovery (trusted_setup::recover_cells / recover_cells_and_proofs;
include/kzg.h) driven by tests/cpp/test_recover_cells.cpp under kzg::init(BLS12-381) on a 300-point
setup with the golden fixtures' tau -- a blob from half of the cells the C ABI computed, against all
of them and against create_coset_proofs, in both orders -- then the throws."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_recover_cells")
GOLD = os.path.join(ROOT, "tests", "golden")


def test_cpp_recover_cells():
    assert os.path.exists(BIN), "run __graft_entry__.build()"
    with open(os.path.join(GOLD, "BLS12381.json")) as f:
        tau = json.load(f)["tau"]
    res = subprocess.run([BIN, tau], capture_output=True, text=True, timeout=300)
    out = res.stdout.splitlines()
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert not [l for l in out if l.startswith("FAILED")]
    assert len([l for l in out if l.startswith("PASSED")]) == 29
    assert out[-1] == "ALL TESTS PASSED"
