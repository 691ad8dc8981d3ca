"""GPU: the C++ facade's compressed point encodings (commit / proof::serialize_compressed and
deserialize_compressed_batch, trusted_setup::from_compressed, the verify_coset_proofs overload
on packed records; include/kzg.h) driven by tests/cpp/test_point_codec.cpp on a 40-point setup
with the golden fixtures' tau.  On BLS12-381 the wrapper hands the driver a curve point outside
the prime-order subgroup, built and checked with the Python oracle."""
import json
import os
import subprocess

import pytest

import kzg_ref as K
from test_subgroup_consts import g1_member, g1_order_point

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_point_codec")
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.mark.parametrize("curve_id,name", [(0, "BN254"), (1, "BLS12381")])
def test_cpp_point_codec(curve_id, name):
    assert os.path.exists(BIN), "run __graft_entry__.build()"
    with open(os.path.join(GOLD, name + ".json")) as f:
        tau = json.load(f)["tau"]
    args = [BIN, str(curve_id), tau]
    expected = 21  # one encoding: 9 codec checks, 4 general, 7 on cells, 1 on the identity batch
    if name == "BLS12381":
        C = K.BLS12381
        P = K.point_add(C, K.scalar_mul(C, (C.gx, C.gy), 31415926), g1_order_point(11))
        assert K.on_curve(C, P) and not g1_member(C, P)
        args += ["%096x" % P[0], "%096x" % P[1]]
        expected = 46  # two encodings, the non-member (4) and from_compressed (8)
    res = subprocess.run(args, capture_output=True, text=True, timeout=300)
    out = res.stdout.splitlines()
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert not [l for l in out if l.startswith("FAILED")]
    assert len([l for l in out if l.startswith("PASSED")]) == expected
    assert out[-1] == "ALL TESTS PASSED"
