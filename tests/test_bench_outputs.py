"""bench.py --dump-outputs and the plain / --full split.

CPU: the dump format (float64 arrays of 32-bit words, exact) round-trips.
GPU: one plain run of bench.py at a small batch prints the headline line with
every --full field null, and the dumped outputs of its last timed step are the
commits, proofs and evaluations of the seeded inputs (C oracle identity)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def _ints(words, k):
    """(B, m) float64 32-bit words -> per row, the integers of each k-word group"""
    assert words.dtype == np.float64
    w = words.astype(np.uint64)
    assert np.array_equal(w.astype(np.float64), words) and int(w.max(initial=0)) < 1 << 32
    return [[sum(int(row[g * k + i]) << (32 * i) for i in range(k)) for g in range(w.shape[1] // k)] for row in w]


def test_dump_format_round_trips(tmp_path):
    bench = _bench()
    rng = np.random.default_rng(7)
    limbs = rng.integers(0, 2**64, size=(5, 8), dtype=np.uint64)
    limbs[0, :] = np.uint64(2**64 - 1)
    flags = np.array([0, 1, 0, 0, 1], dtype=np.int32)
    bench.dump_outputs(str(tmp_path / "d"), {"xy": limbs.view(np.int64), "inf": flags})
    bench.dump_outputs(str(tmp_path / "d"), {"xy": limbs}, rank=2)
    xy = np.load(tmp_path / "d" / "xy.npy")
    assert xy.dtype == np.float64 and xy.shape == (5, 16)
    got = _ints(xy, 8)
    assert got == [[sum(int(r[g * 4 + i]) << (64 * i) for i in range(4)) for g in range(2)] for r in limbs]
    inf = np.load(tmp_path / "d" / "inf.npy")
    assert inf.dtype == np.float64 and inf.tolist() == flags.tolist()
    assert np.array_equal(np.load(tmp_path / "d" / "xy_rank2.npy"), xy)


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path, oracle_c):
    bench = _bench()
    import kzg_ref as K
    B, steps = 8, 3
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--batch", str(B),
                        "--fixed-bits", "7", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    line = lines[0]
    assert line["steps"] == steps and line["full"] is False and line["higher_is_better"] is True
    assert line["unit"] == "commits+proofs/s" and line["metric"].startswith("KZG commits/sec + proofs/sec, BN254")
    assert line["dtype"].startswith("u32") and line["ms_per_step"] > 0
    assert abs(line["value"] - 2 * B / (line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
    # nothing beyond the headline ran
    assert line["parity"] is None and line["cpu_baseline"] is None
    sec = line["secondary"]
    for k in ("default_table", "pippenger", "latency", "setup_ms", "table_curve", "valu_yardstick", "mad_issue"):
        assert sec[k] is None, k
    assert line["roofline"]["kernel_code"] == {"sha256": None} and line["roofline"]["traffic"] is None
    # the dumped outputs of the last step against the oracle identity
    C = K.BN254
    tau = K.default_tau(C)
    n = bench.DEGREE + 1
    coeffs, zs = bench.bench_inputs(C, "cfg2", B, n)
    cxy = _ints(np.load(out / "commit_xy.npy"), 8)
    pxy = _ints(np.load(out / "proof_xy.npy"), 8)
    ys = _ints(np.load(out / "proof_y.npy"), 8)
    cinf = np.load(out / "commit_inf.npy")
    pinf = np.load(out / "proof_inf.npy")
    assert len(cxy) == len(pxy) == len(ys) == B and cinf.shape == pinf.shape == (B,)
    G = (C.gx, C.gy)
    for b in range(B):
        ptau = oracle_c.poly_eval("BN254", coeffs[b], tau)
        z = int(zs[b, 0])
        pz = oracle_c.poly_eval("BN254", coeffs[b], z)
        qt = (ptau - pz) * pow((tau - z) % C.r, -1, C.r) % C.r
        assert (None if cinf[b] else tuple(cxy[b])) == oracle_c.scalar_mul("BN254", G, ptau), b
        assert (None if pinf[b] else tuple(pxy[b])) == oracle_c.scalar_mul("BN254", G, qt), b
        assert ys[b] == [pz], b
