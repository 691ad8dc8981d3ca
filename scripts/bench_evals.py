#!/usr/bin/env python3
"""Evaluation-form commits and openings against the coefficient-form paths
they feed, and the bare Fr NTT, on one MI355X, in one process.

BLS12-381, a 4097-point SRS with the default table, polynomials of 2^12
evaluations in batches of 2048:
  (a) kzgx_commit_evals_batch_device (inverse NTT into the workspace + MSM)
  (b) kzgx_msm_g1_batch_device on the same polynomials' coefficients
  (c) kzgx_prove_evals_batch_device against kzgx_prove_single_batch_device,
      one polynomial and one point per opening
  (d) kzgx_ntt_device alone at log2 n = 12, 16, 20 over the same number of
      scalars, as achieved bytes/s against a memory-bound schedule of one read
      plus one write of the data per pass (one pass up to 2^KZGX_NTT_TILE_LOG2,
      two above).
Device events around the enqueue on one stream; each pair's two legs alternate
inside one loop after a warm-up of both, median / min / max of --reps rounds.
The results of the two legs of a pair are compared bit for bit.

    python scripts/bench_evals.py [--out profiles/ntt_evals.json]
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kzg-commitments_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))  # tau only


def stats(ms):
    return {"ms": statistics.median(ms), "ms_min_max": [min(ms), max(ms)]}


def timed_pair(fa, fb, reps, torch, st):
    """the two legs alternating, one event pair per call -> (stats a, stats b)"""
    for f in (fa, fb):  # warm-up: code objects, workspaces, the twiddle table
        f()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for f, acc in ((fa, ta), (fb, tb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            f()
            b.record(st)
            b.synchronize()
            acc.append(a.elapsed_time(b))
    return stats(ta), stats(tb)


def timed(fn, reps, torch, st):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return stats(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=12)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--srs", type=int, default=4097)
    ap.add_argument("--ntt-sizes", default="12,16,20")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_evals: no GPU (nothing is measured on a CPU)")
    import kzg_ref as K
    import kzgx

    C = K.BLS12381
    k, batch, reps = args.log2n, args.batch, max(args.reps, 9)
    n = 1 << k
    dev = torch.device("cuda", 0)
    ctx = kzgx.Context("BLS12381")
    ctx.gen_srs(K.default_tau(C), args.srs)  # with the default table
    tc, tn, tb = ctx.default_table_info()
    st = torch.cuda.Stream(device=dev)
    sh = st.cuda_stream

    # canonical scalars: 254 random bits each (r is a 255-bit prime)
    rng = np.random.default_rng(0xE7A15)
    total = batch * n
    ev = rng.integers(0, 1 << 63, size=(total, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(
        0, 2, size=(total, 4), dtype=np.uint64)
    ev[:, 3] &= np.uint64((1 << 62) - 1)
    d_ev = torch.from_numpy(ev.view(np.int64)).to(dev)
    d_co = torch.empty_like(d_ev)
    zs = rng.integers(0, 1 << 62, size=(batch, 4), dtype=np.uint64)
    d_z = torch.from_numpy(zs.view(np.int64)).to(dev)
    w = 2 * ctx.w64
    outs = [torch.zeros((batch, w), dtype=torch.int64, device=dev) for _ in range(2)]
    infs = [torch.zeros((batch,), dtype=torch.int32, device=dev) for _ in range(2)]
    ys = [torch.zeros((batch, 4), dtype=torch.int64, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    # the same polynomials in coefficient form, for the existing paths
    ctx.ntt_device(d_ev.data_ptr(), n, d_co.data_ptr(), n, k, batch, inverse=True, stream=sh)
    st.synchronize()

    res = {"metric": "evaluation-form commits / openings against the coefficient-form paths; bare Fr NTT",
           "timing": "device events around the enqueue, legs of a pair alternating in one loop, median of %d "
                     "after one warm-up of each" % reps,
           "device": torch.cuda.get_device_name(0), "curve": "BLS12381", "log2n": k, "batch": batch,
           "srs_points": args.srs, "default_table": {"c": tc, "points": tn, "bytes": tb},
           "ntt_tile_log2": kzgx.NTT_TILE_LOG2}

    # (a) / (b)
    a, b = timed_pair(
        lambda: ctx.commit_evals_device(d_ev.data_ptr(), k, batch, n, outs[0].data_ptr(), infs[0].data_ptr(), stream=sh),
        lambda: ctx.msm_batch_device(d_co.data_ptr(), n, batch, n, outs[1].data_ptr(), infs[1].data_ptr(), sh),
        reps, torch, st)
    res["commit"] = {"commit_evals_device": a, "msm_batch_device": b, "ratio": a["ms"] / b["ms"],
                     "commits_per_s_evals": batch / a["ms"] * 1e3, "commits_per_s_coeffs": batch / b["ms"] * 1e3,
                     "bit_exact": bool(torch.equal(outs[0], outs[1]) and torch.equal(infs[0], infs[1]))}
    # (c)
    a, b = timed_pair(
        lambda: ctx.prove_evals_device(d_ev.data_ptr(), k, n, d_z.data_ptr(), batch, outs[0].data_ptr(),
                                       infs[0].data_ptr(), ys[0].data_ptr(), stream=sh),
        lambda: ctx.prove_single_batch_device(d_co.data_ptr(), n, n, d_z.data_ptr(), batch, outs[1].data_ptr(),
                                              infs[1].data_ptr(), ys[1].data_ptr(), sh),
        reps, torch, st)
    res["prove"] = {"prove_evals_device": a, "prove_single_batch_device": b, "ratio": a["ms"] / b["ms"],
                    "bit_exact": bool(torch.equal(outs[0], outs[1]) and torch.equal(infs[0], infs[1])
                                      and torch.equal(ys[0], ys[1]))}
    res["within_25_percent"] = bool(res["commit"]["ratio"] <= 1.25 and 0.75 <= res["prove"]["ratio"] <= 1.25)

    # (d) the same 2^(log2n) x batch scalars as fewer, longer transforms
    res["ntt_device"] = {}
    for kk in [int(x) for x in args.ntt_sizes.split(",")]:
        bb = max(1, total >> kk)
        nbytes = (bb << kk) * 32
        passes = 1 if kk <= kzgx.NTT_TILE_LOG2 else 2
        row = {"batch": bb, "bytes": nbytes, "passes": passes}
        for tag, inv, br in (("forward", False, False), ("inverse", True, False), ("inverse_bitrev", True, True)):
            t = timed(lambda: ctx.ntt_device(d_ev.data_ptr(), 1 << kk, d_co.data_ptr(), 1 << kk, kk, bb, inv, br, sh),
                      reps, torch, st)
            t["achieved_bytes_per_s"] = passes * 2 * nbytes / (t["ms"] * 1e-3)
            row[tag] = t
        res["ntt_device"][str(kk)] = row
    # the round trip at the flagship size, as a check of what was timed
    ctx.ntt_device(d_ev.data_ptr(), n, d_co.data_ptr(), n, k, batch, stream=sh)
    ctx.ntt_device(d_co.data_ptr(), n, d_co.data_ptr(), n, k, batch, inverse=True, stream=sh)
    st.synchronize()
    res["round_trip_exact"] = bool(torch.equal(d_co, d_ev))
    ctx.close()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
