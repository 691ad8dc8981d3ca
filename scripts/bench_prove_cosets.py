#!/usr/bin/env python3
"""Coset (cell) openings (kzgx_prove_cosets_batch_device, the multi-point FK20) against
the path that existed before them -- one kzgx_prove_range call per coset, R calls per
polynomial -- and, at cosets of one point, against kzgx_prove_all_batch_device, on one
MI355X, in one process.

BLS12-381, an SRS of 4097 points with the default table (which serves the baseline's
n-point MSMs).
  (log2n, log2l) = (12, 6) extended, bit-reversed, evaluation input: 128 cells of 64 values per
      polynomial, at each batch of --batches (1, 8, 64).  The new leg produces the proofs
      and the 8192 values; the baseline takes the coefficients and produces the proofs only.
  (12, 0) natural order, coefficient input, at batch 1 and 8: the same work as
      kzgx_prove_all_batch_device, which is the other leg.
  kzgx_prove_cosets_prepare of both shapes (host wall clock around the blocking call)
The new path and prove_all are timed with device events around the enqueue on one
stream.  kzgx_prove_range has host pointers only and blocks, so the baseline is timed on
the HOST WALL CLOCK (the stream drained before and after); it includes its own staging
copies, which is what a caller of the parent commit pays.  The two legs alternate inside
one loop after a warm-up of both, median / min / max of --reps rounds.  Every measured
pair is compared bit for bit before it is timed.

    python scripts/bench_prove_cosets.py [--out profiles/prove_cosets.json]
Prints one JSON line (and writes it to --out); progress goes to stderr."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kzg-commitments_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))  # tau only


def stats(ms):
    return {"ms": statistics.median(ms), "ms_min_max": [min(ms), max(ms)]}


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_prove_cosets: no GPU (nothing is measured on a CPU)")
    import kzg_ref as K
    import kzgx

    C = K.BLS12381
    reps = max(args.reps, 9)
    dev = torch.device("cuda", 0)
    ctx = kzgx.Context("BLS12381")
    ctx.gen_srs(K.default_tau(C), 4097)  # with the default table
    tc, tn, tb = ctx.default_table_info()
    st = torch.cuda.Stream(device=dev)
    sh = st.cuda_stream
    w = 2 * ctx.w64
    rng = np.random.default_rng(0xC05E7)

    def scalars(count):  # canonical: 254 random bits each (r is a 255-bit prime)
        v = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(
            0, 2, size=(count, 4), dtype=np.uint64)
        v[:, 3] &= np.uint64((1 << 62) - 1)
        return v

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        return a.elapsed_time(b)

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3

    def alternate(fa, ta, fb, tb):
        """warm-up of both, then the legs alternating -> (stats a, stats b)"""
        fa()
        fb()
        torch.cuda.synchronize()
        xa, xb = [], []
        for _ in range(reps):
            xa.append(ta(fa))
            xb.append(tb(fb))
        return stats(xa), stats(xb)

    res = {"metric": "coset openings (multi-point FK20) against one kzgx_prove_range call per coset; cosets of one "
                     "point against kzgx_prove_all_batch_device",
           "timing": "new path and prove_all: device events around the enqueue; kzgx_prove_range (host pointers, "
                     "blocking): host wall clock with the stream drained before and after; legs of a pair "
                     "alternating in one loop, median of %d after one warm-up of each" % reps,
           "device": torch.cuda.get_device_name(0), "curve": "BLS12381", "srs_points": 4097,
           "default_table": {"c": tc, "points": tn, "bytes": tb}, "chunk_points": kzgx.G1_NTT_CHUNK_POINTS,
           "prepare_ms": {}, "cases": {}}

    def prepare(k, kl):
        ctx.sync()
        t0 = time.perf_counter()
        ctx.prove_cosets_prepare(k, kl)
        res["prepare_ms"]["(%d,%d)" % (k, kl)] = (time.perf_counter() - t0) * 1e3

    # ---- (12, 6) extended: the data-availability shape -----------------------------------------------
    k, kl = 12, 6
    n, R, l = 1 << k, 128, 64
    prepare(k, kl)
    cells = [kzgx.coset_points("BLS12381", k, kl, p, extended=True, bitrev=True) for p in range(R)]
    for batch in [int(x) for x in args.batches.split(",") if x]:
        coeffs = scalars(batch * n).reshape(batch, n, 4)
        blob = ctx.ntt(coeffs, bitrev=True)
        d_in = torch.from_numpy(blob.view(np.int64)).to(dev)
        d_out = torch.zeros((batch * R, w), dtype=torch.int64, device=dev)
        d_inf = torch.zeros((batch * R,), dtype=torch.int32, device=dev)
        d_y = torch.zeros((batch * R * l, 4), dtype=torch.int64, device=dev)
        ref = np.zeros((batch, R, w), dtype=np.uint64)
        ref_inf = np.zeros((batch, R), dtype=bool)
        torch.cuda.synchronize()

        def new():
            ctx.prove_cosets_device(d_in.data_ptr(), k, kl, batch, n, d_out.data_ptr(), d_inf.data_ptr(),
                                    d_y.data_ptr(), extended=True, evals=True, bitrev=True, stream=sh)

        def old():
            for b in range(batch):
                for p in range(R):
                    ref[b, p], ref_inf[b, p] = ctx.prove_range(coeffs[b], cells[p])

        new()
        old()
        torch.cuda.synchronize()
        same = bool((d_out.cpu().numpy().view(np.uint64).reshape(batch, R, w) == ref).all()
                    and (d_inf.cpu().numpy().reshape(batch, R).astype(bool) == ref_inf).all())
        note("(12,6) extended x %d: bit_exact %s" % (batch, same))
        a, b_ = alternate(new, event_ms, old, wall_ms)
        res["cases"]["(12,6) extended x %d" % batch] = {
            "log2n": k, "log2l": kl, "extended": True, "polynomials": batch, "proofs": batch * R,
            "prove_cosets_device": a, "prove_range_per_coset_host_wall": b_, "speedup": b_["ms"] / a["ms"],
            "bit_exact": same, "proofs_per_s": batch * R / a["ms"] * 1e3}
        note(json.dumps(res["cases"]["(12,6) extended x %d" % batch]))

    # ---- (12, 0): cosets of one point, the work of prove_all -----------------------------------------
    prepare(k, 0)
    ctx.prove_all_prepare(k)
    for batch in (1, 8):
        d_in = torch.from_numpy(scalars(batch * n).view(np.int64)).to(dev)
        outs = [torch.zeros((batch * n, w), dtype=torch.int64, device=dev) for _ in range(2)]
        infs = [torch.zeros((batch * n,), dtype=torch.int32, device=dev) for _ in range(2)]
        ys = [torch.zeros((batch * n, 4), dtype=torch.int64, device=dev) for _ in range(2)]
        torch.cuda.synchronize()

        def new1():
            ctx.prove_cosets_device(d_in.data_ptr(), k, 0, batch, n, outs[0].data_ptr(), infs[0].data_ptr(),
                                    ys[0].data_ptr(), stream=sh)

        def all1():
            ctx.prove_all_device(d_in.data_ptr(), k, batch, n, outs[1].data_ptr(), infs[1].data_ptr(),
                                 ys[1].data_ptr(), stream=sh)

        new1()
        all1()
        torch.cuda.synchronize()
        same = bool(torch.equal(outs[0], outs[1]) and torch.equal(infs[0], infs[1]) and torch.equal(ys[0], ys[1]))
        a, b_ = alternate(new1, event_ms, all1, event_ms)
        res["cases"]["(12,0) x %d" % batch] = {
            "log2n": k, "log2l": 0, "extended": False, "polynomials": batch, "proofs": batch * n,
            "prove_cosets_device": a, "prove_all_device": b_, "speedup": b_["ms"] / a["ms"], "bit_exact": same}
        note(json.dumps(res["cases"]["(12,0) x %d" % batch]))
    ctx.close()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
