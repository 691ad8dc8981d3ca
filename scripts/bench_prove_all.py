#!/usr/bin/env python3
"""All-domain openings (kzgx_prove_all_batch_device, FK20 over the G1 NTT) against
the path that existed before them -- kzgx_prove_evals_batch_device with
eval_stride == 0 and zs = the whole domain, n openings of n-point MSMs -- and the
bare G1 NTT, on one MI355X, in one process.

BLS12-381, an SRS of 2^16 + 1 points with the default table (which serves the
baseline's MSMs at n = 2^12; above it they run the batched Pippenger).  Both legs
take the polynomial's evaluations and produce the n proofs and the n values:
  n = 2^12, 1 polynomial      both legs
  n = 2^12, 32 polynomials    both legs (the baseline leg is 32 calls)
  n = 2^14, 1 polynomial      both legs
  n = 2^16, 1 polynomial      the new path; the baseline as 16 x the measured 2^14 time, an extrapolation
  kzgx_g1_ntt_device of 2^13 points at batch 1 and batch 32
  kzgx_prove_all_prepare, the one-off setup per size (host wall clock around the blocking call)
Device events around the enqueue on one stream; the two legs alternate inside one
loop after a warm-up of both, median / min / max of --reps rounds.  The legs'
proofs are compared bit for bit.

    python scripts/bench_prove_all.py [--out profiles/prove_all.json]
Prints one JSON line (and writes it to --out)."""
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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--skip-2p14-baseline", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_prove_all: no GPU (nothing is measured on a CPU)")
    import kzg_ref as K
    import kzgx

    C = K.BLS12381
    reps, nb = max(args.reps, 9), args.batch
    dev = torch.device("cuda", 0)
    ctx = kzgx.Context("BLS12381")
    ctx.gen_srs(K.default_tau(C), (1 << 16) + 1)  # with the default table
    tc, tn, tb = ctx.default_table_info()
    st = torch.cuda.Stream(device=dev)
    sh = st.cuda_stream
    w = 2 * ctx.w64

    # canonical scalars: 254 random bits each (r is a 255-bit prime)
    rng = np.random.default_rng(0xF4B20)

    def scalars(count):
        v = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(
            0, 2, size=(count, 4), dtype=np.uint64)
        v[:, 3] &= np.uint64((1 << 62) - 1)
        return torch.from_numpy(v.view(np.int64)).to(dev)

    def domain(k):
        r, wk = C.r, kzgx.domain_root("BLS12381", k)
        z, out = 1, []
        for _ in range(1 << k):
            out.append(z)
            z = z * wk % r
        raw = b"".join(v.to_bytes(32, "little") for v in out)
        return torch.from_numpy(np.frombuffer(raw, dtype=np.int64).reshape(-1, 4).copy()).to(dev)

    res = {"metric": "all-domain openings (FK20) against n single openings over the domain; bare G1 NTT",
           "timing": "device events around the enqueue, legs of a pair alternating in one loop, median of %d "
                     "after one warm-up of each" % reps,
           "device": torch.cuda.get_device_name(0), "curve": "BLS12381", "srs_points": (1 << 16) + 1,
           "default_table": {"c": tc, "points": tn, "bytes": tb}, "chunk_points": kzgx.G1_NTT_CHUNK_POINTS,
           "prepare_ms": {}, "cases": {}}

    def prepare(k):
        ctx.sync()
        t0 = time.perf_counter()
        ctx.prove_all_prepare(k)
        res["prepare_ms"][str(k)] = (time.perf_counter() - t0) * 1e3

    def case(k, batch, baseline):
        n = 1 << k
        d_ev = scalars(batch * n)
        outs = [torch.zeros((batch * n, w), dtype=torch.int64, device=dev) for _ in range(2)]
        infs = [torch.zeros((batch * n,), dtype=torch.int32, device=dev) for _ in range(2)]
        ys = [torch.zeros((batch * n, 4), dtype=torch.int64, device=dev) for _ in range(2)]
        torch.cuda.synchronize()

        def new():
            ctx.prove_all_device(d_ev.data_ptr(), k, batch, n, outs[0].data_ptr(), infs[0].data_ptr(),
                                 ys[0].data_ptr(), evals=True, stream=sh)

        row = {"log2n": k, "polynomials": batch}
        if not baseline:
            row["prove_all_device"] = timed(new, reps, torch, st)
        else:
            d_z = domain(k)

            def old():
                for b in range(batch):
                    ctx.prove_evals_device(d_ev.data_ptr() + b * n * 32, k, 0, d_z.data_ptr(), n,
                                           outs[1].data_ptr() + b * n * w * 8, infs[1].data_ptr() + b * n * 4,
                                           ys[1].data_ptr() + b * n * 32, stream=sh)

            a, b = timed_pair(new, old, reps, torch, st)
            row.update({"prove_all_device": a, "prove_evals_device_over_the_domain": b,
                        "speedup": b["ms"] / a["ms"],
                        "bit_exact": bool(torch.equal(outs[0], outs[1]) and torch.equal(infs[0], infs[1])
                                          and torch.equal(ys[0], ys[1]))})
        row["proofs_per_s"] = batch * n / row["prove_all_device"]["ms"] * 1e3
        res["cases"]["2^%d x %d" % (k, batch)] = row
        return row

    prepare(12)
    case(12, 1, True)
    case(12, nb, True)
    prepare(14)
    r14 = case(14, 1, not args.skip_2p14_baseline)
    prepare(16)
    r16 = case(16, 1, False)
    if "prove_evals_device_over_the_domain" in r14:
        ext = 16 * r14["prove_evals_device_over_the_domain"]["ms"]
        r16["baseline_extrapolated_ms"] = ext
        r16["baseline_note"] = "16 x the measured 2^14 baseline (n^2 scaling), an extrapolation, not a measurement"
        r16["speedup_extrapolated"] = ext / r16["prove_all_device"]["ms"]

    # the bare G1 NTT of 2^13 points (the size of the 2^12 openings' inverse transform)
    res["g1_ntt_device"] = {}
    k = 13
    for batch in (1, nb):
        cnt = batch << k
        # points: the SRS itself, repeated (any on-curve points do)
        srs = torch.from_numpy(ctx.get_srs(1 << k).view(np.int64)).to(dev)
        d_p = srs.repeat(batch, 1).contiguous()
        d_o = torch.zeros_like(d_p)
        d_f = torch.zeros((cnt,), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        row = {"points": cnt}
        for tag, inv in (("forward", False), ("inverse", True)):
            row[tag] = timed(lambda: ctx.g1_ntt_device(d_p.data_ptr(), None, d_o.data_ptr(), d_f.data_ptr(), k, batch,
                                                        inverse=inv, stream=sh), reps, torch, st)
        res["g1_ntt_device"]["2^%d x %d" % (k, batch)] = row
    ctx.close()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
