#!/usr/bin/env python3
"""Per-cell verdicts (kzgx_verify_cells_each_device: one boolean per cell of a batch) against the two
routes that existed before it, on one MI355X, in one process:
  - one kzgx_verify_proof call per cell, the only way to learn WHICH cell failed;
  - kzgx_verify_cells_aggregate_device on the same batch, which answers with one bit.

BLS12-381, 4097 G1 points and 65 G2 points; the data-availability shape (log2n, log2l) = (12, 6),
extended and bit-reversed: 128 cells of 64 values per blob.  Cells, proofs and commitments come from
kzgx_prove_cosets_batch_device and kzgx_commit_evals_batch and are passed on as they come.
  count = 128 (one blob), 1024 and 8192 (64 blobs), device pointers.
  The device calls are timed with device events around the enqueue on one stream.
  kzgx_verify_proof has host pointers only and blocks, so it is timed on the HOST WALL CLOCK (the stream
  drained before and after) over --sample cells spread over the batch and SCALED to the count; it includes
  its own staging copies, which is what a caller pays.
  The contenders alternate inside one loop after a warm-up of each; median / min / max of --reps.
  Contenders: the new call on a context with the default table, the same with the wave-per-opening
  pairing kernel forced off (kzgx_set_verify_wave_max(0)), the new call on a context built with
  kzgx_set_default_table(0), the aggregate, and the per-cell loop.
  Every timed batch is first checked: all true when valid, false at exactly the tampered cell otherwise.
  The stage breakdown comes from the library's own event spans (kzgx_prof_read) in a run of its own.

    python scripts/bench_verify_cells_each.py [--out profiles/verify_cells_each.json]
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

SPANS = ("cells_intt", "cells_coeffs", "cells_msm", "cells_sub", "verify_wave", "verify_single")


def stats(ms):
    return {"ms": statistics.median(ms), "ms_min_max": [min(ms), max(ms)]}


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--counts", default="128,1024,8192")
    ap.add_argument("--sample", type=int, default=64, help="cells per round of the per-cell baseline")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_verify_cells_each: no GPU (nothing is measured on a CPU)")
    import kzg_ref as K
    import kzgx

    C = K.BLS12381
    reps = max(args.reps, 5)
    counts = [int(x) for x in args.counts.split(",") if x]
    dev = torch.device("cuda", 0)
    tau = K.default_tau(C)
    ctx = kzgx.Context("BLS12381")
    ctx.gen_srs(tau, 4097)  # with the default table
    ctx.gen_srs_g2(tau, 65)
    bare = kzgx.Context("BLS12381")  # no default table: the MSM of the interpolants runs the Pippenger
    bare.set_default_table(0)
    bare.gen_srs(tau, 64)
    bare.gen_srs_g2(tau, 65)
    tc, tn, tb = ctx.default_table_info()
    st = torch.cuda.Stream(device=dev)
    sh = st.cuda_stream
    w = 2 * ctx.w64
    rng = np.random.default_rng(0xCE11E)
    k, kl, R, l, n = 12, 6, 128, 64, 4096
    blobs = (max(counts) + R - 1) // R

    def scalars(count, bits=254):
        v = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(
            0, 2, size=(count, 4), dtype=np.uint64)
        if bits == 128:
            v[:, 2:] = 0
        else:
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

    def alternate(legs):
        """legs: {name: (fn, timer)}; one warm-up of each, then reps rounds in which every leg runs once"""
        for fn, _ in legs.values():
            fn()
        torch.cuda.synchronize()
        xs = {name: [] for name in legs}
        for _ in range(reps):
            for name, (fn, timer) in legs.items():
                xs[name].append(timer(fn))
        return {name: stats(v) for name, v in xs.items()}

    # ---- the producer side: blobs -> commitments, cell proofs, cell values ---------------------------
    blob = ctx.ntt(scalars(blobs * n).reshape(blobs, n, 4), bitrev=True)
    commits, commit_inf = ctx.commit_evals(blob, bitrev=True)
    proofs, proof_inf, ys = ctx.prove_cosets(blob, kl, extended=True, evals=True, bitrev=True)
    proofs, ys = proofs.reshape(blobs * R, w), ys.reshape(blobs * R, l, 4)
    proof_inf = proof_inf.reshape(-1)
    xs = [kzgx.coset_points("BLS12381", k, kl, p, extended=True, bitrev=True) for p in range(R)]
    ci = np.repeat(np.arange(blobs, dtype=np.uint32), R)
    idx = np.tile(np.arange(R, dtype=np.uint32), blobs)
    ch = scalars(blobs * R, bits=128)
    ch[0] = (1, 0, 0, 0)

    def to_dev(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)

    d_c, d_p, d_y, d_r = (to_dev(a, np.int64) for a in (commits, proofs, ys, ch))
    d_ci, d_idx = to_dev(ci, np.int32), to_dev(idx, np.int32)
    d_cf = to_dev(commit_inf.astype(np.uint32), np.int32)
    d_pf = to_dev(proof_inf.astype(np.uint32), np.int32)
    d_bad = d_y.clone()
    d_oks = torch.zeros((max(counts),), dtype=torch.int32, device=dev)
    d_ok1 = torch.zeros((2,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    res = {"metric": "count verdicts from one call (kzgx_verify_cells_each_device) against one kzgx_verify_proof "
                     "call per cell and against the one-bit kzgx_verify_cells_aggregate_device",
           "timing": "device calls: device events around the enqueue; kzgx_verify_proof (host pointers, blocking): "
                     "host wall clock with the stream drained before and after, over a sample of cells SCALED to "
                     "the count; contenders alternating in one loop, median [min, max] of %d after one warm-up of "
                     "each" % reps,
           "device": torch.cuda.get_device_name(0), "curve": "BLS12381", "srs_points": [4097, 65],
           "default_table": {"c": tc, "points": tn, "bytes": tb},
           "shape": {"log2n": k, "log2l": kl, "extended": True, "bit_reversed": True}, "cases": {}}

    def head(count):
        nb = (count + R - 1) // R
        return (d_c.data_ptr(), d_cf.data_ptr(), nb, d_ci.data_ptr(), d_idx.data_ptr(), d_p.data_ptr(), d_pf.data_ptr())

    def each_call(c, count, d_vals, ok=None):
        o = (d_oks if ok is None else ok).data_ptr()
        c.verify_cells_each_device(*head(count), d_vals.data_ptr(), count, k, kl, o, extended=True, bitrev=True,
                                   stream=sh)

    def agg_call(count):
        ctx.verify_cells_aggregate_device(*head(count), d_y.data_ptr(), d_r.data_ptr(), count, k, kl, d_ok1.data_ptr(),
                                          extended=True, bitrev=True, stream=sh)

    def answers(c, count):
        """the valid batch is all true; one changed value of the middle cell makes exactly that cell false"""
        bad_cell = count // 2
        d_bad.copy_(d_y)
        d_bad[bad_cell, 7, 0] += 1
        good = torch.full((count,), 7, dtype=torch.int32, device=dev)
        bad = torch.full((count,), 7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        each_call(c, count, d_y, good)
        each_call(c, count, d_bad, bad)
        st.synchronize()
        return bool((good == 1).all()) and [i for i, v in enumerate(bad.tolist()) if v != 1] == [bad_cell], bad_cell

    for count in counts:
        sample = sorted(set(np.linspace(0, count - 1, min(args.sample, count)).astype(int).tolist()))
        ok_wave, bad_cell = answers(ctx, count)
        ctx.set_verify_wave_max(0)
        ok_lane, _ = answers(ctx, count)
        ctx.set_verify_wave_max(8192)
        ok_bare, _ = answers(bare, count)
        bad_ys = ys[bad_cell].copy()
        bad_ys[7, 0] += np.uint64(1)

        def per_cell(j, vals=None):
            return ctx.verify_proof(commits[ci[j]], bool(commit_inf[ci[j]]), proofs[j], bool(proof_inf[j]),
                                    xs[idx[j]], ys[j] if vals is None else vals)

        base_ok = all(per_cell(j) for j in sample) and per_cell(bad_cell, bad_ys) is False
        note("count %d: verdicts right (wave, lane, no table) = %s, per-cell sample ok %s"
             % (count, [ok_wave, ok_lane, ok_bare], base_ok))

        def lane():
            ctx.set_verify_wave_max(0)
            each_call(ctx, count, d_y)
            ctx.set_verify_wave_max(8192)

        def old():
            for j in sample:
                per_cell(j)

        t = alternate({"each": (lambda: each_call(ctx, count, d_y), event_ms), "each_lane_path": (lane, event_ms),
                       "each_no_default_table": (lambda: each_call(bare, count, d_y), event_ms),
                       "aggregate": (lambda: agg_call(count), event_ms), "per_cell": (old, wall_ms)})
        scale = count / len(sample)
        b = t["per_cell"]
        b_scaled = {"ms": b["ms"] * scale, "ms_min_max": [v * scale for v in b["ms_min_max"]],
                    "sampled_cells": len(sample), "ms_per_call": b["ms"] / len(sample), "scaled": True}
        best = min(t["each"]["ms"], t["each_lane_path"]["ms"])
        res["cases"]["count %d" % count] = {
            "count": count, "commitments": (count + R - 1) // R,
            "verify_cells_each_device": t["each"],
            "verify_cells_each_device_wave_max_0": t["each_lane_path"],
            "verify_cells_each_device_default_table_0": t["each_no_default_table"],
            "verify_cells_aggregate_device": t["aggregate"],
            "verify_proof_per_cell_host_wall": b_scaled,
            "speedup_over_per_cell": b_scaled["ms"] / t["each"]["ms"],
            "cost_over_aggregate": t["each"]["ms"] / t["aggregate"]["ms"],
            "faster_pairing_path": "wave" if t["each"]["ms"] <= t["each_lane_path"]["ms"] else "lane",
            "best_path_ms": best,
            "verdicts_right": bool(ok_wave and ok_lane and ok_bare and base_ok),
            "cells_per_s": count / t["each"]["ms"] * 1e3}
        note(json.dumps(res["cases"]["count %d" % count]))

    per_call = statistics.median(c["verify_proof_per_cell_host_wall"]["ms_per_call"] for c in res["cases"].values())
    res["verify_proof_ms_per_call"] = per_call

    # ---- one and two cells: the separate calls are expected to win -------------------------------------
    small = {}
    for count in (1, 2):
        def old_small():
            for j in range(count):
                ctx.verify_proof(commits[ci[j]], bool(commit_inf[ci[j]]), proofs[j], bool(proof_inf[j]), xs[idx[j]],
                                 ys[j])

        t = alternate({"each": (lambda: each_call(ctx, count, d_y), event_ms), "per_cell": (old_small, wall_ms)})
        small["count %d" % count] = {"verify_cells_each_device": t["each"],
                                     "verify_proof_per_cell_host_wall": t["per_cell"],
                                     "each_is_slower": t["each"]["ms"] > t["per_cell"]["ms"]}
        note(json.dumps(small["count %d" % count]))
    res["small_counts"] = small
    res["separate_calls_win_below_count"] = small["count 1"]["verify_cells_each_device"]["ms"] / per_call

    # ---- said plainly: every count at which the new call (as it runs by default) loses ----------------
    loses = []
    for c in res["cases"].values():
        mine = c["verify_cells_each_device"]["ms"]
        for other in ("verify_proof_per_cell_host_wall", "verify_cells_aggregate_device",
                      "verify_cells_each_device_wave_max_0"):
            if c[other]["ms"] < mine:
                loses.append({"count": c["count"], "to": other, "ms": [mine, c[other]["ms"]],
                              "ratio": mine / c[other]["ms"]})
    for name, c in small.items():
        if c["each_is_slower"]:
            loses.append({"count": int(name.split()[1]), "to": "verify_proof_per_cell_host_wall",
                          "ms": [c["verify_cells_each_device"]["ms"], c["verify_proof_per_cell_host_wall"]["ms"]],
                          "ratio": c["verify_cells_each_device"]["ms"] / c["verify_proof_per_cell_host_wall"]["ms"]})
    res["loses"] = loses
    note("loses:", json.dumps(loses))

    # ---- where the time goes: the library's own spans, a run of its own ----------------------------
    shares = {}
    for label, c, vw in (("default", ctx, 8192), ("wave_max_0", ctx, 0), ("default_table_0", bare, 8192)):
        for count in counts:
            c.set_verify_wave_max(vw)
            each_call(c, count, d_y)
            st.synchronize()
            c.prof_clear()
            c.prof_enable(True)
            total = event_ms(lambda: each_call(c, count, d_y))
            spans = {name: c.prof_read(name)[0] for name in SPANS}
            c.prof_enable(False)
            c.prof_clear()
            c.set_verify_wave_max(8192)
            shares["%s, count %d" % (label, count)] = {
                "call_ms_with_spans": total,
                "spans_ms": {"transform_and_scalars": spans["cells_intt"] + spans["cells_coeffs"],
                             "msm": spans["cells_msm"], "subtraction": spans["cells_sub"],
                             "pairing_kernel": spans["verify_wave"] + spans["verify_single"]},
                "pairing_share": (spans["verify_wave"] + spans["verify_single"]) / total}
            note(label, count, json.dumps(shares["%s, count %d" % (label, count)]))
    res["stages"] = shares
    ctx.close()
    bare.close()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
