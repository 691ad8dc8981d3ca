#!/usr/bin/env python3
"""Aggregated cell verification (kzgx_verify_cells_aggregate_device: one pairing check for many
coset openings) against the path that existed before it -- one kzgx_verify_proof call per cell --
on one MI355X, in one process.

BLS12-381, 4097 G1 points (with the default table, which serves the baseline's MSMs) and 65 G2
points; the data-availability shape (log2n, log2l) = (12, 6), extended and bit-reversed: 128 cells
of 64 values per blob.  Cells, proofs and commitments come from kzgx_prove_cosets_batch_device and
kzgx_commit_evals_batch, and are passed to the verifier as they come.
  count = 128 (one blob), 1024 and 8192 (64 blobs), explicit 128-bit challenges.
  The new leg is timed with device events around the enqueue on one stream.
  kzgx_verify_proof has host pointers only and blocks, so the baseline is timed on the HOST WALL
  CLOCK (the stream drained before and after) over --sample cells spread over the batch and scaled
  to the count; it includes its own staging copies, which is what a caller of the parent commit
  pays.  The legs alternate inside one loop after a warm-up of both, median / min / max of --reps.
  Every timed batch is first checked to give true, and false with one value tampered.
  At 8192 the checked form (subgroup test on) runs against the unchecked one the same way.
  The share of the fold kernels comes from the library's own event spans (kzgx_prof_read) in a
  run of its own, and that of the batched inverse NTT from device events around kzgx_ntt_device.

    python scripts/bench_verify_cells.py [--out profiles/verify_cells.json]
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
    ap.add_argument("--counts", default="128,1024,8192")
    ap.add_argument("--sample", type=int, default=128, help="cells per round of the per-cell baseline")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_verify_cells: no GPU (nothing is measured on a CPU)")
    import kzg_ref as K
    import kzgx

    C = K.BLS12381
    reps = max(args.reps, 9)
    counts = [int(x) for x in args.counts.split(",") if x]
    dev = torch.device("cuda", 0)
    ctx = kzgx.Context("BLS12381")
    tau = K.default_tau(C)
    ctx.gen_srs(tau, 4097)  # with the default table
    ctx.gen_srs_g2(tau, 65)
    tc, tn, tb = ctx.default_table_info()
    st = torch.cuda.Stream(device=dev)
    sh = st.cuda_stream
    w = 2 * ctx.w64
    rng = np.random.default_rng(0xCE115)
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

    def alternate(fa, ta, fb, tb):
        fa()
        fb()
        torch.cuda.synchronize()
        xa, xb = [], []
        for _ in range(reps):
            xa.append(ta(fa))
            xb.append(tb(fb))
        return stats(xa), stats(xb)

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
    d_ok = torch.zeros((2,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    res = {"metric": "one pairing check for count cells (kzgx_verify_cells_aggregate_device) against one "
                     "kzgx_verify_proof call per cell",
           "timing": "new path: device events around the enqueue; kzgx_verify_proof (host pointers, blocking): host "
                     "wall clock with the stream drained before and after, over a sample of cells scaled to the "
                     "count; legs alternating in one loop, median of %d after one warm-up of each" % reps,
           "device": torch.cuda.get_device_name(0), "curve": "BLS12381", "srs_points": [4097, 65],
           "default_table": {"c": tc, "points": tn, "bytes": tb}, "shape": {"log2n": k, "log2l": kl, "extended": True,
                                                                             "bit_reversed": True},
           "cases": {}}

    def new_call(count, d_vals, checked=None, ok=None):
        nb = (count + R - 1) // R
        a = (d_c.data_ptr(), d_cf.data_ptr(), nb, d_ci.data_ptr(), d_idx.data_ptr(), d_p.data_ptr(), d_pf.data_ptr(),
             d_vals.data_ptr(), d_r.data_ptr(), count, k, kl)
        o = (d_ok if ok is None else ok).data_ptr()
        if checked is None:
            ctx.verify_cells_aggregate_device(*a, o, extended=True, bitrev=True, stream=sh)
        else:
            ctx.verify_cells_aggregate_checked_device(*a, checked, o, extended=True, bitrev=True, stream=sh)

    def answers(count, checked=None):
        """(valid batch, the batch with one value of its middle cell changed)"""
        bad_cell = count // 2
        d_bad.copy_(d_y)
        d_bad[bad_cell, 7, 0] += 1
        oks = torch.full((2,), 7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        new_call(count, d_y, checked, oks[0:])
        new_call(count, d_bad, checked, oks[1:])
        st.synchronize()
        return [int(v) for v in oks.tolist()], bad_cell

    for count in counts:
        sample = sorted(set(np.linspace(0, count - 1, min(args.sample, count)).astype(int).tolist()))
        got, bad_cell = answers(count)
        bad_ys = ys[bad_cell].copy()
        bad_ys[7, 0] += np.uint64(1)

        def per_cell(j, vals=None):
            return ctx.verify_proof(commits[ci[j]], bool(commit_inf[ci[j]]), proofs[j], bool(proof_inf[j]),
                                    xs[idx[j]], ys[j] if vals is None else vals)

        base_ok = all(per_cell(j) for j in sample) and per_cell(bad_cell, bad_ys) is False
        note("count %d: aggregate (valid, tampered) = %s, per-cell sample ok %s" % (count, got, base_ok))

        def new():
            new_call(count, d_y)

        def old():
            for j in sample:
                per_cell(j)

        a, b = alternate(new, event_ms, old, wall_ms)
        scale = count / len(sample)
        b_scaled = {"ms": b["ms"] * scale, "ms_min_max": [v * scale for v in b["ms_min_max"]],
                    "sampled_cells": len(sample), "ms_per_call": b["ms"] / len(sample)}
        res["cases"]["count %d" % count] = {
            "count": count, "commitments": (count + R - 1) // R, "verify_cells_aggregate_device": a,
            "verify_proof_per_cell_host_wall": b_scaled, "speedup": b_scaled["ms"] / a["ms"],
            "valid_true_tampered_false": got == [1, 0] and base_ok, "cells_per_s": count / a["ms"] * 1e3}
        note(json.dumps(res["cases"]["count %d" % count]))

    # the count below which the separate calls win: t_new(count) against count * t_call
    per_call = statistics.median(c["verify_proof_per_cell_host_wall"]["ms_per_call"] for c in res["cases"].values())
    smallest = res["cases"]["count %d" % min(counts)]
    res["verify_proof_ms_per_call"] = per_call
    res["separate_calls_win_below_count"] = smallest["verify_cells_aggregate_device"]["ms"] / per_call

    # ---- the checked form at the largest count ---------------------------------------------------------
    count = max(counts)
    got, _ = answers(count, checked=True)
    a, b = alternate(lambda: new_call(count, d_y, True), event_ms, lambda: new_call(count, d_y), event_ms)
    res["checked"] = {"count": count, "subgroup": True, "verify_cells_aggregate_checked_device": a,
                      "verify_cells_aggregate_device": b, "ratio": a["ms"] / b["ms"],
                      "valid_true_tampered_false": got == [1, 0]}
    note(json.dumps(res["checked"]))

    # ---- where the time goes: the library's own spans, a run of its own ----------------------------
    shares = {}
    for count in counts:
        d_t = torch.zeros((count * l, 4), dtype=torch.int64, device=dev)
        ntt_ms = statistics.median(event_ms(lambda: ctx.ntt_device(d_y.data_ptr(), l, d_t.data_ptr(), l, kl, count,
                                                                   inverse=True, bitrev=True, stream=sh))
                                   for _ in range(reps))
        ctx.prof_clear()
        ctx.prof_enable(True)
        total = event_ms(lambda: new_call(count, d_y))
        spans = {name: ctx.prof_read(name)[0] for name in ("cells_scalars", "var_sort", "var_accum", "var_reduce",
                                                            "var_horner", "pair2_wave")}
        ctx.prof_enable(False)
        ctx.prof_clear()
        shares["count %d" % count] = {"call_ms_with_spans": total, "inverse_ntt_ms": ntt_ms, "spans_ms": spans,
                                      "fold_share": spans["cells_scalars"] / total,
                                      "inverse_ntt_share": ntt_ms / total}
        note(json.dumps(shares["count %d" % count]))
    res["shares"] = shares
    ctx.close()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
