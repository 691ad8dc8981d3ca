#!/usr/bin/env python3
"""Compressed points (kzgx_g1_decompress_batch_device, kzgx_g1_compress_batch_device,
kzgx_verify_cells_aggregate_bytes_device) on one MI355X, BLS12-381, ZCash
encoding, device pointers, in one process.

  (a) kzgx_g1_decompress_batch_device at 128, 1024 and 8192 + 64 records, without
      and with the subgroup test;
  (b) kzgx_g1_check_batch_device on the same points uncompressed: the yardstick of
      (a).  From the operation counts (a square root of ~476 field products beside
      a membership chain of ~1320) decompression with the test should cost about
      1.36x the test alone; the ratio is reported as measured;
  (c) kzgx_verify_cells_aggregate_bytes_device against
      kzgx_verify_cells_aggregate_checked_device at (12, 6) extended, bit-reversed,
      at 128, 1024 and 8192 cells, subgroup test on;
  (d) kzgx_g1_compress_batch_device of 8192 proofs.
Device events around the enqueue on a caller's stream; the legs of a comparison
alternate in one loop; medians of --reps after one warm-up of each.  Every timed
call's answer is checked: the recovered limbs equal the points that were
compressed, all flags are 1, one broken record makes the AND 0, the verify is
true on the honest cells and false with one value changed.

    python scripts/bench_point_codec.py [--out profiles/point_codec.json]
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kzg-commitments_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))  # the setup's tau only


def stats(ms):
    return {"ms": statistics.median(ms), "ms_min_max": [min(ms), max(ms)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="128,1024,8192")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace-leg", default="", choices=["", "bytes", "points"],
                    help="run only that leg of (c) at the largest count, --reps times, for a kernel trace "
                         "(rocprofv3 --kernel-trace --stats -- python scripts/bench_point_codec.py --trace-leg ...)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_point_codec: no GPU (nothing is measured on a CPU)")
    import kzg_ref as K
    import kzgx

    name, C, enc = "BLS12381", K.BLS12381, kzgx.ENC_ZCASH
    reps = max(args.reps, 1)
    counts = [int(x) for x in args.counts.split(",") if x]
    dev = torch.device("cuda", 0)
    ctx = kzgx.Context(name)
    tau = K.default_tau(C)
    ctx.gen_srs(tau, 4097)  # with the default table, as scripts/bench_verify_cells.py
    ctx.gen_srs_g2(tau, 65)
    st = torch.cuda.Stream(device=dev)
    sh = st.cuda_stream
    w = 2 * ctx.w64
    rng = np.random.default_rng(0xC0DEC)
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

    def alternate(*fns):
        for f in fns:
            f()
        torch.cuda.synchronize()
        xs = [[] for _ in fns]
        for _ in range(reps):
            for x, f in zip(xs, fns):
                x.append(event_ms(f))
        return [stats(x) for x in xs]

    def to_dev(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)

    # ---- the producer side: blobs -> commitments, cell proofs, cell values, all compressed on the device
    blob = ctx.ntt(scalars(blobs * n).reshape(blobs, n, 4), bitrev=True)
    commits, commit_inf = ctx.commit_evals(blob, bitrev=True)
    proofs, proof_inf, ys = ctx.prove_cosets(blob, kl, extended=True, evals=True, bitrev=True)
    proofs, ys = proofs.reshape(blobs * R, w), ys.reshape(blobs * R, l, 4)
    assert not proof_inf.any() and not np.asarray(commit_inf).any()
    ci = np.repeat(np.arange(blobs, dtype=np.uint32), R)
    idx = np.tile(np.arange(R, dtype=np.uint32), blobs)
    ch = scalars(blobs * R, bits=128)
    ch[0] = (1, 0, 0, 0)
    nmax = blobs * R
    pts = np.concatenate([proofs, commits])  # 8192 proofs + 64 commitments: the records of one verify
    npts = pts.shape[0]
    d_pts = to_dev(pts, np.int64)
    d_rec = torch.zeros((npts * 48,), dtype=torch.uint8, device=dev)
    d_xy = torch.zeros((npts, w), dtype=torch.int64, device=dev)
    d_inf = torch.zeros((npts,), dtype=torch.int32, device=dev)
    d_flags = torch.zeros((npts,), dtype=torch.int32, device=dev)
    d_all = torch.zeros((1,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.g1_compress_device(d_pts.data_ptr(), None, npts, enc, d_rec.data_ptr(), sh)
    st.synchronize()

    res = {"metric": "compressed G1 points: batched decompression against the point check of the same points, the "
                     "cell verify on records against the checked verify on points, compression",
           "timing": "device events around the enqueue on a caller's stream; the legs of a comparison alternate in "
                     "one loop; median of %d after one warm-up of each" % reps,
           "device": torch.cuda.get_device_name(0), "curve": name, "encoding": "KZGX_ENC_ZCASH",
           "expected_ratio_from_operation_counts": 1.36, "decompress": {}, "verify_cells": {}}

    # ---- (a), (b) ------------------------------------------------------------------------------------
    sizes = sorted(set(counts[:-1] + [max(counts) + blobs]))
    if args.trace_leg:
        sizes, counts = [], [max(counts)]
    for m in sizes:
        def dec(sg):
            ctx.g1_decompress_device(d_rec.data_ptr(), m, enc, sg, d_xy.data_ptr(), d_inf.data_ptr(),
                                     d_flags.data_ptr(), d_all.data_ptr(), sh)

        def chk(sg):
            ctx.g1_check_device(d_pts.data_ptr(), None, m, sg, d_flags.data_ptr(), d_all.data_ptr(), sh)

        t = alternate(lambda: dec(0), lambda: dec(1), lambda: chk(0), lambda: chk(1))
        # answers: the limbs come back, every flag is 1; one record without a root makes the AND 0
        d_xy.zero_()
        torch.cuda.synchronize()
        dec(1)
        st.synchronize()
        good = bool(d_all.item()) and bool(d_flags[:m].all().item()) and bool((d_xy[:m] == d_pts[:m]).all().item())
        d_one = d_rec.clone()
        d_one[(m // 3) * 48:(m // 3 + 1) * 48] = 0
        d_one[(m // 3) * 48] = 0x80
        d_one[(m // 3 + 1) * 48 - 1] = 1  # x = 1: x^3 + 4 = 5 is not a square
        torch.cuda.synchronize()
        ctx.g1_decompress_device(d_one.data_ptr(), m, enc, 1, d_xy.data_ptr(), d_inf.data_ptr(), d_flags.data_ptr(),
                                 d_all.data_ptr(), sh)
        st.synchronize()
        fl = d_flags[:m].cpu().numpy()
        good = good and not d_all.item() and int(fl.sum()) == m - 1 and not fl[m // 3]
        row = {"records": m, "decompress": t[0], "decompress_subgroup": t[1], "g1_check": t[2],
               "g1_check_subgroup": t[3], "checked": bool(good),
               "records_per_s_subgroup": m / t[1]["ms"] * 1e3,
               "decompress_subgroup_over_check_subgroup": t[1]["ms"] / t[3]["ms"],
               "decompress_over_check_curve_only": t[0]["ms"] / t[2]["ms"],
               "root_alone_over_check_subgroup": t[0]["ms"] / t[3]["ms"]}
        res["decompress"][str(m)] = row
        sys.stderr.write(json.dumps(row) + "\n")

    # ---- (c) -----------------------------------------------------------------------------------------
    d_p, d_c = d_pts[:nmax], d_pts[nmax:]
    d_prec, d_crec = d_rec[:nmax * 48], d_rec[nmax * 48:]
    d_y, d_r = to_dev(ys, np.int64), to_dev(ch, np.int64)
    d_ci, d_idx = to_dev(ci, np.int32), to_dev(idx, np.int32)
    d_bad = d_y.clone()
    torch.cuda.synchronize()
    for count in counts:
        nb = (count + R - 1) // R

        def on_bytes(vals, ok):
            ctx.verify_cells_aggregate_bytes_device(d_crec.data_ptr(), nb, d_ci.data_ptr(), d_idx.data_ptr(),
                                                    d_prec.data_ptr(), vals.data_ptr(), d_r.data_ptr(), count, k, kl,
                                                    enc, True, ok.data_ptr(), extended=True, bitrev=True, stream=sh)

        def on_points(vals, ok):
            ctx.verify_cells_aggregate_checked_device(d_c.data_ptr(), None, nb, d_ci.data_ptr(), d_idx.data_ptr(),
                                                      d_p.data_ptr(), None, vals.data_ptr(), d_r.data_ptr(), count, k,
                                                      kl, True, ok.data_ptr(), extended=True, bitrev=True, stream=sh)

        oks = torch.full((4,), 7, dtype=torch.int32, device=dev)
        if args.trace_leg:
            for _ in range(reps + 1):
                (on_bytes if args.trace_leg == "bytes" else on_points)(d_y, oks[0:])
            st.synchronize()
            ctx.close()
            return
        d_bad.copy_(d_y)
        d_bad[count // 2, 7, 0] += 1
        torch.cuda.synchronize()
        on_bytes(d_y, oks[0:])
        on_bytes(d_bad, oks[1:])
        on_points(d_y, oks[2:])
        on_points(d_bad, oks[3:])
        st.synchronize()
        t = alternate(lambda: on_bytes(d_y, oks[0:]), lambda: on_points(d_y, oks[2:]))
        row = {"count": count, "commitments": nb, "verify_cells_aggregate_bytes_device": t[0],
               "verify_cells_aggregate_checked_device": t[1], "ratio": t[0]["ms"] / t[1]["ms"],
               "extra_ms": t[0]["ms"] - t[1]["ms"], "valid_true_tampered_false": oks.tolist() == [1, 0, 1, 0]}
        res["verify_cells"]["count %d" % count] = row
        sys.stderr.write(json.dumps(row) + "\n")

    # ---- (d) -----------------------------------------------------------------------------------------
    d_out = torch.zeros((nmax * 48,), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    t = alternate(lambda: ctx.g1_compress_device(d_p.data_ptr(), None, nmax, enc, d_out.data_ptr(), sh))
    st.synchronize()
    res["compress"] = {"points": nmax, "g1_compress": t[0], "points_per_s": nmax / t[0]["ms"] * 1e3,
                       "checked": bool((d_out == d_prec).all().item())}
    ctx.close()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
