#!/usr/bin/env python3
"""Cell recovery (kzgx_recover_cells_device / kzgx_recover_cells_and_proofs_device) against its floors
on one MI355X, in one process.

BLS12-381, 4097 G1 points (with the default table); the data-availability shape (log2n, log2l) =
(12, 6), extended and bit-reversed: 128 cells of 64 values per blob, of which 64 random ones per blob
are handed to the recovery, the flat list shuffled across the blobs.  For 1, 8 and 64 blobs:
  1. kzgx_recover_cells_device against its transform floor: four kzgx_ntt_device calls of the same
     batch x 8192 scalars (inverse, forward, inverse, forward, in place), timed in the same loop;
     the library's own event spans (kzgx_prof_read) say where the rest goes, in a run of its own.
  2. kzgx_recover_cells_and_proofs_device against kzgx_prove_cosets_batch_device alone on the same
     blobs from their coefficients: recovery must recompute every proof, so that is its floor.
  3. for context, once, on the host wall clock: kzgx_poly_interpolate of one blob's 4096 received
     points, the only route from half the cells to the coefficients before this entry point.
Device events around the enqueue on one stream, the two legs of a pair alternating in one loop after
a warm-up of both, median / min / max of --reps.  Every timed call is first checked against the
producer's values, coefficients and proofs.

    python scripts/bench_recover_cells.py [--out profiles/recover_cells.json]
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

SPANS = ("rec_locator", "rec_mask", "rec_shift", "rec_scale", "rec_unshift", "rec_finish")


def stats(ms):
    return {"ms": statistics.median(ms), "ms_min_max": [min(ms), max(ms)]}


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--blobs", default="1,8,64")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_recover_cells: no GPU (nothing is measured on a CPU)")
    import kzg_ref as K
    import kzgx

    C = K.BLS12381
    reps = max(args.reps, 9)
    sizes = [int(x) for x in args.blobs.split(",") if x]
    dev = torch.device("cuda", 0)
    ctx = kzgx.Context("BLS12381")
    ctx.gen_srs(K.default_tau(C), 4097)  # with the default table
    tc, tn, tb = ctx.default_table_info()
    st = torch.cuda.Stream(device=dev)
    sh = st.cuda_stream
    w = 2 * ctx.w64
    rng = np.random.default_rng(0x2EC0)
    k, kl, R, l, n, D = 12, 6, 128, 64, 4096, 8192
    blobs = max(sizes)

    def scalars(count):
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

    def alternate(fa, fb):
        fa()
        fb()
        torch.cuda.synchronize()
        xa, xb = [], []
        for _ in range(reps):
            xa.append(event_ms(fa))
            xb.append(event_ms(fb))
        return stats(xa), stats(xb)

    def to_dev(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)

    # ---- the producer side: coefficients -> cells and proofs ------------------------------------------
    coeffs = scalars(blobs * n).reshape(blobs, n, 4)
    proofs, proof_inf, ys = ctx.prove_cosets(coeffs, kl, extended=True, bitrev=True)
    d_coef = to_dev(coeffs, np.int64)
    d_y = torch.zeros((blobs * D, 4), dtype=torch.int64, device=dev)
    d_c = torch.zeros((blobs * n, 4), dtype=torch.int64, device=dev)
    d_xy = torch.zeros((blobs * R, w), dtype=torch.int64, device=dev)
    d_inf = torch.zeros((blobs * R,), dtype=torch.int32, device=dev)
    d_xy2, d_inf2 = torch.zeros_like(d_xy), torch.zeros_like(d_inf)
    d_ok = torch.zeros((blobs,), dtype=torch.int32, device=dev)
    d_scratch = torch.zeros((blobs * D, 4), dtype=torch.int64, device=dev)

    res = {"metric": "kzgx_recover_cells_device against four kzgx_ntt_device calls of the same size; "
                     "kzgx_recover_cells_and_proofs_device against kzgx_prove_cosets_batch_device from coefficients",
           "timing": "device events around the enqueue on one stream; the legs of a pair alternating in one loop, "
                     "median of %d after one warm-up of each; kzgx_poly_interpolate: host wall clock, one call" % reps,
           "device": torch.cuda.get_device_name(0), "curve": "BLS12381", "srs_points": 4097,
           "default_table": {"c": tc, "points": tn, "bytes": tb},
           "shape": {"log2n": k, "log2l": kl, "extended": True, "bit_reversed": True, "cells_per_blob": R,
                     "cells_given_per_blob": R // 2},
           "cases": {}}

    for nb in sizes:
        keep = [np.sort(rng.permutation(R)[:R // 2]) for _ in range(nb)]
        bi = np.repeat(np.arange(nb, dtype=np.uint32), R // 2)
        ci = np.concatenate(keep).astype(np.uint32)
        order = rng.permutation(nb * (R // 2))
        bi, ci = bi[order], ci[order]
        cells = ys[bi, ci]
        d_bi, d_ci, d_cells = to_dev(bi, np.int32), to_dev(ci, np.int32), to_dev(cells, np.int64)
        cnt = len(bi)
        torch.cuda.synchronize()

        def rec():
            ctx.recover_cells_device(d_bi.data_ptr(), d_ci.data_ptr(), d_cells.data_ptr(), cnt, nb, k, kl,
                                     d_y.data_ptr(), d_c.data_ptr(), d_ok.data_ptr(), bitrev=True, stream=sh)

        def four_ntts():
            p = d_scratch.data_ptr()
            for inverse in (True, False, True, False):
                ctx.ntt_device(p, D, p, D, k + 1, nb, inverse=inverse, bitrev=True, stream=sh)

        def rec_proofs():
            ctx.recover_cells_and_proofs_device(d_bi.data_ptr(), d_ci.data_ptr(), d_cells.data_ptr(), cnt, nb, k, kl,
                                                d_y.data_ptr(), None, d_xy.data_ptr(), d_inf.data_ptr(),
                                                d_ok.data_ptr(), bitrev=True, stream=sh)

        def prove():
            ctx.prove_cosets_device(d_coef.data_ptr(), k, kl, nb, n, d_xy2.data_ptr(), d_inf2.data_ptr(), None,
                                    extended=True, bitrev=True, stream=sh)

        # the answers first
        d_y.zero_(), d_c.zero_(), d_ok.zero_()
        torch.cuda.synchronize()
        rec()
        st.synchronize()
        plain_ok = (bool((d_ok[:nb] == 1).all()) and
                    d_y[:nb * D].cpu().numpy().tobytes() == ys[:nb].tobytes() and
                    d_c[:nb * n].cpu().numpy().tobytes() == coeffs[:nb].tobytes())
        d_y.zero_(), d_ok.zero_()
        torch.cuda.synchronize()
        rec_proofs()
        st.synchronize()
        proofs_ok = (bool((d_ok[:nb] == 1).all()) and
                     d_y[:nb * D].cpu().numpy().tobytes() == ys[:nb].tobytes() and
                     d_xy[:nb * R].cpu().numpy().tobytes() == proofs[:nb].tobytes() and
                     (d_inf[:nb * R].cpu().numpy().astype(bool) == proof_inf[:nb].reshape(-1)).all())
        note("%d blobs: recovered exactly: %s, with proofs: %s" % (nb, plain_ok, bool(proofs_ok)))

        a, b = alternate(rec, four_ntts)
        c, d = alternate(rec_proofs, prove)
        ctx.prof_clear()
        ctx.prof_enable(True)
        total = event_ms(rec)
        spans = {name: ctx.prof_read(name)[0] for name in SPANS}
        ctx.prof_enable(False)
        ctx.prof_clear()
        res["cases"]["%d blobs" % nb] = {
            "blobs": nb, "cells_given": cnt, "exact": bool(plain_ok and proofs_ok),
            "recover_cells_device": a, "four_ntt_device": b, "ratio_to_transform_floor": a["ms"] / b["ms"],
            "own_kernels_ms": a["ms"] - b["ms"], "blobs_per_s": nb / a["ms"] * 1e3,
            "recover_cells_and_proofs_device": c, "prove_cosets_batch_device": d,
            "overhead_over_proving_ms": c["ms"] - d["ms"], "ratio_to_proving": c["ms"] / d["ms"],
            "spans": {"call_ms_with_spans": total, "spans_ms": spans}}
        note(json.dumps(res["cases"]["%d blobs" % nb]))

    # ---- context: the parent commit's only route, one blob's 4096 received points through the interpolation ----
    kept = np.sort(rng.permutation(R)[:R // 2])
    xs = np.concatenate([kzgx.coset_points("BLS12381", k, kl, int(p), extended=True, bitrev=True) for p in kept])
    vals = ys[0, kept].reshape(-1, 4)
    ctx.interpolate(xs[:64], vals[:64])  # the code object and the workspaces, not the size
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = ctx.interpolate(xs, vals)
    ctx.sync()
    ms = (time.perf_counter() - t0) * 1e3
    # the interpolant of 4096 points on a polynomial of 4096 coefficients is that polynomial
    res["poly_interpolate_one_blob_host_wall"] = {"points": int(xs.shape[0]), "ms": ms, "calls": 1,
                                                  "exact": got.tobytes() == coeffs[0].tobytes()}
    note(json.dumps(res["poly_interpolate_one_blob_host_wall"]))
    ctx.close()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
