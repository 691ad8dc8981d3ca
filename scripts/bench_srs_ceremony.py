#!/usr/bin/env python3
"""Setup ceremony (kzgx_srs_update, kzgx_srs_verify_structure) on one MI355X,
in one process, BLS12-381 by default.

Per (G1 points, G2 points) size, legs alternating inside every repetition:
  (a) update:    kzgx_srs_update(s) over both halves, witness included (the
                 variable-base double-and-add, a lane per point) + the
                 install path
      generate:  kzgx_gen_srs_g1 + kzgx_gen_srs_g2 of the same sizes (the
                 fixed-base comb) + the same install path
  (b) structure: kzgx_srs_verify_structure under explicit challenges
      check:     kzgx_srs_check(subgroup = 1)
Every call synchronises, so all times are wall clock: one warm-up, then the
median / min / max of --reps runs.  The default table is off (both legs of
(a) would build the same one).  Every timed answer is checked: the update
of a generated setup for tau equals a second context's generated setup for
tau s on every point, the structure test and the point check answer
(1, 1), and one swapped pair of G1 points turns the structure test to
(0, 1) while the point check still passes.  There is no pass threshold:
the script reports, including where the new path is the slower one.

    python scripts/bench_srs_ceremony.py [--out profiles/srs_ceremony.json]
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))  # the curve order and the default tau only

RHO, SIGMA = 0x9E3779B97F4A7C15F39CC0605CEDC834, 0xD1B54A32D192ED03C2B2AE3D27D4EB4F


def stats(ms):
    return {"ms": statistics.median(ms), "ms_min_max": [min(ms), max(ms)]}


def alternate(legs, reps):
    """legs: name -> callable; one warm-up of each, then reps rounds in order"""
    for fn in legs.values():
        fn()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: stats(v) for k, v in ms.items()}


def run_size(name, n, m, reps):
    import kzg_ref as K
    import kzgx

    C = K.CURVES[name]
    tau, s = K.default_tau(C), 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % C.r
    ctx, ref = kzgx.Context(name), kzgx.Context(name)
    ctx.set_default_table(0)
    ref.set_default_table(0)
    row = {"g1_points": n, "g2_points": m}

    def generate():
        ctx.gen_srs(tau, n)
        ctx.gen_srs_g2(tau, m)

    # (a) the update always runs on whatever the generate leg just installed
    generate()
    row.update(alternate({"update": lambda: ctx.srs_update(s), "generate": generate}, reps))
    row["update_over_generate"] = row["update"]["ms"] / row["generate"]["ms"]
    generate()
    ctx.srs_update(s)
    ref.gen_srs(tau * s % C.r, n)
    ref.gen_srs_g2(tau * s % C.r, m)
    g1, g2, r1, r2 = ctx.get_srs(), ctx.get_srs_g2(), ref.get_srs(), ref.get_srs_g2()
    row["update_checked"] = bool(np.array_equal(g1, r1) and np.array_equal(g2, r2))
    ref.close()
    # (b)
    out = {"structure": [], "check": []}
    row.update(alternate({"structure": lambda: out["structure"].append(ctx.srs_verify_structure(RHO, SIGMA, True)),
                          "check": lambda: out["check"].append(ctx.srs_check(True))}, reps))
    row["structure_over_check"] = row["structure"]["ms"] / row["check"]["ms"]
    good = all(o == (True, True) for o in out["structure"] + out["check"])
    g1[[n // 2, n // 2 + 1]] = g1[[n // 2 + 1, n // 2]]
    ctx.load_srs(g1)
    row["structure_checked"] = bool(good and ctx.srs_verify_structure(RHO, SIGMA) == (False, True)
                                    and ctx.srs_check(True) == (True, True))
    ctx.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curve", default="BLS12381")
    ap.add_argument("--sizes", default="4097:65,65536:65,1048576:65", help="G1:G2 point counts")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_srs_ceremony: no GPU (nothing is measured on a CPU)")
    res = {"metric": "powers-of-tau update against fixed-base generation; structure test against the per-point check",
           "timing": "wall clock, every call synchronises; legs alternate; median of %d after one warm-up" % args.reps,
           "device": torch.cuda.get_device_name(0), "curve": args.curve, "sizes": []}
    for sz in args.sizes.split(","):
        n, m = (int(x) for x in sz.split(":"))
        res["sizes"].append(run_size(args.curve, n, m, max(args.reps, 1)))
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
