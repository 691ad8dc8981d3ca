#!/usr/bin/env python3
"""Batched point validation (kzgx_g1_check_batch_device, kzgx_srs_check,
kzgx_verify_aggregate_checked_device) on one MI355X, in one process.

Per curve:
  (a) kzgx_g1_check_batch_device at 64, 4096 and 65536 points, with the curve
      test only and with the subgroup test: device events around the enqueue,
      a warm-up and the median of --reps timed calls;
  (b) the per-point path it replaces: a loop of kzgx_g1_validate (one launch
      and one synchronisation per point) over 4096 points, against ONE
      kzgx_g1_check_batch call on the same host array -- both wall clock, both
      including their copies, median / min / max of --loop-reps runs;
  (c) kzgx_verify_aggregate_device against the checked form (curve test only,
      and with the subgroup test) at 32768 openings, same run, device events;
  (d) kzgx_srs_check on a 4097-point G1 + G2 setup (wall clock: the call
      synchronises), with and without the subgroup test.
The points are honest proofs [q_k(tau)]G; every timed call's answer is checked
(all flags 1; one y + 1 makes the AND 0; the checked aggregate equals the
unchecked one on members).

    python scripts/bench_point_check.py [--out profiles/point_check.json]
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))  # input generation only


def limbs(vals):
    return np.array([[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in vals], dtype=np.uint64)


def timed(fn, reps, torch, st):
    fn()  # warm-up: code objects, workspaces
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms": statistics.median(ms), "ms_min_max": [min(ms), max(ms)]}


def wall(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms": statistics.median(ms), "ms_min_max": [min(ms), max(ms)]}


def run_curve(name, sizes, n_loop, n_agg, n_srs, reps, loop_reps, torch):
    import kzg_ref as K
    import kzgx

    C = K.CURVES[name]
    tau = K.default_tau(C)
    dev = torch.device("cuda", 0)
    ctx = kzgx.Context(name)
    ctx.set_default_table(0)  # no MSM over the SRS is measured here
    ctx.gen_srs(tau, n_srs)
    ctx.gen_srs_g2(tau, n_srs)
    nmax = max(max(sizes), n_agg, n_loop)
    S = limbs(K.random_scalars(C, 4, 0xA66))
    com, cinf = ctx.msm(S)
    zs = np.zeros((nmax, 4), dtype=np.uint64)
    zs[:, 0] = np.arange(nmax, dtype=np.uint64) + 1
    parts = [ctx.prove_single_batch(S, zs[i:i + 32768]) for i in range(0, nmax, 32768)]
    prf = np.concatenate([p[0] for p in parts])
    yv = np.concatenate([p[2] for p in parts])
    assert not cinf and not np.concatenate([p[1] for p in parts]).any()

    def dv(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)

    st = torch.cuda.Stream(device=dev)
    sh = st.cuda_stream
    d_p = dv(prf)
    bad = prf.copy()
    bad[:, kzgx.BASE_LIMBS[name]] ^= np.uint64(1)  # y +- 1 everywhere: off the curve
    d_ok = torch.zeros(nmax, dtype=torch.int32, device=dev)
    d_all = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    res = {"g1_check_device": {}}
    # (a)
    for n in sizes:
        row = {}
        for tag, sg in (("curve", 0), ("subgroup", 1)):
            def call():
                ctx.g1_check_device(d_p.data_ptr(), None, n, sg, d_ok.data_ptr(), d_all.data_ptr(), sh)
            row[tag] = timed(call, reps, torch, st)
            row[tag]["points_per_s"] = n / row[tag]["ms"] * 1e3
            good = bool(d_all.item()) and bool(d_ok[:n].all().item())
            one = prf[:n].copy()
            one[n // 3] = bad[n // 3]
            d_one = dv(one)
            torch.cuda.synchronize()
            ctx.g1_check_device(d_one.data_ptr(), None, n, sg, d_ok.data_ptr(), d_all.data_ptr(), sh)
            st.synchronize()
            flags = d_ok[:n].cpu().numpy()
            row[tag]["checked"] = bool(good and not d_all.item() and int(flags.sum()) == n - 1 and not flags[n // 3])
        res["g1_check_device"][str(n)] = row
    # (b)
    host = np.ascontiguousarray(prf[:n_loop])

    def loop():
        ok = True
        for k in range(n_loop):
            ok = ctx.g1_validate(host[k]) and ok
        assert ok

    def batch(sg=False):
        assert ctx.g1_check(host, None, subgroup=sg).all()

    lp = wall(loop, loop_reps)
    bt = wall(batch, loop_reps)
    bs = wall(lambda: batch(True), loop_reps)
    res["per_point_loop_vs_batch"] = {
        "points": n_loop, "g1_validate_loop": lp, "g1_check_batch": bt, "g1_check_batch_subgroup": bs,
        "speedup": lp["ms"] / bt["ms"], "loop_spread_ms": lp["ms_min_max"][1] - lp["ms_min_max"][0],
        "batch_beats_loop_by_more_than_its_spread": bool(
            lp["ms_min_max"][0] - bt["ms_min_max"][1] > lp["ms_min_max"][1] - lp["ms_min_max"][0])}
    # (c)
    rng = np.random.default_rng(0xC4A11)
    ch = rng.integers(0, 1 << 63, size=(n_agg, 4), dtype=np.uint64)
    ch[:, 2:] = 0  # 128-bit challenges
    ch[:, 0] |= np.uint64(1)
    d_c = dv(np.repeat(com[None, :], n_agg, axis=0))
    d_z, d_y, d_r = dv(zs[:n_agg]), dv(yv[:n_agg]), dv(ch)
    d_ok1 = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    agg = {}
    for tag, sg in (("unchecked", None), ("checked_curve", 0), ("checked_subgroup", 1)):
        def call():
            if sg is None:
                ctx.verify_aggregate_device(d_c.data_ptr(), None, d_p.data_ptr(), None, d_z.data_ptr(), d_y.data_ptr(),
                                            d_r.data_ptr(), n_agg, d_ok1.data_ptr(), sh)
            else:
                ctx.verify_aggregate_checked_device(d_c.data_ptr(), None, d_p.data_ptr(), None, d_z.data_ptr(),
                                                    d_y.data_ptr(), d_r.data_ptr(), n_agg, sg, d_ok1.data_ptr(), sh)
        agg[tag] = timed(call, reps, torch, st)
        agg[tag]["ok"] = bool(d_ok1.item())
    agg["openings"] = n_agg
    agg["checked_curve_over_unchecked"] = agg["checked_curve"]["ms"] / agg["unchecked"]["ms"]
    agg["checked_subgroup_over_unchecked"] = agg["checked_subgroup"]["ms"] / agg["unchecked"]["ms"]
    agg["checked"] = bool(agg["unchecked"]["ok"] and agg["checked_curve"]["ok"] and agg["checked_subgroup"]["ok"])
    res["verify_aggregate"] = agg
    # (d)
    srs = {"points": n_srs}
    for tag, sg in (("curve", False), ("subgroup", True)):
        out = []
        srs[tag] = wall(lambda: out.append(ctx.srs_check(sg)), loop_reps)
        srs[tag]["ok"] = bool(all(o == (True, True) for o in out))
    res["srs_check"] = srs
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="BN254,BLS12381")
    ap.add_argument("--sizes", default="64,4096,65536")
    ap.add_argument("--loop-points", type=int, default=4096)
    ap.add_argument("--openings", type=int, default=32768)
    ap.add_argument("--srs", type=int, default=4097)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--loop-reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_point_check: no GPU (nothing is measured on a CPU)")
    res = {"metric": "batched G1 point validation, checked aggregate verify, SRS check",
           "timing": "device events around the enqueue (median of %d after one warm-up); wall clock where the call "
                     "synchronises (median of %d)" % (args.reps, args.loop_reps),
           "device": torch.cuda.get_device_name(0), "curves": {}}
    for name in args.curves.split(","):
        res["curves"][name] = run_curve(name, [int(x) for x in args.sizes.split(",")], args.loop_points, args.openings,
                                        args.srs, max(args.reps, 1), max(args.loop_reps, 1), torch)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
