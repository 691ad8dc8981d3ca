#!/usr/bin/env python3
"""Aggregated verification against the per-opening batch, and the variable-base
MSM it runs on, on one MI355X: device buffers in, device events around the
enqueue, a warm-up and the median of --reps (>= 9) timed calls per figure.

Per curve and opening count (1024, 4096, 32768, 2^20): openings/s of
kzgx_verify_aggregate_device and of kzgx_verify_single_batch_device (the
existing per-opening path) in the same process.  kzgx_msm_g1_points_device
points/s at 2^12, 2^16, 2^20 points for 128-bit and for full-width scalars.

Every boolean is checked once, outside the timed region, against exponent
arithmetic with the known tau: the openings are (C, pi_k, z_k, y_k) of one
cubic P, so c = P(tau), p_k = (c - y_k) / (tau - z_k) and the aggregate holds
iff  tau sum r_k p_k == sum r_k (c - y_k + z_k p_k)  (mod r).  The y_k the GPU
produced are compared with P(z_k) for every k, and a sample of the proof
points with [p_k]G (the C oracle).

    python scripts/bench_verify_aggregate.py [--out profiles/verify_aggregate.json]
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kzg-commitments_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))  # checker only


def limbs(vals):
    return np.array([[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in vals], dtype=np.uint64)


def batch_inv(r, vals):
    pre, acc = [], 1
    for v in vals:
        pre.append(acc)
        acc = acc * v % r
    inv = pow(acc, -1, r)
    out = [0] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        out[i] = inv * pre[i] % r
        inv = inv * vals[i] % r
    return out


def timed(fn, reps, torch, st):
    fn()  # warm-up: code objects, workspaces, tables
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def run_curve(name, counts, msm_sizes, reps, torch):
    import corc
    import kzg_ref as K
    import kzgx

    C = K.CURVES[name]
    r = C.r
    tau = K.default_tau(C)
    dev = torch.device("cuda", 0)
    ctx = kzgx.Context(name)
    ctx.gen_srs(tau, 8)
    ctx.gen_srs_g2(tau, 2)
    nmax = max(max(counts), max(msm_sizes))
    P = K.random_scalars(C, 4, 0xA66)
    S = limbs(P)
    com, cinf = ctx.msm(S)
    zs = np.zeros((nmax, 4), dtype=np.uint64)
    zs[:, 0] = np.arange(nmax, dtype=np.uint64) + 1
    parts = [ctx.prove_single_batch(S, zs[i:i + 32768]) for i in range(0, nmax, 32768)]
    prf = np.concatenate([p[0] for p in parts])
    pinf = np.concatenate([p[1] for p in parts])
    yv = np.concatenate([p[2] for p in parts])
    assert not cinf and not pinf.any()
    # exponent oracle of the inputs
    c_e = sum(a * pow(tau, i, r) for i, a in enumerate(P)) % r
    y_e = [(((P[3] * z + P[2]) * z + P[1]) * z + P[0]) % r for z in range(1, nmax + 1)]
    assert (yv == limbs(y_e)).all(), "GPU evaluations differ from P(z)"
    inv = batch_inv(r, [(tau - z) % r for z in range(1, nmax + 1)])
    p_e = [(c_e - y) * i % r for y, i in zip(y_e, inv)]
    for k in (0, 1, nmax // 2, nmax - 1):
        exp = corc.scalar_mul(name, (C.gx, C.gy), p_e[k])
        assert corc.array_to_points(name, prf[k][None, :])[0] == exp, "proof %d is not [p_k]G" % k
    rng = np.random.default_rng(0xC4A11)
    ch = rng.integers(0, 1 << 63, size=(nmax, 4), dtype=np.uint64)
    ch[:, 2:] = 0  # 128-bit challenges
    ch[:, 0] |= np.uint64(1)
    ch_e = [int(a) | (int(b) << 64) for a, b in ch[:, :2]]

    def oracle(n, bad=None):
        lhs = tau * sum(rk * p for rk, p in zip(ch_e[:n], p_e[:n]))
        rhs = sum(rk * (c_e - y + (k + 1) * p) for k, (rk, y, p) in enumerate(zip(ch_e[:n], y_e[:n], p_e[:n])))
        if bad is not None:
            rhs -= ch_e[bad]  # y_bad + 1
        return (lhs - rhs) % r == 0

    def dv(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)

    d_c = dv(np.repeat(com[None, :], nmax, axis=0))
    d_p, d_z, d_y, d_r = dv(prf), dv(zs), dv(yv), dv(ch)
    ybad = yv.copy()
    d_ok1 = torch.zeros(1, dtype=torch.int32, device=dev)
    d_okn = torch.zeros(nmax, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(device=dev)  # every timed call and its events run on this stream
    sh = st.cuda_stream
    torch.cuda.synchronize()
    res = {"verify": {}, "msm_points": {}}
    for n in counts:
        bad = n // 3
        ybad[:] = yv
        ybad[bad] = limbs([(y_e[bad] + 1) % r])[0]
        d_yb = dv(ybad[:n])

        def agg(y=d_y):
            ctx.verify_aggregate_device(d_c.data_ptr(), None, d_p.data_ptr(), None, d_z.data_ptr(), y.data_ptr(),
                                        d_r.data_ptr(), n, d_ok1.data_ptr(), sh)

        def single(y=d_y):
            ctx.verify_single_batch_device(d_c.data_ptr(), None, d_p.data_ptr(), None, d_z.data_ptr(), y.data_ptr(),
                                           n, d_okn.data_ptr(), sh)

        a_ms = timed(agg, reps, torch, st)
        ok_good = bool(d_ok1.item())
        s_ms = timed(single, reps, torch, st)
        singles_ok = bool(d_okn[:n].all().item())
        torch.cuda.synchronize()
        agg(d_yb)
        st.synchronize()
        ok_bad = bool(d_ok1.item())
        single(d_yb)
        st.synchronize()
        sb = d_okn[:n].cpu().numpy()
        checked = (ok_good == oracle(n) and ok_good and ok_bad == oracle(n, bad) and not ok_bad and singles_ok
                   and int(sb.sum()) == n - 1 and not sb[bad])
        res["verify"][str(n)] = {
            "aggregate_ms": a_ms[0], "aggregate_ms_min_max": [a_ms[1], a_ms[2]], "aggregate_per_s": n / a_ms[0] * 1e3,
            "single_batch_ms": s_ms[0], "single_batch_ms_min_max": [s_ms[1], s_ms[2]],
            "single_batch_per_s": n / s_ms[0] * 1e3, "speedup": s_ms[0] / a_ms[0], "checked": bool(checked)}
    # the variable-base MSM alone: the proofs as points
    full = rng.integers(0, 1 << 63, size=(nmax, 4), dtype=np.uint64)
    full[:, 3] >>= np.uint64(2)  # < 2^253 < r on both curves
    d_full = dv(full)
    d_out = torch.zeros(2 * kzgx.BASE_LIMBS[name], dtype=torch.int64, device=dev)
    d_oi = torch.zeros(1, dtype=torch.int32, device=dev)
    for n in msm_sizes:
        row = {}
        for tag, d_s, host in (("scalars_128", d_r, ch), ("scalars_253", d_full, full)):
            def msm():
                ctx.msm_points_device(d_p.data_ptr(), None, d_s.data_ptr(), n, d_out.data_ptr(), d_oi.data_ptr(), sh)
            ms = timed(msm, reps, torch, st)
            row[tag] = {"ms": ms[0], "ms_min_max": [ms[1], ms[2]], "points_per_s": n / ms[0] * 1e3}
            if n <= 4096:  # sum s_k p_k in the exponent
                e = sum((sum(int(host[k, i]) << (64 * i) for i in range(4))) * p_e[k] for k in range(n)) % r
                got = corc.array_to_points(name, d_out.cpu().numpy().view(np.uint64)[None, :])[0]
                row[tag]["checked"] = bool(got == corc.scalar_mul(name, (C.gx, C.gy), e) and not d_oi.item())
        res["msm_points"][str(n)] = row
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="BN254,BLS12381")
    ap.add_argument("--counts", default="1024,4096,32768,1048576")
    ap.add_argument("--msm", default="4096,65536,1048576")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_verify_aggregate: no GPU (nothing is measured on a CPU)")
    counts = [int(x) for x in args.counts.split(",")]
    sizes = [int(x) for x in args.msm.split(",")]
    res = {"metric": "aggregated verify vs per-opening batch (openings/s), variable-base MSM (points/s)",
           "timing": "device events around the enqueue, median of %d after one warm-up" % args.reps,
           "device": torch.cuda.get_device_name(0), "window_pin": os.environ.get("KZGX_VAR_WINDOW", ""), "curves": {}}
    for name in args.curves.split(","):
        res["curves"][name] = run_curve(name, counts, sizes, max(args.reps, 1), torch)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
