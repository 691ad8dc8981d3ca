#!/usr/bin/env python3
"""Batch openings against the per-claim route, on one MI355X: device buffers in, device events
around the enqueue on one stream, one warm-up and the median of --reps (>= 9) timed calls per
figure, the two legs of every comparison alternating in one process.

Per curve and shape (n coefficients, polynomials, two groups; every polynomial opened once):
  prove   kzgx_prove_multi_batch_device (fold + one quotient launch + one batched MSM of 2, values
          y_k included) against the route without it: kzgx_prove_single_batch_device over all
          `count` (polynomial, point) pairs;
  verify  kzgx_verify_multi_batch_device against kzgx_verify_aggregate_device over the `count`
          separate openings;
  kernels the fold's and the evaluation's own times (the context's event profiler, a pass of its
          own), the fold's achieved bytes/s (count x n scalars read, groups x n written) against
          the guide's HBM figures (6.29 TB/s measured copy, 8.0 TB/s datasheet).

Checked once, outside the timed region: the multi proof of a group equals the weighted sum of the
per-claim proofs (KZG is additively homomorphic; kzgx_msm_g1_points), Y_g equals sum w_k y_k in
Python integers, both verifiers say 1 on the honest claims and 0 with one value off by one.

    python scripts/bench_prove_multi.py [--out profiles/prove_multi.json]
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

HBM_MEASURED = 6.29e12
HBM_SPEC = 8.0e12


def limbs(vals):
    return np.array([[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in vals], dtype=np.uint64)


def ints(a):
    return [sum(int(w) << (64 * i) for i, w in enumerate(row)) for row in np.asarray(a, dtype=np.uint64).reshape(-1, 4)]


def alternating(fa, fb, reps, torch, st):
    """medians (and min, max) of two legs timed turn by turn after one warm-up each"""
    fa()
    fb()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(reps):
        for leg, fn in enumerate((fa, fb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            fn()
            b.record(st)
            b.synchronize()
            ms[leg].append(a.elapsed_time(b))
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def run_shape(ctx, name, C, n, sizes, reps, torch):
    import kzgx
    r = C.r
    dev = torch.device("cuda", 0)
    nl = kzgx.BASE_LIMBS[name]
    n_polys = count = sum(sizes)
    ng = len(sizes)
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    index = np.arange(count, dtype=np.uint32)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0xBA7C4 + n)
    coeffs = torch.randint(0, 1 << 62, (n_polys, n, 4), dtype=torch.int64, device=dev, generator=gen)
    coeffs[:, :, 3] >>= 2  # < 2^252 < r on both curves
    rng = np.random.default_rng(0x5EED + n)
    z_e = [int(v) for v in rng.integers(2, 1 << 62, size=ng)]
    w_e = [int(a) | (int(b) << 64) for a, b in rng.integers(1, 1 << 62, size=(count, 2))]  # 126-bit weights
    r_e = [1] + [int(a) | (int(b) << 64) for a, b in rng.integers(1, 1 << 62, size=(ng - 1, 2))]
    group_of = np.repeat(np.arange(ng), sizes)
    rk_e = [int(a) | (int(b) << 64) for a, b in rng.integers(1, 1 << 62, size=(count, 2))]

    def dv(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.int64 if a.dtype == np.uint64 else np.int32)).to(dev)

    d_index, d_start = dv(index), dv(start)
    d_z, d_w, d_r = dv(limbs(z_e)), dv(limbs(w_e)), dv(limbs(r_e))
    d_zk, d_rk = dv(limbs([z_e[g] for g in group_of])), dv(limbs(rk_e))
    m_out = torch.zeros((ng, 2 * nl), dtype=torch.int64, device=dev)
    m_inf = torch.zeros(ng, dtype=torch.int32, device=dev)
    m_y = torch.zeros((count, 4), dtype=torch.int64, device=dev)
    m_Y = torch.zeros((ng, 4), dtype=torch.int64, device=dev)
    m_ok = torch.zeros(1, dtype=torch.int32, device=dev)
    s_out = torch.zeros((count, 2 * nl), dtype=torch.int64, device=dev)
    s_inf = torch.zeros(count, dtype=torch.int32, device=dev)
    s_y = torch.zeros((count, 4), dtype=torch.int64, device=dev)
    com = torch.zeros((n_polys, 2 * nl), dtype=torch.int64, device=dev)
    cinf = torch.zeros(n_polys, dtype=torch.int32, device=dev)
    v_ok = torch.zeros(2, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(device=dev)
    sh = st.cuda_stream
    torch.cuda.synchronize()
    ctx.msm_batch_device(coeffs.data_ptr(), n, n_polys, n, com.data_ptr(), cinf.data_ptr(), sh)
    st.synchronize()

    def multi():
        ctx.prove_multi_device(coeffs.data_ptr(), n, n, n_polys, d_index.data_ptr(), d_start.data_ptr(), ng,
                               d_z.data_ptr(), d_w.data_ptr(), count, m_out.data_ptr(), m_inf.data_ptr(),
                               m_y.data_ptr(), m_Y.data_ptr(), m_ok.data_ptr(), stream=sh)

    def singles():
        ctx.prove_single_batch_device(coeffs.data_ptr(), n, n, d_zk.data_ptr(), count, s_out.data_ptr(),
                                      s_inf.data_ptr(), s_y.data_ptr(), sh)

    def v_multi(y=None):
        ctx.verify_multi_device(com.data_ptr(), cinf.data_ptr(), n_polys, d_index.data_ptr(), d_start.data_ptr(), ng,
                                d_z.data_ptr(), (m_y if y is None else y).data_ptr(), d_w.data_ptr(),
                                m_out.data_ptr(), m_inf.data_ptr(), d_r.data_ptr(), count, v_ok.data_ptr(),
                                stream=sh)

    def v_agg(y=None):
        ctx.verify_aggregate_device(com.data_ptr(), cinf.data_ptr(), s_out.data_ptr(), s_inf.data_ptr(),
                                    d_zk.data_ptr(), (s_y if y is None else y).data_ptr(), d_rk.data_ptr(), count,
                                    v_ok[1:].data_ptr(), sh)

    p_ms = alternating(multi, singles, reps, torch, st)
    v_ms = alternating(v_multi, v_agg, reps, torch, st)
    st.synchronize()
    # checks, outside the timed region
    ok_good = v_ok.cpu().tolist()
    y_host = m_y.cpu().numpy().view(np.uint64)
    same_y = bool((y_host == s_y.cpu().numpy().view(np.uint64)).all())
    y_e = ints(y_host)
    Y_ok = ints(m_Y.cpu().numpy().view(np.uint64)) == [
        sum(w_e[k] * y_e[k] for k in range(start[g], start[g + 1])) % r for g in range(ng)]
    proofs_s, inf_s = s_out.cpu().numpy().view(np.uint64), s_inf.cpu().numpy()
    proofs_m, inf_m = m_out.cpu().numpy().view(np.uint64), m_inf.cpu().numpy()
    homomorphic = True
    for g in range(ng):
        a, b = int(start[g]), int(start[g + 1])
        pt, pinf = ctx.msm_points(proofs_s[a:b], limbs(w_e[a:b]), inf_s[a:b])
        homomorphic = homomorphic and bool(pinf) == bool(inf_m[g]) and bool((pt == proofs_m[g]).all())
    bad = y_host.copy()
    bad[count // 2] = limbs([(y_e[count // 2] + 1) % r])[0]
    d_bad = dv(bad)
    v_multi(d_bad)
    v_agg(d_bad)
    st.synchronize()
    ok_bad = v_ok.cpu().tolist()
    checked = (same_y and Y_ok and homomorphic and ok_good == [1, 1] and ok_bad == [0, 0]
               and int(m_ok.item()) == 1)
    # the kernels' own times
    ctx.prof_enable(True)
    ctx.prof_clear()
    for _ in range(reps):
        multi()
    st.synchronize()
    fold_ms, fold_n = ctx.prof_read("multi_fold")
    eval_ms, eval_n = ctx.prof_read("multi_eval")
    quot_ms, quot_n = ctx.prof_read("quotient_single")
    ctx.prof_enable(False)
    ctx.prof_clear()
    fold_ms, eval_ms, quot_ms = fold_ms / fold_n, eval_ms / eval_n, quot_ms / quot_n
    fold_bytes = (count + ng) * n * 32
    rate = fold_bytes / (fold_ms * 1e-3)
    return {
        "n": n, "polynomials": n_polys, "groups": [int(s) for s in sizes], "claims": count,
        "prove_multi_ms": p_ms[0][0], "prove_multi_ms_min_max": list(p_ms[0][1:]),
        "prove_single_batch_ms": p_ms[1][0], "prove_single_batch_ms_min_max": list(p_ms[1][1:]),
        "prove_speedup": p_ms[1][0] / p_ms[0][0],
        "verify_multi_ms": v_ms[0][0], "verify_multi_ms_min_max": list(v_ms[0][1:]),
        "verify_aggregate_ms": v_ms[1][0], "verify_aggregate_ms_min_max": list(v_ms[1][1:]),
        "verify_speedup": v_ms[1][0] / v_ms[0][0],
        "fold_kernel_ms": fold_ms, "eval_kernel_ms": eval_ms, "quotient_kernel_ms": quot_ms,
        "fold_bytes": fold_bytes, "fold_bytes_per_s": rate, "fold_share_of_hbm_measured": rate / HBM_MEASURED,
        "fold_share_of_hbm_spec": rate / HBM_SPEC,
        "eval_bytes_per_s": count * n * 32 / (eval_ms * 1e-3), "checked": bool(checked)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="BN254,BLS12381")
    ap.add_argument("--shapes", default="4096:29+3,1048576:25+3", help="n:group sizes, comma separated")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_prove_multi: no GPU (nothing is measured on a CPU)")
    import kzg_ref as K
    import kzgx
    shapes = [(int(s.split(":")[0]), [int(v) for v in s.split(":")[1].split("+")]) for s in args.shapes.split(",")]
    res = {"metric": "batch openings vs one opening per claim (ms per call), fold / evaluation kernel times",
           "timing": "device events around the enqueue, legs alternating, median of %d after one warm-up" % args.reps,
           "device": torch.cuda.get_device_name(0), "hbm_bytes_per_s": {"measured_copy": HBM_MEASURED, "spec": HBM_SPEC},
           "curves": {}}
    for name in args.curves.split(","):
        C = K.CURVES[name]
        tau = K.default_tau(C)
        rows = []
        for n, sizes in shapes:
            ctx = kzgx.Context(name)
            ctx.gen_srs(tau, n)
            ctx.gen_srs_g2(tau, 2)
            rows.append(run_shape(ctx, name, C, n, sizes, max(args.reps, 1), torch))
            ctx.close()
            print(json.dumps({name: rows[-1]}), flush=True)
        res["curves"][name] = rows
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
