#!/usr/bin/env python3
"""Blob proofs (kzgx_prove_blobs_batch_device, kzgx_verify_blobs_batch_device,
kzgx_blob_challenges_device, kzgx_evals_at_batch_device) on one MI355X, BLS12-381,
log2n = 12, bit-reversed 32-byte big-endian elements, device pointers, one process.
For 1, 8, 64 and 2048 blobs:

  (1) kzgx_prove_blobs_batch_device against kzgx_commit_evals_batch_device +
      kzgx_prove_evals_batch_device on the same blobs as limbs with z supplied: the
      difference is what the hash, the decode and the compression cost;
  (2) kzgx_verify_blobs_batch_device against kzgx_verify_aggregate_checked_device on
      the decoded points with z and y supplied; and kzgx_evals_at_batch_device alone
      against the route to y that existed before: kzgx_ntt_device (inverse) into a
      coefficient buffer + kzgx_quotient_single_batch_device with the quotient thrown away;
  (3) kzgx_blob_challenges_device alone against the honest competitor: a device-to-host
      copy of the blobs and hashlib.sha256 on the host, wall clock (the device leg is
      also taken by wall clock around a synchronise, so both sides are the same kind
      of number).
Device events around the enqueue on a caller's stream unless stated; the legs of a
comparison alternate in one loop; medians of --reps after one warm-up of each.
Every timed call's answer is checked: both prove routes give the same records, the
verifies are true on the honest batch and false with one value changed, z equals
hashlib's, y equals the quotient route's.

    python scripts/bench_blob_proofs.py [--out profiles/blob_proofs.json]
Prints one JSON line (and writes it to --out)."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kzg-commitments_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))  # the setup's tau only

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def stats(ms):
    return {"ms": statistics.median(ms), "ms_min_max": [min(ms), max(ms)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="1,8,64,2048")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_blob_proofs: no GPU (nothing is measured on a CPU)")
    import kzg_ref as K
    import kzgx

    name, C, enc = "BLS12381", K.BLS12381, kzgx.ENC_ZCASH
    reps = max(args.reps, 1)
    counts = [int(x) for x in args.counts.split(",") if x]
    k, n = 12, 4096
    dev = torch.device("cuda", 0)
    ctx = kzgx.Context(name)
    tau = K.default_tau(C)
    ctx.gen_srs(tau, 4097)  # with the default table, as the other benchmarks of this shape
    ctx.gen_srs_g2(tau, 2)
    st = torch.cuda.Stream(device=dev)
    sh = st.cuda_stream
    w = 2 * ctx.w64
    rng = np.random.default_rng(0xB10B)
    cmax = max(counts)

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        return a.elapsed_time(b)

    def wall_ms(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def alternate(*fns, timer=event_ms):
        for f in fns:
            f()
        torch.cuda.synchronize()
        xs = [[] for _ in fns]
        for _ in range(reps):
            for x, f in zip(xs, fns):
                x.append(timer(f))
        return [stats(x) for x in xs]

    # cmax blobs of canonical elements: limbs, and the same as big-endian bytes
    limbs = rng.integers(0, 1 << 63, size=(cmax * n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(
        0, 2, size=(cmax * n, 4), dtype=np.uint64)
    limbs[:, 3] &= np.uint64((1 << 62) - 1)  # < 2^254 < r
    be = np.ascontiguousarray(limbs[:, ::-1]).byteswap().view(np.uint8).reshape(-1)
    d_limbs = torch.from_numpy(limbs.view(np.int64)).to(dev)
    d_be = torch.from_numpy(be).to(dev)
    i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=dev)
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)
    d_crec, d_prec, d_crec2, d_prec2 = u8(cmax * 48), u8(cmax * 48), u8(cmax * 48), u8(cmax * 48)
    d_z, d_y, d_y2, d_z2 = i64(cmax, 4), i64(cmax, 4), i64(cmax, 4), i64(cmax, 4)
    d_ok = i32(cmax)
    d_cxy, d_pxy, d_cinf, d_pinf = i64(cmax, w), i64(cmax, w), i32(cmax), i32(cmax)
    d_coef, d_q = i64(cmax * n, 4), i64(cmax * (n - 1), 4)
    ch = rng.integers(0, 1 << 63, size=(cmax, 4), dtype=np.uint64)
    ch[:, 2:] = 0
    ch[0] = (1, 0, 0, 0)
    d_r = torch.from_numpy(ch.view(np.int64)).to(dev)
    d_bad = d_be.clone()
    torch.cuda.synchronize()

    res = {"metric": "blob proofs at log2n = 12, bit-reversed big-endian bytes: prove and verify against the entries "
                     "they chain with z (and y) supplied, the value kernel against the inverse NTT + quotient route, "
                     "the challenge kernel against a device-to-host copy + hashlib",
           "timing": "device events around the enqueue on a caller's stream (wall clock where stated); the legs of a "
                     "comparison alternate in one loop; median of %d after one warm-up of each" % reps,
           "device": torch.cuda.get_device_name(0), "curve": name, "log2n": k, "counts": {}}

    for m in counts:
        def prove_blobs():
            ctx.prove_blobs_device(d_be.data_ptr(), k, m, d_crec.data_ptr(), d_prec.data_ptr(), d_z.data_ptr(),
                                   d_y.data_ptr(), d_ok.data_ptr(), bytes_mode=True, bitrev=True, stream=sh)

        def prove_parts():
            ctx.commit_evals_device(d_limbs.data_ptr(), k, m, n, d_cxy.data_ptr(), d_cinf.data_ptr(), bitrev=True,
                                    stream=sh)
            ctx.prove_evals_device(d_limbs.data_ptr(), k, n, d_z.data_ptr(), m, d_pxy.data_ptr(), d_pinf.data_ptr(),
                                   d_y2.data_ptr(), bitrev=True, stream=sh)

        prove_blobs()  # fills z for the parts
        st.synchronize()
        t_prove = alternate(prove_blobs, prove_parts)
        ctx.g1_compress_device(d_cxy.data_ptr(), d_cinf.data_ptr(), m, enc, d_crec2.data_ptr(), sh)
        ctx.g1_compress_device(d_pxy.data_ptr(), d_pinf.data_ptr(), m, enc, d_prec2.data_ptr(), sh)
        st.synchronize()
        same = bool((d_crec[:m * 48] == d_crec2[:m * 48]).all().item()) and \
            bool((d_prec[:m * 48] == d_prec2[:m * 48]).all().item()) and bool((d_y[:m] == d_y2[:m]).all().item()) and \
            bool(d_ok[:m].all().item())

        oks = torch.full((4,), 7, dtype=torch.int32, device=dev)

        def verify_blobs(blobs, ok):
            ctx.verify_blobs_device(blobs.data_ptr(), k, m, d_crec.data_ptr(), d_prec.data_ptr(), d_r.data_ptr(), True,
                                    ok.data_ptr(), bytes_mode=True, bitrev=True, stream=sh)

        def verify_points(y, ok):
            ctx.verify_aggregate_checked_device(d_cxy.data_ptr(), d_cinf.data_ptr(), d_pxy.data_ptr(),
                                                d_pinf.data_ptr(), d_z.data_ptr(), y.data_ptr(), d_r.data_ptr(), m,
                                                True, ok.data_ptr(), sh)

        d_bad.copy_(d_be)
        d_bad[(m // 2) * n * 32 + 32 * 7 + 31] += 1  # one value of the middle blob
        d_ybad = d_y.clone()
        d_ybad[m // 2, 0] += 1
        torch.cuda.synchronize()
        verify_blobs(d_be, oks[0:])
        verify_blobs(d_bad, oks[1:])
        verify_points(d_y, oks[2:])
        verify_points(d_ybad, oks[3:])
        st.synchronize()
        t_verify = alternate(lambda: verify_blobs(d_be, oks[0:]), lambda: verify_points(d_y, oks[2:]))

        def evals_at():
            ctx.evals_at_device(d_be.data_ptr(), k, n, d_z.data_ptr(), m, d_y2.data_ptr(), bytes_mode=True,
                                bitrev=True, stream=sh)

        def ntt_quotient():
            ctx.ntt_device(d_limbs.data_ptr(), n, d_coef.data_ptr(), n, k, m, inverse=True, bitrev=True, stream=sh)
            ctx.quotient_single_device(d_coef.data_ptr(), n, n, d_z.data_ptr(), m, d_q.data_ptr(), n - 1,
                                       d_y.data_ptr(), stream=sh)

        d_y2.zero_()
        t_value = alternate(evals_at, ntt_quotient)
        st.synchronize()
        value_same = bool((d_y[:m] == d_y2[:m]).all().item())

        def challenges():
            ctx.blob_challenges_device(d_be.data_ptr(), k, m, d_crec.data_ptr(), d_z2.data_ptr(), d_ok.data_ptr(),
                                       bytes_mode=True, bitrev=True, stream=sh)

        def challenges_wall():
            challenges()
            st.synchronize()

        host_z = []

        def copy_and_hashlib():
            host = d_be[:m * n * 32].cpu().numpy().tobytes()
            recs = d_crec[:m * 48].cpu().numpy().tobytes()
            head = b"FSBLOBVERIFY_V1_" + n.to_bytes(16, "big")
            host_z[:] = [int.from_bytes(hashlib.sha256(head + host[b * n * 32:(b + 1) * n * 32] +
                                                       recs[48 * b:48 * b + 48]).digest(), "big") % R for b in range(m)]

        t_chal = alternate(challenges)
        t_wall = alternate(challenges_wall, copy_and_hashlib, timer=wall_ms)
        zd = d_z2[:m].cpu().numpy().view(np.uint64)
        z_same = [sum(int(r[i]) << (64 * i) for i in range(4)) for r in zd] == host_z and \
            bool((d_z2[:m] == d_z[:m]).all().item())

        row = {"blobs": m,
               "prove_blobs_batch_device": t_prove[0], "commit_evals_plus_prove_evals_z_supplied": t_prove[1],
               "prove_ratio": t_prove[0]["ms"] / t_prove[1]["ms"], "prove_extra_ms": t_prove[0]["ms"] - t_prove[1]["ms"],
               "prove_routes_agree": same,
               "verify_blobs_batch_device": t_verify[0], "verify_aggregate_checked_zy_supplied": t_verify[1],
               "verify_ratio": t_verify[0]["ms"] / t_verify[1]["ms"],
               "verify_extra_ms": t_verify[0]["ms"] - t_verify[1]["ms"],
               "valid_true_tampered_false": oks.tolist() == [1, 0, 1, 0],
               "evals_at_batch_device": t_value[0], "inverse_ntt_plus_quotient": t_value[1],
               "value_ratio": t_value[0]["ms"] / t_value[1]["ms"], "value_routes_agree": value_same,
               "blob_challenges_device": t_chal[0], "blob_challenges_device_wall": t_wall[0],
               "copy_to_host_plus_hashlib_wall": t_wall[1],
               "challenge_wall_ratio": t_wall[0]["ms"] / t_wall[1]["ms"], "z_equals_hashlib": z_same,
               "blobs_per_s_challenge": m / t_chal[0]["ms"] * 1e3}
        res["counts"][str(m)] = row
        sys.stderr.write(json.dumps(row) + "\n")

    ctx.close()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
