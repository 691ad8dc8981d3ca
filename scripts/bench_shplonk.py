#!/usr/bin/env python3
"""Shplonk openings (kzgx_shplonk_commit_device + kzgx_shplonk_open_device, kzgx_shplonk_verify_device)
against what a caller does without them, on one MI355X, in one process, both curves.

Shape: a proof-system table.  25 polynomials of n coefficients, T = {z, z w, z / w}; 20 polynomials are
opened at {z}, 4 at {z, z w} and 1 at all three.  n = 4096 and n = 2^20.
  (1) whole call.  Shplonk: commit + open (one proof of 2 G1 points) and verify.  Before:
      kzgx_prove_multi_batch_device with one group per point of T (25, 5 and 1 claims; 3 G1 points) and
      kzgx_verify_multi_batch_device on those groups.
  (2) the fused quotient kernels alone (the library's own event span "shplonk_quotient" inside the commit
      call) against the chain of single-point divisions they replace, built from the exported entry
      kzgx_quotient_single_batch_device: max d_s rounds, ping-ponging between two buffers, each round over
      the sets that still have a point left.  Both sides start from folded polynomials F_s in device memory
      (random canonical scalars: the time does not depend on the values).  The chain's last step, the sum of
      the per-set quotients, is NOT run: no exported entry adds polynomials, so the chain's figure lacks it.
      A second shape: 8 sets of 16 points, one claim each.
Device pointers and device events throughout; the legs alternate inside one loop after a warm-up of each;
median / min / max of --reps.  Every timed proof is first verified by the library (ok = 1) and one wrong
value is refuted (ok = 0); the tests, not this script, compare against the integer model.

    python scripts/bench_shplonk.py [--out profiles/shplonk.json] [--ns 4096,1048576] [--curves BN254,BLS12381]
Prints one JSON line (and writes it to --out after every case); progress goes to stderr."""
import argparse
import json
import os
import statistics
import sys

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
    ap.add_argument("--ns", default="4096,1048576")
    ap.add_argument("--curves", default="BN254,BLS12381")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_shplonk: no GPU (nothing is measured on a CPU)")
    import kzg_ref as K
    import kzgx

    reps = max(args.reps, 5)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    sh = st.cuda_stream
    rng = np.random.default_rng(0x5A9107)

    def scalars(count):
        v = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64)
        v[:, 3] &= np.uint64((1 << 60) - 1)  # < r on both curves
        return v

    def to_dev(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.int64 if a.dtype == np.uint64 else np.int32)).to(dev)

    def u32(v):
        return to_dev(np.array(list(v), dtype=np.uint32))

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        return a.elapsed_time(b)

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

    res = {"metric": "Shplonk openings against one batch-opening proof per point, and the fused multi-point "
                     "quotient against the chain of single-point divisions",
           "timing": "device pointers, device events around the enqueue on one stream (the quotient kernels: the "
                     "library's event span inside the commit call), legs alternating in one loop, median [min, max] "
                     "of %d after one warm-up of each" % reps,
           "device": torch.cuda.get_device_name(0),
           "proof_size_g1_points": {"shplonk": 2, "one_batch_proof_per_point": 3}, "cases": {}}

    def flush():
        line = json.dumps(res)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return line

    for name in [c for c in args.curves.split(",") if c]:
        C = getattr(K, name)
        tau = K.default_tau(C)
        nl = 4 if name == "BN254" else 6
        for n in [int(x) for x in args.ns.split(",") if x]:
            ctx = kzgx.Context(name)
            ctx.gen_srs(tau, n)
            ctx.gen_srs_g2(tau, 2)
            n_polys = 25
            polys = scalars(n_polys * n).reshape(n_polys, n, 4)
            commits = np.zeros((n_polys, 2 * nl), dtype=np.uint64)
            for j in range(n_polys):
                commits[j], inf = ctx.msm(polys[j])
                assert not inf
            d_polys, d_commits = to_dev(polys), to_dev(commits)
            T = scalars(3)
            d_T, d_z, d_gamma = to_dev(T), to_dev(scalars(1)), to_dev(scalars(1))  # d_T: the route before

            def shplonk_case(sets, T, label, whole):
                """sets: (point indices, polynomial indices) over the points T; times the quotient span against the
                chain and, with whole, commit + open and verify"""
                d_T = to_dev(T)
                sps, sp, cs, ix = [0], [], [0], []
                for pts, cl in sets:
                    sp += pts
                    ix += cl
                    sps.append(len(sp))
                    cs.append(len(ix))
                count, nv, ns = len(ix), sum(len(a) * len(b) for a, b in sets), len(sets)
                d_sps, d_sp, d_cs, d_ix = u32(sps), u32(sp), u32(cs), u32(ix)
                W = torch.zeros((2, 2 * nl), dtype=torch.int64, device=dev)  # W then W'
                Winf = torch.zeros((2,), dtype=torch.int32, device=dev)
                h = torch.zeros((n, 4), dtype=torch.int64, device=dev)
                y = torch.zeros((max(nv, 1), 4), dtype=torch.int64, device=dev)
                ok = torch.zeros((2,), dtype=torch.int32, device=dev)
                table = (d_T.data_ptr(), len(T), d_sps.data_ptr(), d_sp.data_ptr(), len(sp), d_cs.data_ptr())

                def commit():
                    ctx.shplonk_commit_device(d_polys.data_ptr(), n, n, n_polys, *table, d_ix.data_ptr(), ns,
                                              d_gamma.data_ptr(), count, nv, W.data_ptr(), Winf.data_ptr(),
                                              h.data_ptr(), y.data_ptr(), ok.data_ptr(), powers=True, stream=sh)

                def prove():
                    commit()
                    ctx.shplonk_open_device(d_polys.data_ptr(), n, n, n_polys, *table, d_ix.data_ptr(), ns,
                                            d_gamma.data_ptr(), count, h.data_ptr(), d_z.data_ptr(),
                                            W[1].data_ptr(), Winf[1:].data_ptr(), None, None, powers=True, stream=sh)

                def verify(vals=None, out=None):
                    ctx.shplonk_verify_device(d_commits.data_ptr(), None, n_polys, d_ix.data_ptr(), *table, ns,
                                              (y if vals is None else vals).data_ptr(), nv, d_gamma.data_ptr(), count,
                                              d_z.data_ptr(), W.data_ptr(), Winf.data_ptr(),
                                              (ok if out is None else out)[1:].data_ptr(), powers=True, stream=sh)

                prove()
                bad, okb = y.clone(), torch.zeros((2,), dtype=torch.int32, device=dev)
                bad[0, 0] += 1
                verify()
                verify(bad, okb)
                st.synchronize()
                right = ok.tolist() == [1, 1] and okb.tolist()[1] == 0

                def quotient_span():
                    ctx.prof_clear()
                    ctx.prof_enable(True)
                    commit()
                    st.synchronize()
                    ms = ctx.prof_read("shplonk_quotient")[0]
                    ctx.prof_enable(False)
                    ctx.prof_clear()
                    return ms

                # the chain: F_s rows (random scalars), max d_s rounds of single-point divisions, the sets with the
                # most points first so that every round is one batched call over a prefix of the rows
                order = sorted(range(ns), key=lambda s: -len(sets[s][0]))
                dmax = len(sets[order[0]][0])
                F = to_dev(scalars(ns * n).reshape(ns, n, 4))
                buf = [F.clone(), F.clone()]
                rounds = []
                for j in range(min(dmax, n - 1)):
                    act = [s for s in order if len(sets[s][0]) > j]
                    rounds.append((len(act), to_dev(T[[sets[s][0][j] for s in act]])))

                def chain():
                    for j, (na, zs) in enumerate(rounds):
                        src, dst = (F if j == 0 else buf[j & 1]), buf[(j + 1) & 1]
                        ctx.quotient_single_device(src.data_ptr(), n - j, n, zs.data_ptr(), na, dst.data_ptr(), n, None,
                                                   stream=sh)

                legs = {"quotient_fused": (quotient_span, lambda fn: fn()), "quotient_chain": (chain, event_ms)}
                if whole:
                    legs.update({"shplonk_prove": (prove, event_ms), "shplonk_verify": (verify, event_ms)})
                t = alternate(legs)
                out = {"sets_points_claims": [[len(a), len(b)] for a, b in sets], "claims": count, "values": nv,
                       "answers_right": right, "fused_quotient_kernels": t["quotient_fused"],
                       "single_division_chain_without_the_final_sum": dict(t["quotient_chain"], rounds=len(rounds)),
                       "fused_over_chain": t["quotient_fused"]["ms"] / t["quotient_chain"]["ms"]}
                if whole:
                    out.update({"shplonk_commit_plus_open": t["shplonk_prove"], "shplonk_verify": t["shplonk_verify"]})
                note(name, n, label, json.dumps(out))
                return out

            table_sets = [([0], list(range(20))), ([0, 1], [20, 21, 22, 23]), ([0, 1, 2], [24])]
            case = {"n": n, "curve": name, "table": shplonk_case(table_sets, T, "table", True)}
            # the route before: one group per point of T
            groups = [list(range(25)), [20, 21, 22, 23, 24], [24]]
            gi = [j for g in groups for j in g]
            gs = [0, 25, 30, 31]
            d_gi, d_gs, d_gam3, d_ch = u32(gi), u32(gs), to_dev(scalars(3)), to_dev(scalars(3))
            P3 = torch.zeros((3, 2 * nl), dtype=torch.int64, device=dev)
            P3inf = torch.zeros((3,), dtype=torch.int32, device=dev)
            y3 = torch.zeros((31, 4), dtype=torch.int64, device=dev)
            ok3 = torch.zeros((2,), dtype=torch.int32, device=dev)

            def multi_prove():
                ctx.prove_multi_device(d_polys.data_ptr(), n, n, n_polys, d_gi.data_ptr(), d_gs.data_ptr(), 3,
                                       d_T.data_ptr(), d_gam3.data_ptr(), 31, P3.data_ptr(), P3inf.data_ptr(),
                                       y3.data_ptr(), None, ok3.data_ptr(), powers=True, stream=sh)

            def multi_verify():
                ctx.verify_multi_device(d_commits.data_ptr(), None, n_polys, d_gi.data_ptr(), d_gs.data_ptr(), 3,
                                        d_T.data_ptr(), y3.data_ptr(), d_gam3.data_ptr(), P3.data_ptr(),
                                        P3inf.data_ptr(), d_ch.data_ptr(), 31, ok3[1:].data_ptr(), powers=True,
                                        stream=sh)

            multi_prove()
            multi_verify()
            st.synchronize()
            t = alternate({"multi_prove": (multi_prove, event_ms), "multi_verify": (multi_verify, event_ms)})
            case["one_batch_proof_per_point"] = {"groups": [25, 5, 1], "answers_right": ok3.tolist() == [1, 1],
                                                 "prove_multi_batch_device": t["multi_prove"],
                                                 "verify_multi_batch_device": t["multi_verify"]}
            case["prove_shplonk_over_before"] = case["table"]["shplonk_commit_plus_open"]["ms"] / t["multi_prove"]["ms"]
            case["verify_shplonk_over_before"] = case["table"]["shplonk_verify"]["ms"] / t["multi_verify"]["ms"]
            note(name, n, "before", json.dumps(case["one_batch_proof_per_point"]))
            res["cases"]["%s n=%d" % (name, n)] = case
            flush()
            # the second quotient shape: 8 sets of 16 points, one claim each
            sets16 = [(list(range(16 * q, 16 * q + 16)), [q]) for q in range(8)]
            case["eight_sets_of_16_points"] = shplonk_case(sets16, scalars(128), "8 sets of 16", False)
            flush()
            ctx.close()
            del d_polys, polys
            torch.cuda.empty_cache()
    # said plainly: where the new path loses
    loses = []
    for key, c in res["cases"].items():
        if c["prove_shplonk_over_before"] > 1:
            loses.append({"case": key, "what": "commit + open is slower than one batch proof per point",
                          "ratio": c["prove_shplonk_over_before"]})
        if c["verify_shplonk_over_before"] > 1:
            loses.append({"case": key, "what": "verify is slower than the batch openings' verify",
                          "ratio": c["verify_shplonk_over_before"]})
        for shape in ("table", "eight_sets_of_16_points"):
            if c[shape] and c[shape]["fused_over_chain"] > 1:
                loses.append({"case": key, "shape": shape,
                              "what": "the fused quotient kernels are slower than the chain of single divisions "
                                      "(which lacks its final sum)", "ratio": c[shape]["fused_over_chain"]})
    res["loses"] = loses
    note("loses:", json.dumps(loses))
    print(flush(), flush=True)


if __name__ == "__main__":
    main()
