#!/usr/bin/env python3
"""Per-step summary of a two-stream block-table run's kernel trace.

    python3 scripts/joint_timeline.py TRACE.csv [--steps 20] [--json OUT] [--trim OUT.csv]

TRACE.csv is a rocprofv3 --kernel-trace CSV of bench.py (cfg2 / cfg3 / cfg4).
The window is the last --steps steps: from the start of the first of their
2 x steps accumulations to the end of the last.  Printed: the duration of
each tail kernel inside it (median, min, max, per stream), per step the time
with two accumulations resident, with one and with none, and how long the
next accumulation has run when one ends.  --trim writes the trace's
rows of that window alone (every kernel, the setup's dropped): the form kept
under profiles/."""
import argparse
import csv
import json
import statistics

TAILS = ("k_joint_index", "k_joint_horner1", "k_joint_horner2_glv", "k_joint_horner2", "k_joint_finish_glv",
         "k_fixed_finish", "k_quotient_single", "k_joint_accum")


def short(name):
    for t in TAILS:
        if "::" + t + "<" in name or "::" + t + "(" in name:
            return t
    return None


def overlap(ivs):
    """(ms with >= 2 intervals open, ms with exactly 1, first start, last end) of [(start, end)] in ns"""
    ev = sorted([(s, 1) for s, _ in ivs] + [(e, -1) for _, e in ivs])
    two = one = 0
    cur, last = 0, ev[0][0]
    for t, d in ev:
        if cur >= 2:
            two += t - last
        elif cur == 1:
            one += t - last
        cur += d
        last = t
    return two / 1e6, one / 1e6, ev[0][0], ev[-1][0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trim", default=None)
    a = ap.parse_args()
    rows = []
    with open(a.trace, newline="") as f:
        for r in csv.DictReader(f):
            k = short(r["Kernel_Name"])
            if k:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), k, r.get("Stream_Id", r["Queue_Id"])))
    rows.sort()
    acc = [r for r in rows if r[2] == "k_joint_accum"]
    per_step = 2
    n = a.steps * per_step
    if len(acc) < n + per_step:
        raise SystemExit("trace holds %d accumulations, fewer than %d steps" % (len(acc), a.steps))
    acc = acc[-n:]
    t0, t1 = acc[0][0], acc[-1][1]
    win = [r for r in rows if r[0] >= t0 and r[1] <= t1]
    out = {"trace": a.trace, "steps": a.steps, "window_ms": (t1 - t0) / 1e6, "ms_per_step": (t1 - t0) / 1e6 / a.steps,
           "kernels": {}}
    for k in TAILS:
        for stream in sorted({r[3] for r in win if r[2] == k}):
            d = [(r[1] - r[0]) / 1e6 for r in win if r[2] == k and r[3] == stream]
            if d:
                out["kernels"]["%s@stream%s" % (k, stream)] = {
                    "launches": len(d), "median_ms": round(statistics.median(d), 4), "min_ms": round(min(d), 4),
                    "max_ms": round(max(d), 4)}
    two, one, _, _ = overlap([(r[0], r[1]) for r in acc])
    span = (t1 - t0) / 1e6
    out["accum_resident_ms_per_step"] = {"two": round(two / a.steps, 4), "one": round(one / a.steps, 4),
                                         "none": round((span - two - one) / a.steps, 4)}
    # the overlap at each launch's end: how long the next accumulation (either stream) has run when this one ends
    ends = []
    for i, r in enumerate(acc[:-1]):
        nxt = acc[i + 1]
        ends.append(max(0.0, (r[1] - nxt[0]) / 1e6))
    out["overlap_at_launch_end_ms"] = {"median": round(statistics.median(ends), 4), "min": round(min(ends), 4),
                                       "max": round(max(ends), 4)}
    if a.trim:
        with open(a.trace, newline="") as f, open(a.trim, "w", newline="") as g:
            rd = csv.DictReader(f)
            wr = csv.DictWriter(g, fieldnames=rd.fieldnames, quoting=csv.QUOTE_NONNUMERIC)
            wr.writeheader()
            for r in rd:
                if int(r["Start_Timestamp"]) >= t0 and int(r["End_Timestamp"]) <= t1:
                    wr.writerow({k: (int(v) if v.lstrip("-").isdigit() else v) for k, v in r.items()})
    text = json.dumps(out, indent=1)
    print(text)
    if a.json:
        with open(a.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
