#!/usr/bin/env python3
"""Per call of the sumcheck prover in a rocprofv3 --kernel-trace csv: what happens before round 1
-- the conversion (k_sumcheck_load), round 0 and the first fold -- and the call's kernel time in
all, for the engine-form path and the columns path side by side.

    rocprofv3 --kernel-trace --output-format csv -d <dir> -o r -- \
        python tools/sumcheck_bench.py <n> <degree> <products> <samples> --fields 0 --column-bytes 8
    python tools/prof/sumcheck_first_round.py <dir>/**/r_kernel_trace.csv <calls per leg>

A call starts at a k_sumcheck_load (engine-form tables) or at a k_sumcheck_columns_round /
k_sumcheck_columns_generic (typed columns).  tools/sumcheck_bench.py makes `calls per leg` =
samples + 1 calls of each leg in the order host, device, columns, columns32; the first call of a
leg (warm-up) is left out of the medians.  Prints one JSON line per leg, microseconds."""
import csv
import json
import statistics
import sys


def short(name):
    for key in ("k_sumcheck_columns_round", "k_sumcheck_columns_generic", "k_sumcheck_columns_fold",
                "k_sumcheck_load", "k_sumcheck_round", "k_sumcheck_finish", "k_sumcheck_fold"):
        if key in name:
            return key
    return None


def main():
    path, per_leg = sys.argv[1], int(sys.argv[2])
    ev = []
    for r in csv.DictReader(open(path)):
        name = short(r["Kernel_Name"])
        if name is not None:
            ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name))
    ev.sort()
    calls = []
    for start, end, name in ev:
        if name in ("k_sumcheck_load", "k_sumcheck_columns_round", "k_sumcheck_columns_generic"):
            calls.append({"kind": "tables" if name == "k_sumcheck_load" else "columns", "ev": []})
        if calls:
            calls[-1]["ev"].append((name, (end - start) / 1e3))
    legs = {"tables": ["host", "device"], "columns": ["columns", "columns32"]}
    for kind, names in legs.items():
        mine = [c for c in calls if c["kind"] == kind]
        for k, leg in enumerate(names):
            rows = []
            for c in mine[k * per_leg + 1:(k + 1) * per_leg]:
                e = c["ev"]
                load = e[0][1] if kind == "tables" else 0.0
                rounds = [d for n, d in e if "round" in n or "generic" in n]
                folds = [d for n, d in e if n.endswith("fold")]
                rows.append({"load_us": load, "round0_us": rounds[0], "first_fold_us": folds[0],
                             "before_round1_us": load + rounds[0] + folds[0],
                             "kernels_us": sum(d for _, d in e), "kernels": len(e)})
            if rows:
                print(json.dumps({"leg": leg, "calls": len(rows),
                                  **{key: round(statistics.median(r[key] for r in rows), 2)
                                     for key in rows[0]}}))


if __name__ == "__main__":
    main()
