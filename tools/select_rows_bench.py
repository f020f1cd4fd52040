#!/usr/bin/env python3
"""Device timings of bzamd_select_rows_device and bzamd_take_rows_device, warm, on one GPU, beside
two yardsticks in the same process, taken in turn: a device-to-device copy of the bytes the call
must move, and bzamd_combine_columns_device on the same columns (the streaming yardstick of the
other tools: reads the columns, writes 32 bytes a row).

    python tools/select_rows_bench.py [--rows 65536,1048576,4194304] [--columns u8,i64,4xi64,element]
                                      [--samples 15] [--repeat 10] [--out FILE]

Selection: a u8 selector (reject 0) over --rows rows with one u8, one i64, four i64 or one 32-byte
column, keep rates 0, 1/64, 1/2, 63/64 and 1, the kept rows `scattered` (every row drawn on its
own) or in `runs` (whole blocks of 1024 rows drawn), capacity = rows, with and without zero_tail;
count is asked for, indices are not; every selection is taken in both store shapes, `shape` a (each
kept lane stores its row) and b (a tile's kept rows packed in LDS, whole 16-byte pieces), which
bzamd_select_rows_packed_width switches.  Gather: the same columns taken at `rows` indices, a sorted
and a random draw from all rows.  A sample is --repeat calls between two device events on the
stream, divided by the repeat count; --samples of them are taken for the legs of a group in turn
(select a, select b, copy, combine, select a, ...), so that every leg sees the same seconds of the
same device.
Printed per leg, one JSON line (appended to --out, default profiles/select_rows_bench.jsonl):
median, min and max in microseconds and the bytes the call must move --
  select   the selector once, the kept rows read and the kept rows written (with zero_tail: the
           rows of the tail written as well);
  take     the indices once, every row read and written;
  copy     one hipMemcpy device to device of half those bytes: it reads them and writes them;
  combine  the columns once and 32 bytes a row out
-- and for select and take `of_copy`, the copy's median over the leg's: the fraction of the
copy's rate the call reaches on the same bytes.  Needs a GPU: there is no CPU fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mle_opening_bench import elements  # noqa: E402
from multiplicity_bench import sample_us  # noqa: E402

COLUMNS = {"u8": [(1, False)], "i64": [(8, True)], "4xi64": [(8, True)] * 4,
           "element": [(32, False)]}
RATES = {"0": 0.0, "1/64": 1 / 64, "1/2": 0.5, "63/64": 63 / 64, "1": 1.0}
RUN = 1024


class Group:
    """n rows of one column set: a selector per (rate, layout), two index columns, the outputs"""

    def __init__(self, torch, api, n, columns):
        dev = torch.device("cuda", 0)
        self.torch, self.api, self.n, self.name = torch, api, n, columns
        self.kinds = COLUMNS[columns]
        self.row_bytes = sum(width for width, _ in self.kinds)
        rng = np.random.default_rng(n)
        self.columns = []
        for width, _ in self.kinds:
            if width == 32:
                few = torch.from_numpy(elements(rng, 0, 4096)).to(dev)
                self.columns.append(few[torch.randint(0, 4096, (n,), device=dev)].contiguous())
            else:
                self.columns.append(torch.randint(0, 256, (n, width), dtype=torch.uint8, device=dev))
        self.selectors, self.kept = {}, {}
        for rate, p in RATES.items():
            for layout in ("scattered", "runs"):
                if layout == "runs" and p in (0.0, 1.0):
                    continue
                if layout == "scattered":
                    flags = torch.rand(n, device=dev) < p
                else:
                    flags = (torch.rand((n + RUN - 1) // RUN, device=dev) < p).repeat_interleave(
                        RUN)[:n]
                self.selectors[(rate, layout)] = flags.to(torch.uint8).contiguous()
                self.kept[(rate, layout)] = int(flags.sum())
        random = torch.randint(0, n, (n,), device=dev, dtype=torch.int32)
        self.indices = {"random": random, "sorted": random.sort().values.contiguous()}
        self.selected = [torch.empty((n, width), dtype=torch.uint8, device=dev)
                         for width, _ in self.kinds]
        self.count = torch.zeros(1, dtype=torch.int64, device=dev)
        self.workspace_bytes = api.select_rows_workspace_bytes(n)
        self.workspace = torch.empty(self.workspace_bytes, dtype=torch.uint8, device=dev)
        self.combined = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        self.ones = torch.from_numpy(np.tile(elements(rng, 0, 1), (len(self.kinds), 1))).to(dev)
        most = n * (1 + 4 + 2 * self.row_bytes)
        self.copy_from = torch.empty(most // 2 + 1, dtype=torch.uint8, device=dev)
        self.copy_to = torch.empty(most // 2 + 1, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

    def descriptors(self):
        return [(c.data_ptr(), self.n, width, signed)
                for c, (width, signed) in zip(self.columns, self.kinds)]

    def bytes(self, what, case):
        n = self.n
        if what == "combine":
            return n * self.row_bytes + 32 * n
        if case[0] == "take":
            return 4 * n + 2 * n * self.row_bytes
        _, rate, layout, zero_tail = case
        kept = self.kept[(rate, layout)]
        return n + 2 * kept * self.row_bytes + (n - kept) * self.row_bytes * (1 if zero_tail else 0)

    def call(self, what, case, stream):
        if what == "combine":
            self.api.combine_columns_device(0, self.descriptors(), self.ones.data_ptr(), self.n,
                                            self.combined.data_ptr(), stream=stream)
        elif what == "copy":
            # on the current stream, which is the one the legs are timed on
            half = self.bytes("call", case) // 2
            self.copy_to[:half].copy_(self.copy_from[:half], non_blocking=True)
        elif case[0] == "take":
            self.api.take_rows_device(self.indices[case[1]].data_ptr(), self.n, self.descriptors(),
                                      [s.data_ptr() for s in self.selected], stream=stream)
        else:
            # shape (a): every column one row a lane; shape (b): every column packed in LDS
            _, rate, layout, zero_tail = case
            self.api.select_rows_packed_width(32 if what == "call_b" else 0)
            self.api.select_rows_device(
                self.count.data_ptr(), None,
                (self.selectors[(rate, layout)].data_ptr(), self.n, 1, False), self.descriptors(),
                [s.data_ptr() for s in self.selected], self.n, self.workspace.data_ptr(),
                self.workspace_bytes, zero_tail=zero_tail, stream=stream)

    def check(self, case, what="call"):
        """the count is the number of set flags and the first column's kept rows are where they
        belong (with zero_tail: zeros behind them); a gather's first column is the rows asked for"""
        torch = self.torch
        if case[0] == "take":
            self.call("call", case, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            at = self.indices[case[1]].long()
            assert bool((self.selected[0] == self.columns[0][at]).all()), (self.n, self.name, case)
            return
        _, rate, layout, zero_tail = case
        self.selected[0].fill_(0x5A)
        self.call(what, case, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        kept = self.kept[(rate, layout)]
        assert int(self.count[0]) == kept, (self.n, self.name, case)
        rows = self.selectors[(rate, layout)].nonzero().reshape(-1)
        assert bool((self.selected[0][:kept] == self.columns[0][rows]).all()), (self.n, self.name,
                                                                                  case)
        if zero_tail:
            assert not bool(self.selected[0][kept:].any())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="65536,1048576,4194304")
    ap.add_argument("--columns", default="u8,i64,4xi64,element")
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_rows_bench.jsonl"))
    args = ap.parse_args()
    from inner_product_bench import Worker  # torch first, then the library, the GPU backend
    worker = Worker()
    torch, api = worker.torch, worker.api
    assert hasattr(api.load(), "bzamd_select_rows_device"), "no row selection here"
    sizes = [int(x) for x in args.rows.split(",") if x]
    column_sets = [x for x in args.columns.split(",") if x]

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    def run(group):
        cases = [("select", rate, layout, zero_tail) for (rate, layout) in group.selectors
                 for zero_tail in (False, True)]
        cases += [("take", "sorted"), ("take", "random")]
        for case in cases:
            calls = ["call_a", "call_b"] if case[0] == "select" else ["call"]
            for what in calls:
                group.check(case, what)
            order = [(what, case) for what in calls + ["copy", "combine"]]
            for key in order:
                sample_us(torch, group, key, 2)
            us = {key: [] for key in order}
            for _ in range(args.samples):
                for key in order:
                    us[key].append(sample_us(torch, group, key, args.repeat))
            copy_median = statistics.median(us[("copy", case)])
            for what, _ in order:
                got = us[(what, case)]
                median = statistics.median(got)
                rec = {"n": group.n, "columns": group.name, "call": case[0] if what.startswith("call")
                       else what, "samples": len(got), "repeat": args.repeat,
                       "median_us": round(median, 2), "min_us": round(min(got), 2),
                       "max_us": round(max(got), 2)}
                if case[0] == "select":
                    rec.update({"keep": case[1], "layout": case[2], "zero_tail": case[3],
                                "kept": group.kept[(case[1], case[2])]})
                else:
                    rec["indices"] = case[1]
                rec["bytes"] = group.bytes(what, case)
                rec["gb_per_s"] = round(rec["bytes"] / median / 1e3, 1)
                if what.startswith("call"):
                    rec["of_copy"] = round(copy_median / median, 3)
                if what in ("call_a", "call_b"):
                    rec["shape"] = what[-1]
                emit(rec)

    warm = Group(torch, api, max(sizes), column_sets[0])
    t_end = time.perf_counter() + 1.0
    while time.perf_counter() < t_end:
        for what in ("call_a", "call_b", "copy", "combine"):
            warm.call(what, ("select", "1/2", "scattered", True),
                      torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    del warm
    for n in sizes:
        for columns in column_sets:
            run(Group(torch, api, n, columns))


if __name__ == "__main__":
    main()
