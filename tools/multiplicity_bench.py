#!/usr/bin/env python3
"""Device timings of bzamd_count_multiplicities_device, warm, on one GPU, beside two yardsticks on
the same lookup column in the same process, taken in turn: bzamd_combine_columns_device (the
streaming yardstick: reads the column, writes 32 bytes a row) and bzamd_invert_columns_device (the
call it sits beside in a proof).

    python tools/multiplicity_bench.py [--tables 256,65536,1048576] [--lookups 1048576,4194304]
                                       [--range-rows 33554432] [--samples 9] [--sample-ms 15]
                                       [--out FILE]

Hashed legs: both fields; tables of --tables rows of distinct keys, as i64 and as 32-byte elements;
lookup columns of --lookups rows of the table's own kind, every row a hit, in three distributions:
  uniform   rows drawn evenly from the whole table;
  hot       every row the same key (a constant column);
  keys256   rows drawn evenly from 256 of the table's keys (a byte-valued or enumerated column).
Range legs (--range-rows lookups, 0 to skip): the table 0 .. 255 on a u8 column and 0 .. 65535 on a
u16 column, uniform and hot.
A sample is `repeat` calls between two device events on the stream, divided by the repeat count;
`repeat` is chosen per leg after the warm-up so that a sample lasts --sample-ms, and --samples of
them are taken for the legs of a group in turn (count, combine, invert, count, ...), so that every
leg sees the same seconds of the same device.  Printed per leg, one JSON line (appended to --out,
default profiles/multiplicity_bench.jsonl): median, min and max in microseconds and the bytes the
call has to touch at least --
  count (hashed)  the lookups once, a slot and a table row per lookup, the table once and its slots
                  twice (clear, insert), the multiplicities once;
  count (range)   the lookups once, the multiplicities once;
  combine, invert the lookups once and 32 bytes a row out
-- and for `count` the ratio to either yardstick.  Needs a GPU: there is no CPU fallback."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mle_opening_bench import elements  # noqa: E402

DISTRIBUTIONS = ("uniform", "hot", "keys256")
KINDS = {"i64": (8, True), "element": (32, False)}


def slot_count(m):
    s = 2
    while s < 2 * m:
        s *= 2
    return s


class Group:
    """one table (None: the range table), one lookup column per distribution, the outputs"""

    def __init__(self, torch, api, m, n, kind, width=None, distributions=DISTRIBUTIONS):
        dev = torch.device("cuda", 0)
        self.torch, self.api, self.m, self.n, self.kind = torch, api, m, n, kind
        rng = np.random.default_rng(m + n)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.distributions = distributions
        index = {"uniform": lambda: torch.randint(0, m, (n,), device=dev),
                 "hot": lambda: torch.full((n,), min(5, m - 1), dtype=torch.int64, device=dev),
                 "keys256": lambda: torch.randint(0, 256, (n,), device=dev) * max(m // 256, 1)}
        if kind == "range":
            self.width, self.signed, self.table = width, False, None
            dtype = torch.uint8 if width == 1 else torch.int16
            self.lookups = {d: index[d]().to(dtype) for d in distributions}
            self.workspace_bytes, self.workspace = 0, None
        else:
            self.width, self.signed = KINDS[kind]
            # distinct keys: an odd multiple of a permutation; as elements, three more words that
            # follow from the first, the top one short enough for the value to stay below p
            keys = torch.randperm(m, device=dev) * 0x9E3779B1 + 12345
            if kind == "element":
                keys = torch.stack([keys, keys * 0x2545F4914F6CDD1D, keys * 0x27BB2EE687B0B0FD,
                                    (keys * 0x369DEA0F31A53F85 >> 8) & ((1 << 55) - 1)], dim=1)
            self.table = keys.contiguous()
            self.lookups = {d: self.table[index[d]()].contiguous() for d in distributions}
            self.workspace_bytes = api.count_multiplicities_workspace_bytes(m)
            self.workspace = torch.empty(self.workspace_bytes, dtype=torch.uint8, device=dev)
        self.multiplicities = torch.zeros(m, dtype=torch.int64, device=dev)
        self.misses = torch.zeros(1, dtype=torch.int64, device=dev)
        self.out = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        self.one = {f: up(elements(rng, f, 1)) for f in (0, 1)}
        torch.cuda.synchronize()

    def call(self, what, distribution, field_id, stream):
        lookups = (self.lookups[distribution].data_ptr(), self.n, self.width, self.signed)
        if what == "count":
            table = (None if self.table is None else self.table.data_ptr(), self.m,
                     8 if self.table is None else self.width, self.signed)
            self.api.count_multiplicities_device(
                field_id, self.multiplicities.data_ptr(), self.misses.data_ptr(), table, lookups,
                None if self.workspace is None else self.workspace.data_ptr(),
                self.workspace_bytes, stream=stream)
        elif what == "combine":
            self.api.combine_columns_device(field_id, [lookups], self.one[field_id].data_ptr(),
                                            self.n, self.out.data_ptr(), stream=stream)
        else:
            self.api.invert_columns_device(field_id, self.out.data_ptr(), None, [lookups], None,
                                           self.one[field_id].data_ptr(), self.n, stream=stream)

    def check(self, distribution, field_id):
        """every lookup is a hit: the counts add up to n and nothing is missed"""
        stream = self.torch.cuda.current_stream().cuda_stream
        self.call("count", distribution, field_id, stream)
        self.torch.cuda.synchronize()
        assert int(self.multiplicities.sum()) == self.n and int(self.misses[0]) == 0, (
            self.kind, self.m, self.n, distribution, field_id)

    def bytes(self, what):
        read = self.n * self.width
        if what != "count":
            return read + 32 * self.n
        if self.table is None:
            return read + 8 * self.m
        return (read + self.n * (4 + self.width) + self.m * self.width
                + 2 * 4 * slot_count(self.m) + 8 * self.m)


def sample_us(torch, target, key, repeat):
    stream = torch.cuda.current_stream()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(stream)
    for _ in range(repeat):
        target.call(*key, stream.cuda_stream)
    end.record(stream)
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / repeat


def measure(torch, target, order, samples, sample_ms):
    """-> {key: (us per call of every sample, repeat)}; the legs in turn"""
    repeat = {}
    for key in order:
        sample_us(torch, target, key, 2)
        once = sample_us(torch, target, key, 4)
        repeat[key] = max(4, math.ceil(sample_ms * 1e3 / max(once, 1.0)))
    us = {key: [] for key in order}
    for _ in range(samples):
        for key in order:
            us[key].append(sample_us(torch, target, key, repeat[key]))
    return {key: (us[key], repeat[key]) for key in order}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", default="256,65536,1048576")
    ap.add_argument("--lookups", default="1048576,4194304")
    ap.add_argument("--range-rows", type=int, default=32 * 1048576)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--sample-ms", type=float, default=15.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multiplicity_bench.jsonl"))
    args = ap.parse_args()
    from inner_product_bench import Worker  # torch first, then the library, the GPU backend
    worker = Worker()
    torch, api = worker.torch, worker.api
    assert hasattr(api.load(), "bzamd_count_multiplicities_device"), "no multiplicity count here"
    tables = [int(x) for x in args.tables.split(",") if x]
    sizes = [int(x) for x in args.lookups.split(",") if x]

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    def run(group, table_name):
        order = [(what, d, f) for d in group.distributions for f in (0, 1)
                 for what in ("count", "combine", "invert")]
        for d in group.distributions:
            for f in (0, 1):
                group.check(d, f)
        got = measure(torch, group, order, args.samples, args.sample_ms)
        for what, d, f in order:
            us, repeat = got[(what, d, f)]
            median = statistics.median(us)
            rec = {"m": group.m, "n": group.n, "table": table_name, "lookup_width": group.width,
                   "distribution": d, "call": what, "field_id": f, "samples": len(us),
                   "repeat": repeat, "median_us": round(median, 2), "min_us": round(min(us), 2),
                   "max_us": round(max(us), 2), "bytes": group.bytes(what)}
            rec["gb_per_s"] = round(rec["bytes"] / median / 1e3, 1)
            if what == "count":
                for yardstick in ("combine", "invert"):
                    rec["ratio_to_" + yardstick] = round(
                        median / statistics.median(got[(yardstick, d, f)][0]), 2)
            emit(rec)

    if tables and sizes:
        warm = Group(torch, api, max(tables), max(sizes), "i64")
        t_end = time.perf_counter() + 1.0
        while time.perf_counter() < t_end:
            for what in ("count", "combine", "invert"):
                warm.call(what, "uniform", 0, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        del warm
    for n in sizes:
        for m in tables:
            for kind in KINDS:
                run(Group(torch, api, m, n, kind), kind)
    if args.range_rows:
        for m, width in ((256, 1), (65536, 2)):
            run(Group(torch, api, m, args.range_rows, "range", width, ("uniform", "hot")), "range")


if __name__ == "__main__":
    main()
