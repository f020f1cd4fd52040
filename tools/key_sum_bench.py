#!/usr/bin/env python3
"""Device timings of bzamd_sum_by_key_device, warm, on one GPU, beside two yardsticks in the same
process, taken in turn: bzamd_count_multiplicities_device on the same key columns (the same call
minus the sums) and bzamd_combine_columns_device on the value columns (the streaming yardstick:
reads the values, writes 32 bytes a row).

    python tools/key_sum_bench.py [--tables 16,256,65536,1048576] [--lookups 1048576,4194304]
                                  [--values i64,4xi64,element] [--samples 9] [--sample-ms 15]
                                  [--out FILE]

Tables of --tables rows of distinct i64 keys; lookup columns of --lookups rows, every row a hit, in
three distributions:
  uniform   rows drawn evenly from the whole table;
  hot       every row the same key (one group);
  keys256   rows drawn evenly from 256 of the table's keys (all of a smaller table).
Value columns (--values): one i64, four i64, one 32-byte column of canonical elements; random rows.
Both fields.  A sample is `repeat` calls between two device events on the stream, divided by the
repeat count; `repeat` is chosen per leg after the warm-up so that a sample lasts --sample-ms, and
--samples of them are taken for the legs of a group in turn (sum, count, combine, sum, ...), so
that every leg sees the same seconds of the same device.  Printed per leg, one JSON line (appended
to --out, default profiles/key_sum_bench.jsonl): median, min and max in microseconds, the bytes
the call has to touch at least --
  sum      the lookups once, a slot and a table row per lookup, the values once, the table once
           and its slots twice (clear, insert), the accumulators twice (clear, finish), sums,
           scalars, counts and matches once;
  count    as tools/multiplicity_bench.py;
  combine  the values once and 32 bytes a row out
-- and for `sum` the 64-bit adds of the value columns: `lds_adds` on chip (tables summed in bins
in LDS), `global_adds` to memory (an upper bound: zero chunks are skipped; bins in LDS: non-zero
bins per workgroup at its end; a hot key: one per wavefront, turn and accumulator), `busiest_word`
the adds that reach one accumulator, and the ratio to either yardstick.  Needs a GPU: there is no
CPU fallback."""
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

from mle_opening_bench import MODULUS, elements  # noqa: E402
from multiplicity_bench import measure, slot_count  # noqa: E402

DISTRIBUTIONS = ("uniform", "hot", "keys256")
VALUES = {"i64": [(8, True)], "4xi64": [(8, True)] * 4, "element": [(32, False)]}
THREADS, LDS_BLOCKS, BLOCKS, LDS_BINS, LDS_SUM_BINS = 256, 1024, 2048, 4096, 4096


class Group:
    """one table, one lookup column per distribution, the value columns, the outputs"""

    def __init__(self, torch, api, m, n, values):
        dev = torch.device("cuda", 0)
        self.torch, self.api, self.m, self.n, self.values = torch, api, m, n, values
        self.kinds = VALUES[values]
        self.row_chunks = sum((width + 3) // 4 for width, _ in self.kinds)
        rng = np.random.default_rng(m + n)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        index = {"uniform": lambda: torch.randint(0, m, (n,), device=dev),
                 "hot": lambda: torch.full((n,), min(5, m - 1), dtype=torch.int64, device=dev),
                 "keys256": lambda: (torch.randint(0, 256, (n,), device=dev) % m) * max(m // 256, 1)}
        self.table = (torch.randperm(m, device=dev) * 0x9E3779B1 + 12345).contiguous()
        self.lookups = {d: self.table[index[d]()].contiguous() for d in DISTRIBUTIONS}
        # value columns per field: a 32-byte column holds the field's own elements
        self.columns = {}
        for f in (0, 1):
            self.columns[f] = []
            for width, _ in self.kinds:
                if width == 32:
                    few = up(elements(rng, f, 4096))
                    self.columns[f].append(few[torch.randint(0, 4096, (n,), device=dev)].contiguous())
                else:
                    self.columns[f].append(torch.randint(-2**63, 2**63 - 1, (n,), dtype=torch.int64,
                                                         device=dev))
        count = len(self.kinds)
        self.workspace_bytes = api.sum_by_key_workspace_bytes(m, count)
        self.workspace = torch.empty(self.workspace_bytes, dtype=torch.uint8, device=dev)
        self.sums = torch.empty((count, m, 32), dtype=torch.uint8, device=dev)
        self.scalars = torch.empty((count, m, 32), dtype=torch.uint8, device=dev)
        self.counts = torch.zeros(m, dtype=torch.int64, device=dev)
        self.misses = torch.zeros(1, dtype=torch.int64, device=dev)
        self.matches = torch.empty(n, dtype=torch.int32, device=dev)
        self.out = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        self.ones = {f: up(np.tile(elements(rng, f, 1), (count, 1))) for f in (0, 1)}
        torch.cuda.synchronize()

    def descriptors(self, field_id):
        return [(c.data_ptr(), self.n, width, signed)
                for c, (width, signed) in zip(self.columns[field_id], self.kinds)]

    def call(self, what, distribution, field_id, stream):
        table = (self.table.data_ptr(), self.m, 8, True)
        lookups = (self.lookups[distribution].data_ptr(), self.n, 8, True)
        if what == "sum":
            self.api.sum_by_key_device(
                field_id, self.sums.data_ptr(), self.scalars.data_ptr(), self.counts.data_ptr(),
                self.misses.data_ptr(), self.matches.data_ptr(), table, lookups,
                self.descriptors(field_id), self.workspace.data_ptr(), self.workspace_bytes,
                stream=stream)
        elif what == "count":
            self.api.count_multiplicities_device(
                field_id, self.counts.data_ptr(), self.misses.data_ptr(), table, lookups,
                self.workspace.data_ptr(), self.workspace_bytes, stream=stream)
        else:
            self.api.combine_columns_device(field_id, self.descriptors(field_id),
                                            self.ones[field_id].data_ptr(), self.n,
                                            self.out.data_ptr(), stream=stream)

    def check(self, distribution, field_id):
        """every lookup is a hit: the counts add up to n, nothing is missed, and (tables of at most
        2^16 rows) the sums of a column over all groups are the sum of the column"""
        torch = self.torch
        self.call("sum", distribution, field_id, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert int(self.counts.sum()) == self.n and int(self.misses[0]) == 0, (
            self.m, self.n, self.values, distribution, field_id)
        assert bool((self.table[self.matches.long()] == self.lookups[distribution]).all())
        if self.m > 65536 or self.kinds[0][0] == 32:
            return
        p = MODULUS[field_id]
        rows = self.scalars[0].cpu().numpy()
        got = sum(int.from_bytes(bytes(r), "little") for r in rows) % p
        column = self.columns[field_id][0].cpu().numpy()
        want = ((int((column >> 32).sum()) << 32) + int((column & 0xFFFFFFFF).sum())) % p
        assert got == want, (self.m, self.n, self.values, distribution, field_id)

    def in_lds(self):
        return self.m <= LDS_BINS and self.m * self.row_chunks <= LDS_SUM_BINS

    def adds(self, distribution):
        """-> (lds_adds, global_adds, busiest_word): upper bounds from the shapes"""
        n, chunks = self.n, self.row_chunks
        groups = {"uniform": self.m, "hot": 1, "keys256": min(self.m, 256)}[distribution]
        if self.in_lds():
            blocks = min(LDS_BLOCKS, math.ceil(n / THREADS))
            return n * chunks, blocks * groups * chunks, blocks
        if distribution == "hot":
            turns = math.ceil(n / 64)
            return 0, turns * chunks, turns
        return 0, n * chunks, math.ceil(n / groups)

    def bytes(self, what):
        m, n = self.m, self.n
        value_bytes = n * sum(width for width, _ in self.kinds)
        probe = n * 8 + n * (4 + 8) + m * 8 + 2 * 4 * slot_count(m)
        if what == "combine":
            return value_bytes + 32 * n
        if what == "count":
            return probe + 8 * m
        return (probe + value_bytes + 2 * 8 * m * self.row_chunks
                + 2 * 32 * m * len(self.kinds) + 8 * m + 4 * n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", default="16,256,65536,1048576")
    ap.add_argument("--lookups", default="1048576,4194304")
    ap.add_argument("--values", default="i64,4xi64,element")
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--sample-ms", type=float, default=15.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "key_sum_bench.jsonl"))
    args = ap.parse_args()
    from inner_product_bench import Worker  # torch first, then the library, the GPU backend
    worker = Worker()
    torch, api = worker.torch, worker.api
    assert hasattr(api.load(), "bzamd_sum_by_key_device"), "no sums by key here"
    tables = [int(x) for x in args.tables.split(",") if x]
    sizes = [int(x) for x in args.lookups.split(",") if x]
    value_sets = [x for x in args.values.split(",") if x]

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    def run(group):
        order = [(what, d, f) for d in DISTRIBUTIONS for f in (0, 1)
                 for what in ("sum", "count", "combine")]
        for d in DISTRIBUTIONS:
            for f in (0, 1):
                group.check(d, f)
        got = measure(torch, group, order, args.samples, args.sample_ms)
        for what, d, f in order:
            us, repeat = got[(what, d, f)]
            median = statistics.median(us)
            rec = {"m": group.m, "n": group.n, "values": group.values, "distribution": d,
                   "call": what, "field_id": f, "samples": len(us), "repeat": repeat,
                   "median_us": round(median, 2), "min_us": round(min(us), 2),
                   "max_us": round(max(us), 2), "bytes": group.bytes(what)}
            rec["gb_per_s"] = round(rec["bytes"] / median / 1e3, 1)
            if what == "sum":
                rec["lds_adds"], rec["global_adds"], rec["busiest_word"] = group.adds(d)
                rec["in_lds"] = group.in_lds()
                for yardstick in ("count", "combine"):
                    rec["ratio_to_" + yardstick] = round(
                        median / statistics.median(got[(yardstick, d, f)][0]), 2)
            emit(rec)

    warm = Group(torch, api, max(tables), max(sizes), value_sets[0])
    t_end = time.perf_counter() + 1.0
    while time.perf_counter() < t_end:
        for what in ("sum", "count", "combine"):
            warm.call(what, "uniform", 0, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    del warm
    for n in sizes:
        for m in tables:
            for values in value_sets:
                run(Group(torch, api, m, n, values))


if __name__ == "__main__":
    main()
