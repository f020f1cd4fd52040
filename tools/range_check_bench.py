#!/usr/bin/env python3
"""Device timings of the range check's word columns, warm, on one GPU: bzamd_decompose_words_device
and bzamd_map_words_device beside the two ways a caller had before them, on the same planes in the
same process, taken in turn, and bzamd_combine_columns_device on the same column as the streaming
yardstick (reads the column, writes 32 bytes a row).

    python tools/range_check_bench.py [--rows 65536,1048576,4194304] [--samples 9]
                                      [--sample-ms 15] [--out FILE]

Columns: i64 with the shift 2^63 (8 words), i128 (16 words) and 32-byte elements (31 words), both
fields.  Inputs: uniform keys, small values (below 2^16: the upper words are zero) and a constant
column.  Legs of a group:
  decompose      bzamd_decompose_words_device: planes, counts and overflow in one call;
  count_planes   (A) what gave the counts before: bzamd_count_multiplicities_device in its range
                 form (table 0 .. 255), once a plane, on planes that are already there;
  map            (B) one inversion of the 256-row table 1 / (alpha + v) and bzamd_map_words_device
                 over all planes;
  invert_planes  (B) what gave the inverse-word columns before: bzamd_invert_columns_device once a
                 plane;
  combine        the yardstick.
A sample is `repeat` calls between two device events on the stream, divided by the repeat count;
`repeat` is chosen per leg after the warm-up so that a sample lasts --sample-ms, and --samples of
them are taken for the legs of a group in turn, so that every leg sees the same seconds of the same
device.  Before a group is timed its results are checked against each other: the counts add up to
num_words n, the per-plane range counts add up to the counts, a mapped column equals the inverted
plane byte for byte.  Printed per leg, one JSON line (appended to --out, default
profiles/range_check_bench.jsonl): median, min and max in microseconds, the bytes the call has to
touch at least, and for decompose and map the ratio to the earlier way with that way's max - min
beside it.  Needs a GPU: there is no CPU fallback."""
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

from mle_opening_bench import MODULUS, elements  # noqa: E402
from multiplicity_bench import measure  # noqa: E402

KINDS = {"i64": (8, True, 8), "i128": (16, True, 16), "element": (32, False, 31)}
INPUTS = ("uniform", "small", "constant")
LEGS = ("decompose", "count_planes", "map", "invert_planes", "combine")
EARLIER = {"decompose": "count_planes", "map": "invert_planes"}


def element_form(field_id, value):
    p = MODULUS[field_id]
    value = value * (1 << 256) % p if field_id == 1 else value % p
    return np.frombuffer(value.to_bytes(32, "little"), np.uint8)


class Group:
    """one column, its planes, and the outputs of every leg"""

    def __init__(self, torch, api, kind, n, input_name, field_id):
        dev = torch.device("cuda", 0)
        self.torch, self.api, self.kind, self.n, self.field_id = torch, api, kind, n, field_id
        self.width, self.signed, self.num_words = KINDS[kind]
        rng = np.random.default_rng(n)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        width = self.width
        if kind == "element":
            # small values and the constant through a table of element forms; uniform keys are
            # random bytes below 2^248 (field 1: whatever they mean, the key is uniform too)
            if input_name == "uniform":
                column = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev)
                column[:, 31] = 0
            else:
                forms = up(np.stack([element_form(field_id, v) for v in range(1 << 16)]))
                index = (torch.randint(0, 1 << 16, (n,), device=dev) if input_name == "small"
                         else torch.full((n,), 12345, dtype=torch.int64, device=dev))
                column = forms[index].contiguous()
        else:
            column = torch.zeros((n, width), dtype=torch.uint8, device=dev)
            if input_name == "uniform":
                column = torch.randint(0, 256, (n, width), dtype=torch.uint8, device=dev)
                if kind == "i128":
                    column[:, width - 1] &= 0x7F   # non-negative: a negative i128 is p - |x|
            elif input_name == "small":
                column[:, :2] = torch.randint(0, 256, (n, 2), dtype=torch.uint8, device=dev)
            else:
                column[:, :3] = up(np.array([0x39, 0x30, 0x01], np.uint8))
        self.column = column
        self.shift = up(element_form(field_id, 1 << 63)) if kind == "i64" else None
        self.planes = torch.zeros((self.num_words, n), dtype=torch.uint8, device=dev)
        self.counts = torch.zeros(257, dtype=torch.int64, device=dev)
        self.plane_counts = torch.zeros((self.num_words, 257), dtype=torch.int64, device=dev)
        self.bytes256 = up(np.arange(256, dtype=np.uint8))
        self.alpha = up(elements(rng, field_id, 1))
        self.one = up(element_form(field_id, 1))
        self.table = torch.zeros((256, 32), dtype=torch.uint8, device=dev)
        self.mapped = torch.empty((self.num_words, n, 32), dtype=torch.uint8, device=dev)
        self.out = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

    def call(self, what, stream):
        api, f, n = self.api, self.field_id, self.n
        if what == "decompose":
            api.decompose_words_device(
                f, self.planes.data_ptr(), self.counts.data_ptr(), self.counts.data_ptr() + 2048,
                (self.column.data_ptr(), n, self.width, self.signed), self.num_words, n,
                shift_ptr=None if self.shift is None else self.shift.data_ptr(), stream=stream)
        elif what == "count_planes":
            for k in range(self.num_words):
                api.count_multiplicities_device(
                    f, self.plane_counts[k].data_ptr(), self.plane_counts[k].data_ptr() + 2048,
                    (None, 256, 8, False), (self.planes[k].data_ptr(), n, 1, False), None, 0,
                    stream=stream)
        elif what == "map":
            api.invert_columns_device(f, self.table.data_ptr(), None,
                                      [(self.bytes256.data_ptr(), 256, 1, False)], None,
                                      self.alpha.data_ptr(), 256, stream=stream)
            api.map_words_device(self.mapped.data_ptr(), self.planes.data_ptr(),
                                 self.table.data_ptr(), self.num_words, n, n, 32 * n, stream=stream)
        elif what == "invert_planes":
            for k in range(self.num_words):
                api.invert_columns_device(f, self.out.data_ptr(), None,
                                          [(self.planes[k].data_ptr(), n, 1, False)], None,
                                          self.alpha.data_ptr(), n, stream=stream)
        else:
            api.combine_columns_device(f, [(self.column.data_ptr(), n, self.width, self.signed)],
                                       self.one.data_ptr(), n, self.out.data_ptr(), stream=stream)

    def check(self):
        """the legs agree with each other before they are timed"""
        torch = self.torch
        stream = torch.cuda.current_stream().cuda_stream
        for what in ("decompose", "count_planes", "map", "invert_planes"):
            self.call(what, stream)
        torch.cuda.synchronize()
        where = (self.kind, self.n, self.field_id)
        assert int(self.counts[:256].sum()) == self.num_words * self.n, where
        assert not bool(self.plane_counts[:, 256].any()), where
        assert torch.equal(self.plane_counts[:, :256].sum(dim=0), self.counts[:256]), where
        # invert_planes leaves the last plane's inverses
        assert torch.equal(self.mapped[self.num_words - 1], self.out), where

    def bytes(self, what):
        n, planes = self.n, self.num_words * self.n
        return {"decompose": n * self.width + planes + 2056,
                "count_planes": planes + 2056 * self.num_words,
                "map": 33 * planes + 256 * 33,
                "invert_planes": 33 * planes,
                "combine": n * self.width + 32 * n}[what]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="65536,1048576,4194304")
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--sample-ms", type=float, default=15.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_check_bench.jsonl"))
    args = ap.parse_args()
    from inner_product_bench import Worker  # torch first, then the library, the GPU backend
    worker = Worker()
    torch, api = worker.torch, worker.api
    assert hasattr(api.load(), "bzamd_decompose_words_device"), "no word columns here"
    sizes = [int(x) for x in args.rows.split(",") if x]

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    class Target:
        def __init__(self, group):
            self.group = group

        def call(self, what, stream):
            self.group.call(what, stream)

    warm = Group(torch, api, "i64", max(sizes), "uniform", 0)
    t_end = time.perf_counter() + 1.0
    while time.perf_counter() < t_end:
        for what in ("decompose", "map", "combine"):
            warm.call(what, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    del warm
    for n in sizes:
        for kind in KINDS:
            for input_name in INPUTS:
                for field_id in (0, 1):
                    group = Group(torch, api, kind, n, input_name, field_id)
                    group.check()
                    got = measure(torch, Target(group), [(what,) for what in LEGS], args.samples,
                                  args.sample_ms)
                    for what in LEGS:
                        us, repeat = got[(what,)]
                        median = statistics.median(us)
                        rec = {"n": n, "column": kind, "num_words": group.num_words,
                               "input": input_name, "field_id": field_id, "call": what,
                               "samples": len(us), "repeat": repeat,
                               "median_us": round(median, 2), "min_us": round(min(us), 2),
                               "max_us": round(max(us), 2), "bytes": group.bytes(what)}
                        rec["gb_per_s"] = round(rec["bytes"] / median / 1e3, 1)
                        if what in EARLIER:
                            earlier = got[(EARLIER[what],)][0]
                            rec["earlier"] = EARLIER[what]
                            rec["ratio_to_earlier"] = round(median / statistics.median(earlier), 3)
                            rec["earlier_max_minus_min_us"] = round(max(earlier) - min(earlier), 2)
                        emit(rec)
                    del group
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
