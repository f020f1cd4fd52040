#!/usr/bin/env python3
"""Device timings of bzamd_invert_columns_device, warm, on one GPU, beside
bzamd_combine_columns_device on the same columns in the same process, taken in turn.

    python tools/column_inverse_bench.py [--sizes 65536,1048576,4194304] [--samples 15]
                                         [--sample-ms 25] [--chain-size 1048576] [--out FILE]

Legs per size n, on both fields, each as `invert` (the inverse column in element form) and as
`combine` (the streaming yardstick: the same reads and the same 32 n byte write, one product a row
and column and one on the way out):
  one_i64    one signed 8-byte column with a shift (the yardstick: coefficient 1);
  four_i64   four signed 8-byte columns with coefficients and a shift;
  one_32     one column of 32-byte elements with a shift.
A sample is `repeat` calls between two device events on the stream, divided by the repeat count;
`repeat` is chosen per leg after the warm-up so that a sample lasts --sample-ms, and --samples of
them are taken for every leg in turn (invert f0, combine f0, invert f1, ..., then again), so that
every leg sees the same minutes of the same device: 15 x 25 ms = 375 ms of timed calls a leg.
Printed per size and leg, one JSON line (appended to --out, default
profiles/column_inverse_bench.jsonl): median, min and max in microseconds, the bytes the algorithm
moves, the field products counted in the head comment of proof/column_inverse.hip (invert:
K + 3.12 a row and one inversion per 2048 rows, counted apart; combine: K + 1), and for `invert`
the measured ratio to the yardstick beside the ratio of the product counts.

--chain-size: at that n, field 0, what the inverse column feeds, timed the same way: the inverse
column with both outputs, the one-column bzamd_msm_device over `scalars` with resident generators,
and bzamd_prove_sumcheck_transcript_device_columns over {c, inverses} with the products
1 * c * inv + alpha * inv.  Needs a GPU: there is no CPU fallback."""
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

LEGS = {"one_i64": (1, 8), "four_i64": (4, 8), "one_32": (1, 32)}  # columns, width
TILE_ROWS = 2048           # kInverseTile of proof/column_inverse.hip
INVERT_ROW_PRODUCTS = 3.12  # beside one per column: prefix, the walk back, the tile's tree


class Legs:
    """the resident operands of one size and the two calls on them"""

    def __init__(self, torch, api, n):
        dev = torch.device("cuda", 0)
        self.torch, self.api, self.n = torch, api, n
        rng = np.random.default_rng(n)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.out = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        self.scalars = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        # random bytes serve as i64 rows and, cut to 250 bits, as canonical elements of either
        # field: the arithmetic does not depend on the values
        self.i64 = [torch.randint(0, 256, (n, 8), dtype=torch.uint8, device=dev) for _ in range(4)]
        self.wide = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev)
        self.wide[:, 31] &= 0x03
        self.coefficients = {f: up(elements(rng, f, 4)) for f in (0, 1)}
        self.shift = {f: up(elements(rng, f, 1)) for f in (0, 1)}
        self.descriptors = {
            "one_i64": [(self.i64[0].data_ptr(), n, 8, True)],
            "four_i64": [(c.data_ptr(), n, 8, True) for c in self.i64],
            "one_32": [(self.wide.data_ptr(), n, 32, False)]}

    def call(self, what, leg, field_id, stream):
        if what == "invert":
            self.api.invert_columns_device(
                field_id, self.out.data_ptr(), None, self.descriptors[leg],
                self.coefficients[field_id].data_ptr() if leg == "four_i64" else None,
                self.shift[field_id].data_ptr(), self.n, stream=stream)
        else:
            self.api.combine_columns_device(field_id, self.descriptors[leg],
                                            self.coefficients[field_id].data_ptr(), self.n,
                                            self.out.data_ptr(), stream=stream)


class Chain:
    """field 0: the inverse column of one i64 column in both forms, and what reads them"""
    LEGS = ("invert_both", "msm_one_column", "sumcheck_c_inv")

    def __init__(self, torch, api, n):
        dev = torch.device("cuda", 0)
        self.torch, self.api, self.n = torch, api, n
        rng = np.random.default_rng(n + 1)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.column = torch.randint(0, 256, (n, 8), dtype=torch.uint8, device=dev)
        self.alpha_bytes = elements(rng, 0, 1)
        self.alpha = up(self.alpha_bytes)
        self.inverses = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        self.scalars = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        self.generators = torch.empty((n, 160), dtype=torch.uint8, device=dev)
        api.load().bzamd_ristretto255_generators_device(
            self.generators.data_ptr(), 0, n, torch.cuda.current_stream(dev).cuda_stream)
        self.commitment = torch.zeros(32, dtype=torch.uint8, device=dev)
        self.scalar_desc = (api.sxt_sequence_descriptor * 1)(
            api.sxt_sequence_descriptor(32, n, self.scalars.data_ptr(), 0))
        one = np.zeros(32, np.uint8)
        one[0] = 1
        # the product table: a multiplier and the number of its terms per product
        self.table = np.zeros((2, api.SUMCHECK_PRODUCT_STRIDE[0]), np.uint8)
        for i, (multiplier, length) in enumerate(((one, 2), (self.alpha_bytes[0], 1))):
            self.table[i, :32] = multiplier
            self.table[i, 32:36] = np.frombuffer(np.uint32(length).tobytes(), np.uint8)
        self.terms = [0, 1, 1]
        v = max((n - 1).bit_length(), 1)
        self.polys = torch.zeros((v, 3, 32), dtype=torch.uint8, device=dev)
        self.point = torch.zeros((v, 32), dtype=torch.uint8, device=dev)
        self.evaluations = torch.zeros((2, 32), dtype=torch.uint8, device=dev)
        self.transcript0 = up(api.transcript_new("column inverse bench"))
        self.transcript = torch.zeros_like(self.transcript0)
        self.workspace_bytes = api.sumcheck_transcript_columns_workspace_bytes(0, n, 2, 2, 3, 2)
        self.workspace = torch.empty(self.workspace_bytes, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

    def call(self, what, leg, field_id, stream):
        api, n = self.api, self.n
        if leg == "invert_both":
            api.invert_columns_device(0, self.inverses.data_ptr(), self.scalars.data_ptr(),
                                      [(self.column.data_ptr(), n, 8, True)], None,
                                      self.alpha.data_ptr(), n, stream=stream)
        elif leg == "msm_one_column":
            api.load().bzamd_msm_device(0, self.commitment.data_ptr(), 1, self.scalar_desc,
                                        self.generators.data_ptr(), stream)
        else:
            self.transcript.copy_(self.transcript0)
            api.prove_sumcheck_transcript_device_columns(
                0, [(self.column.data_ptr(), n, 8, True), (self.inverses.data_ptr(), n, 32, False)],
                self.table, self.terms, n, 2, self.polys.data_ptr(), self.point.data_ptr(),
                self.evaluations.data_ptr(), self.transcript.data_ptr(),
                self.workspace.data_ptr(), self.workspace_bytes, stream=stream)


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
    ap.add_argument("--sizes", default="65536,1048576,4194304")
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--sample-ms", type=float, default=25.0)
    ap.add_argument("--chain-size", type=int, default=1048576)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "column_inverse_bench.jsonl"))
    args = ap.parse_args()
    from inner_product_bench import Worker  # torch first, then the library, the GPU backend
    worker = Worker()
    torch, api = worker.torch, worker.api
    assert hasattr(api.load(), "bzamd_invert_columns_device"), "this build has no column inversion"
    sizes = [int(x) for x in args.sizes.split(",") if x]
    order = [(what, leg, f) for leg in LEGS for f in (0, 1) for what in ("invert", "combine")]

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    def record(n, what, leg, f, us, repeat):
        median = statistics.median(us)
        return {"n": n, "call": what, "leg": leg, "field_id": f, "samples": len(us),
                "repeat": repeat, "median_us": round(median, 2), "min_us": round(min(us), 2),
                "max_us": round(max(us), 2)}

    if sizes:
        warm = Legs(torch, api, max(sizes))
        t_end = time.perf_counter() + 1.0
        while time.perf_counter() < t_end:
            for key in order:
                warm.call(*key, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        del warm
    for n in sizes:
        legs = Legs(torch, api, n)
        got = measure(torch, legs, order, args.samples, args.sample_ms)
        for what, leg, f in order:
            us, repeat = got[(what, leg, f)]
            columns, width = LEGS[leg]
            rec = record(n, what, leg, f, us, repeat)
            rec["columns"] = columns
            rec["bytes"] = columns * width * n + 32 * n
            rec["gb_per_s"] = round(rec["bytes"] / rec["median_us"] / 1e3, 1)
            if what == "invert":
                rec["field_products"] = round((columns + INVERT_ROW_PRODUCTS) * n)
                rec["inversions"] = (n + TILE_ROWS - 1) // TILE_ROWS
                yardstick = statistics.median(got[("combine", leg, f)][0])
                rec["ratio_to_combine"] = round(rec["median_us"] / yardstick, 2)
                rec["counted_ratio"] = round((columns + INVERT_ROW_PRODUCTS) / (columns + 1), 2)
            else:
                rec["field_products"] = (columns + 1) * n
            emit(rec)
        del legs
    if args.chain_size:
        n = args.chain_size
        chain = Chain(torch, api, n)
        chain_order = [("chain", leg, 0) for leg in Chain.LEGS]
        got = measure(torch, chain, chain_order, args.samples, args.sample_ms)
        for key in chain_order:
            us, repeat = got[key]
            emit(record(n, "chain", key[1], 0, us, repeat))


if __name__ == "__main__":
    main()
