#!/usr/bin/env python3
"""Device timings of the opening bridge, warm, on one GPU: bzamd_mle_evaluation_vector_device,
bzamd_combine_columns_device and bzamd_evaluate_columns_device on resident operands, beside the
bytes they move.

    python tools/mle_opening_bench.py [--sizes 65536,1048576,4194304] [--samples 15] [--repeat 10]
                                      [--inner-product-sizes 65536,1048576] [--out FILE]

Legs per size n (v = ceil_log2(n)), on both fields, after two untimed calls each, taken in turn
(vector f0, vector f1, combine_i64 f0, ..., then again) so that every leg sees the same minutes of
the same device:
  vector       the evaluation vector of a random point: 32 n bytes written;
  combine_i64  8 signed 8-byte columns of n rows with random coefficients and the product:
               64 n bytes read, 32 n written;
  combine_32   8 columns of 32-byte elements: 256 n bytes read, 32 n written;
  evaluate_i64 the evaluations of 16 signed 8-byte columns against a vector of n elements: 128 n
               bytes of columns and, at 8 columns to a launch, the vector twice, 64 n bytes;
  evaluate_32  the evaluations of 4 columns of 32-byte elements: 128 n bytes and the vector once.
The evaluation legs also print their field products (one per row and column).
A sample is `--repeat` calls between two device events on the stream, divided by the repeat count;
printed per size and leg, one JSON line (appended to --out): median, min and max in microseconds,
the bytes moved and the bandwidth the median implies.  Before the first sample the device runs the
largest size's legs for a second, so the clock is warm.

--inner-product-sizes: after the legs of such a size, bzamd_prove_inner_product_device at the same
n on the same device in the same process (tools/inner_product_bench.py Worker, device form with the
built-in generators, host clock around enqueue and synchronise), --samples times: what the opening
itself costs beside the bridge.  Needs a GPU: there is no CPU fallback."""
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

MODULUS = {0: 2**252 + 27742317777372353535851937790883648493,
           1: 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001}
NUM_COLUMNS = 8
EVALUATE_COLUMNS = {"evaluate_i64": 16, "evaluate_32": 4}
EVALUATE_CHUNK = 8  # kEvaluateChunk of proof/mle_opening.hip: the vector is read once per chunk


def elements(rng, field_id, count):
    """canonical elements in the caller's representation (field 1: Montgomery form, R = 2^256)"""
    p = MODULUS[field_id]
    out = np.zeros((count, 32), np.uint8)
    for i in range(count):
        v = int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % p
        if field_id == 1:
            v = v * (1 << 256) % p
        out[i] = np.frombuffer(v.to_bytes(32, "little"), np.uint8)
    return out


class Legs:
    """the resident operands of one size and the three calls on them"""

    def __init__(self, torch, api, n):
        dev = torch.device("cuda", 0)
        self.torch, self.api, self.n = torch, api, n
        self.v = max((n - 1).bit_length(), 1)
        rng = np.random.default_rng(n)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.out = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        self.product = torch.empty(32, dtype=torch.uint8, device=dev)
        # random bytes serve as i64 rows and, cut to 250 bits, as canonical elements of either
        # field: the arithmetic does not depend on the values
        self.i64 = [torch.randint(0, 256, (n, 8), dtype=torch.uint8, device=dev)
                    for _ in range(EVALUATE_COLUMNS["evaluate_i64"])]
        self.wide = []
        for _ in range(NUM_COLUMNS):
            column = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev)
            column[:, 31] &= 0x03
            self.wide.append(column)
        self.point = {f: up(elements(rng, f, self.v)) for f in (0, 1)}
        self.coefficients = {f: up(elements(rng, f, NUM_COLUMNS)) for f in (0, 1)}
        self.evaluations = {f: up(elements(rng, f, NUM_COLUMNS)) for f in (0, 1)}
        self.descriptors = {
            "combine_i64": [(c.data_ptr(), n, 8, True) for c in self.i64[:NUM_COLUMNS]],
            "combine_32": [(c.data_ptr(), n, 32, False) for c in self.wide],
            "evaluate_i64": [(c.data_ptr(), n, 8, True) for c in self.i64],
            "evaluate_32": [(c.data_ptr(), n, 32, False)
                            for c in self.wide[:EVALUATE_COLUMNS["evaluate_32"]]]}
        self.bytes = {"vector": 32 * n + 32 * self.v,
                      "combine_i64": NUM_COLUMNS * 8 * n + 32 * n,
                      "combine_32": NUM_COLUMNS * 32 * n + 32 * n}
        # the evaluation's vector (an element column serves) and its outputs and workspace
        self.b = self.wide[-1]
        self.evaluated = torch.empty((max(EVALUATE_COLUMNS.values()), 32), dtype=torch.uint8,
                                     device=dev)
        self.workspace = {}
        for leg, columns in EVALUATE_COLUMNS.items():
            width = 8 if leg == "evaluate_i64" else 32
            chunks = (columns + EVALUATE_CHUNK - 1) // EVALUATE_CHUNK
            self.bytes[leg] = columns * width * n + chunks * 32 * n + 32 * columns
            for f in (0, 1):
                size = api.evaluate_columns_workspace_bytes(f, columns, n)
                self.workspace[(leg, f)] = (torch.empty(size, dtype=torch.uint8, device=dev), size)

    def call(self, leg, field_id, stream):
        if leg == "vector":
            self.api.mle_evaluation_vector_device(field_id, self.out.data_ptr(),
                                                  self.point[field_id].data_ptr(), self.v, self.n,
                                                  stream=stream)
            return
        if leg in EVALUATE_COLUMNS:
            workspace, size = self.workspace[(leg, field_id)]
            self.api.evaluate_columns_device(field_id, self.descriptors[leg], self.b.data_ptr(),
                                             self.n, self.evaluated.data_ptr(), workspace.data_ptr(),
                                             size, stream=stream)
            return
        self.api.combine_columns_device(field_id, self.descriptors[leg],
                                        self.coefficients[field_id].data_ptr(), self.n,
                                        self.out.data_ptr(),
                                        evaluations_ptr=self.evaluations[field_id].data_ptr(),
                                        product_ptr=self.product.data_ptr(), stream=stream)

    def sample_us(self, leg, field_id, repeat):
        torch = self.torch
        stream = torch.cuda.current_stream()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        for _ in range(repeat):
            self.call(leg, field_id, stream.cuda_stream)
        end.record(stream)
        end.synchronize()
        return start.elapsed_time(end) * 1e3 / repeat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,1048576,4194304")
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--inner-product-sizes", default="")
    ap.add_argument("--out")
    args = ap.parse_args()
    from inner_product_bench import Worker  # torch first, then the library, the GPU backend
    worker = Worker()
    torch, api = worker.torch, worker.api
    assert hasattr(api.load(), "bzamd_combine_columns_device"), "this build has no opening bridge"
    sizes = [int(x) for x in args.sizes.split(",")]
    inner_product_sizes = [int(x) for x in args.inner_product_sizes.split(",") if x]
    assert hasattr(api.load(), "bzamd_evaluate_columns_device"), "this build has no evaluation"
    order = [(leg, f) for leg in ("vector", "combine_i64", "combine_32", "evaluate_i64",
                                  "evaluate_32") for f in (0, 1)]

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    warm = Legs(torch, api, max(sizes))
    t_end = time.perf_counter() + 1.0
    while time.perf_counter() < t_end:
        for leg, f in order:
            warm.call(leg, f, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    del warm
    for n in sizes:
        legs = Legs(torch, api, n)
        for leg, f in order:
            legs.sample_us(leg, f, 2)
        us = {key: [] for key in order}
        for _ in range(args.samples):
            for leg, f in order:
                us[(leg, f)].append(legs.sample_us(leg, f, args.repeat))
        for leg, f in order:
            median = statistics.median(us[(leg, f)])
            columns = 0 if leg == "vector" else EVALUATE_COLUMNS.get(leg, NUM_COLUMNS)
            rec = {"n": n, "leg": leg, "field_id": f, "columns": columns,
                   "samples": args.samples, "repeat": args.repeat, "median_us": round(median, 2),
                   "min_us": round(min(us[(leg, f)]), 2), "max_us": round(max(us[(leg, f)]), 2),
                   "bytes": legs.bytes[leg],
                   "gb_per_s": round(legs.bytes[leg] / median / 1e3, 1)}
            if leg in EVALUATE_COLUMNS:
                rec["field_products"] = columns * n
                rec["products_per_ns"] = round(columns * n / median / 1e3, 2)
            emit(rec)
        del legs
        if n in inner_product_sizes:
            worker.setup(n)
            worker.sample("device_builtin")  # warm: the engine's buffers grow here
            ms = [worker.sample("device_builtin")["ms"] for _ in range(args.samples)]
            emit({"n": n, "leg": "prove_inner_product_device", "field_id": 0,
                  "samples": args.samples, "median_us": round(statistics.median(ms) * 1e3, 1),
                  "min_us": round(min(ms) * 1e3, 1), "max_us": round(max(ms) * 1e3, 1)})


if __name__ == "__main__":
    main()
