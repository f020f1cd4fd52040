#!/usr/bin/env python3
"""Device timings of the univariate-opening stages, warm, on one GPU: bzamd_fold_polynomial_device,
bzamd_evaluate_polynomials_device and bzamd_batch_quotients_device on resident operands, beside the
bytes they move, the project's own streaming yardstick and, for field 1, the two MSM calls they
feed.

    python tools/univariate_opening_bench.py [--sizes 65536,1048576,4194304] [--samples 15]
                                             [--repeat 10] [--out FILE] [--no-msm]

Legs per size n (l = ceil_log2(n), three points), on both fields, after two untimed calls each,
taken in turn so that every leg sees the same minutes of the same device:
  fold       P_1 .. P_{l-1} in element and scalar form and the evaluation: P_0 and the levels 10
             and 20 read, every level written twice;
  evaluate   all l polynomials at three points: every level read once;
  quotients  the three quotients of the combination, B made on the fly: every level read twice, 3 n
             rows written;
  yardstick  bzamd_evaluate_columns_device of one 32-byte column against a vector of n elements:
             64 n bytes read.  Each stage's bytes / time is printed next to this leg's.
A sample is `--repeat` calls between two device events on the stream, divided by the repeat count;
printed per size and leg, one JSON line (appended to --out, default
profiles/univariate_opening_bench.jsonl): median, min and max in microseconds, the bytes moved, the
bandwidth the median implies and its ratio to the yardstick's.  Before the first sample the device
runs the largest size's legs for a second, so the clock is warm.

Field 1 only, unless --no-msm: bzamd_msm_device over bn254 with generators (i + 1) G from
bzamd_generator_multiples_device, on the scalars the stages wrote: `msm_levels`, l - 1 columns of
len_i rows, and `msm_quotients`, 3 columns of n rows; the host clock around enqueue and
synchronise, --samples times after one warm call.  Needs a GPU: there is no CPU fallback."""
import argparse
import ctypes
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
BN254_P = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
BN254 = 2           # SXT_CURVE_BN_254
NUM_POINTS = 3
FOLD_LEVELS = 10    # kFoldLevels of proof/univariate_opening.hip: the levels a launch reads again
STAGES = ("fold", "evaluate", "quotients", "yardstick")


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


def stage_bytes(n, num_variables, layout):
    """bytes each stage moves, from the shapes"""
    rows = sum(length for _, length in layout)
    lengths = [n] + [length for _, length in layout]
    again = sum(lengths[i] for i in range(FOLD_LEVELS, num_variables, FOLD_LEVELS))
    return {"fold": 32 * (n + again + 2 * rows) + 32 * num_variables + 32,
            "evaluate": 32 * (n + rows) + 32 * NUM_POINTS * (1 + num_variables),
            "quotients": 2 * 32 * (n + rows) + 32 * NUM_POINTS * n,
            "yardstick": 64 * n}


class Legs:
    """the resident operands of one size and the calls on them"""

    def __init__(self, torch, api, n):
        dev = torch.device("cuda", 0)
        self.torch, self.api, self.n = torch, api, n
        self.v = max((n - 1).bit_length(), 1)
        self.layout = api.folded_layout(n, self.v)
        rows = sum(length for _, length in self.layout)
        rng = np.random.default_rng(n)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        empty = lambda r: torch.empty((max(r, 1), 32), dtype=torch.uint8, device=dev)  # noqa: E731
        # random bytes cut to 250 bits are canonical elements of either field: the arithmetic does
        # not depend on the values
        self.polynomial = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev)
        self.polynomial[:, 31] &= 0x03
        self.vector = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev)
        self.vector[:, 31] &= 0x03
        self.folded, self.scalars = empty(rows), empty(rows)
        self.evaluation, self.evaluations = empty(1), empty(NUM_POINTS * self.v)
        self.quotients, self.remainders = empty(NUM_POINTS * n), empty(NUM_POINTS)
        self.yard = empty(1)
        self.point = {f: up(elements(rng, f, self.v)) for f in (0, 1)}
        self.points = {f: up(elements(rng, f, NUM_POINTS)) for f in (0, 1)}
        self.q = {f: up(elements(rng, f, 1)) for f in (0, 1)}
        self.bytes = stage_bytes(n, self.v, self.layout)
        self.workspace = {}
        for f in (0, 1):
            for stage, size in (
                    ("evaluate", api.evaluate_polynomials_workspace_bytes(f, n, self.v, NUM_POINTS)),
                    ("quotients", api.batch_quotients_workspace_bytes(f, n, self.v, NUM_POINTS)),
                    ("yardstick", api.evaluate_columns_workspace_bytes(f, 1, n))):
                self.workspace[(stage, f)] = (torch.empty(size, dtype=torch.uint8, device=dev), size)

    def call(self, stage, f, stream):
        api, n, v = self.api, self.n, self.v
        if stage == "fold":
            api.fold_polynomial_device(f, self.folded.data_ptr(), self.scalars.data_ptr(),
                                       self.evaluation.data_ptr(), self.polynomial.data_ptr(), n,
                                       self.point[f].data_ptr(), v, stream=stream)
            return
        workspace, size = self.workspace[(stage, f)]
        if stage == "evaluate":
            api.evaluate_polynomials_device(f, self.evaluations.data_ptr(),
                                            self.polynomial.data_ptr(), self.folded.data_ptr(), n, v,
                                            self.points[f].data_ptr(), NUM_POINTS,
                                            workspace.data_ptr(), size, stream=stream)
        elif stage == "quotients":
            api.batch_quotients_device(f, self.quotients.data_ptr(), self.remainders.data_ptr(),
                                       self.polynomial.data_ptr(), self.folded.data_ptr(), n, v,
                                       self.q[f].data_ptr(), self.points[f].data_ptr(), NUM_POINTS,
                                       workspace.data_ptr(), size, stream=stream)
        else:
            api.evaluate_columns_device(f, [(self.polynomial.data_ptr(), n, 32, False)],
                                        self.vector.data_ptr(), n, self.yard.data_ptr(),
                                        workspace.data_ptr(), size, stream=stream)

    def sample_us(self, stage, f, repeat):
        torch = self.torch
        stream = torch.cuda.current_stream()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        for _ in range(repeat):
            self.call(stage, f, stream.cuda_stream)
        end.record(stream)
        end.synchronize()
        return start.elapsed_time(end) * 1e3 / repeat

    def msm_legs(self, samples):
        """field 1: the commitments the stages feed, over generators (i + 1) G"""
        torch, api, n = self.torch, self.api, self.n
        lib = api.load()
        dev = self.polynomial.device
        stream = torch.cuda.current_stream().cuda_stream
        vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        r = (1 << 256) % BN254_P
        base = np.zeros(72, np.uint8)
        base[:64] = np.frombuffer((1 * r % BN254_P).to_bytes(32, "little")
                                  + (2 * r % BN254_P).to_bytes(32, "little"), np.uint8)
        d_base = torch.from_numpy(base).to(dev)
        generators = torch.empty((n, 72), dtype=torch.uint8, device=dev)
        lib.bzamd_generator_multiples_device(BN254, vp(generators), vp(d_base), n,
                                             ctypes.c_void_p(stream))
        # the scalars of field 1
        self.call("fold", 1, stream)
        self.call("quotients", 1, stream)
        torch.cuda.synchronize()
        columns = {
            "msm_levels": [(self.scalars.data_ptr() + 32 * offset, length)
                           for offset, length in self.layout],
            "msm_quotients": [(self.quotients.data_ptr() + 32 * n * k, n)
                              for k in range(NUM_POINTS)]}
        out = {}
        for leg, cols in columns.items():
            if not cols:
                continue
            desc = (api.sxt_sequence_descriptor * len(cols))()
            for i, (ptr, rows) in enumerate(cols):
                desc[i] = api.sxt_sequence_descriptor(32, rows, ptr, 0)
            result = torch.empty((len(cols), 72), dtype=torch.uint8, device=dev)
            ms = []
            for sample in range(samples + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lib.bzamd_msm_device(BN254, vp(result), len(cols), desc, vp(generators),
                                     ctypes.c_void_p(stream))
                torch.cuda.synchronize()
                if sample > 0:  # the first call is warm-up: the engine's buffers grow there
                    ms.append((time.perf_counter() - t0) * 1e3)
            out[leg] = (len(cols), sum(rows for _, rows in cols), ms)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,1048576,4194304")
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--no-msm", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "univariate_opening_bench.jsonl"))
    args = ap.parse_args()
    assert args.samples >= 15, "at least 15 samples"
    from inner_product_bench import Worker  # torch first, then the library, the GPU backend
    worker = Worker()
    torch, api = worker.torch, worker.api
    assert hasattr(api.load(), "bzamd_batch_quotients_device"), \
        "this build has no univariate openings"
    sizes = [int(x) for x in args.sizes.split(",")]
    order = [(stage, f) for stage in STAGES for f in (0, 1)]

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")

    warm = Legs(torch, api, max(sizes))
    t_end = time.perf_counter() + 1.0
    while time.perf_counter() < t_end:
        for stage, f in order:
            warm.call(stage, f, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    del warm
    for n in sizes:
        legs = Legs(torch, api, n)
        for stage, f in order:
            legs.sample_us(stage, f, 2)
        us = {key: [] for key in order}
        for _ in range(args.samples):
            for stage, f in order:
                us[(stage, f)].append(legs.sample_us(stage, f, args.repeat))
        rate = {key: legs.bytes[key[0]] / statistics.median(us[key]) / 1e3 for key in order}
        for stage, f in order:
            median = statistics.median(us[(stage, f)])
            emit({"n": n, "num_variables": legs.v, "leg": stage, "field_id": f,
                  "num_points": 0 if stage in ("fold", "yardstick") else NUM_POINTS,
                  "samples": args.samples, "repeat": args.repeat, "median_us": round(median, 2),
                  "min_us": round(min(us[(stage, f)]), 2), "max_us": round(max(us[(stage, f)]), 2),
                  "bytes": legs.bytes[stage], "gb_per_s": round(rate[(stage, f)], 1),
                  "yardstick_gb_per_s": round(rate[("yardstick", f)], 1),
                  "of_yardstick": round(rate[(stage, f)] / rate[("yardstick", f)], 2)})
        if not args.no_msm:
            for leg, (columns, rows, ms) in legs.msm_legs(args.samples).items():
                emit({"n": n, "num_variables": legs.v, "leg": leg, "field_id": 1, "curve": "bn254",
                      "columns": columns, "rows": rows, "samples": args.samples,
                      "median_us": round(statistics.median(ms) * 1e3, 1),
                      "min_us": round(min(ms) * 1e3, 1), "max_us": round(max(ms) * 1e3, 1)})
        del legs


if __name__ == "__main__":
    main()
