#!/usr/bin/env python3
"""Per-column generator offsets on device-resident operands, warm (include/blitzar_amd.h,
bzamd_msm_device_offsets), built-in ristretto generators as the generator sequence:

  (a) C independent R-row sets -- column i on generators [i R, (i + 1) R) -- as ONE offsets call;
  (b) the same work as C bzamd_msm_device calls, one per column (the only way before the offsets);
  (c) C x R over ONE shared set of R generators: the offsets entry point with zero offsets, and
      the plain bzamd_msm_device call (the two must take the same time and give the same bytes).

    python tools/offsets_bench.py [--columns 64,256,1024] [--rows 256,1024,4096] [--reps 5]

Prints one JSON line per (columns, rows): ms per call of every case and the stage times
(bzamd_stage_timing_*: prepare, recode, sort, accumulate, reduce, combine; ms per call, (b): per
whole set of C calls), and checks that (a) == (b) and (c) offsets == (c) plain byte for byte.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch  # (before the library: torch's HIP runtime first, tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from blitzar_amd import api  # noqa: E402

STAGES = ["prepare", "recode", "sort", "accumulate", "reduce", "combine"]
GEN_BYTES = 160  # sxt_ristretto255


def timed(fn, reps, lib, stream):
    """ms per invocation of fn (warm: one untimed run first) and the stage times per invocation"""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / reps
    # the stage times in a run of their own (every recorded stage is an event pair)
    lib.bzamd_stage_timing_begin(1 << 20)
    fn()
    torch.cuda.synchronize()
    out = (ctypes.c_double * 6)()
    lib.bzamd_stage_timing_collect(out)
    return ms, {s: round(out[i], 4) for i, s in enumerate(STAGES)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--columns", default="64,256,1024")
    ap.add_argument("--rows", default="256,1024,4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    args = ap.parse_args()
    lib = api.load()
    lib.bzamd_stage_timing_collect.restype = ctypes.c_uint64
    lib.bzamd_kernel_launch_count.restype = ctypes.c_uint64
    api.reset_for_testing()
    assert api.init(api.SXT_GPU_BACKEND, 0) == 0
    dev = torch.device("cuda", 0)
    stream_ptr = torch.cuda.current_stream().cuda_stream
    stream = ctypes.c_void_p(stream_ptr)
    columns = [int(x) for x in args.columns.split(",")]
    rows_list = [int(x) for x in args.rows.split(",")]
    total = max(columns) * max(rows_list)
    d_gens = torch.empty((total, GEN_BYTES), dtype=torch.uint8, device=dev)
    lib.bzamd_ristretto255_generators_device(ctypes.c_void_p(d_gens.data_ptr()), 0, total, stream)
    rng = np.random.default_rng(1)
    d_scalars = torch.from_numpy(rng.integers(0, 256, (total, 32), dtype=np.uint8)).to(dev)
    torch.cuda.synchronize()
    lines = []
    for cols in columns:
        for rows in rows_list:
            desc = (api.sxt_sequence_descriptor * cols)()
            for i in range(cols):
                desc[i] = api.sxt_sequence_descriptor(32, rows, d_scalars.data_ptr() + 32 * i * rows, 0)
            one = [(api.sxt_sequence_descriptor * 1)() for _ in range(cols)]
            for i in range(cols):
                one[i][0] = desc[i]
            disjoint = np.arange(cols, dtype=np.uint64) * rows
            zeros = np.zeros(cols, dtype=np.uint64)
            p_disjoint = disjoint.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
            p_zeros = zeros.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
            outs = {k: torch.zeros((cols, 32), dtype=torch.uint8, device=dev)
                    for k in ("a", "b", "c_offsets", "c_plain")}
            gptr = d_gens.data_ptr()

            def case_a():
                lib.bzamd_msm_device_offsets(0, ctypes.c_void_p(outs["a"].data_ptr()), cols, desc,
                                             ctypes.c_void_p(gptr), cols * rows, p_disjoint, stream)

            def case_b():
                base = outs["b"].data_ptr()
                for i in range(cols):
                    lib.bzamd_msm_device(0, ctypes.c_void_p(base + 32 * i), 1, one[i],
                                         ctypes.c_void_p(gptr + GEN_BYTES * i * rows), stream)

            def case_c_offsets():
                lib.bzamd_msm_device_offsets(0, ctypes.c_void_p(outs["c_offsets"].data_ptr()), cols,
                                             desc, ctypes.c_void_p(gptr), rows, p_zeros, stream)

            def case_c_plain():
                lib.bzamd_msm_device(0, ctypes.c_void_p(outs["c_plain"].data_ptr()), cols, desc,
                                     ctypes.c_void_p(gptr), stream)

            rec = {"columns": cols, "rows": rows}
            for name, fn, reps in (("a_offsets_call", case_a, args.reps),
                                   ("b_separate_calls", case_b, max(1, args.reps // 2))):
                ms, stages = timed(fn, reps, lib, stream)
                rec[name + "_ms"] = round(ms, 4)
                rec[name + "_stages_ms"] = stages
            # the two forms of (c) in alternating order, median of three rounds each (what runs
            # first after the C separate calls of (b) meets a different clock state)
            runs = {"c_shared_offsets": [], "c_shared_plain": []}
            for r in range(3):
                pair = [("c_shared_offsets", case_c_offsets), ("c_shared_plain", case_c_plain)]
                for name, fn in (pair if r % 2 == 0 else pair[::-1]):
                    runs[name].append(timed(fn, args.reps, lib, stream))
            for name, res in runs.items():
                ms, stages = sorted(res, key=lambda x: x[0])[1]
                rec[name + "_ms"] = round(ms, 4)
                rec[name + "_stages_ms"] = stages
            rec["a_over_b_speedup"] = round(rec["b_separate_calls_ms"] / rec["a_offsets_call_ms"], 2)
            rec["a_equals_b"] = bool(torch.equal(outs["a"], outs["b"]))
            rec["c_offsets_equals_plain"] = bool(torch.equal(outs["c_offsets"], outs["c_plain"]))
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
            assert rec["a_equals_b"] and rec["c_offsets_equals_plain"], "results differ"
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
