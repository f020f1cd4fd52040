#!/usr/bin/env python3
"""Sumcheck prover, warm, on one GPU: the arguments and the workload of the reference's
benchmark/sumcheck/benchmark.m.cc (degree x num_products random MLEs of n rows, every product of
length `degree`, a hash transcript), for both fields of the ABI.

    python tools/sumcheck_bench.py <n> <degree> <num_products> <num_samples> [--fields 0,1]
                                   [--column-bytes 1|2|4|8] [--transcript]
    python tools/sumcheck_bench.py <n> <degree> <num_products> <num_samples> --transcript
                                   --column-bytes W

Timed, with a device synchronise inside the clock, after one untimed call:
  host    sxt_prove_sumcheck: the tables start in host memory (their upload is part of the call);
  device  bzamd_prove_sumcheck_device: the tables are resident in HBM before the clock starts.
With --column-bytes W the MLEs are signed integers of W bytes, the tables of the two legs above are
those values widened to 32 bytes, and two more legs run beside them on resident operands:
  columns     bzamd_prove_sumcheck_device_columns on the W-byte columns;
  columns32   the same entry point on the widened tables, as num_mles columns of 32 bytes.
Both must return the device leg's bytes; `device_bytes` is the device memory each form allocated.
The transcript callback is Python (one ctypes call and one SHA-256 per round); its cost is timed
alone and printed beside the two (`callback_ms`) -- it is inside both figures and is not kernel time.
With --transcript the transcript is the library's own Merlin (the reference's reference_transcript)
and two legs on resident tables alternate in one process, A, B, A, B, ..., after one untimed call each:
  A  bzamd_prove_sumcheck_device with the native bzamd_sumcheck_transcript_round as its callback (no
     Python in the loop; one host round trip per round);
  B  bzamd_prove_sumcheck_transcript_device: enqueue only, timed to a stream synchronise after it.
Both must leave the same bytes.  Printed per field: the medians, the spread of the A samples (max -
min) and whether B's median is within that spread of A's or better (`b_not_slower`).
With --transcript --column-bytes W the MLEs are signed integers of W bytes and the two legs are the
enqueue-only forms, alternating B, C, B, C, ... in one process after one untimed call each:
  B  bzamd_prove_sumcheck_transcript_device on the values widened to 32 bytes;
  C  bzamd_prove_sumcheck_transcript_device_columns on the W-byte columns.
Both must leave the same outputs and transcript.  Printed per field: the medians, the spread of the
B samples, whether C's median is within that spread of B's or better (`c_not_slower`), and the
workspace bytes of both forms.  (Field 1 draws its values from a pool of 2^16 integers, widened in
Python integers once: the kernels' time does not depend on the values.)
BLITZAR_AMD_LIB selects the library (A/B against another build in one session); a library without
bzamd_prove_sumcheck_device reports the device leg as absent.  Prints one JSON line.  Needs a GPU:
there is no CPU fallback."""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # (before the library: torch's HIP runtime first, tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from blitzar_amd import api  # noqa: E402

MODULUS = {0: 2**252 + 27742317777372353535851937790883648493,
           1: 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001}
TOP_BYTE_MASK = {0: 0x0f, 1: 0x1f}  # below the modulus: canonical in either representation


def random_elements(rng, field_id, count):
    out = rng.integers(0, 256, (count, 32), dtype=np.uint8)
    out[:, 31] &= TOP_BYTE_MASK[field_id]
    return out


def integer_columns(rng, width, n, num_mles):
    """num_mles columns of n signed integers of `width` bytes, as int64 and as their own bytes"""
    bits = 8 * width
    values = rng.integers(-(1 << (bits - 1)), (1 << (bits - 1)) - 1, (num_mles, n), dtype=np.int64,
                          endpoint=True)
    raw = np.ascontiguousarray(values.view(np.uint8).reshape(num_mles, n, 8)[:, :, :width])
    return values, raw


def widen(field_id, values):
    """int64 [..] -> the field elements v mod p in the caller's representation, uint8 [.., 32]"""
    p = MODULUS[field_id]
    if field_id == 0:
        # plain little-endian integers: |v| in limb 0, and p - |v| for v < 0 (p's limb 0 may borrow
        # from limb 1, which is not zero)
        limbs = np.zeros(values.shape + (4,), np.uint64)
        negative = values < 0
        magnitude = np.where(negative, -values, values).astype(np.uint64)
        p_limbs = [np.uint64((p >> (64 * k)) & (2**64 - 1)) for k in range(4)]
        limbs[..., 0] = np.where(negative, p_limbs[0] - magnitude, magnitude)
        limbs[..., 1] = np.where(negative, p_limbs[1] - (magnitude > p_limbs[0]).astype(np.uint64), 0)
        limbs[..., 2] = np.where(negative, p_limbs[2], 0)
        limbs[..., 3] = np.where(negative, p_limbs[3], 0)
        return limbs.view(np.uint8).reshape(values.shape + (32,))
    r = (1 << 256) % p  # Montgomery form; in Python integers
    flat = b"".join((int(v) * r % p).to_bytes(32, "little") for v in values.reshape(-1).tolist())
    return np.frombuffer(flat, np.uint8).reshape(values.shape + (32,)).copy()


def hash_callback(field_id):
    p = MODULUS[field_id]

    def cb(r_ptr, ctx, poly_ptr, length):
        poly = ctypes.string_at(poly_ptr, 32 * length)
        v = int.from_bytes(hashlib.sha256(poly).digest(), "little") % p
        ctypes.memmove(r_ptr, v.to_bytes(32, "little"), 32)
    return cb


def samples_ms(fn, num_samples):
    fn()  # warm
    torch.cuda.synchronize()
    out = []
    for _ in range(num_samples):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "samples_ms": [round(x, 4) for x in ms]}


def transcript_legs(field_id, dev, n, degree, num_products, num_samples):
    """--transcript: legs A and B of the docstring for one field"""
    num_mles = degree * num_products
    rounds = max((n - 1).bit_length(), 1)
    rng = np.random.default_rng(1 + field_id)
    mles = random_elements(rng, field_id, n * num_mles).reshape(num_mles, n, 32)
    table = np.zeros((num_products, api.SUMCHECK_PRODUCT_STRIDE[field_id]), np.uint8)
    table[:, :32] = random_elements(rng, field_id, num_products)
    table[:, 32:36] = np.frombuffer(np.uint32(degree).tobytes(), np.uint8)
    terms = np.arange(num_mles, dtype=np.uint32)
    d_mles = torch.from_numpy(mles).to(dev)
    t0 = api.transcript_new("sumcheck bench")
    out = {}
    t_a = t0.copy()
    context = api.bzamd_sumcheck_transcript_context(t_a.ctypes.data, field_id)

    def leg_a():
        t_a[:] = t0
        api.sumcheck_transcript_begin(t_a, rounds, degree)
        out["a"] = api.prove_sumcheck_device(field_id, d_mles.data_ptr(), num_mles, table, terms, n,
                                             degree, api.SUMCHECK_TRANSCRIPT_ROUND,
                                             context=ctypes.addressof(context))

    d_t0 = torch.from_numpy(t0).to(dev)
    d_t = torch.zeros_like(d_t0)
    d_polys = torch.zeros((rounds, degree + 1, 32), dtype=torch.uint8, device=dev)
    d_point = torch.zeros((rounds, 32), dtype=torch.uint8, device=dev)
    d_evaluations = torch.zeros((num_mles, 32), dtype=torch.uint8, device=dev)
    workspace_bytes = api.sumcheck_transcript_workspace_bytes(field_id, n, num_mles, num_products,
                                                              num_mles, degree)
    d_workspace = torch.empty(workspace_bytes, dtype=torch.uint8, device=dev)

    def leg_b():
        d_t.copy_(d_t0)
        api.prove_sumcheck_transcript_device(
            field_id, d_mles.data_ptr(), num_mles, table, terms, n, degree, d_polys.data_ptr(),
            d_point.data_ptr(), d_evaluations.data_ptr(), d_t.data_ptr(), d_workspace.data_ptr(),
            workspace_bytes, stream=torch.cuda.current_stream(dev).cuda_stream)

    for leg in (leg_a, leg_b):
        leg()  # warm
        torch.cuda.synchronize()
    ms = {"a": [], "b": []}
    for _ in range(num_samples):
        for name, leg in (("a", leg_a), ("b", leg_b)):
            t_start = time.perf_counter()
            leg()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t_start) * 1e3)
    got = (d_polys.cpu().numpy(), d_point.cpu().numpy(), d_evaluations.cpu().numpy())
    same = all(np.array_equal(a, b) for a, b in zip(out["a"], got)) and \
        np.array_equal(t_a, d_t.cpu().numpy())
    assert same, "the device transcript form disagrees with the callback form"
    a, b = summary(ms["a"]), summary(ms["b"])
    spread = a["max_ms"] - a["min_ms"]
    return {"A_callback": a, "B_device_transcript": b, "a_spread_ms": round(spread, 4),
            "b_over_a": round(b["median_ms"] / a["median_ms"], 4),
            "b_not_slower": bool(b["median_ms"] <= a["median_ms"] + spread),
            "b_equals_a": True,
            "polynomials_sha256": hashlib.sha256(got[0].tobytes()).hexdigest()[:16]}


def transcript_columns_legs(field_id, dev, n, degree, num_products, num_samples, width):
    """--transcript --column-bytes: legs B and C of the docstring for one field"""
    num_mles = degree * num_products
    rounds = max((n - 1).bit_length(), 1)
    rng = np.random.default_rng(1 + field_id)
    if field_id == 0:
        values, raw = integer_columns(rng, width, n, num_mles)
        mles = widen(field_id, values)
    else:
        pool_values, pool_raw = integer_columns(rng, width, 1 << 16, 1)
        pool_wide = widen(field_id, pool_values)
        pick = rng.integers(0, 1 << 16, (num_mles, n))
        raw, mles = pool_raw[0][pick], pool_wide[0][pick]
        del pick
    table = np.zeros((num_products, api.SUMCHECK_PRODUCT_STRIDE[field_id]), np.uint8)
    table[:, :32] = random_elements(rng, field_id, num_products)
    table[:, 32:36] = np.frombuffer(np.uint32(degree).tobytes(), np.uint8)
    terms = np.arange(num_mles, dtype=np.uint32)
    d_mles = torch.from_numpy(np.ascontiguousarray(mles)).to(dev)
    d_raw = torch.from_numpy(np.ascontiguousarray(raw)).to(dev)
    del mles, raw
    descriptors = [(d_raw.data_ptr() + j * n * width, n, width, True) for j in range(num_mles)]
    d_t0 = torch.from_numpy(api.transcript_new("sumcheck bench")).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    sizes = {"b": api.sumcheck_transcript_workspace_bytes(field_id, n, num_mles, num_products,
                                                          num_mles, degree),
             "c": api.sumcheck_transcript_columns_workspace_bytes(field_id, n, num_mles,
                                                                  num_products, num_mles, degree)}
    buffers = {}
    for leg in ("b", "c"):
        buffers[leg] = {
            "t": torch.zeros_like(d_t0),
            "polys": torch.zeros((rounds, degree + 1, 32), dtype=torch.uint8, device=dev),
            "point": torch.zeros((rounds, 32), dtype=torch.uint8, device=dev),
            "evaluations": torch.zeros((num_mles, 32), dtype=torch.uint8, device=dev),
            "workspace": torch.empty(sizes[leg], dtype=torch.uint8, device=dev)}

    def leg_b():
        o = buffers["b"]
        o["t"].copy_(d_t0)
        api.prove_sumcheck_transcript_device(
            field_id, d_mles.data_ptr(), num_mles, table, terms, n, degree, o["polys"].data_ptr(),
            o["point"].data_ptr(), o["evaluations"].data_ptr(), o["t"].data_ptr(),
            o["workspace"].data_ptr(), sizes["b"], stream=stream)

    def leg_c():
        o = buffers["c"]
        o["t"].copy_(d_t0)
        api.prove_sumcheck_transcript_device_columns(
            field_id, descriptors, table, terms, n, degree, o["polys"].data_ptr(),
            o["point"].data_ptr(), o["evaluations"].data_ptr(), o["t"].data_ptr(),
            o["workspace"].data_ptr(), sizes["c"], stream=stream)

    for leg in (leg_b, leg_c):
        leg()  # warm
        torch.cuda.synchronize()
    ms = {"b": [], "c": []}
    for _ in range(num_samples):
        for name, leg in (("b", leg_b), ("c", leg_c)):
            t_start = time.perf_counter()
            leg()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t_start) * 1e3)
    same = all(torch.equal(buffers["b"][k], buffers["c"][k])
               for k in ("t", "polys", "point", "evaluations"))
    assert same, "the columns form disagrees with the device transcript form"
    b, c = summary(ms["b"]), summary(ms["c"])
    spread = b["max_ms"] - b["min_ms"]
    return {"B_device_transcript": b, "C_device_transcript_columns": c,
            "b_spread_ms": round(spread, 4), "c_over_b": round(c["median_ms"] / b["median_ms"], 4),
            "c_not_slower": bool(c["median_ms"] <= b["median_ms"] + spread), "c_equals_b": True,
            "workspace_bytes": {"B": int(sizes["b"]), "C": int(sizes["c"])},
            "polynomials_sha256":
                hashlib.sha256(buffers["c"]["polys"].cpu().numpy().tobytes()).hexdigest()[:16]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int)
    ap.add_argument("degree", type=int)
    ap.add_argument("num_products", type=int)
    ap.add_argument("num_samples", type=int)
    ap.add_argument("--fields", default="0,1")
    ap.add_argument("--column-bytes", type=int, choices=[1, 2, 4, 8], default=None)
    ap.add_argument("--transcript", action="store_true")
    args = ap.parse_args()
    lib = api.load()
    assert lib.bzamd_device_count() > 0, "sumcheck_bench needs a GPU"
    api.reset_for_testing()
    assert api.init(api.SXT_GPU_BACKEND, 0) == 0
    dev = torch.device("cuda", 0)
    has_device_form = hasattr(lib, "bzamd_prove_sumcheck_device")
    n, degree, num_products = args.n, args.degree, args.num_products
    num_mles = degree * num_products
    rounds = max((n - 1).bit_length(), 1)
    rec = {"n": n, "degree": degree, "num_products": num_products, "num_mles": num_mles,
           "rounds": rounds, "num_samples": args.num_samples, "library": api.LIB_PATH,
           "table_bytes": 32 * n * num_mles, "fields": {}}
    if args.transcript:
        assert hasattr(lib, "bzamd_prove_sumcheck_transcript_device"), \
            "--transcript needs a library with the device transcript form"
        rec["mode"] = "transcript"
        if args.column_bytes is not None:
            assert hasattr(lib, "bzamd_prove_sumcheck_transcript_device_columns"), \
                "--transcript --column-bytes needs a library with the columns transcript form"
            rec["column_bytes"] = args.column_bytes
        for field_id in (int(x) for x in args.fields.split(",")):
            if args.column_bytes is not None:
                rec["fields"][str(field_id)] = transcript_columns_legs(
                    field_id, dev, n, degree, num_products, args.num_samples, args.column_bytes)
                continue
            rec["fields"][str(field_id)] = transcript_legs(field_id, dev, n, degree, num_products,
                                                           args.num_samples)
        print(json.dumps(rec), flush=True)
        return
    if args.column_bytes is not None:
        assert has_device_form and hasattr(lib, "bzamd_prove_sumcheck_device_columns"), \
            "--column-bytes needs a library with the columns form"
        rec["column_bytes"] = args.column_bytes
    for field_id in (int(x) for x in args.fields.split(",")):
        rng = np.random.default_rng(1 + field_id)
        if args.column_bytes is None:
            mles = random_elements(rng, field_id, n * num_mles).reshape(num_mles, n, 32)
        else:
            values, raw = integer_columns(rng, args.column_bytes, n, num_mles)
            mles = widen(field_id, values)
        stride = api.SUMCHECK_PRODUCT_STRIDE[field_id]
        table = np.zeros((num_products, stride), np.uint8)
        table[:, :32] = random_elements(rng, field_id, num_products)
        table[:, 32:36] = np.frombuffer(np.uint32(degree).tobytes(), np.uint8)
        terms = np.arange(num_mles, dtype=np.uint32)
        cb = hash_callback(field_id)
        out = {}

        def host():
            out["host"] = api.prove_sumcheck(field_id, mles, table, terms, n, degree, cb)

        result = {"host": summary(samples_ms(host, args.num_samples))}
        if has_device_form:
            d_mles = torch.from_numpy(mles).to(dev)
            torch.cuda.synchronize()

            def device():
                out["device"] = api.prove_sumcheck_device(field_id, d_mles.data_ptr(), num_mles,
                                                          table, terms, n, degree, cb)

            result["device"] = summary(samples_ms(device, args.num_samples))
            result["device_bytes"] = {"device": int(lib.bzamd_sumcheck_device_bytes())} \
                if hasattr(lib, "bzamd_sumcheck_device_bytes") else {}
            result["device_saves_upload_bytes"] = rec["table_bytes"]
            same = all(np.array_equal(a, b) for a, b in zip(out["host"], out["device"][:2]))
            result["device_equals_host"] = bool(same)
            assert same, "the device form disagrees with sxt_prove_sumcheck"
        else:
            result["device"] = "absent"
        if args.column_bytes is not None:
            d_raw = torch.from_numpy(raw).to(dev)
            torch.cuda.synchronize()
            width = args.column_bytes
            legs = {"columns": [(d_raw.data_ptr() + j * n * width, n, width, True)
                                for j in range(num_mles)],
                    "columns32": [(d_mles.data_ptr() + j * n * 32, n, 32, False)
                                  for j in range(num_mles)]}
            for leg, descriptors in legs.items():
                def columns():
                    out[leg] = api.prove_sumcheck_device_columns(field_id, descriptors, table, terms,
                                                                 n, degree, cb)

                result[leg] = summary(samples_ms(columns, args.num_samples))
                result["device_bytes"][leg] = int(lib.bzamd_sumcheck_device_bytes())
                same = all(np.array_equal(a, b) for a, b in zip(out[leg], out["device"]))
                assert same, f"the {leg} form disagrees with bzamd_prove_sumcheck_device"
            result["columns_equal_device"] = True
        # the Python transcript alone: `rounds` calls through ctypes, as the prover makes them
        c_cb = api.SUMCHECK_CALLBACK(cb)
        poly = np.ascontiguousarray(out["host"][0][0])
        r = np.zeros(32, np.uint8)
        t0 = time.perf_counter()
        for _ in range(10 * rounds):
            c_cb(r.ctypes.data, None, poly.ctypes.data, degree + 1)
        result["callback_ms"] = round((time.perf_counter() - t0) * 1e3 / 10, 4)
        result["polynomials_sha256"] = hashlib.sha256(out["host"][0].tobytes()).hexdigest()[:16]
        rec["fields"][str(field_id)] = result
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
