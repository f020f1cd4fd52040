#!/usr/bin/env python3
"""Timings of the verifier's checks in front of the inner-product verifier, warm, on one GPU:
bzamd_verify_sumcheck_device and bzamd_check_sumcheck_evaluations_device against the host forms
looped over a batch that lies in HBM, and bzamd_combine_commitments_device.

    python tools/verifier_bench.py [--batches 1,256,4096] [--variables 20] [--degree 3]
                                   [--commitments 8,1024] [--samples 15] [--out FILE]
                                   [--parent-lib <libblitzar_amd.so of the parent commit>]
                                   [--inner-product 1024:1,16,256/65536:1,16,64]
                                   [--legs sumcheck,combine,inner_product]

Legs, per field and batch B (proofs of --variables variables at round degree --degree; one accepted
proof repeated B times: the work of a proof does not depend on its bytes, only on being accepted to
the last round):
  rounds_host    (A) the proofs' polynomials, sums and transcripts copied to the host, then
                 bzamd_verify_sumcheck once per proof;
  rounds_device  (B) one bzamd_verify_sumcheck_device call on the batch where it lies;
  check_host     the expected sums and evaluations copied to the host, then
                 bzamd_check_sumcheck_evaluations once per proof (three products over three MLEs);
  check_device   one bzamd_check_sumcheck_evaluations_device call.
A and B alternate, sample by sample.  Then, per count K of --commitments:
  combine_device bzamd_combine_commitments_device over K commitments the library made itself.
With --parent-lib, per n and batch B of --inner-product (one accepted proof of n elements, made by
this build, repeated B times in the batch layout; built-in generators from offset 0):
  ip_single_loop_parent  (A) bzamd_verify_inner_product_device of --parent-lib (BLITZAR_AMD_LIB
                 selects it, as in tools/inner_product_bench.py) enqueued B times on one stream with
                 one workspace, in a child process of its own;
  ip_batch_device        (B) one bzamd_verify_inner_product_batch_device call of this build, in a
                 second child process.
Both children take their samples by the same protocol, in turn; both must accept the intact batch
and reject exactly the tampered proof of a batch with one tampered ap.
A sample is the time between two device events around the leg and a synchronise, after two untimed
runs of every leg; printed per leg, one JSON line (appended to --out, default
profiles/verifier_bench.jsonl): median, min and max in microseconds.  No figure here is an
acceptance condition.  Needs a GPU: there is no CPU fallback."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

MODULUS = {0: 2**252 + 27742317777372353535851937790883648493,
           1: 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001}
PRODUCTS = [[0, 1, 2], [2, 2], [0]]


def value_of(field_id, raw):
    v = int.from_bytes(bytes(raw), "little")
    p = MODULUS[field_id]
    return v * pow(1 << 256, -1, p) % p if field_id == 1 else v % p


def element(field_id, value):
    p = MODULUS[field_id]
    v = value * (1 << 256) % p if field_id == 1 else value % p
    return np.frombuffer(v.to_bytes(32, "little"), np.uint8)


def accepted_proof(api, field_id, variables, degree, t0):
    """-> (claimed sum [32], polynomials [v, d + 1, 32]): random polynomials with p[1] fixed to the
    running sum, the challenges drawn by the library's own transcript"""
    p = MODULUS[field_id]
    rng = np.random.default_rng(1000 + field_id)
    draw = lambda: int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % p  # noqa: E731
    lib = api.load()
    t = t0.copy()
    lib.bzamd_sumcheck_transcript_begin(t.ctypes.data, variables, degree)
    running = draw()
    claimed = element(field_id, running)
    polys = np.zeros((variables, degree + 1, 32), np.uint8)
    context = api.bzamd_sumcheck_transcript_context(t.ctypes.data, field_id)
    r_bytes = np.zeros(32, np.uint8)
    for rnd in range(variables):
        c = [draw() for _ in range(degree + 1)]
        c[1] = (running - 2 * c[0] - sum(c[2:])) % p
        for k, ck in enumerate(c):
            polys[rnd, k] = element(field_id, ck)
        lib.bzamd_sumcheck_transcript_round(r_bytes.ctypes.data, ctypes.byref(context),
                                            polys[rnd].ctypes.data, degree + 1)
        r = value_of(field_id, r_bytes)
        running = sum(ck * pow(r, k, p) for k, ck in enumerate(c)) % p
    ok, _, _, _ = api.verify_sumcheck(field_id, claimed, polys, t0)
    assert ok, "the constructed proof is not accepted"
    return claimed, polys


class Batch:
    """B copies of one proof and one evaluation statement in HBM, and the legs on them"""

    def __init__(self, torch, api, field_id, batch, variables, degree):
        dev = torch.device("cuda", 0)
        self.torch, self.api, self.field_id, self.batch = torch, api, field_id, batch
        self.variables, self.degree = variables, degree
        self.t0 = api.transcript_new("verifier bench")
        claimed, polys = accepted_proof(api, field_id, variables, degree, self.t0)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.polys = up(np.tile(polys.reshape(1, -1), (batch, 1)))
        self.claimed = up(np.tile(claimed, (batch, 1)))
        self.start = up(np.tile(self.t0, (batch, 1)))
        self.sums = torch.empty_like(self.claimed)
        self.transcripts = torch.empty_like(self.start)
        self.points = torch.empty((batch, variables, 32), dtype=torch.uint8, device=dev)
        self.verdicts = torch.zeros(batch, dtype=torch.int32, device=dev)
        # the statement of the evaluation check and evaluations that satisfy it
        rng = np.random.default_rng(7 + field_id)
        p = MODULUS[field_id]
        values = [int(x) for x in rng.integers(1, 1 << 62, 3)]
        multipliers = [int(x) for x in rng.integers(1, 1 << 62, 3)]
        total = 0
        for m, terms in zip(multipliers, PRODUCTS):
            for j in terms:
                m = m * values[j] % p
            total = (total + m) % p
        stride = api.SUMCHECK_PRODUCT_STRIDE[field_id]
        self.table = np.zeros((3, stride), np.uint8)
        for k, (m, terms) in enumerate(zip(multipliers, PRODUCTS)):
            self.table[k, :32] = element(field_id, m)
            self.table[k, 32] = len(terms)
        self.terms = np.array([j for terms in PRODUCTS for j in terms], np.uint32)
        self.evaluations = up(np.tile(np.stack([element(field_id, x) for x in values]).reshape(1, -1),
                                      (batch, 1)))
        self.expected = up(np.tile(element(field_id, total), (batch, 1)))
        self.workspace_bytes = api.check_sumcheck_evaluations_workspace_bytes(field_id, 3, 6)
        self.workspace = torch.empty(self.workspace_bytes, dtype=torch.uint8, device=dev)

    def rounds_device(self, stream):
        self.sums.copy_(self.claimed)
        self.transcripts.copy_(self.start)
        self.api.verify_sumcheck_device(
            self.field_id, self.variables, self.degree, self.batch, self.polys.data_ptr(),
            self.sums.data_ptr(), self.points.data_ptr(), self.transcripts.data_ptr(),
            self.verdicts.data_ptr(), stream=stream.cuda_stream)

    def rounds_host(self, stream):
        polys = self.polys.cpu().numpy()
        sums = self.claimed.cpu().numpy()
        transcripts = self.start.cpu().numpy()
        point = np.zeros((self.variables, 32), np.uint8)
        verify = self.api.load().bzamd_verify_sumcheck
        accepted = 0
        for i in range(self.batch):
            accepted += verify(sums[i].ctypes.data, point.ctypes.data, transcripts[i].ctypes.data,
                               self.field_id, polys[i].ctypes.data, self.variables, self.degree)
        assert accepted == self.batch

    def check_device(self, stream):
        self.api.check_sumcheck_evaluations_device(
            self.field_id, 3, self.table, self.terms, self.batch, self.expected.data_ptr(),
            self.evaluations.data_ptr(), self.verdicts.data_ptr(), self.workspace.data_ptr(),
            self.workspace_bytes, stream=stream.cuda_stream)

    def check_host(self, stream):
        expected = self.expected.cpu().numpy()
        evaluations = self.evaluations.cpu().numpy()
        check = self.api.load().bzamd_check_sumcheck_evaluations
        accepted = 0
        for i in range(self.batch):
            accepted += check(self.field_id, expected[i].ctypes.data, evaluations[i].ctypes.data, 3,
                              self.table.ctypes.data, self.terms.ctypes.data, 3, 6)
        assert accepted == self.batch

    def verify_results(self):
        self.torch.cuda.synchronize()
        assert bool((self.verdicts == 1).all()), "a device verdict is not 1"


class Combination:
    def __init__(self, torch, api, count):
        dev = torch.device("cuda", 0)
        rng = np.random.default_rng(count)
        columns = [(rng.integers(0, 256, (1, 8), dtype=np.uint8), False) for _ in range(count)]
        self.api, self.count = api, count
        self.commitments = torch.from_numpy(api.compute_pedersen_commitments(0, columns)).to(dev)
        self.coefficients = torch.randint(0, 256, (count, 32), dtype=torch.uint8, device=dev)
        self.combined = torch.zeros(160, dtype=torch.uint8, device=dev)
        self.valid = torch.zeros(1, dtype=torch.int32, device=dev)
        self.workspace_bytes = api.combine_commitments_workspace_bytes(count)
        self.workspace = torch.empty(self.workspace_bytes, dtype=torch.uint8, device=dev)

    def combine_device(self, stream):
        self.api.combine_commitments_device(
            self.count, self.commitments.data_ptr(), self.coefficients.data_ptr(),
            self.combined.data_ptr(), self.valid.data_ptr(), self.workspace.data_ptr(),
            self.workspace_bytes, stream=stream.cuda_stream)


class InnerProductBatch:
    """B copies of one inner-product statement in the batch layout of
    bzamd_verify_inner_product_batch_device, and the two legs on them"""

    def __init__(self, worker, n, batch, path):
        torch, api, dev = worker.torch, worker.api, worker.dev
        self.torch, self.api, self.n, self.batch = torch, api, n, batch
        st = {k: np.ascontiguousarray(v).view(np.uint8).reshape(-1) for k, v in np.load(path).items()}
        self.rounds = max(n - 1, 0).bit_length()
        pad = np.zeros(32, np.uint8)
        tile = lambda a: torch.from_numpy(np.tile(a, batch)).to(dev)  # noqa: E731
        self.b, self.product, self.commit = tile(st["b"]), tile(st["product"]), tile(st["commit"])
        self.l = tile(st["l"] if self.rounds else pad)
        self.r = tile(st["r"] if self.rounds else pad)
        self.ap, self.t0 = tile(st["ap"]), tile(st["t0"])
        self.tampered_at = batch // 2
        self.ap_tampered = self.ap.clone()
        self.ap_tampered[32 * self.tampered_at] ^= 1
        self.transcripts = torch.zeros_like(self.t0)
        self.verdicts = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.has_batch = hasattr(api.load(), "bzamd_verify_inner_product_batch_device")
        need = (api.inner_product_verify_batch_workspace_bytes(n, batch) if self.has_batch
                else api.inner_product_verify_workspace_bytes(n))
        self.workspace = torch.empty(need, dtype=torch.uint8, device=dev)

    def single_loop(self, stream, ap):
        n, rounds, at = self.n, self.rounds, lambda t: t.data_ptr()  # noqa: E731
        single = self.api.inner_product_verify_workspace_bytes(n)
        for i in range(self.batch):
            self.api.verify_inner_product_device(
                n, 0, at(self.b) + 32 * n * i, at(self.product) + 32 * i, at(self.commit) + 160 * i,
                at(self.l) + 32 * rounds * i, at(self.r) + 32 * rounds * i, at(ap) + 32 * i,
                at(self.transcripts) + 203 * i, at(self.verdicts) + 4 * i, at(self.workspace),
                single, stream=stream.cuda_stream)

    def batch_call(self, stream, ap):
        at = lambda t: t.data_ptr()  # noqa: E731
        self.api.verify_inner_product_batch_device(
            self.n, self.batch, 0, at(self.b), at(self.product), at(self.commit), at(self.l),
            at(self.r), at(ap), at(self.transcripts), at(self.verdicts), at(self.workspace),
            self.workspace.numel(), stream=stream.cuda_stream)

    def sample(self, leg, tampered):
        """-> {"us", "verdicts_ok"}: resetting the transcripts and the verdicts and reading them
        back are outside the clock"""
        torch = self.torch
        self.transcripts.copy_(self.t0)
        want = torch.ones_like(self.verdicts)
        if tampered:
            want[self.tampered_at] = 0
        self.verdicts.copy_(1 - want)  # the opposite of what is expected
        torch.cuda.synchronize()
        ap = self.ap_tampered if tampered else self.ap
        run = self.single_loop if leg == "single" else self.batch_call
        us = sample_us(torch, lambda stream: run(stream, ap))
        return {"us": us, "verdicts_ok": bool((self.verdicts == want).all())}


def serve_inner_product():
    """a child of the inner-product legs: one process, one library (BLITZAR_AMD_LIB)"""
    from inner_product_bench import Worker
    worker = Worker()
    print(json.dumps({"ready": True, "library": worker.api.LIB_PATH}), flush=True)
    state = None
    for line in sys.stdin:
        words = line.split()
        if not words or words[0] == "quit":
            break
        if words[0] == "statement":
            worker.make_statement(int(words[1]), words[2])
            print(json.dumps({"ok": True}), flush=True)
        elif words[0] == "setup":
            state = None  # (frees the previous batch first)
            state = InnerProductBatch(worker, int(words[1]), int(words[2]), words[3])
            print(json.dumps({"ok": True}), flush=True)
        else:
            print(json.dumps(state.sample(words[1], tampered=len(words) > 2)), flush=True)


def inner_product_legs(args, emit):
    from inner_product_bench import Child  # (its worker entry is replaced below)

    class IpChild(Child):
        def __init__(self, library):
            env = dict(os.environ)
            if library is not None:
                env["BLITZAR_AMD_LIB"] = os.path.abspath(library)
            else:
                env.pop("BLITZAR_AMD_LIB", None)
            self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--ip-worker"],
                                      stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True,
                                      env=env, cwd=ROOT)
            self.hello = self.reply()

    assert os.path.exists(args.parent_lib), "--parent-lib: no such library"
    parent, mine = IpChild(args.parent_lib), IpChild(None)
    legs = [("ip_single_loop_parent", parent, "single"), ("ip_batch_device", mine, "batch")]
    tmp = tempfile.TemporaryDirectory()
    try:
        for shape in args.inner_product.split("/"):
            n, batches = shape.split(":")
            n = int(n)
            path = os.path.join(tmp.name, f"statement_{n}.npz")
            mine.ask(f"statement {n} {path}")
            for batch in (int(x) for x in batches.split(",")):
                for _, child, _ in legs:
                    child.ask(f"setup {n} {batch} {path}")
                for name, child, leg in legs * 2:  # two untimed runs of every leg
                    assert child.ask(f"sample {leg}")["verdicts_ok"], f"{name}: an intact batch"
                us = {name: [] for name, _, _ in legs}
                for _ in range(args.samples):
                    for name, child, leg in legs:
                        got = child.ask(f"sample {leg}")
                        assert got["verdicts_ok"], f"{name} rejected a proof of an intact batch"
                        us[name].append(got["us"])
                for name, child, leg in legs:
                    assert child.ask(f"sample {leg} tampered")["verdicts_ok"], \
                        f"{name}: not exactly the tampered proof was rejected"
                    emit({"n": n, "batch": batch, "leg": name, "samples": args.samples,
                          "median_us": round(statistics.median(us[name]), 1),
                          "min_us": round(min(us[name]), 1), "max_us": round(max(us[name]), 1)})
    finally:
        for child in (parent, mine):
            child.close()
        tmp.cleanup()


def sample_us(torch, leg):
    stream = torch.cuda.current_stream()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(stream)
    leg(stream)
    stream.synchronize()
    end.record(stream)
    end.synchronize()
    return start.elapsed_time(end) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,256,4096")
    ap.add_argument("--variables", type=int, default=20)
    ap.add_argument("--degree", type=int, default=3)
    ap.add_argument("--commitments", default="8,1024")
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verifier_bench.jsonl"))
    ap.add_argument("--parent-lib")
    ap.add_argument("--inner-product", default="1024:1,16,256/65536:1,16,64")
    ap.add_argument("--legs", default="sumcheck,combine,inner_product")
    ap.add_argument("--ip-worker", action="store_true")
    args = ap.parse_args()
    if args.ip_worker:
        serve_inner_product()
        return
    wanted = args.legs.split(",")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")

    # (children of their own, before this process opens the device)
    if "inner_product" in wanted and args.parent_lib:
        inner_product_legs(args, emit)
    if "sumcheck" not in wanted and "combine" not in wanted:
        return
    from inner_product_bench import Worker  # torch first, then the library, the GPU backend
    worker = Worker()
    torch, api = worker.torch, worker.api
    assert hasattr(api.load(), "bzamd_combine_commitments_device"), "this build has no verifier"

    def run(legs, common):
        """legs: [(name, callable)], taken in turn"""
        for _, leg in legs * 2:
            sample_us(torch, leg)
        us = {name: [] for name, _ in legs}
        for _ in range(args.samples):
            for name, leg in legs:
                us[name].append(sample_us(torch, leg))
        for name, _ in legs:
            emit({**common, "leg": name, "samples": args.samples,
                  "median_us": round(statistics.median(us[name]), 1),
                  "min_us": round(min(us[name]), 1), "max_us": round(max(us[name]), 1)})

    for field_id in (0, 1) if "sumcheck" in wanted else ():
        for batch in [int(x) for x in args.batches.split(",")]:
            b = Batch(torch, api, field_id, batch, args.variables, args.degree)
            common = {"field_id": field_id, "batch": batch, "variables": args.variables,
                      "degree": args.degree}
            run([("rounds_host", b.rounds_host), ("rounds_device", b.rounds_device)], common)
            b.verify_results()
            run([("check_host", b.check_host), ("check_device", b.check_device)], common)
            b.verify_results()
    for count in [int(x) for x in args.commitments.split(",")] if "combine" in wanted else []:
        c = Combination(torch, api, count)
        run([("combine_device", c.combine_device)], {"commitments": count})
        torch.cuda.synchronize()
        assert int(c.valid.cpu().numpy()[0]) == 1


if __name__ == "__main__":
    main()
