#!/usr/bin/env python3
"""Inner-product prover, warm, on one GPU: the blocking entry of another build against this
build's, and this build's device form on resident vectors.

    python tools/inner_product_bench.py --parent-lib <libblitzar_amd.so of the parent commit>
                                        [--sizes 4096,65536,1048576] [--samples 20] [--out FILE]
    python tools/inner_product_bench.py --profile-one 4096

Legs, alternating A, B1, B2, B2g, A, ... after one untimed call each, reduced scalars, built-in
generators from offset 0:
  A    sxt_curve25519_prove_inner_product of --parent-lib (build the parent commit with
       BZ_VARIANT=parent python -m blitzar_amd.build; BLITZAR_AMD_LIB selects it), host operands,
       in a child process of its own;
  B1   the same entry of this build, host operands, in a second child process;
  B2   bzamd_prove_inner_product_device on resident a and b, built-in generators, in a third
       child process: timed from the enqueue to the stream synchronise after it, with the time the
       enqueueing call itself took beside it (`enqueue_median_ms`: the host thread's share);
  B2g  the same with np + 1 caller-supplied resident generators.
Hashing the outputs and resetting the transcript are outside the clock.  The children stay alive
for the whole run and take one sample per request, so the legs see the same minutes of the same
device.  All four must return the same proof.  Printed per size, one
JSON line (appended to --out): medians, min, max, the spread of A (max - min), B1 / A and B2 / A,
and `b1_not_slower`: B1's median within A's spread of A's median, or better.
--profile-one N runs a warm-up and one device-form proof of N elements and nothing else: the
process to put under a kernel trace.  Needs a GPU: there is no CPU fallback.

--verify measures the verifier the same way: A is sxt_curve25519_verify_inner_product of
--parent-lib, B1 this build's, B2 / B2g bzamd_verify_inner_product_device on a resident proof with
the built-in / with resident caller generators.  The proof, the commitment and the product are made
once per size by this build (the B1 child) outside the clock and handed to the other children in a
file.  Every leg must return 1 and leave the same transcript, and after the timed samples one call
per leg with a tampered ap must return 0.  --verify --profile-one N: a warm-up and one device-form
verification."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def inputs(n):
    """reduced scalars: a seeded numpy stream with the top four bits cleared (below 2^252)"""
    rng = np.random.default_rng(n)
    a = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    b = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    a[:, 31] &= 0x0f
    b[:, 31] &= 0x0f
    return a, b


def proof_hash(parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(np.ascontiguousarray(p).tobytes())
    return h.hexdigest()[:16]


class Worker:
    """one process, one library: takes samples on request"""

    def __init__(self):
        import torch  # (before the library: torch's HIP runtime first, tests/conftest.py)
        from blitzar_amd import api
        self.torch, self.api = torch, api
        lib = api.load()
        assert lib.bzamd_device_count() > 0, "inner_product_bench needs a GPU"
        api.reset_for_testing()
        assert api.init(api.SXT_GPU_BACKEND, 0) == 0
        self.dev = torch.device("cuda", 0)
        self.has_device_form = hasattr(lib, "bzamd_prove_inner_product_device")
        self.has_verify_form = hasattr(lib, "bzamd_verify_inner_product_device")

    def setup(self, n):
        torch, api, dev = self.torch, self.api, self.dev
        self.n = n
        self.a, self.b = inputs(n)
        self.t0 = api.transcript_new("inner product bench")
        if not self.has_device_form:
            return
        rounds = max(n - 1, 0).bit_length()
        np_ = 1 << rounds
        self.d_a = torch.from_numpy(self.a).to(dev)
        self.d_b = torch.from_numpy(self.b).to(dev)
        self.d_t0 = torch.from_numpy(self.t0).to(dev)
        self.d_t = torch.zeros_like(self.d_t0)
        self.d_l = torch.zeros((max(rounds, 1), 32), dtype=torch.uint8, device=dev)
        self.d_r = torch.zeros((max(rounds, 1), 32), dtype=torch.uint8, device=dev)
        self.d_ap = torch.zeros(32, dtype=torch.uint8, device=dev)
        self.workspace_bytes = api.inner_product_workspace_bytes(n)
        self.d_workspace = torch.empty(self.workspace_bytes, dtype=torch.uint8, device=dev)
        self.d_generators = torch.empty((np_ + 1, 160), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        api.load().bzamd_ristretto255_generators_device(self.d_generators.data_ptr(), 0, np_ + 1,
                                                        stream)
        torch.cuda.synchronize()
        self.rounds = rounds

    def device_hash(self):
        return proof_hash((self.d_l.cpu().numpy()[:self.rounds], self.d_r.cpu().numpy()[:self.rounds],
                           self.d_ap.cpu().numpy(), self.d_t.cpu().numpy()))

    def sample(self, leg):
        """one timed proof; hashing the outputs and resetting the transcript are outside the clock"""
        torch, api = self.torch, self.api
        if leg == "blocking":
            torch.cuda.synchronize()
            t_start = time.perf_counter()
            proof = api.prove_inner_product(self.t0, self.n, 0, self.a, self.b)
            ms = (time.perf_counter() - t_start) * 1e3
            return {"ms": ms, "sha256": proof_hash(proof)}
        stream = torch.cuda.current_stream(self.dev)
        self.d_t.copy_(self.d_t0)
        torch.cuda.synchronize()
        t_start = time.perf_counter()
        api.prove_inner_product_device(
            self.n, 0, self.d_a.data_ptr(), self.d_b.data_ptr(), self.d_l.data_ptr(),
            self.d_r.data_ptr(), self.d_ap.data_ptr(), self.d_t.data_ptr(),
            self.d_workspace.data_ptr(), self.workspace_bytes,
            self.d_generators.data_ptr() if leg == "device_generators" else None,
            stream=stream.cuda_stream)
        enqueue_ms = (time.perf_counter() - t_start) * 1e3
        stream.synchronize()
        ms = (time.perf_counter() - t_start) * 1e3
        return {"ms": ms, "enqueue_ms": enqueue_ms, "sha256": self.device_hash()}

    def make_statement(self, n, path):
        """what a verifier is handed, by this build: the proof of inputs(n), the commitment of a and
        <a, b> mod l"""
        api = self.api
        a, b = inputs(n)
        t0 = api.transcript_new("inner product bench")
        l, r, ap, _ = api.prove_inner_product(t0, n, 0, a, b)
        commit = api.msm_projective(0, [(a, False)], api.get_generators(n, 0))[0].view(np.uint64)
        order = 2**252 + 27742317777372353535851937790883648493
        words = lambda x: [int.from_bytes(row.tobytes(), "little") for row in x]  # noqa: E731
        product = sum(x * y for x, y in zip(words(a), words(b))) % order
        np.savez(path, b=b, t0=t0, l=l, r=r, ap=ap, commit=commit,
                 product=np.frombuffer(product.to_bytes(32, "little"), np.uint8))

    def setup_verify(self, n, path):
        torch, api, dev = self.torch, self.api, self.dev
        self.n = n
        self.st = {k: v for k, v in np.load(path).items()}
        self.rounds = max(n - 1, 0).bit_length()
        tampered = self.st["ap"].copy()
        tampered[0] ^= 1
        self.st["ap_tampered"] = tampered
        if not self.has_verify_form:
            return
        np_ = 1 << self.rounds
        self.d = {k: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8)).to(dev)
                  for k, v in self.st.items()}
        self.d_t = torch.zeros_like(self.d["t0"])
        self.d_verdict = torch.zeros(1, dtype=torch.int32, device=dev)
        self.workspace_bytes = api.inner_product_verify_workspace_bytes(n)
        self.d_workspace = torch.empty(self.workspace_bytes, dtype=torch.uint8, device=dev)
        self.d_generators = torch.empty((np_ + 1, 160), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        api.load().bzamd_ristretto255_generators_device(self.d_generators.data_ptr(), 0, np_ + 1,
                                                        stream)
        torch.cuda.synchronize()

    def sample_verify(self, leg, tampered=False):
        """one timed verification; reading the verdict back and resetting the transcript are
        outside the clock"""
        torch, api, st = self.torch, self.api, self.st
        ap = "ap_tampered" if tampered else "ap"
        if leg == "blocking":
            torch.cuda.synchronize()
            t_start = time.perf_counter()
            ok, t_after = api.verify_inner_product(st["t0"], self.n, 0, st["b"], st["product"],
                                                   st["commit"], st["l"], st["r"], st[ap])
            ms = (time.perf_counter() - t_start) * 1e3
            return {"ms": ms, "verdict": int(ok), "sha256": proof_hash((t_after,))}
        d = self.d
        stream = torch.cuda.current_stream(self.dev)
        self.d_t.copy_(d["t0"])
        self.d_verdict.fill_(1 if tampered else 0)
        torch.cuda.synchronize()
        t_start = time.perf_counter()
        api.verify_inner_product_device(
            self.n, 0, d["b"].data_ptr(), d["product"].data_ptr(), d["commit"].data_ptr(),
            d["l"].data_ptr(), d["r"].data_ptr(), d[ap].data_ptr(), self.d_t.data_ptr(),
            self.d_verdict.data_ptr(), self.d_workspace.data_ptr(), self.workspace_bytes,
            self.d_generators.data_ptr() if leg == "device_generators" else None,
            stream=stream.cuda_stream)
        enqueue_ms = (time.perf_counter() - t_start) * 1e3
        stream.synchronize()
        ms = (time.perf_counter() - t_start) * 1e3
        return {"ms": ms, "enqueue_ms": enqueue_ms, "verdict": int(self.d_verdict.cpu().numpy()[0]),
                "sha256": proof_hash((self.d_t.cpu().numpy(),))}

    def serve(self):
        print(json.dumps({"ready": True, "library": self.api.LIB_PATH,
                          "device_form": self.has_device_form,
                          "verify_form": self.has_verify_form}), flush=True)
        for line in sys.stdin:
            words = line.split()
            if not words or words[0] == "quit":
                break
            if words[0] == "setup":
                self.setup(int(words[1]))
                print(json.dumps({"ok": True}), flush=True)
            elif words[0] == "statement":
                self.make_statement(int(words[1]), words[2])
                print(json.dumps({"ok": True}), flush=True)
            elif words[0] == "setup_verify":
                self.setup_verify(int(words[1]), words[2])
                print(json.dumps({"ok": True}), flush=True)
            elif words[0] == "verify":
                print(json.dumps(self.sample_verify(words[1], tampered=len(words) > 2)), flush=True)
            else:
                print(json.dumps(self.sample(words[1])), flush=True)


class Child:
    def __init__(self, library):
        env = dict(os.environ)
        if library is not None:
            env["BLITZAR_AMD_LIB"] = os.path.abspath(library)
        else:
            env.pop("BLITZAR_AMD_LIB", None)
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker"],
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env,
                                  cwd=ROOT)
        self.hello = self.reply()

    def reply(self):
        line = self.p.stdout.readline()
        assert line, "a worker died"
        return json.loads(line)

    def ask(self, text):
        self.p.stdin.write(text + "\n")
        self.p.stdin.flush()
        return self.reply()

    def close(self):
        self.p.stdin.write("quit\n")
        self.p.stdin.flush()
        self.p.wait(timeout=60)


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "samples_ms": [round(x, 4) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--sizes", default="4096,65536,1048576")
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--out")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--profile-one", type=int)
    ap.add_argument("--verify", action="store_true")
    args = ap.parse_args()
    if args.worker:
        Worker().serve()
        return
    if args.verify and args.profile_one is not None:
        w = Worker()
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "statement.npz")
            w.make_statement(args.profile_one, path)
            w.setup_verify(args.profile_one, path)
        w.sample_verify("device_builtin")  # warm: the engine's buffers grow here
        print(json.dumps({"n": args.profile_one, **w.sample_verify("device_builtin")}), flush=True)
        return
    if args.profile_one is not None:
        w = Worker()
        w.setup(args.profile_one)
        w.sample("device_builtin")  # warm: the engine's buffers grow here
        print(json.dumps({"n": args.profile_one, **w.sample("device_builtin")}), flush=True)
        return
    assert args.parent_lib and os.path.exists(args.parent_lib), "--parent-lib: no such library"
    parent, mine, resident = Child(args.parent_lib), Child(None), Child(None)
    children = (parent, mine, resident)
    assert resident.hello["device_form"], "this build has no device form"
    assert not args.verify or resident.hello["verify_form"], "this build has no device verifier"
    command = "verify" if args.verify else "sample"
    tmp = tempfile.TemporaryDirectory()
    legs = [("A_parent_blocking", parent, "blocking"), ("B1_blocking", mine, "blocking"),
            ("B2_device", resident, "device_builtin"),
            ("B2g_device_generators", resident, "device_generators")]
    try:
        for n in (int(x) for x in args.sizes.split(",")):
            if args.verify:
                path = os.path.join(tmp.name, f"statement_{n}.npz")
                mine.ask(f"statement {n} {path}")
            for child in children:
                child.ask(f"setup_verify {n} {path}" if args.verify else f"setup {n}")
            warm = {name: child.ask(f"{command} {leg}") for name, child, leg in legs}
            digests = {name: got["sha256"] for name, got in warm.items()}
            assert len(set(digests.values())) == 1, f"the legs disagree: {digests}"
            if args.verify:
                assert all(got["verdict"] == 1 for got in warm.values()), f"not accepted: {warm}"
            ms = {name: [] for name, _, _ in legs}
            enqueue = {name: [] for name, _, _ in legs}
            for _ in range(args.samples):
                for name, child, leg in legs:
                    got = child.ask(f"{command} {leg}")
                    assert not args.verify or got["verdict"] == 1, f"{name} rejected the proof"
                    ms[name].append(got["ms"])
                    if "enqueue_ms" in got:
                        enqueue[name].append(got["enqueue_ms"])
            rec = {"n": n, "samples": args.samples, "parent_library": os.path.relpath(parent.hello["library"], ROOT),
                   "library": os.path.relpath(resident.hello["library"], ROOT), "proof_sha256": digests["A_parent_blocking"]}
            if args.verify:
                rec["what"] = "verify"
                tampered = {name: child.ask(f"verify {leg} tampered")["verdict"]
                            for name, child, leg in legs}
                assert not any(tampered.values()), f"a tampered ap was accepted: {tampered}"
                rec["tampered_verdicts"] = tampered
            for name, _, _ in legs:
                rec[name] = summary(ms[name])
                if enqueue[name]:
                    rec[name]["enqueue_median_ms"] = round(statistics.median(enqueue[name]), 4)
            a = rec["A_parent_blocking"]
            spread = a["max_ms"] - a["min_ms"]
            rec["a_spread_ms"] = round(spread, 4)
            for name in ("B1_blocking", "B2_device", "B2g_device_generators"):
                rec[name.split("_")[0].lower() + "_over_a"] = round(
                    rec[name]["median_ms"] / a["median_ms"], 4)
            rec["b1_not_slower"] = bool(rec["B1_blocking"]["median_ms"] <= a["median_ms"] + spread)
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as fh:
                    fh.write(line + "\n")
    finally:
        for child in children:
            child.close()
        tmp.cleanup()


if __name__ == "__main__":
    main()
