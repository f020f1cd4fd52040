"""The batch form of the inner-product verifier (include/blitzar_amd.h:
bzamd_verify_inner_product_batch_device): num_proofs proofs of one length over one generator set,
back to back in every operand, against the reference's own verifier per proof (oracle.ip_verify):
each verdict word and each proof's 203 bytes of transcript afterwards.  At most 8 distinct
statements per length, tiled so that neighbouring proofs differ in seed and transcript label; every
verdict word holds the opposite of what is expected before the call."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from blitzar_amd import api
from tests.test_inner_product import L_ORDER, scalars
from tests.test_inner_product_device import padded, rounds_of
from tests.test_inner_product_verify_device import (DeviceVerify, Statement, tampered,
                                                    undecodable_encodings)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DISTINCT = 8

_statements = {}  # n -> the distinct statements of that length, grown on demand
_expected = {}    # id(statement) -> (statement, what the reference says)


def offset_of(n):
    """a non-zero generator offset, one per length"""
    return 1 + n % 7


def distinct(oracle, n, count):
    have = _statements.setdefault(n, [])
    while len(have) < min(count, DISTINCT):
        k = len(have)
        have.append(Statement(oracle, n, offset_of(n), 5000 + 16 * n + k, label=f"batch proof {k}"))
    return have[:min(count, DISTINCT)]


def tiled(oracle, n, num_proofs):
    base = distinct(oracle, n, num_proofs)
    return [base[i % len(base)] for i in range(num_proofs)]


def expected(oracle, st):
    """-> (verdict, transcript after) of the reference, computed once per statement"""
    if id(st) not in _expected:
        _expected[id(st)] = (st, st.expected(oracle))
    return _expected[id(st)][1]


def lifted(value):
    """value + l: the same scalar, unreduced"""
    return np.frombuffer((int.from_bytes(value.tobytes(), "little") + L_ORDER).to_bytes(32, "little"),
                         np.uint8)


class DeviceBatch:
    """operands of one bzamd_verify_inner_product_batch_device call in torch tensors; `misalign`:
    every operand array starts at an odd address; `resident`: tensors used where they lie"""

    NAMES = ("b", "product", "commit", "l", "r", "ap")

    def __init__(self, statements, want_verdicts, misalign=False, d_generators=None, offset=None,
                 **resident):
        import torch
        self.dev = torch.device("cuda", 0)
        self.misalign = misalign
        first = statements[0]
        self.n, self.count, self.rounds = first.n, len(statements), rounds_of(first.n)
        assert all(st.n == first.n and st.offset == first.offset for st in statements)
        self.offset = first.offset if offset is None else offset
        rows = max(self.rounds, 1)
        pad = np.zeros((rows, 32), np.uint8)
        self.host = {
            "b": np.concatenate([st.b.reshape(-1) for st in statements]),
            "product": np.concatenate([st.product.reshape(-1) for st in statements]),
            "commit": np.concatenate([np.asarray(st.commit).view(np.uint8).reshape(-1)
                                      for st in statements]),
            "l": np.concatenate([(st.l if self.rounds else pad).reshape(-1) for st in statements]),
            "r": np.concatenate([(st.r if self.rounds else pad).reshape(-1) for st in statements]),
            "ap": np.concatenate([st.ap.reshape(-1) for st in statements]),
        }
        assert self.host["b"].size == 32 * self.n * self.count
        assert self.host["commit"].size == 160 * self.count
        assert self.host["l"].size == 32 * rows * self.count
        for name in self.NAMES:
            setattr(self, name, resident[name] if name in resident else self.place(self.host[name]))
        self.transcript = self.place(np.concatenate([st.t0.reshape(-1) for st in statements]))
        assert self.transcript.numel() == 203 * self.count
        # the opposite of what is expected
        words = np.array([0 if want else 1 for want in want_verdicts], "<u4")
        self.verdict = self.place(words.view(np.uint8))
        self.workspace = resident.get("workspace")
        if self.workspace is None:
            need = api.inner_product_verify_batch_workspace_bytes(self.n, self.count)
            assert need > 0
            self.workspace = self.place(np.zeros(need, np.uint8))
        self.d_generators = d_generators

    def place(self, array):
        import torch
        array = np.ascontiguousarray(array, np.uint8).reshape(-1)
        buffer = torch.zeros(array.size + 16, dtype=torch.uint8, device=self.dev)
        at = (9 if self.misalign else 8) - buffer.data_ptr() % 8
        view = buffer[at:at + array.size]
        view.copy_(torch.from_numpy(array.copy()))
        assert view.data_ptr() % 8 == (1 if self.misalign else 0)
        return view

    def enqueue(self, lib_api, stream, workspace_bytes=None):
        lib_api.verify_inner_product_batch_device(
            self.n, self.count, self.offset, self.b.data_ptr(), self.product.data_ptr(),
            self.commit.data_ptr(), self.l.data_ptr(), self.r.data_ptr(), self.ap.data_ptr(),
            self.transcript.data_ptr(), self.verdict.data_ptr(), self.workspace.data_ptr(),
            self.workspace.numel() if workspace_bytes is None else workspace_bytes,
            None if self.d_generators is None else self.d_generators.data_ptr(),
            stream=stream.cuda_stream)

    def results(self):
        """-> ([verdict words], transcripts [count, 203])"""
        words = self.verdict.cpu().numpy().copy().view("<u4")
        return [int(w) for w in words], self.transcript.cpu().numpy().reshape(self.count, 203)

    def assert_inputs_unchanged(self):
        for name in self.NAMES:
            got = getattr(self, name).cpu().numpy().reshape(-1)
            assert np.array_equal(got, self.host[name]), f"{name} was modified"


def verify_batch(lib_api, oracle, statements, **how):
    """one call on a side stream, every proof checked against the oracle -> (verdicts, launches)"""
    import torch
    want = [expected(oracle, st) for st in statements]
    call = DeviceBatch(statements, [ok for ok, _ in want], **how)
    side = torch.cuda.Stream(device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    launches = lib_api.load().bzamd_kernel_launch_count
    before = launches()
    call.enqueue(lib_api, side)
    moved = launches() - before
    side.synchronize()
    verdicts, transcripts = call.results()
    for i, (want_ok, want_t) in enumerate(want):
        assert verdicts[i] == int(want_ok), f"proof {i}: verdict {verdicts[i]}, not {want_ok}"
        assert np.array_equal(transcripts[i], want_t), f"proof {i}: the transcript differs"
    call.assert_inputs_unchanged()
    return verdicts, moved


ACCEPTED_CASES = [(1, 1), (1, 5), (2, 3), (3, 70), (5, 65), (64, 4), (100, 3), (257, 2), (1000, 3),
                  (4097, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,num_proofs", ACCEPTED_CASES)
def test_accepted_batches(gpu_backend, oracle, n, num_proofs):
    statements = tiled(oracle, n, num_proofs)
    if num_proofs > 1:
        assert not np.array_equal(statements[0].t0, statements[1].t0)
        assert not np.array_equal(statements[0].b, statements[1].b)
    verdicts, moved = verify_batch(gpu_backend, oracle, statements)
    assert verdicts == [1] * num_proofs
    assert moved > 0, "no kernel ran"


def tamper(oracle, st, name):
    return dict((k, bad) for k, bad, _ in tampered(oracle, st))[name]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 1000])
def test_mixed_batch(gpu_backend, oracle, n):
    """proofs 0, 3 and 6 intact, each of the others tampered in another operand: every verdict and
    every transcript -- the rejected proofs' too -- is the reference's for that proof.  Seven
    proofs leave four places for the six operands, so a second batch takes the other two (and two
    of the first again, at other places)."""
    want = [1, 0, 0, 1, 0, 0, 1]
    for names in (("last b entry", "product bit", "a_commit is another generator",
                   "last L replaced by last R"),
                  ("first R replaced by a valid point", "ap bit", "last b entry",
                   "a_commit is another generator")):
        statements = list(tiled(oracle, n, 7))
        for at, name in zip((1, 2, 4, 5), names):
            statements[at] = tamper(oracle, statements[at], name)
        verdicts, _ = verify_batch(gpu_backend, oracle, statements)
        assert verdicts == want


@pytest.mark.gpu
def test_undecodable_points(gpu_backend, oracle):
    """an undecodable L in one proof and an undecodable R in another: verdict 0 for those two, the
    third is accepted with the reference's transcript"""
    n = 5
    rounds = rounds_of(n)
    base = tiled(oracle, n, 3)
    for case, (name, encoding) in enumerate(undecodable_encodings()):
        bad_l, bad_r = base[0].l.copy(), base[2].r.copy()
        bad_l[case % rounds] = encoding
        bad_r[(case + 1) % rounds] = encoding
        # which of the three is intact moves with the case
        statements = [base[0].copy(l=bad_l), base[1], base[2].copy(r=bad_r)]
        order = [(case + k) % 3 for k in range(3)]
        statements = [statements[k] for k in order]
        verdicts, _ = verify_batch(gpu_backend, oracle, statements)
        assert verdicts == [1 if k == 1 else 0 for k in order], name


@pytest.mark.gpu
def test_unreduced_scalars(gpu_backend, oracle):
    """raw 256-bit b, and product and ap lifted by l, in the middle proof of three: taken as given"""
    n = 5
    base = tiled(oracle, n, 3)
    raw = Statement(oracle, n, offset_of(n), 5900, label="unreduced", reduced=False)
    assert any(int.from_bytes(row.tobytes(), "little") >= L_ORDER for row in raw.b)
    middle = raw.copy(product=lifted(raw.product), ap=lifted(raw.ap))
    verdicts, _ = verify_batch(gpu_backend, oracle, [base[0], middle, base[2]])
    assert verdicts[0] == 1 and verdicts[2] == 1  # (the middle one: the reference's, checked above)
    noise = np.random.default_rng(5901).integers(0, 256, 32, dtype=np.uint8)
    noise[31] |= 0xf0
    verdicts, _ = verify_batch(gpu_backend, oracle, [base[0], middle.copy(ap=noise), base[2]])
    assert verdicts == [1, 0, 1]


@pytest.mark.gpu
@pytest.mark.parametrize("n,num_proofs", [(3, 3), (300, 2)])
def test_misaligned_operands(gpu_backend, oracle, n, num_proofs):
    """every operand array, the verdicts and the workspace included, starts at an odd address"""
    statements = tiled(oracle, n, num_proofs)
    verdicts, _ = verify_batch(gpu_backend, oracle, statements, misalign=True)
    assert verdicts == [1] * num_proofs
    b_last = statements[-1].b.copy()
    b_last[n - 1, 0] ^= 1
    bad = statements[:-1] + [statements[-1].copy(b=b_last)]
    verdicts, _ = verify_batch(gpu_backend, oracle, bad, misalign=True)
    assert verdicts == [1] * (num_proofs - 1) + [0]


@pytest.mark.gpu
def test_callers_generators(gpu_backend, oracle):
    """np + 1 resident generators of the caller's, the last one Q; generators_offset is ignored"""
    import torch
    dev = torch.device("cuda", 0)
    n, num_proofs = 100, 3
    np_ = padded(n)
    statements = tiled(oracle, n, num_proofs)
    d_generators = torch.empty((np_ + 1, 160), dtype=torch.uint8, device=dev)
    gpu_backend.load().bzamd_ristretto255_generators_device(
        ctypes.c_void_p(d_generators.data_ptr()), offset_of(n), np_ + 1,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    generators = d_generators.cpu().numpy().copy()
    verdicts, _ = verify_batch(gpu_backend, oracle, statements, offset=0, d_generators=d_generators)
    assert verdicts == [1] * num_proofs
    assert np.array_equal(d_generators.cpu().numpy(), generators), "the generators were modified"


@pytest.mark.gpu
def test_behind_the_device_prover(gpu_backend, oracle):
    """three device proofs written straight into the batch layout, a batch verify, a second batch
    verify with one ap flipped: one stream, one workspace, nothing but the final synchronise"""
    import torch
    dev = torch.device("cuda", 0)
    n, offset, num_proofs, flipped = 100, 3, 3, 1
    rounds = rounds_of(n)
    rng = np.random.default_rng(6000)
    gens = oracle.ristretto_generators(n, offset)
    statements, a_vectors = [], []
    for k in range(num_proofs):
        a, b = scalars(rng, n), scalars(rng, n)
        st = object.__new__(Statement)
        st.__dict__.update(n=n, offset=offset, b=b, t0=oracle.transcript_new(f"prove then verify {k}"),
                           commit=oracle.msm_projective(0, [(a, False)], gens)[0],
                           product=oracle.s25_inner_product(a, b))
        st.l, st.r, st.ap, _ = oracle.ip_prove(st.t0, n, offset, a, b)
        statements.append(st)
        a_vectors.append(a)
    bad_ap = statements[flipped].ap.copy()
    bad_ap[0] ^= 1
    bad_statements = list(statements)
    bad_statements[flipped] = statements[flipped].copy(ap=bad_ap)

    zeros = {"l": torch.zeros(32 * rounds * num_proofs, dtype=torch.uint8, device=dev),
             "r": torch.zeros(32 * rounds * num_proofs, dtype=torch.uint8, device=dev),
             "ap": torch.zeros(32 * num_proofs, dtype=torch.uint8, device=dev)}
    first = DeviceBatch(statements, [True] * num_proofs, **zeros)
    d_a = torch.from_numpy(np.concatenate(a_vectors).copy()).to(dev)
    prover_t = torch.from_numpy(np.stack([st.t0 for st in statements]).copy()).to(dev)
    prover_w = torch.empty(api.inner_product_workspace_bytes(n), dtype=torch.uint8, device=dev)
    ap_flipped = torch.zeros(32 * num_proofs, dtype=torch.uint8, device=dev)
    second = DeviceBatch(bad_statements, [k != flipped for k in range(num_proofs)],
                         workspace=first.workspace, b=first.b, l=first.l, r=first.r, ap=ap_flipped)

    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    for k in range(num_proofs):
        gpu_backend.prove_inner_product_device(
            n, offset, d_a.data_ptr() + 32 * n * k, first.b.data_ptr() + 32 * n * k,
            first.l.data_ptr() + 32 * rounds * k, first.r.data_ptr() + 32 * rounds * k,
            first.ap.data_ptr() + 32 * k, prover_t.data_ptr() + 203 * k, prover_w.data_ptr(),
            prover_w.numel(), stream=side.cuda_stream)
    first.enqueue(gpu_backend, side)
    with torch.cuda.stream(side):
        ap_flipped.copy_(first.ap)
        ap_flipped[32 * flipped] ^= 1
    second.enqueue(gpu_backend, side)
    side.synchronize()

    for name in ("l", "r", "ap"):
        assert np.array_equal(getattr(first, name).cpu().numpy(), first.host[name]), name
    verdicts, transcripts = first.results()
    assert verdicts == [1, 1, 1]
    for k, st in enumerate(statements):
        assert np.array_equal(transcripts[k], expected(oracle, st)[1])
    verdicts, transcripts = second.results()
    assert verdicts == [0 if k == flipped else 1 for k in range(num_proofs)]
    for k, st in enumerate(bad_statements):
        want_ok, want_t = expected(oracle, st)
        assert bool(verdicts[k]) == want_ok and np.array_equal(transcripts[k], want_t)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5, 1000])
def test_batch_of_one_is_the_single_entry(gpu_backend, oracle, n):
    import torch
    st = distinct(oracle, n, 1)[0]
    bad_ap = st.ap.copy()
    bad_ap[0] ^= 1
    side = torch.cuda.Stream(device=torch.device("cuda", 0))
    for statement in (st, st.copy(ap=bad_ap)):
        want_ok, want_t = expected(oracle, statement)
        single = DeviceVerify(statement, want_ok)
        batch = DeviceBatch([statement], [want_ok])
        torch.cuda.synchronize()
        single.enqueue(gpu_backend, side)
        batch.enqueue(gpu_backend, side)
        side.synchronize()
        verdict, t_after = single.results()
        verdicts, transcripts = batch.results()
        assert verdicts == [verdict] == [int(want_ok)]
        assert np.array_equal(transcripts[0], t_after) and np.array_equal(t_after, want_t)


@pytest.mark.gpu
def test_launch_count_does_not_grow_with_the_batch(gpu_backend, oracle):
    """65 proofs in one call launch fewer than 8 times the kernels of one single-proof call (a loop
    over the proofs would launch 65 times as many)"""
    import torch
    n, num_proofs = 5, 65
    statements = tiled(oracle, n, num_proofs)
    single = DeviceVerify(statements[0], True)
    side = torch.cuda.Stream(device=torch.device("cuda", 0))
    launches = gpu_backend.load().bzamd_kernel_launch_count
    torch.cuda.synchronize()
    before = launches()
    single.enqueue(gpu_backend, side)
    one = launches() - before
    side.synchronize()
    assert single.results()[0] == 1 and one > 0
    verdicts, moved = verify_batch(gpu_backend, oracle, statements)
    assert verdicts == [1] * num_proofs
    print(f"launches: single {one}, batch of {num_proofs}: {moved}")
    assert moved < 8 * one


@pytest.mark.gpu
def test_short_workspace_aborts(gpu_backend):
    """one byte short: the call aborts before it launches anything (a child process; the device
    operands are never touched, so host addresses stand in for them)"""
    code = ("import numpy as np\nfrom blitzar_amd import api\n"
            "assert api.init(api.SXT_GPU_BACKEND, 0) == 0\n"
            "need = api.inner_product_verify_batch_workspace_bytes(5, 3)\n"
            "assert need > 0\n"
            "b = np.zeros(8192 + need, np.uint8)\n"
            "at = b.ctypes.data\n"
            "print('calling', flush=True)\n"
            "api.verify_inner_product_batch_device(5, 3, 0, at, at + 512, at + 1024, at + 2048,\n"
            "                                      at + 3072, at + 4096, at + 5120, at + 6144,\n"
            "                                      at + 8192, need - 1)\n"
            "print('returned', flush=True)\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode < 0, r.stdout + r.stderr
    assert "the inner-product verifier's workspace is too small" in r.stderr, r.stderr
    assert "calling" in r.stdout and "returned" not in r.stdout
