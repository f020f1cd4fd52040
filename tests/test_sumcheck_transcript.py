"""Sumcheck with the library's own transcript (include/blitzar_amd.h: bzamd_sumcheck_transcript_*,
bzamd_prove_sumcheck_transcript, bzamd_prove_sumcheck_transcript_device, bzamd_verify_sumcheck).

The expected bytes everywhere are the reference's own prover (oracle.prove_sumcheck) driven by the
plain-Python Merlin of tests/merlin_ref.py as its transcript callback, which tests/test_merlin_ref.py
pins to the compiled reference: round polynomials, evaluation point and the 203 bytes of the
transcript after the proof.  mle_evaluations are checked against bzamd_prove_sumcheck replaying
the same challenges, the verifier against its own definition in Python integers."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from blitzar_amd import api
from tests import merlin_ref
from tests.test_sumcheck import CASES
from tests.test_sumcheck_device import MODULUS, folded_evaluations, make_inputs, to_bytes, to_int

TAIL_ROWS = 256     # kTailRows of proof/sumcheck_transcript.hip
FIXED_DEGREE = 5    # kFixedDegree of proof/sumcheck_rows.h


def variables(n):
    return max((int(n) - 1).bit_length(), 1)


def one_product(degree):
    """(num_mles, products) of round degree `degree`: one product of that length, one of length 1"""
    return degree, [list(range(degree)), [0]]


def reference_proof(oracle, field_id, mles, table, terms, n, degree, transcript):
    """-> (polynomials, evaluation_point, transcript after) of the reference's prover with the
    Python transcript, continuing `transcript`"""
    t = merlin_ref.Transcript(raw=transcript)
    merlin_ref.sumcheck_begin(t, variables(n), degree)
    polys, point = oracle.prove_sumcheck(field_id, mles, table, terms, n, degree,
                                         merlin_ref.sumcheck_callback(t, field_id))
    return polys, point, t.array()


def replay_callback(point):
    """a transcript that hands out the given challenges"""
    state = {"round": 0}

    def cb(r_ptr, ctx, poly_ptr, length):
        ctypes.memmove(r_ptr, point[state["round"]].tobytes(), 32)
        state["round"] += 1
    return cb


def expected_evaluations(lib_api, field_id, mles, table, terms, n, degree, point):
    return lib_api.prove_sumcheck_with_evaluations(field_id, mles, table, terms, n, degree,
                                                   replay_callback(point))[2]


#--------------------------------------------------------------------------------------------------
# host
#--------------------------------------------------------------------------------------------------
def _library_callback_case(cpu_backend, oracle, field_id, n, num_mles, products, seed):
    mles, _, table, terms, degree = make_inputs(field_id, n, num_mles, products, seed)
    t0 = merlin_ref.Transcript(label="library callback").array()
    want = reference_proof(oracle, field_id, mles, table, terms, n, degree, t0)
    t = t0.copy()
    cpu_backend.sumcheck_transcript_begin(t, variables(n), degree)
    context = api.bzamd_sumcheck_transcript_context(t.ctypes.data, field_id)
    native = cpu_backend.load().bzamd_sumcheck_transcript_round

    def through_the_library(r_ptr, ctx, poly_ptr, length):  # the oracle passes no context on
        native(r_ptr, ctypes.addressof(context), poly_ptr, length)

    polys, point = oracle.prove_sumcheck(field_id, mles, table, terms, n, degree,
                                         through_the_library)
    assert np.array_equal(polys, want[0]), "round polynomials differ"
    assert np.array_equal(point, want[1]), "evaluation points differ"
    assert np.array_equal(t, want[2]), "transcripts differ"


@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("degree", range(1, 9))
def test_library_callback_one_round(cpu_backend, oracle, field_id, degree):
    """n = 2: one round, the transcript without the arithmetic; from degree 5 on the 166-byte rate
    boundary falls inside the "P" message"""
    num_mles, products = one_product(degree)
    _library_callback_case(cpu_backend, oracle, field_id, 2, num_mles, products, 1000 + degree)


@pytest.mark.parametrize("field_id", [0, 1])
def test_library_callback_nine_rounds(cpu_backend, oracle, field_id):
    """n = 300, degree 3: the rate boundary walks through every phase of a round"""
    _library_callback_case(cpu_backend, oracle, field_id, 300, 3, [[0, 1, 2], [0, 0]], 1100)


def _check_host_prover(lib_api, oracle, field_id, case, seed):
    n, num_mles, products = CASES[case]
    mles, _, table, terms, degree = make_inputs(field_id, n, num_mles, products, seed + case)
    t0 = merlin_ref.Transcript(label="host prover").array()
    want = reference_proof(oracle, field_id, mles, table, terms, n, degree, t0)
    polys, point, evaluations, t = lib_api.prove_sumcheck_transcript(field_id, mles, table, terms, n,
                                                                     degree, t0)
    assert np.array_equal(polys, want[0]), "round polynomials differ"
    assert np.array_equal(point, want[1]), "evaluation points differ"
    assert np.array_equal(t, want[2]), "transcripts differ"
    assert np.array_equal(evaluations, expected_evaluations(lib_api, field_id, mles, table, terms, n,
                                                            degree, point))
    polys, point, evaluations, t = lib_api.prove_sumcheck_transcript(
        field_id, mles, table, terms, n, degree, t0, with_evaluations=False)
    assert evaluations is None
    assert np.array_equal(polys, want[0]) and np.array_equal(point, want[1])
    assert np.array_equal(t, want[2])


@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_host_prover(cpu_backend, oracle, field_id, case):
    _check_host_prover(cpu_backend, oracle, field_id, case, 1200)


def claimed_sum(field_id, mles, mults, products):
    p = MODULUS[field_id]
    m = [to_int(field_id, x) for x in mults]
    total = 0
    for row in range(mles.shape[1]):
        values = [to_int(field_id, mles[j, row]) for j in range(mles.shape[0])]
        for mult, terms in zip(m, products):
            term = mult
            for j in terms:
                term = term * values[j] % p
            total = (total + term) % p
    return total


@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_verifier(cpu_backend, field_id, case):
    n, num_mles, products = CASES[case]
    p = MODULUS[field_id]
    mles, mults, table, terms, degree = make_inputs(field_id, n, num_mles, products, 1300 + case)
    t0 = merlin_ref.Transcript(label="verifier").array()
    polys, point, evaluations, t = cpu_backend.prove_sumcheck_transcript(field_id, mles, table, terms,
                                                                         n, degree, t0)
    claim = to_bytes(field_id, claimed_sum(field_id, mles, mults, products))
    ok, expected, v_point, v_t = cpu_backend.verify_sumcheck(field_id, claim, polys, t0)
    assert ok
    assert np.array_equal(v_point, point) and np.array_equal(v_t, t)
    # what the caller's final evaluation must equal
    e = [to_int(field_id, x) for x in evaluations]
    final = 0
    for mult, product in zip([to_int(field_id, x) for x in mults], products):
        term = mult
        for j in product:
            term = term * e[j] % p
        final = (final + term) % p
    assert to_int(field_id, expected) == final
    # a wrong claim
    wrong = claim.copy()
    wrong[3] ^= 0x10
    assert not cpu_backend.verify_sumcheck(field_id, wrong, polys, t0)[0]
    # a wrong polynomial in a middle round
    forged = polys.copy()
    forged[polys.shape[0] // 2, polys.shape[1] - 1, 7] ^= 0x01
    assert not cpu_backend.verify_sumcheck(field_id, claim, forged, t0)[0]


def test_verifier_stops_at_the_failing_round(cpu_backend):
    """on 0 the outputs and the transcript are as the rounds before the failing one left them"""
    field_id = 0
    n, num_mles, products = CASES[5]
    mles, mults, table, terms, degree = make_inputs(field_id, n, num_mles, products, 1400)
    t0 = merlin_ref.Transcript(label="verifier").array()
    polys, point, _, _ = cpu_backend.prove_sumcheck_transcript(field_id, mles, table, terms, n, degree,
                                                               t0)
    claim = to_bytes(field_id, claimed_sum(field_id, mles, mults, products))
    forged = polys.copy()
    forged[4, 0, 0] ^= 0x01
    ok, expected, v_point, v_t = cpu_backend.verify_sumcheck(field_id, claim, forged, t0)
    assert not ok
    t = merlin_ref.Transcript(raw=t0)
    merlin_ref.sumcheck_begin(t, polys.shape[0], degree)
    for rnd in range(4):
        assert merlin_ref.sumcheck_round(t, field_id, polys[rnd].tobytes()) == point[rnd].tobytes()
    assert np.array_equal(v_t, t.array())
    assert np.array_equal(v_point[:4], point[:4]) and not v_point[4:].any()
    p = MODULUS[field_id]
    acc = 0
    for c in reversed([to_int(field_id, c) for c in polys[3]]):
        acc = (acc * to_int(field_id, point[3]) + c) % p
    assert to_int(field_id, expected) == acc


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "sumcheck_transcript_golden.npz")
GOLDEN_CASES = [0, 2, 4, 5]  # of tests.test_sumcheck.CASES: (n, D) = (1, 1), (5, 2), (37, 4), (300, 3)


@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_golden(cpu_backend, field_id, case):
    """A second, independent pin.  Recorded once from the reference's own
    prfsk::reference_transcript + prfsk::prove_sum (cpu_driver) + verify_sumcheck_no_evaluation by
    a driver that is not part of the repository, for the tables make_inputs(field_id, *CASES[case],
    seed 50 + case) yields, per case under the key f<field>_n<n>_d<D>: `label` (the transcript is
    prft::transcript{label}), `polynomials`, `point`, `transcript` (the 203 bytes after proving),
    `claim` (p_0(0) + p_0(1), the verifier's expected_sum going in) and `expected_sum` (the
    verifier's expected_sum coming out; it returned true, with the prover's point and transcript)."""
    n, num_mles, products = CASES[case]
    mles, _, table, terms, degree = make_inputs(field_id, n, num_mles, products, 50 + case)
    golden = np.load(GOLDEN)
    key = f"f{field_id}_n{n}_d{degree}_"
    t0 = merlin_ref.Transcript(label=golden[key + "label"].tobytes()).array()
    polys, point, _, t = cpu_backend.prove_sumcheck_transcript(field_id, mles, table, terms, n, degree,
                                                               t0)
    assert np.array_equal(polys, golden[key + "polynomials"])
    assert np.array_equal(point, golden[key + "point"])
    assert np.array_equal(t, golden[key + "transcript"])
    ok, expected, v_point, v_t = cpu_backend.verify_sumcheck(field_id, golden[key + "claim"],
                                                             golden[key + "polynomials"], t0)
    assert ok and np.array_equal(expected, golden[key + "expected_sum"])
    assert np.array_equal(v_point, golden[key + "point"])
    assert np.array_equal(v_t, golden[key + "transcript"])
    # the Python transcript the other tests expect by, on the recorded polynomials
    py = merlin_ref.Transcript(raw=t0)
    merlin_ref.sumcheck_begin(py, polys.shape[0], degree)
    for rnd in range(polys.shape[0]):
        r = merlin_ref.sumcheck_round(py, field_id, golden[key + "polynomials"][rnd].tobytes())
        assert r == golden[key + "point"][rnd].tobytes()
    assert np.array_equal(py.array(), golden[key + "transcript"])


def _hipcc():
    from blitzar_amd import build
    return build.HIPCC if os.path.exists(build.HIPCC) else shutil.which("hipcc")


@pytest.mark.skipif(_hipcc() is None, reason="hipcc is not installed")
def test_transcript_kernels_use_no_scratch(tmp_path):
    """the compiler's own resource report, with the flags the library is built with: the tail
    kernel (round degrees 1 .. 5, both fields) and the challenge kernel keep the round polynomial
    and the transcript step out of scratch memory"""
    from blitzar_amd import build
    src = "proof/sumcheck_transcript.hip"
    r = subprocess.run([_hipcc(), *build.FLAGS, *build.TU_FLAGS.get(src, []), "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(build.CSRC, src), "-o", str(tmp_path / "transcript.o")],
                       capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-4000:]
    scratch, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name is not None:
            scratch[name] = int(m.group(1))
    tail = {k: v for k, v in scratch.items() if "k_sumcheck_tail" in k}
    challenge = {k: v for k, v in scratch.items() if "k_sumcheck_challenge" in k}
    print(scratch)
    assert len(tail) == 10, f"expected 5 round degrees x 2 fields, found {sorted(tail)}"
    assert len(challenge) == 2, sorted(challenge)
    assert all(v == 0 for v in tail.values()), tail
    assert all(v == 0 for v in challenge.values()), challenge


#--------------------------------------------------------------------------------------------------
# GPU
#--------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_host_prover_on_gpu(gpu_backend, oracle, field_id, case):
    before = gpu_backend.load().bzamd_kernel_launch_count()
    _check_host_prover(gpu_backend, oracle, field_id, case, 1500)
    assert gpu_backend.load().bzamd_kernel_launch_count() > before, "no kernel ran"


def expected_launches(n, degree, with_evaluations):
    """the load, three per round before the tail, the tail; round degrees
    above 5 have no tail and no last fold without mle_evaluations"""
    v = variables(n)
    if degree <= FIXED_DEGREE:
        chain_rounds = max(v - 1 - (TAIL_ROWS.bit_length() - 1), 0)
        return 1 + 3 * chain_rounds + 1
    return 1 + 3 * v - (0 if with_evaluations else 1)


class DeviceProof:
    """operands of one bzamd_prove_sumcheck_transcript_device call in torch tensors"""

    def __init__(self, field_id, d_mles, num_mles, table, terms, n, degree, transcript,
                 with_evaluations=True):
        import torch
        dev = d_mles.device
        v = variables(n)
        self.args = (field_id, num_mles, table, terms, n, degree)
        self.d_mles = d_mles
        self.polys = torch.zeros((v, degree + 1, 32), dtype=torch.uint8, device=dev)
        self.point = torch.zeros((v, 32), dtype=torch.uint8, device=dev)
        self.evaluations = (torch.zeros((num_mles, 32), dtype=torch.uint8, device=dev)
                            if with_evaluations else None)
        if isinstance(transcript, np.ndarray):
            transcript = torch.from_numpy(transcript.copy()).to(dev)
        self.transcript = transcript  # a device tensor is used in place
        lengths = np.ascontiguousarray(table, np.uint8).size // api.SUMCHECK_PRODUCT_STRIDE[field_id]
        self.workspace_bytes = api.sumcheck_transcript_workspace_bytes(field_id, n, num_mles, lengths,
                                                                       len(terms), degree)
        self.workspace = torch.empty(self.workspace_bytes, dtype=torch.uint8, device=dev)

    def enqueue(self, lib_api, stream):
        field_id, num_mles, table, terms, n, degree = self.args
        lib_api.prove_sumcheck_transcript_device(
            field_id, self.d_mles.data_ptr(), num_mles, table, terms, n, degree,
            self.polys.data_ptr(), self.point.data_ptr(),
            None if self.evaluations is None else self.evaluations.data_ptr(),
            self.transcript.data_ptr(), self.workspace.data_ptr(), self.workspace_bytes,
            stream=stream.cuda_stream)

    def results(self):
        return (self.polys.cpu().numpy(), self.point.cpu().numpy(),
                None if self.evaluations is None else self.evaluations.cpu().numpy(),
                self.transcript.cpu().numpy())


D3 = (4, [[0, 1, 2], [3, 1], [2]])
DEVICE_FORM_CASES = (
    # tail only; 512 is the first size wholly inside it, 513 has one chain round before it, 1027 two
    [(n, *D3) for n in (1, 2, 5, 37, 300, 512, 513, 1027)]
    # many workgroups' partials in k_sumcheck_challenge
    + [((1 << 14) + 77, *D3)]
    # every instantiation of the tail
    + [(513, *one_product(d)) for d in (1, 2, 4, 5)]
    # the generic chain down to the last round
    + [(n, *one_product(d)) for d in (6, 8) for n in (37, 513)])


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("case", range(len(DEVICE_FORM_CASES)))
def test_device_form(gpu_backend, oracle, field_id, case):
    import torch
    dev = torch.device("cuda", 0)
    n, num_mles, products = DEVICE_FORM_CASES[case]
    mles, _, table, terms, degree = make_inputs(field_id, n, num_mles, products, 1600 + case)
    t0 = merlin_ref.Transcript(label="device form").array()
    want = reference_proof(oracle, field_id, mles, table, terms, n, degree, t0)
    d_mles = torch.from_numpy(mles.copy()).to(dev)
    side = torch.cuda.Stream(device=dev)
    launches = gpu_backend.load().bzamd_kernel_launch_count
    for with_evaluations in (True, False):
        proof = DeviceProof(field_id, d_mles, num_mles, table, terms, n, degree, t0, with_evaluations)
        torch.cuda.synchronize()
        before = launches()
        proof.enqueue(gpu_backend, side)
        assert launches() - before == expected_launches(n, degree, with_evaluations)
        side.synchronize()
        polys, point, evaluations, t = proof.results()
        assert np.array_equal(polys, want[0]), "round polynomials differ"
        assert np.array_equal(point, want[1]), "evaluation points differ"
        assert np.array_equal(t, want[2]), "transcripts differ"
        if with_evaluations:
            assert np.array_equal(evaluations, expected_evaluations(
                gpu_backend, field_id, mles, table, terms, n, degree, point))
    assert np.array_equal(d_mles.cpu().numpy(), mles), "the device tables were modified"


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_device_form_back_to_back(gpu_backend, oracle, field_id):
    """two proofs enqueued on one stream with nothing between them but the final synchronise, and
    a third that continues the first one's transcript where it lies"""
    import torch
    dev = torch.device("cuda", 0)
    shapes = [(1027, *D3), (300, *one_product(2)), (513, *one_product(6))]
    inputs = [make_inputs(field_id, n, num_mles, products, 1700 + i)
              for i, (n, num_mles, products) in enumerate(shapes)]
    t0 = [merlin_ref.Transcript(label=f"proof {i}").array() for i in range(2)]
    d_mles = [torch.from_numpy(inp[0].copy()).to(dev) for inp in inputs]
    proofs = []
    for i in range(3):
        (n, num_mles, _), (_, _, table, terms, degree) = shapes[i], inputs[i]
        transcript = t0[i] if i < 2 else proofs[0].transcript
        proofs.append(DeviceProof(field_id, d_mles[i], num_mles, table, terms, n, degree, transcript))
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    for proof in proofs:
        proof.enqueue(gpu_backend, side)
    side.synchronize()
    want, after_first = [], None
    for i in range(3):
        (n, _, _), (mles, _, table, terms, degree) = shapes[i], inputs[i]
        want.append(reference_proof(oracle, field_id, mles, table, terms, n, degree,
                                    t0[i] if i < 2 else after_first))
        if i == 0:
            after_first = want[0][2]
    for i in (1, 2):
        polys, point, _, t = proofs[i].results()
        assert np.array_equal(polys, want[i][0]) and np.array_equal(point, want[i][1])
        assert np.array_equal(t, want[i][2])
    polys, point, _, _ = proofs[0].results()
    assert np.array_equal(polys, want[0][0]) and np.array_equal(point, want[0][1])
    # the host form doing the same: the third proof continues the first one's transcript
    (n, _, _), (mles, _, table, terms, degree) = shapes[2], inputs[2]
    host = gpu_backend.prove_sumcheck_transcript(field_id, mles, table, terms, n, degree, after_first)
    third = proofs[2].results()
    for h, d in zip(host, third):
        assert np.array_equal(h, d)


# n = 2 with one MLE and one product: round degree 1 is k_sumcheck_tail alone, 6 (above kFixedDegree)
# k_sumcheck_challenge and k_sumcheck_fold_slot
SWEEP_PRODUCTS = {1: [[0]], 6: [[0] * 6]}


def sweep_fields(pos):
    """the field alternates with the position's parity; every 8th position takes both"""
    return (pos % 2, 1 - pos % 2) if pos % 8 == 0 else (pos % 2,)


def sweep_model(t0, field_id, degree, polynomial=None):
    t = merlin_ref.TracedTranscript(raw=t0)
    merlin_ref.sumcheck_begin(t, 1, degree)
    r = merlin_ref.sumcheck_round(t, field_id, bytes(32 * (degree + 1)) if polynomial is None else polynomial)
    return t, r


@pytest.mark.parametrize("degree", sorted(SWEEP_PRODUCTS))
def test_sponge_sweep_reaches_every_boundary_class(degree):
    """a one-round proof from each of the 166 positions crosses the rate boundary in every way a
    32-byte challenge can (which edges are reached depends on lengths alone)"""
    reached, positions = set(), {0: 0, 1: 0}
    for pos, t0 in enumerate(merlin_ref.padded_starts()):
        for field_id in sweep_fields(pos):
            reached |= sweep_model(t0, field_id, degree)[0].classes
            positions[field_id] += 1
    assert reached == merlin_ref.BOUNDARY_CLASSES, sorted(merlin_ref.BOUNDARY_CLASSES - reached)
    assert positions == {0: 83, 1: 83 + 21}


def test_host_transcript_at_every_sponge_position(cpu_backend):
    """the host twin of the sweep: strobe128_over / transcript_over are one text for both sponges;
    bzamd_sumcheck_transcript_begin and _round from each position, every polynomial length"""
    rng = np.random.default_rng(1900)
    native = cpu_backend.load().bzamd_sumcheck_transcript_round
    reached = set()
    for pos, t0 in enumerate(merlin_ref.padded_starts()):
        for field_id, degree in ((pos % 2, 1 + pos % 8), (1 - pos % 2, 1 + (pos // 8) % 8)):
            polynomial = rng.integers(0, 256, 32 * (degree + 1), dtype=np.uint8)
            model, want = sweep_model(t0, field_id, degree, polynomial.tobytes())
            t, r = t0.copy(), np.zeros(32, np.uint8)
            cpu_backend.sumcheck_transcript_begin(t, 1, degree)
            context = api.bzamd_sumcheck_transcript_context(t.ctypes.data, field_id)
            native(r.ctypes.data_as(ctypes.c_void_p), ctypes.byref(context),
                   polynomial.ctypes.data_as(ctypes.c_void_p), degree + 1)
            assert np.array_equal(t, model.array()), (pos, field_id, degree)
            assert r.tobytes() == want, (pos, field_id, degree)
            reached |= model.classes
    assert reached == merlin_ref.BOUNDARY_CLASSES


@pytest.mark.gpu
@pytest.mark.parametrize("degree", sorted(SWEEP_PRODUCTS))
def test_device_form_at_every_sponge_position(gpu_backend, oracle, degree):
    """a caller who continues a transcript hands the prover any position of the sponge"""
    import torch
    dev = torch.device("cuda", 0)
    n, num_mles, products = 2, 1, SWEEP_PRODUCTS[degree]
    inputs = [make_inputs(field_id, n, num_mles, products, 1800 + degree + field_id) for field_id in (0, 1)]
    d_mles = [torch.from_numpy(inp[0].copy()).to(dev) for inp in inputs]
    side = torch.cuda.Stream(device=dev)
    reached = set()
    for pos, t0 in enumerate(merlin_ref.padded_starts()):
        for field_id in sweep_fields(pos):
            mles, _, table, terms, _ = inputs[field_id]
            proof = DeviceProof(field_id, d_mles[field_id], num_mles, table, terms, n, degree, t0)
            proof.enqueue(gpu_backend, side)
            side.synchronize()
            polys, point, evaluations, t = proof.results()
            where = f"position {pos}, field {field_id}"
            # the Python model fed the device's own polynomial first: a difference there is the sponge's
            model, r = sweep_model(t0, field_id, degree, polys[0].tobytes())
            assert np.array_equal(t, model.array()), f"{where}: the transcript differs from the model"
            assert point[0].tobytes() == r, f"{where}: the challenge differs from the model"
            reached |= model.classes
            want = reference_proof(oracle, field_id, mles, table, terms, n, degree, t0)
            assert np.array_equal(polys, want[0]), f"{where}: round polynomials differ"
            assert np.array_equal(point, want[1]), f"{where}: evaluation points differ"
            assert np.array_equal(t, want[2]), f"{where}: transcripts differ"
            assert np.array_equal(evaluations, folded_evaluations(field_id, mles, point)), where
    assert reached == merlin_ref.BOUNDARY_CLASSES
