"""The device forms of the verifier's checks in front of the inner-product verifier
(include/blitzar_amd.h: bzamd_verify_sumcheck_device, bzamd_check_sumcheck_evaluations_device,
bzamd_combine_commitments_device), and the whole chain from commitment to verified opening on one
stream with nothing left to the host.

The proofs, statements and commitments are those of tests/verify_opening_cases.py (Python integers,
tests/merlin_ref.py, tests/refmath.py).  Every batch of sumcheck proofs is compared byte for byte
with the Python transcript and with bzamd_verify_sumcheck (the host form, pinned to the reference by
tests/test_sumcheck_transcript.py) on verdict, expected sum, evaluation point and transcript.  The
host forms of the other two checks are host arithmetic on every backend, so what they return here
is what the host backend returns (tests/test_verify_opening.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from blitzar_amd import api
from tests import merlin_ref
from tests.test_inner_product_device import DeviceProof
from tests.test_mle_opening import as_bytes
from tests.test_mle_opening_device import ProvenColumns
from tests.test_sumcheck_device import MODULUS, to_int
from tests.test_sumcheck_transcript import variables
from tests.verify_opening_cases import (CANARY, REJECTION_CLASSES, Commitments, Proof, Statement,
                                        encoding_of, fail_rounds_of, flipped, raw_element,
                                        rejected_encodings)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64  # canary bytes behind every buffer


def _launches():
    return api.load().bzamd_kernel_launch_count()


def _device():
    import torch
    return torch.device("cuda", 0)


def _up(array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array).copy()).to(_device())


def _guarded(payload, lead=0):
    """the bytes on the device, `lead` canary bytes in front (the payload's address is then `lead`
    past an aligned one) and GUARD behind -> (tensor, address of the payload)"""
    raw = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
    host = np.full(lead + raw.size + GUARD, CANARY, np.uint8)
    host[lead:lead + raw.size] = raw
    tensor = _up(host)
    return tensor, tensor.data_ptr() + lead


def _payload(tensor, lead, size):
    got = tensor.cpu().numpy()
    assert np.all(got[:lead] == CANARY) and np.all(got[lead + size:] == CANARY), \
        "bytes around a buffer were written"
    return got[lead:lead + size]


#--------------------------------------------------------------------------------------------------
# the sumcheck rounds
#--------------------------------------------------------------------------------------------------
def verify_batch(lib_api, proofs, lead=1):
    """one bzamd_verify_sumcheck_device call over `proofs` (one shape), every buffer at an odd
    address but the verdicts; checks each proof's four outputs against the Python transcript and
    the host form, the canaries, the launch count and that the polynomials are left alone"""
    import torch
    field_id, v, d, count = proofs[0].field_id, proofs[0].v, proofs[0].d, len(proofs)
    polys = np.stack([p.polys for p in proofs])
    d_polys, polys_at = _guarded(polys, lead)
    d_sums, sums_at = _guarded(np.stack([p.claimed for p in proofs]), lead)
    d_points, points_at = _guarded(np.full((count, v, 32), CANARY, np.uint8), lead)
    d_transcripts, transcripts_at = _guarded(np.stack([p.t0 for p in proofs]), lead)
    verdicts = torch.full((count + 1,), 7, dtype=torch.int32, device=_device())
    side = torch.cuda.Stream(device=_device())
    torch.cuda.synchronize()
    before = _launches()
    lib_api.verify_sumcheck_device(field_id, v, d, count, polys_at, sums_at, points_at,
                                   transcripts_at, verdicts.data_ptr(), stream=side.cuda_stream)
    assert _launches() - before == 1
    side.synchronize()
    got_verdicts = verdicts.cpu().numpy()
    assert got_verdicts[count] == 7, "the word behind the verdicts was written"
    assert np.array_equal(_payload(d_polys, lead, polys.size), polys.reshape(-1))
    sums = _payload(d_sums, lead, 32 * count).reshape(count, 32)
    points = _payload(d_points, lead, 32 * v * count).reshape(count, v, 32)
    transcripts = _payload(d_transcripts, lead, 203 * count).reshape(count, 203)
    for i, proof in enumerate(proofs):
        where = f"proof {i} (fails at {proof.fail_round})"
        assert got_verdicts[i] == int(proof.ok), where
        assert np.array_equal(sums[i], proof.expected), where
        assert np.array_equal(points[i], proof.point), where  # CANARY in the unwritten rows
        assert np.array_equal(transcripts[i], proof.transcript), where
        ok, expected, point, transcript = proof.host()
        written = proof.written()
        assert ok == bool(got_verdicts[i]), where
        assert np.array_equal(expected, sums[i]), where
        assert np.array_equal(point[:written], points[i][:written]), where
        assert np.array_equal(transcript, transcripts[i]), where


def shape_proofs(field_id, v, d, seed):
    """accepted proofs from every start of the 166-byte rate for the short shapes (the "P" message
    of 32 (d + 1) bytes and the 32-byte squeeze then meet the boundary inside, on and off it) and
    from four starts for the long ones, whose rounds move the position themselves; then proofs
    failing at the first, a middle and the last round"""
    starts = merlin_ref.padded_starts()
    chosen = range(len(starts)) if v <= 3 else (0, 59, 131, 165)
    proofs = [Proof(field_id, v, d, starts[k], seed + k) for k in chosen]
    for k, fail_round in enumerate(fail_rounds_of(v)[1:] * 2):
        proofs.append(Proof(field_id, v, d, starts[(41 * k + 17) % len(starts)], seed + 1000 + k,
                            fail_round))
    return proofs


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("v,d", [(1, 1), (1, 8), (3, 2), (13, 3), (30, 8)])
def test_verify_sumcheck_device(gpu_backend, field_id, v, d):
    verify_batch(gpu_backend, shape_proofs(field_id, v, d, 100 * v + d))


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("count", [1, 3, 300])
def test_verify_sumcheck_device_batch(gpu_backend, field_id, count):
    """accepted proofs mixed with proofs failing at different rounds; 300 workgroups are more than
    the device has compute units; the transcripts lie 203 bytes apart"""
    v, d = 4, 3
    starts = merlin_ref.padded_starts()
    fails = fail_rounds_of(v)  # accepted, then failing at rounds 0, 2 and 3
    proofs = [Proof(field_id, v, d, starts[(29 * i + count) % len(starts)], 7000 + i,
                    fails[i % len(fails)]) for i in range(count)]
    if count >= 3:
        assert {p.fail_round for p in proofs} >= set(fails[:3])
    verify_batch(gpu_backend, proofs, lead=0 if count == 1 else 3)


#--------------------------------------------------------------------------------------------------
# the final evaluation check
#--------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("num_products", [1, 5, 200])
@pytest.mark.parametrize("count", [1, 300])
def test_check_evaluations_device(gpu_backend, field_id, num_products, count):
    """one statement, `count` proofs with evaluations of their own; every third proof has one bit
    of its expected sum flipped, every seventh an unreduced expected sum.  At count = 1 the same
    call again with the flipped sum.  The verdicts are the host form's"""
    import torch
    st = Statement(field_id, num_products, 900 + num_products)
    evaluations, sums, want = [], [], []
    for i in range(count):
        rows, values = st.evaluations(33 * count + i)
        total = raw_element(field_id, st.expected_sum(values), unreduced=i % 7 == 6)
        evaluations.append(rows)
        sums.append(flipped(total, (37 * i) % 252) if i % 3 == 2 else total)
        want.append(int(i % 3 != 2))
    if count == 1:
        evaluations, sums, want = evaluations * 2, [sums[0], flipped(sums[0], 100)], [1, 0]
    proofs = len(want)
    d_evaluations, evaluations_at = _guarded(np.stack(evaluations), 1)
    d_sums, sums_at = _guarded(np.stack(sums), 1)
    verdicts = torch.full((proofs + 1,), 7, dtype=torch.int32, device=_device())
    bytes_needed = api.check_sumcheck_evaluations_workspace_bytes(field_id, num_products,
                                                                  len(st.terms))
    workspace = torch.full((bytes_needed + GUARD,), CANARY, dtype=torch.uint8, device=_device())
    side = torch.cuda.Stream(device=_device())
    torch.cuda.synchronize()
    before = _launches()
    gpu_backend.check_sumcheck_evaluations_device(
        field_id, st.NUM_MLES, st.table, st.terms, proofs, sums_at, evaluations_at,
        verdicts.data_ptr(), workspace.data_ptr(), bytes_needed, stream=side.cuda_stream)
    assert _launches() - before == 1
    side.synchronize()
    got = verdicts.cpu().numpy()
    assert got[proofs] == 7
    assert list(got[:proofs]) == want
    assert np.all(workspace.cpu().numpy()[bytes_needed:] == CANARY)
    _payload(d_evaluations, 1, 32 * st.NUM_MLES * proofs)
    _payload(d_sums, 1, 32 * proofs)
    for i in range(0, proofs, 41):
        assert gpu_backend.check_sumcheck_evaluations(field_id, sums[i], evaluations[i], st.table,
                                                      st.terms) == bool(want[i])


@pytest.mark.gpu
def test_check_evaluations_short_workspace_aborts(gpu_backend):
    """one byte short: the call aborts before it copies or launches anything (a child process; the
    device operands are never touched, so host addresses stand in for them)"""
    code = ("import numpy as np\nfrom blitzar_amd import api\n"
            "assert api.init(api.SXT_GPU_BACKEND, 0) == 0\n"
            "table = np.zeros((1, 36), np.uint8)\ntable[0, 32] = 2\n"
            "need = api.check_sumcheck_evaluations_workspace_bytes(0, 1, 2)\n"
            "assert need > 0\n"
            "b = np.zeros(4096 + need, np.uint8)\n"
            "at = b.ctypes.data\n"
            "print('calling', flush=True)\n"
            "api.check_sumcheck_evaluations_device(0, 3, table, [0, 2], 1, at, at + 64, at + 512,\n"
            "                                      at + 1024, need - 1)\n"
            "print('returned', flush=True)\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode < 0, r.stdout + r.stderr
    assert "the evaluation check's workspace is too small" in r.stderr, r.stderr
    assert "calling" in r.stdout and "returned" not in r.stdout


#--------------------------------------------------------------------------------------------------
# combining compressed commitments
#--------------------------------------------------------------------------------------------------
def combine_on_device(lib_api, commitments, coefficients):
    """-> (valid, the encoding of `combined`); checks the launch count, the canaries and that the
    inputs are left alone"""
    import torch
    count = len(commitments)
    d_commitments, commitments_at = _guarded(commitments, 1)
    d_coefficients, coefficients_at = _guarded(coefficients)
    d_combined, combined_at = _guarded(np.zeros(160, np.uint8))
    valid = torch.full((2,), 7, dtype=torch.int32, device=_device())
    bytes_needed = api.combine_commitments_workspace_bytes(count)
    workspace = torch.full((bytes_needed + GUARD,), CANARY, dtype=torch.uint8, device=_device())
    side = torch.cuda.Stream(device=_device())
    torch.cuda.synchronize()
    before = _launches()
    lib_api.combine_commitments_device(count, commitments_at, coefficients_at, combined_at,
                                       valid.data_ptr(), workspace.data_ptr(), bytes_needed,
                                       stream=side.cuda_stream)
    assert _launches() - before >= 2, "the decode kernel and the engine's"
    side.synchronize()
    got_valid = valid.cpu().numpy()
    assert got_valid[1] == 7
    assert np.all(workspace.cpu().numpy()[bytes_needed:] == CANARY)
    assert np.array_equal(_payload(d_commitments, 1, 32 * count), np.asarray(commitments).reshape(-1))
    assert np.array_equal(_payload(d_coefficients, 0, 32 * count),
                          np.asarray(coefficients).reshape(-1))
    return int(got_valid[0]), encoding_of(_payload(d_combined, 0, 160).copy())


def check_combination(lib_api, case):
    valid, encoding = combine_on_device(lib_api, case.commitments, case.coefficients)
    assert valid == int(case.valid)
    assert np.array_equal(encoding, case.expected_encoding())
    host_valid, host_combined = lib_api.combine_commitments(case.commitments, case.coefficients)
    assert valid == int(host_valid)
    assert np.array_equal(encoding, encoding_of(host_combined))


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 3, 64, 65, 1000])
def test_combine_commitments_device(gpu_backend, count):
    check_combination(gpu_backend, Commitments(count, 700 + count))


@pytest.mark.gpu
@pytest.mark.parametrize("why", REJECTION_CLASSES)
def test_combine_commitments_device_rejected_encoding(gpu_backend, why):
    """valid = 0 and the sum of the other terms, as the host form; a later call on the same
    workspace size is not disturbed"""
    encoding = rejected_encodings()[why]
    for count, at in ((1, 0), (65, 64), (300, 7)):
        check_combination(gpu_backend, Commitments(count, 800 + count + at, {at: encoding}))
    check_combination(gpu_backend, Commitments(65, 899))


@pytest.mark.gpu
def test_combine_commitments_device_every_class_at_once(gpu_backend):
    encodings = rejected_encodings()
    rejected = {3 + 70 * k: encodings[why] for k, why in enumerate(REJECTION_CLASSES)}
    check_combination(gpu_backend, Commitments(300, 850, rejected))


@pytest.mark.gpu
def test_commitments_of_the_engine_combine_to_the_combined_columns(gpu_backend, oracle):
    """the commitments bzamd_msm_device wrote for three i64 columns combine to the commitment of
    sum_j c_j column_j, which the reference's CPU backend computes"""
    import torch
    n, p = 100, MODULUS[0]
    rng = np.random.default_rng(5151)
    columns = [rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64) for _ in range(3)]
    coefficients = [int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % p
                    for _ in range(3)]
    combined = as_bytes(0, [sum(c * int(col[i]) for c, col in zip(coefficients, columns))
                            for i in range(n)])
    generators = oracle.ristretto_generators(n, 0)
    want = oracle.msm_projective(0, [(combined, False)], generators)[0]

    keep = [_up(col.view(np.uint8)) for col in columns]
    desc = (api.sxt_sequence_descriptor * 3)()
    for j, d_col in enumerate(keep):
        desc[j] = api.sxt_sequence_descriptor(8, n, d_col.data_ptr(), 1)
    d_generators = _up(np.asarray(generators).view(np.uint8))
    d_commitments = torch.zeros((3, 32), dtype=torch.uint8, device=_device())
    d_coefficients = _up(as_bytes(0, coefficients))
    d_combined = torch.zeros(160, dtype=torch.uint8, device=_device())
    valid = torch.full((1,), 7, dtype=torch.int32, device=_device())
    workspace = torch.empty(api.combine_commitments_workspace_bytes(3), dtype=torch.uint8,
                            device=_device())
    side = torch.cuda.Stream(device=_device())
    torch.cuda.synchronize()
    before = _launches()
    api.load().bzamd_msm_device(0, d_commitments.data_ptr(), 3, desc, d_generators.data_ptr(),
                                side.cuda_stream)
    gpu_backend.combine_commitments_device(3, d_commitments.data_ptr(), d_coefficients.data_ptr(),
                                           d_combined.data_ptr(), valid.data_ptr(),
                                           workspace.data_ptr(), workspace.numel(),
                                           stream=side.cuda_stream)
    assert _launches() > before
    side.synchronize()
    assert int(valid.cpu().numpy()[0]) == 1
    assert np.array_equal(encoding_of(d_combined.cpu().numpy()),
                          encoding_of(np.asarray(want).view(np.uint8)))


#--------------------------------------------------------------------------------------------------
# the whole chain
#--------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_whole_chain_on_one_stream_with_the_verifier_on_device(gpu_backend):
    """tests/test_mle_opening_device.py::test_whole_chain_on_one_stream with nothing left to the
    host: the columns are committed by bzamd_msm_device, a_commit comes from
    bzamd_combine_commitments_device over those commitments, and the rounds and the final
    evaluations are checked by the two device calls on what the prover chain left in HBM.  One
    synchronise at the end; all three verdicts and `valid` are 1.

    Then one bit is flipped in turn in a round polynomial, in an evaluation and in a commitment,
    and the verifier's four calls run again.  The checks are chained through the running sum the
    rounds' verifier leaves, so in these runs the evaluation check reads the sum the accepted run
    left: exactly the check that owns the flipped byte then says 0."""
    import torch
    field_id, n, dev = 0, 600, _device()
    p = MODULUS[field_id]
    v = variables(n)
    proven = ProvenColumns(field_id, n, 4200)
    rng = np.random.default_rng(4201)
    coefficients = [int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % p
                    for _ in range(3)]
    # the claim: sum_i sum_p mult_p prod_{j in terms_p} column_j[i], columns zero past their end
    multipliers = [to_int(field_id, row[:32]) for row in proven.table]
    claimed = 0
    for i in range(n):
        for m, terms in zip(multipliers, proven.PRODUCTS):
            term = m
            for j in terms:
                term = term * (proven.values[j][i] if i < len(proven.values[j]) else 0) % p
            claimed = (claimed + term) % p

    d_generators = _up(gpu_backend.get_generators(n, 0).view(np.uint8))
    d_commitments = torch.zeros((3, 32), dtype=torch.uint8, device=dev)
    d_coefficients = _up(as_bytes(field_id, coefficients))
    combined = torch.full((n + 1, 32), CANARY, dtype=torch.uint8, device=dev)
    product = torch.zeros(32, dtype=torch.uint8, device=dev)
    t_sumcheck = merlin_ref.Transcript(label="opening").array()  # ProvenColumns' own
    t_open = merlin_ref.Transcript(label="open the evaluations").array()
    proof = DeviceProof(n, 0, combined, proven.vector, t_open)
    combine_workspace = torch.empty(api.combine_commitments_workspace_bytes(3), dtype=torch.uint8,
                                    device=dev)
    check_bytes = api.check_sumcheck_evaluations_workspace_bytes(field_id, 3, len(proven.terms))
    check_workspace = torch.empty(check_bytes, dtype=torch.uint8, device=dev)
    verify_workspace = torch.empty(api.inner_product_verify_workspace_bytes(n), dtype=torch.uint8,
                                   device=dev)

    class Verifier:
        """the verifier's four calls and what they write"""

        def __init__(self, polys, evaluations, commitments, sum_for_check=None):
            self.expected = _up(raw_element(field_id, claimed))
            self.point = torch.zeros((v, 32), dtype=torch.uint8, device=dev)
            self.verdicts = torch.full((3,), 7, dtype=torch.int32, device=dev)
            self.valid = torch.full((1,), 7, dtype=torch.int32, device=dev)
            self.a_commit = torch.zeros(160, dtype=torch.uint8, device=dev)
            self.t_sumcheck, self.t_open = _up(t_sumcheck), _up(t_open)
            self.polys, self.evaluations, self.commitments = polys, evaluations, commitments
            self.sum_for_check = self.expected if sum_for_check is None else sum_for_check

        def enqueue(self, side):
            words = self.verdicts.data_ptr()
            gpu_backend.verify_sumcheck_device(
                field_id, v, 3, 1, self.polys.data_ptr(), self.expected.data_ptr(),
                self.point.data_ptr(), self.t_sumcheck.data_ptr(), words, stream=side.cuda_stream)
            gpu_backend.check_sumcheck_evaluations_device(
                field_id, 3, proven.table, proven.terms, 1, self.sum_for_check.data_ptr(),
                self.evaluations.data_ptr(), words + 4, check_workspace.data_ptr(), check_bytes,
                stream=side.cuda_stream)
            gpu_backend.combine_commitments_device(
                3, self.commitments.data_ptr(), d_coefficients.data_ptr(), self.a_commit.data_ptr(),
                self.valid.data_ptr(), combine_workspace.data_ptr(), combine_workspace.numel(),
                stream=side.cuda_stream)
            gpu_backend.verify_inner_product_device(
                n, 0, proven.vector.data_ptr(), product.data_ptr(), self.a_commit.data_ptr(),
                proof.l.data_ptr(), proof.r.data_ptr(), proof.ap.data_ptr(), self.t_open.data_ptr(),
                words + 8, verify_workspace.data_ptr(), verify_workspace.numel(), None,
                stream=side.cuda_stream)

        def results(self):
            """-> ([rounds, evaluations, inner product], valid)"""
            return list(self.verdicts.cpu().numpy()), int(self.valid.cpu().numpy()[0])

    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    before = _launches()
    api.load().bzamd_msm_device(0, d_commitments.data_ptr(), 3, proven.desc,
                                d_generators.data_ptr(), side.cuda_stream)
    proven.enqueue_sumcheck_and_vector(gpu_backend, side)
    gpu_backend.combine_columns_device(field_id, proven.desc, d_coefficients.data_ptr(), n,
                                       combined.data_ptr(),
                                       evaluations_ptr=proven.evaluations.data_ptr(),
                                       product_ptr=product.data_ptr(), stream=side.cuda_stream)
    proof.enqueue(gpu_backend, side)
    honest = Verifier(proven.polys, proven.evaluations, d_commitments)
    honest.enqueue(side)
    assert _launches() > before
    side.synchronize()  # the only one

    assert honest.results() == ([1, 1, 1], 1)
    assert np.all(combined.cpu().numpy()[n] == CANARY)
    # the verifier drew the prover's point and left the prover's transcript
    assert np.array_equal(honest.point.cpu().numpy(), proven.point.cpu().numpy())
    assert np.array_equal(honest.t_sumcheck.cpu().numpy(), proven.transcript.cpu().numpy())
    assert np.array_equal(honest.t_open.cpu().numpy(), proof.transcript.cpu().numpy())

    def flipped_on_device(tensor, byte, bit):
        out = tensor.clone()
        out.view(-1)[byte] ^= 1 << bit
        return out

    good_sum = honest.expected.clone()
    tampered = [
        ("a round polynomial", [0, 1, 1],
         Verifier(flipped_on_device(proven.polys, 32 * 4 * (v // 2) + 37, 2), proven.evaluations,
                  d_commitments, good_sum)),
        ("an evaluation", [1, 0, 1],
         Verifier(proven.polys, flipped_on_device(proven.evaluations, 32 + 5, 0), d_commitments,
                  good_sum)),
        ("a commitment", [1, 1, 0],
         Verifier(proven.polys, proven.evaluations, flipped_on_device(d_commitments, 64 + 3, 4),
                  good_sum)),
    ]
    for _, _, verifier in tampered:
        verifier.enqueue(side)
    side.synchronize()
    for name, want, verifier in tampered:
        verdicts, valid = verifier.results()
        assert verdicts == want, name
        assert valid == 1 or name == "a commitment", name
