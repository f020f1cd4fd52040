"""The device form of the column evaluation (include/blitzar_amd.h: bzamd_evaluate_columns_device),
the host form on the GPU backend, the identity that ties it to the sumcheck prover's own
evaluations, and the chain from the sumcheck to the verified opening with every evaluation computed
by the library.

Inputs and expected bytes are those of tests/test_evaluate_columns.py and tests/test_mle_opening.py
(Python integers); the sizes follow the kernel's constants (proof/mle_opening.hip), mirrored below."""
import os
import subprocess
import sys

import numpy as np
import pytest

from blitzar_amd import api
from tests import merlin_ref
from tests.test_evaluate_columns import expected_evaluations, vector_of
from tests.test_inner_product_device import DeviceProof
from tests.test_mle_opening import Columns, as_bytes, element_value
from tests.test_mle_opening_device import ProvenColumns
from tests.test_sumcheck_device import MODULUS, to_bytes, to_int

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = 256   # kEvaluateThreads
BLOCKS = 1024   # kEvaluateBlocks: the grid's cap
CHUNK = 8       # kEvaluateChunk: columns to a launch of the partial sums
SWEEP = 4       # kEvaluateSweep: rows a lane adds between two carry sweeps
CANARY = 0xA5


def _launches():
    return api.load().bzamd_kernel_launch_count()


def _device():
    import torch
    return torch.device("cuda", 0)


def _up(array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array).copy()).to(_device())


def launches_of(num_columns):
    return (num_columns + CHUNK - 1) // CHUNK + 1


class Resident:
    """a flat column buffer and a vector on the device, with what they held on the host"""

    def __init__(self, flat, vector):
        self.flat, self.vector = flat, vector
        self.d_flat, self.d_vector = _up(flat), _up(vector)

    def check_untouched(self):
        assert np.array_equal(self.d_vector.cpu().numpy(), self.vector), "the vector was modified"
        assert np.array_equal(self.d_flat.cpu().numpy(), self.flat), "the columns were modified"


def enqueue(lib_api, field_id, resident, specs, n, side, d_workspace, offset=0):
    """one call over the (offset in flat, rows, width, signed) columns -> the evaluations' tensor,
    one canary element behind them; asserts the launches the call counted"""
    import torch
    d_evaluations = torch.full((len(specs) + 1, 32), CANARY, dtype=torch.uint8, device=_device())
    descriptors = [(resident.d_flat.data_ptr() + o, rows, w, s) for o, rows, w, s in specs]
    workspace_bytes = api.evaluate_columns_workspace_bytes(field_id, len(specs), n)
    assert workspace_bytes > 0 and d_workspace.numel() >= offset + workspace_bytes
    before = _launches()
    lib_api.evaluate_columns_device(field_id, descriptors, resident.d_vector.data_ptr(), n,
                                    d_evaluations.data_ptr(), d_workspace.data_ptr() + offset,
                                    workspace_bytes, stream=side.cuda_stream)
    assert _launches() - before == launches_of(len(specs))
    return d_evaluations


def evaluate_on_device(lib_api, field_id, resident, specs, n, offset=0):
    """-> uint8 [num_columns, 32]; side stream, one synchronise; checks the launch count, the canary
    behind the evaluations, the canaries around the workspace and that no input changed"""
    import torch
    workspace_bytes = api.evaluate_columns_workspace_bytes(field_id, len(specs), n)
    d_workspace = torch.full((offset + workspace_bytes + 64,), CANARY, dtype=torch.uint8,
                             device=_device())
    side = torch.cuda.Stream(device=_device())
    torch.cuda.synchronize()
    d_evaluations = enqueue(lib_api, field_id, resident, specs, n, side, d_workspace, offset)
    side.synchronize()
    got = d_evaluations.cpu().numpy()
    assert np.all(got[len(specs)] == CANARY), "the element behind the evaluations was written"
    workspace = d_workspace.cpu().numpy()
    assert np.all(workspace[:offset] == CANARY), "the bytes before the workspace were written"
    assert np.all(workspace[offset + workspace_bytes:] == CANARY), \
        "the bytes behind the workspace were written"
    resident.check_untouched()
    return got[:len(specs)]


#--------------------------------------------------------------------------------------------------
# the device form
#--------------------------------------------------------------------------------------------------
DEVICE_CASES = [(1, 1), (2, 6), (255, 6), (256, 6), (257, 7), (300, CHUNK), (300, CHUNK + 1),
                (300, 2 * CHUNK + 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("n,num_columns", DEVICE_CASES)
def test_evaluation_device_form(gpu_backend, field_id, n, num_columns):
    """the kinds, lengths, placements (0, 1 and 3 past a multiple of 8) and extreme rows of
    tests/test_mle_opening.py Columns against a vector with 0, 1, p - 1 and an unreduced entry; one
    chunk, one column more, and two chunks and three columns"""
    for shift in ((0, 1, 2, 3) if n == 257 else (0,)):
        case = Columns(field_id, n, num_columns, 3000 * num_columns + n + shift, shift)
        vector = vector_of(field_id, n, 11 + shift)
        got = evaluate_on_device(gpu_backend, field_id, Resident(case.flat, vector), case.specs, n)
        assert np.array_equal(got, expected_evaluations(field_id, case.values, vector)), \
            f"shift {shift}"


def raw_rows(array):
    """the little-endian integer of every row of a uint8 [rows, width] array"""
    data = np.ascontiguousarray(array)
    width = data.shape[1]
    buffer = data.tobytes()
    return [int.from_bytes(buffer[k:k + width], "little") for k in range(0, len(buffer), width)]


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_second_trip_of_the_grid_stride_loop(gpu_backend, field_id):
    """one row more than the capped grid covers, and 299 beyond: the first 300 lanes take a second
    row.  An i64 column of n rows and a 32-byte column of n - 1 rows against a random vector (every
    entry below 2^252, canonical in both fields); the expectation is the definition"""
    p, n = MODULUS[field_id], BLOCKS * THREADS + 300
    rng = np.random.default_rng(31 + field_id)
    narrow = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
    wide = rng.integers(0, 256, (n - 1, 32), dtype=np.uint8)
    vector = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    wide[:, 31] &= 0x0F
    vector[:, 31] &= 0x0F
    flat = np.concatenate([narrow.view(np.uint8), wide.reshape(-1)])
    specs = [(0, n, 8, True), (8 * n, n - 1, 32, False)]
    got = evaluate_on_device(gpu_backend, field_id, Resident(flat, vector), specs, n)
    # 32 bytes mean raw / 2^256 in field 1: taken out of the sums once
    b = raw_rows(vector)
    out = pow(1 << 256, -1, p) if field_id == 1 else 1
    want = [sum(int(x) * y for x, y in zip(narrow, b)) * out,
            sum(x * y for x, y in zip(raw_rows(wide), b)) * out * out]
    assert np.array_equal(got, as_bytes(field_id, want))


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_lazy_accumulation_at_its_bound(gpu_backend, field_id):
    """the largest rows against the largest entries: an unsigned 31-byte column of 0xFF bytes and a
    signed 16-byte column of -2^127 against a vector of p - 1 (field 0: also of 2^256 - 1, sixteen
    times the modulus).  n = twice the sweep interval for every lane of the capped grid, and one row
    short of seven rows a lane (all lanes end between two sweeps, n = 3 mod 4).  Closed form:
    n * X * B"""
    p = MODULUS[field_id]
    n_full = BLOCKS * THREADS * 2 * SWEEP
    n_short = BLOCKS * THREADS * (2 * SWEEP - 1) - 1
    assert n_short % SWEEP == SWEEP - 1
    flat = np.concatenate([np.full(31 * n_full, 0xFF, np.uint8),
                           np.tile(np.frombuffer((-(1 << 127)).to_bytes(16, "little", signed=True),
                                                 np.uint8), n_full)])
    rows = [(1 << 248) - 1, -(1 << 127)]
    entries = [to_bytes(field_id, p - 1)]
    if field_id == 0:
        entries.append(np.full(32, 0xFF, np.uint8))
    for entry in entries:
        resident = Resident(flat, np.tile(entry, (n_full, 1)))
        b = element_value(field_id, entry)
        for n in (n_full, n_short):
            specs = [(0, n, 31, False), (31 * n_full, n, 16, True)]
            got = evaluate_on_device(gpu_backend, field_id, resident, specs, n)
            assert np.array_equal(got, as_bytes(field_id, [n * x * b for x in rows])), f"n = {n}"


#--------------------------------------------------------------------------------------------------
# the workspace
#--------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_workspace_exact_and_misaligned(gpu_backend, field_id):
    """exactly workspace_bytes at a pointer one byte past an allocation's start: the same result,
    and nothing written before or behind it"""
    n, num_columns = 700, CHUNK + 2
    case = Columns(field_id, n, num_columns, 510, 2)
    vector = vector_of(field_id, n, 51)
    got = evaluate_on_device(gpu_backend, field_id, Resident(case.flat, vector), case.specs, n,
                             offset=1)
    assert np.array_equal(got, expected_evaluations(field_id, case.values, vector))


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_two_calls_share_the_workspace(gpu_backend, field_id):
    import torch
    first = Columns(field_id, 600, CHUNK + 1, 520, 0)
    second = Columns(field_id, 300, 3, 521, 1)
    vectors = [vector_of(field_id, 600, 52), vector_of(field_id, 300, 53)]
    residents = [Resident(first.flat, vectors[0]), Resident(second.flat, vectors[1])]
    workspace_bytes = max(api.evaluate_columns_workspace_bytes(field_id, CHUNK + 1, 600),
                          api.evaluate_columns_workspace_bytes(field_id, 3, 300))
    d_workspace = torch.full((workspace_bytes + 64,), CANARY, dtype=torch.uint8, device=_device())
    side = torch.cuda.Stream(device=_device())
    torch.cuda.synchronize()
    before = _launches()
    d_first = enqueue(gpu_backend, field_id, residents[0], first.specs, 600, side, d_workspace)
    d_second = enqueue(gpu_backend, field_id, residents[1], second.specs, 300, side, d_workspace)
    assert _launches() - before == launches_of(CHUNK + 1) + launches_of(3)
    side.synchronize()
    for d_got, case, vector, resident in zip((d_first, d_second), (first, second), vectors, residents):
        got = d_got.cpu().numpy()
        assert np.all(got[-1] == CANARY)
        assert np.array_equal(got[:-1], expected_evaluations(field_id, case.values, vector))
        resident.check_untouched()
    assert np.all(d_workspace.cpu().numpy()[workspace_bytes:] == CANARY)


@pytest.mark.gpu
def test_workspace_one_byte_short_aborts():
    """in a child process on the GPU backend, at n = 1: the size is checked before anything is
    enqueued"""
    code = ("import torch\nfrom blitzar_amd import api\n"
            "assert api.init(api.SXT_GPU_BACKEND, 0) == 0\n"
            "dev = torch.device('cuda', 0)\n"
            "column = torch.ones(8, dtype=torch.uint8, device=dev)\n"
            "vector = torch.zeros(32, dtype=torch.uint8, device=dev)\n"
            "out = torch.zeros(32, dtype=torch.uint8, device=dev)\n"
            "size = api.evaluate_columns_workspace_bytes(0, 1, 1)\n"
            "work = torch.zeros(size, dtype=torch.uint8, device=dev)\n"
            "torch.cuda.synchronize()\n"
            "api.evaluate_columns_device(0, [(column.data_ptr(), 1, 8, False)], vector.data_ptr(),\n"
            "    1, out.data_ptr(), work.data_ptr(), size - 1)\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode < 0 and "the column evaluation workspace is too small" in r.stderr, r.stderr


#--------------------------------------------------------------------------------------------------
# the host form on the GPU backend
#--------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("n,num_columns", [(1, 1), (257, 7), (300, CHUNK + 1)])
def test_evaluation_host_form_on_gpu(gpu_backend, field_id, n, num_columns):
    case = Columns(field_id, n, num_columns, 580 + n, 1)
    vector = vector_of(field_id, n, 58)
    columns, passed = case.host_columns(), vector.copy()
    before = _launches()
    got = gpu_backend.evaluate_columns(field_id, columns, passed, n)
    assert _launches() - before == launches_of(num_columns), "no kernel ran"
    assert np.array_equal(got, expected_evaluations(field_id, case.values, vector))
    assert np.array_equal(passed, vector), "the vector was modified"
    for (after, _), (earlier, _) in zip(columns, case.arrays):
        assert np.array_equal(after, earlier), "a column was modified"


#--------------------------------------------------------------------------------------------------
# behind the sumcheck prover
#--------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("n", [1, 5, 600, 4097])
def test_evaluation_equals_the_provers(gpu_backend, field_id, n):
    """sum_i T_0[j][i] vector[i] = mle_evaluations[j], the header's identity, computed by the
    library on the stream of the prover and the evaluation vector with no synchronise in between.
    The prover is pinned to the compiled reference by tests/test_sumcheck_transcript_columns.py"""
    import torch
    proven = ProvenColumns(field_id, n, 6000 + n)
    workspace_bytes = api.evaluate_columns_workspace_bytes(field_id, 3, n)
    d_workspace = torch.empty(workspace_bytes, dtype=torch.uint8, device=_device())
    d_evaluations = torch.full((4, 32), CANARY, dtype=torch.uint8, device=_device())
    flat_before = [keep.cpu().numpy() for keep in proven.keep]
    side = torch.cuda.Stream(device=_device())
    torch.cuda.synchronize()
    proven.enqueue_sumcheck_and_vector(gpu_backend, side)
    before = _launches()
    gpu_backend.evaluate_columns_device(field_id, proven.desc, proven.vector.data_ptr(), n,
                                        d_evaluations.data_ptr(), d_workspace.data_ptr(),
                                        workspace_bytes, stream=side.cuda_stream)
    assert _launches() - before == launches_of(3)
    side.synchronize()
    got = d_evaluations.cpu().numpy()
    assert np.all(got[3] == CANARY)
    assert np.array_equal(got[:3], proven.evaluations.cpu().numpy())
    vector = proven.check_identity()  # the same identity in Python integers; the canary behind it
    assert np.array_equal(proven.vector.cpu().numpy()[:n], as_bytes(field_id, vector))
    for keep, earlier in zip(proven.keep, flat_before):
        assert np.array_equal(keep.cpu().numpy(), earlier), "a column was modified"


@pytest.mark.gpu
def test_chain_with_the_librarys_evaluations(gpu_backend, oracle):
    """the sequence of tests/test_mle_opening_device.py test_whole_chain_on_one_stream over four
    columns, the prover's three and an i32 column the sumcheck never saw: sumcheck, evaluation
    vector, the four evaluations, combination with `product`, inner-product proof and verification
    on one stream with one synchronise.  The verifier accepts, and rejects with one bit of the
    product flipped"""
    import torch
    field_id, n, dev = 0, 600, _device()
    p = MODULUS[field_id]
    proven = ProvenColumns(field_id, n, 6100)
    rng = np.random.default_rng(6101)
    fourth = rng.integers(-2**31, 2**31 - 1, n, dtype=np.int32)
    d_fourth = _up(fourth.view(np.uint8))
    values = proven.values + [[int(x) % p for x in fourth]]
    desc = (api.sxt_sequence_descriptor * 4)()
    for j in range(3):
        desc[j] = proven.desc[j]
    desc[3] = api.sxt_sequence_descriptor(4, n, d_fourth.data_ptr(), 1)
    coefficients = [int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % p
                    for _ in range(4)]
    want_combined = [0] * n
    for c, column in zip(coefficients, values):
        for i, x in enumerate(column):
            want_combined[i] = (want_combined[i] + c * x) % p
    want_combined = as_bytes(field_id, want_combined)
    commit = oracle.msm_projective(0, [(want_combined, False)], oracle.ristretto_generators(n, 0))[0]

    d_coefficients = _up(as_bytes(field_id, coefficients))
    d_commit = _up(np.asarray(commit).view(np.uint8))
    evaluations = torch.full((5, 32), CANARY, dtype=torch.uint8, device=dev)
    workspace_bytes = api.evaluate_columns_workspace_bytes(field_id, 4, n)
    d_workspace = torch.empty(workspace_bytes, dtype=torch.uint8, device=dev)
    combined = torch.full((n + 1, 32), CANARY, dtype=torch.uint8, device=dev)
    product = torch.zeros(32, dtype=torch.uint8, device=dev)
    t0 = merlin_ref.Transcript(label="open the evaluations").array()
    proof = DeviceProof(n, 0, combined, proven.vector, t0)
    verdict = torch.full((1,), 7, dtype=torch.int32, device=dev)
    verify_transcript = _up(t0)
    verify_workspace = torch.empty(api.inner_product_verify_workspace_bytes(n), dtype=torch.uint8,
                                   device=dev)

    def enqueue_verify(d_product, d_verdict, d_transcript, side):
        gpu_backend.verify_inner_product_device(
            n, 0, proven.vector.data_ptr(), d_product.data_ptr(), d_commit.data_ptr(),
            proof.l.data_ptr(), proof.r.data_ptr(), proof.ap.data_ptr(), d_transcript.data_ptr(),
            d_verdict.data_ptr(), verify_workspace.data_ptr(), verify_workspace.numel(), None,
            stream=side.cuda_stream)

    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    proven.enqueue_sumcheck_and_vector(gpu_backend, side)
    before = _launches()
    gpu_backend.evaluate_columns_device(field_id, desc, proven.vector.data_ptr(), n,
                                        evaluations.data_ptr(), d_workspace.data_ptr(),
                                        workspace_bytes, stream=side.cuda_stream)
    assert _launches() - before == launches_of(4)
    gpu_backend.combine_columns_device(field_id, desc, d_coefficients.data_ptr(), n,
                                       combined.data_ptr(), evaluations_ptr=evaluations.data_ptr(),
                                       product_ptr=product.data_ptr(), stream=side.cuda_stream)
    proof.enqueue(gpu_backend, side)
    enqueue_verify(product, verdict, verify_transcript, side)
    side.synchronize()

    assert int(verdict.cpu().numpy()[0]) == 1, "the verifier rejected the opening"
    vector = proven.check_identity()
    got = evaluations.cpu().numpy()
    assert np.all(got[4] == CANARY)
    assert np.array_equal(got[:3], proven.evaluations.cpu().numpy())
    opened = [sum(x * b for x, b in zip(column, vector)) for column in values]
    assert np.array_equal(got[:4], as_bytes(field_id, opened))
    got_combined = combined.cpu().numpy()
    assert np.all(got_combined[n] == CANARY)
    assert np.array_equal(got_combined[:n], want_combined)
    want_product = sum(c * to_int(field_id, e) for c, e in zip(coefficients, got[:4])) % p
    assert np.array_equal(product.cpu().numpy(), to_bytes(field_id, want_product))

    # one bit of the product flipped: rejected
    flipped = product.clone()
    flipped[0] ^= 1
    verdict_flipped = torch.full((1,), 7, dtype=torch.int32, device=dev)
    enqueue_verify(flipped, verdict_flipped, _up(t0), side)
    side.synchronize()
    assert int(verdict_flipped.cpu().numpy()[0]) == 0, "a wrong product was accepted"
