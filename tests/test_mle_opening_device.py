"""The device forms of the opening bridge (include/blitzar_amd.h:
bzamd_mle_evaluation_vector_device, bzamd_combine_columns_device), the host forms on the GPU
backend, the identity that ties the evaluation vector's bit order to the sumcheck prover, and the
whole chain on one stream: sumcheck over typed columns, evaluation vector, combination,
inner-product proof, verification.

Inputs and expected bytes are those of tests/test_mle_opening.py (Python integers); the sizes of
the evaluation vector follow the kernel's split (proof/mle_opening.hip): 5 low and 5 middle bits,
tiles of 1024 rows, at most 2048 workgroups."""

import numpy as np
import pytest

from blitzar_amd import api
from tests import merlin_ref
from tests.test_inner_product_device import DeviceProof, rounds_of
from tests.test_mle_opening import (KINDS, Columns, as_bytes, element_value, expected_vector,
                                    point_bytes, point_of, vector_entry)
from tests.test_sumcheck import elements, product_table
from tests.test_sumcheck_device import MODULUS, to_bytes, to_int
from tests.test_sumcheck_transcript import variables

TILE_ROWS = 1024     # 2^(kLowBits + kMidBits) of proof/mle_opening.hip
VECTOR_BLOCKS = 2048  # kVectorBlocks
COMBINE_CHUNK = 32   # kCombineChunk
CANARY = 0xA5


def _launches():
    return api.load().bzamd_kernel_launch_count()


def _device():
    import torch
    return torch.device("cuda", 0)


def _up(array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array).copy()).to(_device())


#--------------------------------------------------------------------------------------------------
# the evaluation vector
#--------------------------------------------------------------------------------------------------
def vector_on_device(lib_api, field_id, point, n):
    """-> uint8 [n, 32]; checks the launch count and the canary element behind the vector"""
    import torch
    d_point = _up(point_bytes(field_id, point))
    d_vector = torch.full(((n + 1), 32), CANARY, dtype=torch.uint8, device=_device())
    side = torch.cuda.Stream(device=_device())
    torch.cuda.synchronize()
    before = _launches()
    lib_api.mle_evaluation_vector_device(field_id, d_vector.data_ptr(), d_point.data_ptr(),
                                         len(point), n, stream=side.cuda_stream)
    assert _launches() - before == 1
    side.synchronize()
    got = d_vector.cpu().numpy()
    assert np.all(got[n] == CANARY), "the element behind the vector was written"
    assert np.array_equal(d_point.cpu().numpy(), point_bytes(field_id, point))
    return got[:n]


VECTOR_CASES = ([(1, 1), (1, 2), (2, 3), (5, 3), (9, 511), (9, 512), (10, 513), (15, (1 << 14) + 1),
                 (17, 1 << 17)]
                # one row short of a tile, the tile, one row into the second tile (the first row
                # whose high field is not zero), and a high field of two bits ending inside a tile
                + [(10, TILE_ROWS - 1), (10, TILE_ROWS), (11, TILE_ROWS + 1),
                   (12, 3 * TILE_ROWS + 7)]
                # fewer variables than low bits, than low and middle bits, and more than n needs
                + [(4, 16), (7, 100), (30, 3), (30, 2 * TILE_ROWS + 1)])


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("v,n", VECTOR_CASES)
def test_evaluation_vector_device_form(gpu_backend, field_id, v, n):
    point = point_of(field_id, v, 100 + v + n)
    got = vector_on_device(gpu_backend, field_id, point, n)
    assert np.array_equal(got, as_bytes(field_id, expected_vector(field_id, point, n)))


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_evaluation_vector_random_point(gpu_backend, field_id):
    """no special entry in the point: no factor of a row is 0 or 1"""
    p = MODULUS[field_id]
    rng = np.random.default_rng(77)
    point = [int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % p
             for _ in range(12)]
    n = 2 * TILE_ROWS + 300
    got = vector_on_device(gpu_backend, field_id, point, n)
    assert np.array_equal(got, as_bytes(field_id, expected_vector(field_id, point, n)))


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_evaluation_vector_more_tiles_than_workgroups(gpu_backend, field_id):
    """2050 tiles on 2048 workgroups: two workgroups walk a second tile.  The first and the last two
    tiles whole, 1500 rows in between, each from the definition"""
    v, n = 22, VECTOR_BLOCKS * TILE_ROWS + TILE_ROWS + 1
    point = point_of(field_id, v, 9)
    point[0] = MODULUS[field_id] - 2  # not 0 or 1: the second half of the rows is not zero
    got = vector_on_device(gpu_backend, field_id, point, n)
    rng = np.random.default_rng(3)
    rows = (list(range(2 * TILE_ROWS)) + list(range(n - 2 * TILE_ROWS - 1, n))
            + [int(i) for i in rng.integers(0, n, 1500)])
    want = as_bytes(field_id, [vector_entry(field_id, point, i) for i in rows])
    assert np.array_equal(got[rows], want)


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("v,n", [(1, 1), (5, 3), (12, 2 * TILE_ROWS + 1)])
def test_evaluation_vector_host_form_on_gpu(gpu_backend, field_id, v, n):
    point = point_of(field_id, v, 5)
    before = _launches()
    got = gpu_backend.mle_evaluation_vector(field_id, point_bytes(field_id, point), n)
    assert _launches() - before == 1, "no kernel ran"
    assert np.array_equal(got, as_bytes(field_id, expected_vector(field_id, point, n)))


#--------------------------------------------------------------------------------------------------
# the combination
#--------------------------------------------------------------------------------------------------
def combine_on_device(lib_api, case, with_evaluations=True, with_product=True):
    """-> (combined uint8 [n, 32], product uint8 [32]); checks the launch count, the canary behind
    `combined` and that every input is byte for byte what it was"""
    import torch
    n, field_id = case.n, case.field_id
    d_flat = _up(case.flat)
    d_coefficients = _up(case.coefficient_bytes())
    d_evaluations = _up(case.evaluation_bytes())
    d_combined = torch.full((n + 1, 32), CANARY, dtype=torch.uint8, device=_device())
    d_product = torch.full((32,), 0x5A, dtype=torch.uint8, device=_device())
    side = torch.cuda.Stream(device=_device())
    torch.cuda.synchronize()
    before = _launches()
    lib_api.combine_columns_device(
        field_id, case.device_descriptors(d_flat.data_ptr()), d_coefficients.data_ptr(), n,
        d_combined.data_ptr(),
        evaluations_ptr=d_evaluations.data_ptr() if with_evaluations else None,
        product_ptr=d_product.data_ptr() if with_product else None, stream=side.cuda_stream)
    chunks = (len(case.specs) + COMBINE_CHUNK - 1) // COMBINE_CHUNK
    assert _launches() - before == chunks + (1 if with_evaluations and with_product else 0)
    side.synchronize()
    got = d_combined.cpu().numpy()
    assert np.all(got[n] == CANARY), "the element behind `combined` was written"
    assert np.array_equal(d_flat.cpu().numpy(), case.flat), "the columns were modified"
    assert np.array_equal(d_coefficients.cpu().numpy(), case.coefficient_bytes())
    assert np.array_equal(d_evaluations.cpu().numpy(), case.evaluation_bytes())
    return got[:n], d_product.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1000])
@pytest.mark.parametrize("num_columns", [1, 2, 7, 33])
def test_combination_device_form(gpu_backend, field_id, n, num_columns):
    """the kinds, lengths, placements and extreme rows of tests/test_mle_opening.py Columns; 33
    columns take a second launch that adds to the first one's rows"""
    for shift in ((0, 1, 2, 3) if num_columns != 33 else (n % 4,)):
        case = Columns(field_id, n, num_columns, 1000 * num_columns + n + shift, shift)
        combined, product = combine_on_device(gpu_backend, case)
        assert np.array_equal(combined, case.expected_combined()), f"shift {shift}"
        assert np.array_equal(product, case.expected_product()), f"shift {shift}"


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_every_kind_at_every_length_and_placement(gpu_backend, field_id):
    """six columns, one of each kind, four shifts: kinds x lengths and kinds x placements (byte path
    at 1 and 3 past a multiple of 8, word path on one)"""
    for shift in (0, 1, 2, 3):
        case = Columns(field_id, 257, len(KINDS), 60 + shift, shift)
        combined, product = combine_on_device(gpu_backend, case)
        assert np.array_equal(combined, case.expected_combined()), f"shift {shift}"
        assert np.array_equal(product, case.expected_product()), f"shift {shift}"


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_product_is_written_only_with_evaluations(gpu_backend, field_id):
    case = Columns(field_id, 300, 7, 70)
    for with_evaluations, with_product in ((False, True), (True, False)):
        combined, product = combine_on_device(gpu_backend, case, with_evaluations, with_product)
        assert np.array_equal(combined, case.expected_combined())
        assert np.all(product == 0x5A), "product was written"


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_more_rows_than_one_sweep(gpu_backend, field_id):
    """4096 workgroups of 256 rows cover 2^20 rows: one i64 column of 2^20 + 300 rows, where the
    first lanes take a second row; sampled rows from the definition, the ends whole"""
    p, n = MODULUS[field_id], (1 << 20) + 300
    import torch
    rng = np.random.default_rng(8)
    column = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
    c = int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % p
    d_column, d_c = _up(column.view(np.uint8)), _up(to_bytes(field_id, c))
    d_combined = torch.full((n + 1, 32), CANARY, dtype=torch.uint8, device=_device())
    side = torch.cuda.Stream(device=_device())
    torch.cuda.synchronize()
    gpu_backend.combine_columns_device(field_id, [(d_column.data_ptr(), n, 8, True)],
                                       d_c.data_ptr(), n, d_combined.data_ptr(),
                                       stream=side.cuda_stream)
    side.synchronize()
    got = d_combined.cpu().numpy()
    assert np.all(got[n] == CANARY)
    rows = (list(range(600)) + list(range(n - 600, n))
            + [int(i) for i in rng.integers(0, n, 1500)])
    want = as_bytes(field_id, [c * int(column[i]) for i in rows])
    assert np.array_equal(got[rows], want)


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("n,num_columns", [(1, 1), (257, 7), (300, 33)])
def test_combination_host_form_on_gpu(gpu_backend, field_id, n, num_columns):
    case = Columns(field_id, n, num_columns, 80 + n, 1)
    columns = case.host_columns()
    product = np.full(32, 0x5A, np.uint8)
    before = _launches()
    combined, _ = gpu_backend.combine_columns(field_id, columns, case.coefficient_bytes(), n,
                                              case.evaluation_bytes(), product)
    assert _launches() > before, "no kernel ran"
    assert np.array_equal(combined, case.expected_combined())
    assert np.array_equal(product, case.expected_product())
    for (got, _), (want, _) in zip(columns, case.arrays):
        assert np.array_equal(got, want), "a column was modified"
    untouched = np.full(32, 0x5A, np.uint8)
    combined, _ = gpu_backend.combine_columns(field_id, columns, case.coefficient_bytes(), n, None,
                                              untouched)
    assert np.array_equal(combined, case.expected_combined())
    assert np.all(untouched == 0x5A)


#--------------------------------------------------------------------------------------------------
# behind the sumcheck prover
#--------------------------------------------------------------------------------------------------
class ProvenColumns:
    """an i64, a 1-byte unsigned and a 32-byte column of n, n - 1 and n rows (n = 1: 1, 0, 1) on the
    device, and one bzamd_prove_sumcheck_transcript_device_columns call over them"""
    PRODUCTS = [[0, 1, 2], [2, 2], [0]]

    def __init__(self, field_id, n, seed):
        import torch
        p = MODULUS[field_id]
        rng = np.random.default_rng(seed)
        self.field_id, self.n = field_id, n
        self.host = [rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64).view(np.uint8).reshape(n, 8),
                     rng.integers(0, 256, (n - 1, 1), dtype=np.uint8),
                     elements(rng, field_id, n)]
        self.signed = [True, False, False]
        self.values = []
        for c, signed in zip(self.host, self.signed):
            if c.shape[1] == 32:
                self.values.append([element_value(field_id, row) for row in c])
            else:
                self.values.append([int.from_bytes(row.tobytes(), "little", signed=signed) % p
                                    for row in c])
        self.keep = [_up(c.reshape(-1)) for c in self.host]
        self.desc = (api.sxt_sequence_descriptor * 3)()
        for j, (c, signed) in enumerate(zip(self.host, self.signed)):
            self.desc[j] = api.sxt_sequence_descriptor(
                c.shape[1], len(c), self.keep[j].data_ptr() if len(c) else None, int(signed))
        self.terms = [i for t in self.PRODUCTS for i in t]
        self.table = product_table(field_id, elements(rng, field_id, 3), [3, 2, 1],
                                   api.SUMCHECK_PRODUCT_STRIDE[field_id])
        v = variables(n)
        dev = _device()
        self.polys = torch.zeros((v, 4, 32), dtype=torch.uint8, device=dev)
        self.point = torch.zeros((v, 32), dtype=torch.uint8, device=dev)
        self.evaluations = torch.zeros((3, 32), dtype=torch.uint8, device=dev)
        self.transcript = _up(merlin_ref.Transcript(label="opening").array())
        self.workspace_bytes = api.sumcheck_transcript_columns_workspace_bytes(
            field_id, n, 3, 3, len(self.terms), 3)
        self.workspace = torch.empty(self.workspace_bytes, dtype=torch.uint8, device=dev)
        self.vector = torch.full((n + 1, 32), CANARY, dtype=torch.uint8, device=dev)

    def enqueue_sumcheck_and_vector(self, lib_api, side):
        lib_api.prove_sumcheck_transcript_device_columns(
            self.field_id, self.desc, self.table, self.terms, self.n, 3, self.polys.data_ptr(),
            self.point.data_ptr(), self.evaluations.data_ptr(), self.transcript.data_ptr(),
            self.workspace.data_ptr(), self.workspace_bytes, stream=side.cuda_stream)
        # no synchronise: the point is read in stream order
        lib_api.mle_evaluation_vector_device(self.field_id, self.vector.data_ptr(),
                                             self.point.data_ptr(), variables(self.n), self.n,
                                             stream=side.cuda_stream)

    def check_identity(self):
        """<column_j, vector> = mle_evaluations[j], in Python integers"""
        p, field_id, n = MODULUS[self.field_id], self.field_id, self.n
        got = self.vector.cpu().numpy()
        assert np.all(got[n] == CANARY)
        vector = [to_int(field_id, row) for row in got[:n]]
        evaluations = self.evaluations.cpu().numpy()
        for j, values in enumerate(self.values):
            opened = sum(x * b for x, b in zip(values, vector)) % p
            assert opened == to_int(field_id, evaluations[j]), f"column {j}"
        return vector


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("n", [1, 5, 600, 4097])
def test_vector_opens_the_provers_evaluations(gpu_backend, field_id, n):
    """the bit order of the evaluation vector is the prover's: the prover is pinned to the compiled
    reference by tests/test_sumcheck_transcript_columns.py"""
    import torch
    proven = ProvenColumns(field_id, n, 4000 + n)
    side = torch.cuda.Stream(device=_device())
    torch.cuda.synchronize()
    before = _launches()
    proven.enqueue_sumcheck_and_vector(gpu_backend, side)
    assert _launches() > before
    side.synchronize()
    vector = proven.check_identity()
    point = [to_int(field_id, r) for r in proven.point.cpu().numpy()]
    assert vector == expected_vector(field_id, point, n)


@pytest.mark.gpu
def test_whole_chain_on_one_stream(gpu_backend, oracle):
    """sumcheck, evaluation vector, combination, inner-product proof and its verification enqueued
    on one stream with one synchronise at the end: the verifier accepts the product the combination
    made of the sumcheck's evaluations, and rejects it with one bit flipped.  `combined` depends on
    the columns and the coefficients alone, so its commitment is made beforehand from the Python
    expectation, the way tests/test_inner_product_verify_device.py Statement makes one"""
    import torch
    field_id, n, dev = 0, 600, _device()
    p = MODULUS[field_id]
    proven = ProvenColumns(field_id, n, 4100)
    rng = np.random.default_rng(4101)
    coefficients = [int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % p
                    for _ in range(3)]
    want_combined = [0] * n
    for c, values in zip(coefficients, proven.values):
        for i, x in enumerate(values):
            want_combined[i] = (want_combined[i] + c * x) % p
    want_combined = as_bytes(field_id, want_combined)
    commit = oracle.msm_projective(0, [(want_combined, False)], oracle.ristretto_generators(n, 0))[0]

    d_coefficients = _up(as_bytes(field_id, coefficients))
    d_commit = _up(np.asarray(commit).view(np.uint8))
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
    before = _launches()
    proven.enqueue_sumcheck_and_vector(gpu_backend, side)
    gpu_backend.combine_columns_device(field_id, proven.desc, d_coefficients.data_ptr(), n,
                                       combined.data_ptr(),
                                       evaluations_ptr=proven.evaluations.data_ptr(),
                                       product_ptr=product.data_ptr(), stream=side.cuda_stream)
    proof.enqueue(gpu_backend, side)
    enqueue_verify(product, verdict, verify_transcript, side)
    assert _launches() > before
    side.synchronize()

    assert int(verdict.cpu().numpy()[0]) == 1, "the verifier rejected the opening"
    vector = proven.check_identity()
    got_combined = combined.cpu().numpy()
    assert np.all(got_combined[n] == CANARY)
    assert np.array_equal(got_combined[:n], want_combined)
    evaluations = [to_int(field_id, e) for e in proven.evaluations.cpu().numpy()]
    want_product = sum(c * e for c, e in zip(coefficients, evaluations)) % p
    assert np.array_equal(product.cpu().numpy(), to_bytes(field_id, want_product))
    # which is the inner product of the two vectors
    assert sum(to_int(field_id, a) * b for a, b in zip(got_combined[:n], vector)) % p == want_product

    # the same bytes and transcript as the host entry point on the downloaded vectors
    host_vector = proven.vector.cpu().numpy()[:n]
    want = gpu_backend.prove_inner_product(t0, n, 0, got_combined[:n].copy(), host_vector.copy())
    rounds = rounds_of(n)
    for name, g, w in zip(("L", "R", "ap", "transcript"), proof.results(), want):
        assert np.array_equal(g, w), f"{name} differs from sxt_curve25519_prove_inner_product"
    assert rounds == len(want[0])

    # one bit of the product flipped: rejected
    flipped = product.clone()
    flipped[0] ^= 1
    verdict_flipped = torch.full((1,), 7, dtype=torch.int32, device=dev)
    enqueue_verify(flipped, verdict_flipped, _up(t0), side)
    side.synchronize()
    assert int(verdict_flipped.cpu().numpy()[0]) == 0, "a wrong product was accepted"
