"""The device forms of the univariate-opening entry points (include/blitzar_amd.h:
bzamd_fold_polynomial_device, bzamd_evaluate_polynomials_device, bzamd_batch_quotients_device), the
host forms on the GPU backend, and the whole chain of a HyperKZG opening on one stream, checked
without a pairing.

Expected values are those of tests/univariate_cases.py (Python integers) and every comparison is of
bytes.  The sizes follow the kernels' constants (proof/univariate_opening.hip): the fold's tile of
2^10 rows on at most 1024 workgroups, four rows a lane and 1024 rows a tile in the evaluation and
the division, at most 1024 chunks of a whole number of tiles per level, 256 chunks per pass of the
carry scan."""
import functools
import hashlib

import numpy as np
import pytest

from blitzar_amd import api
from tests import univariate_cases as uc
from tests.test_mle_opening import point_of
from tests.test_sumcheck_device import MODULUS, to_bytes

FOLD_LEVELS = 10               # kFoldLevels
T = 1 << FOLD_LEVELS           # kFoldTile
FOLD_BLOCKS = 1024             # kFoldBlocks
LANE_ROWS = 4                  # kLaneRows
W = Q = 1024                   # kTileRows: the evaluation's and the division's tile
CHUNK_BLOCKS = 1024            # kChunkBlocks
CARRY_PASS = 256               # kCarryPass
CANARY = 0xA5
# more fold tiles than workgroups, a third fold launch, chunks of two tiles in the evaluation and the
# division, and more chunks than one pass of the carry scan takes
BIG_N = T * T + T + 5


def _launches():
    return api.load().bzamd_kernel_launch_count()


def _device():
    import torch
    return torch.device("cuda", 0)


def _up(array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array).copy()).to(_device())


def _canaries(rows):
    import torch
    return torch.full((rows, 32), CANARY, dtype=torch.uint8, device=_device())


def ceil_log2(n):
    return max((n - 1).bit_length(), 1)


def fold_launches(num_variables):
    return (num_variables + FOLD_LEVELS - 1) // FOLD_LEVELS


class OnDevice:
    """the operands of one case in device memory, every output with a canary row behind it, and a
    side stream for the calls"""

    def __init__(self, case, num_points=None, polynomial=None):
        import torch
        self.case, self.f = case, case.field_id
        self.v, self.n = case.num_variables, case.n
        self.t = len(case.points) if num_points is None else num_points
        self.polynomial = case.polynomial_bytes() if polynomial is None else polynomial
        self.rows = sum(length for _, length in api.folded_layout(self.n, self.v))
        self.d_polynomial = _up(self.polynomial)
        self.d_point = _up(case.point_bytes())
        self.d_points = _up(case.points_bytes()[:self.t])
        self.d_q = _up(case.q_bytes())
        self.d_folded = _canaries(self.rows + 1)
        self.d_scalars = _canaries(self.rows + 1)
        self.d_evaluation = _canaries(2)
        self.d_evaluations = _canaries(self.t * self.v + 1)
        self.d_quotients = _canaries(self.t * self.n + 1)
        self.d_remainders = _canaries(self.t + 1)
        self.stream = torch.cuda.Stream(device=_device())
        torch.cuda.synchronize()

    def fold(self, lib_api):
        before = _launches()
        lib_api.fold_polynomial_device(self.f, self.d_folded.data_ptr(), self.d_scalars.data_ptr(),
                                       self.d_evaluation.data_ptr(), self.d_polynomial.data_ptr(),
                                       self.n, self.d_point.data_ptr(), self.v,
                                       stream=self.stream.cuda_stream)
        return _launches() - before

    def upload_folded(self):
        self.d_folded[:self.rows] = _up(self.case.folded_bytes())

    def evaluate(self, lib_api, d_workspace, workspace_bytes=None):
        before = _launches()
        lib_api.evaluate_polynomials_device(
            self.f, self.d_evaluations.data_ptr(), self.d_polynomial.data_ptr(),
            self.d_folded.data_ptr(), self.n, self.v, self.d_points.data_ptr(), self.t,
            d_workspace.data_ptr(),
            d_workspace.numel() if workspace_bytes is None else workspace_bytes,
            stream=self.stream.cuda_stream)
        return _launches() - before

    def quotients(self, lib_api, d_workspace):
        before = _launches()
        lib_api.batch_quotients_device(
            self.f, self.d_quotients.data_ptr(), self.d_remainders.data_ptr(),
            self.d_polynomial.data_ptr(), self.d_folded.data_ptr(), self.n, self.v,
            self.d_q.data_ptr(), self.d_points.data_ptr(), self.t, d_workspace.data_ptr(),
            d_workspace.numel(), stream=self.stream.cuda_stream)
        return _launches() - before

    def workspace(self, which, fill=0xFF, misalign=0):
        import torch
        size = (api.evaluate_polynomials_workspace_bytes if which == "evaluate"
                else api.batch_quotients_workspace_bytes)(self.f, self.n, self.v, self.t)
        assert size > 0
        return torch.full((size + misalign,), fill, dtype=torch.uint8,
                          device=_device())[misalign:]

    def finish(self):
        """synchronise; the inputs are what they were and nothing was written behind an output"""
        self.stream.synchronize()
        assert np.array_equal(self.d_polynomial.cpu().numpy(), self.polynomial)
        assert np.array_equal(self.d_point.cpu().numpy(), self.case.point_bytes())
        assert np.array_equal(self.d_points.cpu().numpy(), self.case.points_bytes()[:self.t])
        assert np.array_equal(self.d_q.cpu().numpy(), self.case.q_bytes())
        for name, tensor, rows in (("folded", self.d_folded, self.rows),
                                   ("scalars", self.d_scalars, self.rows),
                                   ("evaluation", self.d_evaluation, 1),
                                   ("evaluations", self.d_evaluations, self.t * self.v),
                                   ("quotients", self.d_quotients, self.t * self.n),
                                   ("remainders", self.d_remainders, self.t)):
            assert bool((tensor[rows] == CANARY).all()), f"the row behind {name} was written"


class BigCase(uc.Opening):
    """BIG_N rows of 62 random bits each (made with numpy; the values are what the bytes mean),
    three points and one q; the model's levels once per field"""

    def __init__(self, field_id):
        p, v = MODULUS[field_id], ceil_log2(BIG_N)
        rng = np.random.default_rng(50 + field_id)
        raw = rng.integers(0, 1 << 62, BIG_N, dtype=np.uint64)
        self.raw_bytes = np.zeros((BIG_N, 32), np.uint8)
        self.raw_bytes[:, :8] = raw.view(np.uint8).reshape(BIG_N, 8)
        scale = pow(1 << 256, -1, p) if field_id == 1 else 1
        self.field_id, self.num_variables, self.n = field_id, v, BIG_N
        self.p0 = [int(x) * scale % p for x in raw]
        self.point = point_of(field_id, v, 4)
        self.point[0] = p - 2  # not 0 or 1
        self.levels, self.evaluation = uc.levels(field_id, self.p0, self.point)
        self.points = uc.points_of(field_id, 3, 0)
        self.q = uc.random_values(field_id, 1, 123)[0]

    def polynomial_bytes(self):
        return self.raw_bytes


@functools.lru_cache(maxsize=None)
def big_case(field_id):
    return BigCase(field_id)


#--------------------------------------------------------------------------------------------------
# fold
#--------------------------------------------------------------------------------------------------
FOLD_SIZES = [1, 2, 3, T - 1, T, T + 1, 2 * T + 1, 3 * T - 1]


def check_fold(lib_api, case):
    dev = OnDevice(case)
    assert dev.fold(lib_api) == fold_launches(case.num_variables)
    dev.finish()
    assert np.array_equal(dev.d_folded.cpu().numpy()[:dev.rows], case.folded_bytes())
    assert np.array_equal(dev.d_scalars.cpu().numpy()[:dev.rows], case.folded_bytes(scalar=True))
    assert np.array_equal(dev.d_evaluation.cpu().numpy()[0], to_bytes(case.field_id, case.evaluation))


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("n", FOLD_SIZES)
def test_fold_device_form(gpu_backend, field_id, n):
    check_fold(gpu_backend, uc.Opening(field_id, ceil_log2(n), n, 10 + n % 7))


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("n", FOLD_SIZES)
def test_fold_device_form_30_variables(gpu_backend, field_id, n):
    """levels that stay at one row through three launches"""
    check_fold(gpu_backend, uc.Opening(field_id, 30, n, 20 + n % 5))


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("v", [11, 20, 21])
def test_fold_more_variables_than_rows_need(gpu_backend, field_id, v):
    """the second and third launch start from a level of one or two rows"""
    check_fold(gpu_backend, uc.Opening(field_id, v, T + 1, 31))


def sample_rows(length, tile, rng):
    """the first and last two tiles of a level and 1500 random rows"""
    if length <= 4 * tile:
        return list(range(length))
    return sorted(set(range(2 * tile)) | set(range(length - 2 * tile, length))
                  | {int(i) for i in rng.integers(0, length, 1500)})


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_fold_more_tiles_than_workgroups(gpu_backend, field_id):
    """T^2 + T + 5 rows: 1026 tiles on 1024 workgroups and three launches.  Levels below the tenth:
    the first and last two tiles and 1500 random rows; from the tenth on: whole"""
    case = big_case(field_id)
    assert (case.n + T - 1) // T > FOLD_BLOCKS and fold_launches(case.num_variables) == 3
    dev = OnDevice(case, num_points=1)
    assert dev.fold(gpu_backend) == 3
    dev.finish()
    folded = dev.d_folded.cpu().numpy()
    scalars = dev.d_scalars.cpu().numpy()
    rng = np.random.default_rng(8)
    for level, (offset, length) in enumerate(api.folded_layout(case.n, case.num_variables), 1):
        rows = list(range(length)) if level >= FOLD_LEVELS else sample_rows(length, T >> level, rng)
        values = [case.levels[level][j] for j in rows]
        at = [offset + j for j in rows]
        assert np.array_equal(folded[at], uc.element_rows(field_id, values)), f"level {level}"
        assert np.array_equal(scalars[at], uc.scalar_rows(field_id, values)), f"level {level}"
    assert np.array_equal(dev.d_evaluation.cpu().numpy()[0], to_bytes(field_id, case.evaluation))


@pytest.mark.gpu
def test_fold_launch_count_does_not_depend_on_n(gpu_backend):
    import torch
    counts = []
    for n, v in ((T + 1, 11), (1 << 20, 20)):
        d_polynomial = torch.zeros((n, 32), dtype=torch.uint8, device=_device())
        d_point = torch.zeros((v, 32), dtype=torch.uint8, device=_device())
        d_folded = torch.zeros((n + v, 32), dtype=torch.uint8, device=_device())
        before = _launches()
        gpu_backend.fold_polynomial_device(1, d_folded.data_ptr(), None, None,
                                           d_polynomial.data_ptr(), n, d_point.data_ptr(), v)
        counts.append(_launches() - before)
        torch.cuda.synchronize()
    assert counts == [fold_launches(11), fold_launches(20)] == [2, 2]


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("v,n", [(1, 1), (6, 37), (12, 2 * T + 3), (13, 2 * T + 3)])
def test_fold_evaluation_is_the_column_evaluation(gpu_backend, field_id, v, n):
    """`evaluation` against bzamd_mle_evaluation_vector_device and bzamd_evaluate_columns_device
    on the same stream, with no synchronise in between"""
    import torch
    case = uc.Opening(field_id, v, n, 41)
    dev = OnDevice(case)
    d_vector = _canaries(n + 1)
    d_expected = _canaries(2)
    size = api.evaluate_columns_workspace_bytes(field_id, 1, n)
    d_workspace = torch.zeros(size, dtype=torch.uint8, device=_device())
    torch.cuda.synchronize()
    stream = dev.stream.cuda_stream
    dev.fold(gpu_backend)
    gpu_backend.mle_evaluation_vector_device(field_id, d_vector.data_ptr(), dev.d_point.data_ptr(),
                                             v, n, stream=stream)
    gpu_backend.evaluate_columns_device(field_id, [(dev.d_polynomial.data_ptr(), n, 32, False)],
                                        d_vector.data_ptr(), n, d_expected.data_ptr(),
                                        d_workspace.data_ptr(), size, stream=stream)
    dev.finish()
    got = dev.d_evaluation.cpu().numpy()[0]
    assert np.array_equal(got, d_expected.cpu().numpy()[0])
    assert np.array_equal(got, to_bytes(field_id, case.evaluation))


#--------------------------------------------------------------------------------------------------
# evaluate
#--------------------------------------------------------------------------------------------------
EVALUATE_SIZES = [1, 2, LANE_ROWS - 1, LANE_ROWS, LANE_ROWS + 1, W - 1, W, W + 1, 2 * W + 1,
                  (1 << 14) + 77]


def expected_evaluations(case, num_points):
    want = case.evaluations()[:num_points]
    return uc.element_rows(case.field_id, [e for row in want for e in row])


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("n", EVALUATE_SIZES)
def test_evaluate_device_form(gpu_backend, field_id, n):
    """every P_i(u_k); a workspace of 0xFF at an odd address, used again by a second call with other
    points"""
    v = ceil_log2(n) + (n % 3 == 0)
    num_points = (4, 3, 1)[n % 3]
    case = uc.Opening(field_id, v, n, n % 4, num_points=4)
    dev = OnDevice(case, num_points)
    dev.upload_folded()
    d_workspace = dev.workspace("evaluate", misalign=3)
    assert dev.evaluate(gpu_backend, d_workspace) == 2
    dev.finish()
    got = dev.d_evaluations.cpu().numpy()[:num_points * v]
    assert np.array_equal(got, expected_evaluations(case, num_points))
    # the same workspace, other points
    case.points = uc.points_of(field_id, 4, n % 4 + 1)
    dev.d_points.copy_(_up(case.points_bytes()[:num_points]))
    dev.evaluate(gpu_backend, d_workspace)
    dev.finish()
    got = dev.d_evaluations.cpu().numpy()[:num_points * v]
    assert np.array_equal(got, expected_evaluations(case, num_points))


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_evaluate_30_variables(gpu_backend, field_id):
    """one-row levels: 30 x 4 values, most of them a single row"""
    case = uc.Opening(field_id, 30, 5, 2, num_points=4)
    dev = OnDevice(case)
    dev.upload_folded()
    assert dev.evaluate(gpu_backend, dev.workspace("evaluate")) == 2
    dev.finish()
    assert np.array_equal(dev.d_evaluations.cpu().numpy()[:120], expected_evaluations(case, 4))


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_evaluate_more_tiles_than_workgroups(gpu_backend, field_id):
    """T^2 + T + 5 rows: chunks of two tiles.  The levels are the fold's, on the same stream with no
    synchronise in between; P_0 and P_1 at two points against the model"""
    case = big_case(field_id)
    assert (case.n + W - 1) // W > CHUNK_BLOCKS
    dev = OnDevice(case, num_points=2)
    d_workspace = dev.workspace("evaluate")
    dev.fold(gpu_backend)
    assert dev.evaluate(gpu_backend, d_workspace) == 2
    dev.finish()
    got = dev.d_evaluations.cpu().numpy()
    v = case.num_variables
    for k in range(2):
        want = [uc.evaluate(field_id, case.levels[i], case.points[k]) for i in (0, 1)]
        assert np.array_equal(got[k * v:k * v + 2], uc.element_rows(field_id, want)), f"point {k}"


#--------------------------------------------------------------------------------------------------
# batch and divide
#--------------------------------------------------------------------------------------------------
DIVIDE_SIZES = [1, 2, Q - 1, Q, Q + 1, 2 * Q + 1, (1 << 14) + 77]


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("num_points", [1, 3])
@pytest.mark.parametrize("n", DIVIDE_SIZES)
def test_quotients_device_form(gpu_backend, field_id, num_points, n):
    """every row of every quotient; the remainders against sum_i q^i evaluations[k l + i] of the
    evaluation on the same stream"""
    p = MODULUS[field_id]
    v = ceil_log2(n) + (n % 3 == 0)
    q = {0: None, 1: 0, 2: 1}[(n + num_points) % 3] if n < Q else None
    case = uc.Opening(field_id, v, n, (n + num_points) % 4, num_points=3, q=q)
    dev = OnDevice(case, num_points)
    dev.upload_folded()
    d_evaluate_workspace = dev.workspace("evaluate")
    d_workspace = dev.workspace("quotients", misalign=5)
    dev.evaluate(gpu_backend, d_evaluate_workspace)
    assert dev.quotients(gpu_backend, d_workspace) == 3
    dev.finish()
    hs, rs = case.quotients()
    got = dev.d_quotients.cpu().numpy()
    for k in range(num_points):
        assert np.array_equal(got[k * n:(k + 1) * n], uc.scalar_rows(field_id, hs[k])), f"point {k}"
        assert not got[k * n + n - 1].any()
    remainders = dev.d_remainders.cpu().numpy()[:num_points]
    assert np.array_equal(remainders, uc.element_rows(field_id, rs[:num_points]))
    evaluations = uc.element_values(field_id, dev.d_evaluations.cpu().numpy()[:num_points * v])
    for k in range(num_points):
        combined = sum(pow(case.q, i, p) * e for i, e in enumerate(evaluations[k * v:(k + 1) * v]))
        assert combined % p == rs[k]


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_quotients_more_chunks_than_one_pass(gpu_backend, field_id):
    """T^2 + T + 5 rows: 514 chunks of two tiles, three passes of the carry scan.  The top and the
    bottom Q rows and 1500 random rows, one point"""
    case = big_case(field_id)
    n = case.n
    chunk_rows = Q * (((n + Q - 1) // Q + CHUNK_BLOCKS - 1) // CHUNK_BLOCKS)
    assert chunk_rows == 2 * Q and (n + chunk_rows - 1) // chunk_rows > 2 * CARRY_PASS
    dev = OnDevice(case, num_points=1)
    d_workspace = dev.workspace("quotients")
    dev.fold(gpu_backend)
    assert dev.quotients(gpu_backend, d_workspace) == 3
    dev.finish()
    h, remainder = uc.quotient(field_id, case.batched(), case.points[0])
    rng = np.random.default_rng(12)
    rows = sorted(set(range(Q)) | set(range(n - Q, n)) | {int(i) for i in rng.integers(0, n, 1500)})
    got = dev.d_quotients.cpu().numpy()
    assert np.array_equal(got[rows], uc.scalar_rows(field_id, [h[j] for j in rows]))
    assert np.array_equal(dev.d_remainders.cpu().numpy()[0], to_bytes(field_id, remainder))


@pytest.mark.gpu
def test_quotient_launch_count_does_not_depend_on_n(gpu_backend):
    import torch
    counts = []
    for n, v in ((5, 3), (1 << 20, 20)):
        d_polynomial = torch.zeros((n, 32), dtype=torch.uint8, device=_device())
        d_folded = torch.zeros((n + v, 32), dtype=torch.uint8, device=_device())
        d_small = torch.zeros((8, 32), dtype=torch.uint8, device=_device())
        d_quotients = torch.zeros((3 * n, 32), dtype=torch.uint8, device=_device())
        size = api.batch_quotients_workspace_bytes(1, n, v, 3)
        d_workspace = torch.zeros(size, dtype=torch.uint8, device=_device())
        before = _launches()
        gpu_backend.batch_quotients_device(1, d_quotients.data_ptr(), None, d_polynomial.data_ptr(),
                                           d_folded.data_ptr(), n, v, d_small.data_ptr(),
                                           d_small[1:].data_ptr(), 3, d_workspace.data_ptr(), size)
        counts.append(_launches() - before)
        torch.cuda.synchronize()
    assert counts == [3, 3]


#--------------------------------------------------------------------------------------------------
# host forms on the GPU backend
#--------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("v,n", [(1, 1), (6, 37), (12, 2 * T + 1)])
def test_host_forms_on_gpu(gpu_backend, field_id, v, n):
    """the bytes of the model, which are the host backend's (tests/test_univariate_opening.py), and
    kernels ran"""
    from tests.test_univariate_opening import run_host_forms
    case = uc.Opening(field_id, v, n, 3, num_points=4)
    before = _launches()
    run_host_forms(gpu_backend, case, 3)
    assert _launches() - before == fold_launches(v) + 2 + 3, "the kernels did not run"
    only, none_scalars, none_evaluation = gpu_backend.fold_polynomial(
        field_id, case.polynomial_bytes(), case.point_bytes(), scalars=None, evaluation=None)
    assert np.array_equal(only, case.folded_bytes()) and none_scalars is None
    quotients, none_remainders = gpu_backend.batch_quotients(
        field_id, case.polynomial_bytes(), only, case.q_bytes(), case.points_bytes()[:1], v,
        remainders=None)
    hs, _ = case.quotients()
    assert none_remainders is None and np.array_equal(quotients[0], uc.scalar_rows(field_id, hs[0]))


#--------------------------------------------------------------------------------------------------
# the whole chain on one stream
#--------------------------------------------------------------------------------------------------
def challenge(*arrays):
    """a stand-in for the caller's transcript: a field element out of the bytes so far"""
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return int.from_bytes(h.digest() + h.digest(), "little") % MODULUS[1]


def msm(lib_api, d_out, descriptors, d_generators, stream):
    import ctypes
    desc = (api.sxt_sequence_descriptor * len(descriptors))()
    for i, (ptr, rows) in enumerate(descriptors):
        desc[i] = api.sxt_sequence_descriptor(32, rows, ptr, 0)
    lib_api.load().bzamd_msm_device(api.SXT_CURVE_BN_254, ctypes.c_void_p(d_out.data_ptr()),
                                    len(descriptors), desc,
                                    ctypes.c_void_p(d_generators.data_ptr()),
                                    ctypes.c_void_p(stream))
    return desc


@pytest.mark.gpu
@pytest.mark.parametrize("n", [37, 2 * T + 1])
def test_whole_chain_on_one_stream(gpu_backend, n):
    """fold -> MSM over the levels -> r -> evaluate -> q -> batch quotients -> MSM over the
    quotients, field 1 with BN254 commitments over G_i = tau^i G; the downloads behind r and q are
    the only synchronisations before the results are read"""
    import torch
    f, v, p = 1, ceil_log2(n), MODULUS[1]
    case = uc.Opening(f, v, n, 6)
    dev = OnDevice(case, num_points=3)
    stream = dev.stream.cuda_stream
    d_generators = _up(uc.affine_bytes(uc.tau_generators(n, uc.SMALL_TAU)))
    d_p0_scalars = _up(uc.scalar_rows(f, case.p0))
    d_level_commitments = torch.zeros((v, 72), dtype=torch.uint8, device=_device())
    d_quotient_commitments = torch.zeros((3, 72), dtype=torch.uint8, device=_device())
    d_evaluate_workspace = dev.workspace("evaluate")
    d_workspace = dev.workspace("quotients")
    layout = api.folded_layout(n, v)
    torch.cuda.synchronize()
    with torch.cuda.stream(dev.stream):
        # 1, 2: the levels and their commitments
        dev.fold(gpu_backend)
        columns = [(d_p0_scalars.data_ptr(), n)] + [
            (dev.d_scalars.data_ptr() + 32 * offset, length) for offset, length in layout]
        keep = msm(gpu_backend, d_level_commitments, columns, d_generators, stream)
        # 3: transcript -> r (the first round trip)
        level_commitments = d_level_commitments.cpu().numpy()
        r = challenge(level_commitments)
        case.points = [r, (p - r) % p, r * r % p]
        dev.d_points.copy_(torch.from_numpy(case.points_bytes()))
        # 4: the evaluations
        dev.evaluate(gpu_backend, d_evaluate_workspace)
        # 5: transcript -> q (the second round trip)
        evaluations = dev.d_evaluations.cpu().numpy()[:3 * v]
        case.q = challenge(level_commitments, evaluations)
        dev.d_q.copy_(torch.from_numpy(case.q_bytes()))
        # 6, 7: the quotients and their commitments
        dev.quotients(gpu_backend, d_workspace)
        keep2 = msm(gpu_backend, d_quotient_commitments,
                    [(dev.d_quotients.data_ptr() + 32 * n * k, n) for k in range(3)], d_generators,
                    stream)
    dev.finish()
    del keep, keep2
    # the outputs against the model
    assert np.array_equal(dev.d_scalars.cpu().numpy()[:dev.rows], case.folded_bytes(scalar=True))
    assert np.array_equal(evaluations, expected_evaluations(case, 3))
    hs, rs = case.quotients()
    quotients = dev.d_quotients.cpu().numpy()
    for k in range(3):
        assert np.array_equal(quotients[k * n:(k + 1) * n], uc.scalar_rows(f, hs[k]))
    remainders = dev.d_remainders.cpu().numpy()[:3]
    assert np.array_equal(remainders, uc.element_rows(f, rs))
    # the equation, on the device's commitments
    quotient_commitments = d_quotient_commitments.cpu().numpy()
    assert uc.opening_equation_holds(
        v, case.q, case.points, [uc.affine_point(c) for c in level_commitments],
        [uc.affine_point(c) for c in quotient_commitments], rs, tau=uc.SMALL_TAU)
    # and the commitments are those of the model's scalars through the same MSM
    d_model = _up(np.concatenate([uc.scalar_rows(f, case.p0), case.folded_bytes(scalar=True)]
                                 + [uc.scalar_rows(f, h) for h in hs]))
    d_again = torch.zeros((v + 3, 72), dtype=torch.uint8, device=_device())
    at = d_model.data_ptr()
    columns = ([(at, n)] + [(at + 32 * (n + offset), length) for offset, length in layout]
               + [(at + 32 * (n + dev.rows + n * k), n) for k in range(3)])
    keep = msm(gpu_backend, d_again, columns, d_generators, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    again = d_again.cpu().numpy()
    assert np.array_equal(again[:v], level_commitments)
    assert np.array_equal(again[v:], quotient_commitments)
