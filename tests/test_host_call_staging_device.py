"""What the staging of the blocking proof calls on host operands decides by itself on the GPU
backend (proof/host_call.h): which operand is uploaded, which result comes back, what a null
pointer and a column of no rows mean.  The cases here are the ones the host-form tests beside the
device forms do not reach; each compares with the device form of the same call or with the
Python model, as those tests do.  The shapes are tiny: the kernels are not what is under test."""
import ctypes

import numpy as np
import pytest

from blitzar_amd import api
from tests import column_inverse_cases as cic
from tests import multiplicity_cases as mc
from tests import univariate_cases as uc
from tests.test_column_inverse_device import Case as InverseCase
from tests.test_column_inverse_device import invert_on_device
from tests.test_mle_opening import Columns
from tests.test_multiplicities_device import HASHED, RANGE, count_on_device, i64_column
from tests.test_sumcheck_device import to_bytes

ROWS = 37


def _launches():
    return api.load().bzamd_kernel_launch_count()


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_invert_columns_scalars_alone(gpu_backend, field_id):
    """`inverses` a null pointer: straight through the library, the wrapper always brings inverses"""
    case = InverseCase(field_id, ROWS, 4, 7800 + field_id)
    _, scalars = invert_on_device(gpu_backend, case, "scalars")
    descs, keep = api.make_descriptors([(data.copy(), signed) for data, signed in case.arrays])
    coefficients = np.ascontiguousarray(case.coefficient_bytes(), dtype=np.uint8)
    shift = np.ascontiguousarray(case.shift_bytes(), dtype=np.uint8)
    v = api.bzamd_column_inversion(descs, coefficients.ctypes.data, shift.ctypes.data, len(keep),
                                   case.n)
    alone = np.zeros((case.n, 32), np.uint8)
    before = _launches()
    api.load().bzamd_invert_columns(None, alone.ctypes.data_as(ctypes.c_void_p), field_id,
                                    ctypes.byref(v))
    assert _launches() - before == 1, "no kernel ran"
    assert np.array_equal(alone, scalars) and np.array_equal(alone, case.want[1])


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_invert_columns_without_coefficients_and_shift(gpu_backend, field_id):
    """neither coefficients nor a shift, and a column of no rows beside one of n"""
    import torch
    column = np.arange(1, ROWS + 1, dtype=np.int64).view(np.uint8).reshape(ROWS, 8)
    dev = torch.device("cuda", 0)
    d_column = torch.from_numpy(column.copy()).to(dev)
    d_inverses = torch.zeros((ROWS, 32), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    gpu_backend.invert_columns_device(field_id, d_inverses.data_ptr(), None,
                                      [(d_column.data_ptr(), ROWS, 8, True), (None, 0, 2, False)],
                                      None, None, ROWS)
    torch.cuda.synchronize()
    got = gpu_backend.invert_columns(field_id, [(column, True), (np.zeros((0, 2), np.uint8), False)],
                                     ROWS)
    assert np.array_equal(got, d_inverses.cpu().numpy())
    want = cic.inverses(field_id, [i + 1 for i in range(ROWS)])
    assert np.array_equal(got, cic.expected_bytes(field_id, want)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("hashed", [True, False])
def test_count_multiplicities_without_misses(gpu_backend, field_id, hashed):
    """`misses` a null pointer: a hashed table with no lookup at all, and the range table, which
    has neither rows to upload nor a workspace"""
    if hashed:
        table = i64_column([5, -7, 11, 2**40, -2**50])
        lookups = (np.zeros((0, 8), np.uint8), True)
    else:
        table = None
        rng = np.random.default_rng(field_id)
        lookups = (rng.integers(0, 1100, ROWS).astype(np.uint16).view(np.uint8).reshape(ROWS, 2),
                   False)
    case = mc.Case(field_id, table, lookups, table_rows=1000)
    got, _ = count_on_device(gpu_backend, case, want_misses=False)
    before = _launches()
    host = gpu_backend.count_multiplicities(
        field_id, (table[0].copy(), True) if hashed else (None, 1000),
        (lookups[0].copy(), lookups[1]), want_misses=False)
    assert _launches() - before == (HASHED if hashed else RANGE), "no kernel ran"
    assert np.array_equal(host, got) and np.array_equal(host, case.want_multiplicities())


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_combine_columns_without_product(gpu_backend, field_id):
    """evaluations and no product (a null pointer): no product launch either"""
    case = Columns(field_id, ROWS, 7, 117, 1)
    before = _launches()
    combined, _ = gpu_backend.combine_columns(field_id, case.host_columns(),
                                              case.coefficient_bytes(), ROWS,
                                              case.evaluation_bytes(), None)
    assert _launches() - before == 1
    assert np.array_equal(combined, case.expected_combined())


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_fold_evaluation_alone_and_four_points(gpu_backend, field_id):
    """the fold with its evaluation and no scalars; the quotients at the most points there are,
    with their remainders"""
    v = 6
    case = uc.Opening(field_id, v, ROWS, 3, num_points=4)
    folded, none_scalars, evaluation = gpu_backend.fold_polynomial(
        field_id, case.polynomial_bytes(), case.point_bytes(), scalars=None)
    assert none_scalars is None and np.array_equal(folded, case.folded_bytes())
    assert np.array_equal(evaluation, to_bytes(field_id, case.evaluation))
    before = _launches()
    quotients, remainders = gpu_backend.batch_quotients(
        field_id, case.polynomial_bytes(), folded, case.q_bytes(), case.points_bytes(), v)
    assert _launches() - before == 3, "no kernel ran"
    hs, rs = case.quotients()
    assert len(hs) == 4
    for k in range(4):
        assert np.array_equal(quotients[k], uc.scalar_rows(field_id, hs[k])), f"point {k}"
    assert np.array_equal(remainders, uc.element_rows(field_id, rs))
