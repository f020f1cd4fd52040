"""The device form of the inverse column (include/blitzar_amd.h: bzamd_invert_columns_device), the
host form on the GPU backend, and the log-derivative identity proved from device-resident data on
one stream: inverse column, its commitment, the sumcheck over it, verification.

Expected bytes are Python integers (tests/column_inverse_cases.py).  The sizes follow the kernel's
constants (proof/column_inverse.hip): 256 lanes of 8 rows, tiles of 2048 rows, at most 512
workgroups; lane t of a tile holds the tile's rows t + 256 r, r < 8."""
import numpy as np
import pytest

from blitzar_amd import api
from tests import column_inverse_cases as cic
from tests import merlin_ref
from tests.test_mle_opening import as_bytes
from tests.test_sumcheck import product_table
from tests.test_sumcheck_device import MODULUS, to_bytes, to_int
from tests.test_sumcheck_transcript import variables

THREADS = 256              # kInverseThreads
LANE_ROWS = 8              # kLaneRows
TILE = THREADS * LANE_ROWS  # kInverseTile
GRID_CAP = 512             # kInverseBlocks
LAUNCHES = 1               # of one call, whatever n and the data are
CANARY = 0xA5
SIZES = [1, LANE_ROWS - 1, LANE_ROWS, LANE_ROWS + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]
NARROW = [(1, False), (2, True), (8, True), (16, True), (31, False)]


def _launches():
    return api.load().bzamd_kernel_launch_count()


def _device():
    import torch
    return torch.device("cuda", 0)


def _up(array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array).copy()).to(_device())


def _random(rng, p):
    return int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % p


def zero_rows(n):
    """where the kernel can go wrong: the first and the last row, every row of lane 5 of tile 0, the
    last row of tile 0 and the first of tile 1, and all of tile 1"""
    rows = {0, n - 1, TILE - 1, TILE} | {5 + THREADS * r for r in range(LANE_ROWS)}
    if n > 2 * TILE:
        rows |= set(range(TILE, 2 * TILE))
    return sorted(i for i in rows if 0 <= i < n)


class Case:
    """num_columns typed columns over n rows in one flat buffer, column j one, three or no bytes
    past a multiple of 8, and the denominators that are zero at zero_rows(n).
    num_columns 1: one i64 column, no coefficients, a shift; the column is -shift at the zero rows.
    More: narrow columns of every width, some signed, of n, n - 1, 3 * 256 + 100 (it ends in the
    middle of the lanes' fourth rows), 1 and 0 rows, then one column of n 32-byte elements, which
    cancels the others at the zero rows; random coefficients and a shift."""

    def __init__(self, field_id, n, num_columns, seed):
        p = MODULUS[field_id]
        rng = np.random.default_rng(seed)
        self.field_id, self.n = field_id, n
        self.zeros = zero_rows(n)
        self.shift = _random(rng, p)
        arrays, self.values = [], []
        if num_columns == 1:
            self.coefficients = None
            self.shift = int(rng.integers(1, 2**62))
            column = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
            column[self.zeros] = -self.shift
            arrays.append((column.view(np.uint8).reshape(n, 8), True))
            self.values.append(cic.integer_values(field_id, column, True))
        else:
            self.coefficients = [_random(rng, p) for _ in range(num_columns)]
            self.coefficients[-1] = self.coefficients[-1] or 1
            lengths = [n, n - 1, min(n, 3 * THREADS + 100), min(n, 1), 0]
            for j in range(num_columns - 1):
                width, signed = NARROW[j % len(NARROW)]
                rows = lengths[(j + j // len(NARROW)) % len(lengths)]
                data = rng.integers(0, 256, (rows, width), dtype=np.uint8)
                if signed and rows > 1:
                    low = -(1 << (8 * width - 1))
                    data[0] = np.frombuffer(low.to_bytes(width, "little", signed=True), np.uint8)
                    data[1] = 0xFF
                arrays.append((data, signed))
                self.values.append(cic.integer_values(field_id, data, signed))
            rest = cic.denominators(field_id, self.values, self.coefficients[:-1], self.shift, n)
            last = [_random(rng, p) for _ in range(n)]
            negated_inverse = p - pow(self.coefficients[-1], -1, p)
            for i in self.zeros:
                last[i] = rest[i] * negated_inverse % p
            arrays.append((as_bytes(field_id, last), False))
            self.values.append(last)
        self.arrays = arrays
        self.specs, at = [], 64
        for j, (data, signed) in enumerate(arrays):
            at = (at + 7) // 8 * 8 + (1, 0, 3)[j % 3]
            self.specs.append((at, data.shape[0], data.shape[1], signed))
            at += data.size + 8
        self.flat = np.full(at + 64, CANARY, np.uint8)
        for (data, _), (offset, _, _, _) in zip(arrays, self.specs):
            self.flat[offset:offset + data.size] = data.reshape(-1)
        ds = cic.denominators(field_id, self.values, self.coefficients, self.shift, n)
        assert [i for i, d in enumerate(ds) if d == 0] == self.zeros
        self.want = cic.expected_bytes(field_id, cic.inverses(field_id, ds))

    def coefficient_bytes(self):
        return None if self.coefficients is None else as_bytes(self.field_id, self.coefficients)

    def shift_bytes(self):
        return to_bytes(self.field_id, self.shift)


def invert_on_device(lib_api, case, outputs):
    """-> (inverses or None, scalars or None); checks the launch count, the canary row behind each
    output and that every input is byte for byte what it was"""
    import torch
    n, field_id = case.n, case.field_id
    d_flat = _up(case.flat)
    d_coefficients = None if case.coefficients is None else _up(case.coefficient_bytes())
    d_shift = _up(case.shift_bytes())
    out = {name: torch.full((n + 1, 32), CANARY, dtype=torch.uint8, device=_device())
           for name in ("inverses", "scalars") if outputs in (name, "both")}
    side = torch.cuda.Stream(device=_device())
    torch.cuda.synchronize()
    before = _launches()
    lib_api.invert_columns_device(
        field_id, out["inverses"].data_ptr() if "inverses" in out else None,
        out["scalars"].data_ptr() if "scalars" in out else None,
        [(d_flat.data_ptr() + o, rows, w, signed) for o, rows, w, signed in case.specs],
        None if d_coefficients is None else d_coefficients.data_ptr(), d_shift.data_ptr(), n,
        stream=side.cuda_stream)
    assert _launches() - before == LAUNCHES
    side.synchronize()
    got = {name: rows.cpu().numpy() for name, rows in out.items()}
    for name, rows in got.items():
        assert np.all(rows[n] == CANARY), f"the row behind `{name}` was written"
    assert np.array_equal(d_flat.cpu().numpy(), case.flat), "the columns were modified"
    if d_coefficients is not None:
        assert np.array_equal(d_coefficients.cpu().numpy(), case.coefficient_bytes())
    assert np.array_equal(d_shift.cpu().numpy(), case.shift_bytes())
    return tuple(got[name][:n] if name in got else None for name in ("inverses", "scalars"))


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("num_columns", [1, 4, 32])
@pytest.mark.parametrize("n", SIZES)
def test_device_form(gpu_backend, field_id, num_columns, n):
    case = Case(field_id, n, num_columns, 7000 + 40 * n + num_columns)
    for outputs in ("both", "inverses", "scalars"):
        inverses, scalars = invert_on_device(gpu_backend, case, outputs)
        if inverses is not None:
            assert np.array_equal(inverses, case.want[0]), outputs
        if scalars is not None:
            assert np.array_equal(scalars, case.want[1]), outputs
    for rows in (inverses, scalars):
        assert rows is None or not rows[case.zeros].any()


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_every_denominator_zero(gpu_backend, field_id):
    """no shift over a zero column: a tile whose every leaf of the product tree is a stand-in"""
    import torch
    n = TILE + 3
    out = torch.full((2, n + 1, 32), CANARY, dtype=torch.uint8, device=_device())
    torch.cuda.synchronize()
    gpu_backend.invert_columns_device(field_id, out[0].data_ptr(), out[1].data_ptr(),
                                      [(0, 0, 8, True)], None, None, n)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not got[:, :n].any() and np.all(got[:, n] == CANARY)


@pytest.mark.gpu
def test_more_tiles_than_workgroups(gpu_backend):
    """513 tiles and five rows on 512 workgroups: workgroup 0 walks a second tile and workgroup 1 a
    tile of five rows.  Field 1, one i64 column with a shift, every row against Python's own batch
    inversion (three multiplications a row and one pow), a slice of which is checked with pow
    beforehand; the same single launch as at n = 1"""
    import torch
    field_id, n = 1, GRID_CAP * TILE + TILE + 5
    p = MODULUS[field_id]
    rng = np.random.default_rng(31)
    shift = int(rng.integers(1, 2**62))
    column = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
    zeros = [0, TILE, GRID_CAP * TILE - 1, GRID_CAP * TILE, n - 1]
    column[zeros] = -shift
    ds = [(x + shift) % p for x in column.tolist()]
    want = cic.batch_inverses(field_id, ds)
    sample = list(range(300)) + list(range(n - 300, n)) + [int(i) for i in rng.integers(0, n, 400)]
    assert [want[i] for i in sample] == cic.inverses(field_id, [ds[i] for i in sample])
    assert [i for i in sample if want[i] == 0] == [0, n - 1]
    d_column, d_shift = _up(column.view(np.uint8)), _up(to_bytes(field_id, shift))
    d_inverses = torch.full((n + 1, 32), CANARY, dtype=torch.uint8, device=_device())
    side = torch.cuda.Stream(device=_device())
    torch.cuda.synchronize()
    before = _launches()
    gpu_backend.invert_columns_device(field_id, d_inverses.data_ptr(), None,
                                      [(d_column.data_ptr(), n, 8, True)], None,
                                      d_shift.data_ptr(), n, stream=side.cuda_stream)
    assert _launches() - before == LAUNCHES
    side.synchronize()
    got = d_inverses.cpu().numpy()
    assert np.all(got[n] == CANARY)
    assert np.array_equal(got[:n], cic.expected_bytes(field_id, want)[0])
    assert not got[zeros].any()


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_host_form_on_gpu_equals_the_device_form(gpu_backend, field_id):
    case = Case(field_id, TILE + 300, 4, 7700 + field_id)
    inverses, scalars = invert_on_device(gpu_backend, case, "both")
    columns = [(data.copy(), signed) for data, signed in case.arrays]
    before = _launches()
    got, got_scalars = gpu_backend.invert_columns(field_id, columns, case.n,
                                                  coefficients=case.coefficient_bytes(),
                                                  shift=case.shift_bytes(), want_scalars=True)
    assert _launches() - before == LAUNCHES, "no kernel ran"
    assert np.array_equal(got, inverses) and np.array_equal(got_scalars, scalars)
    assert np.array_equal(got, case.want[0]) and np.array_equal(got_scalars, case.want[1])
    only = gpu_backend.invert_columns(field_id, columns, case.n,
                                      coefficients=case.coefficient_bytes(),
                                      shift=case.shift_bytes())
    assert np.array_equal(only, inverses)
    for (kept, _), (data, _) in zip(columns, case.arrays):
        assert np.array_equal(kept, data), "a column was modified"


@pytest.mark.gpu
def test_log_derivative_identity_on_one_stream(gpu_backend):
    """sum_i (c[i] + alpha) / (c[i] + alpha) = n, from a column in HBM to a verified sumcheck with
    no synchronise in between: the inverse column in both forms, its commitment from `scalars`, the
    sumcheck over {c, inverses} with the products 1 * c * inv + alpha * inv, then on the host the
    verifier's rounds against the claimed sum n and the final evaluations"""
    import torch
    field_id, n, dev = 0, 300, _device()
    p = MODULUS[field_id]
    rng = np.random.default_rng(41)
    alpha = _random(rng, p)
    column = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
    ds = cic.denominators(field_id, [cic.integer_values(field_id, column, True)], None, alpha, n)
    assert all(ds), "alpha makes a denominator zero"
    want_elements, want_scalars = cic.expected_bytes(field_id, cic.inverses(field_id, ds))

    d_column, d_alpha = _up(column.view(np.uint8)), _up(to_bytes(field_id, alpha))
    inverses = torch.full((n + 1, 32), CANARY, dtype=torch.uint8, device=dev)
    scalars = torch.full((n + 1, 32), CANARY, dtype=torch.uint8, device=dev)
    d_model = _up(want_scalars)
    d_generators = _up(api.get_generators(n).view(np.uint8))
    commitments = torch.zeros((2, 32), dtype=torch.uint8, device=dev)
    scalar_desc = (api.sxt_sequence_descriptor * 1)(
        api.sxt_sequence_descriptor(32, n, scalars.data_ptr(), 0))
    model_desc = (api.sxt_sequence_descriptor * 1)(
        api.sxt_sequence_descriptor(32, n, d_model.data_ptr(), 0))
    mles = [(d_column.data_ptr(), n, 8, True), (inverses.data_ptr(), n, 32, False)]
    terms = [0, 1, 1]
    table = product_table(field_id, [to_bytes(field_id, 1), to_bytes(field_id, alpha)], [2, 1],
                          api.SUMCHECK_PRODUCT_STRIDE[field_id])
    v = variables(n)
    polys = torch.zeros((v, 3, 32), dtype=torch.uint8, device=dev)
    point = torch.zeros((v, 32), dtype=torch.uint8, device=dev)
    evaluations = torch.zeros((2, 32), dtype=torch.uint8, device=dev)
    t0 = merlin_ref.Transcript(label="log-derivative").array()
    transcript = _up(t0)
    workspace_bytes = api.sumcheck_transcript_columns_workspace_bytes(field_id, n, 2, 2, 3, 2)
    workspace = torch.empty(workspace_bytes, dtype=torch.uint8, device=dev)

    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    before = _launches()
    gpu_backend.invert_columns_device(field_id, inverses.data_ptr(), scalars.data_ptr(),
                                      [(d_column.data_ptr(), n, 8, True)], None, d_alpha.data_ptr(),
                                      n, stream=side.cuda_stream)
    assert _launches() - before == LAUNCHES
    lib = api.load()
    lib.bzamd_msm_device(0, commitments[0].data_ptr(), 1, scalar_desc, d_generators.data_ptr(),
                         side.cuda_stream)
    lib.bzamd_msm_device(0, commitments[1].data_ptr(), 1, model_desc, d_generators.data_ptr(),
                         side.cuda_stream)
    gpu_backend.prove_sumcheck_transcript_device_columns(
        field_id, mles, table, terms, n, 2, polys.data_ptr(), point.data_ptr(),
        evaluations.data_ptr(), transcript.data_ptr(), workspace.data_ptr(), workspace_bytes,
        stream=side.cuda_stream)
    side.synchronize()

    got_inverses, got_scalars = inverses.cpu().numpy(), scalars.cpu().numpy()
    assert np.all(got_inverses[n] == CANARY) and np.all(got_scalars[n] == CANARY)
    assert np.array_equal(got_inverses[:n], want_elements)
    assert np.array_equal(got_scalars[:n], want_scalars)
    got_commitments = commitments.cpu().numpy()
    assert got_commitments[0].any()
    assert np.array_equal(got_commitments[0], got_commitments[1])
    host_polys = polys.cpu().numpy()
    ok, expected, v_point, _ = gpu_backend.verify_sumcheck(field_id, to_bytes(field_id, n),
                                                           host_polys, t0)
    assert ok, "the verifier rejected the rounds against the claimed sum n"
    assert np.array_equal(v_point, point.cpu().numpy())
    host_evaluations = evaluations.cpu().numpy()
    assert gpu_backend.check_sumcheck_evaluations(field_id, expected, host_evaluations, table, terms)
    assert not gpu_backend.verify_sumcheck(field_id, to_bytes(field_id, n - 1), host_polys, t0)[0]
    e = [to_int(field_id, x) for x in host_evaluations]
    assert to_int(field_id, expected) == (e[0] * e[1] + alpha * e[1]) % p
