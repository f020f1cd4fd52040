"""The device form of the multiplicity column (include/blitzar_amd.h:
bzamd_count_multiplicities_device), the host form on the GPU backend, and the lookup argument
proved from device-resident data on one stream: multiplicities, the two inverse columns, the
commitment to the multiplicities, the sumcheck over all three, verification.

Expected counts are Python integers (tests/multiplicity_cases.py).  The sizes follow the kernels'
constants (proof/multiplicities.hip): wavefronts of 64 lanes, workgroups of 256, at most 2048 of
them; tables of at most 4096 rows are counted in bins in LDS (at most 1024 workgroups), larger
ones with aggregated adds to global memory.  Every call is checked for its launch count, the
canaries behind `multiplicities`, around `misses` and behind the workspace, its untouched inputs,
and against the model."""
import numpy as np
import pytest

from blitzar_amd import api
from tests import column_inverse_cases as cic
from tests import merlin_ref
from tests import multiplicity_cases as mc
from tests.test_sumcheck import product_table
from tests.test_sumcheck_device import MODULUS, to_bytes
from tests.test_sumcheck_transcript import variables

W = 64            # lanes of a wavefront
B = 256           # kCountThreads
GRID_CAP = 2048   # kCountBlocks
LDS_BINS = 4096   # kLdsBins
HASHED, RANGE = 3, 2  # launches of one call, whatever m, n and the data are
CANARY = mc.CANARY
CANARY_WORD = int.from_bytes(bytes([CANARY]) * 8, "little")


def _launches():
    return api.load().bzamd_kernel_launch_count()


def _device():
    import torch
    return torch.device("cuda", 0)


def _up(array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array).copy()).to(_device())


def count_on_device(lib_api, case, want_misses=True):
    """-> (multiplicities, misses or None) of the device form on a stream of its own, the workspace
    one byte past an allocation; checks the launch count, the canaries and the inputs"""
    import torch
    m, dev = case.m, _device()
    d_flat = _up(case.flat)
    out = torch.full((m + 1 + 3,), CANARY, dtype=torch.uint8, device=dev).repeat_interleave(8)
    multiplicities, misses = out.data_ptr(), out.data_ptr() + 8 * (m + 2)
    hashed = case.table is not None
    workspace_bytes = lib_api.count_multiplicities_workspace_bytes(m) if hashed else 0
    workspace = torch.full((workspace_bytes + 1 + 64,), CANARY, dtype=torch.uint8, device=dev)
    table, lookups = case.descriptors(d_flat.data_ptr())
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    before = _launches()
    lib_api.count_multiplicities_device(
        case.field_id, multiplicities, misses if want_misses else None, table, lookups,
        workspace.data_ptr() + 1 if hashed else None, workspace_bytes, stream=side.cuda_stream)
    assert _launches() - before == (HASHED if hashed else RANGE)
    side.synchronize()
    words = out.cpu().numpy().view(np.uint64)
    assert words[m] == CANARY_WORD, "the word behind `multiplicities` was written"
    assert words[m + 1] == CANARY_WORD and words[m + 3] == CANARY_WORD, "a word beside `misses`"
    assert want_misses or words[m + 2] == CANARY_WORD
    tail = workspace.cpu().numpy()
    assert tail[0] == CANARY and np.all(tail[1 + workspace_bytes:] == CANARY), "past the workspace"
    assert np.array_equal(d_flat.cpu().numpy(), case.flat), "the columns were modified"
    return words[:m].copy(), int(words[m + 2]) if want_misses else None


def check(lib_api, case, want_misses=True):
    got, misses = count_on_device(lib_api, case, want_misses)
    assert np.array_equal(got, case.want_multiplicities())
    assert misses == (case.want[1] if want_misses else None)


def i64_column(values):
    return (np.array(values, np.int64).view(np.uint8).reshape(len(values), 8), True)


def distinct(rng, count_, low=-2**62, high=2**62):
    values = set()
    while len(values) < count_:
        values.add(int(rng.integers(low, high)))
    return sorted(values, key=lambda _: rng.random())


#--------------------------------------------------------------------------------------------------
# tiny tables: the probe wraps, the table is as full as it gets
#--------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("n", [0, 1, W - 1, W, W + 1, 3 * B + 5])
@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 8])
def test_tiny_tables(gpu_backend, field_id, m, n):
    rng = np.random.default_rng(1000 * m + n + field_id)
    keys = distinct(rng, m + 3)                   # the last three are in no table row
    drawn = [keys[int(i)] for i in rng.integers(0, m + 3, n)]
    if (m + n) % 2 == 0:
        lookups = i64_column(drawn) if n else (np.zeros((0, 8), np.uint8), True)
    else:
        lookups = (mc.rows_of(field_id, drawn, 32) if n else np.zeros((0, 32), np.uint8), False)
    case = mc.Case(field_id, i64_column(keys[:m]), lookups)
    assert n < W or (case.want[1] > 0 and sum(case.want[0]) > 0)
    check(gpu_backend, case)


#--------------------------------------------------------------------------------------------------
# built clusters
#--------------------------------------------------------------------------------------------------
def keys_starting_at(field_id, table_rows, wanted, count_, start):
    """the next count_ integers x >= start (as keys) whose probe starts at a slot of `wanted`, by
    brute force over bzamd_multiplicity_first_slot -> (keys, the next start)"""
    found, x = [], start
    while len(found) < count_:
        element = mc.rows_of(field_id, [x], 32)[0]
        if api.multiplicity_first_slot(field_id, element, table_rows) in wanted:
            found.append(x)
        x += 1
    return found, x


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_cluster_of_forty_keys(gpu_backend, field_id):
    """40 table keys with ONE first slot among 128: whichever order they arrive in, they lie in 40
    consecutive slots; lookups hit the last row, the first and every other one; missing keys that
    start at the cluster's head, inside it and at its last slot walk to its end"""
    m, at = 40, 100
    assert mc.slots(m) == 128
    table, x = keys_starting_at(field_id, m, {at}, m, 1)
    inside = {(at + d) % 128 for d in range(m)}
    missing, x = keys_starting_at(field_id, m, inside, 30, x)
    missing += keys_starting_at(field_id, m, {at}, 2, x)[0]
    missing += keys_starting_at(field_id, m, {(at + m - 1) % 128}, 1, x)[0]
    lookups = [table[39]] * 70 + table + missing + [table[39], table[0]] * 10
    case = mc.Case(field_id, i64_column(table), i64_column(lookups))
    assert case.want[0][39] == 81 and case.want[1] >= 33
    check(gpu_backend, case)


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_cluster_wraps_past_the_last_slot(gpu_backend, field_id):
    """m = 5 in 16 slots: four keys start at slot 15 and lie in 15, 0, 1, 2, a key that starts at 0
    lies behind them; misses start at 15, 0 and 2 and end at the first empty slot"""
    m = 5
    last, x = keys_starting_at(field_id, m, {15}, 4, 1)
    zero, x = keys_starting_at(field_id, m, {0}, 1, x)
    table = last + zero
    missing, x = keys_starting_at(field_id, m, {15}, 3, x)
    missing += keys_starting_at(field_id, m, {0, 1, 2}, 6, x)[0]
    lookups = (table * 3 + missing) * 5 + [table[3], table[4]] * W
    case = mc.Case(field_id, i64_column(table),
                   (mc.rows_of(field_id, lookups, 32), False))
    assert case.want[1] == 45 and case.want[0] == [15, 15, 15, 15 + W, 15 + W]
    check(gpu_backend, case)


#--------------------------------------------------------------------------------------------------
# duplicates in the table
#--------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_table_of_equal_rows(gpu_backend, field_id):
    """3 B + 5 equal rows, all inserted at once into one slot: only row 0 counts"""
    m = 3 * B + 5
    table = (np.full(m, -77, np.int16).view(np.uint8).reshape(m, 2), True)
    case = mc.Case(field_id, table, i64_column([-77, 77, -77, -77, 5]))
    assert case.want == ([3] + [0] * (m - 1), 2)
    check(gpu_backend, case)


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_every_key_twice(gpu_backend, field_id):
    """copies at distance 1 (the same wavefront) and at distance B (the next workgroup); the copy
    BEFORE which the lookups' rows lie is the one that counts"""
    rng = np.random.default_rng(77)
    near, far = distinct(rng, B // 2), distinct(rng, B, low=2**62, high=2**63 - 1)
    table = [k for key in near for k in (key, key)] + far + far
    lookups = [table[int(i)] for i in rng.integers(0, len(table), 3 * B + 5)] + [1 - 2**63] * 3
    case = mc.Case(field_id, i64_column(table), i64_column(lookups))
    counts = case.want[0]
    assert not any(counts[1:B:2]) and not any(counts[2 * B:]) and case.want[1] == 3
    assert sum(counts) == 3 * B + 5
    check(gpu_backend, case)


#--------------------------------------------------------------------------------------------------
# aggregation within the wavefront
#--------------------------------------------------------------------------------------------------
AGGREGATION = {
    "one_key": lambda keys, i: keys[7],
    "one_missing_key": lambda keys, i: keys[-1],
    "two_keys_alternating_by_lane": lambda keys, i: keys[3 + (i & 1)],
    "a_hit_and_a_miss_alternating": lambda keys, i: keys[-1 - (i & 1) * 5],
    "64_distinct_keys_in_each_wavefront": lambda keys, i: keys[i % W],
    "lanes_in_four_runs": lambda keys, i: keys[(i % W) // 16],
}


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("padding", [0, LDS_BINS])
@pytest.mark.parametrize("n", [3 * B + 5, W + 1])
@pytest.mark.parametrize("shape", sorted(AGGREGATION))
def test_aggregation(gpu_backend, field_id, shape, n, padding):
    """n = 3 B + 5 and W + 1: the last wavefront has five lanes (one lane) inside n.  padding: rows
    behind the table's 73 that nothing looks up; with them the table is too large for the bins in
    LDS and every add is the wavefront's aggregated one"""
    rng = np.random.default_rng(5)
    keys = distinct(rng, W + 10)   # the last one is in no table row
    lookups = [AGGREGATION[shape](keys, i) for i in range(n)]
    unused = distinct(rng, padding, low=2**62, high=2**63 - 1)
    case = mc.Case(field_id, i64_column(keys[:-1] + unused), i64_column(lookups))
    check(gpu_backend, case)
    check(gpu_backend, case, want_misses=False)


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("m", [LDS_BINS - 1, LDS_BINS, LDS_BINS + 1])
def test_tables_around_the_bins_in_lds(gpu_backend, field_id, m):
    """the last table counted in LDS and the first counted in global memory; the last rows of the
    table are looked up, runs of one key cross the wavefronts, and 3 B + 5 lookups on more than
    one workgroup add to the same rows"""
    rng = np.random.default_rng(m)
    keys = distinct(rng, m + 20)
    drawn = [keys[int(i)] for i in rng.integers(0, m + 20, 2 * B)]
    lookups = drawn + [keys[m - 1]] * (B + 3) + [keys[m - 2], keys[0]]
    case = mc.Case(field_id, i64_column(keys[:m]), i64_column(lookups))
    assert case.want[0][m - 1] >= B + 3 and case.want[1] > 0
    check(gpu_backend, case)


#--------------------------------------------------------------------------------------------------
# kinds
#--------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_kinds(gpu_backend, field_id):
    p = MODULUS[field_id]
    rng = np.random.default_rng(9)
    # i16 lookups into an i64 table
    table = [int(v) for v in rng.integers(-300, 300, 200)] + [2**40, -2**40, -2**15, 2**15 - 1]
    lookups = [int(v) for v in rng.integers(-400, 400, 1000)] + [-2**15, 2**15 - 1, -1]
    case = mc.Case(field_id, i64_column(table),
                   (np.array(lookups, np.int16).view(np.uint8).reshape(len(lookups), 2), True))
    assert case.want[1] > 0 and sum(case.want[0]) > 100
    check(gpu_backend, case)
    # i8 negatives into the 32-byte p - |x|
    table = [p - x for x in range(1, 100)] + [5, 6]
    lookups = [int(v) for v in rng.integers(-128, 8, 500)]
    case = mc.Case(field_id, (mc.rows_of(field_id, table, 32), False),
                   (np.array(lookups, np.int8).view(np.uint8).reshape(len(lookups), 1), True))
    assert case.want[1] > 0 and sum(case.want[0][:99]) > 100
    check(gpu_backend, case)
    # unreduced 32-byte rows on both sides: x + p against x, the largest 32 bytes against its value
    values = distinct(rng, 50, low=0, high=2**62)
    raw = [cic.element_raw(field_id, v) for v in values]
    top = (1 << 256) - 1
    table = [r + p if i % 2 else r for i, r in enumerate(raw)] + [top]
    lookups = [raw[int(i)] + (p if i % 3 == 0 else 0) for i in rng.integers(0, 50, 400)]
    lookups += [cic.element_raw(field_id, cic.raw_value(field_id, top)), top, raw[0] + 1]
    case = mc.Case(field_id, (mc.rows_of(field_id, table, 32, raw=True), False),
                   (mc.rows_of(field_id, lookups, 32, raw=True), False))
    assert case.want[0][50] == 2 and sum(case.want[0]) == 402 and case.want[1] == 1
    check(gpu_backend, case)
    # the same elements against the narrow integers they mean
    case = mc.Case(field_id, (mc.rows_of(field_id, values, 9), False),
                   (mc.rows_of(field_id, lookups[:400], 32, raw=True), False))
    assert sum(case.want[0]) == 400
    check(gpu_backend, case)


#--------------------------------------------------------------------------------------------------
# more rows than the grid covers in one stride, on each side
#--------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_more_rows_than_one_stride_of_the_grid(gpu_backend):
    """2^20 + 256 table rows and as many lookups on at most 2048 workgroups of 256: every lane
    takes a second row, the lanes of workgroup 0 a third.  Checked in full against the model; the
    same three launches as at m = 1"""
    import torch
    field_id, rows = 0, (1 << 20) + B
    assert rows > 2 * GRID_CAP * B
    rng = np.random.default_rng(31)
    table = rng.permutation(rows).astype(np.int64) * 3 + 1
    table[rows - 1000:] = table[:1000]                      # duplicates a million rows apart
    lookups = table[rng.integers(0, rows, rows)]
    lookups[-300:] = table[12345]
    lookups[::5] += 1                                       # 3 k + 2: in no table row
    # a wavefront's row in one turn of its loop and in the next are the same row
    lookups[:2 * B] = lookups[GRID_CAP * B:GRID_CAP * B + 2 * B] = table[7]
    want, want_misses = mc.count(table.tolist(), lookups.tolist())
    assert rows // 6 < want_misses <= len(lookups[::5]) and not any(want[rows - 1000:])
    assert want[7] >= 4 * B
    d_table, d_lookups = _up(table.view(np.uint8)), _up(lookups.view(np.uint8))
    out = torch.full((rows + 2,), CANARY, dtype=torch.uint8, device=_device()).repeat_interleave(8)
    workspace_bytes = gpu_backend.count_multiplicities_workspace_bytes(rows)
    workspace = torch.empty(workspace_bytes, dtype=torch.uint8, device=_device())
    side = torch.cuda.Stream(device=_device())
    torch.cuda.synchronize()
    before = _launches()
    gpu_backend.count_multiplicities_device(
        field_id, out.data_ptr(), out.data_ptr() + 8 * (rows + 1),
        (d_table.data_ptr(), rows, 8, True), (d_lookups.data_ptr(), rows, 8, True),
        workspace.data_ptr(), workspace_bytes, stream=side.cuda_stream)
    assert _launches() - before == HASHED
    side.synchronize()
    words = out.cpu().numpy().view(np.uint64)
    assert words[rows] == CANARY_WORD and words[rows + 1] == want_misses
    assert np.array_equal(words[:rows], np.array(want, np.uint64))
    assert np.array_equal(d_table.cpu().numpy(), table.view(np.uint8))
    assert np.array_equal(d_lookups.cpu().numpy(), lookups.view(np.uint8))


#--------------------------------------------------------------------------------------------------
# the range table
#--------------------------------------------------------------------------------------------------
RANGE_KINDS = {"u8": (1, False), "i8": (1, True), "u16": (2, False), "i64": (8, True),
               "element": (32, False)}
RANGE_ROWS = 10000   # u8: 625 16-byte loads on three workgroups; i64: 40 workgroups


def range_lookups(field_id, rng, m, kind):
    width, signed = kind
    p = MODULUS[field_id]
    if width == 32:
        values = [int(v) for v in rng.integers(0, m + max(m // 4, 2), RANGE_ROWS - 6)]
        values += [m - 1, m, p - 1, 1 << 64, (1 << 192) + (m - 1), (1 << 128)]
        values[64:364] = [m - 1] * 300
        return (mc.rows_of(field_id, values, 32), False)
    low = -(1 << (8 * width - 1)) if signed else 0
    high = (1 << (8 * width - 1)) if signed else (1 << (8 * width))
    top = min(high, m + max(m // 4, 2))
    values = [int(v) for v in rng.integers(max(low, -top), top, RANGE_ROWS - 4)]
    values += [v for v in (m - 1, m, low, high - 1) if low <= v < high]
    values[64:364] = [min(m, high) - 1] * 300   # a run of one row across lanes and wavefronts
    return (mc.rows_of(field_id, values, width, signed), signed)


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("kind", sorted(RANGE_KINDS))
@pytest.mark.parametrize("m", [1, 255, 256, 257, LDS_BINS - 1, LDS_BINS, LDS_BINS + 1])
def test_range_table(gpu_backend, field_id, m, kind):
    """bins in LDS up to 4096 rows and global adds above; lookups at odd addresses (a one-byte
    column: rows one at a time up to the first multiple of 16, whole 16 bytes from there) and at
    multiples of 16; values at m - 1 and m, negative ones, 32-byte keys with a high word set; two
    and more workgroups add to the same rows"""
    rng = np.random.default_rng(m + len(kind))
    lookups = range_lookups(field_id, rng, m, RANGE_KINDS[kind])
    for aligned in (False, True):
        case = mc.Case(field_id, None, lookups, table_rows=m, aligned=aligned)
        assert case.want[0][m - 1] >= 1 or not mc.fits(m - 1, *RANGE_KINDS[kind])
        assert case.want[1] >= 1 or (kind == "u8" and m >= 256)
        check(gpu_backend, case)
    check(gpu_backend, case, want_misses=False)


@pytest.mark.gpu
def test_range_table_without_lookups(gpu_backend):
    case = mc.Case(0, None, (np.zeros((0, 1), np.uint8), False), table_rows=LDS_BINS + 5)
    check(gpu_backend, case)


#--------------------------------------------------------------------------------------------------
# host form on the gpu backend
#--------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_host_form_on_gpu_equals_the_device_form(gpu_backend, field_id):
    rng = np.random.default_rng(field_id)
    keys = distinct(rng, 600)
    table = keys[:500] + keys[:50]
    lookups = [keys[int(i)] for i in rng.integers(0, 600, 3000)]
    case = mc.Case(field_id, (mc.rows_of(field_id, table, 32), False), i64_column(lookups))
    got, misses = count_on_device(gpu_backend, case)
    before = _launches()
    host, host_misses = gpu_backend.count_multiplicities(
        field_id, (case.table[0].copy(), False), (case.lookups[0].copy(), True))
    assert _launches() - before == HASHED, "no kernel ran"
    assert np.array_equal(host, got) and host_misses == misses
    assert np.array_equal(host, case.want_multiplicities()) and misses == case.want[1]
    small = (np.array(lookups, np.int64) & 1023).astype(np.uint16)
    case = mc.Case(field_id, None, (small.view(np.uint8).reshape(len(small), 2), False),
                   table_rows=1000)
    got, misses = count_on_device(gpu_backend, case)
    before = _launches()
    host, host_misses = gpu_backend.count_multiplicities(field_id, (None, 1000), small)
    assert _launches() - before == RANGE, "no kernel ran"
    assert np.array_equal(host, got) and host_misses == misses == case.want[1]
    assert np.array_equal(host, case.want_multiplicities())


#--------------------------------------------------------------------------------------------------
# the lookup argument on one stream
#--------------------------------------------------------------------------------------------------
def prove_lookup_on_one_stream(gpu_backend, table, lookups, alpha):
    """count, invert both columns with the shift alpha, commit to the multiplicities (beside the
    model's column), prove sum_i M[i] starT[i] - starL[i] = 0 over n = len(lookups) rows; nothing
    synchronises before the end -> what the host needs to judge"""
    import torch
    field_id, dev = 0, _device()
    m, n = len(table), len(lookups)
    want, want_misses = mc.count(table.tolist(), lookups.tolist())
    d_table, d_lookups = _up(table.view(np.uint8)), _up(lookups.view(np.uint8))
    d_alpha = _up(to_bytes(field_id, alpha))
    out = torch.full((m + 3,), CANARY, dtype=torch.uint8, device=dev).repeat_interleave(8)
    multiplicities, misses = out.data_ptr(), out.data_ptr() + 8 * (m + 1)
    count_bytes = gpu_backend.count_multiplicities_workspace_bytes(m)
    count_workspace = torch.empty(count_bytes, dtype=torch.uint8, device=dev)
    star_t = torch.zeros((m, 32), dtype=torch.uint8, device=dev)
    star_l = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    d_model = _up(np.array(want, np.uint64).view(np.uint8))
    d_generators = _up(api.get_generators(m).view(np.uint8))
    commitments = torch.zeros((2, 32), dtype=torch.uint8, device=dev)
    got_desc = (api.sxt_sequence_descriptor * 1)(api.sxt_sequence_descriptor(8, m, multiplicities, 0))
    model_desc = (api.sxt_sequence_descriptor * 1)(
        api.sxt_sequence_descriptor(8, m, d_model.data_ptr(), 0))
    p = MODULUS[field_id]
    mles = [(multiplicities, m, 8, False), (star_t.data_ptr(), m, 32, False),
            (star_l.data_ptr(), n, 32, False)]
    terms = [0, 1, 2]
    table_of_products = product_table(field_id, [to_bytes(field_id, 1), to_bytes(field_id, p - 1)],
                                      [2, 1], api.SUMCHECK_PRODUCT_STRIDE[field_id])
    v = variables(n)
    polys = torch.zeros((v, 3, 32), dtype=torch.uint8, device=dev)
    point = torch.zeros((v, 32), dtype=torch.uint8, device=dev)
    evaluations = torch.zeros((3, 32), dtype=torch.uint8, device=dev)
    t0 = merlin_ref.Transcript(label="lookup").array()
    transcript = _up(t0)
    workspace_bytes = api.sumcheck_transcript_columns_workspace_bytes(field_id, n, 3, 2, 3, 2)
    workspace = torch.empty(workspace_bytes, dtype=torch.uint8, device=dev)

    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    before = _launches()
    gpu_backend.count_multiplicities_device(
        field_id, multiplicities, misses, (d_table.data_ptr(), m, 8, True),
        (d_lookups.data_ptr(), n, 8, True), count_workspace.data_ptr(), count_bytes,
        stream=side.cuda_stream)
    assert _launches() - before == HASHED
    gpu_backend.invert_columns_device(field_id, star_t.data_ptr(), None,
                                      [(d_table.data_ptr(), m, 8, True)], None, d_alpha.data_ptr(),
                                      m, stream=side.cuda_stream)
    gpu_backend.invert_columns_device(field_id, star_l.data_ptr(), None,
                                      [(d_lookups.data_ptr(), n, 8, True)], None,
                                      d_alpha.data_ptr(), n, stream=side.cuda_stream)
    lib = api.load()
    lib.bzamd_msm_device(0, commitments[0].data_ptr(), 1, got_desc, d_generators.data_ptr(),
                         side.cuda_stream)
    lib.bzamd_msm_device(0, commitments[1].data_ptr(), 1, model_desc, d_generators.data_ptr(),
                         side.cuda_stream)
    gpu_backend.prove_sumcheck_transcript_device_columns(
        field_id, mles, table_of_products, terms, n, 2, polys.data_ptr(), point.data_ptr(),
        evaluations.data_ptr(), transcript.data_ptr(), workspace.data_ptr(), workspace_bytes,
        stream=side.cuda_stream)
    side.synchronize()

    words = out.cpu().numpy().view(np.uint64)
    assert words[m] == CANARY_WORD and words[m + 2] == CANARY_WORD
    assert np.array_equal(words[:m], np.array(want, np.uint64)) and words[m + 1] == want_misses
    got_commitments = commitments.cpu().numpy()
    assert got_commitments[0].any()
    assert np.array_equal(got_commitments[0], got_commitments[1])
    host_polys = polys.cpu().numpy()
    accepted = {}
    for claimed in (0, 1):
        ok, expected, v_point, _ = gpu_backend.verify_sumcheck(
            field_id, to_bytes(field_id, claimed), host_polys, t0)
        accepted[claimed] = bool(ok)
        if ok:
            assert np.array_equal(v_point, point.cpu().numpy())
            assert gpu_backend.check_sumcheck_evaluations(
                field_id, expected, evaluations.cpu().numpy(), table_of_products, terms)
    return want, int(words[m + 1]), accepted


@pytest.mark.gpu
def test_lookup_argument_on_one_stream(gpu_backend):
    """sum_t m[t] / (alpha + T[t]) = sum_i 1 / (alpha + L[i]) from two columns in HBM to a verified
    sumcheck; with one lookup row outside the table the count reports it and the proof of the
    claimed sum 0 is rejected"""
    p = MODULUS[0]
    rng = np.random.default_rng(41)
    alpha = int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % p
    table = np.array(distinct(rng, 300), np.int64)
    drawn = rng.integers(0, 250, 700)            # rows 250 .. 299 are never drawn
    drawn[100:170] = 17                          # one row more than 64 times
    lookups = table[drawn]
    assert all((int(x) + alpha) % p for x in table)
    want, misses, accepted = prove_lookup_on_one_stream(gpu_backend, table, lookups, alpha)
    assert misses == 0 and accepted == {0: True, 1: False}
    assert want[17] > 64 and not any(want[250:]) and sum(want) == 700
    outside = lookups.copy()
    outside[333] = int(table.max()) + 1
    assert (int(outside[333]) + alpha) % p
    want, misses, accepted = prove_lookup_on_one_stream(gpu_backend, table, outside, alpha)
    assert misses == 1 and sum(want) == 699 and accepted == {0: False, 1: False}
