"""The device form of the sums by key (include/blitzar_amd.h: bzamd_sum_by_key_device), the host
form on the GPU backend, and a group-by chain on one stream: sums, counts, their commitments, the
inverse columns and the log-derivative identity.

Expected values are Python integers (tests/key_sum_cases.py).  The sizes follow the kernels'
constants (proof/key_sums.hip, proof/key_table.h): wavefronts of 64 lanes, workgroups of 256, at
most 2048 of them; a table of at most 4096 rows whose rows x accumulators (one per 32 bits of every
value column) are at most 4096 is summed in bins in LDS (at most 1024 workgroups), larger ones with
adds to global memory, reduced across the wavefront when all its hit lanes share a row.  Every
call is checked for its launch count, the canaries behind each output, around `misses` and behind
the workspace (placed one byte past an allocation), its untouched inputs, against the model, and is
run twice: the two results must be the same bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

from blitzar_amd import api
from tests import key_sum_cases as kc
from tests import multiplicity_cases as mc
from tests.test_multiplicities_device import AGGREGATION, distinct, keys_starting_at
from tests.test_sumcheck_device import MODULUS, to_bytes
from tests.univariate_cases import scalar_values

W = 64               # lanes of a wavefront
B = 256              # kCountThreads
GRID_CAP = 2048      # kCountBlocks
LDS_BINS = 4096      # kLdsBins: table rows counted in LDS
LDS_SUM_BINS = 4096  # kLdsSumBins: rows x accumulators summed in LDS
HASHED, RANGE = 4, 3  # launches of one call, whatever m, n, num_values and the data are
CANARY = kc.CANARY
OUTPUTS = ("sums", "scalars", "counts", "misses", "matches")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64, I128, U248, ELEMENT = (8, True), (16, True), (31, False), (32, False)


def _launches():
    return api.load().bzamd_kernel_launch_count()


def _device():
    import torch
    return torch.device("cuda", 0)


def _up(array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array).copy()).to(_device())


def lds_threshold(kinds):
    """the most table rows summed in LDS with value columns of these kinds"""
    row_chunks = sum(kc.chunks_of(width) for width, _ in kinds)
    return min(LDS_BINS, LDS_SUM_BINS // row_chunks) if row_chunks else LDS_BINS


def once(lib_api, case, want, d_flat, d_values):
    """one call on a stream of its own -> the raw bytes of every output, canaries included"""
    import torch
    m, n, count, dev = case.m, case.n, len(case.values), _device()
    sizes = {"sums": 32 * m * count, "scalars": 32 * m * count, "counts": 8 * m, "misses": 8,
             "matches": 4 * n}
    out = {name: torch.full((8 + sizes[name] + 8,), CANARY, dtype=torch.uint8, device=dev)
           for name in OUTPUTS}
    hashed = case.table is not None
    need = lib_api.sum_by_key_workspace_bytes(m, count) if hashed or count else 0
    workspace = torch.full((need + 1 + 64,), CANARY, dtype=torch.uint8, device=dev)
    table, lookups = case.descriptors(d_flat.data_ptr())
    values = case.value_descriptors(d_values.data_ptr())
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    before = _launches()
    lib_api.sum_by_key_device(
        case.field_id, *(out[name].data_ptr() + 8 if name in want else None for name in OUTPUTS),
        table, lookups, values, workspace.data_ptr() + 1 if need else None, need,
        stream=side.cuda_stream)
    assert _launches() - before == (HASHED if hashed else RANGE)
    side.synchronize()
    host = {name: out[name].cpu().numpy() for name in OUTPUTS}
    for name in OUTPUTS:
        body = host[name][8:8 + sizes[name]]
        assert np.all(host[name][:8] == CANARY), f"before `{name}`"
        assert np.all(host[name][8 + sizes[name]:] == CANARY), f"behind `{name}`"
        assert name in want or np.all(body == CANARY), f"`{name}` was written"
    tail = workspace.cpu().numpy()
    assert tail[0] == CANARY and np.all(tail[1 + need:] == CANARY), "past the workspace"
    assert np.array_equal(d_flat.cpu().numpy(), case.flat), "the key columns were modified"
    assert np.array_equal(d_values.cpu().numpy(), case.value_flat), "a value column was modified"
    return {name: host[name][8:8 + sizes[name]] for name in want}


def run(lib_api, case, want=OUTPUTS):
    """twice, bit-identical -> the outputs in `want`, shaped"""
    d_flat, d_values = _up(case.flat), _up(case.value_flat)
    first = once(lib_api, case, want, d_flat, d_values)
    second = once(lib_api, case, want, d_flat, d_values)
    for name in want:
        assert np.array_equal(first[name], second[name]), f"`{name}` differs between two runs"
    m, count = case.m, len(case.values)
    shaped = {"sums": lambda a: a.reshape(count, m, 32), "scalars": lambda a: a.reshape(count, m, 32),
              "counts": lambda a: a.copy().view(np.uint64),
              "misses": lambda a: int(a.copy().view(np.uint64)[0]),
              "matches": lambda a: a.copy().view(np.uint32)}
    return {name: shaped[name](first[name]) for name in want}


def check(lib_api, case, want=OUTPUTS):
    got = run(lib_api, case, want)
    expected = {"sums": case.want_sums, "scalars": case.want_scalars, "counts": case.want_counts,
                "misses": lambda: case.want[1], "matches": case.want_matches}
    for name in want:
        assert np.array_equal(got[name], expected[name]()), name
    return got


def value_columns(field_id, rng, kinds, n, short=True):
    """one column per kind, extremes among the rows; every other one a few rows shorter than n"""
    columns = []
    for j, kind in enumerate(kinds):
        rows = max(n - (5 * j if short and j % 2 else 0), 0)
        columns.append(kc.column(field_id, kc.drawn(rng, kind, rows), kind))
    return columns


def keys_column(field_id, keys, as_elements):
    if not keys:
        return (np.zeros((0, 32 if as_elements else 8), np.uint8), not as_elements)
    return (mc.rows_of(field_id, keys, 32), False) if as_elements else kc.i64_column(keys)


#--------------------------------------------------------------------------------------------------
# tiny tables: the probe wraps, the table is as full as it gets
#--------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("n", [0, 1, W - 1, W, W + 1, 3 * B + 5])
@pytest.mark.parametrize("m", [1, 2, 3, 5, 8])
def test_tiny_tables(gpu_backend, field_id, m, n):
    rng = np.random.default_rng(1000 * m + n + field_id)
    keys = distinct(rng, m + 3)                   # the last three are in no table row
    lookups = [keys[int(i)] for i in rng.integers(0, m + 3, n)]
    values = value_columns(field_id, rng, [I64, ELEMENT, I128, (3, False)], n)
    case = kc.Case(field_id, kc.i64_column(keys[:m]),
                   keys_column(field_id, lookups, (m + n) % 2 == 1), values)
    assert n < W or (case.want[1] > 0 and sum(case.want[0]) > 0)
    check(gpu_backend, case)


#--------------------------------------------------------------------------------------------------
# around the bins in LDS
#--------------------------------------------------------------------------------------------------
THRESHOLD_KINDS = {"one_i64": [I64], "eight_i64": [I64] * kc.MAX_VALUES, "one_element": [ELEMENT],
                   "none": []}


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("kinds", sorted(THRESHOLD_KINDS))
def test_tables_around_the_bins_in_lds(gpu_backend, field_id, kinds, delta):
    """the last table summed in LDS and the first summed in global memory, for one and for the
    most value columns (2048, 256, 512 rows; 4096 without values): the last rows of the table are
    looked up, a run of one key crosses the wavefronts, and 3 B + 5 lookups on more than one
    workgroup add to the same rows"""
    kinds = THRESHOLD_KINDS[kinds]
    m = lds_threshold(kinds) + delta
    rng = np.random.default_rng(m)
    keys = distinct(rng, m + 20)
    drawn = [keys[int(i)] for i in rng.integers(0, m + 20, 2 * B)]
    lookups = drawn + [keys[m - 1]] * (B + 3) + [keys[m - 2], keys[0]]
    values = value_columns(field_id, rng, kinds, len(lookups))
    case = kc.Case(field_id, kc.i64_column(keys[:m]), kc.i64_column(lookups), values)
    assert case.want[0][m - 1] >= B + 3 and case.want[1] > 0
    check(gpu_backend, case, OUTPUTS if kinds else ("counts", "misses", "matches"))


#--------------------------------------------------------------------------------------------------
# the hot key, runs within the wavefront, clusters
#--------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("padding", [0, LDS_BINS])
@pytest.mark.parametrize("n", [3 * B + 5, W + 1])
@pytest.mark.parametrize("shape", sorted(AGGREGATION))
def test_runs_within_the_wavefront(gpu_backend, field_id, shape, n, padding):
    """one key in every lane (the hot key: with the padding rows the table is above the bins in
    LDS and the wavefront adds once per accumulator), a key no table row has, two keys alternating
    by lane, hits and misses alternating, 64 keys in each wavefront, four runs; n = 3 B + 5 and
    W + 1: the last wavefront has five lanes (one lane) inside n.  Value columns a few rows short:
    lanes of a wavefront on one row of which some have no value"""
    rng = np.random.default_rng(5)
    keys = distinct(rng, W + 10)   # the last one is in no table row
    lookups = [AGGREGATION[shape](keys, i) for i in range(n)]
    unused = distinct(rng, padding, low=2**62, high=2**63 - 1)
    values = value_columns(field_id, rng, [I64, ELEMENT, I128], n)
    case = kc.Case(field_id, kc.i64_column(keys[:-1] + unused), kc.i64_column(lookups), values)
    check(gpu_backend, case)
    check(gpu_backend, case, want=("scalars",))


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_hot_key_that_cancels(gpu_backend, field_id):
    """a table above the bins in LDS, every lookup on one key: +x and -x by lane cancel inside the
    wavefront's sum (nothing is added), rows of p - 1 wrap p, the i128 extremes meet"""
    p = MODULUS[field_id]
    m, n = LDS_BINS + 7, 5 * B + 9
    rng = np.random.default_rng(11)
    keys = distinct(rng, m)
    low, high = kc.extremes(I128)
    cancel = [(-1) ** i * 123456789012345 for i in range(n - 1)] + [0]
    extremes = [low if i % 3 else high for i in range(n)]
    values = [kc.column(field_id, cancel, I64), kc.column(field_id, [p - 1] * n, ELEMENT),
              kc.column(field_id, extremes, I128), kc.column(field_id, [(1 << 248) - 1] * n, U248)]
    case = kc.Case(field_id, kc.i64_column(keys), kc.i64_column([keys[m - 3]] * n), values)
    assert case.sums[0][m - 3] == 0 and case.sums[1][m - 3] == (-n) % p
    got = check(gpu_backend, case)
    assert not got["sums"][0].any()


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_cluster_that_wraps_past_the_last_slot(gpu_backend, field_id):
    """m = 5 in 16 slots: four keys start at slot 15 and lie in 15, 0, 1, 2, a key that starts at 0
    lies behind them; misses start at 15, 0 and 2 and end at the first empty slot"""
    m = 5
    last, x = keys_starting_at(field_id, m, {15}, 4, 1)
    zero, x = keys_starting_at(field_id, m, {0}, 1, x)
    table = last + zero
    missing, x = keys_starting_at(field_id, m, {15}, 3, x)
    missing += keys_starting_at(field_id, m, {0, 1, 2}, 6, x)[0]
    lookups = (table * 3 + missing) * 5 + [table[3], table[4]] * W
    rng = np.random.default_rng(3)
    values = value_columns(field_id, rng, [I64, ELEMENT], len(lookups))
    case = kc.Case(field_id, kc.i64_column(table), (mc.rows_of(field_id, lookups, 32), False),
                   values)
    assert case.want[1] == 45 and case.want[0] == [15, 15, 15, 15 + W, 15 + W]
    check(gpu_backend, case)


@pytest.mark.gpu
def test_cluster_of_forty_keys_with_duplicates(gpu_backend):
    """40 table keys with ONE first slot among 128 and every key a second time behind them: sums
    go to the first occurrences, the copies stay zero"""
    field_id, m, at = 1, 40, 100
    table, x = keys_starting_at(field_id, 2 * m, {at}, m, 1)
    missing = keys_starting_at(field_id, 2 * m, {at}, 2, x)[0]
    lookups = [table[39]] * 70 + table + missing + [table[39], table[0]] * 10
    rng = np.random.default_rng(4)
    values = value_columns(field_id, rng, [I128, ELEMENT], len(lookups))
    case = kc.Case(field_id, kc.i64_column(table + table), kc.i64_column(lookups), values)
    assert case.want[0][39] == 81 and not any(case.want[0][m:]) and case.want[1] == 2
    got = check(gpu_backend, case)
    assert not got["sums"][:, m:].any() and kc.MISS in case.matches


#--------------------------------------------------------------------------------------------------
# more rows than the grid covers in one stride
#--------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_more_rows_than_one_stride_of_the_grid(gpu_backend):
    """n = 2048 x 256 + 65 i64 rows on at most 2048 workgroups of 256: the first 65 lanes take a
    second row.  A table above the bins in LDS; a wavefront's row in one turn of its loop and in
    the next are the same row; the same four launches as at m = 1"""
    field_id, m, n = 0, LDS_BINS // 2 + 1, GRID_CAP * B + 65
    assert lds_threshold([I64]) < m
    rng = np.random.default_rng(31)
    table = rng.permutation(m).astype(np.int64) * 3 + 1
    lookups = table[rng.integers(0, m, n)]
    lookups[::7] += 1                                       # 3 k + 2: in no table row
    lookups[:2 * B] = lookups[GRID_CAP * B:] = table[7]
    amounts = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
    case = kc.Case(field_id, (table.view(np.uint8).reshape(m, 8), True),
                   (lookups.view(np.uint8).reshape(n, 8), True),
                   [(amounts.view(np.uint8).reshape(n, 8), True)])
    assert case.want[1] > n // 10 and min(case.want[0]) > 0
    check(gpu_backend, case)


#--------------------------------------------------------------------------------------------------
# the range table
#--------------------------------------------------------------------------------------------------
RANGE_KINDS = {"u8": (1, False), "i16": (2, True), "i64": I64, "element": ELEMENT}


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("kind", sorted(RANGE_KINDS))
@pytest.mark.parametrize("m", [1, 255, 2048, 2049, LDS_BINS + 1])
def test_range_table(gpu_backend, field_id, m, kind):
    """T[t] = t, three launches: bins in LDS up to 2048 rows with one i64 value column, global adds
    above; keys at m - 1 and m, negative ones, 32-byte keys with a high word set; a run of one key
    across lanes and wavefronts; columns at odd addresses and at multiples of 16"""
    width, signed = RANGE_KINDS[kind]
    p = MODULUS[field_id]
    rng = np.random.default_rng(m + width)
    low, high = (0, p) if width == 32 else kc.extremes((width, signed))
    top = min(high, m + max(m // 4, 2))
    keys = [int(v) for v in rng.integers(max(low, -top), top, 3 * B + 5)]
    keys += [v for v in (m - 1, m, low, -1) if low <= v <= high]
    if width == 32:
        keys += [1 << 64, (1 << 192) + (m - 1), p - 1]
    keys[64:364] = [min(m - 1, high)] * 300
    values = value_columns(field_id, rng, [I64], len(keys))
    for aligned in (False, True):
        case = kc.Case(field_id, None, kc.column(field_id, keys, (width, signed)), values,
                       table_rows=m, aligned=aligned)
        assert case.want[0][min(m - 1, high)] >= 300
        check(gpu_backend, case)
    join = kc.Case(field_id, None, kc.column(field_id, keys, (width, signed)), [], table_rows=m)
    check(gpu_backend, join, want=("matches",))


#--------------------------------------------------------------------------------------------------
# every output null in turn, matches alone
#--------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("m", [300, LDS_BINS + 300])
def test_outputs_null_in_turn(gpu_backend, field_id, m):
    rng = np.random.default_rng(m)
    keys = distinct(rng, m + 30)
    lookups = [keys[int(i)] for i in rng.integers(0, m + 30, 3 * B + 5)]
    values = value_columns(field_id, rng, [I64, ELEMENT], len(lookups))
    case = kc.Case(field_id, kc.i64_column(keys[:m]), kc.i64_column(lookups), values)
    for missing in OUTPUTS:
        check(gpu_backend, case, want=tuple(name for name in OUTPUTS if name != missing))
    check(gpu_backend, case, want=("sums",))
    join = kc.Case(field_id, kc.i64_column(keys[:m]), kc.i64_column(lookups), [])
    check(gpu_backend, join, want=("matches",))


#--------------------------------------------------------------------------------------------------
# host form on the gpu backend
#--------------------------------------------------------------------------------------------------
CPU_CHILD = """
import sys
import numpy as np
from blitzar_amd import api
assert api.init(api.SXT_CPU_BACKEND, 0) == 0
data = np.load(sys.argv[1])
got = api.sum_by_key(int(data["field_id"]), (data["table"], True), (data["lookups"], True),
                     [(data["amounts"], True), (data["elements"], False)])
np.savez(sys.argv[2], **got)
"""


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_host_form_on_gpu_equals_the_cpu_backend(gpu_backend, field_id, tmp_path):
    """bzamd_sum_by_key on the gpu backend (the device's accumulators) against the cpu backend in a
    child process (one field addition a row), and both against the model"""
    rng = np.random.default_rng(field_id)
    keys = distinct(rng, 600)
    table = keys[:500] + keys[:50]
    lookups = [keys[int(i)] for i in rng.integers(0, 600, 3000)]
    values = value_columns(field_id, rng, [I64, ELEMENT], len(lookups))
    case = kc.Case(field_id, kc.i64_column(table), kc.i64_column(lookups), values)
    before = _launches()
    host = gpu_backend.sum_by_key(field_id, case.table, case.lookups, case.values)
    assert _launches() - before == HASHED, "no kernel ran"
    np.savez(tmp_path / "in.npz", field_id=field_id, table=case.table[0], lookups=case.lookups[0],
             amounts=values[0][0], elements=values[1][0])
    subprocess.run([sys.executable, "-c", CPU_CHILD, str(tmp_path / "in.npz"),
                    str(tmp_path / "out.npz")], cwd=ROOT, check=True, timeout=120)
    cpu = np.load(tmp_path / "out.npz")
    for name in OUTPUTS:
        assert np.array_equal(host[name], cpu[name]), name
    assert np.array_equal(host["sums"], case.want_sums())
    assert np.array_equal(host["scalars"], case.want_scalars())
    assert np.array_equal(host["counts"], case.want_counts()) and host["misses"] == case.want[1]
    assert np.array_equal(host["matches"], case.want_matches())
    ranged = gpu_backend.sum_by_key(field_id, (None, 1000),
                                    (np.array(lookups, np.int64) & 1023).astype(np.uint16),
                                    [case.values[0]], want=("scalars", "counts", "misses"))
    small = kc.Case(field_id, None,
                    kc.column(field_id, [k & 1023 for k in lookups], (2, False)), [case.values[0]],
                    table_rows=1000)
    assert np.array_equal(ranged["scalars"], small.want_scalars())
    assert np.array_equal(ranged["counts"], small.want_counts())
    assert ranged["misses"] == small.want[1]


#--------------------------------------------------------------------------------------------------
# a group-by on one stream
#--------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_group_by_on_one_stream(gpu_backend):
    """sums and counts by key, the commitments to both beside those of the model's columns, the two
    inverse columns, and
      sum_t sums_v[t] / (alpha + T[t]) = sum_i value_v[i] / (alpha + L[i])
    in Python integers from the downloaded inverses; nothing synchronises before the end"""
    import torch
    field_id, dev = 0, _device()
    p = MODULUS[field_id]
    rng = np.random.default_rng(41)
    alpha = int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % p
    m, n = 300, 2000
    table = np.array(distinct(rng, m), np.int64)
    picked = rng.integers(0, 250, n)             # rows 250 .. 299 are never drawn
    picked[100:170] = 17                         # one row more than 64 times
    lookups = table[picked]
    amounts = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
    case = kc.Case(field_id, (table.view(np.uint8).reshape(m, 8), True),
                   (lookups.view(np.uint8).reshape(n, 8), True),
                   [(amounts.view(np.uint8).reshape(n, 8), True)])
    assert case.want[1] == 0 and all((int(x) + alpha) % p for x in table)
    d_table, d_lookups, d_amounts = (_up(a.view(np.uint8)) for a in (table, lookups, amounts))
    d_alpha = _up(to_bytes(field_id, alpha))
    scalars = torch.zeros((m, 32), dtype=torch.uint8, device=dev)
    counts = torch.zeros(m, dtype=torch.int64, device=dev)
    misses = torch.full((1,), -1, dtype=torch.int64, device=dev)
    need = gpu_backend.sum_by_key_workspace_bytes(m, 1)
    workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    star_t = torch.zeros((m, 32), dtype=torch.uint8, device=dev)
    star_l = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    d_want_scalars, d_want_counts = _up(case.want_scalars()[0]), _up(case.want_counts().view(np.uint8))
    d_generators = _up(api.get_generators(m).view(np.uint8))
    commitments = torch.zeros((4, 32), dtype=torch.uint8, device=dev)
    D = api.sxt_sequence_descriptor
    columns = [(D * 1)(D(32, m, scalars.data_ptr(), 0)), (D * 1)(D(8, m, counts.data_ptr(), 0)),
               (D * 1)(D(32, m, d_want_scalars.data_ptr(), 0)),
               (D * 1)(D(8, m, d_want_counts.data_ptr(), 0))]
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    before = _launches()
    gpu_backend.sum_by_key_device(
        field_id, None, scalars.data_ptr(), counts.data_ptr(), misses.data_ptr(), None,
        (d_table.data_ptr(), m, 8, True), (d_lookups.data_ptr(), n, 8, True),
        [(d_amounts.data_ptr(), n, 8, True)], workspace.data_ptr(), need, stream=side.cuda_stream)
    assert _launches() - before == HASHED
    lib = api.load()
    for j, column in enumerate(columns):
        lib.bzamd_msm_device(0, commitments[j].data_ptr(), 1, column, d_generators.data_ptr(),
                             side.cuda_stream)
    gpu_backend.invert_columns_device(field_id, None, star_t.data_ptr(),
                                      [(d_table.data_ptr(), m, 8, True)], None, d_alpha.data_ptr(),
                                      m, stream=side.cuda_stream)
    gpu_backend.invert_columns_device(field_id, None, star_l.data_ptr(),
                                      [(d_lookups.data_ptr(), n, 8, True)], None,
                                      d_alpha.data_ptr(), n, stream=side.cuda_stream)
    side.synchronize()
    assert int(misses[0]) == 0
    assert np.array_equal(scalars.cpu().numpy(), case.want_scalars()[0])
    assert np.array_equal(counts.cpu().numpy().view(np.uint64), case.want_counts())
    got = commitments.cpu().numpy()
    assert got[0].any() and got[1].any() and not np.array_equal(got[0], got[1])
    assert np.array_equal(got[0], got[2]) and np.array_equal(got[1], got[3])
    sums = scalar_values(scalars.cpu().numpy())
    inverse_t, inverse_l = scalar_values(star_t.cpu().numpy()), scalar_values(star_l.cpu().numpy())
    assert all((int(x) + alpha) * y % p == 1 for x, y in zip(table[:5], inverse_t))
    left = sum(s * y for s, y in zip(sums, inverse_t)) % p
    right = sum(int(a) % p * y for a, y in zip(amounts, inverse_l)) % p
    assert left == right and left != 0
