"""The device forms of the row selection (include/blitzar_amd.h: bzamd_select_rows_device,
bzamd_take_rows_device), the host forms on the GPU backend, and three chains on one stream: a
WHERE with its commitment, the distinct keys of a group-by, and a join with its anti-join.

Expected values come from the model in tests/select_row_cases.py.  The sizes follow the kernels'
constants (proof/select_rows.h): wavefronts of 64 lanes, a wavefront's 256 rows of a tile in four
rounds, tiles of 1024 rows, at most 2048 spans of whole tiles, one workgroup of 256 threads each.
Every call is checked for its launch count, the canaries before and behind each output, past the
workspace (placed one byte past an allocation) and in the tail without zero_tail, its untouched
inputs, against the model, and is run twice: the two results must be the same bits.  The selection
tests run in each store shape of the second launch (the `store_shape` fixture): one row a lane,
packed in LDS, and columns of up to 8 bytes packed beside wider ones that are not."""
import os
import subprocess
import sys

import numpy as np
import pytest

from blitzar_amd import api
from tests import select_row_cases as sc

W = sc.W                  # lanes of a wavefront
WAVE_ROWS = sc.WAVE_ROWS  # kSelectWaveRows
TILE = sc.TILE            # kSelectTileRows
MAX_SPANS = sc.MAX_SPANS  # kMaxSelectSpans
SELECT, TAKE = 2, 1       # launches of one call, whatever n, the columns and the data are
CANARY = sc.CANARY
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _launches():
    return api.load().bzamd_kernel_launch_count()


def _device():
    import torch
    return torch.device("cuda", 0)


def _up(array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array).copy()).to(_device())


def _canaries(nbytes):
    """eight canary bytes before and behind `nbytes` bytes of device memory, the body 8-byte
    aligned"""
    import torch
    return torch.full((8 + nbytes + 8,), CANARY, dtype=torch.uint8, device=_device())


def _body(buffer, name):
    host = buffer.cpu().numpy()
    assert np.all(host[:8] == CANARY), f"before `{name}`"
    assert np.all(host[-8:] == CANARY), f"behind `{name}`"
    return host[8:-8]


@pytest.fixture(params=[0, 8, 32], ids=["lane_stores", "packed_to_8", "packed"])
def store_shape(request, gpu_backend):
    """the second launch's store shape: every column one row a lane (a), columns of up to 8 bytes
    packed in LDS and the wider ones not, every column packed (b)"""
    before = gpu_backend.select_rows_packed_width(request.param)
    yield request.param
    gpu_backend.select_rows_packed_width(before)


class Case:
    """a selection with its inputs laid out in one flat buffer and what the call must leave in
    every output, computed once"""

    def __init__(self, selector, columns, reject=0, invert=False, capacity=None, zero_tail=False,
                 aligned=False, want_count=True, want_indices=True, skews=None):
        self.selector, self.columns = selector, list(columns)
        self.reject, self.invert, self.zero_tail = reject, invert, zero_tail
        self.capacity = len(selector) if capacity is None else capacity
        self.want_count, self.want_indices = want_count, want_indices
        self.layout = sc.Layout([selector, *self.columns], aligned, skews)
        self.count, self.indices, self.selected = sc.select(selector, self.columns, reject, invert,
                                                            self.capacity, zero_tail)


def once(lib_api, case, d_flat):
    """one call on a stream of its own, everything checked -> the bytes of every output"""
    import torch
    dev, capacity = _device(), case.capacity
    n = len(case.selector)
    count = _canaries(8)
    indices = _canaries(4 * capacity)
    selected = [_canaries(capacity * c.shape[1]) for c in case.columns]
    need = lib_api.select_rows_workspace_bytes(n)
    workspace = torch.full((need + 1 + 64,), CANARY, dtype=torch.uint8, device=dev)
    descriptors = case.layout.descriptors(d_flat.data_ptr())
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    before = _launches()
    lib_api.select_rows_device(
        count.data_ptr() + 8 if case.want_count else None,
        indices.data_ptr() + 8 if case.want_indices else None, descriptors[0], descriptors[1:],
        [b.data_ptr() + 8 for b in selected], capacity, workspace.data_ptr() + 1, need,
        reject=case.reject, invert=case.invert, zero_tail=case.zero_tail, stream=side.cuda_stream)
    assert _launches() - before == SELECT
    side.synchronize()
    tail = workspace.cpu().numpy()
    assert tail[0] == CANARY and np.all(tail[1 + need:] == CANARY), "past the workspace"
    assert np.array_equal(d_flat.cpu().numpy(), case.layout.flat), "an input was modified"
    got = [_body(count, "count"), _body(indices, "indices")]
    got += [_body(b, f"selected[{j}]") for j, b in enumerate(selected)]
    if case.want_count:
        assert int(got[0].view(np.uint64)[0]) == case.count
    else:
        assert np.all(got[0] == CANARY), "`count` was written"
    if case.want_indices:
        assert np.array_equal(got[1].view(np.uint32), case.indices), "indices"
    else:
        assert np.all(got[1] == CANARY), "`indices` was written"
    for j, want in enumerate(case.selected):
        assert np.array_equal(got[2 + j].reshape(want.shape), want), f"selected[{j}]"
    return np.concatenate(got)


def check(lib_api, case):
    """twice, bit-identical"""
    d_flat = _up(case.layout.flat)
    first = once(lib_api, case, d_flat)
    assert np.array_equal(first, once(lib_api, case, d_flat)), "two runs differ"
    return case.count


def check_take(lib_api, indices, columns, aligned=False):
    """bzamd_take_rows_device twice: one launch, canaries, untouched inputs, the model"""
    indices = np.ascontiguousarray(indices, dtype=np.uint32)
    layout = sc.Layout(columns, aligned)
    d_flat, d_indices = _up(layout.flat), _up(indices)
    want = sc.take(indices, columns)
    results = []
    for _ in range(2):
        import torch
        taken = [_canaries(len(indices) * c.shape[1]) for c in columns]
        side = torch.cuda.Stream(device=_device())
        torch.cuda.synchronize()
        before = _launches()
        lib_api.take_rows_device(d_indices.data_ptr(), len(indices),
                                 layout.descriptors(d_flat.data_ptr()),
                                 [b.data_ptr() + 8 for b in taken], stream=side.cuda_stream)
        assert _launches() - before == TAKE
        side.synchronize()
        assert np.array_equal(d_flat.cpu().numpy(), layout.flat), "a column was modified"
        assert np.array_equal(d_indices.cpu().numpy(), indices), "the indices were modified"
        got = [_body(b, f"taken[{j}]") for j, b in enumerate(taken)]
        for j, expected in enumerate(want):
            assert np.array_equal(got[j].reshape(expected.shape), expected), f"taken[{j}]"
        results.append(np.concatenate(got))
    assert np.array_equal(results[0], results[1]), "two runs differ"


#--------------------------------------------------------------------------------------------------
# shapes x patterns
#--------------------------------------------------------------------------------------------------
def span_rows(n):
    return sc.spans(n)[1] * TILE


def _only(n, rows):
    keep = np.zeros(n, bool)
    keep[np.array([r for r in rows if 0 <= r < n], dtype=np.int64)] = True
    return keep


def _runs(n):
    """kept runs that straddle a wavefront's round, a wavefront's rows, a tile and a span"""
    rows = []
    for boundary in (W, WAVE_ROWS, TILE, span_rows(n), 2 * span_rows(n), n):
        rows += list(range(boundary - 5, boundary + 7))
    return _only(n, rows)


PATTERNS = {
    "all": lambda n: np.ones(n, bool),
    "none": lambda n: np.zeros(n, bool),
    "first": lambda n: _only(n, [0]),
    "last": lambda n: _only(n, [n - 1]),
    "alternating": lambda n: np.arange(n) % 2 == 1,
    "runs": _runs,
    "one_per_span": lambda n: _only(n, [g * span_rows(n) + g * 37 % span_rows(n)
                                        for g in range(sc.spans(n)[0])]),
}
SMALL = [1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1]
# every span gets one tile, and then a second
LARGE = [MAX_SPANS * TILE - 1, MAX_SPANS * TILE, MAX_SPANS * TILE + 1]


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("n", SMALL)
def test_small_shapes(gpu_backend, n, pattern, store_shape):
    """a u8 selector with an i64, a u8 and a 3-byte column at odd addresses, capacity n with the
    zero tail and capacity n + 3 without"""
    rng = np.random.default_rng(n)
    keep = PATTERNS[pattern](n)
    selector = sc.selector_of(keep, 1, 0, rng)
    columns = sc.random_columns(rng, [8, 1, 3], n)
    assert check(gpu_backend, Case(selector, columns, zero_tail=True)) == keep.sum()
    check(gpu_backend, Case(selector, columns, capacity=n + 3))


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("n", LARGE)
def test_every_span(gpu_backend, n, pattern, store_shape):
    """2048 spans of one tile, and one row more: 1025 spans of two tiles, the last one short; a
    u8 selector at a multiple of 16 (read 16 bytes a lane in the count) with an i64 column"""
    rng = np.random.default_rng(n)
    keep = PATTERNS[pattern](n)
    assert sc.spans(n) == ((MAX_SPANS, 1) if n <= MAX_SPANS * TILE else (MAX_SPANS // 2 + 1, 2))
    selector = sc.selector_of(keep, 1, 0)
    columns = sc.random_columns(rng, [8], n)
    capacity = min(n, int(keep.sum()) + 100)
    case = Case(selector, columns, capacity=capacity, zero_tail=True, aligned=True)
    assert check(gpu_backend, case) == keep.sum()


#--------------------------------------------------------------------------------------------------
# selectors
#--------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [False, True])
@pytest.mark.parametrize("width", range(1, 9))
def test_selector_widths(gpu_backend, width, aligned, store_shape):
    """every selector width at an odd address (byte by byte) and at a multiple of 16 (one load a
    row for 1, 2, 4 and 8 bytes; 16 bytes a lane in the count for 1 and 2), with reject 0, all ones
    and a middle value, kept and rejected rows; n is no multiple of 16 and more than one span"""
    rng = np.random.default_rng(width)
    n = 3 * TILE + 37
    ones = (1 << (8 * width)) - 1
    for reject, invert in ((0, False), (ones, False), (0x8081828384858687 & ones, True)):
        selector = sc.selector_of(rng.integers(0, 2, n).astype(bool), width, reject, rng)
        columns = sc.random_columns(rng, [8], n)
        count = check(gpu_backend, Case(selector, columns, reject, invert, aligned=aligned))
        assert 0 < count < n
    assert check(gpu_backend, Case(selector, [], reject=2**64 - 1 if width < 8 else 1)) > n - 20


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 7, 8, 3 * TILE + 37])
@pytest.mark.parametrize("skew", [2, 6, 14])
@pytest.mark.parametrize("width", [1, 2])
def test_selector_head_before_the_whole_pieces(gpu_backend, width, skew, n):
    """a 1- or 2-byte selector at its own alignment but `skew` bytes behind a multiple of 16: the
    count reads 16 bytes a lane, and the rows before the first whole 16 bytes of every span (7, 5
    and 1 two-byte rows) go the general way; with 3 and 7 rows the head is the span or all but
    its last row"""
    rng = np.random.default_rng(100 * width + skew + n)
    selector = sc.selector_of(rng.integers(0, 2, n).astype(bool), width, 0, rng)
    columns = sc.random_columns(rng, [8], n)
    case = Case(selector, columns, zero_tail=True, skews=[skew, 0])
    assert case.layout.at[0] % 16 == skew
    check(gpu_backend, case)


#--------------------------------------------------------------------------------------------------
# columns
#--------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [False, True])
def test_column_widths(gpu_backend, aligned, store_shape):
    """widths 1, 2, 3, 8, 16, 31 and 32 at odd addresses (copied byte by byte) and at multiples of
    16 (in pieces of up to 16 bytes); one column ends inside the second tile, one has no rows"""
    rng = np.random.default_rng(3)
    n = 2 * TILE + 100
    widths = [1, 2, 3, 8, 16, 31, 32, 8, 32]
    rows = [n] * 7 + [TILE + 300, 0]
    selector = sc.selector_of(rng.integers(0, 3, n) != 0, 1, 0, rng)
    columns = sc.random_columns(rng, widths, rows)
    for zero_tail in (False, True):
        check(gpu_backend, Case(selector, columns, capacity=n, zero_tail=zero_tail,
                                aligned=aligned))


@pytest.mark.gpu
def test_sixteen_columns(gpu_backend, store_shape):
    rng = np.random.default_rng(4)
    n = TILE + 77
    widths = [8, 32, 1, 4, 16, 2, 31, 8, 3, 5, 12, 24, 32, 7, 8, 1]
    rows = [n - 3 * (j % 4) for j in range(16)]
    selector = sc.selector_of(rng.integers(0, 2, n).astype(bool), 4, 0xFFFFFFFF, rng)
    columns = sc.random_columns(rng, widths, rows)
    check(gpu_backend, Case(selector, columns, 0xFFFFFFFF, zero_tail=True, capacity=n))
    check(gpu_backend, Case(selector, columns, 0xFFFFFFFF, invert=True, aligned=True))


#--------------------------------------------------------------------------------------------------
# capacity and the outputs asked for
#--------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("zero_tail", [False, True])
@pytest.mark.parametrize("capacity", [0, 1, 40, TILE - 1, TILE, TILE + 300, 2 * TILE,
                                      3 * TILE + 5, 3 * TILE + 6, 5 * TILE + 9])
def test_capacities(gpu_backend, capacity, zero_tail, store_shape):
    """every row kept, so rank = row: the capacity cuts inside a wavefront, inside a tile, exactly
    at a span boundary, at count, and lies above n; count stays exact"""
    rng = np.random.default_rng(capacity)
    n = 3 * TILE + 5
    selector = sc.selector_of(np.ones(n, bool), 2, 0xFFFF, rng)
    columns = sc.random_columns(rng, [8, 3], [n, n - 50])
    assert check(gpu_backend, Case(selector, columns, 0xFFFF, capacity=capacity,
                                   zero_tail=zero_tail)) == n
    half = sc.selector_of(np.arange(n) % 2 == 0, 2, 0xFFFF, rng)
    check(gpu_backend, Case(half, columns, 0xFFFF, capacity=capacity, zero_tail=zero_tail))


@pytest.mark.gpu
def test_outputs_asked_for(gpu_backend, store_shape):
    """count alone, indices alone, columns alone; n = 0 with the tail"""
    rng = np.random.default_rng(9)
    n = TILE + 9
    selector = sc.selector_of(rng.integers(0, 2, n).astype(bool), 8, 0, rng)
    columns = sc.random_columns(rng, [8], n)
    check(gpu_backend, Case(selector, [], want_indices=False))
    check(gpu_backend, Case(selector, [], want_count=False))
    check(gpu_backend, Case(selector, columns, want_count=False, want_indices=False))
    empty = np.zeros((0, 1), np.uint8)
    for zero_tail in (False, True):
        assert check(gpu_backend, Case(empty, [np.zeros((0, 8), np.uint8)], capacity=300,
                                       zero_tail=zero_tail)) == 0


#--------------------------------------------------------------------------------------------------
# the gather
#--------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [False, True])
def test_take_rows(gpu_backend, aligned):
    """sorted and random indices, repeated ones, indices at a column's end and 0xFFFFFFFF, against
    columns of different lengths and every kind of width; more than one workgroup, and one row"""
    rng = np.random.default_rng(10)
    columns = sc.random_columns(rng, [8, 1, 32, 31, 4, 16, 2],
                                [5000, 2000, 3500, 5000, 0, 4999, 5000])
    scattered = rng.integers(0, 5200, 3 * TILE + 11)
    scattered[:8] = [0, 4999, 5000, 2000, 1999, sc.NO_ROW, 7, 7]
    check_take(gpu_backend, scattered, columns, aligned)
    check_take(gpu_backend, np.sort(scattered), columns, aligned)
    check_take(gpu_backend, [3], columns[:1], aligned)


#--------------------------------------------------------------------------------------------------
# host forms on the gpu backend
#--------------------------------------------------------------------------------------------------
CPU_CHILD = """
import sys
import numpy as np
from blitzar_amd import api
assert api.init(api.SXT_CPU_BACKEND, 0) == 0
data = np.load(sys.argv[1])
out = {}
for name, capacity, zero_tail in (("a", None, False), ("b", 5000, True), ("c", 100, False)):
    count, indices, selected = api.select_rows(data["selector"], [data["amounts"], data["rows"]],
                                               reject=3, capacity=capacity, zero_tail=zero_tail)
    out.update({name + "_count": count, name + "_indices": indices, name + "_0": selected[0],
                name + "_1": selected[1]})
taken = api.take_rows(data["indices"], [data["amounts"], data["rows"]])
np.savez(sys.argv[2], taken_0=taken[0], taken_1=taken[1], **out)
"""


@pytest.mark.gpu
def test_host_forms_on_gpu_equal_the_cpu_backend(gpu_backend, tmp_path):
    """bzamd_select_rows and bzamd_take_rows on the gpu backend against the cpu backend in a child
    process, and against the model through tests/test_select_rows.py's checked calls (canaries in
    the unwritten tail included)"""
    from tests.test_select_rows import select_rows, take_rows
    rng = np.random.default_rng(11)
    n = 3 * TILE + 50
    selector = rng.integers(0, 5, n).astype(np.uint16)
    amounts = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
    rows = rng.integers(0, 256, (n - 70, 32), dtype=np.uint8)
    indices = rng.integers(0, n + 10, 2000).astype(np.uint32)
    np.savez(tmp_path / "in.npz", selector=selector, amounts=amounts, rows=rows, indices=indices)
    subprocess.run([sys.executable, "-c", CPU_CHILD, str(tmp_path / "in.npz"),
                    str(tmp_path / "out.npz")], cwd=ROOT, check=True, timeout=120)
    cpu = np.load(tmp_path / "out.npz")
    for name, capacity, zero_tail in (("a", None, False), ("b", 5000, True), ("c", 100, False)):
        before = _launches()
        count, got_indices, selected = gpu_backend.select_rows(
            selector, [amounts, rows], reject=3, capacity=capacity, zero_tail=zero_tail)
        assert _launches() - before == SELECT, "no kernel ran"
        assert count == int(cpu[name + "_count"]) and 0 < count < n
        assert np.array_equal(got_indices, cpu[name + "_indices"])
        assert np.array_equal(selected[0], cpu[name + "_0"])
        assert np.array_equal(selected[1], cpu[name + "_1"])
    before = _launches()
    taken = gpu_backend.take_rows(indices, [amounts, rows])
    assert _launches() - before == TAKE, "no kernel ran"
    assert np.array_equal(taken[0], cpu["taken_0"]) and np.array_equal(taken[1], cpu["taken_1"])
    as_bytes = [selector.view(np.uint8).reshape(n, 2), amounts.view(np.uint8).reshape(n, 8), rows]
    for capacity, zero_tail in ((None, False), (n + 9, True), (100, False), (0, True)):
        select_rows(gpu_backend, as_bytes[0], as_bytes[1:], 3, capacity=capacity,
                    zero_tail=zero_tail)
    select_rows(gpu_backend, as_bytes[0], [], 3, want_indices=False)
    select_rows(gpu_backend, np.zeros((0, 1), np.uint8), [np.zeros((0, 8), np.uint8)], capacity=7,
                zero_tail=True)
    take_rows(gpu_backend, indices, as_bytes[1:])


#--------------------------------------------------------------------------------------------------
# three chains on one stream, no synchronise between the calls
#--------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_where_on_one_stream(gpu_backend):
    """an i64 column filtered by a u8 column with the zero tail, committed over `capacity` rows:
    the commitment of the model's filtered column through the host path"""
    import torch
    dev = _device()
    rng = np.random.default_rng(12)
    n = 3000
    flags = (rng.integers(0, 3, n) == 0).astype(np.uint8)
    amounts = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
    d_flags, d_amounts = _up(flags), _up(amounts.view(np.uint8))
    selected = torch.full((8 * n,), CANARY, dtype=torch.uint8, device=dev)
    count = torch.full((1,), -1, dtype=torch.int64, device=dev)
    need = gpu_backend.select_rows_workspace_bytes(n)
    workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    generators = api.get_generators(n)
    d_generators = _up(generators.view(np.uint8))
    commitment = torch.zeros((1, 32), dtype=torch.uint8, device=dev)
    D = api.sxt_sequence_descriptor
    column = (D * 1)(D(8, n, selected.data_ptr(), 1))
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    gpu_backend.select_rows_device(count.data_ptr(), None, (d_flags.data_ptr(), n, 1, False),
                                   [(d_amounts.data_ptr(), n, 8, True)], [selected.data_ptr()], n,
                                   workspace.data_ptr(), need, zero_tail=True,
                                   stream=side.cuda_stream)
    api.load().bzamd_msm_device(0, commitment.data_ptr(), 1, column, d_generators.data_ptr(),
                                side.cuda_stream)
    side.synchronize()
    filtered = amounts[flags != 0]
    assert int(count[0]) == len(filtered) and 0 < len(filtered) < n
    got = selected.cpu().numpy().view(np.int64)
    assert np.array_equal(got[:len(filtered)], filtered) and np.all(got[len(filtered):] == 0)
    want = gpu_backend.compute_pedersen_commitments(0, [(filtered, True)], generators=generators)
    assert commitment.cpu().numpy().any()
    assert np.array_equal(commitment.cpu().numpy(), want)


@pytest.mark.gpu
def test_distinct_keys_on_one_stream(gpu_backend):
    """the multiplicities of the key column against itself are non-zero at first occurrences:
    selecting the keys by them gives the distinct keys in first-appearance order, and that table
    (zero tail and all) serves bzamd_sum_by_key_device: no misses, the counts sum to n"""
    import torch
    field_id, dev = 0, _device()
    rng = np.random.default_rng(13)
    n, capacity = 3000, 256
    pool = rng.choice(np.arange(1, 10**6, dtype=np.int64), 200, replace=False)
    keys = pool[rng.integers(0, 200, n)]
    _, first = np.unique(keys, return_index=True)
    distinct = keys[np.sort(first)]
    d_keys = _up(keys.view(np.uint8))
    firsts = torch.zeros(n, dtype=torch.int64, device=dev)
    table = torch.full((8 * capacity,), CANARY, dtype=torch.uint8, device=dev)
    counts = torch.zeros(capacity, dtype=torch.int64, device=dev)
    scalars = torch.zeros((3, 8), dtype=torch.int64, device=dev)   # count, misses of both calls
    need = max(gpu_backend.count_multiplicities_workspace_bytes(n),
               gpu_backend.select_rows_workspace_bytes(n),
               gpu_backend.sum_by_key_workspace_bytes(capacity, 0))
    workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    key_column = (d_keys.data_ptr(), n, 8, True)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    gpu_backend.count_multiplicities_device(field_id, firsts.data_ptr(), scalars[1].data_ptr(),
                                            key_column, key_column, workspace.data_ptr(), need,
                                            stream=side.cuda_stream)
    gpu_backend.select_rows_device(scalars[0].data_ptr(), None, (firsts.data_ptr(), n, 8, False),
                                   [key_column], [table.data_ptr()], capacity,
                                   workspace.data_ptr(), need, zero_tail=True,
                                   stream=side.cuda_stream)
    gpu_backend.sum_by_key_device(field_id, None, None, counts.data_ptr(), scalars[2].data_ptr(),
                                  None, (table.data_ptr(), capacity, 8, True), key_column, [],
                                  workspace.data_ptr(), need, stream=side.cuda_stream)
    side.synchronize()
    got = table.cpu().numpy().view(np.int64)
    number = int(scalars[0][0])
    assert number == len(distinct) == 200
    assert np.array_equal(got[:number], distinct) and np.all(got[number:] == 0)
    assert int(scalars[1][0]) == 0 and int(scalars[2][0]) == 0
    per_key = counts.cpu().numpy()
    assert per_key.sum() == n and np.all(per_key[number:] == 0)
    assert np.array_equal(per_key[:number], [(keys == k).sum() for k in distinct])


@pytest.mark.gpu
@pytest.mark.parametrize("invert", [False, True])
def test_join_on_one_stream(gpu_backend, invert, store_shape):
    """matches from bzamd_sum_by_key_device; the lookup side's columns and the matches themselves
    selected by reject = 0xFFFFFFFF; the table's columns taken at the compacted matches: both
    sides equal the model's inner join row for row.  invert: the anti-join, the lookup rows that
    hit nothing"""
    import torch
    field_id, dev = 0, _device()
    rng = np.random.default_rng(14)
    m, n = 300, 2000
    pool = rng.choice(np.arange(1, 10**6, dtype=np.int64), m + 60, replace=False)
    table_keys = pool[:m]
    payload = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    lookup_keys = pool[rng.integers(0, m + 60, n)]           # the last 60 are in no table row
    amounts = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
    row_of = {int(k): t for t, k in enumerate(table_keys)}
    hits = np.array([int(k) in row_of for k in lookup_keys])
    kept = np.flatnonzero(hits != invert)
    hit_rows = np.array([row_of[int(k)] for k in lookup_keys[hits]], dtype=np.int64)
    assert 0 < len(kept) < n
    d_table, d_payload = _up(table_keys.view(np.uint8)), _up(payload)
    d_lookups, d_amounts = _up(lookup_keys.view(np.uint8)), _up(amounts.view(np.uint8))
    matches = torch.zeros(n, dtype=torch.int32, device=dev)
    left_amounts = torch.full((8 * n,), CANARY, dtype=torch.uint8, device=dev)
    left_keys = torch.full((8 * n,), CANARY, dtype=torch.uint8, device=dev)
    compacted = torch.full((4 * n,), CANARY, dtype=torch.uint8, device=dev)
    rows = torch.full((4 * n,), CANARY, dtype=torch.uint8, device=dev)
    right_payload = torch.full((32 * n,), CANARY, dtype=torch.uint8, device=dev)
    right_keys = torch.full((8 * n,), CANARY, dtype=torch.uint8, device=dev)
    count = torch.full((1,), -1, dtype=torch.int64, device=dev)
    need = max(gpu_backend.sum_by_key_workspace_bytes(m, 0),
               gpu_backend.select_rows_workspace_bytes(n))
    workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    before = _launches()
    gpu_backend.sum_by_key_device(field_id, None, None, None, None, matches.data_ptr(),
                                  (d_table.data_ptr(), m, 8, True),
                                  (d_lookups.data_ptr(), n, 8, True), [], workspace.data_ptr(),
                                  need, stream=side.cuda_stream)
    gpu_backend.select_rows_device(
        count.data_ptr(), rows.data_ptr(), (matches.data_ptr(), n, 4, False),
        [(d_amounts.data_ptr(), n, 8, True), (d_lookups.data_ptr(), n, 8, True),
         (matches.data_ptr(), n, 4, False)],
        [left_amounts.data_ptr(), left_keys.data_ptr(), compacted.data_ptr()], n,
        workspace.data_ptr(), need, reject=sc.NO_ROW, invert=invert, zero_tail=True,
        stream=side.cuda_stream)
    gpu_backend.take_rows_device(compacted.data_ptr(), n,
                                 [(d_payload.data_ptr(), m, 32, False),
                                  (d_table.data_ptr(), m, 8, True)],
                                 [right_payload.data_ptr(), right_keys.data_ptr()],
                                 stream=side.cuda_stream)
    assert _launches() - before == 4 + SELECT + TAKE
    side.synchronize()
    number = int(count[0])
    assert number == len(kept)
    assert np.array_equal(rows.cpu().numpy().view(np.uint32)[:number], kept)
    assert np.all(rows.cpu().numpy().view(np.uint32)[number:] == sc.NO_ROW)
    got_amounts = left_amounts.cpu().numpy().view(np.int64)
    got_left_keys = left_keys.cpu().numpy().view(np.int64)
    assert np.array_equal(got_amounts[:number], amounts[kept]) and np.all(got_amounts[number:] == 0)
    assert np.array_equal(got_left_keys[:number], lookup_keys[kept])
    got_matches = compacted.cpu().numpy().view(np.uint32)
    got_payload = right_payload.cpu().numpy().reshape(n, 32)
    got_right_keys = right_keys.cpu().numpy().view(np.int64)
    if invert:
        # every kept row is a miss: 0xFFFFFFFF takes zero bytes
        assert np.all(got_matches[:number] == sc.NO_ROW)
        assert np.all(got_payload[:number] == 0) and np.all(got_right_keys[:number] == 0)
    else:
        assert np.array_equal(got_matches[:number], hit_rows)
        assert np.array_equal(got_payload[:number], payload[hit_rows])
        assert np.array_equal(got_right_keys[:number], got_left_keys[:number])
    # the tail of a column output is zero bytes, which as an index is row 0 of the table
    assert np.all(got_matches[number:] == 0)
    assert np.all(got_payload[number:] == payload[0])
