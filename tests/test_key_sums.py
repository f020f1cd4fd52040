"""Sums of value columns by key (include/blitzar_amd.h: bzamd_sum_by_key), host form on the host
backend, with the workspace size, the aborts and the kernels' resources.

Every expected value is Python integers (tests/key_sum_cases.py).  The plain C++ half of the
device's accumulator scheme is in tests/test_key_sums_host.py, the device form in
tests/test_key_sums_device.py."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from blitzar_amd import api
from tests import column_inverse_cases as cic
from tests import key_sum_cases as kc
from tests import multiplicity_cases as mc
from tests.test_multiplicities import column_of, drawn_values
from tests.test_sumcheck_device import MODULUS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0x5A
OUTPUTS = ("sums", "scalars", "counts", "misses", "matches")


def sum_by_key(lib_api, case, want=OUTPUTS):
    """bzamd_sum_by_key through ctypes on the columns where they lie -> a dict of the outputs in
    `want` (the others are null pointers), with the bytes behind every output, the words around
    `misses` and the inputs checked"""
    m, n, count = case.m, case.n, len(case.values)
    if case.table is None:
        table_desc = api.sxt_sequence_descriptor(8, m, None, 0)
    else:
        descs, keep_table = api.make_descriptors([case.table])
        table_desc = descs[0]
    lookup_descs, keep_lookups = api.make_descriptors([case.lookups])
    value_descs, keep_values = api.make_descriptors(case.values)
    columns = [c for c in (case.table, case.lookups, *case.values) if c is not None]
    before = [np.array(c[0], copy=True) for c in columns]
    sizes = {"sums": 32 * m * count, "scalars": 32 * m * count, "counts": 8 * m, "misses": 8,
             "matches": 4 * n}
    # eight canary bytes before and behind every output
    buffers = {name: np.full(sizes[name] + 16, CANARY, np.uint8) for name in OUTPUTS}
    assert all(b.ctypes.data % 8 == 0 for b in buffers.values())
    pointers = [buffers[name][8:].ctypes.data if name in want else None for name in OUTPUTS]
    k = api.bzamd_key_sums(table_desc, lookup_descs[0], value_descs if count else None, count)
    lib_api.load().bzamd_sum_by_key(*pointers, case.field_id, ctypes.byref(k))
    for name in OUTPUTS:
        body = buffers[name][8:8 + sizes[name]]
        assert np.all(buffers[name][:8] == CANARY) and np.all(buffers[name][8 + sizes[name]:] ==
                                                              CANARY), f"around `{name}`"
        assert name in want or np.all(body == CANARY), f"`{name}` was written"
    for column, kept in zip(columns, before):
        assert np.array_equal(column[0], kept), "a column was modified"
    shaped = {"sums": lambda a: a.reshape(count, m, 32), "scalars": lambda a: a.reshape(count, m, 32),
              "counts": lambda a: a.view(np.uint64), "misses": lambda a: int(a.view(np.uint64)[0]),
              "matches": lambda a: a.view(np.uint32)}
    return {name: shaped[name](buffers[name][8:8 + sizes[name]].copy()) for name in want}


def check(lib_api, case, want=OUTPUTS):
    got = sum_by_key(lib_api, case, want)
    expected = {"sums": case.want_sums, "scalars": case.want_scalars, "counts": case.want_counts,
                "misses": lambda: case.want[1], "matches": case.want_matches}
    for name in want:
        assert np.array_equal(got[name], expected[name]()), name
    return got


#--------------------------------------------------------------------------------------------------
# host form against the model
#--------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("value_kind", mc.KINDS)
@pytest.mark.parametrize("key_kind", mc.KINDS)
def test_host_form(cpu_backend, field_id, key_kind, value_kind):
    """every key kind x value kind: a table with duplicates, lookups that hit and lookups that
    miss, a value column of n rows with the extremes of its kind among them and one shorter than
    n; `counts` is what bzamd_count_multiplicities returns for the same columns"""
    rng = np.random.default_rng(100 * key_kind[0] + value_kind[0] + field_id)
    shared = drawn_values(field_id, rng, 24, key_kind, key_kind)
    table_values = shared[:16] + shared[3:9]           # six duplicates behind the first occurrences
    lookup_values = [shared[int(i)] for i in rng.integers(0, 24, 200)]  # 16 .. 23: misses
    values = [kc.column(field_id, kc.drawn(rng, value_kind, 200), value_kind),
              kc.column(field_id, kc.drawn(rng, value_kind, 131), value_kind)]
    case = kc.Case(field_id, column_of(field_id, table_values, key_kind),
                   column_of(field_id, lookup_values, key_kind), values)
    assert case.want[1] > 0 and sum(case.want[0]) > 0
    assert all(x == 0 for row in case.sums for x in row[16:])
    got = check(cpu_backend, case)
    multiplicities, misses = cpu_backend.count_multiplicities(field_id, case.table, case.lookups)
    assert np.array_equal(got["counts"], multiplicities) and got["misses"] == misses


@pytest.mark.parametrize("field_id", [0, 1])
def test_unreduced_and_montgomery_rows(cpu_backend, field_id):
    """32-byte values as raw bytes: x and x + p are one value, the largest 32 bytes are a value,
    and in field 1 the bytes are Montgomery words: the sum of rows of a known value is that value
    times the count"""
    p = MODULUS[field_id]
    x = 0x1234567890ABCDEF1234567890ABCDEF
    raw = cic.element_raw(field_id, x)
    assert raw + p < 1 << 256
    top = (1 << 256) - 1
    rows = [raw, raw + p, raw, top, raw + p]
    keys = [7, 7, 9, 9, 7]
    case = kc.Case(field_id, kc.i64_column([9, 7]), kc.i64_column(keys),
                   [(mc.rows_of(field_id, rows, 32, raw=True), False)])
    assert case.sums[0] == [(x + cic.raw_value(field_id, top)) % p, 3 * x % p]
    check(cpu_backend, case)


@pytest.mark.parametrize("field_id", [0, 1])
def test_sums_that_wrap_the_modulus(cpu_backend, field_id):
    """300 rows of p - 1 on one key and 200 of 2^248 - 1: the sums pass p many times"""
    p = MODULUS[field_id]
    n = 500
    keys = [3] * 300 + [4] * 200
    wide = [p - 1] * 300 + [p - 2] * 200
    narrow = [(1 << 248) - 1] * n
    case = kc.Case(field_id, kc.i64_column([4, 3, 5]), kc.i64_column(keys),
                   [kc.column(field_id, wide, (32, False)), kc.column(field_id, narrow, (31, False))])
    assert case.sums[0] == [(-400) % p, (-300) % p, 0]
    assert case.sums[1][1] == 300 * ((1 << 248) - 1) % p and 300 * ((1 << 248) - 1) > p
    check(cpu_backend, case)


@pytest.mark.parametrize("field_id", [0, 1])
def test_extremes_and_cancellation(cpu_backend, field_id):
    """all-ones 31-byte rows, the i128 minimum, and positive and negative rows that cancel to zero
    on one key while another keeps a negative sum"""
    p = MODULUS[field_id]
    low, high = kc.extremes((16, True))
    keys = [1, 1, 1, 1, 2, 2]
    i128 = [low, high, 1, low, low, low]
    cancel = [high, -high, low, high, -5, 2]               # key 1: low + high = -1
    ones = [(1 << 248) - 1] * 6
    case = kc.Case(field_id, kc.i64_column([1, 2]), kc.i64_column(keys),
                   [kc.column(field_id, i128, (16, True)), kc.column(field_id, cancel, (16, True)),
                    kc.column(field_id, ones, (31, False)),
                    kc.column(field_id, [5, -5, 7, -7, 0, 0], (1, True))])
    assert case.sums[0] == [(2 * low + high + 1) % p, 2 * low % p]
    assert case.sums[1] == [p - 1, p - 3] and case.sums[3] == [0, 0]
    got = check(cpu_backend, case)
    assert not got["sums"][3].any() and not got["scalars"][3].any()


@pytest.mark.parametrize("field_id", [0, 1])
def test_matches_alone_and_every_output_null_in_turn(cpu_backend, field_id):
    rng = np.random.default_rng(field_id)
    table = [int(v) for v in rng.integers(-50, 50, 40)]
    lookups = [int(v) for v in rng.integers(-60, 60, 300)]
    join = kc.Case(field_id, kc.i64_column(table), kc.i64_column(lookups), [])
    got = check(cpu_backend, join, want=("matches",))
    assert kc.MISS in got["matches"].tolist() and got["matches"].dtype == np.uint32
    check(cpu_backend, join, want=("counts", "misses", "matches"))
    values = [kc.column(field_id, kc.drawn(rng, (8, True), 300), (8, True)),
              kc.column(field_id, kc.drawn(rng, (32, False), 300), (32, False))]
    case = kc.Case(field_id, kc.i64_column(table), kc.i64_column(lookups), values)
    check(cpu_backend, case)
    for missing in OUTPUTS:
        check(cpu_backend, case, want=tuple(name for name in OUTPUTS if name != missing))
    check(cpu_backend, case, want=("scalars",))
    check(cpu_backend, case, want=("sums",))


@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("m", [1, 2, 256, 1000])
def test_range_table(cpu_backend, field_id, m):
    """T[t] = t: values at m - 1 and m, negative keys and 32-byte keys with a high word set miss;
    matches are the keys themselves"""
    p = MODULUS[field_id]
    rng = np.random.default_rng(m)
    keys = [int(v) for v in rng.integers(0, m + max(m // 4, 2), 300)] + [m - 1, m, 0]
    for kind in [(2, False), (8, True), (32, False)]:
        mine = list(keys)
        if kind != (2, False):
            mine += [-1, -m]
        if kind[0] == 32:
            mine += [1 << 64, (1 << 192) + 1, p - 1]
        values = [kc.column(field_id, kc.drawn(rng, (8, True), len(mine)), (8, True))]
        case = kc.Case(field_id, None, column_of(field_id, mine, kind), values, table_rows=m)
        assert case.want[0][m - 1] >= 1 and case.want[1] >= 1
        got = check(cpu_backend, case)
        hits = got["matches"] != kc.MISS
        assert [int(x) for x in got["matches"][hits]] == [k for k in case.lookup_keys if k < m]


@pytest.mark.parametrize("field_id", [0, 1])
def test_no_lookups_and_wrapper(cpu_backend, field_id):
    p = MODULUS[field_id]
    table = np.array([5, -7, 5, 9], np.int64)
    lookups = np.array([5, 5, -7, 1, 9, 9, 9], np.int16)
    price = np.array([10, -20, 30, 40, 50, 60], np.int32)        # shorter than n: row 6 is zero
    got = cpu_backend.sum_by_key(field_id, table, lookups, [price])
    assert got["counts"].tolist() == [2, 1, 0, 3] and got["misses"] == 1
    assert got["matches"].tolist() == [0, 0, 1, kc.MISS, 3, 3, 3]
    from tests.univariate_cases import scalar_values
    assert scalar_values(got["scalars"][0]) == [p - 10, 30, 0, 110]
    assert np.array_equal(got["sums"][0], kc.element_rows(field_id, [-10, 30, 0, 110]))
    only = cpu_backend.sum_by_key(field_id, (None, 6), lookups, [], want=("matches", "counts"))
    assert sorted(only) == ["counts", "matches"]
    assert only["counts"].tolist() == [0, 1, 0, 0, 0, 2]
    assert only["matches"].tolist() == [5, 5, kc.MISS, 1, kc.MISS, kc.MISS, kc.MISS]
    empty = (np.zeros((0, 8), np.uint8), True)
    case = kc.Case(field_id, kc.i64_column([1, 2, 3]), empty, [empty, (np.zeros((0, 32), np.uint8),
                                                                      False)])
    got = check(cpu_backend, case)
    assert not got["sums"].any() and got["misses"] == 0 and got["matches"].size == 0


#--------------------------------------------------------------------------------------------------
# the workspace: no backend
#--------------------------------------------------------------------------------------------------
def test_workspace_bytes():
    api.reset_for_testing()
    for m in (1, 2, 3, 64, 65, 4096, 2**28):
        slots = (4 * mc.slots(m) + 255) // 256 * 256
        for values in range(9):
            assert api.sum_by_key_workspace_bytes(m, values) == slots + 64 * m * values + 256
        assert api.sum_by_key_workspace_bytes(m, 0) >= api.count_multiplicities_workspace_bytes(m)
        assert api.sum_by_key_workspace_bytes(m, 9) == 0
    assert api.sum_by_key_workspace_bytes(0, 1) == 0
    assert api.sum_by_key_workspace_bytes(2**28 + 1, 1) == 0


#--------------------------------------------------------------------------------------------------
# aborts (host backend only; each in a child process)
#--------------------------------------------------------------------------------------------------
SETUP = ("lib = api.load()\n"
         "tab = np.arange(8, dtype=np.int64); look = np.arange(16, dtype=np.int64)\n"
         "val = np.arange(16, dtype=np.int64)\n"
         "sums = np.zeros(64, np.uint64); sca = np.zeros(64, np.uint64)\n"
         "cnt = np.zeros(16, np.uint64); mis = np.zeros(4, np.uint64)\n"
         "mat = np.zeros(32, np.uint32); work = np.zeros(2048, np.uint8)\n"
         "T, L, V, S, C, N, M, X, W = (a.ctypes.data for a in (tab, look, val, sums, sca, cnt, mis,"
         " mat, work))\n"
         "D = api.sxt_sequence_descriptor\n"
         "tab8, look16, val16 = (8, 8, T, 1), (8, 16, L, 1), (8, 16, V, 1)\n"
         "def struct(table, lookups, values):\n"
         "    descs = (D * max(len(values), 1))(*[D(*v) for v in values])\n"
         "    return api.bzamd_key_sums(D(*table), D(*lookups), descs, len(values)), descs\n"
         "def call(outputs, table=tab8, lookups=look16, values=(val16,), field=0):\n"
         "    k, keep = struct(table, lookups, values)\n"
         "    lib.bzamd_sum_by_key(*outputs, field, ctypes.byref(k))\n"
         "def device(outputs, workspace, workspace_bytes, table=tab8, values=(val16,)):\n"
         "    k, keep = struct(table, look16, values)\n"
         "    lib.bzamd_sum_by_key_device(*outputs, 0, ctypes.byref(k), workspace, workspace_bytes,"
         " None)\n"
         "ALL = (S, C, N, M, X)\n"
         "NEED = api.sum_by_key_workspace_bytes(8, 1)\n")
ABORTS = {
    "null_k": ("lib.bzamd_sum_by_key(S, C, N, M, X, 0, None)\n",
               "null argument to `bzamd_sum_by_key`"),
    "null_values": ("k = api.bzamd_key_sums(D(*tab8), D(*look16), None, 1)\n"
                    "lib.bzamd_sum_by_key(S, C, N, M, X, 0, ctypes.byref(k))\n",
                    "null argument to `bzamd_sum_by_key`"),
    "null_k_device": ("lib.bzamd_sum_by_key_device(S, C, N, M, X, 0, None, W, 2048, None)\n",
                      "null argument to `bzamd_sum_by_key_device`"),
    "nine_values": ("call(ALL, values=(val16,) * 9)\n", "need num_values <= 8"),
    "sums_without_values": ("call((S, None, N, M, X), values=())\n",
                            "num_values = 0 need sums and scalars null"),
    "scalars_without_values": ("call((None, C, N, M, X), values=())\n",
                               "num_values = 0 need sums and scalars null"),
    "values_without_sums": ("call((None, None, N, M, X))\n",
                            "num_values >= 1 need sums or scalars"),
    "no_output": ("call((None, None, None, None, None), values=())\n", "need an output"),
    "table_width_33": ("call(ALL, table=(33, 8, T, 0))\n", "element_nbytes must be in [1, 32]"),
    "value_width_0": ("call(ALL, values=((0, 16, V, 0),))\n", "element_nbytes must be in [1, 32]"),
    "value_signed_17": ("call(ALL, values=((17, 4, V, 1),))\n",
                        "signed sequences need element_nbytes <= 16"),
    "value_null_data": ("call(ALL, values=((8, 16, None, 1),))\n",
                        "descriptor has n > 0 but null data"),
    "range_table_width_4": ("call(ALL, table=(4, 8, None, 0))\n", "a NULL table is the range table"),
    "value_longer_than_n": ("call(ALL, values=((4, 17, V, 1),))\n", "is longer than n"),
    "table_0_rows": ("call(ALL, table=(8, 0, T, 1))\n", "need 1 <= table rows <= 2^28"),
    "table_above_2_pow_28": ("call((None, None, N, M, X), table=(8, 2**28 + 1, None, 0), "
                             "values=())\n", "need 1 <= table rows <= 2^28"),
    "lookups_above_2_pow_30": ("call((None, None, N, M, None), lookups=(1, 2**30 + 1, L, 0), "
                               "values=())\n", "need lookup rows <= 2^30"),
    "misaligned_sums": ("call((S + 4, C, N, M, X))\n", "must be 8-byte aligned"),
    "misaligned_scalars": ("call((S, C + 4, N, M, X))\n", "must be 8-byte aligned"),
    "misaligned_counts": ("call((S, C, N + 4, M, X))\n", "must be 8-byte aligned"),
    "misaligned_misses": ("call((S, C, N, M + 4, X))\n", "must be 8-byte aligned"),
    "misaligned_matches": ("call((S, C, N, M, X + 2))\n", "matches must be 4-byte aligned"),
    "sums_overlap_scalars": ("call((S, S + 248, N, M, X))\n",
                             "the outputs of the sums by key overlap"),
    "matches_overlap_counts": ("call((S, C, N, M, N + 56))\n",
                               "the outputs of the sums by key overlap"),
    "sums_overlap_the_table": ("call((T + 56, C, N, M, X))\n", "an output overlaps an input"),
    "matches_overlap_the_lookups": ("call((S, C, N, M, L + 124))\n", "an output overlaps an input"),
    "misses_overlap_a_value_column": ("call((S, C, N, V + 120, X))\n",
                                      "an output overlaps an input"),
    "field_2": ("call(ALL, field=2)\n", "unsupported field id"),
    "workspace_too_small": ("device(ALL, W, NEED - 1)\n",
                            "the workspace of the sums by key is too small"),
    "workspace_null": ("device(ALL, None, 2048)\n",
                       "the workspace of the sums by key is too small"),
    "range_workspace_null_with_values": ("device(ALL, None, 0, table=(8, 8, None, 0))\n",
                                         "the workspace of the sums by key is too small"),
    "counts_overlap_the_workspace": ("device((S, C, W + NEED - 8, M, X), W, NEED)\n",
                                     "an output overlaps the workspace"),
    "device_form_on_cpu": ("device(ALL, W, 2048)\n", "device entry points need the GPU backend"),
    "range_device_form_on_cpu": ("device((None, None, N, M, X), None, 0, table=(8, 8, None, 0), "
                                 "values=())\n", "device entry points need the GPU backend"),
}


@pytest.mark.parametrize("name", sorted(ABORTS))
def test_bad_arguments_abort(name):
    call, message = ABORTS[name]
    code = ("import ctypes\nimport numpy as np\nfrom blitzar_amd import api\n"
            "api.init(api.SXT_CPU_BACKEND, 0)\n" + SETUP + call)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode < 0 and message in r.stderr, r.stderr


#--------------------------------------------------------------------------------------------------
# the kernels' resources
#--------------------------------------------------------------------------------------------------
def _hipcc():
    from blitzar_amd import build
    return build.HIPCC if os.path.exists(build.HIPCC) else shutil.which("hipcc")


# kernel -> instantiations: the clear serves both fields; the accumulation has its hashed and its
# range form, each with its LDS and its global form
KERNELS = {"k_clear_key_sums": 1, "k_insert_rows": 2, "k_accumulate_rows": 8, "k_finish_sums": 2}


@pytest.mark.skipif(_hipcc() is None, reason="hipcc is not installed")
def test_kernels_use_no_scratch(tmp_path):
    """the compiler's own resource report of proof/key_sums.hip with the flags the library is built
    with: every kernel of the file, both fields"""
    from blitzar_amd import build
    src = "proof/key_sums.hip"
    assert src in build.SOURCES
    r = subprocess.run([_hipcc(), *build.FLAGS, *build.TU_FLAGS.get(src, []), "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(build.CSRC, src), "-o", str(tmp_path / "key_sums.o")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    scratch, name = {}, None
    for line in r.stderr.splitlines():
        found = re.search(r"Function Name: (\S+)", line)
        if found:
            name = found.group(1)
        found = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if found and name is not None:
            scratch[name] = int(found.group(1))
    print(scratch)
    assert len(scratch) == sum(KERNELS.values()), sorted(scratch)
    for kernel, instantiations in KERNELS.items():
        found = {k: v for k, v in scratch.items() if kernel in k}
        assert len(found) == instantiations, f"{kernel}: found {sorted(found)}"
        assert all(v == 0 for v in found.values()), found
