"""The multiplicity column of a log-derivative argument (include/blitzar_amd.h:
bzamd_count_multiplicities), host form on the host backend, with the workspace size, the first-slot
diagnostic, the aborts and the kernels' resources.

Every expected value is Python integers (tests/multiplicity_cases.py).  The sequential model alone
is in tests/test_multiplicities_host.py, the device form in tests/test_multiplicities_device.py."""
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
from tests import multiplicity_cases as mc
from tests.test_sumcheck_device import MODULUS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0x5A


def count(lib_api, field_id, table, lookups, table_rows=None, want_misses=True):
    """bzamd_count_multiplicities through ctypes on the columns where they lie.  table: an (array,
    signed) pair or None (the range table of table_rows rows) -> (multiplicities, misses or None),
    with the word behind `multiplicities`, the words around `misses` and the inputs checked"""
    if table is None:
        table_desc, m = api.sxt_sequence_descriptor(8, table_rows, None, 0), table_rows
    else:
        descs, keep_table = api.make_descriptors([table])
        table_desc, m = descs[0], table[0].shape[0]
    descs, keep_lookups = api.make_descriptors([lookups])
    before = [np.array(c[0], copy=True) for c in (table, lookups) if c is not None]
    out = np.full(m + 1, 0x5A5A5A5A5A5A5A5A, np.uint64)
    misses = np.full(3, 0x5A5A5A5A5A5A5A5A, np.uint64)
    c = api.bzamd_multiplicity_count(table_desc, descs[0])
    lib_api.load().bzamd_count_multiplicities(
        api._ptr(out), misses[1:].ctypes.data if want_misses else None, field_id, ctypes.byref(c))
    assert out[m] == 0x5A5A5A5A5A5A5A5A, "the word behind `multiplicities` was written"
    assert misses[0] == misses[2] == 0x5A5A5A5A5A5A5A5A, "a word beside `misses` was written"
    assert want_misses or misses[1] == 0x5A5A5A5A5A5A5A5A
    for column, kept in zip([c for c in (table, lookups) if c is not None], before):
        assert np.array_equal(column[0], kept), "a column was modified"
    return out[:m], int(misses[1]) if want_misses else None


def check(lib_api, case):
    for want_misses in (True, False):
        got, misses = count(lib_api, case.field_id, case.table, case.lookups, case.m, want_misses)
        assert np.array_equal(got, case.want_multiplicities())
        assert misses == (case.want[1] if want_misses else None)


def drawn_values(field_id, rng, count_, kind_a, kind_b):
    """values both kinds can hold (so that rows of either side can be equal), negative ones when
    both are signed or 32 bytes wide"""
    (wa, sa), (wb, sb) = kind_a, kind_b
    bits = 8 * min(wa, wb) - (1 if (sa and wa < 32) or (sb and wb < 32) else 0)
    bits = min(bits, 250)
    values = [int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little")
              % (1 << bits) for _ in range(count_)]
    values[0], values[1] = 0, (1 << bits) - 1
    if (sa or wa == 32) and (sb or wb == 32):
        values[2], values[3] = -1, -(1 << (bits - 1)) if bits < 250 else -12345
    return values


def column_of(field_id, values, kind):
    width, signed = kind
    if width == 32:
        return (mc.rows_of(field_id, [v % MODULUS[field_id] for v in values], 32), False)
    return (mc.rows_of(field_id, values, width, signed), signed)


#--------------------------------------------------------------------------------------------------
# host form against the model
#--------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("lookup_kind", mc.KINDS)
@pytest.mark.parametrize("table_kind", mc.KINDS)
def test_host_form(cpu_backend, field_id, table_kind, lookup_kind):
    """every width on either side, the extremes both can hold among the values: a table with
    duplicates, lookups that hit and lookups that miss"""
    rng = np.random.default_rng(100 * table_kind[0] + lookup_kind[0] + field_id)
    shared = drawn_values(field_id, rng, 24, table_kind, lookup_kind)
    table_values = shared[:16] + shared[3:9]           # six duplicates behind the first occurrences
    lookup_values = [shared[int(i)] for i in rng.integers(0, 24, 200)]  # 16 .. 23: misses
    case = mc.Case(field_id, column_of(field_id, table_values, table_kind),
                   column_of(field_id, lookup_values, lookup_kind))
    assert case.want[1] > 0 and sum(case.want[0]) > 0
    assert all(x == 0 for x in case.want[0][16:])
    check(cpu_backend, case)


@pytest.mark.parametrize("field_id", [0, 1])
def test_equal_keys_across_kinds(cpu_backend, field_id):
    """an i8 -1, an i64 -1 and the 32-byte p - 1 are one key; x and x + p are one key; in field 1 a
    32-byte row and a narrow row compare by value"""
    p = MODULUS[field_id]
    minus_one_32 = mc.rows_of(field_id, [p - 1], 32)
    i8, i64 = np.array([-1, 5], np.int8), np.array([7, -1], np.int64)
    for table, lookups, want in [
            ((i8.view(np.uint8).reshape(2, 1), True), (i64.view(np.uint8).reshape(2, 8), True), [1, 0]),
            ((i64.view(np.uint8).reshape(2, 8), True), (minus_one_32, False), [0, 1]),
            ((minus_one_32, False), (i8.view(np.uint8).reshape(2, 1), True), [1])]:
        got, misses = count(cpu_backend, field_id, table, lookups)
        assert got.tolist() == want and misses == lookups[0].shape[0] - 1
    # x and x + p (raw 32 bytes; what they mean is the same value)
    x = 123456789
    raw = cic.element_raw(field_id, x)
    assert raw + p < 1 << 256
    table = (mc.rows_of(field_id, [raw + p, raw], 32, raw=True), False)
    lookups = (mc.rows_of(field_id, [raw, raw + p, raw + 1], 32, raw=True), False)
    got, misses = count(cpu_backend, field_id, table, lookups)
    assert got.tolist() == [2, 0] and misses == 1
    # the element against the narrow integer of its value
    narrow = (np.array([x, x + 5], np.uint32).view(np.uint8).reshape(2, 4), False)
    got, misses = count(cpu_backend, field_id, narrow, lookups)
    assert got.tolist() == [2, 0] and misses == 1
    # the largest 32 bytes
    top = (1 << 256) - 1
    table = (mc.rows_of(field_id, [top, 0], 32, raw=True), False)
    value = cic.raw_value(field_id, top)
    lookups = (mc.rows_of(field_id, [value, 0, value], 32), False)
    got, misses = count(cpu_backend, field_id, table, lookups)
    assert got.tolist() == [2, 1] and misses == 0


@pytest.mark.parametrize("field_id", [0, 1])
def test_all_equal_table_and_no_lookups(cpu_backend, field_id):
    table = (np.full(37, -3, np.int16).view(np.uint8).reshape(37, 2), True)
    lookups = (np.array([-3, 3, -3, -3], np.int64).view(np.uint8).reshape(4, 8), True)
    got, misses = count(cpu_backend, field_id, table, lookups)
    assert got.tolist() == [3] + [0] * 36 and misses == 1
    for empty in ((np.zeros((0, 8), np.uint8), True), (np.zeros((0, 32), np.uint8), False)):
        got, misses = count(cpu_backend, field_id, table, empty)
        assert not got.any() and misses == 0
        got, misses = count(cpu_backend, field_id, None, empty, table_rows=5)
        assert got.tolist() == [0] * 5 and misses == 0


@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("m", [1, 2, 256, 1000])
def test_range_table(cpu_backend, field_id, m):
    """values at m - 1 and m, negative ones and 32-byte keys with a high word set"""
    p = MODULUS[field_id]
    rng = np.random.default_rng(m)
    values = [int(v) for v in rng.integers(0, m + max(m // 4, 2), 300)] + [m - 1, m, 0]
    for kind in [(2, False), (8, True), (32, False)]:
        mine = list(values)
        if kind != (2, False):
            mine += [-1, -m]
        if kind[0] == 32:
            mine += [1 << 64, (1 << 192) + 1, p - 1]
        case = mc.Case(field_id, None, column_of(field_id, mine, kind), table_rows=m)
        assert case.want[0][m - 1] >= 1 and case.want[1] >= 1
        check(cpu_backend, case)
    # unreduced: m - 1 + p hits row m - 1
    raw = [cic.element_raw(field_id, m - 1) + p, cic.element_raw(field_id, m)]
    got, misses = count(cpu_backend, field_id, None, (mc.rows_of(field_id, raw, 32, raw=True), False),
                        table_rows=m)
    assert got.tolist() == [0] * (m - 1) + [1] and misses == 1


@pytest.mark.parametrize("field_id", [0, 1])
def test_wrapper(cpu_backend, field_id):
    table = np.array([5, -7, 5, 9], np.int64)
    lookups = np.array([5, 5, -7, 1, 9, 9, 9], np.int16)
    got, misses = cpu_backend.count_multiplicities(field_id, table, lookups)
    assert got.dtype == np.uint64 and got.tolist() == [2, 1, 0, 3] and misses == 1
    only = cpu_backend.count_multiplicities(field_id, table, lookups, want_misses=False)
    assert only.tolist() == [2, 1, 0, 3]
    got, misses = cpu_backend.count_multiplicities(field_id, (None, 6), lookups)
    assert got.tolist() == [0, 1, 0, 0, 0, 2] and misses == 4


#--------------------------------------------------------------------------------------------------
# the workspace and the first slot: no backend
#--------------------------------------------------------------------------------------------------
def test_workspace_bytes():
    api.reset_for_testing()
    want = {0: 0, 1: 4 * 2 + 256, 2: 4 * 4 + 256, 3: 4 * 8 + 256, 2**28: 4 * 2**29 + 256,
            2**28 + 1: 0}
    for m, size in want.items():
        assert api.count_multiplicities_workspace_bytes(m) == size, m


@pytest.mark.parametrize("field_id", [0, 1])
def test_first_slot(field_id):
    api.reset_for_testing()
    p = MODULUS[field_id]
    rng = np.random.default_rng(5)
    none = (1 << 64) - 1
    for m in (1, 2, 3, 64, 1000, 2**28):
        slots = mc.slots(m)
        for _ in range(20):
            x = int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % p
            if x + p >= 1 << 256:
                continue
            first = api.multiplicity_first_slot(field_id, mc.rows_of(field_id, [x], 32, raw=True)[0], m)
            assert first < slots
            assert first == api.multiplicity_first_slot(
                field_id, mc.rows_of(field_id, [x + p], 32, raw=True)[0], m)
    element = mc.rows_of(field_id, [1], 32)[0]
    assert api.multiplicity_first_slot(field_id, element, 0) == none
    assert api.multiplicity_first_slot(field_id, element, 2**28 + 1) == none
    assert api.multiplicity_first_slot(2, element, 8) == none
    # small consecutive integers spread: 256 of them start at more than 128 of 512 slots
    starts = {api.multiplicity_first_slot(field_id, mc.rows_of(field_id, [x], 32)[0], 256)
              for x in range(256)}
    assert len(starts) > 128


#--------------------------------------------------------------------------------------------------
# aborts (host backend only; each in a child process)
#--------------------------------------------------------------------------------------------------
SETUP = ("lib = api.load()\n"
         "tab = np.arange(8, dtype=np.int64); look = np.arange(16, dtype=np.int64)\n"
         "out = np.zeros(16, np.uint64); mis = np.zeros(4, np.uint64)\n"
         "work = np.zeros(1024, np.uint8)\n"
         "T, L, O, M, W = (a.ctypes.data for a in (tab, look, out, mis, work))\n"
         "D = api.sxt_sequence_descriptor\n"
         "def call(multiplicities, misses, table, lookups, field=0):\n"
         "    c = api.bzamd_multiplicity_count(D(*table), D(*lookups))\n"
         "    lib.bzamd_count_multiplicities(multiplicities, misses, field, ctypes.byref(c))\n"
         "def device(multiplicities, misses, table, lookups, workspace, workspace_bytes):\n"
         "    api.count_multiplicities_device(0, multiplicities, misses, table, lookups, workspace,\n"
         "                                    workspace_bytes)\n"
         "tab8, look16 = (8, 8, T, 1), (8, 16, L, 1)\n")
ABORTS = {
    "null_c": ("lib.bzamd_count_multiplicities(O, M, 0, None)\n",
               "null argument to `bzamd_count_multiplicities`"),
    "null_multiplicities": ("call(None, M, tab8, look16)\n",
                            "null argument to `bzamd_count_multiplicities`"),
    "table_width_33": ("call(O, M, (33, 8, T, 0), look16)\n", "element_nbytes must be in [1, 32]"),
    "lookups_width_0": ("call(O, M, tab8, (0, 16, L, 0))\n", "element_nbytes must be in [1, 32]"),
    "lookups_signed_17": ("call(O, M, tab8, (17, 4, L, 1))\n",
                          "signed sequences need element_nbytes <= 16"),
    "lookups_null_data": ("call(O, M, tab8, (8, 16, None, 1))\n",
                          "descriptor has n > 0 but null data"),
    "range_table_width_4": ("call(O, M, (4, 8, None, 0), look16)\n",
                            "a NULL table is the range table"),
    "range_table_signed": ("call(O, M, (8, 8, None, 1), look16)\n",
                           "a NULL table is the range table"),
    "range_table_0_rows": ("call(O, M, (8, 0, None, 0), look16)\n",
                           "needs 1 <= table rows <= 2^28"),
    "table_0_rows": ("call(O, M, (8, 0, T, 1), look16)\n", "needs 1 <= table rows <= 2^28"),
    "table_above_2_pow_28": ("call(O, M, (8, 2**28 + 1, None, 0), look16)\n",
                             "needs 1 <= table rows <= 2^28"),
    "lookups_above_2_pow_30": ("call(O, M, tab8, (1, 2**30 + 1, L, 0))\n",
                               "needs lookup rows <= 2^30"),
    "misaligned_multiplicities": ("call(O + 4, M, tab8, look16)\n", "must be 8-byte aligned"),
    "misaligned_misses": ("call(O, M + 4, tab8, look16)\n", "must be 8-byte aligned"),
    "multiplicities_overlap_the_table": ("call(T + 56, M, tab8, look16)\n",
                                         "an output overlaps an input"),
    "multiplicities_overlap_the_lookups": ("call(L + 64, M, tab8, look16)\n",
                                           "an output overlaps an input"),
    "misses_overlap_the_lookups": ("call(O, L + 120, tab8, look16)\n",
                                   "an output overlaps an input"),
    "outputs_overlap": ("call(O, O + 56, tab8, look16)\n",
                        "the outputs of the multiplicity count overlap"),
    "field_2": ("call(O, M, tab8, look16, field=2)\n", "unsupported field id"),
    "workspace_too_small": ("device(O, M, (T, 8, 8, True), (L, 16, 8, True), W, 4 * 16 + 255)\n",
                            "the workspace of the multiplicity count is too small"),
    "workspace_null": ("device(O, M, (T, 8, 8, True), (L, 16, 8, True), None, 1024)\n",
                       "the workspace of the multiplicity count is too small"),
    "multiplicities_overlap_the_workspace": (
        "device(W + 320 - 8, M, (T, 8, 8, True), (L, 16, 8, True), W, 320)\n",
        "an output overlaps the workspace"),
    "misses_overlap_the_workspace": (
        "device(O, W + 8, (T, 8, 8, True), (L, 16, 8, True), W, 320)\n",
        "an output overlaps the workspace"),
    "device_form_on_cpu": ("device(O, M, (T, 8, 8, True), (L, 16, 8, True), W, 1024)\n",
                           "device entry points need the GPU backend"),
    "range_device_form_on_cpu": ("device(O, M, (None, 8, 8, False), (L, 16, 8, True), None, 0)\n",
                                 "device entry points need the GPU backend"),
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


# kernel -> instantiations: the clear serves both fields; either count has its LDS and its global
# form
KERNELS = {"k_clear_multiplicities": 1, "k_insert_rows": 2, "k_count_rows": 4, "k_count_range": 4}


@pytest.mark.skipif(_hipcc() is None, reason="hipcc is not installed")
def test_kernels_use_no_scratch(tmp_path):
    """the compiler's own resource report of proof/multiplicities.hip with the flags the library is
    built with: every kernel of the file, both fields"""
    from blitzar_amd import build
    src = "proof/multiplicities.hip"
    assert src in build.SOURCES
    r = subprocess.run([_hipcc(), *build.FLAGS, *build.TU_FLAGS.get(src, []), "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(build.CSRC, src), "-o", str(tmp_path / "multiplicities.o")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    scratch, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name is not None:
            scratch[name] = int(m.group(1))
    print(scratch)
    assert len(scratch) == sum(KERNELS.values()), sorted(scratch)
    for kernel, instantiations in KERNELS.items():
        found = {k: v for k, v in scratch.items() if kernel in k}
        assert len(found) == instantiations, f"{kernel}: found {sorted(found)}"
        assert all(v == 0 for v in found.values()), found
