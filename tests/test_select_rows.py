"""Selection of rows (include/blitzar_amd.h: bzamd_select_rows, bzamd_take_rows), host forms on
the host backend, with the workspace size, the aborts and the kernels' resources.

Every expected value comes from the model in tests/select_row_cases.py (numpy flatnonzero on the
selector's bits, byte slicing), which a test of its own checks on hand-written cases.  The plain
C++ half of the device form is in tests/test_select_rows_host.py, the device forms in
tests/test_select_rows_device.py."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from blitzar_amd import api
from tests import select_row_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = sc.CANARY


def _buffer(nbytes):
    """eight canary bytes before and behind `nbytes` bytes, the body 8-byte aligned"""
    buffer = np.full(8 + nbytes + 8, CANARY, np.uint8)
    assert buffer.ctypes.data % 8 == 0
    return buffer


def _body(buffer, name):
    assert np.all(buffer[:8] == CANARY), f"before `{name}`"
    assert np.all(buffer[-8:] == CANARY), f"behind `{name}`"
    return buffer[8:-8]


def select_rows(lib_api, selector, columns, reject=0, invert=False, capacity=None,
                zero_tail=False, want_count=True, want_indices=True, signed=False,
                null_outputs=False):
    """bzamd_select_rows through ctypes on the columns where they lie, checked against the model
    byte for byte (what is not written stays CANARY), with the bytes around every output and the
    inputs -> count (None when not asked for)"""
    capacity = len(selector) if capacity is None else capacity
    selector_descs, keep_selector = api.make_descriptors([(selector, signed)])
    descs, keep = api.make_descriptors([(c, False) for c in columns])
    before = [np.array(a, copy=True) for a in (selector, *columns)]
    count = _buffer(8)
    indices = _buffer(4 * capacity)
    selected = [_buffer(capacity * c.shape[1]) for c in columns]
    outputs = api._pointer_array(None if null_outputs else b[8:].ctypes.data for b in selected)
    s = api.bzamd_row_selection(selector_descs[0], reject, 1 if invert else 0,
                                descs if columns else None, outputs if columns else None,
                                len(columns), capacity, 1 if zero_tail else 0)
    lib_api.load().bzamd_select_rows(
        count[8:].ctypes.data if want_count else None,
        indices[8:].ctypes.data if want_indices and not null_outputs else None, ctypes.byref(s))
    for array, kept in zip((selector, *columns), before):
        assert np.array_equal(array, kept), "an input was modified"
    want_number, want_rows, want_selected = sc.select(selector, columns, reject, invert, capacity,
                                                     zero_tail)
    got = _body(count, "count")
    if want_count:
        assert int(got.view(np.uint64)[0]) == want_number
    else:
        assert np.all(got == CANARY), "`count` was written"
    got = _body(indices, "indices")
    if want_indices:
        assert np.array_equal(got.view(np.uint32), want_rows), "indices"
    else:
        assert np.all(got == CANARY), "`indices` was written"
    for j, (buffer, want) in enumerate(zip(selected, want_selected)):
        assert np.array_equal(_body(buffer, f"selected[{j}]").reshape(want.shape), want), j
    return want_number if want_count else None


def take_rows(lib_api, indices, columns):
    """bzamd_take_rows through ctypes, checked against the model, with the bytes around every
    output and the inputs"""
    indices = np.ascontiguousarray(indices, dtype=np.uint32)
    descs, keep = api.make_descriptors([(c, False) for c in columns])
    before = [np.array(a, copy=True) for a in (indices, *columns)]
    taken = [_buffer(len(indices) * c.shape[1]) for c in columns]
    outputs = api._pointer_array(b[8:].ctypes.data for b in taken)
    t = api.bzamd_row_take(indices.ctypes.data, len(indices), descs, outputs, len(columns))
    lib_api.load().bzamd_take_rows(ctypes.byref(t))
    for array, kept in zip((indices, *columns), before):
        assert np.array_equal(array, kept), "an input was modified"
    for j, (buffer, want) in enumerate(zip(taken, sc.take(indices, columns))):
        assert np.array_equal(_body(buffer, f"taken[{j}]").reshape(want.shape), want), j


#--------------------------------------------------------------------------------------------------
# the model on hand-written cases
#--------------------------------------------------------------------------------------------------
def test_model_on_hand_written_cases():
    flags = np.array([[0], [1], [0], [2], [1]], np.uint8)
    column = np.array([[10, 0], [11, 0], [12, 1], [13, 1], [14, 2]], np.uint8)
    short = np.array([[7], [8]], np.uint8)
    assert list(sc.bits(np.array([[1, 2], [255, 255]], np.uint8))) == [0x0201, 0xFFFF]
    assert list(sc.kept_rows(flags)) == [1, 3, 4]
    assert list(sc.kept_rows(flags, reject=1)) == [0, 2, 3]
    assert list(sc.kept_rows(flags, reject=1, invert=True)) == [1, 4]
    assert list(sc.kept_rows(flags, reject=256)) == [0, 1, 2, 3, 4]
    count, indices, (got, got_short) = sc.select(flags, [column, short], capacity=4, zero_tail=True)
    assert count == 3 and list(indices) == [1, 3, 4, sc.NO_ROW]
    assert got.tolist() == [[11, 0], [13, 1], [14, 2], [0, 0]]
    assert got_short.tolist() == [[8], [0], [0], [0]]
    count, indices, (got,) = sc.select(flags, [column], capacity=2)
    assert count == 3 and list(indices) == [1, 3] and got.tolist() == [[11, 0], [13, 1]]
    count, indices, (got,) = sc.select(flags, [column], capacity=4)
    assert list(indices[:3]) == [1, 3, 4] and indices[3] == 0x5A5A5A5A
    assert got[3].tolist() == [CANARY, CANARY]
    taken, = sc.take([4, 0, 5, sc.NO_ROW, 0], [column])
    assert taken.tolist() == [[14, 2], [10, 0], [0, 0], [0, 0], [10, 0]]
    assert sc.spans(0) == (1, 1) and sc.spans(1) == (1, 1) and sc.spans(sc.TILE + 1) == (2, 1)
    assert sc.spans(2048 * sc.TILE) == (2048, 1) and sc.spans(2048 * sc.TILE + 1) == (1025, 2)
    selector = sc.selector_of([True, False, True], width=3, reject=0xFFFFFF)
    assert list(sc.kept_rows(selector, 0xFFFFFF)) == [0, 2]


#--------------------------------------------------------------------------------------------------
# host form against the model
#--------------------------------------------------------------------------------------------------
def _rejects(width):
    ones = (1 << (8 * width)) - 1
    return {"zero": 0, "ones": ones, "middle": 0x8081828384858687 & ones}


@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("reject", ["zero", "ones", "middle"])
@pytest.mark.parametrize("width", range(1, 9))
def test_selector_widths(cpu_backend, width, reject, invert):
    """every selector width with reject 0, all ones and a middle value, kept and rejected rows
    mixed; a signed descriptor selects the same rows"""
    rng = np.random.default_rng(8 * width + invert)
    reject = _rejects(width)[reject]
    n = 300
    selector = sc.selector_of(rng.integers(0, 2, n).astype(bool), width, reject, rng)
    columns = sc.random_columns(rng, [8, 5], n)
    count = select_rows(cpu_backend, selector, columns, reject, invert)
    assert 0 < count < n
    assert select_rows(cpu_backend, selector, columns, reject, invert, signed=True) == count


def test_reject_wider_than_the_selector(cpu_backend):
    """the row's bits are zero-extended: no row of one byte equals 0x100, and none 2^64 - 1"""
    selector = np.arange(256, dtype=np.uint8).reshape(256, 1)
    for reject in (0x100, 2**64 - 1):
        assert select_rows(cpu_backend, selector, [selector], reject) == 256
        assert select_rows(cpu_backend, selector, [selector], reject, invert=True) == 0


@pytest.mark.parametrize("first", [1, 17])
def test_column_widths(cpu_backend, first):
    """every column width 1 .. 32, sixteen columns a call"""
    rng = np.random.default_rng(first)
    n = 77
    selector = sc.selector_of(rng.integers(0, 2, n).astype(bool))
    columns = sc.random_columns(rng, list(range(first, first + 16)), n)
    select_rows(cpu_backend, selector, columns, zero_tail=True, capacity=n + 3)
    take_rows(cpu_backend, rng.integers(0, n + 5, 50), columns)


@pytest.mark.parametrize("num_columns", [0, 1, 16])
def test_column_counts_and_short_columns(cpu_backend, num_columns):
    """0, 1 and 16 columns; columns shorter than n, down to no rows and a null pointer: kept rows
    at or past a column's end are zero bytes"""
    rng = np.random.default_rng(num_columns)
    n = 200
    selector = sc.selector_of(rng.integers(0, 4, n) != 0)
    rows = [n, 0, 1, n - 1, 100, 0, n, 37][:num_columns] + [n - j for j in range(8)][:max(
        num_columns - 8, 0)]
    widths = [8, 32, 1, 3, 16, 7, 31, 2, 4, 5, 6, 9, 12, 24, 30, 32][:num_columns]
    columns = sc.random_columns(rng, widths, rows)
    for zero_tail in (False, True):
        assert select_rows(cpu_backend, selector, columns, zero_tail=zero_tail) > 100


@pytest.mark.parametrize("zero_tail", [False, True])
def test_capacities(cpu_backend, zero_tail):
    """capacity 0, count - 1, count, count + 1 and above n: count is exact, nothing at or past
    min(count, capacity) is written without the tail, and with it the rest is zeros and
    0xFFFFFFFF"""
    rng = np.random.default_rng(5)
    n = 150
    selector = sc.selector_of(rng.integers(0, 2, n).astype(bool), width=4, reject=0xFFFFFFFF)
    columns = sc.random_columns(rng, [8, 3, 32], [n, n, 90])
    count = len(sc.kept_rows(selector, 0xFFFFFFFF))
    for capacity in (0, count - 1, count, count + 1, n + 10):
        assert select_rows(cpu_backend, selector, columns, 0xFFFFFFFF, capacity=capacity,
                           zero_tail=zero_tail) == count
    assert select_rows(cpu_backend, selector, columns, 0xFFFFFFFF, capacity=0, zero_tail=zero_tail,
                       null_outputs=True) == count


def test_count_alone_and_indices_alone(cpu_backend):
    rng = np.random.default_rng(6)
    selector = sc.selector_of(rng.integers(0, 2, 99).astype(bool), width=8, reject=0)
    assert select_rows(cpu_backend, selector, [], want_indices=False) > 0
    assert select_rows(cpu_backend, selector, [], want_count=False) is None
    columns = sc.random_columns(rng, [8], 99)
    assert select_rows(cpu_backend, selector, columns, want_count=False,
                       want_indices=False) is None


@pytest.mark.parametrize("zero_tail", [False, True])
def test_no_rows(cpu_backend, zero_tail):
    """n = 0 with a null selector: count = 0, and the tail rule still applies"""
    selector = np.zeros((0, 1), np.uint8)
    columns = [np.zeros((0, 8), np.uint8), np.zeros((0, 3), np.uint8)]
    assert select_rows(cpu_backend, selector, columns, capacity=5, zero_tail=zero_tail) == 0
    assert select_rows(cpu_backend, selector, [], capacity=0) == 0


def test_wrapper(cpu_backend):
    rng = np.random.default_rng(7)
    flags = rng.integers(0, 2, 60).astype(np.uint8)
    values = rng.integers(-2**62, 2**62, 60, dtype=np.int64)
    count, indices, (selected,) = cpu_backend.select_rows(flags, [values])
    rows = np.flatnonzero(flags)
    assert count == len(rows) and np.array_equal(indices, rows)
    assert np.array_equal(selected.view(np.int64).reshape(-1), values[rows])
    count, indices, (selected,) = cpu_backend.select_rows(flags, [values], capacity=64,
                                                          zero_tail=True, invert=True)
    assert count == 60 - len(rows) and len(indices) == 64 and np.all(indices[count:] == sc.NO_ROW)
    assert np.all(selected[count:] == 0)
    taken, = cpu_backend.take_rows(indices, [values])
    assert np.array_equal(taken[:count].view(np.int64).reshape(-1), values[flags == 0])
    assert np.all(taken[count:] == 0)


#--------------------------------------------------------------------------------------------------
# the gather
#--------------------------------------------------------------------------------------------------
def test_take_rows(cpu_backend):
    """indices in range, at a column's end, at 0xFFFFFFFF and repeated, against columns of
    different lengths, a column of no rows among them"""
    rng = np.random.default_rng(8)
    columns = sc.random_columns(rng, [8, 1, 32, 31, 4], [50, 20, 35, 50, 0])
    indices = [0, 49, 50, 20, 19, 35, 34, sc.NO_ROW, 7, 7, 7, 2**31, 0] + list(
        rng.integers(0, 60, 40))
    take_rows(cpu_backend, indices, columns)
    take_rows(cpu_backend, [3], columns[:1])


#--------------------------------------------------------------------------------------------------
# the workspace: no backend
#--------------------------------------------------------------------------------------------------
def test_packed_width_switch():
    """the diagnostic that picks the device form's store shape: clamped to 32, a negative width
    only asks"""
    first = api.select_rows_packed_width()
    assert 0 <= first <= 32
    assert api.select_rows_packed_width(100) == first and api.select_rows_packed_width() == 32
    assert api.select_rows_packed_width(8) == 32 and api.select_rows_packed_width(-5) == 8
    assert api.select_rows_packed_width(first) == 8 and api.select_rows_packed_width() == first


def test_workspace_bytes():
    api.reset_for_testing()
    tile = sc.TILE
    for n in (0, 1, tile, tile + 1, 2048 * tile, 2048 * tile + 1, 2**30 - 1, 2**30):
        assert api.select_rows_workspace_bytes(n) == sc.workspace_bytes(n) != 0, n
    assert api.select_rows_workspace_bytes(0) == 4 + 256
    assert api.select_rows_workspace_bytes(2**30) == 4 * 2048 + 256
    assert api.select_rows_workspace_bytes(2**30 + 1) == 0
    assert api.select_rows_workspace_bytes(2**64 - 1) == 0


#--------------------------------------------------------------------------------------------------
# aborts (host backend only; each in a child process)
#--------------------------------------------------------------------------------------------------
SETUP = ("lib = api.load()\n"
         "sel = np.ones(16, np.uint8); col = np.arange(16, dtype=np.int64)\n"
         "out = np.zeros(32, np.uint64); out2 = np.zeros(32, np.uint64)\n"
         "idx = np.zeros(32, np.uint32); cnt = np.zeros(4, np.uint64)\n"
         "work = np.zeros(2048, np.uint8)\n"
         "S, C, O, P, X, N, W = (a.ctypes.data for a in (sel, col, out, out2, idx, cnt, work))\n"
         "D = api.sxt_sequence_descriptor\n"
         "sel16, col16 = (1, 16, S, 0), (8, 16, C, 1)\n"
         "def struct(selector, columns, outputs, capacity):\n"
         "    descs = (D * max(len(columns), 1))(*[D(*c) for c in columns])\n"
         "    outs = api._pointer_array(outputs)\n"
         "    return api.bzamd_row_selection(D(*selector), 0, 0, descs, outs, len(columns),"
         " capacity, 0), descs, outs\n"
         "def call(count=N, indices=X, selector=sel16, columns=(col16,), outputs=(O,),"
         " capacity=16):\n"
         "    s = struct(selector, columns, outputs, capacity)\n"
         "    lib.bzamd_select_rows(count, indices, ctypes.byref(s[0]))\n"
         "def device(workspace, workspace_bytes, count=N, outputs=(O,)):\n"
         "    s = struct(sel16, (col16,), outputs, 16)\n"
         "    lib.bzamd_select_rows_device(count, X, ctypes.byref(s[0]), workspace,"
         " workspace_bytes, None)\n"
         "def take_struct(indices, num_rows, columns, outputs):\n"
         "    descs = (D * max(len(columns), 1))(*[D(*c) for c in columns])\n"
         "    outs = api._pointer_array(outputs)\n"
         "    return api.bzamd_row_take(indices, num_rows, descs, outs, len(columns)), descs, outs\n"
         "def take(indices=X, num_rows=16, columns=(col16,), outputs=(O,)):\n"
         "    t = take_struct(indices, num_rows, columns, outputs)\n"
         "    lib.bzamd_take_rows(ctypes.byref(t[0]))\n"
         "NEED = api.select_rows_workspace_bytes(16)\n")
ABORTS = {
    "null_s": ("lib.bzamd_select_rows(N, X, None)\n", "null argument to `bzamd_select_rows`"),
    "null_s_device": ("lib.bzamd_select_rows_device(N, X, None, W, 2048, None)\n",
                      "null argument to `bzamd_select_rows_device`"),
    "null_columns": ("s = api.bzamd_row_selection(D(*sel16), 0, 0, None, api._pointer_array([O]),"
                     " 1, 16, 0)\nlib.bzamd_select_rows(N, X, ctypes.byref(s))\n",
                     "null argument to `bzamd_select_rows`"),
    "null_selected": ("descs = (D * 1)(D(*col16))\n"
                      "s = api.bzamd_row_selection(D(*sel16), 0, 0, descs, None, 1, 16, 0)\n"
                      "lib.bzamd_select_rows(N, X, ctypes.byref(s))\n",
                      "null argument to `bzamd_select_rows`"),
    "seventeen_columns": ("call(columns=(col16,) * 17, outputs=(O,) * 17)\n",
                          "needs num_columns <= 16"),
    "selector_width_9": ("call(selector=(9, 1, S, 0))\n", "needs a selector of 1 .. 8 bytes"),
    "selector_width_0": ("call(selector=(0, 16, S, 0))\n", "element_nbytes must be in [1, 32]"),
    "selector_null_data": ("call(selector=(1, 16, None, 0))\n",
                           "descriptor has n > 0 but null data"),
    "column_width_33": ("call(columns=((33, 1, C, 0),))\n", "element_nbytes must be in [1, 32]"),
    "column_signed_17": ("call(columns=((17, 4, C, 1),))\n",
                         "signed sequences need element_nbytes <= 16"),
    "column_null_data": ("call(columns=((8, 16, None, 1),))\n",
                         "descriptor has n > 0 but null data"),
    "column_longer_than_n": ("call(columns=((4, 17, C, 0),))\n", "is longer than n"),
    "n_above_2_pow_30": ("call(indices=None, selector=(1, 2**30 + 1, S, 0), columns=(), outputs=(),"
                         " capacity=0)\n", "needs n <= 2^30"),
    "capacity_above_2_pow_30": ("call(capacity=2**30 + 1)\n", "needs capacity <= 2^30"),
    "no_output": ("call(count=None, indices=None, columns=(), outputs=())\n", "needs an output"),
    "null_output_pointer": ("call(outputs=(None,))\n", "null output of the row selection"),
    "misaligned_count": ("call(count=N + 4)\n", "must be 8-byte aligned"),
    "misaligned_output": ("call(outputs=(O + 4,))\n", "must be 8-byte aligned"),
    "misaligned_indices": ("call(indices=X + 2)\n", "indices must be 4-byte aligned"),
    "outputs_overlap": ("call(columns=(col16, col16), outputs=(O, O + 120))\n",
                        "the outputs of the row selection overlap"),
    "indices_overlap_count": ("call(count=X + 56)\n", "the outputs of the row selection overlap"),
    "in_place": ("call(outputs=(C,))\n", "an output overlaps an input"),
    "output_overlaps_the_selector": ("call(selector=(1, 16, O + 127, 0))\n",
                                     "an output overlaps an input"),
    "indices_overlap_a_column": ("call(indices=C + 124)\n", "an output overlaps an input"),
    "workspace_too_small": ("device(W, NEED - 1)\n",
                            "the workspace of the row selection is too small"),
    "workspace_null": ("device(None, 2048)\n", "the workspace of the row selection is too small"),
    "output_overlaps_the_workspace": ("device(W, NEED, outputs=(W + 256,))\n",
                                      "an output overlaps the workspace"),
    "device_form_on_cpu": ("device(W, 2048)\n", "device entry points need the GPU backend"),
    "take_null_t": ("lib.bzamd_take_rows(None)\n", "null argument to `bzamd_take_rows`"),
    "take_null_indices": ("take(indices=None)\n", "null argument to `bzamd_take_rows`"),
    "take_null_t_device": ("lib.bzamd_take_rows_device(None, None)\n",
                           "null argument to `bzamd_take_rows_device`"),
    "take_no_rows": ("take(num_rows=0)\n", "needs 1 <= num_rows <= 2^30"),
    "take_rows_above_2_pow_30": ("take(num_rows=2**30 + 1)\n", "needs 1 <= num_rows <= 2^30"),
    "take_no_columns": ("take(columns=(), outputs=())\n", "needs 1 <= num_columns <= 16"),
    "take_seventeen_columns": ("take(columns=(col16,) * 17, outputs=(O,) * 17)\n",
                               "needs 1 <= num_columns <= 16"),
    "take_column_width_0": ("take(columns=((0, 16, C, 0),))\n", "element_nbytes must be in [1, 32]"),
    "take_null_output": ("take(outputs=(None,))\n", "null output of the row gather"),
    "take_misaligned_output": ("take(outputs=(O + 4,))\n", "must be 8-byte aligned"),
    "take_misaligned_indices": ("take(indices=X + 2, num_rows=8)\n",
                                "indices must be 4-byte aligned"),
    "take_outputs_overlap": ("take(columns=(col16, col16), outputs=(O, O + 120))\n",
                             "the outputs of the row gather overlap"),
    "take_in_place": ("take(outputs=(C,))\n", "an output overlaps an input"),
    "take_output_overlaps_indices": ("take(outputs=(X,), num_rows=4)\n",
                                     "an output overlaps an input"),
    "take_device_form_on_cpu": ("t = take_struct(X, 16, (col16,), (O,))\n"
                                "lib.bzamd_take_rows_device(ctypes.byref(t[0]), None)\n",
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


# kernel -> instantiations: the scatter with and without the stage in LDS
KERNELS = {"k_select_count": 1, "k_select_scatter": 2, "k_take_rows": 1}


@pytest.mark.skipif(_hipcc() is None, reason="hipcc is not installed")
def test_kernels_use_no_scratch(tmp_path):
    """the compiler's own resource report of proof/select_rows.hip with the flags the library is
    built with: every kernel of the file"""
    from blitzar_amd import build
    src = "proof/select_rows.hip"
    assert src in build.SOURCES
    r = subprocess.run([_hipcc(), *build.FLAGS, *build.TU_FLAGS.get(src, []), "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(build.CSRC, src), "-o", str(tmp_path / "select_rows.o")],
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
