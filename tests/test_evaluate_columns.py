"""The MLE evaluations of typed columns against the evaluation vector (include/blitzar_amd.h:
bzamd_evaluate_columns, bzamd_evaluate_columns_workspace_bytes), host form on the host backend.

evaluations[j] = sum_i column_j[i] * vector[i]: every expected value is plain Python integers mod l
(field 0) or mod the Grumpkin modulus (field 1, Montgomery form x 2^256 at the boundary), and every
comparison is of bytes.  The columns, their kinds, lengths and extreme rows are those of
tests/test_mle_opening.py; the device form is in tests/test_evaluate_columns_device.py, which takes
its vectors and expectations from here."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests.test_mle_opening import KINDS, Columns, as_bytes, element_value
from tests.test_sumcheck_device import MODULUS, to_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def unreduced_entry(field_id):
    """32 bytes that are no canonical element: 2^256 - 1, or the bytes of p + 5"""
    top = (1 << 256) - 1 if field_id == 0 else MODULUS[field_id] + 5
    return np.frombuffer(top.to_bytes(32, "little"), np.uint8)


def vector_of(field_id, n, seed):
    """uint8 [n, 32]: 0, 1, p - 1 and an unreduced entry among random canonical ones, at rows that
    move with the seed (n < 4: the first n of the four, starting with the seed's)"""
    p = MODULUS[field_id]
    rng = np.random.default_rng(seed)
    rows = [to_bytes(field_id, int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(),
                                              "little") % p) for _ in range(n)]
    specials = [to_bytes(field_id, 0), to_bytes(field_id, 1), to_bytes(field_id, p - 1),
                unreduced_entry(field_id)]
    for k in range(min(n, 4)):
        at = (seed + 61 * k) % n if n >= 4 else k
        rows[at] = specials[(seed + k) % 4 if n < 4 else k]
    return np.stack(rows).copy()


def vector_values(field_id, vector):
    return [element_value(field_id, row) for row in vector]


def expected_evaluations(field_id, values, vector):
    """values[j]: the rows of column j as field integers; vector: uint8 [n, 32] -> uint8 [., 32]"""
    b = vector_values(field_id, vector)
    return as_bytes(field_id, [sum(x * y for x, y in zip(column, b)) for column in values])


@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 257])
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_evaluation_host_form(cpu_backend, field_id, n, shift):
    """six columns, one of every kind; the four shifts put every length (n, n - 1, 1 and 0 rows with
    a null pointer) on every kind; every input is what it was afterwards"""
    case = Columns(field_id, n, len(KINDS), 120 + shift, shift)
    vector = vector_of(field_id, n, 7 + shift)
    columns, passed = case.host_columns(), vector.copy()
    got = cpu_backend.evaluate_columns(field_id, columns, passed, n)
    assert got.shape == (len(KINDS), 32)
    assert np.array_equal(got, expected_evaluations(field_id, case.values, vector))
    assert np.array_equal(passed, vector), "the vector was modified"
    for (after, _), (before, _) in zip(columns, case.arrays):
        assert np.array_equal(after, before), "a column was modified"


@pytest.mark.parametrize("field_id", [0, 1])
def test_every_special_entry_meets_a_row(field_id):
    """the vectors of test_evaluation_host_form hold all four special entries where n allows"""
    p = MODULUS[field_id]
    want = {0, 1, p - 1, element_value(field_id, unreduced_entry(field_id))}
    for shift in (0, 1, 2, 3):
        vector = vector_of(field_id, 257, 7 + shift)
        assert want <= set(vector_values(field_id, vector))
        assert any(np.array_equal(row, unreduced_entry(field_id)) for row in vector)
    single = {bytes(vector_of(field_id, 1, 7 + shift)[0]) for shift in (0, 1, 2, 3)}
    assert len(single) == 4


@pytest.mark.parametrize("field_id", [0, 1])
def test_many_columns_host_form(cpu_backend, field_id):
    case = Columns(field_id, 9, 70, 150)
    vector = vector_of(field_id, 9, 3)
    got = cpu_backend.evaluate_columns(field_id, case.host_columns(), vector, 9)
    assert np.array_equal(got, expected_evaluations(field_id, case.values, vector))


def test_a_zero_column_evaluates_to_zero(cpu_backend):
    for field_id in (0, 1):
        got = cpu_backend.evaluate_columns(field_id, [np.zeros((0, 8), np.uint8)],
                                           vector_of(field_id, 5, 1), 5)
        assert np.array_equal(got, np.zeros((1, 32), np.uint8))


def test_workspace_bytes():
    """needs no backend; 0 for what the call would reject; grows with either count; the partial sums
    of at most 1024 workgroups are 36 KiB a column (sanity cap: 64 KiB a column and 1 MiB)"""
    from blitzar_amd import api
    size = api.evaluate_columns_workspace_bytes
    for field_id in (0, 1):
        assert size(field_id, 0, 5) == 0
        assert size(field_id, 3, 0) == 0
        assert size(field_id, 3, (1 << 30) + 1) == 0
        assert size(field_id, 1, 1) > 0
        ns = [1, 2, 255, 256, 257, 1000, 1 << 16, (1 << 18) + 300, 1 << 20, 1 << 30]
        counts = [1, 2, 7, 8, 9, 16, 17, 70, 1000]
        for a, b in zip(ns, ns[1:]):
            for count in counts:
                assert size(field_id, count, a) <= size(field_id, count, b)
        for n in ns:
            for a, b in zip(counts, counts[1:]):
                assert size(field_id, a, n) <= size(field_id, b, n)
        for count in counts:
            assert size(field_id, count, 1 << 30) < 64 * 1024 * count + (1 << 20)
    assert size(2, 3, 5) == 0


#--------------------------------------------------------------------------------------------------
# aborts (host backend only; each in a child process)
#--------------------------------------------------------------------------------------------------
RAW = ("import ctypes\n"
       "out, vec = np.zeros((1, 32), np.uint8), np.zeros((2, 32), np.uint8)\n"
       "col = np.ones((1, 8), np.uint8)\n"
       "descs, keep = api.make_descriptors([(col, False)])\n"
       "e = api.bzamd_column_evaluation(descs, 1, 1)\n"
       "call = api.load().bzamd_evaluate_columns\n")
V2 = "v = np.zeros((2, 32), np.uint8)\n"
ABORTS = {
    "null_evaluations": (RAW + "call(None, 0, vec.ctypes.data, ctypes.byref(e))\n",
                         "null argument to `bzamd_evaluate_columns`"),
    "null_vector": (RAW + "call(out.ctypes.data, 0, None, ctypes.byref(e))\n",
                    "null argument to `bzamd_evaluate_columns`"),
    "null_struct": (RAW + "call(out.ctypes.data, 0, vec.ctypes.data, None)\n",
                    "null argument to `bzamd_evaluate_columns`"),
    "null_columns": (RAW + "e = api.bzamd_column_evaluation(None, 1, 1)\n"
                     "call(out.ctypes.data, 0, vec.ctypes.data, ctypes.byref(e))\n",
                     "descriptors is null"),
    "no_columns": (V2 + "api.evaluate_columns(0, [], v, 2)\n", "needs at least one column"),
    "n_zero": (V2 + "api.evaluate_columns(0, [np.ones((0, 8), np.uint8)], v, 0)\n",
               "the column evaluation needs 1 <= n <= 2^30"),
    "n_above_2_pow_30": (V2 + "api.evaluate_columns(0, [np.ones((1, 8), np.uint8)], v, 2**30 + 1)\n",
                         "the column evaluation needs 1 <= n <= 2^30"),
    "column_longer_than_n": (V2 + "api.evaluate_columns(0, [np.ones((3, 8), np.uint8)], v, 2)\n",
                             "an evaluated column is longer than n"),
    "width_33": (V2 + "api.evaluate_columns(0, [np.ones((2, 33), np.uint8)], v, 2)\n",
                 "element_nbytes must be in [1, 32]"),
    "signed_width_17": (V2 + "api.evaluate_columns(0, [(np.ones((2, 17), np.uint8), True)], v, 2)\n",
                        "signed sequences need element_nbytes <= 16"),
    "field_2": (V2 + "api.evaluate_columns(2, [np.ones((2, 8), np.uint8)], v, 2)\n",
                "unsupported field id"),
    "misaligned_vector": (RAW + "buf = np.zeros(72, np.uint8)\n"
                          "at = buf.ctypes.data + 8 - buf.ctypes.data % 8 + 4\n"
                          "call(out.ctypes.data, 0, at, ctypes.byref(e))\n",
                          "the evaluation vector must be 8-byte aligned"),
    "device_form_on_cpu": ("out, vec = np.zeros((1, 32), np.uint8), np.zeros((1, 32), np.uint8)\n"
                           "work = np.zeros(1 << 16, np.uint8)\n"
                           "api.evaluate_columns_device(0, [(vec.ctypes.data, 1, 8, False)],\n"
                           "    vec.ctypes.data, 1, out.ctypes.data, work.ctypes.data, work.size)\n",
                           "device entry points need the GPU backend"),
}


@pytest.mark.parametrize("name", sorted(ABORTS))
def test_bad_arguments_abort(name):
    call, message = ABORTS[name]
    code = ("import numpy as np\nfrom blitzar_amd import api\napi.init(api.SXT_CPU_BACKEND, 0)\n"
            + call)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode < 0 and message in r.stderr, r.stderr


#--------------------------------------------------------------------------------------------------
# the kernels' resources
#--------------------------------------------------------------------------------------------------
def _hipcc():
    from blitzar_amd import build
    return build.HIPCC if os.path.exists(build.HIPCC) else shutil.which("hipcc")


@pytest.mark.skipif(_hipcc() is None, reason="hipcc is not installed")
def test_kernels_use_no_scratch(tmp_path):
    """the compiler's own resource report of proof/mle_opening.hip with the flags the library is
    built with: a lane's accumulators of a whole chunk stay in registers, both fields"""
    from blitzar_amd import build
    src = "proof/mle_opening.hip"
    assert src in build.SOURCES
    r = subprocess.run([_hipcc(), *build.FLAGS, *build.TU_FLAGS.get(src, []), "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(build.CSRC, src), "-o", str(tmp_path / "mle_opening.o")],
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
    for kernel in ("k_evaluate_columns", "k_evaluate_finish"):
        found = {k: v for k, v in scratch.items() if kernel in k}
        assert len(found) == 2, f"{kernel}: found {sorted(found)}"
        assert all(v == 0 for v in found.values()), found
