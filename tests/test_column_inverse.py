"""The inverse column of a log-derivative argument (include/blitzar_amd.h: bzamd_invert_columns),
host form on the host backend.

Every expected value is Python integers (tests/column_inverse_cases.py: the denominators and
pow(d, -1, p) with zero kept as zero) and every comparison is of bytes.  The device form is in
tests/test_column_inverse_device.py."""
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
from tests.test_mle_opening import Columns, as_bytes
from tests.test_sumcheck_device import MODULUS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0x5A


def invert(lib_api, field_id, columns, n, coefficients, shift, outputs):
    """bzamd_invert_columns through ctypes, so that either output can be a null pointer.  columns:
    (array, signed) pairs, passed where they lie; outputs: "inverses", "scalars" or "both"
    -> (inverses or None, scalars or None), each checked for an intact row behind it"""
    descs, keep = api.make_descriptors(columns)
    for (given, _), kept in zip(columns, keep):
        assert kept.size == 0 or kept.ctypes.data == given.ctypes.data, "a column was copied"
    out = {name: np.full((n + 1, 32), CANARY, np.uint8) for name in ("inverses", "scalars")
           if outputs in (name, "both")}
    v = api.bzamd_column_inversion(descs, None if coefficients is None else coefficients.ctypes.data,
                                   None if shift is None else shift.ctypes.data, len(keep), n)
    lib_api.load().bzamd_invert_columns(api._ptr(out.get("inverses")), api._ptr(out.get("scalars")),
                                        field_id, ctypes.byref(v))
    for name, rows in out.items():
        assert np.all(rows[n] == CANARY), f"the row behind `{name}` was written"
    return tuple(out[name][:n] if name in out else None for name in ("inverses", "scalars"))


def check(lib_api, field_id, columns, values, n, coefficients=None, shift=None, outputs="both"):
    """coefficients, shift: raw integers (the bytes the library gets) or None"""
    want = cic.inverses(field_id, cic.denominators(
        field_id, values,
        None if coefficients is None else [cic.raw_value(field_id, c) for c in coefficients],
        None if shift is None else cic.raw_value(field_id, shift), n))
    want_elements, want_scalars = cic.expected_bytes(field_id, want)
    c_bytes = (None if coefficients is None
               else np.stack([cic.element_bytes(field_id, c) for c in coefficients]))
    s_bytes = None if shift is None else cic.element_bytes(field_id, shift)
    before = [np.array(c, copy=True) for c, _ in columns]
    inverses, scalars = invert(lib_api, field_id, columns, n, c_bytes, s_bytes, outputs)
    if outputs != "scalars":
        assert np.array_equal(inverses, want_elements)
    if outputs != "inverses":
        assert np.array_equal(scalars, want_scalars)
    for (c, _), kept in zip(columns, before):
        assert np.array_equal(c, kept), "a column was modified"
    return want


#--------------------------------------------------------------------------------------------------
# the model checks itself
#--------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field_id", [0, 1])
def test_model_batch_inversion_agrees_with_pow(field_id):
    p = MODULUS[field_id]
    rng = np.random.default_rng(3)
    ds = [int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % p
          for _ in range(50)]
    for zero in (0, 1, 17, 18, 49):
        ds[zero] = 0
    inv = cic.inverses(field_id, ds)
    assert cic.batch_inverses(field_id, ds) == inv
    assert all((d * x) % p == (1 if d else 0) for d, x in zip(ds, inv))


#--------------------------------------------------------------------------------------------------
# host form against the model
#--------------------------------------------------------------------------------------------------
def typed_columns(field_id, n, shift):
    """the six kinds of tests/test_mle_opening.py Columns (widths 1, 2, 8 and 16 signed with the
    most negative value and -1, 31, 32 with unreduced rows; lengths n, n - 1, 1 and 0 / NULL),
    taken where they lie in `flat`: one, three or no bytes past a multiple of 8; and a seventh
    column of 32-byte rows with 2^256 - 1, p and p - 1 among them"""
    p = MODULUS[field_id]
    case = Columns(field_id, n, 6, 900 + 10 * n + shift, shift)
    columns = [(case.flat[at:at + rows * width].reshape(rows, width), signed)
               for at, rows, width, signed in case.specs]
    top = [(1 << 256) - 1, p, p - 1, 2 * p + 3, 5][:n]
    columns.append((np.stack([cic.element_bytes(field_id, x) for x in top]), False))
    values = case.values + [[cic.raw_value(field_id, x) for x in top]]
    return case, columns, values


@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 1000])
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_host_form(cpu_backend, field_id, n, shift):
    p = MODULUS[field_id]
    case, columns, values = typed_columns(field_id, n, shift)
    addresses = {c.ctypes.data % 8 for c, _ in columns if c.size}
    assert addresses & {1, 3}, "no column at an odd address"
    assert any(c.shape[0] == 0 for c, _ in columns) and any(c.shape[0] == n - 1 for c, _ in columns)
    rng = np.random.default_rng(shift)
    alpha = int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % p
    coefficients = case.coefficients + [alpha * alpha % p]
    check(cpu_backend, field_id, columns, values, n, coefficients, alpha)
    check(cpu_backend, field_id, columns, values, n, None, alpha, outputs="inverses")
    check(cpu_backend, field_id, columns, values, n, coefficients, None, outputs="scalars")
    check(cpu_backend, field_id, columns, values, n, None, None)
    # unreduced: the largest 32 bytes, and a multiple of p more than the value
    unreduced = list(coefficients)
    unreduced[0] = (1 << 256) - 1
    unreduced[2] = coefficients[2] + 2 * p
    check(cpu_backend, field_id, columns, values, n, unreduced, alpha + 3 * p)
    check(cpu_backend, field_id, columns, values, n, unreduced, (1 << 256) - 1)


@pytest.mark.parametrize("field_id", [0, 1])
def test_wrapper(cpu_backend, field_id):
    """api.invert_columns: inverses alone, or both forms"""
    p, n = MODULUS[field_id], 37
    rng = np.random.default_rng(11)
    column = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
    narrow = rng.integers(0, 256, (n - 4, 3), dtype=np.uint8)
    alpha, beta = 12345678901234567890123 % p, p - 7
    values = [cic.integer_values(field_id, column, True), cic.integer_values(field_id, narrow, False)]
    want = cic.inverses(field_id, cic.denominators(field_id, values, [1, beta], alpha, n))
    elements, scalars = cic.expected_bytes(field_id, want)
    got = cpu_backend.invert_columns(field_id, [column, narrow], n,
                                     coefficients=as_bytes(field_id, [1, beta]),
                                     shift=as_bytes(field_id, [alpha])[0])
    assert np.array_equal(got, elements)
    got, got_scalars = cpu_backend.invert_columns(field_id, [column, narrow], n,
                                                  coefficients=as_bytes(field_id, [1, beta]),
                                                  shift=as_bytes(field_id, [alpha])[0],
                                                  want_scalars=True)
    assert np.array_equal(got, elements) and np.array_equal(got_scalars, scalars)
    if field_id == 0:
        assert np.array_equal(got, got_scalars)
    want = cic.inverses(field_id, cic.denominators(field_id, values, None, None, n))
    assert np.array_equal(cpu_backend.invert_columns(field_id, [column, narrow], n),
                          cic.expected_bytes(field_id, want)[0])


#--------------------------------------------------------------------------------------------------
# zero denominators
#--------------------------------------------------------------------------------------------------
ZERO_ROWS = {
    "first": [0],
    "last": [999],
    "adjacent": [500, 501],
    "across_a_block_of_the_host_form": [255, 256],
    "a_whole_block_of_the_host_form": list(range(256, 512)),
    "all_but_one": [i for i in range(1000) if i != 700],
}


@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("where", sorted(ZERO_ROWS))
def test_zero_denominators_disturb_no_other_row(cpu_backend, field_id, where):
    """column[i] = -shift at the chosen rows: those rows are zero in both forms, every other row is
    exact"""
    p, n = MODULUS[field_id], 1000
    rng = np.random.default_rng(21)
    column = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
    column[ZERO_ROWS[where]] = -987654321
    want = check(cpu_backend, field_id, [(column, True)], [cic.integer_values(field_id, column, True)],
                 n, None, cic.element_raw(field_id, 987654321))
    assert [i for i, x in enumerate(want) if x == 0] == ZERO_ROWS[where]


@pytest.mark.parametrize("field_id", [0, 1])
def test_zero_by_cancellation(cpu_backend, field_id):
    """shift = p - value: the denominator is zero mod p, not as an integer"""
    p, n = MODULUS[field_id], 300
    rng = np.random.default_rng(22)
    column = rng.integers(1, 2**63 - 1, n, dtype=np.uint64)
    value = int(column[123])
    column[7] = value
    shift_raw = cic.element_raw(field_id, p - value)
    want = check(cpu_backend, field_id, [(column, False)],
                 [cic.integer_values(field_id, column, False)], n, None, shift_raw)
    assert [i for i, x in enumerate(want) if x == 0] == [7, 123]
    # and through a coefficient: beta * column + shift with shift = -beta * value
    beta = pow(3, 200, p)
    beta_raw = cic.element_raw(field_id, beta)
    shift_raw = cic.element_raw(field_id, p - beta * value % p)
    want = check(cpu_backend, field_id, [(column, False)],
                 [cic.integer_values(field_id, column, False)], n, [beta_raw], shift_raw)
    assert [i for i, x in enumerate(want) if x == 0] == [7, 123]


@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("n", [1, 5, 700])
def test_every_denominator_zero(cpu_backend, field_id, n):
    """no shift over a zero column (n = 0, data = NULL): every output row is zero"""
    empty = np.zeros((0, 8), np.uint8)
    for outputs in ("inverses", "scalars", "both"):
        inverses, scalars = invert(cpu_backend, field_id, [(empty, True)], n, None, None, outputs)
        for rows in (inverses, scalars):
            assert rows is None or not rows.any()


#--------------------------------------------------------------------------------------------------
# aborts (host backend only; each in a child process)
#--------------------------------------------------------------------------------------------------
SETUP = ("lib = api.load()\n"
         "col = np.arange(8, dtype=np.int64); buf = np.zeros((16, 32), np.uint8)\n"
         "out = np.zeros((16, 32), np.uint8); sc = np.zeros((16, 32), np.uint8)\n"
         "C, B, O, S = (a.ctypes.data for a in (col, buf, out, sc))\n"
         "def desc(*ds):\n"
         "    a = (api.sxt_sequence_descriptor * max(1, len(ds)))()\n"
         "    for i, d in enumerate(ds):\n"
         "        a[i] = api.sxt_sequence_descriptor(*d)\n"
         "    return a\n"
         "def call(inverses, scalars, descs, count, n, coefficients=None, shift=None, field=0):\n"
         "    v = api.bzamd_column_inversion(descs, coefficients, shift, count, n)\n"
         "    lib.bzamd_invert_columns(inverses, scalars, field, ctypes.byref(v))\n"
         "one = desc((8, 8, C, 1))\n")
ABORTS = {
    "null_v": ("lib.bzamd_invert_columns(O, S, 0, None)\n",
               "null argument to `bzamd_invert_columns`"),
    "null_columns": ("call(O, S, None, 1, 8)\n", "descriptors is null"),
    "both_outputs_null": ("call(None, None, one, 1, 8)\n",
                          "null argument to `bzamd_invert_columns`"),
    "width_33": ("call(O, S, desc((33, 8, B, 0)), 1, 8)\n", "element_nbytes must be in [1, 32]"),
    "width_0": ("call(O, S, desc((0, 8, B, 0)), 1, 8)\n", "element_nbytes must be in [1, 32]"),
    "signed_17": ("call(O, S, desc((17, 8, B, 1)), 1, 8)\n",
                  "signed sequences need element_nbytes <= 16"),
    "null_data": ("call(O, S, desc((8, 8, None, 1)), 1, 8)\n",
                  "descriptor has n > 0 but null data"),
    "column_longer_than_n": ("call(O, S, one, 1, 7)\n", "an inverted column is longer than n"),
    "n_0": ("call(O, S, desc((8, 0, None, 1)), 1, 0)\n", "needs 1 <= n <= 2^30"),
    "n_above_2_pow_30": ("call(O, S, one, 1, 2**30 + 1)\n", "needs 1 <= n <= 2^30"),
    "no_columns": ("call(O, S, one, 0, 8)\n", "needs 1 <= num_columns <= 32"),
    "33_columns": ("call(O, S, desc(*[(8, 8, C, 1)] * 33), 33, 8)\n",
                   "needs 1 <= num_columns <= 32"),
    "misaligned_inverses": ("call(O + 4, S, one, 1, 8)\n", "must be 8-byte aligned"),
    "misaligned_scalars": ("call(O, S + 4, one, 1, 8)\n", "must be 8-byte aligned"),
    "inverses_overlap_a_column": ("call(C + 8, S, one, 1, 8)\n", "an output overlaps an input"),
    "scalars_overlap_a_column": ("call(O, B + 32, desc((32, 8, B, 0)), 1, 8)\n",
                                 "an output overlaps an input"),
    "output_overlaps_coefficients": ("call(B, S, one, 1, 8, coefficients=B + 8 * 32 - 1)\n",
                                     "an output overlaps an input"),
    "output_overlaps_shift": ("call(O, B, one, 1, 8, shift=B + 40)\n",
                              "an output overlaps an input"),
    "outputs_overlap": ("call(O, O + 7 * 32, one, 1, 8)\n",
                        "the outputs of the column inversion overlap"),
    "field_2": ("call(O, S, one, 1, 8, field=2)\n", "unsupported field id"),
    "device_form_on_cpu": ("api.invert_columns_device(0, O, S, [(C, 8, 8, True)], None, None, 8)\n",
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


KERNELS = ("k_invert_columns",)


@pytest.mark.skipif(_hipcc() is None, reason="hipcc is not installed")
def test_kernels_use_no_scratch(tmp_path):
    """the compiler's own resource report of proof/column_inverse.hip with the flags the library is
    built with: every kernel of the file, both fields"""
    from blitzar_amd import build
    src = "proof/column_inverse.hip"
    assert src in build.SOURCES
    r = subprocess.run([_hipcc(), *build.FLAGS, *build.TU_FLAGS.get(src, []), "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(build.CSRC, src), "-o", str(tmp_path / "column_inverse.o")],
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
    assert len(scratch) == 2 * len(KERNELS), sorted(scratch)
    for kernel in KERNELS:
        found = {k: v for k, v in scratch.items() if kernel in k}
        assert len(found) == 2, f"{kernel}: found {sorted(found)}"
        assert all(v == 0 for v in found.values()), found
