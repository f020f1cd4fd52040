"""From the sumcheck's outputs to the inner-product argument's inputs (include/blitzar_amd.h:
bzamd_mle_evaluation_vector, bzamd_combine_columns), host forms on the host backend.

Every expected value is plain Python integers mod l (field 0) or mod the Grumpkin modulus (field 1,
Montgomery form x 2^256 at the boundary, tests/test_sumcheck_device.py to_bytes / to_int), and every
comparison is of bytes.  The device forms and the chain through both provers are in
tests/test_mle_opening_device.py, which takes its inputs and expectations from here."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests.test_sumcheck_device import MODULUS, to_bytes, to_int

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


#--------------------------------------------------------------------------------------------------
# the evaluation vector
#--------------------------------------------------------------------------------------------------
def point_of(field_id, num_variables, seed):
    """r_0 .. r_{v-1} as integers: 0, 1 and p - 1 among random ones, at places that move with the seed"""
    p = MODULUS[field_id]
    rng = np.random.default_rng(seed)
    point = [int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % p
             for _ in range(num_variables)]
    for k, special in enumerate((p - 1, 1, 0)):
        if num_variables > k + 1 or (num_variables == 1 and k == seed % 3):
            point[(seed + 2 * k) % num_variables] = special
    return point


def point_bytes(field_id, point):
    return np.stack([to_bytes(field_id, r) for r in point])


def vector_entry(field_id, point, i):
    """prod_t (bit_{v-1-t}(i) ? r_t : 1 - r_t)"""
    p, v, out = MODULUS[field_id], len(point), 1
    for t, r in enumerate(point):
        out = out * (r if (i >> (v - 1 - t)) & 1 else 1 - r) % p
    return out


def expected_vector(field_id, point, n):
    """all n entries as integers, by doubling from the top bit down (Python integers)"""
    p, out = MODULUS[field_id], [1]
    for r in point:
        out = [x * f % p for x in out for f in (1 - r, r)]
        if len(out) >= 2 * n:
            # later bits only split entries further: entries past n - 1 never reach below n
            out = out[:n]
    return out[:n]


def as_bytes(field_id, values):
    return np.stack([to_bytes(field_id, v % MODULUS[field_id]) for v in values])


VECTOR_CASES = [(1, 1), (1, 2), (2, 3), (5, 3), (3, 8), (10, 513)]


def test_expected_vector_helper_agrees_with_the_definition():
    for field_id in (0, 1):
        point = point_of(field_id, 6, 11)
        assert expected_vector(field_id, point, 37) == [vector_entry(field_id, point, i)
                                                        for i in range(37)]


@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("v,n", VECTOR_CASES)
def test_evaluation_vector_host_form(cpu_backend, field_id, v, n):
    for seed in (0, 1, 2):
        point = point_of(field_id, v, seed)
        got = cpu_backend.mle_evaluation_vector(field_id, point_bytes(field_id, point), n)
        assert np.array_equal(got, as_bytes(field_id, expected_vector(field_id, point, n)))
    if (v, n) == (1, 1):
        assert to_int(field_id, got[0]) == (1 - point[0]) % MODULUS[field_id]


@pytest.mark.parametrize("field_id", [0, 1])
def test_evaluation_vector_opens_a_fold(cpu_backend, field_id):
    """<f, vector> is the fold of f by the point's challenges, top bit first (the recurrence above
    bzamd_prove_sumcheck)"""
    p, v, n = MODULUS[field_id], 4, 11
    rng = np.random.default_rng(5)
    f = [int(x) for x in rng.integers(0, 2**62, n)]
    point = point_of(field_id, v, 7)
    vector = cpu_backend.mle_evaluation_vector(field_id, point_bytes(field_id, point), n)
    row = f + [0] * ((1 << v) - n)
    for t, r in enumerate(point):
        mid = 1 << (v - 1 - t)
        row = [((1 - r) * row[i] + r * row[mid + i]) % p for i in range(mid)]
    assert sum(x * to_int(field_id, b) for x, b in zip(f, vector)) % p == row[0]


#--------------------------------------------------------------------------------------------------
# the combination
#--------------------------------------------------------------------------------------------------
KINDS = [(1, False), (2, True), (8, True), (16, True), (31, False), (32, False)]


def element_value(field_id, raw):
    """what 32 bytes of a column mean, unreduced values included"""
    p = MODULUS[field_id]
    v = int.from_bytes(bytes(raw), "little")
    return v * pow(1 << 256, -1, p) % p if field_id == 1 else v % p


class Columns:
    """num_columns typed columns for a combination over n rows: column j has the width and sign
    KINDS[j % 6] and the length (n, n - 1, 1, 0)[(j + shift) % 4] (0: a null pointer), extreme
    values first, so shifts 0 .. 3 give every kind every length.  `flat`: one buffer that holds
    every column behind a guard, column j at an address that is (0, 1, 3)[(j + j // 6 + shift) % 3]
    past a multiple of 8 (1, 3: the byte path; 0: the word path for widths 8, 16 and 32), for the
    device forms; `specs`: (offset, rows, width, signed); `values[j]`: the rows as field integers"""

    def __init__(self, field_id, n, num_columns, seed, shift=0):
        p = MODULUS[field_id]
        rng = np.random.default_rng(seed)
        self.field_id, self.n = field_id, n
        self.arrays, self.specs, self.values = [], [], []
        lengths = [n, n - 1, 1, 0]
        at = 64
        for j in range(num_columns):
            width, signed = KINDS[j % len(KINDS)]
            rows = lengths[(j + shift) % 4]
            data = rng.integers(0, 256, (rows, width), dtype=np.uint8)
            if width == 32 and field_id == 1:
                for i in range(rows):  # mostly canonical elements
                    data[i] = to_bytes(field_id, element_value(0, data[i]) % p)
            extremes = []
            if signed:
                low = -(1 << (8 * width - 1))
                extremes = [low.to_bytes(width, "little", signed=True),
                            (-1).to_bytes(width, "little", signed=True),
                            (-low - 1).to_bytes(width, "little", signed=True)]
            elif width == 32:
                top = (1 << 256) - 1 if field_id == 0 else p + 5  # unreduced
                extremes = [top.to_bytes(32, "little"), (p - 1).to_bytes(32, "little")]
            else:
                extremes = [b"\xff" * width, b"\x00" * width]
            for i, e in enumerate(extremes[:rows]):
                data[i] = np.frombuffer(e, np.uint8)
            if width == 32:
                values = [element_value(field_id, data[i]) for i in range(rows)]
            else:
                values = [int.from_bytes(data[i].tobytes(), "little", signed=signed) % p
                          for i in range(rows)]
            at = (at + 7) // 8 * 8 + (0, 1, 3)[(j + j // 6 + shift) % 3]
            self.arrays.append((data, signed))
            self.specs.append((at, rows, width, signed))
            self.values.append(values)
            at += rows * width + 8
        self.flat = np.full(at + 64, 0xA5, np.uint8)
        for (data, _), (offset, rows, width, _) in zip(self.arrays, self.specs):
            self.flat[offset:offset + rows * width] = data.reshape(-1)
        # 0, 1 and p - 1 among random coefficients, on columns that move with the shift
        self.coefficients = [int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(),
                                            "little") % p for _ in range(num_columns)]
        for k, special in enumerate((p - 1, 1, 0)):
            if num_columns > k + 1:
                self.coefficients[(shift + 5 * k) % num_columns] = special
        self.evaluations = [int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(),
                                           "little") % p for _ in range(num_columns)]

    def host_columns(self):
        return [(data.copy(), signed) for data, signed in self.arrays]

    def device_descriptors(self, base_ptr):
        return [(base_ptr + o, rows, w, signed) for o, rows, w, signed in self.specs]

    def coefficient_bytes(self):
        return as_bytes(self.field_id, self.coefficients)

    def evaluation_bytes(self):
        return as_bytes(self.field_id, self.evaluations)

    def expected_combined(self):
        p = MODULUS[self.field_id]
        out = [0] * self.n
        for c, values in zip(self.coefficients, self.values):
            for i, x in enumerate(values):
                out[i] = (out[i] + c * x) % p
        return as_bytes(self.field_id, out)

    def expected_product(self):
        total = sum(c * e for c, e in zip(self.coefficients, self.evaluations))
        return to_bytes(self.field_id, total % MODULUS[self.field_id])


@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 257])
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_combination_host_form(cpu_backend, field_id, n, shift):
    """six columns, one of every kind; the four shifts put every length on every kind and the
    special coefficients on different columns"""
    case = Columns(field_id, n, len(KINDS), 20 + shift, shift)
    columns = case.host_columns()
    product = np.full(32, 0x5A, np.uint8)
    combined, _ = cpu_backend.combine_columns(field_id, columns, case.coefficient_bytes(), n,
                                              case.evaluation_bytes(), product)
    assert np.array_equal(combined, case.expected_combined())
    assert np.array_equal(product, case.expected_product())
    for (got, _), (want, _) in zip(columns, case.arrays):
        assert np.array_equal(got, want), "a column was modified"


@pytest.mark.parametrize("field_id", [0, 1])
def test_every_length_of_every_kind(field_id):
    """the shifts of test_combination_host_form cover kinds x lengths, and for the device forms
    kinds x the three placements"""
    seen, placed = set(), set()
    for shift in (0, 1, 2, 3):
        case = Columns(field_id, 257, len(KINDS), 20 + shift, shift)
        seen |= {(w, s, rows) for _, rows, w, s in case.specs}
        placed |= {(w, o % 8) for o, _, w, _ in case.specs}
    assert seen == {(w, s, rows) for w, s in KINDS for rows in (257, 256, 1, 0)}
    assert placed == {(w, o) for w, _ in KINDS for o in (0, 1, 3)}


@pytest.mark.parametrize("field_id", [0, 1])
def test_product_is_written_only_with_evaluations(cpu_backend, field_id):
    case = Columns(field_id, 5, 3, 40)
    product = np.full(32, 0x5A, np.uint8)
    combined, _ = cpu_backend.combine_columns(field_id, case.host_columns(),
                                              case.coefficient_bytes(), 5, None, product)
    assert np.array_equal(combined, case.expected_combined())
    assert np.all(product == 0x5A), "product was written without evaluations"
    # and no product asked for: nothing to write to
    combined, _ = cpu_backend.combine_columns(field_id, case.host_columns(),
                                              case.coefficient_bytes(), 5, case.evaluation_bytes())
    assert np.array_equal(combined, case.expected_combined())


@pytest.mark.parametrize("field_id", [0, 1])
def test_many_columns_host_form(cpu_backend, field_id):
    case = Columns(field_id, 9, 33, 50)
    combined, _ = cpu_backend.combine_columns(field_id, case.host_columns(),
                                              case.coefficient_bytes(), 9)
    assert np.array_equal(combined, case.expected_combined())


#--------------------------------------------------------------------------------------------------
# aborts (host backend only; each in a child process)
#--------------------------------------------------------------------------------------------------
VECTOR_CALL = "api.mle_evaluation_vector(0, np.zeros((v, 32), np.uint8), n, num_variables=v)\n"
ABORTS = {
    "n_above_2_pow_v": ("v, n = 2, 5\n" + VECTOR_CALL, "needs 1 <= n <= 2^num_variables"),
    "n_zero": ("v, n = 2, 0\n" + VECTOR_CALL, "needs 1 <= n <= 2^num_variables"),
    "v_0": ("v, n = 0, 1\n" + VECTOR_CALL, "needs 1 <= num_variables <= 30"),
    "v_31": ("v, n = 31, 1\n" + VECTOR_CALL, "needs 1 <= num_variables <= 30"),
    "null_vector": ("p = np.zeros((1, 32), np.uint8)\n"
                    "api.load().bzamd_mle_evaluation_vector(None, 0, p.ctypes.data, 1, 1)\n",
                    "null argument to `bzamd_mle_evaluation_vector`"),
    "null_point": ("out = np.zeros((1, 32), np.uint8)\n"
                   "api.load().bzamd_mle_evaluation_vector(out.ctypes.data, 0, None, 1, 1)\n",
                   "null argument to `bzamd_mle_evaluation_vector`"),
    "field_2": ("api.mle_evaluation_vector(2, np.zeros((1, 32), np.uint8), 1)\n",
                "unsupported field id"),
    "misaligned_vector": ("out, p = np.zeros(72, np.uint8), np.zeros((1, 32), np.uint8)\n"
                          "at = out.ctypes.data + 8 - out.ctypes.data % 8 + 4\n"
                          "api.load().bzamd_mle_evaluation_vector(at, 0, p.ctypes.data, 1, 1)\n",
                          "must be 8-byte aligned"),
    "column_longer_than_n": ("c = np.zeros((1, 32), np.uint8)\n"
                             "api.combine_columns(0, [np.ones((3, 8), np.uint8)], c, 2)\n",
                             "a combined column is longer than n"),
    "no_columns": ("api.combine_columns(0, [], np.zeros((1, 32), np.uint8), 2)\n",
                   "needs at least one column"),
    "width_33": ("c = np.zeros((1, 32), np.uint8)\n"
                 "api.combine_columns(0, [np.ones((2, 33), np.uint8)], c, 2)\n",
                 "element_nbytes must be in [1, 32]"),
    "device_form_on_cpu": ("out = np.zeros((2, 32), np.uint8)\n"
                           "api.mle_evaluation_vector_device(0, out.ctypes.data, out.ctypes.data, 1, 2)\n",
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
    built with: the evaluation vector, the combination and its product, both fields"""
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
    for kernel in ("k_mle_evaluation_vector", "k_combine_columns", "k_combine_product"):
        found = {k: v for k, v in scratch.items() if kernel in k}
        assert len(found) == 2, f"{kernel}: found {sorted(found)}"
        assert all(v == 0 for v in found.values()), found
