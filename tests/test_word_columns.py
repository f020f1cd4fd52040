"""The word columns of a range check (include/blitzar_amd.h: bzamd_decompose_words,
bzamd_map_words), host forms on the host backend, with the aborts, the kernels' resources and the
stand-alone check of the plain-C++ half (tests/native/word_columns_check.cc, built here plain and
under the address and undefined-behaviour sanitizers).

Every expected value is Python integers (tests/word_column_cases.py).  The device forms and the
host forms on the gpu backend are in tests/test_word_columns_device.py."""
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
from tests import word_column_cases as wc
from tests.test_sumcheck_device import MODULUS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = wc.CANARY


def decompose(lib_api, field_id, column, num_words, shift=None, gap=0,
              outputs=("words", "counts", "overflow"), **skews):
    """bzamd_decompose_words through ctypes on one flat buffer (wc.Layout): the outputs asked for,
    the canaries everywhere else and the inputs are checked against the model -> the model's
    (words, counts, overflow)"""
    layout = wc.Layout(column, num_words, shift, gap, **skews)
    words, counts, overflow, col, shift_ptr = layout.pointers(layout.flat.ctypes.data, outputs)
    d = api.bzamd_word_decomposition(
        api.sxt_sequence_descriptor(col[2], col[1], col[0], 1 if col[3] else 0), shift_ptr,
        num_words, layout.plane_stride)
    lib_api.load().bzamd_decompose_words(words, counts, overflow, field_id, ctypes.byref(d))
    want = wc.decompose(wc.keys_of(field_id, column, shift), num_words)
    layout.check(layout.flat, want, outputs)
    return want


#--------------------------------------------------------------------------------------------------
# decompose: host form against the model
#--------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("width", range(1, 33))
def test_every_width(cpu_backend, field_id, width):
    """unsigned and (up to 16 bytes) signed, the extremes among the values: all 32 words, and as
    many words as the column is wide.  Negative rows are p - |x|: they overflow any num_words
    below 32"""
    p = MODULUS[field_id]
    rng = np.random.default_rng(100 * width + field_id)
    for signed in ([False, True] if width <= 16 else [False]):
        values = wc.drawn(rng, 40, width, signed)
        if width == 32:
            values += [p - 1, p - 2, -5, 1 << 200]
        column = wc.column_of(field_id, values, width, signed)
        words, counts, overflow = decompose(cpu_backend, field_id, column, 32)
        assert overflow == 0
        words, counts, overflow = decompose(cpu_backend, field_id, column, min(width, 31))
        negative = sum(1 for v in values if v < 0)
        if width < 32:
            assert overflow == negative and (not signed or negative > 0)
        else:
            assert overflow >= 3


@pytest.mark.parametrize("field_id", [0, 1])
def test_negative_rows_and_the_shift(cpu_backend, field_id):
    """without a shift a negative i64 is p - |x| and its words are that integer's bytes; with the
    shift 2^63 every i64 fits eight words"""
    p = MODULUS[field_id]
    values = [-1, -(1 << 63), (1 << 63) - 1, 0, 5, -77, 1 << 40]
    column = wc.column_of(field_id, values, 8, True)
    words, counts, overflow = decompose(cpu_backend, field_id, column, 8)
    assert overflow == 3
    assert bytes(words[:, 0]) == (p - 1).to_bytes(32, "little")[:8]
    assert bytes(words[:, 5]) == (p - 77).to_bytes(32, "little")[:8]
    shift = cic.element_raw(field_id, 1 << 63)
    words, counts, overflow = decompose(cpu_backend, field_id, column, 8, shift=shift)
    assert overflow == 0
    for i, v in enumerate(values):
        assert bytes(words[:, i]) == (v + (1 << 63)).to_bytes(8, "little")
    # the shift may be unreduced: the same words
    if shift + p < 1 << 256:
        again = decompose(cpu_backend, field_id, column, 8, shift=shift + p)
        assert np.array_equal(again[0], words) and again[2] == 0
    # i8 with the shift 128: one word each
    column = wc.column_of(field_id, [-128, 127, 0, -1], 1, True)
    words, counts, overflow = decompose(cpu_backend, field_id, column, 1,
                                        shift=cic.element_raw(field_id, 128))
    assert words.tolist() == [[0, 255, 128, 127]] and overflow == 0
    # a negative shift: 5 - 6 = p - 1
    words, counts, overflow = decompose(cpu_backend, field_id, wc.column_of(field_id, [5, 6, 7], 2),
                                        32, shift=cic.element_raw(field_id, p - 6))
    assert bytes(words[:, 0]) == (p - 1).to_bytes(32, "little") and words[:, 1].tolist() == [0] * 32
    assert words[0, 2] == 1


@pytest.mark.parametrize("field_id", [0, 1])
def test_unreduced_and_montgomery_rows(cpu_backend, field_id):
    """x and x + p in a 32-byte column give the same words; in field 1 the rows are Montgomery
    words and the words those of the plain integers"""
    p = MODULUS[field_id]
    values = [0, 1, 255, 256, 123456789, (1 << 64) - 1, 1 << 64, p - 1, (1 << 248) - 1]
    raw = [cic.element_raw(field_id, v) for v in values]
    reduced = (mc.rows_of(field_id, raw, 32, raw=True), False)
    lifted = (mc.rows_of(field_id, [r + p if r + p < 1 << 256 else r for r in raw], 32, raw=True),
              False)
    assert not np.array_equal(reduced[0], lifted[0])
    a = decompose(cpu_backend, field_id, reduced, 32)
    b = decompose(cpu_backend, field_id, lifted, 32)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    for i, v in enumerate(values):
        assert bytes(a[0][:, i]) == v.to_bytes(32, "little")
    # the largest 32 bytes
    top = (1 << 256) - 1
    words, _, _ = decompose(cpu_backend, field_id, (mc.rows_of(field_id, [top], 32, raw=True), False), 32)
    assert bytes(words[:, 0]) == cic.raw_value(field_id, top).to_bytes(32, "little")
    # the same values as a narrow column
    narrow = decompose(cpu_backend, field_id, wc.column_of(field_id, values[:7], 9), 32)
    assert np.array_equal(narrow[0], a[0][:, :7])


@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("num_words", [1, 31, 32])
def test_num_words(cpu_backend, field_id, num_words):
    p = MODULUS[field_id]
    values = [0, 255, 256, (1 << 248) - 1, 1 << 248, p - 1, 77]
    column = wc.column_of(field_id, values, 32)
    words, counts, overflow = decompose(cpu_backend, field_id, column, num_words)
    assert overflow == {1: 4, 31: 2, 32: 0}[num_words]
    assert words[0].tolist() == [v & 0xFF for v in values]


@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("w", [1, 2, 7, 8, 9, 15, 16, 17, 24, 31])
def test_either_side_of_overflow(cpu_backend, field_id, w):
    """keys 2^(8 w) - 1 and 2^(8 w) with w words, from a 32-byte column and, where it fits, from a
    narrow one with a shift that carries into the next word"""
    edge = 1 << (8 * w)
    column = wc.column_of(field_id, [edge - 1, edge, edge - 1, edge + 1, 0], 32)
    words, counts, overflow = decompose(cpu_backend, field_id, column, w)
    assert overflow == 2 and words[:, 0].tolist() == [255] * w and words[:, 1].tolist() == [0] * w
    narrow = wc.column_of(field_id, [edge - 2, edge - 1], w)
    words, counts, overflow = decompose(cpu_backend, field_id, narrow, w,
                                        shift=cic.element_raw(field_id, 1))
    assert overflow == 1 and words[:, 0].tolist() == [255] * w and words[:, 1].tolist() == [0] * w
    # without the shift the words above the width are zero by construction
    words, counts, overflow = decompose(cpu_backend, field_id, narrow, min(w + 3, 32))
    assert overflow == 0 and counts[0] == 2 * (min(w + 3, 32) - w)


@pytest.mark.parametrize("field_id", [0, 1])
def test_gaps_and_null_outputs(cpu_backend, field_id):
    """plane_stride > n: the bytes between the planes stay; each output NULL in turn, and alone"""
    rng = np.random.default_rng(3)
    column = wc.column_of(field_id, wc.drawn(rng, 37, 8, True), 8, True)
    shift = cic.element_raw(field_id, 1 << 63)
    for gap in (1, 13, 64):
        decompose(cpu_backend, field_id, column, 8, shift=shift, gap=gap)
    every = ("words", "counts", "overflow")
    for missing in every:
        decompose(cpu_backend, field_id, column, 9, shift=shift, gap=5,
                  outputs=tuple(o for o in every if o != missing))
        decompose(cpu_backend, field_id, column, 9, gap=5, outputs=(missing,))


@pytest.mark.parametrize("field_id", [0, 1])
def test_no_rows(cpu_backend, field_id):
    for width, signed in [(8, True), (32, False), (1, False)]:
        column = (np.zeros((0, width), np.uint8), signed)
        words, counts, overflow = decompose(cpu_backend, field_id, column, 8, gap=4)
        assert counts == [0] * 256 and overflow == 0


@pytest.mark.parametrize("field_id", [0, 1])
def test_wrappers(cpu_backend, field_id):
    values = np.array([-3, 5, 1 << 40, -(1 << 63)], np.int64)
    shift = mc.rows_of(field_id, [1 << 63], 32)[0]
    words, counts, overflow = cpu_backend.decompose_words(field_id, values, 8, shift=shift)
    assert words.shape == (8, 4) and overflow == 0 and int(counts.sum()) == 32
    for i, v in enumerate(values.tolist()):
        assert bytes(words[:, i]) == (v + (1 << 63)).to_bytes(8, "little")
    none, counts2, overflow = cpu_backend.decompose_words(field_id, values, 8, want_words=False)
    assert none is None and overflow == 2 and int(counts2.sum()) == 32
    table = wc.distinct_table()
    got = cpu_backend.map_words(words, table)
    assert got.shape == (8, 4, 32) and np.array_equal(got, wc.mapped(words, table))


#--------------------------------------------------------------------------------------------------
# map: host form against the model
#--------------------------------------------------------------------------------------------------
def map_words(lib_api, words, table, plane_gap=0, mapped_gap=0, skew=3):
    """bzamd_map_words through ctypes: planes `skew` bytes past a multiple of 16 and plane_gap bytes
    apart, the table at an odd address, mapped columns mapped_gap bytes apart; canaries and inputs
    checked -> uint8 [planes, n, 32]"""
    planes, n = words.shape
    plane_stride, mapped_stride = n + plane_gap, 32 * n + mapped_gap
    flat = np.full(64 + planes * plane_stride + 64 + 8192 + 64, CANARY, np.uint8)
    words_at = 48 + skew
    table_at = words_at + planes * plane_stride + 33
    for k in range(planes):
        flat[words_at + k * plane_stride:words_at + k * plane_stride + n] = words[k]
    flat[table_at:table_at + 8192] = table.reshape(-1)
    before = flat.copy()
    out = np.full(planes * mapped_stride + 16, CANARY, np.uint8)
    assert out.ctypes.data % 8 == 0
    m = api.bzamd_word_map(flat.ctypes.data + words_at, flat.ctypes.data + table_at, planes, n,
                           plane_stride, mapped_stride)
    lib_api.load().bzamd_map_words(out.ctypes.data + 8, ctypes.byref(m))
    assert np.array_equal(flat, before), "an input was modified"
    got = np.zeros((planes, n, 32), np.uint8)
    expected = np.full(out.shape, CANARY, np.uint8)
    want = wc.mapped(words, table)
    for k in range(planes):
        at = 8 + k * mapped_stride
        expected[at:at + 32 * n] = want[k].reshape(-1)
    assert np.array_equal(out, expected), "a mapped row is wrong or a byte outside was written"
    return want


@pytest.mark.parametrize("planes", [1, 32])
@pytest.mark.parametrize("n", [1, 17, 300])
def test_map(cpu_backend, planes, n):
    rng = np.random.default_rng(planes + n)
    words = rng.integers(0, 256, (planes, n), dtype=np.uint8)
    words[0, :min(n, 4)] = [0, 255, 1, 254][:min(n, 4)]
    table = wc.distinct_table()
    map_words(cpu_backend, words, table)
    map_words(cpu_backend, words, table, plane_gap=7, mapped_gap=24, skew=0)


#--------------------------------------------------------------------------------------------------
# aborts (host backend only; each in a child process)
#--------------------------------------------------------------------------------------------------
# every buffer lies in one allocation, 4 KiB or more from the next: what a case makes overlap is all
# that overlaps
SETUP = ("lib = api.load()\n"
         "memory = np.zeros(1 << 17, np.uint64)\n"
         "C, S, W, N, O, T, M = (memory.ctypes.data + (1 << 12) * k for k in (1, 2, 3, 4, 6, 8, 16))\n"
         "D = api.sxt_sequence_descriptor\n"
         "def call(w, c, o, column=(8, 16, C, 1), shift=None, num_words=8, stride=16, field=0):\n"
         "    d = api.bzamd_word_decomposition(D(*column), shift, num_words, stride)\n"
         "    lib.bzamd_decompose_words(w, c, o, field, ctypes.byref(d))\n"
         "def wmap(out, words=W, table=T, planes=4, n=16, stride=16, mapped_stride=512):\n"
         "    m = api.bzamd_word_map(words, table, planes, n, stride, mapped_stride)\n"
         "    lib.bzamd_map_words(out, ctypes.byref(m))\n")
ABORTS = {
    "null_d": ("lib.bzamd_decompose_words(W, N, O, 0, None)\n",
               "null argument to `bzamd_decompose_words`"),
    "all_outputs_null": ("call(None, None, None)\n", "null argument to `bzamd_decompose_words`"),
    "width_33": ("call(W, N, O, column=(33, 16, C, 0))\n", "element_nbytes must be in [1, 32]"),
    "width_0": ("call(W, N, O, column=(0, 16, C, 0))\n", "element_nbytes must be in [1, 32]"),
    "signed_17": ("call(W, N, O, column=(17, 4, C, 1))\n",
                  "signed sequences need element_nbytes <= 16"),
    "null_data": ("call(W, N, O, column=(8, 16, None, 1))\n", "descriptor has n > 0 but null data"),
    "rows_above_2_pow_30": ("call(None, N, O, column=(1, 2**30 + 1, C, 0), stride=2**30 + 1)\n",
                            "needs n <= 2^30"),
    "no_words": ("call(W, N, O, num_words=0)\n", "needs 1 <= num_words <= 32"),
    "33_words": ("call(W, N, O, num_words=33)\n", "needs 1 <= num_words <= 32"),
    "stride_below_n": ("call(W, N, O, stride=15)\n", "needs plane_stride >= n"),
    "misaligned_counts": ("call(W, N + 4, O)\n", "must be 8-byte aligned"),
    "misaligned_overflow": ("call(W, N, O + 4)\n", "must be 8-byte aligned"),
    "words_overlap_the_column": ("call(C + 127, N, O)\n", "an output overlaps an input"),
    "last_plane_overlaps_the_column": ("call(C - 7 * 16 - 15, N, O)\n",
                                       "an output overlaps an input"),
    "counts_overlap_the_column": ("call(W, C - 2040, O)\n", "an output overlaps an input"),
    "overflow_overlaps_the_shift": ("call(W, N, S + 24, shift=S)\n", "an output overlaps an input"),
    "words_overlap_the_shift": ("call(S - 127, N, O, shift=S)\n", "an output overlaps an input"),
    "words_overlap_counts": ("call(N + 2047, N, O)\n",
                             "the outputs of the word decomposition overlap"),
    "counts_overlap_overflow": ("call(W, N, N + 2040)\n",
                                "the outputs of the word decomposition overlap"),
    "words_overlap_overflow": ("call(O - 127, N, O)\n",
                               "the outputs of the word decomposition overlap"),
    "field_2": ("call(W, N, O, field=2)\n", "unsupported field id"),
    "device_form_on_cpu": ("api.decompose_words_device(0, W, N, O, (C, 16, 8, True), 8, 16)\n",
                           "device entry points need the GPU backend"),
    "map_null_m": ("lib.bzamd_map_words(M, None)\n", "null argument to `bzamd_map_words`"),
    "map_null_mapped": ("wmap(None)\n", "null argument to `bzamd_map_words`"),
    "map_null_words": ("wmap(M, words=None)\n", "null argument to `bzamd_map_words`"),
    "map_null_table": ("wmap(M, table=None)\n", "null argument to `bzamd_map_words`"),
    "map_no_rows": ("wmap(M, n=0, stride=0, mapped_stride=0)\n", "needs 1 <= n <= 2^30"),
    "map_rows_above_2_pow_30": ("wmap(M, n=2**30 + 1, stride=2**30 + 1, mapped_stride=2**35 + 32)\n",
                                "needs 1 <= n <= 2^30"),
    "map_no_planes": ("wmap(M, planes=0)\n", "needs 1 <= num_planes <= 32"),
    "map_33_planes": ("wmap(M, planes=33)\n", "needs 1 <= num_planes <= 32"),
    "map_stride_below_n": ("wmap(M, stride=15)\n", "needs plane_stride >= n"),
    "map_mapped_stride_below_32_n": ("wmap(M, mapped_stride=504)\n",
                                     "needs mapped_stride >= 32 n, a multiple of 8"),
    "map_mapped_stride_odd": ("wmap(M, mapped_stride=516)\n",
                              "needs mapped_stride >= 32 n, a multiple of 8"),
    "map_misaligned": ("wmap(M + 4)\n", "must be 8-byte aligned"),
    "map_overlaps_the_words": ("wmap(W + 56)\n", "an output overlaps an input"),
    "map_last_column_overlaps_the_table": ("wmap(T - 3 * 512 - 504)\n",
                                           "an output overlaps an input"),
    "map_device_form_on_cpu": ("api.map_words_device(M, W, T, 4, 16, 16, 512)\n",
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


# kernel -> instantiations: the clear and the map serve both fields
KERNELS = {"k_clear_words": 1, "k_decompose_words": 2, "k_map_words": 1}


@pytest.mark.skipif(_hipcc() is None, reason="hipcc is not installed")
def test_kernels_use_no_scratch(tmp_path):
    """the compiler's own resource report of proof/word_columns.hip with the flags the library is
    built with: every kernel of the file, both fields"""
    from blitzar_amd import build
    src = "proof/word_columns.hip"
    assert src in build.SOURCES
    r = subprocess.run([_hipcc(), *build.FLAGS, *build.TU_FLAGS.get(src, []), "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(build.CSRC, src), "-o", str(tmp_path / "word_columns.o")],
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


#--------------------------------------------------------------------------------------------------
# the plain-C++ half on its own: tests/native/word_columns_check.cc, plain and under sanitizers
#--------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def native_lines(tmp_path_factory):
    """the program's lines from a plain build and from one with -fsanitize=address,undefined
    (reports are fatal)"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ is not installed")
    out = tmp_path_factory.mktemp("word_columns_check")
    src = os.path.join(ROOT, "tests", "native", "word_columns_check.cc")
    lines = {}
    for name, flags in (("plain", ["-O2"]),
                        ("san", ["-O1", "-g", "-fsanitize=address,undefined",
                                 "-fno-sanitize-recover=all"])):
        exe = str(out / name)
        subprocess.run([gxx, *flags, "-std=c++20", "-I" + ROOT, src, "-o", exe], check=True,
                       timeout=600)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        lines[name] = [line for line in r.stdout.split("\n") if line]
    return lines


def _numbers(text, base=10):
    return [int(x, base) for x in text.split(",")] if text else []


def test_native_model_agrees_with_python(native_lines):
    """one line per case: the keys, and what model_decompose made of them, planes with a gap"""
    cases = [line for line in native_lines["plain"] if line.startswith("decompose ")]
    assert len(cases) >= 8
    seen = set()
    for line in cases:
        case = dict(f.split("=") for f in line.split()[1:])
        keys, num_words = _numbers(case["keys"], 16), int(case["num_words"])
        seen.add(num_words)
        words, counts, overflow = wc.decompose(keys, num_words)
        assert _numbers(case["words"], 16) == words.reshape(-1).tolist(), line
        assert _numbers(case["counts"]) == counts and int(case["overflow"]) == overflow, line
        assert case["gaps"] == "kept"
    assert {1, 8, 31, 32} <= seen


def test_native_map_and_edges(native_lines):
    lines = native_lines["plain"]
    assert "map planes=1 ok" in lines and "map planes=32 ok" in lines
    edges = dict(f.split("=") for f in [l for l in lines if l.startswith("overflow_edges")][0].split()[1:])
    assert edges == {str(w): "01" for w in range(1, 32)} | {"32": "00"}
    extent = [l for l in lines if l.startswith("extent")][0]
    assert extent == "extent 0 0 10 116 3072"


def test_native_clean_under_address_and_undefined_sanitizers(native_lines):
    assert native_lines["san"] == native_lines["plain"]
