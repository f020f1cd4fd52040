"""bzamd_prove_sumcheck_columns / bzamd_prove_sumcheck_device_columns (include/blitzar_amd.h): the
sumcheck prover over typed columns described by the MSM's descriptors -- little-endian integers of
1 .. 31 bytes, signed up to 16, or 32-byte field elements, each with its own length.

The expected side is always the reference's prover on the columns widened in Python integers
(v mod p, for field 1 times 2^256 mod p) and padded with zero rows to n: round polynomials and
evaluation point byte for byte, mle_evaluations against the fold written in Python integers
(tests/test_sumcheck_device.py).  Columns lie back to back in one buffer, every other one at an odd
address, so both ways of fetching an element are taken (aligned words, any bytes)."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from blitzar_amd import api
from tests.test_sumcheck import GK_P, L_ORDER, challenge_callback, elements, product_table
from tests.test_sumcheck_device import check_closing_identity, folded_evaluations, to_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULUS = {0: L_ORDER, 1: GK_P}

# the MLEs of every case: (width, signed, length) with the length one of 0, 1, "mid" (half the padded
# size), "mid+1", "n"; "zeros": a full-length column of zeros
MLES = [(1, False, "n"), (2, True, "mid+1"), (3, False, "mid"), (4, True, "n"), (8, True, "n"),
        (16, True, 1), (31, False, "n"), (32, False, "mid+1"), (8, False, "zeros"), (16, False, 0),
        (32, False, "n"), (1, True, "mid")]
PRODUCTS = {  # by round degree; LONG5 and LONG8 of tests/test_sumcheck_device.py are the models
    1: [[0], [4], [7], [11]],
    3: [[3, 4, 10], [6, 7], [9], [1, 8, 2], [5, 0, 11]],
    5: [[0, 1, 2, 3, 4], [5, 0], [3], [6, 7, 10], [11, 4, 4, 6]],
    6: [[0, 1, 2, 3, 4, 6], [7, 10], [8, 9, 5], [11]],
}
SMALL_N = [1, 2, 3, 5, 41]


#--------------------------------------------------------------------------------------------------
# inputs and the expected side
#--------------------------------------------------------------------------------------------------
def column_values(rng, width, signed, rows):
    """`rows` integers of `width` bytes, the extreme values first"""
    bits = 8 * width
    if signed:
        extremes = [-(1 << (bits - 1)), -1, (1 << (bits - 1)) - 1, 0, 1]
        low, high = -(1 << (bits - 1)), 1 << (bits - 1)
    else:
        extremes = [(1 << bits) - 1, (1 << (bits - 1)) - 1, 1 << (bits - 1), 0, 1]
        low, high = 0, 1 << bits
    values = []
    for i in range(rows):
        if i < len(extremes):
            values.append(extremes[i])
        else:
            raw = int.from_bytes(rng.integers(0, 256, width, dtype=np.uint8).tobytes(), "little")
            values.append(low + raw % (high - low))
    return values


class Case:
    """columns in one flat buffer, their descriptors, the widened matrix"""

    def __init__(self, field_id, n, degree, seed, mles=MLES):
        rng = np.random.default_rng(seed)
        p = MODULUS[field_id]
        self.field_id, self.n, self.degree = field_id, n, degree
        self.products = PRODUCTS[degree]
        mid = 1 << (max((n - 1).bit_length(), 1) - 1)
        lengths = {"n": n, "mid": min(mid, n), "mid+1": min(mid + 1, n), "zeros": n}
        self.specs, chunks, offset = [], [], 64  # guard bytes in front
        self.widened = np.zeros((len(mles), n, 32), np.uint8)
        for j, (width, signed, length) in enumerate(mles):
            rows = min(lengths.get(length, length), n)
            if width == 32:
                raw = elements(rng, field_id, rows)
                self.widened[j, :rows] = raw
            else:
                values = [0] * rows if length == "zeros" else column_values(rng, width, signed, rows)
                raw = np.zeros((rows, width), np.uint8)
                for i, v in enumerate(values):
                    raw[i] = np.frombuffer((v % (1 << (8 * width))).to_bytes(width, "little"), np.uint8)
                    self.widened[j, i] = to_bytes(field_id, v % p)
            # even columns at a multiple of 8, odd ones one byte past it
            offset = (offset + 7) // 8 * 8 + (j % 2)
            self.specs.append((offset, rows, width, signed))
            chunks.append((offset, raw))
            offset += rows * width
        self.flat = np.full(offset + 64, 0xA5, np.uint8)
        for start, raw in chunks:
            self.flat[start:start + raw.size] = raw.reshape(-1)
        self.lengths = [len(t) for t in self.products]
        self.terms = [i for t in self.products for i in t]
        self.mults = elements(rng, field_id, len(self.products))
        self.table = product_table(field_id, self.mults, self.lengths,
                                   api.SUMCHECK_PRODUCT_STRIDE[field_id])

    def host_columns(self, flat=None):
        flat = self.flat if flat is None else flat
        return [(flat[o:o + rows * w].reshape(rows, w), signed) for o, rows, w, signed in self.specs]

    def device_descriptors(self, base_ptr):
        return [(base_ptr + o, rows, w, signed) for o, rows, w, signed in self.specs]

    def want(self, oracle, log=None):
        return oracle.prove_sumcheck(self.field_id, self.widened, self.table, self.terms, self.n,
                                     self.degree, challenge_callback(self.field_id, [] if log is None else log))

    def check(self, oracle, got, want=None):
        want = self.want(oracle) if want is None else want
        assert np.array_equal(got[0], want[0]), "round polynomials differ"
        assert np.array_equal(got[1], want[1]), "evaluation points differ"
        assert np.array_equal(got[2], folded_evaluations(self.field_id, self.widened, got[1]))


def host_call(lib_api, case, flat=None):
    return lib_api.prove_sumcheck_columns(case.field_id, case.host_columns(flat), case.table,
                                          case.terms, case.n, case.degree,
                                          challenge_callback(case.field_id, []))


#--------------------------------------------------------------------------------------------------
# host backend
#--------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("degree", [1, 3, 5, 6])
@pytest.mark.parametrize("n", SMALL_N)
def test_host_columns_match_oracle(cpu_backend, oracle, field_id, degree, n):
    case = Case(field_id, n, degree, 1000 + 10 * n + degree)
    flat = case.flat.copy()
    case.check(oracle, host_call(cpu_backend, case))
    assert np.array_equal(case.flat, flat), "the columns were modified"


@pytest.mark.parametrize("field_id", [0, 1])
def test_numpy_integer_columns(cpu_backend, oracle, field_id):
    """what a caller holds: i64, i32, bool-as-u8 and one column of scalars, of unequal lengths"""
    rng = np.random.default_rng(1100 + field_id)
    n, p = 37, MODULUS[field_id]
    cols = [rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64),
            rng.integers(-2**31, 2**31 - 1, n - 4, dtype=np.int32),
            rng.integers(0, 2, n, dtype=np.uint8), elements(rng, field_id, 20),
            np.array([np.iinfo(np.int64).min, -1, np.iinfo(np.int64).max], np.int64)]
    widened = np.zeros((len(cols), n, 32), np.uint8)
    for j, c in enumerate(cols):
        for i in range(len(c)):
            widened[j, i] = c[i] if c.ndim == 2 else to_bytes(field_id, int(c[i]) % p)
    products = [[0, 1, 2], [3, 4], [2]]
    mults = elements(rng, field_id, len(products))
    table = product_table(field_id, mults, [len(t) for t in products],
                          api.SUMCHECK_PRODUCT_STRIDE[field_id])
    terms = [i for t in products for i in t]
    want = oracle.prove_sumcheck(field_id, widened, table, terms, n, 3,
                                 challenge_callback(field_id, []))
    got = cpu_backend.prove_sumcheck_columns(field_id, cols, table, terms, n, 3,
                                             challenge_callback(field_id, []))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], folded_evaluations(field_id, widened, got[1]))


@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("n", [1, 5, 41])
def test_full_width_columns_equal_the_matrix_form(cpu_backend, field_id, n):
    """all columns 32 bytes and full length: bzamd_prove_sumcheck byte for byte"""
    case = Case(field_id, n, 3, 1200 + n, mles=[(32, False, "n")] * 12)
    want = cpu_backend.prove_sumcheck_with_evaluations(field_id, case.widened, case.table,
                                                       case.terms, n, 3,
                                                       challenge_callback(field_id, []))
    got = host_call(cpu_backend, case)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("degree", [3, 6])
def test_columns_closing_identity(cpu_backend, field_id, degree):
    """what the verifier checks, from the inputs (widened here) and the outputs alone"""
    case = Case(field_id, 41, degree, 1300 + degree)
    polys, point, evaluations = host_call(cpu_backend, case)
    check_closing_identity(field_id, case.widened, case.mults, case.products, polys, point,
                           evaluations)


ABORTS = {
    "longer_than_n": ("c = [np.ones((3, 8), np.uint8)]\n", "a sumcheck column is longer than n"),
    "width_0": ("c = [np.ones((2, 0), np.uint8)]\n", "element_nbytes must be in [1, 32]"),
    "width_33": ("c = [np.ones((2, 33), np.uint8)]\n", "element_nbytes must be in [1, 32]"),
    "signed_32": ("c = [(np.ones((2, 32), np.uint8), True)]\n",
                  "signed sequences need element_nbytes <= 16"),
    "device_form_on_cpu": ("c = None\n", "device entry points need the GPU backend"),
}


@pytest.mark.parametrize("name", sorted(ABORTS))
def test_bad_columns_abort(name):
    setup, message = ABORTS[name]
    code = ("import numpy as np\nfrom blitzar_amd import api\napi.init(api.SXT_CPU_BACKEND, 0)\n"
            "t = np.zeros((1, 36), np.uint8)\nt[0, 0] = 1\nt[0, 32] = 1\n" + setup +
            "if c is None:\n"
            "    m = np.ones((2, 8), np.uint8)\n"
            "    api.prove_sumcheck_device_columns(0, [(m.ctypes.data, 2, 8, False)], t, [0], 2, 1,\n"
            "                                      lambda *a: None)\n"
            "else:\n"
            "    api.prove_sumcheck_columns(0, c, t, [0], 2, 1, lambda *a: None)\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode < 0 and message in r.stderr, r.stderr


def _hipcc():
    from blitzar_amd import build
    return build.HIPCC if os.path.exists(build.HIPCC) else shutil.which("hipcc")


@pytest.mark.skipif(_hipcc() is None, reason="hipcc is not installed")
def test_column_round_kernels_use_no_scratch(tmp_path):
    """the compiler's own resource report, with the flags the library is built with: round 0 over
    typed columns for round degrees 1 .. 5 on both fields (k_sumcheck_columns_round) keeps the
    element conversion, the partial product and the round polynomial in registers"""
    from blitzar_amd import build
    src = "proof/sumcheck_columns.hip"
    assert src in build.SOURCES
    r = subprocess.run([_hipcc(), *build.FLAGS, *build.TU_FLAGS.get(src, []), "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(build.CSRC, src), "-o", str(tmp_path / "columns.o")],
                       capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-4000:]
    scratch, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name is not None:
            scratch[name] = int(m.group(1))
    print({k: v for k, v in scratch.items() if "k_sumcheck_columns" in k})
    fixed = {k: v for k, v in scratch.items() if "k_sumcheck_columns_round" in k}
    assert len(fixed) == 10, f"expected 5 round degrees x 2 fields, found {sorted(fixed)}"
    assert all(v == 0 for v in fixed.values()), fixed


#--------------------------------------------------------------------------------------------------
# GPU
#--------------------------------------------------------------------------------------------------
def _launches():
    return api.load().bzamd_kernel_launch_count()


def device_call(lib_api, case, d_flat, callback=None, stream=None):
    before = _launches()
    got = lib_api.prove_sumcheck_device_columns(
        case.field_id, case.device_descriptors(d_flat.data_ptr()), case.table, case.terms, case.n,
        case.degree, challenge_callback(case.field_id, []) if callback is None else callback,
        stream=stream)
    assert _launches() > before, "no kernel ran"
    return got


def _check_on_device(gpu_backend, oracle, case):
    import torch
    d_flat = torch.from_numpy(case.flat.copy()).to(torch.device("cuda", 0))
    assert d_flat.data_ptr() % 8 == 0
    want_log, got_log = [], []
    want = case.want(oracle, want_log)
    got = device_call(gpu_backend, case, d_flat, challenge_callback(case.field_id, got_log))
    case.check(oracle, got, want)
    assert got_log == want_log
    # the columns, the gaps between them and the guard bytes around them are only read
    assert np.array_equal(d_flat.cpu().numpy(), case.flat), "device memory was modified"


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("degree", [1, 3, 5, 6])
@pytest.mark.parametrize("n", SMALL_N)
def test_device_columns_match_oracle(gpu_backend, oracle, field_id, degree, n):
    _check_on_device(gpu_backend, oracle, Case(field_id, n, degree, 2000 + 10 * n + degree))


# one row past one and two round workgroups; 2^12 + 9; 128 workgroups (k_sumcheck_finish runs)
@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("n,degree", [(129, 6), (257, 5), ((1 << 12) + 9, 1), ((1 << 14) + 77, 3)])
def test_device_columns_across_workgroups(gpu_backend, oracle, field_id, n, degree):
    _check_on_device(gpu_backend, oracle, Case(field_id, n, degree, 2100 + degree))


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_device_columns_on_a_side_stream(gpu_backend, field_id):
    """the columns are filled by a copy enqueued on the caller's stream just before the call, behind
    enough work that it has not run yet when the call starts; no synchronise in between"""
    import torch
    dev = torch.device("cuda", 0)
    case = Case(field_id, 5000, 3, 2200)
    source = torch.from_numpy(case.flat.copy()).to(dev)
    want = device_call(gpu_backend, case, source.clone())
    a = torch.randn((4096, 4096), device=dev)
    d_flat = torch.zeros_like(source)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        for _ in range(20):
            a = torch.mm(a, a).clamp_(-1, 1)
        d_flat.copy_(source)
        got = device_call(gpu_backend, case, d_flat, stream=side.cuda_stream)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("n,degree", [(3, 3), (41, 6), (2300, 5)])
def test_host_columns_on_gpu_equal_device_columns(gpu_backend, oracle, field_id, n, degree):
    import torch
    case = Case(field_id, n, degree, 2300 + degree)
    before = _launches()
    host = host_call(gpu_backend, case)
    assert _launches() > before, "no kernel ran"
    d_flat = torch.from_numpy(case.flat.copy()).to(torch.device("cuda", 0))
    device = device_call(gpu_backend, case, d_flat)
    for h, d in zip(host, device):
        assert np.array_equal(h, d)
    case.check(oracle, host)


@pytest.mark.gpu
def test_commit_then_prove_over_one_descriptor_array(gpu_backend, oracle):
    """8-byte signed, 1-byte and 32-byte columns on the device: the same descriptor array goes to
    bzamd_msm_device_resident and then to the prover"""
    import torch
    lib, dev, field_id, n = api.load(), torch.device("cuda", 0), 0, 1000
    rng = np.random.default_rng(2400)
    p = MODULUS[field_id]
    cols = [(rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64).view(np.uint8).reshape(n, 8), True),
            (rng.integers(0, 256, (n - 300, 1), dtype=np.uint8), False),
            (elements(rng, field_id, n - 1), False)]
    gens = oracle.ristretto_generators(n)
    want_commitments = oracle.commit(0, cols, gens)
    widened = np.zeros((len(cols), n, 32), np.uint8)
    for j, (c, signed) in enumerate(cols):
        for i in range(len(c)):
            v = int.from_bytes(c[i].tobytes(), "little", signed=signed)
            widened[j, i] = c[i] if c.shape[1] == 32 else to_bytes(field_id, v % p)
    products = [[0, 1, 2], [2, 2], [0]]
    table = product_table(field_id, elements(rng, field_id, 3), [3, 2, 1],
                          api.SUMCHECK_PRODUCT_STRIDE[field_id])
    terms = [i for t in products for i in t]
    want = oracle.prove_sumcheck(field_id, widened, table, terms, n, 3,
                                 challenge_callback(field_id, []))

    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep = [torch.from_numpy(c.copy()).to(dev) for c, _ in cols]
    desc = (api.sxt_sequence_descriptor * len(cols))()
    for i, (c, signed) in enumerate(cols):
        desc[i] = api.sxt_sequence_descriptor(c.shape[1], len(c), keep[i].data_ptr(), int(signed))
    d_gens = torch.from_numpy(gens.copy()).to(dev)
    h = lib.bzamd_generators_new_device(0, ctypes.c_void_p(d_gens.data_ptr()), n, stream)
    out = torch.zeros((len(cols), 32), dtype=torch.uint8, device=dev)
    lib.bzamd_msm_device_resident(ctypes.c_void_p(out.data_ptr()), len(cols), desc, h, stream)
    # the same array, with no synchronise in between
    v = max((n - 1).bit_length(), 1)
    polys, point = np.zeros((v, 4, 32), np.uint8), np.zeros((v, 32), np.uint8)
    tb, tm = np.ascontiguousarray(table), np.ascontiguousarray(terms, dtype=np.uint32)
    columns = api.bzamd_sumcheck_columns(desc, tb.ctypes.data, tm.ctypes.data, n, len(cols), 3,
                                         tm.size, 3)
    fn = lib.bzamd_prove_sumcheck_device_columns
    vp = ctypes.c_void_p
    fn.argtypes = [vp, vp, vp, ctypes.c_uint, ctypes.POINTER(api.bzamd_sumcheck_columns),
                   api.SUMCHECK_CALLBACK, vp, vp]
    fn.restype = None
    before = _launches()
    fn(polys.ctypes.data, point.ctypes.data, None, field_id, ctypes.byref(columns),
       api.SUMCHECK_CALLBACK(challenge_callback(field_id, [])), None, stream)
    assert _launches() > before, "no kernel ran"
    torch.cuda.synchronize()
    lib.bzamd_generators_free(h)
    assert np.array_equal(out.cpu().numpy(), want_commitments)
    assert np.array_equal(polys, want[0]) and np.array_equal(point, want[1])


@pytest.mark.gpu
def test_callback_may_reenter_during_device_columns(gpu_backend, oracle):
    import torch
    case = Case(0, 300, 3, 2500)
    inner, seen = challenge_callback(0, []), []

    def callback(r_ptr, ctx, poly_ptr, length):
        # a blocking sxt_* call from inside the callback: sxt_curve25519_compute_pedersen_commitments
        seen.append(api.compute_pedersen_commitments(0, [(np.arange(5, dtype=np.uint8).reshape(5, 1),
                                                          False)]).copy())
        inner(r_ptr, ctx, poly_ptr, length)

    d_flat = torch.from_numpy(case.flat.copy()).to(torch.device("cuda", 0))
    got = device_call(gpu_backend, case, d_flat, callback)
    case.check(oracle, got)
    expected = oracle.commit(0, [(np.arange(5, dtype=np.uint8).reshape(5, 1), False)],
                             oracle.ristretto_generators(5))
    assert len(seen) == 9 and all(np.array_equal(s, expected) for s in seen)
