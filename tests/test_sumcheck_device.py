"""bzamd_prove_sumcheck / bzamd_prove_sumcheck_device (include/blitzar_amd.h): the sumcheck prover
that also returns the value of every MLE at the evaluation point, and its form on device-resident
tables.  Round polynomials and evaluation point against the reference's prover (byte-identical),
mle_evaluations against a fold written here in Python integers, the verifier's closing identity
from the inputs and the library's outputs alone, and the compiler's resource report for the round
kernels (no scratch memory for product lengths <= 5)."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from blitzar_amd import api
from tests.test_sumcheck import CASES, GK_P, L_ORDER, challenge_callback, elements, product_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULUS = {0: L_ORDER, 1: GK_P}
LONG8 = (19, 8, [[0, 1, 2, 3, 4, 5, 6, 7], [1, 2]])            # a product of length 8
LONG5 = (41, 6, [[0, 1, 2, 3, 4], [5, 0], [3]])                # round degree 5
HOST_CASES = CASES + [LONG8, LONG5]
MIXED = ((1 << 12) + 1, 8, [[0], [1, 2], [0, 3, 4, 5, 6], [0, 1, 2, 3, 4, 5, 6, 7]])
DEVICE_CASES = HOST_CASES + [((1 << 14) + 77, 4, [[0, 1, 2], [3, 1], [2]]), MIXED,
                             ((1 << 12) + 9, 6, [[0, 1, 2, 3, 4], [5, 0], [3]])]


#--------------------------------------------------------------------------------------------------
# inputs and the expected side, in Python integers
#--------------------------------------------------------------------------------------------------
def make_inputs(field_id, n, num_mles, products, seed):
    rng = np.random.default_rng(seed)
    mles = elements(rng, field_id, n * num_mles).reshape(num_mles, n, 32)
    lengths = [len(t) for t in products]
    terms = [i for t in products for i in t]
    mults = elements(rng, field_id, len(products))
    table = product_table(field_id, mults, lengths, api.SUMCHECK_PRODUCT_STRIDE[field_id])
    return mles, mults, table, terms, max(lengths)


def to_int(field_id, raw):
    """the field element behind 32 bytes of the caller's representation"""
    p = MODULUS[field_id]
    v = int.from_bytes(bytes(raw), "little")
    assert v < p, "not canonical"
    if field_id == 1:
        v = v * pow(1 << 256, -1, p) % p  # out of Montgomery form, R = 2^256
    return v


def to_bytes(field_id, v):
    p = MODULUS[field_id]
    if field_id == 1:
        v = v * (1 << 256) % p
    return np.frombuffer(v.to_bytes(32, "little"), np.uint8)


def folded_evaluations(field_id, mles, point):
    """T_v[j][0] of the issue's recurrence, as bytes [num_mles, 32]"""
    p = MODULUS[field_id]
    num_mles, n = mles.shape[0], mles.shape[1]
    v = max((n - 1).bit_length(), 1)
    assert point.shape[0] == v
    out = np.zeros((num_mles, 32), np.uint8)
    for j in range(num_mles):
        row = [to_int(field_id, mles[j, i]) for i in range(n)] + [0] * ((1 << v) - n)
        for t in range(v):
            r = to_int(field_id, point[t])
            mid = 1 << (v - 1 - t)
            row = [((1 - r) * row[i] + r * row[mid + i]) % p for i in range(mid)]
        out[j] = to_bytes(field_id, row[0])
    return out


def evaluate(field_id, coefficients, x):
    p = MODULUS[field_id]
    acc = 0
    for c in reversed([to_int(field_id, c) for c in coefficients]):
        acc = (acc * x + c) % p
    return acc


def check_closing_identity(field_id, mles, mults, products, polys, point, evaluations):
    """what the verifier checks, from the inputs and the prover's outputs alone"""
    p = MODULUS[field_id]
    num_mles, n = mles.shape[0], mles.shape[1]
    m = [to_int(field_id, x) for x in mults]
    claimed = 0
    for row in range(n):
        values = [to_int(field_id, mles[j, row]) for j in range(num_mles)]
        for mult, terms in zip(m, products):
            term = mult
            for j in terms:
                term = term * values[j] % p
            claimed = (claimed + term) % p
    expected = claimed
    for t in range(polys.shape[0]):
        assert (evaluate(field_id, polys[t], 0) + evaluate(field_id, polys[t], 1)) % p == expected, \
            f"round {t}: p(0) + p(1) is not the previous round's value"
        expected = evaluate(field_id, polys[t], to_int(field_id, point[t]))
    e = [to_int(field_id, x) for x in evaluations]
    final = 0
    for mult, terms in zip(m, products):
        term = mult
        for j in terms:
            term = term * e[j] % p
        final = (final + term) % p
    assert final == expected, "the MLE evaluations do not close the proof"


def raw_host_call(lib_api, field_id, mles, table, terms, n, degree, callback, with_evaluations):
    """bzamd_prove_sumcheck through ctypes, mle_evaluations NULL or not"""
    m = np.ascontiguousarray(mles, dtype=np.uint8)
    tb = np.ascontiguousarray(table, dtype=np.uint8)
    tm = np.ascontiguousarray(terms, dtype=np.uint32)
    v = max((n - 1).bit_length(), 1)
    polys = np.zeros((v, degree + 1, 32), np.uint8)
    point = np.zeros((v, 32), np.uint8)
    evaluations = np.zeros((m.shape[0], 32), np.uint8) if with_evaluations else None
    d = api.sumcheck_descriptor(m.ctypes.data, tb.ctypes.data, tm.ctypes.data, n, m.shape[0],
                                tb.size // api.SUMCHECK_PRODUCT_STRIDE[field_id], tm.size, degree)
    fn = lib_api.load().bzamd_prove_sumcheck
    vp = ctypes.c_void_p
    fn.argtypes = [vp, vp, vp, ctypes.c_uint, ctypes.POINTER(api.sumcheck_descriptor),
                   api.SUMCHECK_CALLBACK, vp]
    fn.restype = None
    fn(polys.ctypes.data, point.ctypes.data,
       None if evaluations is None else evaluations.ctypes.data, field_id, ctypes.byref(d),
       api.SUMCHECK_CALLBACK(callback), None)
    return polys, point, evaluations


#--------------------------------------------------------------------------------------------------
# host backend
#--------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("case", range(len(HOST_CASES)))
def test_host_form_matches_oracle(cpu_backend, oracle, field_id, case):
    n, num_mles, products = HOST_CASES[case]
    mles, _, table, terms, degree = make_inputs(field_id, n, num_mles, products, 300 + case)
    want = oracle.prove_sumcheck(field_id, mles, table, terms, n, degree,
                                 challenge_callback(field_id, []))
    for with_evaluations in (False, True):
        got = raw_host_call(cpu_backend, field_id, mles, table, terms, n, degree,
                            challenge_callback(field_id, []), with_evaluations)
        assert np.array_equal(got[0], want[0]), "round polynomials differ"
        assert np.array_equal(got[1], want[1]), "evaluation points differ"
    plain = cpu_backend.prove_sumcheck(field_id, mles, table, terms, n, degree,
                                       challenge_callback(field_id, []))
    assert np.array_equal(plain[0], want[0]) and np.array_equal(plain[1], want[1])


@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 5, 8, 37, 64])
def test_mle_evaluations_are_the_last_fold(cpu_backend, field_id, n):
    """n = 1 (one round, no partner), rows without a partner, powers of two"""
    products = [[0, 1, 2], [1], [2, 0]]
    mles, _, table, terms, degree = make_inputs(field_id, n, 3, products, 400 + n)
    polys, point, evaluations = cpu_backend.prove_sumcheck_with_evaluations(
        field_id, mles, table, terms, n, degree, challenge_callback(field_id, []))
    assert np.array_equal(evaluations, folded_evaluations(field_id, mles, point))


@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("case", range(len(HOST_CASES)))
def test_closing_identity(cpu_backend, field_id, case):
    n, num_mles, products = HOST_CASES[case]
    mles, mults, table, terms, degree = make_inputs(field_id, n, num_mles, products, 500 + case)
    polys, point, evaluations = cpu_backend.prove_sumcheck_with_evaluations(
        field_id, mles, table, terms, n, degree, challenge_callback(field_id, []))
    check_closing_identity(field_id, mles, mults, products, polys, point, evaluations)


def test_cpu_backend_aborts_in_device_form():
    code = ("import numpy as np\nfrom blitzar_amd import api\napi.init(api.SXT_CPU_BACKEND, 0)\n"
            "m = np.ones((1, 2, 32), np.uint8)\nt = np.zeros((1, 36), np.uint8)\nt[0, 0] = 1\n"
            "t[0, 32] = 1\n"
            "api.prove_sumcheck_device(0, m.ctypes.data, 1, t, [0], 2, 1, lambda *a: None)\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode < 0 and "device entry points need the GPU backend" in r.stderr, r.stderr


def _hipcc():
    from blitzar_amd import build
    return build.HIPCC if os.path.exists(build.HIPCC) else shutil.which("hipcc")


@pytest.mark.skipif(_hipcc() is None, reason="hipcc is not installed")
def test_round_kernels_use_no_scratch(tmp_path):
    """the compiler's own resource report, with the flags the library is built with: every
    instantiation of the round kernel that serves product lengths <= 5 (k_sumcheck_round_fixed,
    round degrees 1 .. 5, both fields) keeps its partial product and round polynomial in registers"""
    from blitzar_amd import build
    src = "proof/sumcheck.hip"
    r = subprocess.run([_hipcc(), *build.FLAGS, *build.TU_FLAGS.get(src, []), "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(build.CSRC, src), "-o", str(tmp_path / "sumcheck.o")],
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
    fixed = {k: v for k, v in scratch.items() if "k_sumcheck_round_fixed" in k}
    print({k: v for k, v in scratch.items() if "k_sumcheck_round" in k})
    assert len(fixed) == 10, f"expected 5 round degrees x 2 fields, found {sorted(fixed)}"
    assert all(v == 0 for v in fixed.values()), fixed


#--------------------------------------------------------------------------------------------------
# GPU
#--------------------------------------------------------------------------------------------------
def _launches():
    return api.load().bzamd_kernel_launch_count()


def _device_call(lib_api, field_id, d_mles, num_mles, table, terms, n, degree, callback, stream=None):
    before = _launches()
    got = lib_api.prove_sumcheck_device(field_id, d_mles.data_ptr(), num_mles, table, terms, n,
                                        degree, callback, stream=stream)
    assert _launches() > before, "no kernel ran"
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("case", range(len(DEVICE_CASES)))
def test_device_form_matches_oracle(gpu_backend, oracle, field_id, case):
    import torch
    n, num_mles, products = DEVICE_CASES[case]
    mles, mults, table, terms, degree = make_inputs(field_id, n, num_mles, products, 600 + case)
    want_log, got_log = [], []
    want = oracle.prove_sumcheck(field_id, mles, table, terms, n, degree,
                                 challenge_callback(field_id, want_log))
    d_mles = torch.from_numpy(mles.copy()).to(torch.device("cuda", 0))
    polys, point, evaluations = _device_call(gpu_backend, field_id, d_mles, num_mles, table, terms,
                                             n, degree, challenge_callback(field_id, got_log))
    assert np.array_equal(polys, want[0]), "round polynomials differ"
    assert np.array_equal(point, want[1]), "evaluation points differ"
    assert got_log == want_log
    assert np.array_equal(evaluations, folded_evaluations(field_id, mles, point))
    # the caller's tables are only read
    assert np.array_equal(d_mles.cpu().numpy(), mles), "the device tables were modified"


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_device_tables_are_not_modified(gpu_backend, field_id):
    import torch
    n, num_mles, products = 3000, 4, [[0, 1, 2], [3, 1]]
    mles, mults, table, terms, degree = make_inputs(field_id, n, num_mles, products, 700)
    # guard rows around the tables: nothing next to them is written either
    guard = 64
    flat = np.full((guard + num_mles * n + guard, 32), 0xA5, np.uint8)
    flat[guard:guard + num_mles * n] = mles.reshape(-1, 32)
    d_flat = torch.from_numpy(flat.copy()).to(torch.device("cuda", 0))
    d_mles = d_flat[guard:guard + num_mles * n]
    polys, point, evaluations = _device_call(gpu_backend, field_id, d_mles, num_mles, table, terms,
                                             n, degree, challenge_callback(field_id, []))
    assert np.array_equal(d_flat.cpu().numpy(), flat)
    check_closing_identity(field_id, mles, mults, products, polys, point, evaluations)


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_device_form_on_a_side_stream(gpu_backend, field_id):
    """the tables are produced by a kernel enqueued on the caller's stream just before the call,
    behind enough work that it has not run yet when the call starts; no synchronise in between"""
    import torch
    dev = torch.device("cuda", 0)
    n, num_mles, products = 5000, 4, [[0, 1, 2], [3, 1], [2]]
    mles, _, table, terms, degree = make_inputs(field_id, n, num_mles, products, 800)
    source = torch.from_numpy(mles.copy()).to(dev)
    d_default = source.clone()
    want = _device_call(gpu_backend, field_id, d_default, num_mles, table, terms, n, degree,
                        challenge_callback(field_id, []))
    a = torch.randn((4096, 4096), device=dev)
    d_mles = torch.zeros_like(source)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        for _ in range(20):
            a = torch.mm(a, a).clamp_(-1, 1)
        d_mles.copy_(source)
        got = _device_call(gpu_backend, field_id, d_mles, num_mles, table, terms, n, degree,
                           challenge_callback(field_id, []), stream=side.cuda_stream)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("case", [3, 4, len(CASES), len(CASES) + 1])
def test_host_form_on_gpu_equals_device_form(gpu_backend, field_id, case):
    import torch
    n, num_mles, products = HOST_CASES[case]
    n = n + 2000  # several workgroups
    mles, mults, table, terms, degree = make_inputs(field_id, n, num_mles, products, 900 + case)
    before = _launches()
    host = gpu_backend.prove_sumcheck_with_evaluations(field_id, mles, table, terms, n, degree,
                                                       challenge_callback(field_id, []))
    assert _launches() > before, "no kernel ran"
    d_mles = torch.from_numpy(mles.copy()).to(torch.device("cuda", 0))
    device = _device_call(gpu_backend, field_id, d_mles, num_mles, table, terms, n, degree,
                          challenge_callback(field_id, []))
    for h, d in zip(host, device):
        assert np.array_equal(h, d)
    check_closing_identity(field_id, mles, mults, products, *host)
    plain = gpu_backend.prove_sumcheck(field_id, mles, table, terms, n, degree,
                                       challenge_callback(field_id, []))
    assert np.array_equal(plain[0], host[0]) and np.array_equal(plain[1], host[1])


@pytest.mark.gpu
def test_callback_may_reenter_during_device_form(gpu_backend, oracle):
    import torch
    field_id, n, num_mles, products = 0, 300, 3, [[0, 1], [2]]
    mles, _, table, terms, degree = make_inputs(field_id, n, num_mles, products, 77)
    inner, seen = challenge_callback(field_id, []), []

    def callback(r_ptr, ctx, poly_ptr, length):
        seen.append(api.get_one_commit(3).copy())  # a blocking sxt_* call from inside the callback
        inner(r_ptr, ctx, poly_ptr, length)

    want = oracle.prove_sumcheck(field_id, mles, table, terms, n, degree,
                                 challenge_callback(field_id, []))
    d_mles = torch.from_numpy(mles.copy()).to(torch.device("cuda", 0))
    got = _device_call(gpu_backend, field_id, d_mles, num_mles, table, terms, n, degree, callback)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert len(seen) == 9 and all(np.array_equal(s, oracle.one_commit(3)) for s in seen)
