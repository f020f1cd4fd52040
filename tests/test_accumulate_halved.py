"""k_accumulate<ed25519_niels_msm> on halved Z = 1 addends ((y+x)/2, (y-x)/2, d x y: curve/ed29.h,
add_niels / from_niels; msm/curve_traits.h, niels_of) with 32-bit piece offsets (msm/kernels.h,
accumulate_lds_gather): commitments through bzamd_msm_device on caller generators -- the caller
table normalises them to the stored form -- and through a resident set, against this library's
host backend on the same inputs.

The host backend's commitments come from ONE child process per module (sxt_init is per process and
the session's GPU backend stays as it is); every case asserts that kernels were launched.  The
64-bit piece addresses belong to tables beyond 2^25 rows (4 GiB), which no shape of a few seconds
reaches: that form is covered by the host model only (tests/test_niels_halved_host.py)."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import refmath as rm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = ctypes.c_void_p
ROWS = [1, 63, 64, 65, 2049, 4097]
KINDS = ["negative", "mixed"]
_CACHE = {}


def _points():
    """affine multiples of the base point, one per row of the largest case (computed once)"""
    if "points" not in _CACHE:
        _CACHE["points"] = rm.ed_multiples(max(ROWS), first=3, step=7)
    return _CACHE["points"]


def _rows(points, zs):
    return np.array([rm.ed_point51(rm.ed_extended(pt, z)) for pt, z in zip(points, zs)], np.uint64)


def _scalars(kind, n, rng):
    if kind == "negative":
        # every 16-bit window in [0x8001, 0xfffe]: every digit is stored negative (the carry turns
        # 0xfffe into 0xffff, never into 0)
        words = rng.integers(0x8001, 0xffff, (n, 16), dtype=np.uint16)
        return np.ascontiguousarray(words).view(np.uint8).reshape(n, 32).copy()
    s = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    s[:, 31] &= 0x0f
    return s


def _special():
    """130 rows under factors of their own, with the identity at row 5, a point and its negative
    at rows 10 and 11 (and again across the wavefront edge at 63 and 64) under equal scalars, and
    a generator with Z = 2 at row 70"""
    rng = np.random.default_rng(77)
    n = 130
    pts = list(_points()[:n])
    zs = [int.from_bytes(rng.bytes(32), "little") % (rm.P - 2) + 2 for _ in range(n)]
    pts[5] = (0, 1)
    pts[11] = rm.ed_neg(pts[10])
    pts[64] = rm.ed_neg(pts[63])
    zs[70] = 2
    zs[5] = 1
    s = _scalars("mixed", n, rng)
    s[11] = s[10]
    s[64] = s[63]
    return _rows(pts, zs), s


def _cases():
    """name -> (generator rows, scalars): the same arrays in the child and here"""
    if "cases" not in _CACHE:
        cases = {}
        unit = _rows(_points(), [1] * max(ROWS))
        for n in ROWS:
            for kind in KINDS:
                rng = np.random.default_rng(1000 * n + len(kind))
                cases[f"{kind}_{n}"] = (unit[:n], _scalars(kind, n, rng))
        cases["special"] = _special()
        # the pair alone: the whole sum is the identity
        rows, s = _special()
        cases["pair"] = (rows[10:12].copy(), s[10:12].copy())
        _CACHE["cases"] = cases
    return _CACHE["cases"]


def _host_expectations(path):
    """(in the child process) every case on the host backend -> npz"""
    from blitzar_amd import api
    assert api.init(api.SXT_CPU_BACKEND, 0) == 0
    out = {}
    for name, (rows, s) in _cases().items():
        gens = np.ascontiguousarray(rows).view(np.uint8).reshape(rows.shape[0], -1)
        out[name] = api.compute_pedersen_commitments(0, [(s, False)], generators=gens)
    np.savez(path, **out)


@pytest.fixture(scope="module")
def expected():
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "host.npz")
        code = f"from tests import test_accumulate_halved as m\nm._host_expectations({path!r})\n"
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        with np.load(path) as z:
            return {k: z[k] for k in z.files}


@pytest.fixture()
def backend(gpu_backend):
    """the GPU backend with empty caller tables"""
    import torch
    torch.cuda.synchronize()
    gpu_backend.load().bzamd_caller_table_reset()
    return gpu_backend


def _both_routes(api, rows, s):
    """bzamd_msm_device twice on one generator array (the second call runs on the caller table
    the first one filled), then a resident set made of the same array -> three outputs"""
    import torch
    lib = api.load()
    dev = torch.device("cuda", 0)
    d_gens = torch.from_numpy(np.ascontiguousarray(rows).view(np.uint8).reshape(-1).copy()).to(dev)
    d_col = torch.from_numpy(s.copy()).to(dev)
    desc = (api.sxt_sequence_descriptor * 1)()
    desc[0] = api.sxt_sequence_descriptor(32, s.shape[0], d_col.data_ptr(), 0)
    stream = vp(torch.cuda.current_stream().cuda_stream)
    outs = []
    for _ in range(2):
        out = torch.zeros((1, 32), dtype=torch.uint8, device=dev)
        before = lib.bzamd_kernel_launch_count()
        lib.bzamd_msm_device(0, vp(out.data_ptr()), 1, desc, vp(d_gens.data_ptr()), stream)
        assert lib.bzamd_kernel_launch_count() > before, "no kernels were launched"
        outs.append(out)
    h = lib.bzamd_generators_new_device(0, vp(d_gens.data_ptr()), rows.shape[0], stream)
    try:
        out = torch.zeros((1, 32), dtype=torch.uint8, device=dev)
        before = lib.bzamd_kernel_launch_count()
        lib.bzamd_msm_device_resident(vp(out.data_ptr()), 1, desc, vp(h), stream)
        assert lib.bzamd_kernel_launch_count() > before, "no kernels were launched"
        outs.append(out)
        torch.cuda.synchronize()
    finally:
        lib.bzamd_generators_free(vp(h))
    return [o.cpu().numpy() for o in outs]


def _check(api, expected, name):
    rows, s = _cases()[name]
    want = expected[name]
    for route, got in zip(("caller, call 1", "caller, call 2", "resident set"), _both_routes(api, rows, s)):
        assert np.array_equal(got, want), route


@pytest.mark.parametrize("n", ROWS)
def test_every_digit_negative(backend, expected, n):
    """16-bit windows, every one above 2^15: the opposite sign of the conditional negation and the
    exchanged halves on every addition; 1 .. 63 lanes of the last wavefront without an entry"""
    lib = backend.load()
    lib.bzamd_set_window_bits(16)
    try:
        _check(backend, expected, f"negative_{n}")
    finally:
        lib.bzamd_set_window_bits(0)


@pytest.mark.parametrize("n", ROWS)
def test_mixed_signs(backend, expected, n):
    """random 252-bit scalars, the planner's own window width"""
    _check(backend, expected, f"mixed_{n}")


def test_special_generators(backend, expected):
    """the identity as a generator, P and -P at neighbouring rows under equal scalars (in one
    wavefront and across the edge of two), a generator with Z = 2, every other row under a random Z"""
    _check(backend, expected, "special")


def test_sum_passes_through_the_identity(backend, expected):
    """two rows, P and -P under one scalar: every bucket that holds one holds the other, and the
    commitment is the identity's"""
    assert not expected["pair"].any(), "the host backend's commitment of P - P is the zero bytes"
    _check(backend, expected, "pair")
