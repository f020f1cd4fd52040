"""k_accumulate<ed25519_niels_msm> with the wavefront-cooperative row gather (msm/kernels.h,
accumulate_lds_gather; msm/lds_gather.h): commitments over Z = 1 addends against the reference CPU
backend, at the shapes where lanes of a wavefront have no entry or a short segment.

Two routes reach the kernel: the built-in generators (a resident set, always in the Z = 1 form) and
caller generators in device memory through bzamd_msm_device, whose second call on a pointer runs on
the caller table.  Every case asserts that kernels were launched."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

vp = ctypes.c_void_p
ROWS = [1, 2, 63, 64, 65, 2047, 2048, 4097]
_GENS = {}


def _gens(oracle, n):
    """the reference's first generators, computed once for the largest case"""
    if "all" not in _GENS:
        _GENS["all"] = oracle.ristretto_generators(max(ROWS))
    return _GENS["all"][:n]


def _builtin(api, oracle, cols):
    """commit on the built-in generators -> (got, want)"""
    lib = api.load()
    before = lib.bzamd_kernel_launch_count()
    got = api.compute_pedersen_commitments(0, cols)
    assert lib.bzamd_kernel_launch_count() > before, "no kernels were launched"
    return got, oracle.commit(0, cols, _gens(oracle, max(c.shape[0] for c, _ in cols)))


def _caller(api, oracle, cols, calls=2):
    """bzamd_msm_device `calls` times on one device generator array -> (outputs, want)"""
    import torch
    lib = api.load()
    dev = torch.device("cuda", 0)
    gens = _gens(oracle, max(c.shape[0] for c, _ in cols))
    d_gens = torch.from_numpy(np.ascontiguousarray(gens).view(np.uint8).reshape(-1).copy()).to(dev)
    d_cols = [torch.from_numpy(np.ascontiguousarray(c).view(np.uint8).reshape(c.shape[0], -1).copy()).to(dev)
              for c, _ in cols]
    desc = (api.sxt_sequence_descriptor * len(cols))()
    for i, (c, signed) in enumerate(cols):
        desc[i] = api.sxt_sequence_descriptor(d_cols[i].shape[1], c.shape[0], d_cols[i].data_ptr(),
                                              1 if signed else 0)
    stream = vp(torch.cuda.current_stream().cuda_stream)
    outs = []
    for _ in range(calls):
        out = torch.zeros((len(cols), 32), dtype=torch.uint8, device=dev)
        before = lib.bzamd_kernel_launch_count()
        lib.bzamd_msm_device(0, vp(out.data_ptr()), len(cols), desc, vp(d_gens.data_ptr()), stream)
        assert lib.bzamd_kernel_launch_count() > before, "no kernels were launched"
        outs.append(out)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs], oracle.commit(0, cols, gens)


@pytest.fixture()
def backend(gpu_backend):
    """the GPU backend with empty caller tables"""
    import torch
    torch.cuda.synchronize()
    gpu_backend.load().bzamd_caller_table_reset()
    return gpu_backend


def _check_both_routes(api, oracle, cols):
    got, want = _builtin(api, oracle, cols)
    assert np.array_equal(got, want), "built-in generators"
    outs, want = _caller(api, oracle, cols)
    for call, out in enumerate(outs):
        assert np.array_equal(out, want), f"caller generators, call {call + 1}"


@pytest.mark.parametrize("nbytes", [1, 32])
@pytest.mark.parametrize("n", ROWS)
def test_row_counts(backend, oracle, n, nbytes):
    """1 .. 63 lanes of the last wavefront without an entry, tasks whose last segment is short"""
    rng = np.random.default_rng(1000 * nbytes + n)
    _check_both_routes(backend, oracle, [(rng.integers(0, 256, (n, nbytes), dtype=np.uint8), False)])


@pytest.mark.parametrize("n", [65, 4097])
def test_all_zero_scalars(backend, oracle, n):
    """no entry at all: every wavefront leaves before the first cooperative operation"""
    _check_both_routes(backend, oracle, [(np.zeros((n, 32), np.uint8), False)])


def test_all_equal_scalars(backend, oracle):
    """one bucket per window spans whole segments: the fold of `whole` lanes and the head rules"""
    rng = np.random.default_rng(7)
    s = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    s[0, 31] &= 0x0f
    _check_both_routes(backend, oracle, [(np.tile(s, (4097, 1)), False)])


def test_every_digit_negative(backend, oracle):
    """8-bit windows over bytes in [0x80, 0xfe]: every digit of every row is stored negative (a
    carry turns 0xfe into 0xff, never into 0), 32-byte and 1-byte scalars"""
    lib = backend.load()
    rng = np.random.default_rng(8)
    cols = [(rng.integers(0x80, 0xff, (2047, 32), dtype=np.uint8), False),
            (rng.integers(0x80, 0xff, (65, 1), dtype=np.uint8), False)]
    lib.bzamd_set_window_bits(8)
    try:
        _check_both_routes(backend, oracle, cols)
    finally:
        lib.bzamd_set_window_bits(0)


def _ragged(rng):
    """columns of different lengths and widths: several tasks per launch"""
    return [(rng.integers(0, 256, (4097, 32), dtype=np.uint8), False),
            (rng.integers(0, 256, (2047, 32), dtype=np.uint8), False),
            (rng.integers(0, 256, (65, 1), dtype=np.uint8), False),
            (rng.integers(0, 256, (1, 32), dtype=np.uint8), False),
            (np.zeros((64, 32), np.uint8), False),
            (rng.integers(0, 256, (63, 16), dtype=np.uint8), True),
            (rng.integers(0, 256, (2048, 5), dtype=np.uint8), False)]


def test_columns_of_different_lengths(backend, oracle):
    _check_both_routes(backend, oracle, _ragged(np.random.default_rng(9)))


@pytest.mark.parametrize("window_bits", [2, 16])
def test_forced_windows(backend, oracle, window_bits):
    """small windows (few buckets, long runs of one bucket) and large ones (one entry per bucket)"""
    lib = backend.load()
    lib.bzamd_set_window_bits(window_bits)
    try:
        _check_both_routes(backend, oracle, _ragged(np.random.default_rng(10 + window_bits)))
    finally:
        lib.bzamd_set_window_bits(0)


@pytest.mark.parametrize("segment_log2", [3, 7])
def test_forced_segments(backend, oracle, segment_log2):
    """8 and 128 entries per lane: the ends of the planner's range"""
    lib = backend.load()
    lib.bzamd_set_segments(segment_log2, 0)
    try:
        _check_both_routes(backend, oracle, _ragged(np.random.default_rng(20 + segment_log2)))
    finally:
        lib.bzamd_set_segments(0, 0)


def test_window_table_call(backend, oracle):
    """64 columns x 256 rows with a per-call window table of forced width: the table's rows are
    Z = 1 addends too, gathered by index like a resident set"""
    lib = backend.load()
    rng = np.random.default_rng(11)
    cols = [(rng.integers(0, 256, (256, 32), dtype=np.uint8), False) for _ in range(64)]
    built = lib.bzamd_set_call_tables(10)
    try:
        outs, want = _caller(backend, oracle, cols)
        assert lib.bzamd_set_call_tables(-1) > built, "no table was built"
    finally:
        lib.bzamd_set_call_tables(0)
    for call, out in enumerate(outs):
        assert np.array_equal(out, want), f"call {call + 1}"
