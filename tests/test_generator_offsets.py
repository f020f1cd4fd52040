"""Per-column generator offsets (include/blitzar_amd.h, bzamd_*_offsets):
    commitments[i] = sum_j scalar_ij * G[offsets[i] + j]
checked column by column against the oracle on G[off_i : off_i + n_i], on the host backend and on
the device entry points (blocking host operands, device operands, resident sets, built-in
generators), through the engine's sort paths, window tables, passes and throughput mode."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from blitzar_amd import api
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = [0, 1, 2, 3]


def _expect(oracle, curve_id, cols, gens, offsets):
    """the oracle, one column at a time on its own window of the generators"""
    width = api.CURVE_LAYOUT[curve_id][1]
    out = np.zeros((len(cols), width), dtype=np.uint8)
    for i, ((col, signed), off) in enumerate(zip(cols, offsets)):
        n = col.shape[0]
        window = gens[off:off + n] if n else gens[:1]  # (an empty column reads no generator)
        out[i] = oracle.commit(curve_id, [(col, signed)], window)[0]
    return out


def _columns(rng, lengths, nbytes=32, signed=False):
    return [(rng.integers(0, 256, (n, nbytes), dtype=np.uint8), signed) for n in lengths]


def _generators(curve_id, n):
    if curve_id != 0 and n > 4096:
        return util.weierstrass_generators_big(curve_id, n)
    return util.generators_for(curve_id, n)


def _run_child(code):
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ),
                          capture_output=True, text=True, timeout=120)


#--------------------------------------------------------------------------------------------------
# host backend
#--------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", CURVES)
def test_cpu_backend_parity(cpu_backend, oracle, cid):
    rng = np.random.default_rng(100 + cid)
    num_gens = 90
    gens = util.generators_for(cid, num_gens)
    g_api = util.api_generators(cid, gens)
    cols = (_columns(rng, [20, 7, 0, 33], 32) + _columns(rng, [15], 1) +
            _columns(rng, [12], 4, signed=True) + _columns(rng, [10], 8))
    offsets = [0, 40, 88, 57, 75, 3, 80]  # disjoint, overlapping, empty, one ending at num_gens
    got = cpu_backend.compute_commitments_with_generator_offsets(cid, cols, g_api, offsets)
    assert np.array_equal(got, _expect(oracle, cid, cols, gens, offsets))


@pytest.mark.parametrize("cid", CURVES)
def test_cpu_null_offsets_match_pedersen(cpu_backend, cid):
    rng = np.random.default_rng(200 + cid)
    gens = util.api_generators(cid, util.generators_for(cid, 40))
    cols = _columns(rng, [40, 17, 0], 32) + _columns(rng, [25], 2, signed=True)
    want = cpu_backend.compute_pedersen_commitments(cid, cols, generators=gens)
    got = cpu_backend.compute_commitments_with_generator_offsets(cid, cols, gens, None)
    assert np.array_equal(got, want)
    got = cpu_backend.compute_commitments_with_generator_offsets(cid, cols, gens, [0] * len(cols))
    assert np.array_equal(got, want)


def test_cpu_builtin_generators(cpu_backend, oracle):
    rng = np.random.default_rng(7)
    cols = _columns(rng, [16, 9, 30], 32)
    offsets = [0, 500, 12]
    got = cpu_backend.compute_commitments_with_generator_offsets(0, cols, None, offsets)
    for i, ((col, s), off) in enumerate(zip(cols, offsets)):
        want = oracle.commit(0, [(col, s)], oracle.ristretto_generators(col.shape[0], off))
        assert np.array_equal(got[i], want[0])
    # NULL offsets: the bytes of sxt_curve25519_compute_pedersen_commitments
    assert np.array_equal(cpu_backend.compute_commitments_with_generator_offsets(0, cols, None, None),
                          cpu_backend.compute_pedersen_commitments(0, cols))


def test_cpu_sharded_host_backend(oracle):
    """BLITZAR_AMD_FORCE_SHARDS on the host backend: the column split and the row split (over the
    generator axis) give the oracle's bytes"""
    code = (
        "import numpy as np, sys\n"
        "from blitzar_amd import api\nfrom tests import util\nfrom oracle import ref_oracle as o\n"
        "api.init(api.SXT_CPU_BACKEND, 0)\napi.load().bzamd_set_shard_min_bytes(1)\n"
        "rng = np.random.default_rng(3)\ngens = util.generators_for(2, 3200)\n"
        "g = util.api_generators(2, gens)\n"
        "for lengths, offs in (([40, 30, 50, 10], [0, 200, 60, 290]), ([1500, 1500], [100, 1700])):\n"
        "    cols = [(rng.integers(0, 256, (n, 32), dtype=np.uint8), False) for n in lengths]\n"
        "    got = api.compute_commitments_with_generator_offsets(2, cols, g, offs)\n"
        "    for i, ((c, s), off) in enumerate(zip(cols, offs)):\n"
        "        assert np.array_equal(got[i], o.commit(2, [(c, s)], gens[off:off + len(c)])[0])\n"
        "print('ok')\n")
    env = dict(os.environ, BLITZAR_AMD_FORCE_SHARDS="3")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr


def test_out_of_range_offset_aborts():
    base = ("import numpy as np\nfrom blitzar_amd import api\nfrom tests import util\n"
            "api.init(api.SXT_CPU_BACKEND, 0)\n"
            "g = util.api_generators(2, util.generators_for(2, 10))\n"
            "cols = [(np.ones((4, 32), np.uint8), False)]\n")
    # offset + n == num_generators is fine
    r = _run_child(base + "api.compute_commitments_with_generator_offsets(2, cols, g, [6])\n"
                   "print('fine')\n")
    assert r.returncode == 0 and "fine" in r.stdout, r.stderr
    for off in (7, 10, 2**64 - 2):
        r = _run_child(base + f"api.compute_commitments_with_generator_offsets(2, cols, g, [{off}])\n")
        assert r.returncode < 0 and "exceeds the number of generators" in r.stderr, (off, r.stderr)
    # NULL offsets still check n against num_generators
    r = _run_child(base + "cols = [(np.ones((11, 32), np.uint8), False)]\n"
                   "api.compute_commitments_with_generator_offsets(2, cols, g, None)\n")
    assert r.returncode < 0 and "exceeds the number of generators" in r.stderr, r.stderr


#--------------------------------------------------------------------------------------------------
# GPU
#--------------------------------------------------------------------------------------------------
def _launches():
    return api.load().bzamd_kernel_launch_count()


def _host_call(lib_api, oracle, cid, cols, gens, offsets):
    before = _launches()
    got = lib_api.compute_commitments_with_generator_offsets(cid, cols,
                                                             util.api_generators(cid, gens), offsets)
    assert _launches() > before, "no kernel ran"
    assert np.array_equal(got, _expect(oracle, cid, cols, gens, offsets))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("cid", CURVES)
def test_gpu_window_shapes(gpu_backend, oracle, cid):
    """disjoint, overlapping and identical windows, an empty column, a window that ends exactly at
    num_generators, signed scalars, 1- and 32-byte scalars"""
    rng = np.random.default_rng(300 + cid)
    num_gens = 3000
    gens = util.generators_for(cid, num_gens)
    cases = [
        (_columns(rng, [700, 700, 700], 32), [0, 700, 1400]),                 # disjoint
        (_columns(rng, [900, 800, 1000], 32), [0, 450, 300]),                 # overlapping
        (_columns(rng, [1200, 1200, 1200], 32), [1000, 1000, 1000]),          # identical
        (_columns(rng, [500, 0, 300], 32), [100, 2999, 2700]),                # empty; ends at num_gens
        (_columns(rng, [600, 400], 8, signed=True) + _columns(rng, [350], 2, signed=True),
         [5, 2600, 1234]),                                                     # signed
        (_columns(rng, [1000], 1) + _columns(rng, [999], 32), [2000, 1]),     # 1 / 32 bytes
    ]
    for cols, offsets in cases:
        _host_call(gpu_backend, oracle, cid, cols, gens, offsets)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", CURVES)
def test_gpu_null_offsets_match_pedersen(gpu_backend, cid):
    rng = np.random.default_rng(400 + cid)
    gens = util.api_generators(cid, util.generators_for(cid, 2048))
    cols = _columns(rng, [2048, 1500, 0], 32) + _columns(rng, [700], 4, signed=True)
    want = gpu_backend.compute_pedersen_commitments(cid, cols, generators=gens)
    before = _launches()
    got = gpu_backend.compute_commitments_with_generator_offsets(cid, cols, gens, None)
    assert _launches() > before
    assert np.array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [0, 2])
def test_gpu_many_disjoint_columns(gpu_backend, oracle, cid):
    """256 independent sets back to back (batched MSM with non-shared bases): one task per window
    and column, sorted in one workgroup per task (k_task_sort); rows 256 .. 4096"""
    rng = np.random.default_rng(500 + cid)
    lengths = [256 + (i * 977) % 3841 for i in range(256)]
    offsets = np.cumsum([0] + lengths[:-1]).tolist()
    gens = _generators(cid, int(sum(lengths)))
    cols = _columns(rng, lengths, 32)
    _host_call(gpu_backend, oracle, cid, cols, gens, offsets)


@pytest.mark.gpu
def test_gpu_forced_window_bits_16(gpu_backend, oracle):
    lib = gpu_backend.load()
    rng = np.random.default_rng(600)
    gens = util.generators_for(1, 5000)
    cols = _columns(rng, [3000, 2000, 4000], 32)
    lib.bzamd_set_window_bits(16)
    try:
        _host_call(gpu_backend, oracle, 1, cols, gens, [0, 3000, 1000])
    finally:
        lib.bzamd_set_window_bits(0)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [0, 3])
def test_gpu_forced_call_tables(gpu_backend, oracle, cid):
    """a per-call window table (forced width) over shared windows and over overlapping ones: slices
    span the union of the windows, entries land on w * stride + row_base + row"""
    lib = gpu_backend.load()
    rng = np.random.default_rng(700 + cid)
    gens = util.generators_for(cid, 1100)
    shared = (_columns(rng, [1000] * 8, 32), [100] * 8)
    overlapping = (_columns(rng, [1000] * 8, 32), [0, 100, 50, 25, 75, 100, 10, 90])
    for bits in (8, 11):
        for cols, offsets in (shared, overlapping):
            built = lib.bzamd_set_call_tables(bits)
            try:
                _host_call(gpu_backend, oracle, cid, cols, gens, offsets)
                assert lib.bzamd_set_call_tables(-1) == built + 1, "no table was built"
            finally:
                lib.bzamd_set_call_tables(0)
    # disjoint windows: no table (the union is eight columns long), the same bytes
    cols = _columns(rng, [130] * 8, 32)
    offsets = [130 * i for i in range(8)]
    plain = _host_call(gpu_backend, oracle, cid, cols, gens, offsets)
    lib.bzamd_set_call_tables(11)
    try:
        assert np.array_equal(
            gpu_backend.compute_commitments_with_generator_offsets(
                cid, cols, util.api_generators(cid, gens), offsets), plain)
    finally:
        lib.bzamd_set_call_tables(0)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [0, 2])
def test_gpu_passes_at_nonzero_offset(gpu_backend, oracle, cid):
    lib = gpu_backend.load()
    rng = np.random.default_rng(800 + cid)
    gens = util.generators_for(cid, 4000)
    cols = _columns(rng, [1500, 900, 2000], 32)
    offsets = [1700, 3100, 0]
    lib.bzamd_set_max_rows_per_pass(1024)
    try:
        _host_call(gpu_backend, oracle, cid, cols, gens, offsets)
    finally:
        lib.bzamd_set_max_rows_per_pass(1 << 28)


@pytest.mark.gpu
def test_gpu_builtin_generators(gpu_backend, oracle):
    rng = np.random.default_rng(900)
    cols = _columns(rng, [60, 90, 0, 40], 32)
    offsets = [0, 30, 5, 200]  # inside and beyond the init-time cache of 100
    before = _launches()
    got = gpu_backend.compute_commitments_with_generator_offsets(0, cols, None, offsets)
    assert _launches() > before
    for i, ((col, s), off) in enumerate(zip(cols, offsets)):
        want = oracle.commit(0, [(col, s)], oracle.ristretto_generators(col.shape[0], off))
        assert np.array_equal(got[i], want[0])


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [0, 1])
def test_gpu_append_rows(gpu_backend, cid):
    """committing rows[m:n] at offset m gives the bytes of committing, at offset 0, the length-n
    column whose first m rows are zero -- for several m in one call, one column per m"""
    rng = np.random.default_rng(1000 + cid)
    n = 2000
    gens = util.api_generators(cid, util.generators_for(cid, n))
    rows = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    ms = [0, 1, 8, 999, 1024, 1999]
    appended = [(rows[m:], False) for m in ms]
    padded = []
    for m in ms:
        full = rows.copy()
        full[:m] = 0
        padded.append((full, False))
    before = _launches()
    got = gpu_backend.compute_commitments_with_generator_offsets(cid, appended, gens, ms)
    assert _launches() > before
    want = gpu_backend.compute_commitments_with_generator_offsets(cid, padded, gens, [0] * len(ms))
    assert np.array_equal(got, want)


def _device_columns(torch, dev, cols):
    d_cols = [torch.from_numpy(c.copy()).to(dev) for c, _ in cols]
    desc = (api.sxt_sequence_descriptor * len(cols))()
    for i, ((c, s), d) in enumerate(zip(cols, d_cols)):
        desc[i] = api.sxt_sequence_descriptor(c.shape[1], c.shape[0],
                                              d.data_ptr() if c.shape[0] else None, int(s))
    return d_cols, desc


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [0, 2])
def test_gpu_device_and_resident_forms(gpu_backend, oracle, cid):
    import torch
    lib = gpu_backend.load()
    dev = torch.device("cuda", 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(1100 + cid)
    num_gens = 3000
    gens = util.generators_for(cid, num_gens)
    g_host = np.ascontiguousarray(util.api_generators(cid, gens))
    d_gens = torch.from_numpy(g_host.copy()).to(dev)
    cols = _columns(rng, [1000, 800, 0], 32) + _columns(rng, [500], 4, signed=True)
    offsets = [2000, 700, 0, 2500]
    want = _expect(oracle, cid, cols, gens, offsets)
    d_cols, desc = _device_columns(torch, dev, cols)
    offs, _keep = api.offsets_array(offsets, len(cols))
    out = torch.zeros((len(cols), want.shape[1]), dtype=torch.uint8, device=dev)
    before = _launches()
    lib.bzamd_msm_device_offsets(cid, ctypes.c_void_p(out.data_ptr()), len(cols), desc,
                                 ctypes.c_void_p(d_gens.data_ptr()), num_gens, offs, stream)
    torch.cuda.synchronize()
    assert _launches() > before
    assert np.array_equal(out.cpu().numpy(), want)
    h = lib.bzamd_generators_new_host(cid, g_host.ctypes.data_as(ctypes.c_void_p), num_gens)
    try:
        out.zero_()
        before = _launches()
        lib.bzamd_msm_device_resident_offsets(ctypes.c_void_p(out.data_ptr()), len(cols), desc, h,
                                              offs, stream)
        torch.cuda.synchronize()
        assert _launches() > before
        assert np.array_equal(out.cpu().numpy(), want)
    finally:
        lib.bzamd_generators_free(h)


@pytest.mark.gpu
def test_gpu_pipelined_offsets_calls(gpu_backend, oracle):
    """a throughput-mode sequence of bzamd_msm_device_offsets calls, then bzamd_pipeline_flush"""
    import torch
    lib = gpu_backend.load()
    dev = torch.device("cuda", 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(1200)
    num_gens = 6000
    gens = util.generators_for(0, num_gens)
    d_gens = torch.from_numpy(np.ascontiguousarray(util.api_generators(0, gens)).copy()).to(dev)
    jobs = []
    for offsets in ([0, 3000], [1000, 1000], [3500, 100], [0, 3000]):
        cols = _columns(rng, [2500, 2500], 32)
        d_cols, desc = _device_columns(torch, dev, cols)
        offs, keep = api.offsets_array(offsets, 2)
        jobs.append((desc, d_cols, offs, keep, _expect(oracle, 0, cols, gens, offsets)))
    outs = []
    before = _launches()
    for _ in range(2):
        for desc, _, offs, _, want in jobs:
            out = torch.zeros((2, 32), dtype=torch.uint8, device=dev)
            lib.bzamd_pipeline_next()
            lib.bzamd_msm_device_offsets(0, ctypes.c_void_p(out.data_ptr()), 2, desc,
                                         ctypes.c_void_p(d_gens.data_ptr()), num_gens, offs, stream)
            outs.append((out, want))
    lib.bzamd_pipeline_flush(stream)
    torch.cuda.synchronize()
    assert _launches() > before
    for out, want in outs:
        assert np.array_equal(out.cpu().numpy(), want)
