"""Caller tables (engine.h, msm_context; k_prepare_addends_staged<C, true>): bzamd_msm_device over
caller generators keeps the converted generators of a pointer and converts, on a later call at the
same pointer, only the tiles of 64 generators whose bytes changed.  Every expected commitment comes
from the reference CPU backend, never from a second run of the engine; the conversions are counted
by bzamd_prepare_tiles_converted().

A generator row is replaced by ANOTHER VALID GENERATOR where the commitment is compared: a single
overwritten byte always turns a coordinate into another field element and the row into something
that is not a point of the curve, for which the reference's order of additions and the engine's
bucket order need not agree.  The single-byte overwrites the kernel must notice are made as well,
each followed by a call whose conversion is counted and whose (meaningless) result is not read;
every single bit of a tile is covered on the host by tests/test_caller_table_digest.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = ctypes.c_void_p


def _scalars(rng, n):
    s = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    s[:, 31] &= 0x0f  # 252 bits
    return s


def _rows(curve_id, gens):
    return np.ascontiguousarray(util.api_generators(curve_id, gens))


def _spare_generators(oracle, curve_id, count):
    """valid generators that are in none of the sets below"""
    if curve_id == 0:
        return oracle.ristretto_generators(count, first=5000)
    return np.stack([oracle.random_affine(curve_id, 900 + i, 77) for i in range(count)])


class _Device:
    """device buffers of one column and its generators; one bzamd_msm_device call per `commit`"""

    def __init__(self, api, curve_id, scalars, gens_rows, torch, gens_buffer=None, byte_offset=0):
        self.api, self.lib, self.curve_id, self.torch = api, api.load(), curve_id, torch
        dev = torch.device("cuda", 0)
        self.n = scalars.shape[0]
        self.col = torch.from_numpy(scalars.copy()).to(dev)
        flat = torch.from_numpy(gens_rows.reshape(-1).copy()).to(dev)
        if gens_buffer is None:
            gens_buffer = torch.zeros(flat.numel() + 64, dtype=torch.uint8, device=dev)
        self.buffer = gens_buffer
        self.gens = gens_buffer[byte_offset:byte_offset + flat.numel()]
        self.gens.copy_(flat)
        self.stride = gens_rows.shape[1]
        self.out_bytes = api.CURVE_LAYOUT[curve_id][1]

    def write_row(self, row, row_bytes):
        """a device copy on the caller's stream, behind the calls enqueued so far"""
        src = self.torch.from_numpy(np.ascontiguousarray(row_bytes).view(np.uint8).copy()).to(
            self.gens.device)
        self.gens[row * self.stride:row * self.stride + src.numel()].copy_(src)

    def flip_byte(self, row, byte=0):
        at = row * self.stride + byte
        self.gens[at:at + 1].copy_(self.gens[at:at + 1] ^ 1)

    def commit(self, n=None, pipelined=False):
        n = self.n if n is None else n
        out = self.torch.zeros((1, self.out_bytes), dtype=self.torch.uint8, device=self.col.device)
        desc = (self.api.sxt_sequence_descriptor * 1)()
        desc[0] = self.api.sxt_sequence_descriptor(32, n, self.col.data_ptr(), 0)
        stream = vp(self.torch.cuda.current_stream().cuda_stream)
        if pipelined:
            self.lib.bzamd_pipeline_next()
        self.lib.bzamd_msm_device(self.curve_id, vp(out.data_ptr()), 1, desc,
                                  vp(self.gens.data_ptr()), stream)
        return out


@pytest.fixture()
def table(gpu_backend):
    """(api, lib, torch, converted()) with empty caller tables; converted() counts from here"""
    import torch
    lib = gpu_backend.load()
    torch.cuda.synchronize()
    lib.bzamd_caller_table_reset()
    base = lib.bzamd_prepare_tiles_converted()
    return gpu_backend, lib, torch, lambda: lib.bzamd_prepare_tiles_converted() - base


def _host(out):
    return out.cpu().numpy()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_same_call_three_times_converts_once(table, oracle, n):
    api, lib, torch, converted = table
    rng = np.random.default_rng(100 + n)
    gens = oracle.ristretto_generators(n)
    s = _scalars(rng, n)
    want = oracle.commit(0, [(s, False)], gens)
    d = _Device(api, 0, s, _rows(0, gens), torch)
    for call in range(3):
        assert np.array_equal(_host(d.commit()), want), f"call {call}"
        assert converted() == -(-n // 64), f"after call {call}"


def test_changed_rows_convert_their_tile(table, oracle):
    """n = 200: tiles of 64, 64, 64 and 8 rows; rows 0, 63, 64, 191, 199 in turn"""
    api, lib, torch, converted = table
    n = 200
    rng = np.random.default_rng(7)
    gens = oracle.ristretto_generators(n)
    spare = _spare_generators(oracle, 0, 5)
    s = _scalars(rng, n)
    d = _Device(api, 0, s, _rows(0, gens), torch)
    assert np.array_equal(_host(d.commit()), oracle.commit(0, [(s, False)], gens))
    count = converted()
    assert count == 4
    for k, row in enumerate((0, 63, 64, 191, 199)):
        d.flip_byte(row, byte=(41 * k) % 160)  # one byte; the row is no point now: result not read
        d.commit()
        count += 1
        assert converted() == count, f"one byte of row {row}"
        gens[row] = spare[k]
        d.write_row(row, spare[k])
        got = _host(d.commit())
        count += 1
        assert converted() == count, f"row {row} replaced"
        assert np.array_equal(got, oracle.commit(0, [(s, False)], gens)), f"row {row} replaced"
        assert np.array_equal(_host(d.commit()), got) and converted() == count


def test_change_between_pipelined_calls(table, oracle):
    """throughput mode: six calls, rows of the first and the last tile replaced behind call 3"""
    api, lib, torch, converted = table
    n = 200
    rng = np.random.default_rng(8)
    gens = oracle.ristretto_generators(n)
    spare = _spare_generators(oracle, 0, 2)
    s = _scalars(rng, n)
    old = oracle.commit(0, [(s, False)], gens)
    d = _Device(api, 0, s, _rows(0, gens), torch)
    torch.cuda.current_stream().synchronize()
    outs = [d.commit(pipelined=True) for _ in range(3)]
    for k, row in enumerate((5, 199)):
        gens[row] = spare[k]
        d.write_row(row, spare[k])
    outs += [d.commit(pipelined=True) for _ in range(3)]
    lib.bzamd_pipeline_flush(vp(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    new = oracle.commit(0, [(s, False)], gens)
    assert not np.array_equal(old, new)
    for call, out in enumerate(outs):
        assert np.array_equal(_host(out), old if call < 3 else new), f"pipelined call {call + 1}"
    assert converted() == 4 + 2


def test_shorter_and_longer_calls_share_the_prefix(table, oracle):
    api, lib, torch, converted = table
    rng = np.random.default_rng(9)
    gens = oracle.ristretto_generators(200)
    s = _scalars(rng, 200)
    d = _Device(api, 0, s, _rows(0, gens), torch)
    for call, n in enumerate((200, 70, 200)):
        want = oracle.commit(0, [(s[:n], False)], gens[:n])
        assert np.array_equal(_host(d.commit(n)), want), f"n = {n}"
        assert converted() == 4, f"call {call}, n = {n}"
    # a longer call converts what no call has covered yet, a change inside a shorter call its tile
    spare = _spare_generators(oracle, 0, 1)
    gens[66] = spare[0]
    d.write_row(66, spare[0])
    assert np.array_equal(_host(d.commit(70)), oracle.commit(0, [(s[:70], False)], gens[:70]))
    assert converted() == 5
    assert np.array_equal(_host(d.commit(200)), oracle.commit(0, [(s, False)], gens))
    assert converted() == 5


def test_first_call_is_the_shorter_one(table, oracle):
    api, lib, torch, converted = table
    rng = np.random.default_rng(10)
    gens = oracle.ristretto_generators(200)
    s = _scalars(rng, 200)
    d = _Device(api, 0, s, _rows(0, gens), torch)
    for n, tiles in ((70, 2), (200, 2 + 4), (100, 6), (200, 6)):  # (growth starts the table over)
        want = oracle.commit(0, [(s[:n], False)], gens[:n])
        assert np.array_equal(_host(d.commit(n)), want), f"n = {n}"
        assert converted() == tiles, f"n = {n}"


def test_two_curves_at_one_pointer(table, oracle):
    api, lib, torch, converted = table
    rng = np.random.default_rng(11)
    n = 200
    s = _scalars(rng, n)
    g0 = oracle.ristretto_generators(n)
    g2 = util.generators_for(2, n)
    d0 = _Device(api, 0, s, _rows(0, g0), torch)
    assert np.array_equal(_host(d0.commit()), oracle.commit(0, [(s, False)], g0))
    d2 = _Device(api, 2, s, _rows(2, g2), torch, gens_buffer=d0.buffer)
    assert d2.gens.data_ptr() == d0.gens.data_ptr()
    for _ in range(2):
        assert np.array_equal(_host(d2.commit()), oracle.commit(2, [(s, False)], g2))
    d0.gens.copy_(torch.from_numpy(_rows(0, g0).reshape(-1).copy()).to(d0.gens.device))
    assert np.array_equal(_host(d0.commit()), oracle.commit(0, [(s, False)], g0))


def test_unaligned_pointer_keeps_the_plain_conversion(table, oracle):
    api, lib, torch, converted = table
    rng = np.random.default_rng(12)
    n = 200
    s = _scalars(rng, n)
    gens = oracle.ristretto_generators(n)
    d = _Device(api, 0, s, _rows(0, gens), torch, byte_offset=8)
    assert d.gens.data_ptr() % 16 == 8
    want = oracle.commit(0, [(s, False)], gens)
    for _ in range(2):
        assert np.array_equal(_host(d.commit()), want)
    assert converted() == 0


def test_pointers_in_rotation(table, oracle):
    """two slots: two pointers alternating stay converted, three in rotation are always correct"""
    api, lib, torch, converted = table
    rng = np.random.default_rng(13)
    n = 200
    jobs = []
    for k in range(3):
        gens = oracle.ristretto_generators(n, first=1000 * k)
        s = _scalars(rng, n)
        jobs.append((_Device(api, 0, s, _rows(0, gens), torch), oracle.commit(0, [(s, False)], gens)))
    for k in (0, 1, 0, 1):
        assert np.array_equal(_host(jobs[k][0].commit()), jobs[k][1])
    assert converted() == 2 * 4
    for k in (2, 0, 1, 2, 0, 1):
        assert np.array_equal(_host(jobs[k][0].commit()), jobs[k][1]), f"pointer {k}"


@pytest.mark.parametrize("curve_id", [1, 2])
def test_weierstrass_tiles(table, oracle, curve_id):
    """bls12-381 (104-byte rows) and bn254 (72): n = 65 is a whole tile and one of a single row"""
    api, lib, torch, converted = table
    rng = np.random.default_rng(14 + curve_id)
    n = 65
    s = _scalars(rng, n)
    gens = np.ascontiguousarray(util.generators_for(curve_id, n))
    d = _Device(api, curve_id, s, _rows(curve_id, gens), torch)
    for _ in range(2):
        assert np.array_equal(_host(d.commit()), oracle.commit(curve_id, [(s, False)], gens))
    assert converted() == 2
    spare = _spare_generators(oracle, curve_id, 1)
    gens[64] = spare[0].view(gens.dtype).reshape(gens[64].shape)
    d.write_row(64, spare[0])
    for _ in range(2):
        assert np.array_equal(_host(d.commit()), oracle.commit(curve_id, [(s, False)], gens))
    assert converted() == 3


_SWITCHED_OFF_SCRIPT = r"""
import ctypes, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from blitzar_amd import api
data = np.load(sys.argv[2])
assert api.init(api.SXT_GPU_BACKEND, 0) == 0
lib = api.load()
dev = torch.device("cuda", 0)
col = torch.from_numpy(data["s"]).to(dev)
gens = torch.from_numpy(data["g"]).to(dev)
desc = (api.sxt_sequence_descriptor * 1)()
desc[0] = api.sxt_sequence_descriptor(32, col.shape[0], col.data_ptr(), 0)
outs = []
for _ in range(3):
    out = torch.zeros((1, 32), dtype=torch.uint8, device=dev)
    lib.bzamd_msm_device(0, ctypes.c_void_p(out.data_ptr()), 1, desc, ctypes.c_void_p(gens.data_ptr()),
                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    outs.append(out)
torch.cuda.synchronize()
np.savez(sys.argv[3], out=np.stack([o.cpu().numpy() for o in outs]),
         converted=np.uint64(lib.bzamd_prepare_tiles_converted()))
"""


def test_switched_off_by_the_environment(gpu_backend, oracle, tmp_path):
    """BLITZAR_AMD_CALLER_TABLE=0 (read once, so a process of its own): correct, nothing counted"""
    rng = np.random.default_rng(15)
    n = 200
    s = _scalars(rng, n)
    gens = oracle.ristretto_generators(n)
    src, dst = tmp_path / "in.npz", tmp_path / "out.npz"
    np.savez(src, s=s, g=_rows(0, gens))
    env = dict(os.environ, BLITZAR_AMD_CALLER_TABLE="0")
    r = subprocess.run([sys.executable, "-c", _SWITCHED_OFF_SCRIPT, ROOT, str(src), str(dst)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(dst)
    want = oracle.commit(0, [(s, False)], gens)
    for call in range(3):
        assert np.array_equal(got["out"][call], want)
    assert int(got["converted"]) == 0
