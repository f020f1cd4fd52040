"""curve25519 caller tables in the Z = 1 form (k_prepare_addends_staged<ed25519_niels_msm, true>;
curve_tu.h, msm): a tile of a keyed caller array that converts is normalised -- one inversion shared
by the converting tiles of a workgroup -- and the call runs the 7-product loop of resident sets.

Every expected commitment comes from the reference CPU backend on the Z = 1 forms of the same group
elements; the rows the engine gets are those elements under a random Z of their own
(refmath.ed_extended / ed_point51).  Conversions are counted by bzamd_prepare_tiles_converted()."""
import ctypes

import numpy as np
import pytest

from tests import refmath as rm

pytestmark = pytest.mark.gpu

vp = ctypes.c_void_p
_POINTS = {}


def _points(oracle, count, first=0):
    """affine (x, y) of the reference's generators first .. first + count - 1 (computed once)"""
    missing = [i for i in range(first, first + count) if i not in _POINTS]
    if missing:
        lo, hi = min(missing), max(missing) + 1
        for i, row in enumerate(oracle.ristretto_generators(hi - lo, first=lo)):
            _POINTS[lo + i] = rm.ed_affine(rm.ed_from51([int(v) for v in row]))
    return [_POINTS[i] for i in range(first, first + count)]


def _lambdas(rng, count):
    """factors in [2, p - 1]: never 0, never 1"""
    return [int.from_bytes(rng.bytes(32), "little") % (rm.P - 2) + 2 for _ in range(count)]


def _rows(points, zs):
    return np.array([rm.ed_point51(rm.ed_extended(pt, z)) for pt, z in zip(points, zs)], np.uint64)


def _unit_rows(points):
    return _rows(points, [1] * len(points))


def _scalars(rng, n):
    s = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    s[:, 31] &= 0x0f  # 252 bits
    s[:, 0] |= 1      # no zero scalar unless a test puts one there
    return s


class _Device:
    """columns of scalars and one generator array on the device; bzamd_msm_device per `commit`"""

    def __init__(self, api, torch, columns, rows):
        self.api, self.lib, self.torch = api, api.load(), torch
        self.dev = torch.device("cuda", 0)
        self.cols = [torch.from_numpy(c.copy()).to(self.dev) for c in columns]
        self.gens = torch.from_numpy(rows.view(np.uint8).reshape(-1).copy()).to(self.dev)
        assert self.gens.data_ptr() % 16 == 0

    def write_rows(self, first, rows):
        src = self.torch.from_numpy(np.ascontiguousarray(rows).view(np.uint8).reshape(-1).copy())
        self.gens[first * 160:first * 160 + src.numel()].copy_(src.to(self.dev))

    def write_scalar(self, row, scalar, column=0):
        self.cols[column][row].copy_(self.torch.from_numpy(scalar.copy()).to(self.dev))

    def commit(self, pipelined=False):
        k = len(self.cols)
        out = self.torch.zeros((k, 32), dtype=self.torch.uint8, device=self.dev)
        desc = (self.api.sxt_sequence_descriptor * k)()
        for i, c in enumerate(self.cols):
            desc[i] = self.api.sxt_sequence_descriptor(32, c.shape[0], c.data_ptr(), 0)
        stream = vp(self.torch.cuda.current_stream().cuda_stream)
        if pipelined:
            self.lib.bzamd_pipeline_next()
        self.lib.bzamd_msm_device(0, vp(out.data_ptr()), k, desc, vp(self.gens.data_ptr()), stream)
        return out

    def flush(self):
        self.lib.bzamd_pipeline_flush(vp(self.torch.cuda.current_stream().cuda_stream))
        self.torch.cuda.synchronize()


@pytest.fixture()
def table(gpu_backend):
    """(api, torch, converted()) with empty caller tables; converted() counts from here"""
    import torch
    lib = gpu_backend.load()
    torch.cuda.synchronize()
    lib.bzamd_caller_table_reset()
    base = lib.bzamd_prepare_tiles_converted()
    return gpu_backend, torch, lambda: lib.bzamd_prepare_tiles_converted() - base


def _host(out):
    return out.cpu().numpy()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_random_z(table, oracle, n):
    """the tile edge, the workgroup edge, several inversion groups with a partial last tile: a lone
    call, then three in throughput mode; only the first converts"""
    api, torch, converted = table
    rng = np.random.default_rng(500 + n)
    pts = _points(oracle, n)
    s = _scalars(rng, n)
    want = oracle.commit(0, [(s, False)], _unit_rows(pts))
    d = _Device(api, torch, [s], _rows(pts, _lambdas(rng, n)))
    assert np.array_equal(_host(d.commit()), want)
    tiles = -(-n // 64)
    assert converted() == tiles
    outs = [d.commit(pipelined=True) for _ in range(3)]
    d.flush()
    for call, out in enumerate(outs):
        assert np.array_equal(_host(out), want), f"pipelined call {call + 1}"
    assert converted() == tiles


def test_same_points_other_z_same_pointer(table, oracle):
    """the same group elements under new factors: every tile converts again, the bytes stay"""
    api, torch, converted = table
    n = 257
    rng = np.random.default_rng(41)
    pts = _points(oracle, n)
    s = _scalars(rng, n)
    want = oracle.commit(0, [(s, False)], _unit_rows(pts))
    d = _Device(api, torch, [s], _rows(pts, _lambdas(rng, n)))
    first = _host(d.commit())
    assert np.array_equal(first, want) and converted() == 5
    d.write_rows(0, _rows(pts, _lambdas(rng, n)))
    assert np.array_equal(_host(d.commit()), first)
    assert converted() == 10


_ZERO_ROWS = [(0,), (63,), (64,), (130,), (199,), (0, 63, 64, 130, 199)]


@pytest.mark.parametrize("kind", ["zero_bytes", "z_is_p"])
@pytest.mark.parametrize("bad", _ZERO_ROWS, ids=lambda r: "rows_" + "_".join(map(str, r)))
def test_zero_z_does_not_spread(table, oracle, bad, kind):
    """rows whose Z is zero mod p under zero scalars (a caller's padding): the other rows of the
    shared inversion keep their addends.  Expected: the reference's commitment with the rows and
    their scalars deleted -- nothing is asked of the reference about such a row"""
    api, torch, converted = table
    n = 200
    rng = np.random.default_rng(900 + len(bad) + 17 * bad[0])
    pts = _points(oracle, n)
    spare = _points(oracle, len(bad), first=6000)
    s = _scalars(rng, n)
    rows = _rows(pts, _lambdas(rng, n))
    unit = _unit_rows(pts)
    for r in bad:
        s[r] = 0
        if kind == "zero_bytes":
            rows[r] = 0
        else:
            junk = [int.from_bytes(rng.bytes(31), "little") for _ in range(3)]
            rows[r] = np.array(rm.fe51(junk[0]) + rm.fe51(junk[1]) + rm.fe51(rm.P) + rm.fe51(junk[2]),
                               np.uint64)
    keep = [r for r in range(n) if r not in bad]
    want = oracle.commit(0, [(s[keep], False)], unit[keep])
    d = _Device(api, torch, [s], rows)
    assert np.array_equal(_host(d.commit()), want)
    assert converted() == 4
    # a valid generator and a non-zero scalar in their place: only their tiles convert
    fresh = _scalars(rng, len(bad))
    lam = _lambdas(rng, len(bad))
    for k, r in enumerate(bad):
        s[r] = fresh[k]
        unit[r] = _unit_rows([spare[k]])[0]
        d.write_rows(r, _rows([spare[k]], [lam[k]]))
        d.write_scalar(r, fresh[k])
    got = _host(d.commit())
    assert converted() == 4 + len({r // 64 for r in bad})
    assert np.array_equal(got, oracle.commit(0, [(s, False)], unit))


def test_one_changed_row_among_unchanged_tiles(table, oracle):
    """n = 256 is one workgroup: row 70 replaced, tile 1 converts beside three waves that only take
    part in the inversion.  Their addends are read by the commitment of the whole column and by one
    that leaves tile 1 out"""
    api, torch, converted = table
    n = 256
    rng = np.random.default_rng(43)
    pts = _points(oracle, n)
    s = _scalars(rng, n)
    others = s.copy()
    others[64:128] = 0
    d = _Device(api, torch, [s, others], _rows(pts, _lambdas(rng, n)))
    unit = _unit_rows(pts)
    assert np.array_equal(_host(d.commit()), oracle.commit(0, [(s, False), (others, False)], unit))
    assert converted() == 4
    new = _points(oracle, 1, first=6100)
    d.write_rows(70, _rows(new, _lambdas(rng, 1)))
    unit[70] = _unit_rows(new)[0]
    got = _host(d.commit())
    assert converted() == 5
    assert np.array_equal(got, oracle.commit(0, [(s, False), (others, False)], unit))


@pytest.mark.parametrize("columns", [8, 9])
def test_many_columns_on_the_keyed_pointer(table, oracle, columns):
    """around the least column count of a per-call window table (plan.h, choose_call_table), unforced:
    whichever route the planner takes, the results are the reference's"""
    api, torch, converted = table
    n = 300
    rng = np.random.default_rng(60 + columns)
    pts = _points(oracle, n)
    cols = [_scalars(rng, n) for _ in range(columns)]
    want = oracle.commit(0, [(c, False) for c in cols], _unit_rows(pts))
    d = _Device(api, torch, cols, _rows(pts, _lambdas(rng, n)))
    for call in range(2):
        assert np.array_equal(_host(d.commit()), want), f"call {call}"
