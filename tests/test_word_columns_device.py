"""The device forms of the word columns of a range check (include/blitzar_amd.h:
bzamd_decompose_words_device, bzamd_map_words_device), the host forms on the GPU backend, the
cross-checks against the multiplicity count and the column inversion, and the range check's chain
on one stream: decompose, invert the 256-row table, map.

Expected values are Python integers (tests/word_column_cases.py).  The sizes follow the kernels'
constants (proof/word_columns.hip): wavefronts of 64 lanes, workgroups of 256; decompose walks
tiles of 1024 rows on at most 1024 workgroups, map tiles of 4096 rows of one plane on at most 2048;
planes whose address is a multiple of 16 are stored (loaded) 16 bytes a lane, the others byte by
byte at the ends of every tile.  Every call is checked for its launch count, the canaries behind
each plane, in the stride gaps, around `counts`, `overflow` and the mapped columns, its untouched
inputs, and against the model."""
import numpy as np
import pytest

from blitzar_amd import api
from tests import column_inverse_cases as cic
from tests import multiplicity_cases as mc
from tests import word_column_cases as wc
from tests.test_mle_opening import element_value
from tests.test_sumcheck_device import MODULUS, to_bytes
from tests.test_word_columns import decompose as host_decompose
from tests.test_word_columns import map_words as host_map_words

W = 64             # lanes of a wavefront
B = 256            # kWordThreads
TILE = 1024        # kWordTile
GRID_CAP = 1024    # kDecomposeBlocks
MAP_TILE = 4096    # kMapTile
MAP_GRID_CAP = 2048  # kMapBlocks
DECOMPOSE, MAP = 2, 1  # launches of one call, whatever n, the words and the data are
CANARY = wc.CANARY
ROWS = [1, W - 1, W, W + 1, TILE - 1, TILE, TILE + 1]


def _launches():
    return api.load().bzamd_kernel_launch_count()


def _device():
    import torch
    return torch.device("cuda", 0)


def _up(array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array).copy()).to(_device())


def decompose_on_device(lib_api, field_id, column, num_words, shift=None, gap=0,
                        outputs=("words", "counts", "overflow"), own_column=False, want=None,
                        **skews):
    """the device form on a stream of its own over wc.Layout's buffer in device memory
    (own_column: the column in an allocation of its own, one byte past its start and up to its last
    byte); checks the launch count, every byte of the buffer and the inputs -> the model's triple"""
    import torch
    layout = wc.Layout(column, num_words, shift, gap, **skews)
    d_flat = _up(layout.flat)
    words, counts, overflow, col, shift_ptr = layout.pointers(d_flat.data_ptr(), outputs)
    if own_column:
        alone = torch.full((column[0].size + 1,), CANARY, dtype=torch.uint8, device=_device())
        alone[1:] = _up(column[0].reshape(-1))
        col = (alone.data_ptr() + 1,) + col[1:]
    side = torch.cuda.Stream(device=_device())
    torch.cuda.synchronize()
    before = _launches()
    lib_api.decompose_words_device(field_id, words, counts, overflow, col, num_words,
                                   layout.plane_stride, shift_ptr=shift_ptr, stream=side.cuda_stream)
    assert _launches() - before == DECOMPOSE
    side.synchronize()
    if want is None:
        want = wc.decompose(wc.keys_of(field_id, column, shift), num_words)
    layout.check(d_flat.cpu().numpy(), want, outputs)
    if own_column:
        got = alone.cpu().numpy()
        assert got[0] == CANARY and np.array_equal(got[1:], column[0].reshape(-1))
    return want


def i64_shift(field_id):
    return cic.element_raw(field_id, 1 << 63)


#--------------------------------------------------------------------------------------------------
# decompose: rows around the wavefront and the tile, planes at odd and at even addresses
#--------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("n", ROWS)
def test_rows(gpu_backend, field_id, n):
    """i64 with the shift 2^63, eight words.  Planes three bytes past a multiple of 16 and n + 5
    apart (every plane has a skew of its own: byte stores at both ends of a tile, 16-byte stores
    between), then at multiples of 16 (16-byte stores alone, bytes for the last n mod 16 rows)"""
    rng = np.random.default_rng(n + field_id)
    column = wc.column_of(field_id, wc.drawn(rng, n, 8, True)[:n], 8, True)
    shift = i64_shift(field_id)
    words, counts, overflow = decompose_on_device(gpu_backend, field_id, column, 8, shift=shift,
                                                  gap=5, plane_skew=3)
    assert overflow == 0
    decompose_on_device(gpu_backend, field_id, column, 8, shift=shift, gap=(-n) % 16,
                        plane_skew=0, column_skew=0)
    # without the shift the negative rows are p - |x| and overflow
    words, counts, overflow = decompose_on_device(gpu_backend, field_id, column, 8, gap=1,
                                                  plane_skew=15)
    assert overflow == sum(1 for v in cic.integer_values(field_id, *column) if v >> 64)


@pytest.mark.gpu
def test_one_row_more_than_the_grid_covers(gpu_backend):
    """a u8 column of 1024 x 1024 + 1 rows, two words: workgroup 0 walks a second tile of one row;
    the second plane is zero by construction.  The same two launches as at n = 1"""
    n = GRID_CAP * TILE + 1
    rng = np.random.default_rng(7)
    data = rng.integers(0, 256, (n, 1), dtype=np.uint8)
    data[-1, 0] = 201
    words = np.zeros((2, n), np.uint8)
    words[0] = data[:, 0]
    counts = np.bincount(data[:, 0], minlength=256).astype(np.int64)
    counts[0] += n
    decompose_on_device(gpu_backend, 0, (data, False), 2, gap=3, plane_skew=1,
                        want=(words, counts.tolist(), 0))


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_column_one_byte_past_an_allocation(gpu_backend, field_id):
    """the column in an allocation of its own that ends with the column's last byte"""
    rng = np.random.default_rng(11)
    for width, signed, n, num_words in [(8, True, W + 1, 8), (32, False, W - 1, 31),
                                        (1, False, TILE - 1, 1), (3, False, 2 * B + 7, 4)]:
        column = wc.column_of(field_id, wc.drawn(rng, n, width, signed), width, signed)
        decompose_on_device(gpu_backend, field_id, column, num_words, own_column=True, gap=2)


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_contended_bins_are_exact(gpu_backend, field_id):
    """a constant column (every lane of every wavefront adds to one bin a plane) and a column
    whose upper words are all zero, over more than one tile and with the last chunk ragged; with
    and without the key arithmetic (a shift, a signed column; an unsigned narrow one, whose upper
    planes are zero by construction)"""
    n = 3 * TILE + 5
    rng = np.random.default_rng(5)
    constant = 0x0102030405060708090A0B0C0D0E0F
    column = wc.column_of(field_id, [constant] * n, 16)
    words, counts, overflow = decompose_on_device(gpu_backend, field_id, column, 16, plane_skew=0,
                                                  column_skew=0, gap=11)
    assert counts[0] == n and all(counts[v] == n for v in range(1, 16)) and overflow == 0
    small = [int(v) for v in rng.integers(0, 1 << 12, n)]
    for signed, shift in [(False, None), (True, None), (True, i64_shift(field_id))]:
        column = wc.column_of(field_id, small, 8, signed)
        words, counts, overflow = decompose_on_device(gpu_backend, field_id, column, 8, shift=shift,
                                                      plane_skew=0, column_skew=0)
        assert counts[0] >= (6 if shift is None else 5) * n and overflow == 0
    # counts and overflow alone, the words alone
    decompose_on_device(gpu_backend, field_id, column, 8, outputs=("counts", "overflow"))
    decompose_on_device(gpu_backend, field_id, column, 8, outputs=("words",))
    decompose_on_device(gpu_backend, field_id, column, 3, outputs=("overflow",))


INPUTS = {
    "uniform": lambda rng, p, n: [int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(),
                                                 "little") % p for _ in range(n)],
    "small": lambda rng, p, n: [int(v) for v in rng.integers(0, 1 << 20, n)],
    "constant": lambda rng, p, n: [p - 12345] * n,
}


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("kind", sorted(INPUTS))
def test_elements_at_31_words(gpu_backend, field_id, kind):
    """32-byte elements (field 1: Montgomery words), 31 words: uniform keys, small values and a
    constant column; every third row unreduced where it fits"""
    p = MODULUS[field_id]
    n = TILE + W + 1
    values = INPUTS[kind](np.random.default_rng(len(kind)), p, n)
    raw = [cic.element_raw(field_id, v) for v in values]
    raw = [r + p if i % 3 == 0 and r + p < 1 << 256 else r for i, r in enumerate(raw)]
    column = (mc.rows_of(field_id, raw, 32, raw=True), False)
    words, counts, overflow = decompose_on_device(gpu_backend, field_id, column, 31, gap=9)
    assert overflow == sum(1 for v in values if v >> 248)
    assert bytes(words[:, 1]) == values[1].to_bytes(32, "little")[:31]


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_no_rows_on_device(gpu_backend, field_id):
    column = (np.zeros((0, 8), np.uint8), True)
    words, counts, overflow = decompose_on_device(gpu_backend, field_id, column, 8, gap=4)
    assert counts == [0] * 256 and overflow == 0


#--------------------------------------------------------------------------------------------------
# map
#--------------------------------------------------------------------------------------------------
def map_on_device(lib_api, words, table, plane_gap=0, mapped_gap=0, skew=3, table_skew=1):
    """the device form on a stream of its own: planes `skew` bytes past a multiple of 16, the
    table `table_skew` past one, mapped columns mapped_gap apart between canaries"""
    import torch
    planes, n = words.shape
    plane_stride, mapped_stride = n + plane_gap, 32 * n + mapped_gap
    flat = np.full(64 + planes * plane_stride + 64, CANARY, np.uint8)
    for k in range(planes):
        flat[48 + skew + k * plane_stride:48 + skew + k * plane_stride + n] = words[k]
    d_flat = _up(flat)
    d_table = _up(np.concatenate([np.full(table_skew, CANARY, np.uint8), table.reshape(-1)]))
    out = torch.full((planes * mapped_stride + 16,), CANARY, dtype=torch.uint8, device=_device())
    side = torch.cuda.Stream(device=_device())
    torch.cuda.synchronize()
    before = _launches()
    lib_api.map_words_device(out.data_ptr() + 8, d_flat.data_ptr() + 48 + skew,
                             d_table.data_ptr() + table_skew, planes, n, plane_stride,
                             mapped_stride, stream=side.cuda_stream)
    assert _launches() - before == MAP
    side.synchronize()
    assert np.array_equal(d_flat.cpu().numpy(), flat), "the words were modified"
    assert np.array_equal(d_table.cpu().numpy()[table_skew:], table.reshape(-1))
    expected = np.full(planes * mapped_stride + 16, CANARY, np.uint8)
    want = table[words.astype(np.int64)]            # [planes, n, 32]
    for k in range(planes):
        expected[8 + k * mapped_stride:8 + k * mapped_stride + 32 * n] = want[k].reshape(-1)
    got = out.cpu().numpy()
    wrong = np.nonzero(got != expected)[0]
    assert wrong.size == 0, f"{wrong.size} bytes differ, the first at {int(wrong[0]) - 8}"
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, W - 1, W, W + 1, MAP_TILE - 1, MAP_TILE, MAP_TILE + 1])
def test_map_rows(gpu_backend, n):
    """rows around the wavefront and the tile, three planes: at odd addresses with gaps (byte loads
    at the ends of a tile), at multiples of 16 (16-byte loads, bytes for the last n mod 16 rows);
    the table at an odd and at an even address; against a row-by-row model at the small sizes"""
    rng = np.random.default_rng(n)
    words = rng.integers(0, 256, (3, n), dtype=np.uint8)
    words[0, 0], words[2, n - 1] = 255, 0
    table = wc.distinct_table()
    want = map_on_device(gpu_backend, words, table, plane_gap=5, mapped_gap=24, skew=3)
    if n <= W + 1:
        assert np.array_equal(want, wc.mapped(words, table))
    map_on_device(gpu_backend, words, table, plane_gap=(-n) % 16, skew=0, table_skew=16)


@pytest.mark.gpu
def test_map_32_planes(gpu_backend):
    rng = np.random.default_rng(32)
    words = rng.integers(0, 256, (32, 2 * B + 3), dtype=np.uint8)
    table = rng.integers(0, 256, (256, 32), dtype=np.uint8)
    map_on_device(gpu_backend, words, table, plane_gap=1, mapped_gap=8, skew=9)
    map_on_device(gpu_backend, words[:1], table, skew=15)


@pytest.mark.gpu
def test_map_more_tiles_than_the_grid(gpu_backend):
    """32 planes of 64 x 4096 + 1 rows: 2080 tiles on 2048 workgroups, the first 32 walk a second
    tile.  Compared on the device (268 MB of mapped rows)"""
    import torch
    planes, n = 32, 64 * MAP_TILE + 1
    assert planes * ((n + MAP_TILE - 1) // MAP_TILE) > MAP_GRID_CAP
    generator = torch.Generator(device=_device()).manual_seed(3)
    words = torch.randint(0, 256, (planes, n), dtype=torch.uint8, device=_device(),
                          generator=generator)
    table = _up(wc.distinct_table())
    out = torch.full((planes * n * 32 + 16,), CANARY, dtype=torch.uint8, device=_device())
    torch.cuda.synchronize()
    before = _launches()
    gpu_backend.map_words_device(out.data_ptr() + 8, words.data_ptr(), table.data_ptr(), planes, n,
                                 n, 32 * n)
    assert _launches() - before == MAP
    torch.cuda.synchronize()
    assert bool((out[:8] == CANARY).all()) and bool((out[-8:] == CANARY).all())
    got = out[8:-8].view(planes, n, 32)
    for k in range(planes):   # a plane at a time: the index tensor stays small
        assert torch.equal(got[k], table[words[k].long()]), k


#--------------------------------------------------------------------------------------------------
# against the entry points a caller has today
#--------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_against_the_range_count_and_the_column_inverse(gpu_backend, field_id):
    """n = 3000, i64 with the shift, eight words: the range-table counts of the eight planes add up
    to `counts`; bzamd_invert_columns_device on a plane equals the plane mapped through the
    inverted table, byte for byte, in element form and in scalar form"""
    import torch
    p, n, num_words, dev = MODULUS[field_id], 3000, 8, _device()
    rng = np.random.default_rng(field_id)
    values = [int(v) for v in rng.integers(-(1 << 40), 1 << 40, n)]
    column = wc.column_of(field_id, values, 8, True)
    d_column, d_shift = _up(column[0]), _up(wc.shift_bytes(i64_shift(field_id)))
    alpha = int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % p
    assert all((alpha + v) % p for v in range(256))
    d_alpha = _up(to_bytes(field_id, alpha))
    planes = torch.zeros((num_words, n), dtype=torch.uint8, device=dev)
    counts = torch.zeros(257, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    gpu_backend.decompose_words_device(field_id, planes.data_ptr(), counts.data_ptr(),
                                       counts.data_ptr() + 2048, (d_column.data_ptr(), n, 8, True),
                                       num_words, n, shift_ptr=d_shift.data_ptr(),
                                       stream=side.cuda_stream)
    # (A) the range form of the multiplicity count, once a plane
    per_plane = torch.zeros((num_words, 257), dtype=torch.int64, device=dev)
    for k in range(num_words):
        gpu_backend.count_multiplicities_device(
            field_id, per_plane[k].data_ptr(), per_plane[k].data_ptr() + 2048, (None, 256, 8, False),
            (planes[k].data_ptr(), n, 1, False), None, 0, stream=side.cuda_stream)
    # (B) the inverted table, mapped, against one inversion a row
    d_bytes = _up(np.arange(256, dtype=np.uint8))
    tables = torch.zeros((2, 256, 32), dtype=torch.uint8, device=dev)
    gpu_backend.invert_columns_device(field_id, tables[0].data_ptr(), tables[1].data_ptr(),
                                      [(d_bytes.data_ptr(), 256, 1, False)], None,
                                      d_alpha.data_ptr(), 256, stream=side.cuda_stream)
    mapped = torch.zeros((2, num_words, n, 32), dtype=torch.uint8, device=dev)
    direct = torch.zeros((2, n, 32), dtype=torch.uint8, device=dev)
    for form in range(2):
        gpu_backend.map_words_device(mapped[form].data_ptr(), planes.data_ptr(),
                                     tables[form].data_ptr(), num_words, n, n, 32 * n,
                                     stream=side.cuda_stream)
    plane = 1
    gpu_backend.invert_columns_device(field_id, direct[0].data_ptr(), direct[1].data_ptr(),
                                      [(planes[plane].data_ptr(), n, 1, False)], None,
                                      d_alpha.data_ptr(), n, stream=side.cuda_stream)
    side.synchronize()
    want = wc.decompose(wc.keys_of(field_id, column, i64_shift(field_id)), num_words)
    assert np.array_equal(planes.cpu().numpy(), want[0])
    got_counts = counts.cpu().numpy()
    assert got_counts[:256].tolist() == want[1] and got_counts[256] == 0
    summed = per_plane.cpu().numpy()
    assert not summed[:, 256].any(), "a byte missed the table 0 .. 255"
    assert np.array_equal(summed[:, :256].sum(axis=0), got_counts[:256])
    mapped, direct = mapped.cpu().numpy(), direct.cpu().numpy()
    for form in range(2):
        assert np.array_equal(mapped[form, plane], direct[form]), ("elements", "scalars")[form]
    inverse = pow(alpha + int(want[0][plane, 17]), -1, p)
    assert element_value(field_id, mapped[0, plane, 17]) == inverse
    assert int.from_bytes(mapped[1, plane, 17].tobytes(), "little") == inverse


#--------------------------------------------------------------------------------------------------
# host forms on the gpu backend
#--------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_host_forms_on_gpu(gpu_backend, field_id):
    """the same checks as on the cpu backend (tests/test_word_columns.py), with the gaps of the
    caller's strides kept; each call runs the device form's launches"""
    rng = np.random.default_rng(8)
    every = ("words", "counts", "overflow")
    for width, signed, n, num_words, shift in [(8, True, 2 * TILE + 3, 8, i64_shift(field_id)),
                                               (32, False, 300, 31, None), (2, False, 77, 5, None),
                                               (8, True, 0, 8, None)]:
        column = wc.column_of(field_id, wc.drawn(rng, max(n, 4), width, signed)[:n], width, signed)
        if n == 0:
            column = (np.zeros((0, width), np.uint8), signed)
        before = _launches()
        host_decompose(gpu_backend, field_id, column, num_words, shift=shift, gap=7)
        assert _launches() - before == DECOMPOSE, "no kernel ran"
        for missing in every:
            host_decompose(gpu_backend, field_id, column, num_words, shift=shift, gap=1,
                           outputs=tuple(o for o in every if o != missing))
    words = rng.integers(0, 256, (5, MAP_TILE + 9), dtype=np.uint8)
    before = _launches()
    host_map_words(gpu_backend, words, wc.distinct_table(), plane_gap=3, mapped_gap=16)
    assert _launches() - before == MAP, "no kernel ran"
    host_map_words(gpu_backend, words[:1, :5], wc.distinct_table())
    got = gpu_backend.map_words(words[:, :100], wc.distinct_table())
    assert np.array_equal(got, wc.distinct_table()[words[:, :100].astype(np.int64)])


#--------------------------------------------------------------------------------------------------
# the range check's chain on one stream
#--------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_range_check_on_one_stream(gpu_backend, field_id):
    """decompose an i64 column (shift 2^63, eight words), invert the table 1 / (alpha + v) of 256
    rows, map every plane through it, with nothing synchronising before the end:
    sum_k sum_i mapped_k[i] = sum_v counts[v] inv[v] mod p, in Python integers"""
    import torch
    p, n, num_words, dev = MODULUS[field_id], 300, 8, _device()
    rng = np.random.default_rng(40 + field_id)
    values = rng.integers(-(1 << 63), (1 << 63) - 1, n, dtype=np.int64)
    values[:3] = [-(1 << 63), (1 << 63) - 1, 0]
    alpha = int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % p
    assert all((alpha + v) % p for v in range(256))
    d_column = _up(values.view(np.uint8))
    d_shift, d_alpha = _up(to_bytes(field_id, 1 << 63)), _up(to_bytes(field_id, alpha))
    d_bytes = _up(np.arange(256, dtype=np.uint8))
    planes = torch.zeros((num_words, n), dtype=torch.uint8, device=dev)
    counts = torch.zeros(257, dtype=torch.int64, device=dev)
    table = torch.zeros((256, 32), dtype=torch.uint8, device=dev)
    mapped = torch.zeros((num_words, n, 32), dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    before = _launches()
    gpu_backend.decompose_words_device(field_id, planes.data_ptr(), counts.data_ptr(),
                                       counts.data_ptr() + 2048, (d_column.data_ptr(), n, 8, True),
                                       num_words, n, shift_ptr=d_shift.data_ptr(),
                                       stream=side.cuda_stream)
    gpu_backend.invert_columns_device(field_id, table.data_ptr(), None,
                                      [(d_bytes.data_ptr(), 256, 1, False)], None,
                                      d_alpha.data_ptr(), 256, stream=side.cuda_stream)
    gpu_backend.map_words_device(mapped.data_ptr(), planes.data_ptr(), table.data_ptr(), num_words,
                                 n, n, 32 * n, stream=side.cuda_stream)
    assert _launches() - before == DECOMPOSE + 1 + MAP
    side.synchronize()
    got_counts = [int(c) for c in counts.cpu().numpy()]
    assert got_counts[256] == 0 and sum(got_counts[:256]) == num_words * n
    inverses = [element_value(field_id, row) for row in table.cpu().numpy()]
    assert inverses == [pow(alpha + v, -1, p) for v in range(256)]
    left = sum(element_value(field_id, row) for row in mapped.cpu().numpy().reshape(-1, 32)) % p
    right = sum(c * inv for c, inv in zip(got_counts[:256], inverses)) % p
    assert left == right
    # and the words are those of the shifted values
    got = planes.cpu().numpy()
    for i in (0, 1, 2, n - 1):
        assert bytes(got[:, i]) == (int(values[i]) + (1 << 63)).to_bytes(8, "little")
