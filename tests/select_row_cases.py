"""The model of bzamd_select_rows and bzamd_take_rows (include/blitzar_amd.h): numpy flatnonzero on
the selector's bits, and byte slicing.  Columns and selectors are uint8 [rows, width] arrays.  What
a call does not write holds CANARY in the model's outputs, so a test compares whole buffers.
Shared by tests/test_select_rows.py (host form) and tests/test_select_rows_device.py (device
form)."""
import numpy as np

CANARY = 0x5A
NO_ROW = 0xFFFFFFFF
MAX_COLUMNS = 16
MAX_ROWS = 2**30
# the kernels' constants (blitzar_amd/csrc/proof/select_rows.h)
W = 64                # lanes of a wavefront
WAVE_ROWS = 4 * W     # rows of a tile one wavefront takes, 64 a round
TILE = 4 * WAVE_ROWS  # rows of a tile: a workgroup of four wavefronts
MAX_SPANS = 2048


def bits(selector):
    """uint8 [n, width <= 8] -> uint64 [n]: the rows as little-endian integers, zero-extended"""
    n, width = selector.shape
    padded = np.zeros((n, 8), np.uint8)
    padded[:, :width] = selector
    return padded.view("<u8").reshape(n)


def kept_rows(selector, reject=0, invert=False):
    """the rows i with (bits(selector[i]) != reject) != invert, ascending"""
    return np.flatnonzero((bits(selector) != np.uint64(reject)) != bool(invert))


def select(selector, columns, reject=0, invert=False, capacity=None, zero_tail=False):
    """-> (count, indices uint32 [capacity], [uint8 [capacity, width] per column]); rows that the
    call does not write are CANARY bytes"""
    rows = kept_rows(selector, reject, invert)
    capacity = len(selector) if capacity is None else capacity
    written = min(len(rows), capacity)
    rows = rows[:written]
    indices = np.full(4 * capacity, CANARY, np.uint8).view(np.uint32)
    indices[:written] = rows
    if zero_tail:
        indices[written:] = NO_ROW
    selected = []
    for data in columns:
        out = np.full((capacity, data.shape[1]), CANARY, np.uint8)
        out[:written] = take(rows, [data])[0]
        if zero_tail:
            out[written:] = 0
        selected.append(out)
    return len(kept_rows(selector, reject, invert)), indices, selected


def take(indices, columns):
    """-> [uint8 [len(indices), width] per column]: row r is row indices[r], zeros past the end"""
    indices = np.asarray(indices, dtype=np.int64)
    taken = []
    for data in columns:
        out = np.zeros((len(indices), data.shape[1]), np.uint8)
        present = indices < len(data)
        out[present] = data[indices[present]]
        taken.append(out)
    return taken


def spans(n):
    """(spans, tiles per span) of n rows"""
    tiles = -(-n // TILE)
    per_span = max(1, -(-tiles // MAX_SPANS))
    return max(1, -(-tiles // per_span)), per_span


def workspace_bytes(n):
    return 0 if n > MAX_ROWS else 4 * spans(n)[0] + 256


def selector_of(keep, width=1, reject=0, rng=None):
    """uint8 [n, width]: rows where `keep` is false hold `reject`, the others something else"""
    keep = np.asarray(keep, dtype=bool)
    values = np.full(len(keep), reject, np.uint64)
    other = np.uint64((reject + 1) % (1 << (8 * width)))
    if rng is None:
        values[keep] = other
    else:
        drawn = bits(rng.integers(0, 256, (len(keep), width), dtype=np.uint8))
        drawn[drawn == np.uint64(reject)] = other
        values[keep] = drawn[keep]
    return values.astype("<u8").view(np.uint8).reshape(len(keep), 8)[:, :width].copy()


def random_columns(rng, widths, rows):
    """uint8 [rows_j, width_j] of random bytes; rows: one number for all, or one per column"""
    rows = [rows] * len(widths) if isinstance(rows, int) else rows
    return [rng.integers(0, 256, (r, w), dtype=np.uint8) for w, r in zip(widths, rows)]


class Layout:
    """arrays in one flat uint8 buffer with CANARY between them: at odd offsets, or (`aligned`) at
    multiples of 16, or (`skews`, one per array) that many bytes behind a multiple of 16"""

    def __init__(self, arrays, aligned=False, skews=None):
        self.arrays = [np.ascontiguousarray(a) for a in arrays]
        self.at, at = [], 64
        for j, a in enumerate(self.arrays):
            skew = skews[j] if skews is not None else 0 if aligned else 1 + 2 * (j % 4)
            at = (at + 15) // 16 * 16 + skew
            self.at.append(at)
            at += a.size + 8
        self.flat = np.full(at + 64, CANARY, np.uint8)
        for a, start in zip(self.arrays, self.at):
            self.flat[start:start + a.size] = a.reshape(-1)

    def descriptors(self, base):
        """(pointer, rows, width, signed) per array with the flat buffer at `base`"""
        return [(base + start if a.shape[0] else None, a.shape[0], a.shape[1], False)
                for a, start in zip(self.arrays, self.at)]
