"""The model of bzamd_decompose_words and bzamd_map_words (include/blitzar_amd.h) in Python
integers: key(i) is the value of shift + column[i] in the field, word k its byte k, counts the
histogram of all words, overflow the rows whose key does not fit the planes; a mapped row is the
table row of its word.  Shared by tests/test_word_columns.py (host forms) and
tests/test_word_columns_device.py (device forms)."""
import numpy as np

from tests import column_inverse_cases as cic
from tests import multiplicity_cases as mc
from tests.test_sumcheck_device import MODULUS

CANARY = 0xA5
CANARY_WORD = int.from_bytes(bytes([CANARY]) * 8, "little")


def keys_of(field_id, column, shift=None):
    """column: (uint8 [rows, width], signed); shift: the integer the 32 bytes of `shift` hold as
    they are (element form, may be unreduced), or None -> the keys, integers in [0, p)"""
    p = MODULUS[field_id]
    data, signed = column
    values = cic.integer_values(field_id, data, signed) if data.shape[0] else []
    s = 0 if shift is None else cic.raw_value(field_id, shift)
    return [(v + s) % p for v in values]


def decompose(keys, num_words):
    """-> (words uint8 [num_words, n], counts [256], overflow)"""
    words = np.zeros((num_words, len(keys)), np.uint8)
    counts, overflow = [0] * 256, 0
    for i, key in enumerate(keys):
        for k in range(num_words):
            word = (key >> (8 * k)) & 0xFF
            words[k, i] = word
            counts[word] += 1
        overflow += 1 if key >> (8 * num_words) else 0
    assert sum(counts) == num_words * len(keys)
    return words, counts, overflow


def shift_bytes(raw):
    """the 32 bytes that hold the integer `raw`"""
    return np.frombuffer(int(raw).to_bytes(32, "little"), np.uint8).copy()


def distinct_table():
    """256 rows of 32 bytes: byte b differs from row to row and between the halves of a row"""
    v = np.arange(256, dtype=np.uint32).reshape(256, 1)
    b = np.arange(32, dtype=np.uint32).reshape(1, 32)
    table = ((v ^ (11 * b)) & 0xFF).astype(np.uint8)
    assert all(len(set(table[:, j].tolist())) == 256 for j in range(32))
    assert not np.any(table[:, :16] == table[:, 16:])
    return table


def mapped(words, table):
    """words uint8 [planes, n], table uint8 [256, 32] -> uint8 [planes, n, 32], row by row"""
    out = np.zeros(words.shape + (32,), np.uint8)
    for k in range(words.shape[0]):
        for i in range(words.shape[1]):
            out[k, i] = table[int(words[k, i])]
    return out


def column_of(field_id, values, width, signed=False):
    """(uint8 [rows, width], signed): integers of `width` bytes, or for width 32 the elements with
    these values (negative: p - |x|), canonical"""
    if width == 32:
        return (mc.rows_of(field_id, [v % MODULUS[field_id] for v in values], 32), False)
    return (mc.rows_of(field_id, values, width, signed), signed)


def drawn(rng, count, width, signed):
    """values a column of this kind holds, the extremes first"""
    bits = 8 * min(width, 31)
    low, high = (-(1 << (bits - 1)), 1 << (bits - 1)) if signed else (0, 1 << bits)
    values = [low + int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little")
              % (high - low) for _ in range(count)]
    values[:4] = [low, high - 1, 0, 1 if not signed else -1]
    return values


class Layout:
    """Where the buffers of one decomposition lie in one flat buffer of canary bytes: the column
    `column_skew` bytes past a multiple of 16, the planes `plane_skew` past one and plane_stride
    apart, counts and overflow 8-byte aligned with a canary word on either side, the shift at an
    odd address."""

    def __init__(self, column, num_words, shift=None, gap=0, column_skew=1, plane_skew=3):
        data, self.signed = column
        self.n, self.width = data.shape
        self.num_words, self.plane_stride = num_words, self.n + gap
        at = 64 + column_skew
        self.column_at, at = at, at + data.size
        at = (at + 31) // 16 * 16 + 5
        self.shift_at, at = (at if shift is not None else None), at + 32
        at = (at + 31) // 16 * 16 + plane_skew
        self.words_at, at = at, at + num_words * self.plane_stride
        at = (at + 31) // 8 * 8
        self.counts_at, at = at + 8, at + 8 * 258
        self.overflow_at, at = at + 8, at + 24
        self.flat = np.full(at + 64, CANARY, np.uint8)
        self.flat[self.column_at:self.column_at + data.size] = data.reshape(-1)
        if shift is not None:
            self.flat[self.shift_at:self.shift_at + 32] = shift_bytes(shift)
        self.before = self.flat.copy()

    def check(self, flat, want, outputs=("words", "counts", "overflow")):
        """flat: the buffer after the call; want: decompose()'s triple.  Everything but the asked
        outputs is what it was"""
        flat = np.asarray(flat)
        words, counts, overflow = want
        expected = self.before.copy()
        if "words" in outputs:
            for k in range(self.num_words):
                at = self.words_at + k * self.plane_stride
                expected[at:at + self.n] = words[k]
        if "counts" in outputs:
            expected[self.counts_at:self.counts_at + 2048] = np.array(counts, np.uint64).view(np.uint8)
        if "overflow" in outputs:
            expected[self.overflow_at:self.overflow_at + 8] = np.array([overflow], np.uint64).view(np.uint8)
        wrong = np.nonzero(flat != expected)[0]
        assert wrong.size == 0, (
            f"{wrong.size} bytes differ, the first at {int(wrong[0])} (column {self.column_at}, "
            f"words {self.words_at} stride {self.plane_stride}, counts {self.counts_at}, "
            f"overflow {self.overflow_at}): got {int(flat[wrong[0]])}, want {int(expected[wrong[0]])}")

    def pointers(self, base, outputs=("words", "counts", "overflow")):
        """(words, counts, overflow, column descriptor tuple, shift) with the buffer at `base`"""
        column = (base + self.column_at if self.n else None, self.n, self.width, self.signed)
        return (base + self.words_at if "words" in outputs else None,
                base + self.counts_at if "counts" in outputs else None,
                base + self.overflow_at if "overflow" in outputs else None, column,
                None if self.shift_at is None else base + self.shift_at)
