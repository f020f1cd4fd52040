"""The model of bzamd_sum_by_key (include/blitzar_amd.h) in Python integers: keys, first
occurrences, counts and misses are those of tests/multiplicity_cases.py; the value of a row is its
value in the field (tests/column_inverse_cases.integer_values); a key's sums go to its first row in
the table, lookups that miss contribute nowhere.  Shared by tests/test_key_sums.py (host form) and
tests/test_key_sums_device.py (device form)."""
import numpy as np

from tests import column_inverse_cases as cic
from tests import multiplicity_cases as mc
from tests.test_sumcheck_device import MODULUS
from tests.univariate_cases import element_rows, scalar_rows

MISS = 0xFFFFFFFF
CANARY = mc.CANARY
MAX_VALUES = 8


def chunks_of(width):
    """32-bit accumulators of a value column of this width"""
    return (width + 3) // 4


def sum_by_key(field_id, table_keys, lookup_keys, value_columns, table_rows=None):
    """table_keys: field integers, or None for the range table of table_rows rows; value_columns:
    lists of field integers, each at most as long as lookup_keys
    -> (sums [num_values][m], counts [m], misses, matches [n])"""
    p = MODULUS[field_id]
    if table_keys is None:
        m, first = table_rows, None
    else:
        m, first = len(table_keys), mc.first_occurrences(table_keys)
    sums = [[0] * m for _ in value_columns]
    counts, misses, matches = [0] * m, 0, []
    for i, key in enumerate(lookup_keys):
        t = (key if key < m else None) if first is None else first.get(key)
        if t is None:
            misses += 1
            matches.append(MISS)
            continue
        matches.append(t)
        counts[t] += 1
        for v, column in enumerate(value_columns):
            if i < len(column):
                sums[v][t] = (sums[v][t] + column[i]) % p
    return sums, counts, misses, matches


class Case(mc.Case):
    """mc.Case (table and lookups in one flat buffer between canaries) with value columns, each
    uint8 [rows, width] with its signedness, in a second flat buffer at odd offsets (`aligned`: at
    multiples of 16), and what the call must return"""

    def __init__(self, field_id, table, lookups, values, table_rows=None, aligned=False):
        super().__init__(field_id, table, lookups, table_rows=table_rows, aligned=aligned)
        self.values = list(values)
        self.n = lookups[0].shape[0]
        self.value_ints = [cic.integer_values(field_id, data, signed) if data.shape[0] else []
                           for data, signed in self.values]
        table_keys = None if table is None else self.table_keys
        self.sums, counts, misses, self.matches = sum_by_key(
            field_id, table_keys, self.lookup_keys, self.value_ints, self.m)
        assert (counts, misses) == (list(self.want[0]), self.want[1])
        self.row_chunks = sum(chunks_of(data.shape[1]) for data, _ in self.values)
        self.value_specs, at = [], 64
        for j, (data, signed) in enumerate(self.values):
            at = (at + 15) // 16 * 16 + (0 if aligned else 1 + 2 * (j % 4))
            self.value_specs.append((at, data.shape[0], data.shape[1], signed))
            at += data.size + 8
        self.value_flat = np.full(at + 64, CANARY, np.uint8)
        for (data, _), spec in zip(self.values, self.value_specs):
            self.value_flat[spec[0]:spec[0] + data.size] = data.reshape(-1)

    def want_sums(self):
        """element form, uint8 [num_values, m, 32]"""
        return np.stack([element_rows(self.field_id, s) for s in self.sums]) if self.sums else \
            np.zeros((0, self.m, 32), np.uint8)

    def want_scalars(self):
        return np.stack([scalar_rows(self.field_id, s) for s in self.sums]) if self.sums else \
            np.zeros((0, self.m, 32), np.uint8)

    def want_counts(self):
        return self.want_multiplicities()

    def want_matches(self):
        return np.array(self.matches, dtype=np.uint32)

    def value_descriptors(self, base):
        """the value columns as (pointer, rows, width, signed) with value_flat at `base`"""
        return [(base + at if rows else None, rows, width, signed)
                for at, rows, width, signed in self.value_specs]


def column(field_id, values, kind):
    """(uint8 [rows, width], signed) of integers (negative: p - |x| in a 32-byte column)"""
    width, signed = kind
    if width == 32:
        return (mc.rows_of(field_id, [v % MODULUS[field_id] for v in values], 32), False)
    return (mc.rows_of(field_id, values, width, signed), signed)


def i64_column(values):
    return (np.array(values, np.int64).view(np.uint8).reshape(len(values), 8), True)


def extremes(kind):
    """the least and the largest row of a narrow kind"""
    width, signed = kind
    if signed:
        return -(1 << (8 * width - 1)), (1 << (8 * width - 1)) - 1
    return 0, (1 << (8 * width)) - 1


def drawn(rng, kind, count):
    """rows of a kind: random, with its extremes among them"""
    width, signed = kind
    if width == 32:
        return [int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little")
                for _ in range(count)]
    low, high = extremes(kind)
    values = [int.from_bytes(rng.integers(0, 256, width, dtype=np.uint8).tobytes(), "little",
                             signed=signed) for _ in range(count)]
    for at, value in zip((0, 1, 2, 3), (low, high, high, low)):
        if at < count:
            values[at] = value
    return values
