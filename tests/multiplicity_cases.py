"""The model of bzamd_count_multiplicities (include/blitzar_amd.h) in Python integers: the key of a
row is its value in the field (tests/column_inverse_cases.integer_values), a key's count goes to its
first row in the table, lookups of a key no table row has are misses.  Shared by
tests/test_multiplicities.py (host form), tests/test_multiplicities_host.py (the stand-alone check
of the sequential model) and tests/test_multiplicities_device.py (device form)."""
import numpy as np

from tests import column_inverse_cases as cic
from tests.test_sumcheck_device import MODULUS

CANARY = 0xA5
NARROW = [(1, False), (2, True), (8, True), (16, True), (31, False)]
KINDS = NARROW + [(32, False)]


def first_occurrences(table_keys):
    """key -> the least row that holds it"""
    first = {}
    for t, key in enumerate(table_keys):
        first.setdefault(key, t)
    return first


def count(table_keys, lookup_keys):
    """-> (multiplicities, misses)"""
    first = first_occurrences(table_keys)
    multiplicities, misses = [0] * len(table_keys), 0
    for key in lookup_keys:
        t = first.get(key)
        if t is None:
            misses += 1
        else:
            multiplicities[t] += 1
    return multiplicities, misses


def slots(table_rows):
    """the least power of two >= 2 m"""
    s = 2
    while s < 2 * table_rows:
        s *= 2
    return s


def rows_of(field_id, values, width, signed=False, raw=False):
    """uint8 [len(values), width]: integers of `width` bytes (two's complement when signed), or for
    width 32 the elements with these values, canonical; raw: the 32 bytes of the integers as they
    are (what the library may find unreduced; in field 1 Montgomery words)"""
    if width == 32:
        if not raw:
            values = [cic.element_raw(field_id, v % MODULUS[field_id]) for v in values]
        rows = [int(v).to_bytes(32, "little") for v in values]
    else:
        rows = [int(v).to_bytes(width, "little", signed=signed) for v in values]
    return np.frombuffer(b"".join(rows), np.uint8).reshape(len(values), width).copy()


def fits(value, width, signed):
    """whether the integer (negative: the field's p - |x|) is a row of this kind"""
    if width == 32:
        return True
    if signed:
        return -(1 << (8 * width - 1)) <= value < (1 << (8 * width - 1))
    return 0 <= value < (1 << (8 * width))


class Case:
    """A table (None: the range table of `table_rows` rows) and a lookup column, each uint8
    [rows, width] with its signedness, laid into one flat buffer at odd offsets (one and three
    bytes past a multiple of 8; `aligned`: at multiples of 16) between canary bytes, and what the
    call must return."""

    def __init__(self, field_id, table, lookups, table_rows=None, aligned=False):
        self.field_id = field_id
        self.table, self.lookups = table, lookups
        data, signed = lookups
        self.lookup_keys = cic.integer_values(field_id, data, signed) if data.shape[0] else []
        if table is None:
            self.m = table_rows
            self.want = ([0] * table_rows, 0)
            for key in self.lookup_keys:
                if key < table_rows:
                    self.want[0][key] += 1
                else:
                    self.want = (self.want[0], self.want[1] + 1)
        else:
            self.m = table[0].shape[0]
            self.table_keys = cic.integer_values(field_id, *table)
            self.want = count(self.table_keys, self.lookup_keys)
        assert sum(self.want[0]) + self.want[1] == len(self.lookup_keys)
        self.specs, at = [], 64
        for j, column in enumerate((table, lookups)):
            if column is None:
                self.specs.append(None)
                continue
            at = (at + 15) // 16 * 16 + (0 if aligned else (1, 3)[j])
            self.specs.append((at, column[0].shape[0], column[0].shape[1], column[1]))
            at += column[0].size + 8
        self.flat = np.full(at + 64, CANARY, np.uint8)
        for column, spec in zip((table, lookups), self.specs):
            if column is not None:
                self.flat[spec[0]:spec[0] + column[0].size] = column[0].reshape(-1)

    def want_multiplicities(self):
        return np.array(self.want[0], dtype=np.uint64)

    def descriptors(self, base):
        """(table, lookups) as (pointer, rows, width, signed) with the flat buffer at `base`"""
        out = []
        for spec in self.specs:
            if spec is None:
                out.append((None, self.m, 8, False))
            else:
                at, rows, width, signed = spec
                out.append((base + at if rows else None, rows, width, signed))
        return tuple(out)
