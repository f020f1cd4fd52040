"""The model of bzamd_invert_columns (include/blitzar_amd.h) in Python integers:
denominator[i] = shift + sum_j coefficients[j] column_j[i], inverses[i] = denominator[i]^-1 with
zero kept as zero, and the bytes of both output forms (tests/univariate_cases.py).  Shared by
tests/test_column_inverse.py (host form) and tests/test_column_inverse_device.py (device form)."""
import numpy as np

from tests.test_mle_opening import element_value
from tests.test_sumcheck_device import MODULUS
from tests.univariate_cases import element_rows, scalar_rows


def denominators(field_id, values, coefficients, shift, n):
    """values[j]: the rows of column j as field integers (at most n, the rest is zero);
    coefficients: integers or None (all 1); shift: an integer or None (0)"""
    p = MODULUS[field_id]
    out = [(shift or 0) % p] * n
    for j, rows in enumerate(values):
        c = 1 if coefficients is None else coefficients[j]
        for i, x in enumerate(rows):
            out[i] = (out[i] + c * x) % p
    return out


def inverses(field_id, ds):
    """pow per row, zero kept as zero"""
    p = MODULUS[field_id]
    return [pow(d, -1, p) if d % p else 0 for d in ds]


def batch_inverses(field_id, ds):
    """the same by Montgomery's trick: three multiplications a row and one pow"""
    p = MODULUS[field_id]
    prefix, acc = [], 1
    for d in ds:
        prefix.append(acc)
        if d:
            acc = acc * d % p
    inv = pow(acc, -1, p)
    out = [0] * len(ds)
    for i in range(len(ds) - 1, -1, -1):
        if ds[i]:
            out[i] = inv * prefix[i] % p
            inv = inv * ds[i] % p
    return out


def element_bytes(field_id, raw):
    """32 bytes that hold the integer `raw` as they are: an element the library may find unreduced"""
    return np.frombuffer(int(raw).to_bytes(32, "little"), np.uint8).copy()


def raw_value(field_id, raw):
    """what those 32 bytes mean"""
    return element_value(field_id, element_bytes(field_id, raw))


def element_raw(field_id, value):
    """the integer whose 32 bytes are `value` in element form, canonical"""
    p = MODULUS[field_id]
    return value * (1 << 256) % p if field_id == 1 else value % p


def integer_values(field_id, column, signed):
    """rows of a 1-D integer array or a uint8 [rows, width] array as field integers"""
    p = MODULUS[field_id]
    column = np.ascontiguousarray(column)
    if column.ndim == 1:
        return [int(x) % p for x in column]
    if column.shape[1] == 32:
        return [element_value(field_id, row) for row in column]
    return [int.from_bytes(row.tobytes(), "little", signed=signed) % p for row in column]


def expected_bytes(field_id, inv):
    """(element form, scalar form), uint8 [n, 32] each"""
    return element_rows(field_id, inv), scalar_rows(field_id, inv)
