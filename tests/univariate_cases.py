"""The model of the univariate-opening entry points (include/blitzar_amd.h: bzamd_fold_polynomial,
bzamd_evaluate_polynomials, bzamd_batch_quotients) in Python integers, the byte helpers of both
forms, and the BN254 points of the pairing-free check.  Shared by tests/test_univariate_opening.py
(host forms) and tests/test_univariate_opening_device.py (device forms)."""
import functools

import numpy as np

from tests import refmath
from tests.test_sumcheck_device import MODULUS, to_bytes, to_int


def folded_layout(n, num_variables):
    """[(offset, length)] of P_1 .. P_{l-1} in `folded`"""
    out, offset, length = [], 0, n
    for _ in range(1, num_variables):
        length = (length + 1) // 2
        out.append((offset, length))
        offset += length
    return out


def levels(field_id, p0, point):
    """([P_0, P_1, .. P_{l-1}], evaluation): P_i[j] = P_{i-1}[2j] + x_{l-i} (P_{i-1}[2j+1] -
    P_{i-1}[2j]), a missing P_{i-1}[2j+1] being 0"""
    p, num_variables = MODULUS[field_id], len(point)
    out = [[v % p for v in p0]]
    for i in range(1, num_variables + 1):
        x, prev = point[num_variables - i], out[-1]
        low, high = prev[0::2], prev[1::2]
        high = high + [0] * (len(low) - len(high))
        out.append([(a + x * (b - a)) % p for a, b in zip(low, high)])
    return out[:num_variables], out[num_variables][0]


def evaluate(field_id, rows, u):
    """sum_j rows[j] u^j"""
    p, acc = MODULUS[field_id], 0
    for v in reversed(rows):
        acc = (acc * u + v) % p
    return acc


def batched(field_id, all_levels, q):
    """B[m] = sum_{i, m < len_i} q^i P_i[m]"""
    p = MODULUS[field_id]
    out, power = [0] * len(all_levels[0]), 1
    for rows in all_levels:
        for m, v in enumerate(rows):
            out[m] = (out[m] + power * v) % p
        power = power * q % p
    return out


def quotient(field_id, b, u):
    """(h, remainder) with B(X) = (X - u) h(X) + remainder: h[j-1] = B[j] + u h[j], h[n-1] = 0"""
    p = MODULUS[field_id]
    h, carry = [0] * len(b), 0
    for j in range(len(b) - 1, -1, -1):
        h[j] = carry
        carry = (b[j] + u * carry) % p
    return h, carry


#--------------------------------------------------------------------------------------------------
# bytes
#--------------------------------------------------------------------------------------------------
def element_rows(field_id, values):
    """element form, [len, 32]"""
    if len(values) == 0:
        return np.zeros((0, 32), np.uint8)
    p = MODULUS[field_id]
    if field_id == 1:
        values = [v * (1 << 256) % p for v in values]
    raw = b"".join((v % p).to_bytes(32, "little") for v in values)
    return np.frombuffer(raw, np.uint8).reshape(-1, 32).copy()


def scalar_rows(field_id, values):
    """scalar form, [len, 32]: the canonical value as a plain little-endian integer"""
    if len(values) == 0:
        return np.zeros((0, 32), np.uint8)
    p = MODULUS[field_id]
    raw = b"".join((v % p).to_bytes(32, "little") for v in values)
    return np.frombuffer(raw, np.uint8).reshape(-1, 32).copy()


def scalar_values(rows):
    return [int.from_bytes(bytes(r), "little") for r in np.asarray(rows).reshape(-1, 32)]


def element_values(field_id, rows):
    return [to_int(field_id, r) for r in np.asarray(rows).reshape(-1, 32)]


def folded_rows(field_id, all_levels, scalar=False):
    """P_1 .. P_{l-1} back to back in element (or scalar) form"""
    flat = [v for rows in all_levels[1:] for v in rows]
    return scalar_rows(field_id, flat) if scalar else element_rows(field_id, flat)


def random_values(field_id, n, seed):
    """n values below p with 0, 1 and p - 1 among them"""
    p = MODULUS[field_id]
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    out = [int.from_bytes(r.tobytes(), "little") % p for r in raw]
    for k, special in enumerate((p - 1, 0, 1)):
        if n > 2 * k + 1:
            out[(seed + 2 * k) % n] = special
    return out


def points_of(field_id, num_points, seed):
    """num_points evaluation points: the triple (r, -r, r^2) first for seed 0, else 0, 1, p - 1 and
    random ones at places that move with the seed"""
    p = MODULUS[field_id]
    rng = np.random.default_rng(1000 + seed)
    r = int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % p
    if seed == 0:
        return [r, (p - r) % p, r * r % p, 0][:num_points]
    pool = [0, 1, p - 1, r]
    return [pool[(seed + k) % 4] for k in range(num_points)]


class Opening:
    """the model of one opening: polynomial of n rows, l variables, t points, one q"""

    def __init__(self, field_id, num_variables, n, seed, num_points=3, q=None, point=None):
        from tests.test_mle_opening import point_of
        p = MODULUS[field_id]
        self.field_id, self.num_variables, self.n = field_id, num_variables, n
        self.p0 = random_values(field_id, n, seed)
        self.point = point_of(field_id, num_variables, seed) if point is None else point
        self.levels, self.evaluation = levels(field_id, self.p0, self.point)
        self.points = points_of(field_id, num_points, seed)
        self.q = random_values(field_id, 1, seed + 77)[0] if q is None else q % p

    def polynomial_bytes(self):
        return element_rows(self.field_id, self.p0)

    def point_bytes(self):
        return element_rows(self.field_id, self.point)

    def points_bytes(self):
        return element_rows(self.field_id, self.points)

    def q_bytes(self):
        return element_rows(self.field_id, [self.q])[0]

    def folded_bytes(self, scalar=False):
        return folded_rows(self.field_id, self.levels, scalar)

    def evaluations(self):
        """[k][i] = P_i(u_k)"""
        return [[evaluate(self.field_id, rows, u) for rows in self.levels] for u in self.points]

    def batched(self):
        return batched(self.field_id, self.levels, self.q)

    def quotients(self):
        """([h_k], [remainder_k])"""
        b = self.batched()
        pairs = [quotient(self.field_id, b, u) for u in self.points]
        return [h for h, _ in pairs], [r for _, r in pairs]


#--------------------------------------------------------------------------------------------------
# BN254 G1: the commitments of the pairing-free check (field 1 is its scalar field)
#--------------------------------------------------------------------------------------------------
BN = refmath.BN254
TAU = 0x1d3a5f7c9b2e4d6f8a1c3e5079b2d4f6a8c0e1f3057192b3d5f7a9c1e3f50719 % MODULUS[1]


SMALL_TAU = 5  # for generator sets of thousands of points: a step is three curve operations


@functools.lru_cache(maxsize=None)
def tau_generators(count, tau=TAU):
    """G_i = tau^i G, i < count, affine"""
    out, current = [], BN.base
    for _ in range(count):
        out.append(current)
        current = BN.mul(tau, current)
    return out


def affine_bytes(points):
    """affine points (None: the identity) in the C ABI's 72-byte layout: x, y in Montgomery form
    (R = 2^256) and the infinity flag"""
    out = np.zeros((len(points), 72), np.uint8)
    for i, pt in enumerate(points):
        if pt is None:
            raw = (0).to_bytes(32, "little") + (BN.R64 % BN.p).to_bytes(32, "little") + b"\x01"
        else:
            raw = ((pt[0] * BN.R64 % BN.p).to_bytes(32, "little") +
                   (pt[1] * BN.R64 % BN.p).to_bytes(32, "little") + b"\x00")
        out[i, :len(raw)] = np.frombuffer(raw, np.uint8)
    return out


def affine_point(raw):
    raw = bytes(raw)
    if raw[64] != 0:
        return None
    ri = refmath.inv(BN.R64, BN.p)
    pt = (int.from_bytes(raw[:32], "little") * ri % BN.p,
          int.from_bytes(raw[32:64], "little") * ri % BN.p)
    assert BN.on_curve(pt)
    return pt


def opening_equation_holds(num_variables, q, points, level_commitments, quotient_commitments,
                           remainders, tau=TAU):
    """(tau - u_k) C(h_k) + remainders[k] G == sum_i q^i C(P_i) for every k; commitments as affine
    points, remainders as integers"""
    p = MODULUS[1]
    assert len(level_commitments) == num_variables
    right, power = None, 1
    for c in level_commitments:
        right = BN.add(right, BN.mul(power, c))
        power = power * q % p
    for u, c, rem in zip(points, quotient_commitments, remainders):
        left = BN.add(BN.mul((tau - u) % p, c), BN.mul(rem % p, BN.base))
        if left != right:
            return False
    return True
