"""Inputs and expected results of the verifier's checks in front of the inner-product verifier
(include/blitzar_amd.h: bzamd_verify_sumcheck_device, bzamd_check_sumcheck_evaluations*,
bzamd_combine_commitments*), shared by tests/test_verify_opening.py (host forms) and
tests/test_verify_opening_device.py (device forms).  Everything is Python integers: the transcript is
tests/merlin_ref.py, the points are tests/refmath.py.  No prover is needed for a valid proof: a
round polynomial is drawn at random and one coefficient is fixed so that 2 p[0] + p[1] + .. + p[D]
is the running sum."""
import numpy as np

from blitzar_amd import api
from tests import merlin_ref, refmath
from tests.test_mle_opening import element_value
from tests.test_sumcheck import product_table
from tests.test_sumcheck_device import MODULUS, to_bytes

CANARY = 0xA5


def raw_element(field_id, value, unreduced=False):
    """32 bytes of the caller's representation of `value`; `unreduced`: the same residue, not
    canonical (+ the modulus, which is below 2^256 for both fields)"""
    p = MODULUS[field_id]
    v = int.from_bytes(bytes(to_bytes(field_id, value % p)), "little")
    if unreduced:
        v += p
        assert v < 1 << 256
    return np.frombuffer(v.to_bytes(32, "little"), np.uint8)


def random_value(rng, p):
    return int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % p


#--------------------------------------------------------------------------------------------------
# sumcheck proofs
#--------------------------------------------------------------------------------------------------
class Proof:
    """One proof of `v` variables and round degree `d` over the starting transcript `t0` (203
    bytes), and what bzamd_verify_sumcheck leaves of it, from the Python transcript.  Coefficients
    at 0, p - 1 and unreduced are among the random ones; `claimed` is unreduced for odd seeds.
    `fail_round` (None: the proof is accepted): that round's p[0] is off by one; the rounds behind
    it hold random bytes.  `point` keeps CANARY in the rows the verifier does not write."""

    def __init__(self, field_id, v, d, t0, seed, fail_round=None):
        p = MODULUS[field_id]
        rng = np.random.default_rng(seed)
        self.field_id, self.v, self.d, self.t0 = field_id, v, d, np.array(t0, np.uint8)
        self.fail_round = fail_round
        running = random_value(rng, p)
        self.claimed = raw_element(field_id, running, unreduced=seed % 2 == 1)
        self.polys = rng.integers(0, 256, (v, d + 1, 32), dtype=np.uint8)
        self.point = np.full((v, 32), CANARY, np.uint8)
        self.expected = self.claimed.copy()
        t = merlin_ref.Transcript(raw=self.t0)
        merlin_ref.sumcheck_begin(t, v, d)
        self.ok = True
        for rnd in range(v):
            c = [random_value(rng, p) for _ in range(d + 1)]
            special = int(rng.integers(0, 3))
            at = int(rng.integers(0, d + 1))
            c[at] = (0, p - 1, c[at])[special]
            fixed = (at + 1) % (d + 1)  # the coefficient that makes the round's sum right
            weight = 2 if fixed == 0 else 1
            others = 2 * c[0] + sum(c[1:]) - weight * c[fixed]
            c[fixed] = (running - others) * pow(weight, -1, p) % p
            assert (2 * c[0] + sum(c[1:])) % p == running
            if rnd == fail_round:
                c[0] = (c[0] + 1) % p
            for k in range(d + 1):
                self.polys[rnd, k] = raw_element(field_id, c[k], unreduced=special == 2 and k == at)
            if rnd == fail_round:
                self.ok = False
                break
            r_bytes = merlin_ref.sumcheck_round(t, field_id, self.polys[rnd].tobytes())
            self.point[rnd] = np.frombuffer(r_bytes, np.uint8)
            r = element_value(field_id, r_bytes)
            running = sum(ck * pow(r, k, p) for k, ck in enumerate(c)) % p
            self.expected = raw_element(field_id, running)
        self.transcript = t.array()

    def host(self):
        """bzamd_verify_sumcheck on the same bytes -> (ok, expected_sum, point, transcript)"""
        return api.verify_sumcheck(self.field_id, self.claimed, self.polys, self.t0)

    def check_host(self):
        """the host form agrees with the Python transcript (its point starts as zeros)"""
        ok, expected, point, transcript = self.host()
        written = self.written()
        assert ok == self.ok
        assert np.array_equal(expected, self.expected)
        assert np.array_equal(point[:written], self.point[:written])
        assert not point[written:].any()
        assert np.array_equal(transcript, self.transcript)

    def written(self):
        """rows of the point the verifier writes"""
        return self.v if self.ok else self.fail_round


def fail_rounds_of(v):
    """None (accepted), then the failing round at 0, in the middle and last, without repeats"""
    return [None] + sorted({0, v // 2, v - 1})


#--------------------------------------------------------------------------------------------------
# the final evaluation check
#--------------------------------------------------------------------------------------------------
class Statement:
    """`num_products` products of 1 .. 8 terms over 9 MLEs; the multipliers hold 0, 1, p - 1 and an
    unreduced one among random ones (where there are that many)"""
    NUM_MLES = 9

    def __init__(self, field_id, num_products, seed):
        p = MODULUS[field_id]
        rng = np.random.default_rng(seed)
        self.field_id, self.num_products = field_id, num_products
        self.lengths = [1 + (k + seed) % 8 for k in range(num_products)]
        self.terms = [int(j) for n in self.lengths for j in rng.integers(0, self.NUM_MLES, n)]
        self.multipliers = [random_value(rng, p) for _ in range(num_products)]
        rows = [raw_element(field_id, m) for m in self.multipliers]
        for k, (value, unreduced) in enumerate([(0, False), (1, False), (p - 1, False),
                                                (random_value(rng, p), True)]):
            at = (seed + 3 * k) % num_products
            if num_products > 4 or k == seed % 4:
                self.multipliers[at] = value
                rows[at] = raw_element(field_id, value, unreduced)
        self.table = product_table(field_id, rows, self.lengths,
                                   api.SUMCHECK_PRODUCT_STRIDE[field_id])

    def evaluations(self, seed):
        """-> (uint8 [NUM_MLES, 32] with 0, 1, p - 1 and an unreduced entry, their values)"""
        p = MODULUS[self.field_id]
        rng = np.random.default_rng(seed)
        values = [random_value(rng, p) for _ in range(self.NUM_MLES)]
        values[seed % 9], values[(seed + 2) % 9], values[(seed + 4) % 9] = 0, 1, p - 1
        rows = [raw_element(self.field_id, x, unreduced=j == (seed + 6) % 9)
                for j, x in enumerate(values)]
        return np.stack(rows), values

    def expected_sum(self, values):
        p, total, at = MODULUS[self.field_id], 0, 0
        for m, n in zip(self.multipliers, self.lengths):
            term = m
            for j in self.terms[at:at + n]:
                term = term * values[j] % p
            total, at = (total + term) % p, at + n
        return total


def flipped(raw, bit):
    out = np.array(raw, np.uint8).copy()
    out[bit // 8] ^= 1 << (bit % 8)
    return out


#--------------------------------------------------------------------------------------------------
# compressed commitments
#--------------------------------------------------------------------------------------------------
def decode_class(s):
    """why the ristretto decoder rejects the integer s (RFC 9496 4.3.1), or None"""
    P, D = refmath.P, refmath.D
    if s >= P:
        return "non-canonical"
    if s & 1:
        return "negative s"
    ss = s * s % P
    u1, u2 = (1 - ss) % P, (1 + ss) % P
    v = (-D * u1 * u1 - u2 * u2) % P
    was_square, invsqrt = refmath.sqrt_ratio_m1(1, v * u2 * u2)
    if not was_square:
        return "non-square"
    x = invsqrt * u2 % P
    y = invsqrt * x * v % P
    x = 2 * s * x % P
    if x & 1:
        x = P - x
    y = u1 * y % P
    if (x * y % P) & 1 or y == 0:
        return "negative t or y = 0"
    return None


REJECTION_CLASSES = ("non-canonical", "negative s", "non-square", "negative t or y = 0")


def rejected_encodings():
    """-> {class: 32 bytes}: p itself, 1, and the first even s of each of the other two classes"""
    found = {"non-canonical": refmath.P, "negative s": 1}
    s = 2
    while len(found) < 4:
        why = decode_class(s)
        if why is not None and why not in found:
            found[why] = s
        s += 2
        assert s < 4096, "no rejected even s of some class among the first 2048"
    return {why: np.frombuffer(v.to_bytes(32, "little"), np.uint8) for why, v in found.items()}


class Commitments:
    """K commitments encode(k_j B) with known k_j (the identity's encoding among them from K = 3 on)
    and K coefficients with 0, l - 1, l and 2^256 - 1 among random 256-bit ones.  `rejected`:
    {index: encoding the decoder rejects}; those terms are left out of the expected sum"""

    def __init__(self, count, seed, rejected=None):
        L = refmath.ED_L
        rng = np.random.default_rng(seed)
        first, step = int(rng.integers(1, 1 << 40)), int(rng.integers(1, 1 << 40))
        self.logs = [first + step * j for j in range(count)]
        points = refmath.ed_multiples(count, first, step)
        self.commitments = np.stack([np.frombuffer(refmath.ristretto_encode(refmath.ed_extended(pt)),
                                                   np.uint8) for pt in points]).copy()
        if count >= 3:
            self.logs[count // 2] = 0
            self.commitments[count // 2] = 0
        values = [int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little")
                  for _ in range(count)]
        for k, edge in enumerate((0, L - 1, L, (1 << 256) - 1)):
            if count > 4 or k == seed % 4:
                values[(seed + 5 * k) % count] = edge
        self.values = values
        self.coefficients = np.stack([np.frombuffer(v.to_bytes(32, "little"), np.uint8)
                                      for v in values]).copy()
        self.rejected = dict(rejected or {})
        for at, encoding in self.rejected.items():
            self.commitments[at] = encoding
        self.valid = not self.rejected

    def expected_encoding(self):
        total = sum(c * k for j, (c, k) in enumerate(zip(self.values, self.logs))
                    if j not in self.rejected) % refmath.ED_L
        point = refmath.ed_mul(total, refmath.ED_BASE)
        return np.frombuffer(refmath.ristretto_encode(refmath.ed_extended(point)), np.uint8)


def encoding_of(combined):
    """the canonical encoding of one sxt_ristretto255 of any Z (uint64 [20] or its 160 bytes)"""
    raw = np.ascontiguousarray(combined).view(np.uint8).reshape(1, 1, 160)
    return api.fold_encode(api.SXT_CURVE_RISTRETTO255, raw)[0]
