"""Merlin over STROBE-128 over Keccak-f[1600] in plain Python integers, and the sumcheck use of it
(the reference's prfsk::reference_transcript): test infrastructure, the expected side of
tests/test_sumcheck_transcript.py.  Written from the public specifications (FIPS 202, the STROBE
and Merlin papers) and pinned to the compiled reference by tests/test_merlin_ref.py.

A transcript here is the 203-byte array the C ABI passes around (`sxt_transcript`): 200 bytes of
sponge state, then pos, pos_begin, cur_flags."""
import ctypes

import numpy as np

L_ORDER = 2**252 + 27742317777372353535851937790883648493
GK_P = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
RATE = 166
FLAG_I, FLAG_A, FLAG_C, FLAG_T, FLAG_M, FLAG_K = 1, 2, 4, 8, 16, 32
MASK = (1 << 64) - 1


def _round_constants():
    # FIPS 202 algorithm 5: the LFSR x^8 + x^6 + x^5 + x^4 + 1
    out, r = [], 1
    for _ in range(24):
        rc = 0
        for j in range(7):
            if r & 1:
                rc |= 1 << ((1 << j) - 1)
            r <<= 1
            if r & 0x100:
                r ^= 0x171
        out.append(rc)
    return out


def _rotations():
    # FIPS 202 algorithm 2: (x, y) walks (1, 0) -> (y, 2x + 3y), offset (t + 1)(t + 2) / 2
    rot = [[0] * 5 for _ in range(5)]
    x, y = 1, 0
    for t in range(24):
        rot[x][y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5
    return rot


RC = _round_constants()
ROT = _rotations()


def _rotl(v, s):
    return ((v << s) | (v >> (64 - s))) & MASK if s else v


def keccak_f1600(state):
    """200 bytes -> 200 bytes"""
    a = [int.from_bytes(state[8 * i:8 * i + 8], "little") for i in range(25)]
    for rnd in range(24):
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        d = [c[(x + 4) % 5] ^ _rotl(c[(x + 1) % 5], 1) for x in range(5)]
        a = [a[i] ^ d[i % 5] for i in range(25)]
        b = [0] * 25
        for x in range(5):
            for y in range(5):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = _rotl(a[x + 5 * y], ROT[x][y])
        a = [b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & MASK & b[(x + 2) % 5 + 5 * y])
             for y in range(5) for x in range(5)]
        a[0] ^= RC[rnd]
    return b"".join(v.to_bytes(8, "little") for v in a)


class Transcript:
    """Merlin on a bytearray of 203 bytes"""

    def __init__(self, raw=None, label=None):
        if raw is not None:
            self.raw = bytearray(bytes(raw))
            assert len(self.raw) == 203
            return
        self.raw = bytearray(203)
        self.raw[:18] = bytes([1, RATE + 2, 1, 0, 1, 96]) + b"STROBEv1.0.2"
        self.raw[:200] = keccak_f1600(bytes(self.raw[:200]))
        self._meta_ad(b"Merlin v1.0", False)
        self.append_message(b"dom-sep", label.encode() if isinstance(label, str) else bytes(label))

    def array(self):
        return np.frombuffer(bytes(self.raw), np.uint8).copy()

    # STROBE-128
    def _run_f(self):
        s = self.raw
        s[s[200]] ^= s[201]
        s[s[200] + 1] ^= 0x04
        s[RATE + 1] ^= 0x80
        s[:200] = keccak_f1600(bytes(s[:200]))
        s[200] = 0
        s[201] = 0

    def _absorb(self, data):
        s = self.raw
        for byte in data:
            s[s[200]] ^= byte
            s[200] += 1
            if s[200] == RATE:
                self._run_f()

    def _squeeze(self, n):
        s, out = self.raw, bytearray()
        for _ in range(n):
            out.append(s[s[200]])
            s[s[200]] = 0
            s[200] += 1
            if s[200] == RATE:
                self._run_f()
        return bytes(out)

    def _begin_op(self, flags, more):
        if more:
            return
        s = self.raw
        old_begin = s[201]
        s[201] = (s[200] + 1) & 0xff
        s[202] = flags
        self._absorb(bytes([old_begin, flags]))
        if flags & (FLAG_C | FLAG_K) and s[200] != 0:
            self._run_f()

    def _meta_ad(self, data, more):
        self._begin_op(FLAG_M | FLAG_A, more)
        self._absorb(data)

    def _ad(self, data, more):
        self._begin_op(FLAG_A, more)
        self._absorb(data)

    def _prf(self, n, more):
        self._begin_op(FLAG_I | FLAG_A | FLAG_C, more)
        return self._squeeze(n)

    # Merlin
    def append_message(self, label, message):
        self._meta_ad(bytes(label), False)
        self._meta_ad(len(message).to_bytes(4, "little"), True)
        self._ad(bytes(message), False)

    def challenge_bytes(self, label, n):
        self._meta_ad(bytes(label), False)
        self._meta_ad(int(n).to_bytes(4, "little"), True)
        return self._prf(n, False)

    def append_u64(self, label, v):
        self.append_message(label, int(v).to_bytes(8, "little"))


def challenge_from_bytes(field_id, x):
    """prft::challenge_value: the 32 bytes of r, in the caller's representation, from the 32
    squeezed bytes.  Scalars: the integer mod l.  Grumpkin: one Montgomery reduction (R = 2^256) of
    the integer, canonical -- those bytes are then the element."""
    v = int.from_bytes(x, "little")
    if field_id == 0:
        return (v % L_ORDER).to_bytes(32, "little")
    return (v * pow(1 << 256, -1, GK_P) % GK_P).to_bytes(32, "little")


def sumcheck_begin(t, num_variables, round_degree):
    t.append_message(b"domain-sep", b"sumcheck proof v1")
    t.append_u64(b"n", num_variables)
    t.append_u64(b"k", round_degree)


def sumcheck_round(t, field_id, polynomial):
    t.append_message(b"P", polynomial)
    return challenge_from_bytes(field_id, t.challenge_bytes(b"R", 32))


def sumcheck_callback(t, field_id):
    """the transcript as the callback of a prover's C ABI; sumcheck_begin is the caller's"""
    def cb(r_ptr, ctx, poly_ptr, length):
        r = sumcheck_round(t, field_id, ctypes.string_at(poly_ptr, 32 * length))
        ctypes.memmove(r_ptr, r, 32)
    return cb


#--------------------------------------------------------------------------------------------------
# the model instrumented: which edges of the 166-byte rate boundary a sequence of operations reaches
#--------------------------------------------------------------------------------------------------
# the sponge fills up (position RATE, a permutation) inside a run of bytes or on its last byte, per
# kind of run: the 2-byte header of an operation, a label, the 4-byte length, a message
ABSORB_CLASSES = frozenset(f"{kind}-{where}" for kind in ("header", "label", "length", "message")
                           for where in ("inside", "last"))
# a prf whose header leaves the position off / on the boundary: begin_op forces a permutation / must not
PRF_CLASSES = frozenset(("prf-forced", "prf-unforced"))
BOUNDARY_CLASSES = ABSORB_CLASSES | PRF_CLASSES          # what 32-byte challenges can reach
SQUEEZE_CROSS = "squeeze-cross"                           # a squeeze that goes on across the boundary


class TracedTranscript(Transcript):
    """Transcript that records in `classes` the boundary classes its operations reached and in
    `starts` the position every operation began at"""

    def __init__(self, raw=None, label=None):
        self.classes, self.starts, self._kind = set(), [], "label"
        super().__init__(raw, label)

    def _absorb(self, data):
        s = self.raw
        for i, byte in enumerate(data):
            s[s[200]] ^= byte
            s[200] += 1
            if s[200] == RATE:
                self._run_f()
                self.classes.add(f"{self._kind}-{'last' if i + 1 == len(data) else 'inside'}")

    def _squeeze(self, n):
        s, out = self.raw, bytearray()
        for i in range(n):
            out.append(s[s[200]])
            s[s[200]] = 0
            s[200] += 1
            if s[200] == RATE:
                self._run_f()
                if i + 1 < n:
                    self.classes.add(SQUEEZE_CROSS)
        return bytes(out)

    def _begin_op(self, flags, more):
        if more:
            return
        s = self.raw
        self.starts.append(s[200])
        old_begin = s[201]
        s[201] = (s[200] + 1) & 0xff
        s[202] = flags
        kind, self._kind = self._kind, "header"
        self._absorb(bytes([old_begin, flags]))
        self._kind = kind
        if flags & (FLAG_C | FLAG_K):
            if s[200] != 0:
                self._run_f()
                self.classes.add("prf-forced")
            else:
                self.classes.add("prf-unforced")

    def _meta_ad(self, data, more):
        self._kind = "length" if more else "label"
        super()._meta_ad(data, more)

    def _ad(self, data, more):
        self._kind = "message"
        super()._ad(data, more)


def padded_starts(label=b"sweep"):
    """166 transcripts, the k-th at STROBE position k: a fresh transcript and one padding message of
    0 .. 165 bytes (each more byte moves the position on by one, modulo the rate)"""
    starts = {}
    for k in range(RATE):
        t = Transcript(label=label)
        t.append_message(b"pad", bytes(k))
        starts[t.raw[200]] = t.array()
    assert sorted(starts) == list(range(RATE)), "the padded transcripts miss a position"
    return [starts[k] for k in range(RATE)]


def inner_product_begin(t, n):
    t.append_message(b"domain-sep", b"inner product proof v1")
    t.append_u64(b"n", n)


def inner_product_round(t, l_value, r_value):
    """-> the 32 squeezed bytes x (the challenge is the integer x mod l)"""
    t.append_message(b"L", l_value)
    t.append_message(b"R", r_value)
    return t.challenge_bytes(b"x", 32)
