"""The pieces of the proof kernels, one by one, on the GPU (the `proof` object of
tests/native/device_hooks.hip): the wavefront's Keccak-f[1600] and Merlin of proof/transcript.h at
every position of the 166-byte rate boundary, the arithmetic modulo the group order of
proof/scalar25.h and the element conversions of proof/sumcheck_rows.h at the bounds their headers
state, and the protocol steps of proof/sumcheck_protocol.h and proof/inner_product_protocol.h.
End to end (a proof's bytes against the reference prover) the transcript code sees a handful of
positions and the scalars are random; here every position, every boundary class and every stated
bound is a case.

Expected values come from Python integers, tests/merlin_ref.py and tests/refmath.py, never from
the library.  Every comparison is byte equality.  What needs no GPU (that the chosen cases reach
every boundary class, that the harness rejects what it cannot validate) is not marked `gpu`.
Each test prints its case count per op (run with -s to see them)."""
import ctypes
import functools
import random
import subprocess

import numpy as np
import pytest

from tests import device_hooks as dh
from tests import merlin_ref as mr
from tests import refmath as rm

gpu = pytest.mark.gpu
L = mr.L_ORDER
GK = mr.GK_P
P = rm.P
RATE = mr.RATE
R256 = 1 << 256
TR = 51                 # words of a transcript record: 203 bytes and one of padding
SCALAR_BITS = 253       # kScalarBits of proof/inner_product_protocol.h


@pytest.fixture(scope="module")
def device():
    n = ctypes.c_int(0)      # (the HIP runtime the harness library is linked against)
    assert dh.lib().hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0, "these tests need a GPU"


def count(op, n):
    print(f"[device_proof] {op}: {n} cases")


def words(raw, nbytes=None):
    """bytes -> uint32 words, zero-padded to nbytes (a multiple of 4)"""
    raw = bytes(raw)
    nbytes = len(raw) if nbytes is None else nbytes
    assert len(raw) <= nbytes and nbytes % 4 == 0
    return np.frombuffer(raw + bytes(nbytes - len(raw)), np.uint32)


def le32(x):
    return int(x).to_bytes(32, "little")


def run(op, records, out_words, params=()):
    return dh.run("proof", op, np.stack(records), out_words, params)


def out_bytes(row, first_word, nbytes):
    return row[first_word:].tobytes()[:nbytes]


@functools.lru_cache(None)
def starts():
    return mr.padded_starts()


def test_padded_transcripts_reach_every_position_once():
    got = [int(t[200]) for t in starts()]
    assert got == list(range(RATE))
    assert len({t.tobytes() for t in starts()}) == RATE


#--------------------------------------------------------------------------------------------------
# Keccak-f[1600], one Keccak lane per SIMD lane
#--------------------------------------------------------------------------------------------------
def keccak_states():
    rng = random.Random(1600)
    states = [bytes(200), b"\xff" * 200]
    for lane in range(25):
        states.append(bytes(8 * lane) + b"\xff" * 8 + bytes(8 * (24 - lane)))
        states.append(bytes(8 * lane) + (1 << (lane * 5 % 64)).to_bytes(8, "little") + bytes(8 * (24 - lane)))
    states += [rng.randbytes(200) for _ in range(64)]
    return states


@gpu
def test_keccak_wave(device):
    states = keccak_states()
    rec = [words(s) for s in states]
    once = run("keccak_wave", rec, 50, (1,))
    twice = run("keccak_wave", rec, 50, (2,))        # the write-back to LDS and the reload between two
    for s, h1, h2 in zip(states, once, twice):
        want = mr.keccak_f1600(s)
        assert h1.tobytes() == want
        assert h2.tobytes() == mr.keccak_f1600(want)
    count("keccak_wave (one and two permutations)", 2 * len(states))


#--------------------------------------------------------------------------------------------------
# Merlin on a wavefront, at every position of the sponge
#--------------------------------------------------------------------------------------------------
MESSAGE_BYTES = (0, 1, 31, 32, 165, 166, 167, 288, 332, 512)
LABEL_BYTES = (1, 10, 16)
LABEL = b"rate-boundary-lb"


@functools.lru_cache(None)
def merlin_cases():
    """(position, label bytes, message, challenge bytes, form): every message length at every position;
    the label length and the one 200-byte challenge per position (the only length that crosses the
    boundary while squeezing) move along with position and length so that every pairing occurs; the
    u64 form (integer_bytes as the source of an absorb) once per position"""
    rng = random.Random(166)
    cases = []
    for pos in range(RATE):
        for i, n in enumerate(MESSAGE_BYTES):
            label = LABEL_BYTES[(pos + i) % 3]
            challenge = 200 if (pos + i) % 10 == 0 else 32
            cases.append((pos, label, rng.randbytes(n), challenge, 0))
        cases.append((pos, LABEL_BYTES[pos % 3], rng.randbytes(8), 32, 1))
    return cases


def merlin_model(case, cls=mr.Transcript):
    pos, label, message, challenge, form = case
    t = cls(raw=starts()[pos])
    if form == 0:
        t.append_message(LABEL[:label], message)
    else:
        t.append_u64(LABEL[:label], int.from_bytes(message, "little"))
    return t, t.challenge_bytes(LABEL[:label], challenge)


def test_merlin_cases_reach_every_boundary_class():
    """the thinned cross product, replayed through the instrumented model"""
    reached, begun = set(), set()
    for case in merlin_cases():
        t, _ = merlin_model(case, mr.TracedTranscript)
        reached |= t.classes
        begun |= set(t.starts)
    assert reached == mr.BOUNDARY_CLASSES | {mr.SQUEEZE_CROSS}, sorted(reached)
    assert begun == set(range(RATE)), "an operation begins at every position"
    for n in MESSAGE_BYTES:
        for label in LABEL_BYTES:
            assert any(len(c[2]) == n and c[1] == label for c in merlin_cases())
        assert any(len(c[2]) == n and c[3] == 200 for c in merlin_cases())


@gpu
def test_merlin_wave(device):
    groups = {}
    for case in merlin_cases():
        groups.setdefault((case[1], len(case[2]), case[3], case[4]), []).append(case)
    for (label, n, challenge, form), cases in groups.items():
        rec = [np.concatenate([words(starts()[c[0]].tobytes(), 204), words(LABEL[:label], 16),
                               words(c[2], 512)]) for c in cases]
        got = run("merlin_wave", rec, TR + 64, (label, n, challenge, form))
        for c, h in zip(cases, got):
            t, want = merlin_model(c)
            where = (c[0], label, n, challenge, form)
            assert out_bytes(h, 0, 200) == bytes(t.raw[:200]), ("state", where)
            assert out_bytes(h, 50, 3) == bytes(t.raw[200:]), ("pos, pos_begin, cur_flags", where)
            assert out_bytes(h, TR, challenge) == want, ("challenge", where)
            assert not h[TR:].tobytes()[challenge:].strip(b"\0"), ("bytes past the challenge", where)
    count(f"merlin_wave ({len(groups)} launches)", len(merlin_cases()))


#--------------------------------------------------------------------------------------------------
# scalars modulo l and the element conversions of the two sumcheck fields
#--------------------------------------------------------------------------------------------------
def special_values(m):
    """the bounds of a modulus m and of 256 bits (the largest multiple of m below 2^256: 15 l, 5 p)"""
    return [0, 1, 2, m - 1, m, m + 1, 2 * m - 1, 2**252, 2**253 - 1, 8 * m % R256, (R256 - 1) // m * m,
            2**255 - 19, R256 - 1]


SPECIAL = special_values(L)


def random_values(seed, n=200):
    rng = random.Random(seed)
    return [rng.getrandbits(256) for _ in range(n)]


@gpu
def test_s25_reduce_and_invert(device):
    xs = SPECIAL + random_values(1)
    got = run("s25_reduce", [words(le32(x)) for x in xs], 8)
    for x, h in zip(xs, got):
        assert h.tobytes() == le32(x % L), hex(x)
    count("s25_reduce", len(xs))
    got = run("s25_invert", [words(le32(x)) for x in xs], 8)
    for x, h in zip(xs, got):
        want = pow(x % L, -1, L) if x % L else 0
        assert h.tobytes() == le32(want), hex(x)
    count("s25_invert", len(xs))


@gpu
def test_s25_fold(device):
    rng = random.Random(2)
    vectors = [(0, 0), (L - 1, L - 1), (R256 - 1, R256 - 1), (1, L - 1), (L, 8 * L), (L + 1, 2 * L - 1),
               (rng.getrandbits(256), rng.getrandbits(256))]
    cases = [(ml, mh, u, v) for ml in SPECIAL for mh in SPECIAL for u, v in vectors]
    # sums that vanish modulo l: m_low u + m_high v = 0 with none of the four zero
    for _ in range(20):
        ml, mh, u = (rng.randrange(1, L) for _ in range(3))
        v = (L - ml * u % L) * pow(mh, -1, L) % L
        cases.append((ml + L * rng.randrange(8), mh, u, v + L * rng.randrange(8)))
    cases += [tuple(rng.getrandbits(256) for _ in range(4)) for _ in range(200)]
    got = run("s25_fold", [np.concatenate([words(le32(x)) for x in c]) for c in cases], 8)
    for (ml, mh, u, v), h in zip(cases, got):
        assert h.tobytes() == le32((ml * u + mh * v) % L), [hex(x) for x in (ml, mh, u, v)]
    count("s25_fold", len(cases))


def dot_cases(n, rng):
    """-> list of (a vector, b vector)"""
    top = R256 - 1
    cases = [([top] * n, [top] * n)]                   # the largest lazy sum the contract allows
    for target in (0, L - 1):
        for unreduced in (False, True):
            a = [rng.randrange(1, L) for _ in range(n)]
            b = [rng.randrange(1, L) for _ in range(n)]
            rest = sum(x * y for x, y in zip(a[:-1], b[:-1]))
            b[-1] = (target - rest) * pow(a[-1], -1, L) % L
            if unreduced:
                a = [x + L * rng.randrange(8) for x in a]
                b = [x + L * rng.randrange(8) for x in b]
            assert sum(x * y for x, y in zip(a, b)) % L == target
            cases.append((a, b))
    cases += [([L] * n, [rng.getrandbits(256) for _ in range(n)])]       # every product a multiple of l
    cases += [([rng.getrandbits(256) for _ in range(n)], [rng.getrandbits(256) for _ in range(n)])
              for _ in range(8)]
    return cases


@gpu
def test_s25_dot(device):
    rng = random.Random(3)
    total = 0
    for n in (1, 2, 63, 64):
        cases = dot_cases(n, rng)
        rec = [np.concatenate([words(le32(x) + le32(y)) for x, y in zip(a, b)]) for a, b in cases]
        got = run("s25_dot", rec, 8, (n,))
        for (a, b), h in zip(cases, got):
            assert h.tobytes() == le32(sum(x * y for x, y in zip(a, b)) % L), n
        total += len(cases)
    count("s25_dot (n = 1, 2, 63, 64)", total)


# per field: tag of the ops, modulus, value -> the caller's 32 bytes
def caller_bytes(field_id, value):
    return le32(value % L) if field_id == 0 else le32(value * R256 % GK)


@gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_element_conversions(device, field_id):
    tag, m = ("sc", L) if field_id == 0 else ("gk", GK)
    xs = special_values(m) + random_values(4 + field_id)
    rec = [words(le32(x)) for x in xs]
    # store(load(bytes)): the canonical bytes of the same element
    got = run(f"{tag}_roundtrip", rec, 8)
    for x, h in zip(xs, got):
        assert h.tobytes() == le32(x % m), hex(x)
    count(f"{tag}_roundtrip", len(xs))
    # 1 - r in the caller's representation (Grumpkin: Montgomery form, the element behind x is x / 2^256)
    got = run(f"{tag}_one_minus", rec, 8)
    for x, h in zip(xs, got):
        want = (1 - x) % L if field_id == 0 else (R256 - x) % GK
        assert h.tobytes() == le32(want), hex(x)
    count(f"{tag}_one_minus", len(xs))
    # challenge::make: r's bytes by the reference's rule, and the engine form it returns is that element
    got = run(f"{tag}_challenge_make", rec, 16)
    for x, h in zip(xs, got):
        want = mr.challenge_from_bytes(field_id, le32(x))
        assert out_bytes(h, 0, 32) == want, hex(x)
        assert out_bytes(h, 8, 32) == want, ("the returned engine form", hex(x))
    count(f"{tag}_challenge_make", len(xs))
    # convert(words, element): the element behind 32 bytes of the caller's, as load() ...
    got = run(f"{tag}_convert", [np.concatenate([r, [1]]) for r in rec], 8)
    for x, h in zip(xs, got):
        assert h.tobytes() == le32(x % m), hex(x)
    # ... or an integer below 2^248 (the documented bound) as an element
    rng = random.Random(6)
    small = [0, 1, 2, 2**248 - 1, 2**247, 2**128] + [rng.getrandbits(248) for _ in range(100)]
    got = run(f"{tag}_convert", [np.concatenate([words(le32(x)), [0]]) for x in small], 8)
    for x, h in zip(small, got):
        assert h.tobytes() == caller_bytes(field_id, x), hex(x)
    count(f"{tag}_convert (element, integer)", len(xs) + len(small))


#--------------------------------------------------------------------------------------------------
# the protocol steps on a wavefront, at every position
#--------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def sumcheck_round_cases():
    """(position, field, length, polynomial): the shortest and the longest polynomial at every position,
    the lengths between at every sixth; the field moves along"""
    rng = random.Random(7)
    cases = []
    for pos in range(RATE):
        for field_id, length in ((pos % 2, 2), (1 - pos % 2, 9), (pos // 6 % 2, 3 + pos % 6)):
            cases.append((pos, field_id, length, rng.randbytes(32 * length)))
    return cases


def sumcheck_round_model(case, cls=mr.Transcript):
    pos, field_id, length, polynomial = case
    t = cls(raw=starts()[pos])
    t.append_message(b"P", polynomial)
    x = t.challenge_bytes(b"R", 32)
    return t, x, mr.challenge_from_bytes(field_id, x)


@functools.lru_cache(None)
def ip_round_cases():
    """(position, init, n, L, R)"""
    rng = random.Random(8)
    ns = [1, 2, 2**30, 2**32, 2**64 - 1]
    return [(pos, init, ns[(pos + init) % 5] if pos % 3 else rng.getrandbits(64), rng.randbytes(32),
             rng.randbytes(32)) for pos in range(RATE) for init in (0, 1)]


def ip_round_model(case, cls=mr.Transcript):
    pos, init, n, l_value, r_value = case
    t = cls(raw=starts()[pos])
    if init:
        mr.inner_product_begin(t, n)
    return t, mr.inner_product_round(t, l_value, r_value)


def test_protocol_step_cases_reach_every_boundary_class():
    """(a sumcheck round alone has one-byte labels: the sponge cannot fill inside one)"""
    for cases, model, want in ((sumcheck_round_cases(), sumcheck_round_model, mr.BOUNDARY_CLASSES - {"label-inside"}),
                               (ip_round_cases(), ip_round_model, mr.BOUNDARY_CLASSES)):
        reached = set()
        for case in cases:
            reached |= model(case, mr.TracedTranscript)[0].classes
        assert reached == want, sorted(want - reached)
    seen = {(f, n) for _, f, n, _ in sumcheck_round_cases()}
    assert seen == {(f, n) for f in (0, 1) for n in range(2, 10)}


@gpu
def test_sumcheck_round_wave(device):
    groups = {}
    for case in sumcheck_round_cases():
        groups.setdefault(case[1:3], []).append(case)
    for (field_id, length), cases in groups.items():
        rec = [np.concatenate([words(starts()[c[0]].tobytes(), 204), words(c[3], 288)]) for c in cases]
        got = run("sumcheck_round_wave", rec, TR + 24, (field_id, length))
        for c, h in zip(cases, got):
            t, x, r = sumcheck_round_model(c)
            where = (c[0], field_id, length)
            assert out_bytes(h, 0, 203) == bytes(t.raw), ("transcript", where)
            assert out_bytes(h, TR, 32) == x, ("x", where)
            assert out_bytes(h, TR + 8, 32) == r, ("r", where)
            assert out_bytes(h, TR + 16, 32) == r, ("the returned engine form", where)
    count("sumcheck_round_wave", len(sumcheck_round_cases()))


@gpu
def test_ip_round_wave(device):
    for init in (0, 1):
        cases = [c for c in ip_round_cases() if c[1] == init]
        rec = [np.concatenate([words(starts()[c[0]].tobytes(), 204), words(c[3] + c[4]),
                               words(c[2].to_bytes(8, "little"))]) for c in cases]
        got = run("ip_round_wave", rec, TR + 16, (init,))
        for c, h in zip(cases, got):
            t, x = ip_round_model(c)
            assert out_bytes(h, 0, 203) == bytes(t.raw), ("transcript", c[0], init)
            assert out_bytes(h, TR, 32) == x, ("x", c[0], init)
            assert out_bytes(h, TR + 8, 32) == le32(int.from_bytes(x, "little") % L), ("x mod l", c[0], init)
    count("ip_round_wave", len(ip_round_cases()))


#--------------------------------------------------------------------------------------------------
# a lane of k_fold_generators
#--------------------------------------------------------------------------------------------------
def fold_digits(m_low, m_high):
    """decompose_fold: digit = bit(m_low) + 2 bit(m_high) over 253 bits, zero digits at the top dropped"""
    d = [((m_low >> bit) & 1) + 2 * ((m_high >> bit) & 1) for bit in range(SCALAR_BITS)]
    n = SCALAR_BITS
    while n > 0 and d[n - 1] == 0:
        n -= 1
    return d, n


def fold_multipliers():
    rng = random.Random(9)
    x = rng.randrange(1, L)
    pairs = [(0, 0), (1, 0), (0, 1), (1, 1), (2**252, 1), (L - 1, L - 1), (2**252 + 5, 3), (3, 2**252 + 5),
             (2**251, 2**251), (2, 1), (pow(x, -1, L), x)]
    assert fold_digits(0, 0)[1] == 0
    assert fold_digits(2**252, 1) == ([2] + [0] * 251 + [1], 253)
    assert fold_digits(L - 1, L - 1)[0][-1] == 3 and fold_digits(2**252 + 5, 3)[1] == 253
    assert fold_digits(2**251, 2**251)[1] == 252 and fold_digits(2, 1)[0][:2] == [2, 1]
    return pairs


@gpu
def test_ip_fold_point(device):
    """m_low g_lo + m_high g_hi against double-and-add on Python integers"""
    for a, b in ((rm.ED_BASE, rm.ed_multiples(1, 7)[0]), (rm.ED_IDENTITY, rm.ED_BASE)):   # (the inversion-free addition)
        assert rm.ed_same(rm.ed_ext_add(rm.ed_extended(a, 3), rm.ed_extended(b, 5)), rm.ed_add(a, b))
    g = rm.ed_multiples(4, 1234567, 89)
    zs = [1, 2, P - 1, 2**254 + 99]
    generators = [(g[0], g[1]), (g[2], g[2]), (g[3], rm.ed_neg(g[3])), (rm.ED_IDENTITY, g[1]),
                  (g[1], rm.ED_IDENTITY)]
    cases = [(ml, mh, lo, hi) for ml, mh in fold_multipliers() for lo, hi in generators]
    rec = []
    for i, (ml, mh, lo, hi) in enumerate(cases):
        d, n = fold_digits(ml, mh)
        p51 = [np.array(rm.ed_point51(rm.ed_extended(q, zs[(i + k) % 4])), np.uint64).view(np.uint32)
               for k, q in enumerate((lo, hi))]
        rec.append(np.concatenate([words(bytes(d), 256), [n], *p51]))
    got = run("ip_fold_point", rec, 40)
    for (ml, mh, lo, hi), h in zip(cases, got):
        want = rm.ed_affine(rm.ed_ext_add(rm.ed_ext_mul(ml, lo), rm.ed_ext_mul(mh, hi)))
        ext = rm.ed_from51([int(v) for v in np.ascontiguousarray(h).view(np.uint64)])
        assert rm.ed_same(ext, want), (hex(ml), hex(mh), lo == hi, lo == rm.ED_IDENTITY)
    count("ip_fold_point", len(cases))


#--------------------------------------------------------------------------------------------------
# what the harness cannot validate it rejects, before anything is launched
#--------------------------------------------------------------------------------------------------
def test_harness_rejects_before_it_launches():
    """every rejection is decided on the host: no GPU is needed to see it (the harness library is:
    __graft_entry__.build() compiles it, and tests/device_hooks.py does where hipcc is installed)"""
    try:
        dh.lib()
    except (OSError, subprocess.CalledProcessError) as e:
        pytest.fail(f"the device-hook harness is neither built nor buildable here (it needs hipcc): {e}")
    dh.assert_proof_rejections()
