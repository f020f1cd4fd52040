"""The device arithmetic, primitive by primitive, on the GPU (tests/native/device_hooks.hip), at
the contract bounds that random MSM inputs never reach.  Everything is exact; every generated case
is compared.  Three kinds of assertion:

  (a) device == host, limb for limb, for the headers both sides compile (f29, ed29, mont29, sw29):
      the device twin of every hook of tests/hooks.py, under each flag set the product builds them
      with -- a difference is a device-only branch or the compiler;
  (b) kernel == model, lane for lane, for ed16w and sww::wave<G>: the 64 output lane words of fmul /
      dbl / add / add_cached equal what tools/models computes from the same 64 input lane words,
      which makes the models' interval proofs statements about the kernel; output limbs also stay
      below the bounds the headers document;
  (c) kernel == mathematics: values mod p, points projectively, encodings byte for byte, against
      tests/refmath.py (pinned to the host hooks and the oracle by tests/test_refmath.py).

Each test prints its case count per op (run with -s to see them)."""
import functools
import random

import numpy as np
import pytest

from tests import device_cases as dc
from tests import device_hooks as dh
from tests import hooks
from tests import refmath as rm
from tests.test_host_arith import f29_loose

pytestmark = pytest.mark.gpu
P = rm.P
CURVES = ["bn254", "grumpkin", "bls12_381"]


@pytest.fixture(scope="module", autouse=True)
def device():
    import ctypes
    n = ctypes.c_int(0)      # (the HIP runtime the harness library is linked against)
    assert dh.lib().hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0, "these tests need a GPU"


def count(op, n):
    print(f"[device_arith] {op}: {n} cases")


def u32(rows):
    return np.array(rows, dtype=np.uint32)


def ints(a):
    return [int(v) for v in a]


def u64s(words):
    """(cases, 2k) uint32 -> (cases, k) uint64"""
    return np.ascontiguousarray(words).view(np.uint64)


def w32(a64):
    return np.ascontiguousarray(a64, dtype=np.uint64).view(np.uint32)


#--------------------------------------------------------------------------------------------------
# (a) f29 / ed29: device == host hooks
#--------------------------------------------------------------------------------------------------
def f29_inputs():
    rng = np.random.default_rng(291)
    out = []
    for bound in (1.001, 2.001, 3.001, 5.0, 7.0):
        out += [(bound, f29_loose(rng, bound)) for _ in range(24)]
    for x in (0, 1, P - 1, P, P + 1, 2 * P, 2**255 - 20, 2**256 - 38):
        out.append((1.001, np.array(rm.fe29(x), np.uint32)))
    # the same residues in non-canonical limbs: a unit borrowed from the limb above
    for x in (P, P + 1, P - 1):
        l = rm.fe29(x)
        l[3] -= 1
        l[2] += 1 << 29
        out.append((2.001, np.array(l, np.uint32)))
    for k in (0, 1, 28, 29, 31, 32, 57, 58, 63, 64, 127, 128, 231, 232, 254, 255, 256, 260):
        out.append((1.001, np.array(rm.limbs(1 << k, 29, 9), np.uint32)))
    return out


@pytest.mark.parametrize("tag", ["ed", "ed_niels"])
def test_f29_device_equals_host(tag):
    cases = f29_inputs()
    le1 = [f for b, f in cases if b <= 1.01]
    le2 = [f for b, f in cases if b <= 2.01]
    le3 = [f for b, f in cases if b <= 3.01]
    pairs = [(f, g) for f in le3[::5] for g in le2[::7]] + [(f, g) for f in le2[::7] for g in le3[::6]]
    got = dh.run(tag, "f29_mul", u32([np.concatenate(p) for p in pairs]), 9)
    for (f, g), h in zip(pairs, got):
        assert np.array_equal(h, hooks.f29("mul", f, g))
        assert rm.value(ints(h), 29) % P == rm.value(ints(f), 29) * rm.value(ints(g), 29) % P
    count(f"{tag}/f29_mul", len(pairs))
    got = dh.run(tag, "f29_sq", u32(le2), 9)
    for f, h in zip(le2, got):
        assert np.array_equal(h, hooks.f29("sq", f))
    count(f"{tag}/f29_sq", len(le2))
    subs = [(f, g) for b, f in cases[::2] if b <= 5 for g in le1[::6]]   # sub: B(g) < 1.99, f up to B 5
    got = dh.run(tag, "f29_sub", u32([np.concatenate(p) for p in subs]), 9)
    for (f, g), h in zip(subs, got):
        assert np.array_equal(h, hooks.f29("sub", f, g))
        assert rm.value(ints(h), 29) % P == (rm.value(ints(f), 29) - rm.value(ints(g), 29)) % P
    count(f"{tag}/f29_sub", len(subs))
    every = [f for _, f in cases]
    got = dh.run(tag, "f29_weak_reduce", u32(every), 9)
    for f, h in zip(every, got):
        assert np.array_equal(h, hooks.f29("weak_reduce", f))
    count(f"{tag}/f29_weak_reduce", len(every))
    words = dh.run(tag, "f29_to_words", u32(every), 8)
    packed = dh.run(tag, "f29_pack_words", u32(every), 8)
    for f, w, pk in zip(every, words, packed):
        want = rm.value(ints(f), 29) % P
        assert hooks.f29_to_int(f) == want
        assert int.from_bytes(w.tobytes(), "little") == want and np.array_equal(w, pk)
    back = dh.run(tag, "f29_unpack_words", packed, 9)
    for f, h in zip(every, back):
        assert ints(h) == rm.limbs(rm.value(ints(f), 29) % P, 29, 9)
    count(f"{tag}/f29_to_words, pack_words, unpack_words", len(every))
    inv = dh.run(tag, "f29_invert", u32(le2), 9)
    pw = dh.run(tag, "f29_pow22523", u32(le2), 9)
    for f, h, q in zip(le2, inv, pw):
        assert np.array_equal(h, hooks.f29("invert", f))
        x = rm.value(ints(f), 29) % P
        assert rm.value(ints(h), 29) % P == pow(x, P - 2, P)
        assert rm.value(ints(q), 29) % P == pow(x, (P - 5) // 8, P)
    count(f"{tag}/f29_invert, f29_pow22523", len(le2))
    rng = np.random.default_rng(51)
    mask = (1 << 51) - 1
    f51s = [np.zeros(5, np.uint64), np.full(5, mask, np.uint64),
            np.array([mask - 18, mask, mask, mask, mask], np.uint64),
            np.array([mask - 19, mask, mask, mask, mask], np.uint64), np.full(5, (1 << 54) - 1, np.uint64)]
    f51s += [rng.integers(0, 1 << 51, 5, dtype=np.uint64) + (rng.integers(0, 1 << 51, 5, dtype=np.uint64)
                                                              if i % 2 else 0) for i in range(60)]
    got = dh.run(tag, "f29_from_fe51", u32([w32(f) for f in f51s]), 9)
    for f, h in zip(f51s, got):
        assert np.array_equal(h, hooks.f29_from_fe51(f))
    count(f"{tag}/f29_from_fe51", len(f51s))


def ed_points51():
    """element_p3 inputs: identity, torsion, multiples of the base point, Z != 1"""
    pts = [rm.ED_IDENTITY] + rm.ed_torsion()[1:] + rm.ed_multiples(10, 5, 3)
    zs = [1, 2, P - 1, 2**254 + 99, 12345678901234567890]
    return pts, [np.array(rm.ed_point51(rm.ed_extended(q, zs[i % 5])), np.uint64) for i, q in enumerate(pts)]


def test_ed29_device_equals_host():
    pts, p51 = ed_points51()
    pairs = [(i, j, neg) for i in range(len(pts)) for j in range(i % 3, len(pts), 3) for neg in (0, 1)]
    pairs += [(i, i, neg) for i in range(len(pts)) for neg in (0, 1)]       # doubling, cancellation
    rec = u32([np.concatenate([w32(p51[i]), w32(p51[j]), [neg]]) for i, j, neg in pairs])
    got = u64s(dh.run("ed", "ed29_add", rec, 40))
    gath = u64s(dh.run("ed", "ed29_add_gathered", rec, 40))
    for (i, j, neg), h, g in zip(pairs, got, gath):
        assert np.array_equal(h, hooks.ed29_add(p51[i], p51[j], bool(neg)))
        assert np.array_equal(g, hooks.ed29_add_gathered(p51[i], p51[j], bool(neg)))
        want = rm.ed_add(pts[i], rm.ed_neg(pts[j]) if neg else pts[j])
        assert rm.ed_same(rm.ed_from51(ints(h)), want) and rm.ed_same(rm.ed_from51(ints(g)), want)
    count("ed/ed29_add, ed29_add_gathered", len(pairs))
    gen = u64s(dh.run("ed", "ed29_add_general", rec[:, :80], 40))
    for (i, j, _), h in zip(pairs, gen):
        assert rm.ed_same(rm.ed_from51(ints(h)), rm.ed_add(pts[i], pts[j]))
    count("ed/ed29_add_general", len(pairs))
    dbl = [(i, k) for i in range(len(pts)) for k in (1, 2, 16, 17)]
    got = u64s(dh.run("ed", "ed29_dbl_n", u32([np.concatenate([w32(p51[i]), [k]]) for i, k in dbl]), 40))
    for (i, k), h in zip(dbl, got):
        assert np.array_equal(h, hooks.ed29_dbl_n(p51[i], k))
        assert rm.ed_same(rm.ed_from51(ints(h)), rm.ed_mul(1 << k, pts[i]))
    count("ed/ed29_dbl_n", len(dbl))
    enc = dh.run("ed", "ed29_ristretto_encode", u32([w32(p) for p in p51]), 8)
    for q, p, e in zip(pts, p51, enc):
        assert e.tobytes() == bytes(hooks.ristretto_encode(p)) == rm.ristretto_encode(rm.ed_from51(ints(p)))
    count("ed/ed29_ristretto_encode", len(p51))


@pytest.mark.parametrize("tag", ["ed", "ed_niels"])
def test_ed29_chains_device_equal_host(tag):
    """a lane of k_accumulate: 40 signed additions with repeated points (doubling and cancellation inside
    the chain), through the projective addends, the Z = 1 addends and the loaded-first-entry forms"""
    pts, p51 = ed_points51()
    rng = random.Random(7)
    forms = (1, 3) if tag == "ed_niels" else (0, 1, 2, 3)
    total = 0
    for n in (1, 2, 40):
        chains = []
        for _ in range(6):
            idx = [rng.randrange(9, len(pts)) for _ in range(n)]     # (the Z = 1 forms normalise: no Z = 0)
            sg = [rng.randrange(2) for _ in range(n)]
            if n == 40:
                idx[1], sg[1] = idx[0], sg[0]                          # the second addition is a doubling
                idx[-1], sg[-1] = idx[5], 1 - sg[5]
            chains.append((idx, sg))
        rec = u32([np.concatenate([np.concatenate([w32(p51[i]), [s]]) for i, s in zip(idx, sg)])
                   for idx, sg in chains])
        for form in forms:
            got = u64s(dh.run(tag, "ed29_chain", rec, 40, (n, form)))
            for (idx, sg), h in zip(chains, got):
                q = np.stack([p51[i] for i in idx])
                want = (hooks.ed29_chain(q, sg, niels=form == 1) if form < 2
                        else hooks.ed29_chain_first(q, sg, niels=form == 3))
                assert np.array_equal(h, want), (n, form)
                acc = rm.ED_IDENTITY
                for i, s in zip(idx, sg):
                    acc = rm.ed_add(acc, rm.ed_neg(pts[i]) if s else pts[i])
                assert rm.ed_same(rm.ed_from51(ints(h)), acc)
            total += len(chains)
    count(f"{tag}/ed29_chain (forms {forms})", total)


#--------------------------------------------------------------------------------------------------
# (a) mont29 / sw29: device == host hooks, and the raw-limb ops against integers
#--------------------------------------------------------------------------------------------------
def mont_elements(c):
    rng = random.Random(c.N64)
    vals = [0, 1, c.p - 1, c.R64 % c.p, c.R29 % c.p, c.Rw % c.p, 2, 3, 5, (1 << 64) - 1]
    vals += [1 << k for k in (1, 28, 29, 31, 32, 63, 64, 65, 127, 128, 200, 64 * c.N64 - 4) if (1 << k) < c.p]
    vals += [rng.randrange(c.p) for _ in range(20)]
    return vals


@pytest.mark.parametrize("name", CURVES)
@pytest.mark.parametrize("acc", ["", "_acc"])
def test_mont29_device_equals_host(name, acc):
    c, tag = rm.CURVES[name], name + acc
    vals = mont_elements(c)
    e64 = [np.array(rm.limbs(v, 64, c.N64), np.uint64) for v in vals]
    k = 2 * c.N64
    rinv = rm.inv(c.R64, c.p)
    pairs = [(i, j) for i in range(len(vals)) for j in range(i % 7, len(vals), 7)]
    got = dh.run(tag, "m29_mul", u32([np.concatenate([w32(e64[i]), w32(e64[j])]) for i, j in pairs]), k + 1)
    for (i, j), h in zip(pairs, got):
        assert np.array_equal(u64s(h[:k]), hooks.sw29_field(c.cid, "mul", e64[i], e64[j]))
        assert rm.value(ints(h[:k]), 32) == vals[i] * vals[j] * rinv % c.p
        assert h[k] == 1, "mul_pinned differs from mul"
    count(f"{tag}/m29_mul", len(pairs))
    got = dh.run(tag, "m29_roundtrip", u32([w32(e) for e in e64]), k)
    inv = dh.run(tag, "m29_invert", u32([w32(e) for e in e64[1:]]), k)     # (0 has no inverse)
    for e, h in zip(e64, got):
        assert np.array_equal(u64s(h), e)
    for e, v, h in zip(e64[1:], vals[1:], inv):
        assert np.array_equal(u64s(h), hooks.sw29_field(c.cid, "invert", e))
        assert rm.value(ints(h), 32) * v % c.p == c.R64 * c.R64 % c.p
    count(f"{tag}/m29_roundtrip, m29_invert", len(e64))
    rng = random.Random(2)
    quads = [[rng.randrange(len(vals)) for _ in range(4)] for _ in range(60)]
    got = dh.run(tag, "m29_mul2", u32([np.concatenate([w32(e64[i]) for i in q]) for q in quads]), k + 1)
    for q, h in zip(quads, got):
        assert np.array_equal(u64s(h[:k]), hooks.sw29_field(c.cid, "mul2", *[e64[i] for i in q]))
        a, b, cc, d = (vals[i] for i in q)
        assert rm.value(ints(h[:k]), 32) == (2 * a * b + 3 * cc * d) * rinv % c.p and h[k] == 1
    count(f"{tag}/m29_mul2", len(quads))


def loose_mont(c, rng, b, v):
    """N limbs: the low N - 1 below b 2^LB (saturated now and then), the value below v p"""
    hi = int(b * (1 << c.LB))
    l = [rng.choice([hi - 1, rng.randrange(hi)]) for _ in range(c.N - 1)]
    top_max = (v * c.p >> (c.LB * (c.N - 1))) - int(b) - 2
    l.append(rng.choice([top_max, rng.randrange(top_max + 1)]))
    assert rm.value(l, c.LB) < v * c.p
    return l


@pytest.mark.parametrize("name", CURVES)
@pytest.mark.parametrize("acc", ["", "_acc"])
def test_mont29_raw_limb_ops_match_integers(name, acc):
    """field/mont29.h at its contracts: mul N (B_a B_b + 1) <= 64, sub<K> with every limb of b up to
    2^(LB+1) - 2 and V_b < K - 0.01, mul_b3 with B <= 4 and V < 8"""
    c, tag = rm.CURVES[name], name + acc
    rng = random.Random(c.N)
    N, LB = c.N, c.LB
    r29i = rm.inv(c.R29, c.p)
    ba, bb = (2.0, 3.0) if N == 9 else (1.7, 2.0)
    pairs = [(loose_mont(c, rng, ba, 12), loose_mont(c, rng, bb, 12)) for _ in range(100)]
    pairs += [(rm.limbs(x, LB, N), rm.limbs(y, LB, N)) for x in (0, 1, c.p - 1, c.p, c.p + 1, c.R29 % c.p)
              for y in (0, c.p - 1, c.p, c.R29 % c.p, 5 * c.p + 1)]
    got = dh.run(tag, "m29_raw_mul", u32([a + b for a, b in pairs]), 2 * N)
    for (a, b), h in zip(pairs, got):
        h = ints(h)
        assert h[:N] == h[N:], "mul_pinned differs from mul"
        assert rm.value(h[:N], LB) % c.p == rm.value(a, LB) * rm.value(b, LB) * r29i % c.p
        assert max(h[:N - 1]) < 1 << LB
        assert rm.value(h[:N], LB) < (rm.value(a, LB) * rm.value(b, LB) // c.R29) + c.p + 1
    count(f"{tag}/m29_raw_mul", len(pairs))
    loose = [loose_mont(c, rng, 6.0, 20) for _ in range(60)] + [[(1 << 31) - 1] * (N - 1) + [5] for _ in range(1)]
    got = dh.run(tag, "m29_raw_norm", u32(loose), N)
    for a, h in zip(loose, got):
        assert rm.value(ints(h), LB) == rm.value(a, LB) and max(ints(h)[:N - 1]) < 1 << LB
    count(f"{tag}/m29_raw_norm", len(loose))
    subs = []
    for _ in range(80):
        b = [rng.choice([(2 << LB) - 2, rng.randrange((2 << LB) - 1)]) for _ in range(N - 1)]
        b.append(rng.randrange((19 * c.p // 10 >> (LB * (N - 1))) - 2))
        assert rm.value(b, LB) < 199 * c.p // 100
        subs.append((loose_mont(c, rng, 4.0, 20), b))
    subs += [(rm.limbs(x, LB, N), rm.limbs(y, LB, N)) for x in (0, c.p - 1) for y in (0, 1, c.p - 1, c.p)]
    got = dh.run(tag, "m29_raw_sub", u32([a + b for a, b in subs]), 6 * N)
    for (a, b), h in zip(subs, got):
        h = ints(h)
        for i, K in enumerate((2, 4, 8)):
            assert rm.value(h[i * N:(i + 1) * N], LB) == rm.value(a, LB) + K * c.p - rm.value(b, LB), K
            assert rm.value(h[(3 + i) * N:(4 + i) * N], LB) == K * c.p - rm.value(b, LB), K
    count(f"{tag}/m29_raw_sub (sub<2,4,8>, neg<2,4,8>)", len(subs))
    b3 = 3 * abs(c.b if c.b < c.p // 2 else c.b - c.p)
    xs = [loose_mont(c, rng, 4.0, 8) for _ in range(60)] + [rm.limbs(x, LB, N) for x in (0, 1, c.p - 1, c.p, 7 * c.p)]
    got = dh.run(tag, "m29_raw_mul_b3", u32(xs), N)
    for a, h in zip(xs, got):
        h = ints(h)
        assert rm.value(h, LB) % c.p == b3 * rm.value(a, LB) % c.p
        assert max(h[:N - 1]) < 1 << LB and rm.value(h, LB) < 4 * c.p
    count(f"{tag}/m29_raw_mul_b3", len(xs))


def sw_points64(c):
    pts = [None] + c.multiples(8, 2, 5)
    zs = [1, 2, c.p - 1, 2**200 + 77]
    return pts, [np.array(rm.sw_point64(c, c.projective(q, zs[i % 4])), np.uint64) for i, q in enumerate(pts)]


@pytest.mark.parametrize("name", CURVES)
@pytest.mark.parametrize("acc", ["", "_acc"])
def test_sw29_device_equals_host(name, acc):
    c, tag = rm.CURVES[name], name + acc
    pts, p64 = sw_points64(c)
    k = 6 * c.N64
    pairs = [(i, j) for i in range(len(pts)) for j in range(len(pts))]
    got = dh.run(tag, "sw29_add", u32([np.concatenate([w32(p64[i]), w32(p64[j])]) for i, j in pairs]), k)
    for (i, j), h in zip(pairs, got):
        assert np.array_equal(u64s(h), hooks.sw29_add(c.cid, p64[i], p64[j]))
        assert c.same(rm.sw_from64(c, ints(u64s(h))), c.add(pts[i], pts[j]))
    count(f"{tag}/sw29_add", len(pairs))
    dbl = [(i, n) for i in range(len(pts)) for n in (1, 2, 16, 17)]
    got = dh.run(tag, "sw29_dbl_n", u32([np.concatenate([w32(p64[i]), [n]]) for i, n in dbl]), k)
    for (i, n), h in zip(dbl, got):
        assert np.array_equal(u64s(h), hooks.sw29_dbl_n(c.cid, p64[i], n))
        assert c.same(rm.sw_from64(c, ints(u64s(h))), c.mul(1 << n, pts[i]))
    count(f"{tag}/sw29_dbl_n", len(dbl))
    # chains of mixed additions (k_accumulate's lane), repeated points: doubling and cancellation
    rng = random.Random(3)
    aff = [np.array(rm.limbs(q[0] * c.R64 % c.p, 64, c.N64) + rm.limbs(q[1] * c.R64 % c.p, 64, c.N64), np.uint64)
           for q in pts[1:]]
    total = 0
    for n in (1, 2, 40):
        chains = []
        for t in range(6):
            idx = [rng.randrange(len(aff)) for _ in range(n)]
            sg = [rng.randrange(2) for _ in range(n)]
            if n == 40:
                idx[1], sg[1] = idx[0], sg[0]
                idx[-1], sg[-1] = idx[5], 1 - sg[5]
            chains.append((t % len(p64), idx, sg))
        for lifted in (0, 1):
            rec = u32([np.concatenate([w32(p64[0 if lifted else s])] +
                                      [np.concatenate([w32(aff[i]), [g]]) for i, g in zip(idx, sg)])
                       for s, idx, sg in chains])
            got = dh.run(tag, "sw29_chain", rec, k + 1, (n, lifted))
            for (s, idx, sg), h in zip(chains, got):
                xy = np.stack([aff[i] for i in idx])
                want = (hooks.sw29_chain_lifted(c.cid, xy, sg) if lifted
                        else hooks.sw29_chain(c.cid, p64[s], xy, sg))
                assert np.array_equal(u64s(h[:k]), want), (n, lifted)
                assert h[k] == 1, "add_mixed / add_mixed_acc forms disagree on the device"
                pt = None if lifted else pts[s]
                for i, g in zip(idx, sg):
                    pt = c.add(pt, c.neg(pts[1 + i]) if g else pts[1 + i])
                assert c.same(rm.sw_from64(c, ints(u64s(h[:k]))), pt)
            total += len(chains)
    count(f"{tag}/sw29_chain (add_mixed, add_mixed_acc, lifted)", total)


#--------------------------------------------------------------------------------------------------
# (b) + (c) ed16w
#--------------------------------------------------------------------------------------------------
def test_ed16w_fmul_kernel_equals_model():
    t = dc.ed16w_tables()
    names = list(t["fmul"])
    got = dh.run("ed", "ed16w_fmul", u32([t["fmul"][n][0] + t["fmul"][n][1] for n in names]), 64)
    for n, h in zip(names, got):
        u, v = t["fmul"][n]
        assert ints(h) == t["fmul_model"][n], n
        assert int(h.max()) < 2**16 + 64
        for r, (a, b, x) in enumerate(zip(rm.rows16_values(u), rm.rows16_values(v), rm.rows16_values(ints(h)))):
            assert x % P == a * b % P, (n, r)
    count("ed/ed16w_fmul", 4 * len(names))


def test_ed16w_dbl_add_cached_kernel_equals_model():
    t = dc.ed16w_tables()
    for kind, op in (("dbl", "ed16w_dbl"), ("add", "ed16w_add_cached")):
        names = [n for n in t["point"] if t["point"][n][0] == kind]
        rec = u32([t["point"][n][1] + (t["point"][n][2] or []) for n in names])
        got = dh.run("ed", op, rec, 100)
        for n, h in zip(names, got):
            want = t["point"][n][3]
            assert ints(h[:64]) == t["point_model"][n], n
            assert int(h[:64].max()) < 2**16 + 64
            assert dc.ed_point_matches(rm.rows16_values(ints(h[:64])), want), n
            assert dc.ed_point_matches(rm.ed_from29(ints(h[64:])), want), n      # store_point
        count(f"ed/{op}", len(names))
    # P + P through add_cached and dbl(P) are the same point
    for n in t["point"]:
        if n.endswith("_self"):
            assert dc.proj_equal(rm.rows16_values(t["point_model"][n]),
                                 rm.rows16_values(t["point_model"]["dbl_" + n[4:-5]]))


def test_ed16w_chains_fed_back_raw():
    mult = rm.ed_multiples(3, 9, 4)
    starts = [(rm.ED_IDENTITY, 1), (mult[0], 2**254 + 5), (rm.ed_torsion()[3], P - 2)]
    rec = u32([rm.rows16(list(rm.ed_extended(pt, z))) + rm.ed_cached_rows(rm.ed_extended(mult[2], 77 + z))
               for pt, z in starts])
    short = dh.run("ed", "ed16w_chain", rec, 100, (30,))
    for r, h in zip(rec, short):
        assert ints(h[:64]) == dc.ed_chain_model(ints(r[:64]), ints(r[64:]), 30)
    long = dh.run("ed", "ed16w_chain", rec, 100, (300,))
    for (pt, _), h in zip(starts, long):
        want = dc.ed_chain_point(pt, mult[2], 300)
        assert int(h[:64].max()) < 2**16 + 64
        assert rm.ed_same(rm.rows16_values(ints(h[:64])), want) and rm.ed_same(rm.ed_from29(ints(h[64:])), want)
    count("ed/ed16w_chain (30 steps against the model, 300 against the group law)", 2 * len(starts))


def test_ed16w_gather_row_and_load_point():
    ws = dc.gather_rows()
    got = dh.run("ed", "ed16w_gather", u32(ws), 36)
    for w, h in zip(ws, got):
        for r in range(4):
            assert ints(h[9 * r:9 * r + 9]) == dc.gather_expected(w[16 * r:16 * r + 16]), (w, r)
            assert rm.value(ints(h[9 * r:9 * r + 9]), 29) % P == rm.value(w[16 * r:16 * r + 16], 16) % P
    count("ed/ed16w_gather (store_point of raw limbs)", 4 * len(ws))
    rng = np.random.default_rng(5)
    pts = []
    for i in range(40):
        bound = [1.0, 2.0, 3.0, 7.0, 7.999][i % 5]
        pts.append(np.concatenate([f29_loose(rng, bound) for _ in range(4)]))
    pts.append(np.full(36, 0xffffffff, np.uint32))
    pts.append(np.array(rm.ed_point29((P, P + 1, 2**256 - 1, 0)), np.uint32))
    got = dh.run("ed", "ed16w_roundtrip", u32(pts), 100)
    for p, h in zip(pts, got):
        vals = [rm.value(ints(p[9 * r:9 * r + 9]), 29) % P for r in range(4)]
        assert ints(h[:64]) == rm.rows16(vals)
        assert ints(h[64:]) == rm.ed_point29(vals)
    count("ed/ed16w_roundtrip (load_point -> store_point)", len(pts))


def nonsquare():
    z = 2
    while pow(z, (P - 1) // 2, P) == 1:
        z += 1
    return z


def test_ed16w_pow22523_invert_encode():
    rng = np.random.default_rng(6)
    zs = [np.array(rm.fe29(x), np.uint32) for x in (0, 1, 2, P - 1, nonsquare(), 4, P, 2**255 - 20)]
    for b in (1.0, 2.0, 7.999):
        for _ in range(4):
            f = f29_loose(rng, b)
            zs.append(f)
            sq = pow(rm.value(ints(f), 29), 2, P)                 # a square, in loose limbs
            l = rm.fe29(sq)
            l[1] += 3 << 29
            l[2] -= 3
            if l[2] >= 0:
                zs.append(np.array(l, np.uint32))
    pw = dh.run("ed", "ed16w_pow22523", u32(zs), 9)
    for z, h in zip(zs, pw):
        assert rm.value(ints(h), 29) % P == pow(rm.value(ints(z), 29) % P, (P - 5) // 8, P)
    count("ed/ed16w_pow22523", len(zs))
    tight = [z for z in zs if int(z.max()) <= 2 << 29]      # batch_wave_invert squares z itself: B <= 2.4
    iv = dh.run("ed", "ed_batch_wave_invert", u32(tight), 9)
    for z, g in zip(tight, iv):
        assert rm.value(ints(g), 29) % P == pow(rm.value(ints(z), 29) % P, P - 2, P)
    count("ed/ed_batch_wave_invert", len(tight))
    tors = rm.ed_torsion()
    pts = [(rm.ED_IDENTITY, 1), (rm.ED_IDENTITY, P - 5)]
    base = rm.ed_multiples(3, 11, 6)
    for i, b in enumerate(base):                                   # the representatives of one ristretto point
        pts += [(rm.ed_add(b, tors[k]), 3 + i + k) for k in (0, 2, 4, 6)]
    pts += [(q, 2**200 + i) for i, q in enumerate(rm.ed_multiples(64))]
    got = dh.run("ed", "ed_wave_encode", u32([rm.ed_point29(rm.ed_extended(q, z)) for q, z in pts]), 8)
    for (q, z), e in zip(pts, got):
        ext = rm.ed_extended(q, z)
        assert e.tobytes() == rm.ristretto_encode(ext), (q, z)
        assert e.tobytes() == bytes(hooks.ristretto_encode(np.array(rm.ed_point51(ext), np.uint64)))
    assert got[0].tobytes() == bytes(32) == got[1].tobytes()
    for i in range(3):
        assert len({got[2 + 4 * i + k].tobytes() for k in range(4)}) == 1
    count("ed/ed_wave_encode", len(pts))


#--------------------------------------------------------------------------------------------------
# Horner chains, multiples and doubling tables, both families, against double-and-add
#--------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def ed_multiple(k):
    return rm.ed_mul(k, rm.ED_BASE)


@functools.lru_cache(None)
def sw_multiple(name, k):
    c = rm.CURVES[name]
    return c.mul(k, c.base) if k >= 0 else c.neg(c.mul(-k, c.base))


class EdFamily:
    tag, words = "ed", 36
    ops = {"horner": "ed_wave_horner", "add_multiple": "ed_wave_add_multiple", "chain": "ed_wave_chain"}

    def point(self, k):
        return ed_multiple(k % rm.ED_L)

    def encode(self, pt, z):
        return rm.ed_point29(rm.ed_extended(pt, z))

    def matches(self, words, pt):
        return rm.ed_same(rm.ed_from29(words), pt)


class SwFamily:
    def __init__(self, name):
        self.c, self.tag, self.words = rm.CURVES[name], name, 3 * rm.CURVES[name].N
        self.ops = {"horner": "sww_horner", "add_multiple": "sww_add_multiple", "chain": "sww_wave_chain"}

    def point(self, k):
        return sw_multiple(self.c.name, k)

    def encode(self, pt, z):
        return rm.sw_point29(self.c, self.c.projective(pt, z))

    def matches(self, words, pt):
        # store_point hands the engine's form on: limbs below 2^LB, value below 1.001 p
        c = self.c
        for k in range(3):
            l = words[c.N * k:c.N * (k + 1)]
            assert max(l) < 1 << c.LB and rm.value(l, c.LB) < c.p + (c.p >> 10)
        return c.same(rm.sw_from29(c, words), pt)


FAMILIES = ["ed"] + CURVES


def family(name):
    return EdFamily() if name == "ed" else SwFamily(name)


@pytest.mark.parametrize("fam", FAMILIES)
def test_wave_horner(fam):
    f = family(fam)
    rng = random.Random(11)
    total = 0
    for nw in (1, 2, 17):
        for bits in (1, 2, 16):
            for have_acc in (0, 1):
                cases = [dc.horner_scalars(rng, nw, bits, have_acc, kind) for kind in dc.HORNER_KINDS]
                rec = u32([sum([f.encode(f.point(s), 2 + i + 3 * j) for j, s in enumerate([acc] + ws)], [])
                           for i, (acc, ws) in enumerate(cases)])
                got = dh.run(f.tag, f.ops["horner"], rec, f.words, (nw, bits, have_acc))
                for (acc, ws), kind, h in zip(cases, dc.HORNER_KINDS, got):
                    want = f.point(dc.horner_value(acc, ws, bits, have_acc))
                    assert f.matches(ints(h), want), (nw, bits, have_acc, kind)
                total += len(cases)
    count(f"{f.tag}/{f.ops['horner']} (num_windows 1, 2, 17 x window_bits 1, 2, 16 x have_acc)", total)


@pytest.mark.parametrize("fam", FAMILIES)
def test_wave_add_multiple(fam):
    """v + m s; m != 0 is the function's contract (k_reduce handles a zero block offset before the call)"""
    f = family(fam)
    cases = []
    for i, m in enumerate(dc.MULTIPLES):
        s = 3 + i
        for v in (7 + 2 * i, 0, -m * s, m * s):      # generic | identity | cancels at the end | doubles at the end
            cases.append((v, s, m))
        cases.append((5, 0, m))                        # s the identity
    rec = u32([f.encode(f.point(v), 2 + i) + f.encode(f.point(s), 9 + i) + [m] for i, (v, s, m) in enumerate(cases)])
    got = dh.run(f.tag, f.ops["add_multiple"], rec, f.words)
    for (v, s, m), h in zip(cases, got):
        assert f.matches(ints(h), f.point(v + m * s)), (v, s, m)
    count(f"{f.tag}/{f.ops['add_multiple']}", len(cases))


@pytest.mark.parametrize("fam", FAMILIES)
def test_wave_chain(fam):
    f = family(fam)
    total = 0
    for nw in (1, 2, 17):
        for bits in (1, 2, 16):
            gs = [0, 1, 12345, -7]
            rec = u32([f.encode(f.point(g), 3 + i) for i, g in enumerate(gs)])
            got = dh.run(f.tag, f.ops["chain"], rec, nw * f.words, (nw, bits))
            for g, h in zip(gs, got):
                for w in range(nw):
                    assert f.matches(ints(h[w * f.words:(w + 1) * f.words]), f.point(g << (bits * w))), (nw, bits, g, w)
            total += len(gs)
    count(f"{f.tag}/{f.ops['chain']}", total)


#--------------------------------------------------------------------------------------------------
# (b) + (c) sww::wave<G>
#--------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CURVES)
def test_sww_fmul_kernel_equals_model(name):
    c = rm.CURVES[name]
    t = dc.sww_tables(name)
    names = list(t["fmul"])
    got = dh.run(name, "sww_fmul", u32([t["fmul"][n][0] + t["fmul"][n][1] for n in names]), 64)
    rwi = rm.inv(c.Rw, c.p)
    for n, h in zip(names, got):
        u, v = t["fmul"][n]
        assert ints(h) == t["fmul_model"][n], n
        assert int(h.max()) < (1 << c.LB) + 2
        for r, (a, b, x) in enumerate(zip(rm.wave_values(c, u), rm.wave_values(c, v), rm.wave_values(c, ints(h)))):
            assert x % c.p == a * b * rwi % c.p, (n, r)
    count(f"{name}/sww_fmul", 4 * len(names))


@pytest.mark.parametrize("name", CURVES)
def test_sww_dbl_add_kernel_equals_model(name):
    c = rm.CURVES[name]
    t = dc.sww_tables(name)
    fam = SwFamily(name)
    for kind, op in (("dbl", "sww_dbl"), ("add", "sww_add")):
        names = [n for n in t["point"] if t["point"][n][0] == kind]
        got = dh.run(name, op, u32([t["point"][n][1] + (t["point"][n][2] or []) for n in names]), 64 + 3 * c.N)
        for n, h in zip(names, got):
            want = t["point"][n][3]
            live = [16 * r + j for r in range(4) for j in range(c.NW)]
            assert [int(h[l]) for l in live] == [t["point_model"][n][l] for l in live], n
            assert c.same(rm.wave_values(c, ints(h[:64]))[:3], want), n
            assert fam.matches(ints(h[64:]), want), n                       # store_point
        count(f"{name}/{op}", len(names))


@pytest.mark.parametrize("name", CURVES)
def test_sww_chains_and_roundtrip(name):
    c = rm.CURVES[name]
    fam = SwFamily(name)
    mult = c.multiples(3, 9, 4)
    starts = [None, mult[0], mult[1]]
    rec = []
    for i, pt in enumerate(starts):
        proj = c.projective(pt, 5 + i)
        lanes = []
        for v in proj:
            lanes += rm.limbs(v * c.R29 % c.p + (5 * c.p if i else 0), c.LB, c.N) + [0] * (16 - c.N)
        q = []
        for v in c.projective(mult[2], 77 + i):
            q += rm.limbs(v * c.R29 % c.p, c.LB, c.N) + [0] * (16 - c.N)
        rec.append(lanes + [0] * 16 + q + [0] * 16)
    rec = u32(rec)
    short = dh.run(name, "sww_chain", rec, 64 + 3 * c.N, (12,))
    live = [16 * r + j for r in range(4) for j in range(c.NW)]
    for r, h in zip(rec, short):
        want = dc.sww_chain_model(name, ints(r[:64]), ints(r[64:]), 12)
        assert [int(h[l]) for l in live] == [want[l] for l in live]
    long = dh.run(name, "sww_chain", rec, 64 + 3 * c.N, (300,))
    for pt, h in zip(starts, long):
        want = dc.sw_chain_point(c, pt, mult[2], 300)
        assert c.same(rm.wave_values(c, ints(h[:64]))[:3], want) and fam.matches(ints(h[64:]), want)
    count(f"{name}/sww_chain (12 steps against the model, 300 against the group law)", 2 * len(starts))
    # load_point_value -> store_point: the engine's loosest points (V up to 6) come back reduced
    pts = [None] + c.multiples(5, 4, 9)
    rec = u32([rm.sw_point29(c, c.projective(q, 3 + i), [(0, 0, 0), (5, 5, 5), (5, 0, 3)][i % 3])
               for i, q in enumerate(pts)])
    got = dh.run(name, "sww_roundtrip", rec, 64 + 3 * c.N)
    for q, r, h in zip(pts, rec, got):
        want_lanes = []
        for k in range(3):
            want_lanes += ints(r[c.N * k:c.N * (k + 1)]) + [0] * (16 - c.N)
        assert ints(h[:64]) == want_lanes + [0] * 16
        assert fam.matches(ints(h[64:]), q)
    count(f"{name}/sww_roundtrip", len(pts))


#--------------------------------------------------------------------------------------------------
# add_coop4: 16 independent quads per wavefront
#--------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CURVES)
def test_add_coop4(name):
    c = rm.CURVES[name]
    n3 = 3 * c.N
    m = c.multiples(16, 2, 3)
    pairs = []
    for q in range(16):
        a, kind = m[q], q % 5
        b = [m[(q + 5) % 16], a, a, None, c.neg(a)][kind]     # generic | doubling | identity left | right | inverse
        if kind == 2:
            a, b = None, a
        pairs.append((a, b))
    loose = [(0, 0, 0), (5, 5, 5), (2, 0, 4)]
    total = 0
    for perm in (list(range(16)), [(7 * q + 3) % 16 for q in range(16)]):   # the pairs moved across quads
        rec = []
        for slot, q in enumerate(perm):
            a, b = pairs[q]
            rec += rm.sw_point29(c, c.projective(a, 2 + q), loose[q % 3])
            rec += rm.sw_point29(c, c.projective(b, 11 + q), loose[(q + 1) % 3])
        got = dh.run(name, "sw29_coop4", u32([rec]), 64 * n3)[0]
        for slot, q in enumerate(perm):
            lanes = [ints(got[(4 * slot + r) * n3:(4 * slot + r + 1) * n3]) for r in range(4)]
            assert lanes[0] == lanes[1] == lanes[2] == lanes[3], (slot, q)
            assert c.same(rm.sw_from29(c, lanes[0]), c.add(*pairs[q])), (slot, q)
        total += 16
    count(f"{name}/sw29_coop4 (quads)", total)


def test_harness_rejects_what_it_cannot_validate():
    with pytest.raises(dh.HarnessError):
        dh.run("ed", "no_such_op", u32([[0]]), 1)
    with pytest.raises(dh.HarnessError):
        dh.run("ed", "ed16w_fmul", u32([[0] * 127]), 64)
    with pytest.raises(dh.HarnessError):
        dh.run("ed", "ed_wave_horner", u32([[0] * (19 * 36)]), 36, (18, 16, 1))
    # the proof object: a transcript position, fold digits and their count, parameter ranges
    dh.assert_proof_rejections()
