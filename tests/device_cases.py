"""Case tables of tests/test_device_arith.py: the inputs that put the lane-spread device arithmetic at
its contract bounds, with the expectations of the models (tools/models) and of big integers
(tests/refmath.py).  Pure Python, built once per process; tests/test_refmath.py checks the tables on
the CPU (every case inside the contracts the models assert, model == big integers), the GPU module
compares the kernels with them."""
import functools
import importlib.util
import os
import random

from tests import refmath as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = rm.P


@functools.lru_cache(None)
def model(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", "models", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def waves(rows):
    """rows (lists of 16 lane words) -> wavefronts of 4 rows, the last one padded by repeating"""
    rows = list(rows)
    while len(rows) % 4:
        rows.append(rows[-1])
    return [sum(rows[i:i + 4], []) for i in range(0, len(rows), 4)]


#--------------------------------------------------------------------------------------------------
# ed16w
#--------------------------------------------------------------------------------------------------
ED_UB = int(2**19.3)        # u limbs (ed16_wave.h: u < 2^19.3)
ED_VB = (1 << 24) // 38     # v limbs (the rotated operand times 38 must stay below 2^24)
ED_STATE = (1 << 16) + 63   # what a product may leave in a limb


def limbs16(x):
    return rm.limbs(x, 16, 16, loose_top=False)


def ed_formula_dbl(x, y, z):
    """the doubling ed16w::dbl evaluates, on any residues (projective result)"""
    a, b, zz, m = x * x, y * y, z * z, x * y
    e, h, g, f = 2 * m, a + b, b - a, a + 2 * zz - b
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def ed_formula_add_cached(st, cached):
    x, y, z, t = st
    a, b, zz, c = (y + x) * cached[0], (y - x) * cached[1], z * cached[2], t * cached[3]
    d = 2 * zz
    ez, et, ex, ey = d + c, d - c, a - b, a + b
    return (ex * et % P, ey * ez % P, ez * et % P, ex * ey % P)


def proj_equal(a, b, p=P):
    a, b = [v % p for v in a], [v % p for v in b]
    return any(a) and any(b) and all((a[i] * b[j] - a[j] * b[i]) % p == 0
                                     for i in range(len(a)) for j in range(len(a)))


@functools.lru_cache(None)
def ed16w_tables():
    m = model("ed16_wave_model")
    rng = random.Random(16)
    r16 = lambda: [rng.randrange(1 << 16) for _ in range(16)]  # noqa: E731
    t = {"fmul": {}, "fmul_model": {}, "point": {}, "point_model": {}}

    # ---- field products: pairs of rows, four to a wavefront so rows differ within one ----
    rows = []
    rows.append(([ED_UB] * 16, [ED_VB] * 16))                 # every limb at its bound: the largest columns
    rows.append(([ED_UB] * 16, r16()))
    rows.append((r16(), [ED_VB] * 16))
    rows.append(([rng.randrange(ED_UB + 1) for _ in range(16)], [rng.randrange(ED_VB + 1) for _ in range(16)]))
    for i in range(16):                                        # exactly one limb at the bound
        u, v = r16(), r16()
        u[i] = ED_UB
        rows.append((u, r16()))
        v[(5 * i + 3) % 16] = ED_VB
        rows.append((r16(), v))
        rows.append((u, v))
    special = [0, 1, 2**256 - 1, P, P - 1, 2**255 - 20, 2**256 - 38]   # 2^256 - 1 = 37: all limbs 0xffff
    for a in special:
        for b in special:
            rows.append((limbs16(a), limbs16(b)))
    for k in range(16):      # a carry that crosses every lane and wraps through x38
        v = [0xffff] * 16
        v[k] = 0x10000
        rows.append((limbs16(1), v))
        rows.append((v, limbs16(1)))
        rows.append((v, v))
    for k in range(16):      # a single limb at the bound against a full operand: one column takes it all
        u = [0] * 16
        u[k] = ED_UB
        rows.append((u, [ED_VB] * 16))
    for _ in range(24):
        rows.append(([rng.randrange(ED_STATE + 1) for _ in range(16)], [rng.randrange(ED_VB + 1) for _ in range(16)]))
    for i, (wu, wv) in enumerate(zip(waves([r[0] for r in rows]), waves([r[1] for r in rows]))):
        t["fmul"][f"w{i}"] = (wu, wv)
        t["fmul_model"][f"w{i}"] = m.run_fmul(wu, wv)

    # ---- points: (kind, state lanes, cached lanes or None, expected) ----
    tors = rm.ed_torsion()
    mult = rm.ed_multiples(8, 3, 7)
    zs = [1, 2, P - 1, 2**254 + 12345, 0x1234567890abcdef << 150]

    def state(pt, z):
        return rm.rows16(list(rm.ed_extended(pt, z)))

    def add_case(name, kind, st, q, want):
        t["point"][name] = (kind, st, q, want)
        t["point_model"][name] = m.run_dbl(st) if kind == "dbl" else m.run_add_cached(st, q)

    named = {"identity": rm.ED_IDENTITY, "minus_one": (0, P - 1)}
    named.update({f"torsion{k}": tors[k] for k in range(1, 8)})
    named.update({f"mult{k}": mult[k] for k in range(4)})
    for i, (nm, pt) in enumerate(named.items()):
        z = zs[i % len(zs)]
        add_case(f"dbl_{nm}", "dbl", state(pt, z), None, rm.ed_add(pt, pt))
        for j, (nq, q) in enumerate(list(named.items())[:: 3] + [("self", pt), ("neg", rm.ed_neg(pt))]):
            zq = zs[(i + j + 1) % len(zs)]
            add_case(f"add_{nm}_{nq}", "add", state(pt, z), rm.ed_cached_rows(rm.ed_extended(q, zq)),
                     rm.ed_add(pt, q))
    # Z != 1 and every state limb as large as a previous product may leave it: any residues will do
    # for the formulas, so all four rows sit at 2^16 + 63 (or have one limb there)
    for k in range(6):
        if k == 0:
            st = [ED_STATE - (l >> 4) * (l & 1) for l in range(64)]   # (rows differ: a real doubling)
        else:
            st = [rng.randrange(1 << 16) for _ in range(64)]
            for r in range(4):
                st[16 * r + (k * 5 + r * 3) % 16] = ED_STATE
            if k >= 4:
                st = [rng.choice([ED_STATE, ED_STATE - 1, 0xffff, 0]) for _ in range(64)]
        vals = rm.rows16_values(st)
        cached = [rng.randrange(1 << 16) for _ in range(64)] if k % 2 else [0xffff] * 64
        add_case(f"dbl_loose{k}", "dbl", st, None, ("formula", ed_formula_dbl(*vals[:3])))
        add_case(f"add_loose{k}", "add", st, cached,
                 ("formula", ed_formula_add_cached(vals, rm.rows16_values(cached))))
    return t


def ed_point_matches(got_ext, want):
    """want: an affine point (group law) or ('formula', projective 4-tuple)"""
    if isinstance(want[0], str):
        return proj_equal(got_ext, want[1])
    return rm.ed_same(got_ext, want)


def ed_chain_model(st, q, n):
    m = model("ed16_wave_model")
    for k in range(n):
        st = m.run_add_cached(st, q) if k % 3 == 0 else m.run_dbl(st)
    return st


def ed_chain_point(pt, q, n):
    for k in range(n):
        pt = rm.ed_add(pt, q) if k % 3 == 0 else rm.ed_add(pt, pt)
    return pt


def gather_rows():
    """raw 16-limb rows for ed16w::gather_row / store_point, four to a wavefront"""
    rng = random.Random(17)
    rows = [[0x1ffff] * 16, [0xffff] * 15 + [0x1ffff], [0] * 15 + [0x1ffff], [0x10000 + 63] * 16,
            [0xffff] * 16, limbs16(P), limbs16(P - 1), [0] * 16]
    for _ in range(12):
        rows.append([rng.choice([0x1ffff, 0x10000, 0xffff, rng.randrange(1 << 17)]) for _ in range(16)])
    rng.shuffle(rows)
    return waves(rows)


def gather_expected(row):
    """ed16w::gather_row in integers: 256 bits as 9 x 29, the overflow times 38 into limb 0"""
    total = rm.value(row, 16)
    h = rm.limbs(total % (1 << 256), 29, 9)
    h[0] += 38 * (total >> 256)
    return h


#--------------------------------------------------------------------------------------------------
# sww::wave
#--------------------------------------------------------------------------------------------------
def sww_rows(c, x):
    return rm.limbs(x, c.LB, c.NW) + [0] * (16 - c.NW)


def sww_largest_multiple(c):
    """the largest U = V = k p + (p - 1) the model admits for a product of two such values:
    U V / Rw + (1 + 2^-20) p + 1 < R29 (tools/models/sw_wave_model.py, Wave.mul)"""
    lo, hi = 1, 1 << 40
    ok = lambda k: ((k + 1) * c.p - 1) ** 2 // c.Rw + c.p + (c.p >> 20) + 1 < c.R29  # noqa: E731
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return (lo + 1) * c.p - 1


def sw_formula_add(c, a, b):
    """RCB15 Alg. 7 (a = 0) on any residues"""
    p, b3 = c.p, c.b3
    x1, y1, z1 = a
    x2, y2, z2 = b
    t0, t1, t2 = x1 * x2, y1 * y2, z1 * z2
    t3 = (x1 + y1) * (x2 + y2) - t0 - t1
    t4 = (y1 + z1) * (y2 + z2) - t1 - t2
    y3 = b3 * ((x1 + z1) * (x2 + z2) - t0 - t2)
    u = b3 * t2
    z3, t1m = t1 + u, t1 - u
    return ((t3 * t1m - t4 * y3) % p, (t1m * z3 + y3 * 3 * t0) % p, (z3 * t4 + 3 * t0 * t3) % p)


@functools.lru_cache(None)
def sww_tables(name):
    c = rm.CURVES[name]
    m = model("sw_wave_model")
    rng = random.Random(len(name) * 7)
    p, NW, LB = c.p, c.NW, c.LB
    t = {"fmul": {}, "fmul_model": {}, "point": {}, "point_model": {}}
    big = sww_largest_multiple(c)
    rows = []
    rows.append((sww_rows(c, big), sww_rows(c, big)))          # the largest multiples of p between products
    # ... one operand as large as a 32-bit top limb lets it be, against p - 1
    rows.append((sww_rows(c, ((1 << 31) * c.R29 // p) * p + p - 1), sww_rows(c, p - 1)))
    rows.append((sww_rows(c, 0), sww_rows(c, rng.randrange(p))))   # q = 0
    rows.append((sww_rows(c, rng.randrange(p)), sww_rows(c, 0)))
    rows.append((sww_rows(c, p - 1), sww_rows(c, p - 1)))
    for a in (c.Rw % p, c.R29 % p, 1, p, p + 1):
        for b in (c.Rw % p, c.R29 % p, p - 1):
            rows.append((sww_rows(c, a), sww_rows(c, b)))
    # u v = 0 mod p with u, v != 0 mod Rw
    rows.append((sww_rows(c, p), sww_rows(c, rng.randrange(1, p))))
    rows.append((sww_rows(c, rng.randrange(1, p)), sww_rows(c, 3 * p)))
    rows.append((sww_rows(c, p), sww_rows(c, p)))
    # garbage above lane NW - 1, which `live` must mask in v and the broadcast must not read in u
    for _ in range(3):
        u, v = sww_rows(c, rng.randrange(p)), sww_rows(c, rng.randrange(p))
        for j in range(NW, 16):
            u[j], v[j] = rng.randrange(1, 1 << 32), rng.randrange(1, 1 << 32)
        rows.append((u, v))
    # the low half's fractional part exactly zero with a non-zero carry into the high half:
    # u = 2^(LB-1) in lane a, v = 16 in lane NW-1-a: the only column sum is 2^(LB+3) in lane NW-1
    for a in range(NW):
        u, v = [0] * 16, [0] * 16
        u[a], v[NW - 1 - a] = 1 << (LB - 1), 16
        rows.append((u, v))
    # ... and non-zero: carried elements, and limbs as loose as the formulas hand them on
    for _ in range(12):
        rows.append((sww_rows(c, rng.randrange(p)), sww_rows(c, rng.randrange(p))))
    top = (2 << LB) + 512
    for k in range(8):
        bnd = [top if j < c.N else (8 if j < NW else 0) for j in range(16)]
        u = [b if k == 0 else rng.choice([b, rng.randrange(b + 1)]) for b in bnd]
        v = [b if k == 0 else rng.choice([b, rng.randrange(b + 1)]) for b in bnd]
        rows.append((u, v))
    for i, (wu, wv) in enumerate(zip(waves([r[0] for r in rows]), waves([r[1] for r in rows]))):
        t["fmul"][f"w{i}"] = (wu, wv)
        t["fmul_model"][f"w{i}"] = m.run_fmul(name, wu, wv)

    # ---- points ----
    mult = c.multiples(5, 3, 11)
    zs = [1, 2, p - 1, (1 << (LB * c.N - 9)) + 12345]

    def state(pt, z, k=(0, 0, 0), garbage=False):
        proj = c.projective(pt, z)
        vals = [v * c.R29 % p + ki * p for v, ki in zip(proj, k)]
        lanes = []
        for v in vals:
            lanes += rm.limbs(v, LB, c.N) + [0] * (16 - c.N)
        lanes += [rng.randrange(1 << LB) for _ in range(16)] if garbage else [0] * 16   # row 3 is unused
        return lanes

    def add_case(nm, kind, st, q, want):
        t["point"][nm] = (kind, st, q, want)
        t["point_model"][nm] = m.run_dbl(name, st) if kind == "dbl" else m.run_add(name, st, q)

    named = {"identity": None}
    named.update({f"mult{k}": mult[k] for k in range(4)})
    for i, (nm, pt) in enumerate(named.items()):
        z = zs[i % len(zs)]
        loose = (5, 5, 5) if i % 2 else (0, 0, 0)      # V up to 6, as sw29 hands points on
        add_case(f"dbl_{nm}", "dbl", state(pt, z, loose, garbage=i % 2 == 0), None, c.add(pt, pt))
        for j, (nq, q) in enumerate(list(named.items()) + [("self", pt), ("neg", c.neg(pt))]):
            zq = zs[(i + j + 1) % len(zs)]
            lq = (5, 4, 5) if j % 2 else (0, 0, 0)
            add_case(f"add_{nm}_{nq}", "add", state(pt, z, loose), state(q, zq, lq, garbage=j % 3 == 0),
                     c.add(pt, q))
    return t


def sww_chain_model(name, st, q, n):
    m = model("sw_wave_model")
    for k in range(n):
        st = m.run_add(name, st, q) if k % 3 == 0 else m.run_dbl(name, st)
    return st


def sw_chain_point(c, pt, q, n):
    for k in range(n):
        pt = c.add(pt, q) if k % 3 == 0 else c.add(pt, pt)
    return pt


#--------------------------------------------------------------------------------------------------
# Horner chains, multiples, doubling tables: points as integer multiples of the base point
#--------------------------------------------------------------------------------------------------
def horner_scalars(rng, num_windows, window_bits, have_acc, kind):
    """(acc scalar, window scalars) for acc' = 2^c acc + w_i from the top window down; `kind` places an
    identity, the running value (the addition is a doubling) or its negative (the chain passes through
    the identity) at window `at`"""
    acc = rng.choice(SCALAR_POOL) if have_acc else 0
    ws = [rng.choice(SCALAR_POOL) for _ in range(num_windows)]
    if kind == "plain":
        return acc, ws
    top = num_windows - 1
    at = {"identity_top": top, "identity_low": 0, "double_top": top, "double_low": 0, "cancel_top": top,
          "cancel_low": 0, "all_identity": 0}[kind]
    if kind == "all_identity":
        return acc, [0] * num_windows
    running = acc
    for i in range(top, -1, -1):
        first = not have_acc and i == top
        if not first:
            running <<= window_bits
        if i == at:
            if kind.startswith("identity"):
                ws[i] = 0
            elif kind.startswith("double"):
                ws[i] = running if running else 5
            else:
                ws[i] = -running
        running += ws[i]
    return acc, ws


SCALAR_POOL = [1, 2, 3, 0xffff, 0x10000, 0x12345, 0xfffff, 7 << 40, (1 << 64) - 1, 0xdeadbeefcafe, 11, 1 << 63]
HORNER_KINDS = ["plain", "identity_top", "identity_low", "double_top", "double_low", "cancel_top", "cancel_low",
                "all_identity"]


def horner_value(acc, ws, window_bits, have_acc):
    top = len(ws) - 1
    r = acc
    for i in range(top, -1, -1):
        if not (not have_acc and i == top):
            r <<= window_bits
        r += ws[i]
    return r


MULTIPLES = [1, 2, 3, 4, 7, 8, 0xff, 0x100, 0xffff, 0x10000, 0x7ffff, 0x80000, 0x7fffffff, 0x80000000,
             0xffffffff]
