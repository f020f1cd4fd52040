"""Plain-integer mathematics for the device-arithmetic tests: the expected side of
tests/test_device_arith.py.  Nothing here shares code with the kernels, tests/hooks.py or
tools/models; tests/test_refmath.py pins it to the host hooks (and the oracle where built).

  * GF(2^255 - 19) and the three Montgomery base fields,
  * twisted-Edwards (edwards25519) and short-Weierstrass group laws in affine coordinates, the
    identity handled explicitly, projective equality, the ristretto255 encoding,
  * limb packing for every layout the kernels use: 5 x 51, 9 x 29, N x LB, a wavefront of 4 rows of
    16 x 16 bits, a wavefront of 4 rows of (N + 1) x LB bits,
  * points as integer multiples of a base point (no rejection sampling)."""

#--------------------------------------------------------------------------------------------------
# GF(2^255 - 19), edwards25519, ristretto255
#--------------------------------------------------------------------------------------------------
P = 2**255 - 19
D = -121665 * pow(121666, P - 2, P) % P
SQRT_M1 = pow(2, (P - 1) // 4, P)
ED_L = 2**252 + 27742317777372353535851937790883648493  # order of the base point
ED_IDENTITY = (0, 1)


def inv(x, p=P):
    return pow(x, p - 2, p)


def sqrt_ratio_m1(u, v):
    """RFC 9496 4.2: (was_square, r) with r = sqrt(u / v) or sqrt(i u / v), non-negative"""
    u, v = u % P, v % P
    r = u * pow(v, 3, P) * pow(u * pow(v, 7, P), (P - 5) // 8, P) % P
    check = v * r * r % P
    correct = check == u
    flipped = check == -u % P
    flipped_i = check == -u * SQRT_M1 % P
    if flipped or flipped_i:
        r = r * SQRT_M1 % P
    if r & 1:
        r = P - r
    return correct or flipped, r


def ed_recover_x(y, sign):
    ok, x = sqrt_ratio_m1(y * y - 1, D * y * y + 1)
    assert ok
    if x & 1 != sign:
        x = (P - x) % P
    return x


ED_BASE = (ed_recover_x(4 * inv(5) % P, 0), 4 * inv(5) % P)


def ed_on_curve(pt):
    x, y = pt
    return (-x * x + y * y - 1 - D * x * x * y * y) % P == 0


def ed_add(a, b):
    """affine twisted-Edwards addition (a = -1): complete, the identity is (0, 1)"""
    x1, y1 = a
    x2, y2 = b
    t = D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + x2 * y1) * inv(1 + t) % P, (y1 * y2 + x1 * x2) * inv(1 - t) % P)


def ed_neg(a):
    return ((P - a[0]) % P, a[1])


def ed_mul(k, a):
    acc = ED_IDENTITY
    for bit in bin(k)[2:] if k else "":
        acc = ed_add(acc, acc)
        if bit == "1":
            acc = ed_add(acc, a)
    return acc


def ed_ext_add(a, b):
    """extended twisted-Edwards addition (a = -1) on (X, Y, Z, T): complete, no inversion"""
    x1, y1, z1, t1 = a
    x2, y2, z2, t2 = b
    aa, bb = (y1 - x1) * (y2 - x2) % P, (y1 + x1) * (y2 + x2) % P
    cc, dd = 2 * D * t1 * t2 % P, 2 * z1 * z2 % P
    e, f, g, h = bb - aa, dd - cc, dd + cc, bb + aa
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def ed_ext_mul(k, pt):
    """k pt in extended coordinates, by double-and-add without inversions (pt affine)"""
    acc, ext = (0, 1, 1, 0), (pt[0], pt[1], 1, pt[0] * pt[1] % P)
    for bit in bin(k)[2:] if k else "":
        acc = ed_ext_add(acc, acc)
        if bit == "1":
            acc = ed_ext_add(acc, ext)
    return acc


def ed_multiples(n, first=1, step=1):
    """[first B, (first + step) B, ...], n points"""
    out, cur, inc = [], ed_mul(first, ED_BASE), ed_mul(step, ED_BASE)
    for _ in range(n):
        out.append(cur)
        cur = ed_add(cur, inc)
    return out


def ed_torsion():
    """the 8 points of order dividing 8, as multiples k T8 (k = 0..7) of a point of order 8"""
    y = 2
    while True:
        ok, x = sqrt_ratio_m1(y * y - 1, D * y * y + 1)
        if ok:
            t = ed_mul(ED_L, (x, y))
            if ed_mul(4, t) != ED_IDENTITY:
                return [ed_mul(k, t) for k in range(8)]
        y += 1


def ed_extended(pt, z=1):
    """(X, Y, Z, T) with the given Z"""
    x, y = pt
    z %= P
    return (x * z % P, y * z % P, z, x * y % P * z % P)


def ed_affine(ext):
    zi = inv(ext[2])
    return (ext[0] * zi % P, ext[1] * zi % P)


def ed_same(ext, pt):
    """projective equality of (X : Y : Z : T) with an affine point, T consistent"""
    X, Y, Z, T = (c % P for c in ext)
    x, y = pt
    return Z != 0 and (X - x * Z) % P == 0 and (Y - y * Z) % P == 0 and (X * Y - Z * T) % P == 0


def ristretto_encode(ext):
    """RFC 9496 4.3.2 from extended coordinates -> 32 bytes"""
    x0, y0, z0, t0 = (c % P for c in ext)
    u1 = (z0 + y0) * (z0 - y0) % P
    u2 = x0 * y0 % P
    _, invsqrt = sqrt_ratio_m1(1, u1 * u2 * u2)
    den1 = invsqrt * u1 % P
    den2 = invsqrt * u2 % P
    z_inv = den1 * den2 * t0 % P
    ix0 = x0 * SQRT_M1 % P
    iy0 = y0 * SQRT_M1 % P
    _, invsqrt_a_minus_d = sqrt_ratio_m1(1, (-1 - D) % P)
    enchanted = den1 * invsqrt_a_minus_d % P
    if (t0 * z_inv % P) & 1:
        x, y, den_inv = iy0, ix0, enchanted
    else:
        x, y, den_inv = x0, y0, den2
    if (x * z_inv % P) & 1:
        y = (P - y) % P
    s = den_inv * (z0 - y) % P
    if s & 1:
        s = P - s
    return s.to_bytes(32, "little")


#--------------------------------------------------------------------------------------------------
# Montgomery base fields and short-Weierstrass curves y^2 = x^3 + b
#--------------------------------------------------------------------------------------------------
class Curve:
    def __init__(self, name, cid, p, lb, n, n64, b):
        self.name, self.cid, self.p, self.LB, self.N, self.NW, self.N64, self.b = name, cid, p, lb, n, n + 1, n64, b
        self.R29 = 1 << (lb * n)          # radix of the engine's N x LB form
        self.Rw = 1 << (lb * (n + 1))     # radix of the wave's (N + 1) x LB form
        self.R64 = 1 << (64 * n64)        # radix of the ABI form
        self.mask = (1 << lb) - 1
        self.b3 = 3 * b % p
        self.base = self._first_point()

    def _first_point(self):
        x = 1
        while True:
            y = sqrt_mod((x**3 + self.b) % self.p, self.p)
            if y is not None:
                return (x, min(y, self.p - y))
            x += 1

    def on_curve(self, pt):
        return pt is None or (pt[1] ** 2 - pt[0] ** 3 - self.b) % self.p == 0

    def add(self, a, b):
        """affine chord-and-tangent; None is the identity"""
        p = self.p
        if a is None:
            return b
        if b is None:
            return a
        if a[0] == b[0]:
            if (a[1] + b[1]) % p == 0:
                return None
            lam = 3 * a[0] * a[0] * inv(2 * a[1], p) % p
        else:
            lam = (b[1] - a[1]) * inv(b[0] - a[0], p) % p
        x = (lam * lam - a[0] - b[0]) % p
        return (x, (lam * (a[0] - x) - a[1]) % p)

    def neg(self, a):
        return None if a is None else (a[0], (self.p - a[1]) % self.p)

    def mul(self, k, a):
        acc = None
        for bit in bin(k)[2:] if k else "":
            acc = self.add(acc, acc)
            if bit == "1":
                acc = self.add(acc, a)
        return acc

    def multiples(self, n, first=1, step=1):
        out, cur, inc = [], self.mul(first, self.base), self.mul(step, self.base)
        for _ in range(n):
            out.append(cur)
            cur = self.add(cur, inc)
        return out

    def projective(self, pt, z=1):
        if pt is None:
            return (0, z % self.p, 0)
        return (pt[0] * z % self.p, pt[1] * z % self.p, z % self.p)

    def same(self, proj, pt):
        """projective equality of (X : Y : Z) with an affine point or None"""
        X, Y, Z = (c % self.p for c in proj)
        if pt is None:
            return X == 0 and Z == 0 and Y != 0
        return Z != 0 and (X - pt[0] * Z) % self.p == 0 and (Y - pt[1] * Z) % self.p == 0


def sqrt_mod(a, p):
    """Tonelli-Shanks; None for a non-residue"""
    a %= p
    if a == 0:
        return 0
    if pow(a, (p - 1) // 2, p) != 1:
        return None
    if p % 4 == 3:
        return pow(a, (p + 1) // 4, p)
    q, e = p - 1, 0
    while q % 2 == 0:
        q //= 2
        e += 1
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1:
        z += 1
    m, c, t, r = e, pow(z, q, p), pow(a, q, p), pow(a, (q + 1) // 2, p)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2 = t2 * t2 % p
            i += 1
        b = pow(c, 1 << (m - i - 1), p)
        m, c = i, b * b % p
        t, r = t * c % p, r * b % p
    return r


BN254 = Curve("bn254", 2, 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47, 29, 9, 4, 3)
GRUMPKIN = Curve("grumpkin", 3, 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001, 29, 9, 4,
                 -17)
BLS12_381 = Curve(
    "bls12_381", 1,
    0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab,
    28, 14, 6, 4)
CURVES = {c.name: c for c in (BN254, GRUMPKIN, BLS12_381)}

#--------------------------------------------------------------------------------------------------
# limb layouts
#--------------------------------------------------------------------------------------------------
def limbs(x, bits, n, loose_top=True):
    """n limbs of `bits` bits; the top limb takes whatever is left when loose_top"""
    out = [(x >> (bits * i)) & ((1 << bits) - 1) for i in range(n)]
    if loose_top:
        out[-1] = x >> (bits * (n - 1))
    assert sum(v << (bits * i) for i, v in enumerate(out)) == x
    return out


def value(ls, bits):
    return sum(int(v) << (bits * i) for i, v in enumerate(ls))


def fe51(x):
    return limbs(x, 51, 5)


def fe29(x):
    return limbs(x, 29, 9)


def words(ls64):
    """u64 values -> little-endian pairs of 32-bit words"""
    out = []
    for v in ls64:
        out += [int(v) & 0xffffffff, int(v) >> 32]
    return out


def from_words(ws):
    return [int(ws[2 * i]) | (int(ws[2 * i + 1]) << 32) for i in range(len(ws) // 2)]


def ed_point51(ext):
    """(X, Y, Z, T) -> the 20 u64 of an element_p3"""
    return [l for c in ext for l in fe51(c % P)]


def ed_point29(ext):
    """(X, Y, Z, T) -> the 36 limbs of an ed29_point"""
    return [l for c in ext for l in fe29(c % P)]


def ed_from29(ws):
    return tuple(value(ws[9 * k:9 * k + 9], 29) for k in range(4))


def ed_from51(ls64):
    return tuple(value(ls64[5 * k:5 * k + 5], 51) for k in range(4))


def rows16(vals):
    """4 values < 2^256 -> the 64 lane words of ed16w (row r = value r, lane j = limb j)"""
    out = []
    for v in vals:
        assert 0 <= v < 1 << 256
        out += limbs(v, 16, 16, loose_top=False)
    return out


def rows16_values(lanes):
    """64 lane words (any size) -> the 4 row values, not reduced"""
    return [value(lanes[16 * r:16 * r + 16], 16) for r in range(4)]


def ed_cached_rows(ext):
    """the cached operand of ed16w::add_cached: (Y + X | Y - X | Z | 2 d T), canonical rows"""
    x, y, z, t = ext
    return rows16([(y + x) % P, (y - x) % P, z % P, 2 * D * t % P])


def wave_rows(c, vals):
    """4 values -> 64 lane words of sww::wave (row r = value r in NW limbs of LB bits, lanes >= NW 0)"""
    out = []
    for v in vals:
        out += limbs(v, c.LB, c.NW) + [0] * (16 - c.NW)
    return out


def wave_values(c, lanes):
    return [value(lanes[16 * r:16 * r + c.NW], c.LB) for r in range(4)]


def mont_limbs(c, x):
    """the engine's N x LB limbs of the integer x (callers pass a R29 mod p, or a loose multiple)"""
    return limbs(x, c.LB, c.N)


def sw_point29(c, proj, k=(0, 0, 0)):
    """projective (X, Y, Z) -> 3 N engine limbs: coordinate R29 mod p plus k[i] p"""
    out = []
    for v, ki in zip(proj, k):
        out += mont_limbs(c, v * c.R29 % c.p + ki * c.p)
    return out


def sw_from29(c, ws):
    """3 N engine limbs -> projective residues (X, Y, Z)"""
    ri = inv(c.R29, c.p)
    return tuple(value(ws[c.N * k:c.N * (k + 1)], c.LB) * ri % c.p for k in range(3))


def sw_point64(c, proj):
    """projective (X, Y, Z) -> 3 N64 u64 of the ABI's Montgomery form"""
    out = []
    for v in proj:
        out += limbs(v * c.R64 % c.p, 64, c.N64)
    return out


def sw_from64(c, ls64):
    ri = inv(c.R64, c.p)
    return tuple(value(ls64[c.N64 * k:c.N64 * (k + 1)], 64) * ri % c.p for k in range(3))
