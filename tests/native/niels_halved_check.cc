// Stand-alone host check of the halved Z = 1 addend of curve25519 (blitzar_amd/csrc/curve/ed29.h:
// ed29_niels = ((y+x)/2, (y-x)/2, d x y), add_niels, from_niels, to_niels; msm/curve_traits.h:
// ed25519_niels_msm::niels_of) and of the 32-bit piece offsets of k_accumulate's row gather
// (msm/lds_gather.h: narrow_offsets, piece_offset32).  tests/test_niels_halved_host.py builds and runs
// it (once more with -fsanitize=address,undefined) and reads the lines it prints:
//   <check> <failures> <cases>       every check wants no failure
//   max <name> <value>               the maxima the bounds check saw
// Exit status 0 when no check has a failure.
//
// The bounds check (c) measures limbs in units of u = 2^29 + 2^18, the exclusive limb bound of a
// product's output (field/f29.h: "B ~ 1" is a limb below u).  In that unit the file's bookkeeping is
// exact: a sum of two B 1 values is below 2 u, sub(f, g) = f + 2^30 - 2 - g below B(f) u + 2 u, and
// the contract of mul reads max limb(f) * max limb(g) <= 6 u^2.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "blitzar_amd/csrc/msm/curve_traits.h"
#include "blitzar_amd/csrc/msm/lds_gather.h"

using namespace bz;
using C = ed25519_niels_msm;
using u128 = unsigned __int128;

static fe51 limbs51(const u64 (&v)[5]) {
  fe51 f;
  for (int i = 0; i < 5; ++i) f.v[i] = v[i];
  return f;
}

static bool same_value(const fe29& a, const fe29& b) {
  u64 x[4], y[4];
  f29::to_words(x, a);
  f29::to_words(y, b);
  return std::memcmp(x, y, sizeof(x)) == 0;
}

static fe29 random_fe(std::mt19937_64& rng) {
  u64 v[5];
  for (u64& l : v) l = rng() & ((u64{1} << 51) - 1);
  return f29::from_fe51(limbs51(v));
}

// the same projective point: cross products, and X Y = Z T of `got`
static bool same_point(const ed29_point& got, const ed29_point& want) {
  return same_value(f29::mul(got.X, want.Z), f29::mul(want.X, got.Z)) &&
         same_value(f29::mul(got.Y, want.Z), f29::mul(want.Y, got.Z)) &&
         same_value(f29::mul(got.X, got.Y), f29::mul(got.Z, got.T)) && !f29::is_zero(got.Z);
}

static ed29_point reduced(const ed29_point& p) {
  return {f29::weak_reduce(p.X), f29::weak_reduce(p.Y), f29::weak_reduce(p.Z), f29::weak_reduce(p.T)};
}

static ed29_point base_point() {
  // the ristretto255 base point (RFC 9496, A.1)
  const u8 base[32] = {0xe2, 0xf2, 0xae, 0x0a, 0x6a, 0xbc, 0x4e, 0x71, 0xa8, 0x84, 0xa9,
                       0x61, 0xc5, 0x00, 0x51, 0x5f, 0x58, 0xe3, 0x0b, 0x6a, 0xa5, 0x82,
                       0xdd, 0x8d, 0xb6, 0xa6, 0x59, 0x45, 0xe0, 0x8d, 0x2d, 0x76};
  ed_point decoded;
  if (!ristretto29::decode(decoded, base)) std::abort();
  return ed29::from_ed(decoded);
}

// limbs of p = 2^255 - 19: adding them limb-wise leaves the value and makes the limbs loose
static fe29 limbs_of_p() {
  fe29 p;
  p.v[0] = f29::kMask - 18;
  for (int i = 1; i < 8; ++i) p.v[i] = f29::kMask;
  p.v[8] = (1u << 23) - 1;
  return p;
}

//--------------------------------------------------------------------------------------------------
// (c) add_niels rebuilt in wide integers
//--------------------------------------------------------------------------------------------------
constexpr u64 kUnit = (u64{1} << 29) + (u64{1} << 18); // exclusive limb bound of a product's output

struct bounds {
  unsigned long failures = 0, cases = 0;
  u128 max_high_column = 0; // column sums 9..16 of a product
  u128 max_low_column = 0;  // the running accumulator of columns 0..8, fold and carry included
  u64 max_product_limb = 0; // output limbs of the seven products
  u64 max_limb = 0;         // any intermediate limb (must fit 32 bits)
  double max_bb = 0;        // max limb(f) * max limb(g) / u^2 over the products
  long long min_sub = 1ll << 62; // smallest limb a sub produced, before it is stored
};

struct wide {
  u64 v[9];
};
static wide widen(const fe29& f) {
  wide w;
  for (int i = 0; i < 9; ++i) w.v[i] = f.v[i];
  return w;
}
static u64 max_of(const wide& f) {
  u64 m = 0;
  for (u64 l : f.v) m = l > m ? l : m;
  return m;
}
static void seen(bounds& b, const wide& f) {
  const u64 m = max_of(f);
  if (m > b.max_limb) b.max_limb = m;
  b.failures += m >> 32 != 0 ? 1 : 0;
}
static wide m_add(bounds& b, const wide& f, const wide& g) {
  wide h;
  for (int i = 0; i < 9; ++i) h.v[i] = f.v[i] + g.v[i];
  seen(b, h);
  return h;
}
static wide m_sub(bounds& b, const wide& f, const wide& g) {
  wide h;
  for (int i = 0; i < 9; ++i) {
    const long long bias = i == 0 ? (1ll << 30) - 2 * f29::kWrap : (1ll << 30) - 2;
    const long long t = static_cast<long long>(f.v[i]) + bias - static_cast<long long>(g.v[i]);
    if (t < b.min_sub) b.min_sub = t;
    b.failures += t < 0 ? 1 : 0;
    h.v[i] = static_cast<u64>(t < 0 ? 0 : t);
  }
  seen(b, h);
  return h;
}
// b ? bias - f : f, as cneg_xad computes it
static wide m_cneg(bounds& b, const wide& f, bool negate) {
  wide zero{};
  return negate ? m_sub(b, zero, f) : f;
}
// f29::mul column by column, every sum in 128 bits
static wide m_mul(bounds& b, const wide& f, const wide& g) {
  const double bb = static_cast<double>(max_of(f)) * static_cast<double>(max_of(g)) /
                    (static_cast<double>(kUnit) * static_cast<double>(kUnit));
  if (bb > b.max_bb) b.max_bb = bb;
  u128 c[8];
  for (int k = 9; k <= 16; ++k) {
    u128 t = 0;
    for (int i = k - 8; i <= 8; ++i) t += static_cast<u128>(f.v[i]) * g.v[k - i];
    if (t > b.max_high_column) b.max_high_column = t;
    b.failures += t >> 64 != 0 ? 1 : 0;
    c[k - 9] = t;
  }
  wide h;
  u128 acc = 0;
  for (int k = 0; k <= 8; ++k) {
    if (k < 8) acc += static_cast<u128>(static_cast<u32>(c[k])) * f29::kWrap;
    if (k > 0) acc += static_cast<u128>(static_cast<u32>(c[k - 1] >> 32)) * (8 * f29::kWrap);
    for (int i = 0; i <= k; ++i) acc += static_cast<u128>(f.v[i]) * g.v[k - i];
    if (acc > b.max_low_column) b.max_low_column = acc;
    b.failures += acc >> 64 != 0 ? 1 : 0;
    h.v[k] = static_cast<u64>(acc) & f29::kMask;
    acc >>= 29;
  }
  // (what is left sits at 2^261; the code folds its low and high 32 bits separately)
  b.failures += acc >> 35 != 0 ? 1 : 0;
  const u128 t0 = acc * f29::kWrap + h.v[0];
  b.failures += t0 >> 64 != 0 ? 1 : 0;
  h.v[0] = static_cast<u64>(t0) & f29::kMask;
  h.v[1] += static_cast<u64>(t0 >> 29);
  const u64 m = max_of(h);
  if (m > b.max_product_limb) b.max_product_limb = m;
  b.failures += m >= kUnit ? 1 : 0;
  return h;
}

struct wide_point {
  wide X, Y, Z, T;
};
// add_niels (curve/ed29.h), line by line
static wide_point m_add_niels(bounds& b, const wide_point& p, const ed29_niels& q, bool negate) {
  const wide qa = widen(negate ? q.YmX : q.YpX);
  const wide qb = widen(negate ? q.YpX : q.YmX);
  const wide qt = m_cneg(b, widen(q.T2d), !negate);
  const wide a = m_mul(b, m_add(b, p.Y, p.X), qa);
  const wide bb = m_mul(b, m_sub(b, p.Y, p.X), qb);
  const wide cn = m_mul(b, p.T, qt);
  const wide et = m_add(b, p.Z, cn);
  const wide ez = m_sub(b, p.Z, cn);
  const wide ex = m_sub(b, a, bb);
  const wide ey = m_add(b, a, bb);
  wide_point r;
  r.X = m_mul(b, ex, et);
  r.Y = m_mul(b, ey, ez);
  r.Z = m_mul(b, ez, et);
  r.T = m_mul(b, ex, ey);
  return r;
}
static bool same_limbs(const wide& w, const fe29& f) {
  for (int i = 0; i < 9; ++i) {
    if (w.v[i] != f.v[i]) return false;
  }
  return true;
}

static void print_u128(const char* name, u128 v) {
  // as a multiple of 2^64, six digits: the bound is 1
  std::printf("max %s %.6f\n", name, static_cast<double>(v) / 18446744073709551616.0);
}

int main() {
  int bad = 0;
  std::mt19937_64 rng(0x4a1fed);
  const ed29_point g = base_point();
  const fe29 d2 = f29::const_2d();

  // (a) to_niels and niels_of hold ((y+x)/2, (y-x)/2, d x y): doubled, they are y + x, y - x and
  //     2d x y of the affine point computed separately
  {
    unsigned long failures = 0, cases = 0;
    auto check = [&](const ed29_point& shown, const ed29_point& clean) {
      const fe29 zinv = f29::invert(clean.Z);
      const fe29 x = f29::mul(clean.X, zinv), y = f29::mul(clean.Y, zinv);
      const fe29 ypx = f29::add(y, x), ymx = f29::sub(y, x);
      const fe29 t2d = f29::mul(f29::mul(x, y), d2);
      const ed29_niels forms[2] = {ed29::to_niels(shown),
                                   C::niels_of(shown.X, shown.Y, f29::invert(shown.Z))};
      for (const ed29_niels& n : forms) {
        bool ok = same_value(f29::add(n.YpX, n.YpX), ypx) && same_value(f29::add(n.YmX, n.YmX), ymx) &&
                  same_value(f29::add(n.T2d, n.T2d), t2d);
        for (int k = 0; k < 9; ++k) {
          ok = ok && n.YpX.v[k] < kUnit && n.YmX.v[k] < kUnit && n.T2d.v[k] < kUnit;
        }
        for (int k = 0; k < 5; ++k) ok = ok && n.pad[k] == 0;
        failures += ok ? 0 : 1;
        cases += 1;
      }
    };
    const ed29_point order2 = {f29::zero(), f29::weak_reduce(f29::neg(f29::one())), f29::one(),
                               f29::zero()};
    const ed29_point specials[2] = {ed29::identity(), order2};
    const fe29 p_limbs = limbs_of_p();
    ed29_point p = g;
    for (int i = 0; i < 600; ++i) {
      ed29_point q = i < 2 ? specials[i] : p;
      if (i >= 2) p = ed29::add(p, ed29::dbl_n(p, 1 + i % 3));
      check(q, q); // as it stands (the walk's points have Z != 1)
      fe29 lambda = random_fe(rng);
      if (f29::is_zero(lambda)) lambda = f29::one();
      const ed29_point scaled = {f29::mul(q.X, lambda), f29::mul(q.Y, lambda), f29::mul(q.Z, lambda),
                                 f29::mul(q.T, lambda)};
      check(scaled, scaled);
      // unreduced: X and Y with the bias of a subtraction on every limb (B 3), Z + p (B 2)
      const ed29_point loose = {f29::sub(scaled.X, f29::zero()), f29::sub(scaled.Y, f29::zero()),
                                f29::add(scaled.Z, p_limbs), scaled.T};
      check(loose, scaled);
    }
    std::printf("stored_form %lu %lu\n", failures, cases);
    bad += failures != 0;
  }

  // (b) add_niels and from_niels against ed29::add, both signs; chains that alternate P and -P
  {
    unsigned long failures = 0, cases = 0;
    ed29_point p = g, acc = ed29::dbl_n(g, 7);
    for (int i = 0; i < 500; ++i) {
      p = ed29::add(p, ed29::dbl_n(p, 1 + i % 3));
      const ed29_niels row = ed29::to_niels(p);
      for (int s = 0; s < 2; ++s) {
        const bool negate = s != 0;
        const ed29_point q = negate ? ed29::neg(p) : p;
        failures += same_point(ed29::add_niels(acc, row, negate), ed29::add(acc, q)) ? 0 : 1;
        failures += same_point(ed29::from_niels(row, negate), q) ? 0 : 1;
        failures += same_point(C::first(row, negate), q) ? 0 : 1;
        ed29_point via_traits = acc;
        C::accumulate(via_traits, row, negate);
        failures += same_point(via_traits, ed29::add(acc, q)) ? 0 : 1;
        cases += 4;
      }
      acc = ed29::add_niels(acc, row, (i & 1) != 0);
    }
    std::printf("addition_matches_add %lu %lu\n", failures, cases);
    bad += failures != 0;

    failures = cases = 0;
    for (int chain = 0; chain < 8; ++chain) {
      p = ed29::add(p, ed29::dbl_n(p, 2));
      const ed29_niels row = ed29::to_niels(p);
      const ed29_point minus = ed29::neg(p);
      // from the identity and from the loaded first entry
      ed29_point got = chain % 2 == 0 ? ed29::identity() : ed29::from_niels(row, true);
      ed29_point want = chain % 2 == 0 ? ed29::identity() : minus;
      for (int i = 0; i < 64; ++i) {
        const bool negate = (i & 1) != 0; // + P first, in both kinds of chain
        got = ed29::add_niels(got, row, negate);
        want = reduced(ed29::add(want, negate ? minus : p));
        bool ok = same_point(got, want);
        // the accumulator is the identity after every second addition of the even chains, after
        // every first one of the odd chains
        const bool at_identity = chain % 2 == 0 ? (i & 1) != 0 : (i & 1) == 0;
        if (at_identity) ok = ok && f29::is_zero(got.X) && f29::is_zero(got.T) && same_value(got.Y, got.Z);
        failures += ok ? 0 : 1;
        cases += 1;
      }
    }
    std::printf("chains_through_identity %lu %lu\n", failures, cases);
    bad += failures != 0;
  }

  // (c) the contract: accumulators and addends with every limb at the largest value a product can
  //     leave, zero limbs where a subtraction takes them away, random mixtures of both, and chains
  //     that feed the result back; the model's limbs must be the code's
  {
    bounds b;
    const u32 top = static_cast<u32>(kUnit - 1);
    auto filled = [&](int mode) { // 0: zero, 1: top, 2: per limb one or the other, 3: random below top
      fe29 f;
      for (int i = 0; i < 9; ++i) {
        f.v[i] = mode == 0   ? 0u
                 : mode == 1 ? top
                 : mode == 2 ? ((rng() & 1) != 0 ? top : 0u)
                             : static_cast<u32>(rng() % kUnit);
      }
      return f;
    };
    auto run = [&](ed29_point p, const ed29_niels& q, bool negate, int steps) {
      wide_point w = {widen(p.X), widen(p.Y), widen(p.Z), widen(p.T)};
      for (int s = 0; s < steps; ++s) {
        w = m_add_niels(b, w, q, negate != ((s & 1) != 0));
        p = ed29::add_niels(p, q, negate != ((s & 1) != 0));
        const bool ok = same_limbs(w.X, p.X) && same_limbs(w.Y, p.Y) && same_limbs(w.Z, p.Z) &&
                        same_limbs(w.T, p.T);
        b.failures += ok ? 0 : 1;
        b.cases += 1;
      }
    };
    // every corner: each of X, Y, Z, T and of the three row fields all zero or all top
    for (int corner = 0; corner < 128; ++corner) {
      const ed29_point p = {filled(corner & 1), filled(corner >> 1 & 1), filled(corner >> 2 & 1),
                            filled(corner >> 3 & 1)};
      ed29_niels q{};
      q.YpX = filled(corner >> 4 & 1);
      q.YmX = filled(corner >> 5 & 1);
      q.T2d = filled(corner >> 6 & 1);
      run(p, q, false, 4);
      run(p, q, true, 4);
    }
    for (int i = 0; i < 4000; ++i) {
      const int mode = 2 + i % 2;
      const ed29_point p = {filled(mode), filled(mode), filled(mode), filled(mode)};
      ed29_niels q{};
      q.YpX = filled(mode);
      q.YmX = filled(mode);
      q.T2d = filled(mode);
      run(p, q, (i & 2) != 0, 3);
    }
    b.failures += b.max_bb > 6.0 ? 1 : 0;
    print_u128("high_column_over_2_64", b.max_high_column);
    print_u128("low_column_over_2_64", b.max_low_column);
    std::printf("max product_limb_over_unit %.6f\n",
                static_cast<double>(b.max_product_limb) / static_cast<double>(kUnit));
    std::printf("max limb_over_2_32 %.6f\n", static_cast<double>(b.max_limb) / 4294967296.0);
    std::printf("max b_times_b %.6f\n", b.max_bb);
    std::printf("min sub_limb %lld\n", b.min_sub);
    std::printf("contract %lu %lu\n", b.failures, b.cases);
    bad += b.failures != 0;
  }

  // the 32-bit piece offsets: the same address as the 64-bit form wherever narrow_offsets allows
  // them, and never allowed when a row of the task could lie beyond 4 GiB
  {
    namespace lg = lds_gather;
    unsigned long failures = 0, cases = 0;
    const u64 limit = u64{1} << 25; // rows of 128 bytes in 4 GiB
    const u64 bases[] = {0, 1, 4096, limit / 2, limit - 1, limit, limit + 1, (u64{1} << 31) - 2};
    const u64 counts[] = {1, 2, 65, 1u << 20, limit / 2, limit - 1, limit, limit + 1, (u64{1} << 31) - 1};
    for (u64 base : bases) {
      for (u64 rows : counts) {
        if (base + rows >= (u64{1} << 31)) continue; // (plan.h: a task's rows share 31 bits)
        const bool narrow = lg::narrow_offsets(base, rows);
        const u64 last = base + rows - 1; // the largest row an entry of the task can name
        failures += narrow == (last * lg::kStoredRowBytes + lg::kStoredRowBytes <= (u64{1} << 32)) ? 0 : 1;
        cases += 1;
        if (!narrow) continue;
        const u64 probe[] = {base, last, base + rows / 2, base + rng() % rows};
        for (u64 row : probe) {
          for (u32 i = 0; i < lg::kPieces; ++i) {
            for (u32 lane = 0; lane < lg::kLanes; lane += 9) {
              const u32 chunk = lg::piece_of(i, lane).chunk;
              const u64 want = row * sizeof(ed29_niels) + chunk * lg::kPieceBytes;
              failures += lg::piece_offset32(static_cast<u32>(row), chunk) == want ? 0 : 1;
              failures += want + lg::kPieceBytes <= (u64{1} << 32) ? 0 : 1; // the piece ends inside
              cases += 2;
            }
          }
        }
      }
    }
    std::printf("piece_offsets %lu %lu\n", failures, cases);
    bad += failures != 0;
  }
  return bad == 0 ? 0 : 1;
}
