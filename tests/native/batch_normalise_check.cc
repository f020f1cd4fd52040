// Stand-alone host check of the pieces the normalising caller-table kernel
// (k_prepare_addends_staged<ed25519_niels_msm, true>, blitzar_amd/csrc/msm/kernels.h) is made of and
// that compile for the host: the zero test of a loose coordinate, niels_of(X, Y, 1 / Z), and the
// levels of the shared-inversion tree with one() standing in for a zero leaf (msm/batch_tree.h).
// tests/test_batch_normalise_host.py builds and runs it (once more with
// -fsanitize=address,undefined) and reads the lines it prints:
//   <check> <failures> <cases>
// Exit status 0 when no check has a failure.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "blitzar_amd/csrc/msm/batch_tree.h"
#include "blitzar_amd/csrc/msm/curve_traits.h"

using namespace bz;
using C = ed25519_niels_msm;

static fe51 limbs51(const u64 (&v)[5]) {
  fe51 f;
  for (int i = 0; i < 5; ++i) f.v[i] = v[i];
  return f;
}
// k p + delta (k = 0, 1, 2; delta = -1, 0, 1) in 5 limbs of 51 bits, the top ones loose
static fe51 multiple_of_p(int k, int delta) {
  const u64 m = (u64{1} << 51) - 1;
  u64 v[5] = {0, 0, 0, 0, 0};
  if (k >= 1) {
    const u64 p[5] = {m - 18, m, m, m, m};
    for (int i = 0; i < 5; ++i) v[i] = static_cast<u64>(k) * p[i]; // limb-wise: below 2^52
  }
  if (delta > 0) v[0] += 1;
  if (delta < 0) {
    if (k == 0) { // -1 = p - 1
      const u64 p[5] = {m - 19, m, m, m, m};
      for (int i = 0; i < 5; ++i) v[i] = p[i];
    } else {
      v[0] -= 1;
    }
  }
  return limbs51(v);
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

int main() {
  int bad = 0;
  std::mt19937_64 rng(0x2e10ca11);

  // 1. zero mod p in every encoding loose limbs allow; its neighbours are not
  {
    unsigned long failures = 0, cases = 0;
    for (int k = 0; k <= 2; ++k) {
      for (int delta = -1; delta <= 1; ++delta) {
        const fe29 z = f29::from_fe51(multiple_of_p(k, delta));
        failures += C::batch_is_zero(z) != (delta == 0) ? 1 : 0;
        // what the kernel's leaf makes of it
        const fe29 leaf = tree_leaf<C>(z, true);
        failures += same_value(leaf, delta == 0 ? f29::one() : z) ? 0 : 1;
        cases += 1;
      }
    }
    const fe29 z = random_fe(rng);
    failures += same_value(tree_leaf<C>(z, false), f29::one()) ? 0 : 1; // a lane without a row
    cases += 1;
    std::printf("zero_test %lu %lu\n", failures, cases);
    bad += failures != 0;
  }

  // 2. niels_of(X, Y, 1 / Z) is to_niels of the point, and does not depend on Z
  {
    unsigned long failures = 0, cases = 0;
    // the ristretto255 base point (RFC 9496, A.1)
    const u8 base[32] = {0xe2, 0xf2, 0xae, 0x0a, 0x6a, 0xbc, 0x4e, 0x71, 0xa8, 0x84, 0xa9,
                         0x61, 0xc5, 0x00, 0x51, 0x5f, 0x58, 0xe3, 0x0b, 0x6a, 0xa5, 0x82,
                         0xdd, 0x8d, 0xb6, 0xa6, 0x59, 0x45, 0xe0, 0x8d, 0x2d, 0x76};
    ed_point decoded;
    if (!ristretto29::decode(decoded, base)) return 2;
    ed29_point p = ed29::from_ed(decoded);
    for (int i = 0; i < 2000; ++i) {
      p = ed29::add(p, ed29::dbl_n(p, 1 + i % 3)); // some other point of the group
      fe29 lambda = random_fe(rng);
      if (f29::is_zero(lambda)) lambda = f29::one();
      const fe29 big_x = f29::mul(p.X, lambda), big_y = f29::mul(p.Y, lambda);
      const fe29 big_z = f29::mul(p.Z, lambda);
      const ed29_niels got = C::niels_of(big_x, big_y, f29::invert(big_z));
      const ed29_niels want = ed29::to_niels(p);
      const bool ok = same_value(got.YpX, want.YpX) && same_value(got.YmX, want.YmX) &&
                      same_value(got.T2d, want.T2d);
      bool pad = true;
      for (int k = 0; k < 5; ++k) pad = pad && got.pad[k] == 0;
      failures += ok && pad ? 0 : 1;
      cases += 1;
    }
    std::printf("niels_of %lu %lu\n", failures, cases);
    bad += failures != 0;
  }

  // 3. the tree over 256 leaves, level by level as the kernel walks it, zeros at positions 0, 63,
  //    64 and 255: every other leaf gets its own inverse, the zero leaves get 1
  {
    constexpr u32 T = 256;
    unsigned long failures = 0, cases = 0;
    std::vector<fe29> z(T), tree(2 * T);
    for (fe29& v : z) {
      v = random_fe(rng);
      if (f29::is_zero(v)) v = f29::one();
    }
    z[0] = f29::from_fe51(multiple_of_p(0, 0));
    z[63] = f29::from_fe51(multiple_of_p(1, 0));
    z[64] = f29::from_fe51(multiple_of_p(2, 0));
    z[255] = f29::from_fe51(multiple_of_p(1, 0));
    for (u32 tid = 0; tid < T; ++tid) tree[T + tid] = tree_leaf<C>(z[tid], true);
    for (u32 s = T / 2; s >= 1; s >>= 1) {
      // (a level reads only the level below it: the lanes may run in any order, here descending)
      for (u32 tid = T; tid-- > 0;) tree_product_step<C>(tree.data(), s, tid);
    }
    failures += f29::is_zero(tree[1]) ? 1 : 0; // the product the zeros must not reach
    cases += 1;
    tree[1] = f29::invert(tree[1]);
    for (u32 s = 1; s < T; s <<= 1) {
      for (u32 tid = T; tid-- > 0;) tree_inverse_step<C>(tree.data(), s, tid);
    }
    for (u32 tid = 0; tid < T; ++tid) {
      const bool zero = tid == 0 || tid == 63 || tid == 64 || tid == 255;
      const fe29 prod = f29::mul(tree[T + tid], zero ? f29::one() : z[tid]);
      failures += same_value(prod, f29::one()) ? 0 : 1;
      cases += 1;
    }
    std::printf("tree_with_zero_leaves %lu %lu\n", failures, cases);
    bad += failures != 0;
  }
  return bad == 0 ? 0 : 1;
}
