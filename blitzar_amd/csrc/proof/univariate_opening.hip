// The field work of a HyperKZG opening between its MSM calls (bzamd_fold_polynomial*,
// bzamd_evaluate_polynomials*, bzamd_batch_quotients*), exact in both fields and enqueue-only in
// the device forms.  Sizes: l = num_variables, len_0 = n, len_i = ceil(len_{i-1} / 2); `folded`
// holds P_1 .. P_{l-1} back to back, P_i at row off_i (off_1 = 0, off_{i+1} = off_i + len_i).
//
// Arithmetic.  Every operation here is linear in the rows, so rows never take the engine's
// Montgomery form: a row is the raw residue of its 32 bytes (field 0: x, field 1: x 2^256), a
// challenge is E::load's x R, and the Montgomery product of the two is a raw residue again.  A row
// costs no product on the way in and none on the way out in element form (canonical bytes of the
// raw residue); scalar form is the same bytes in field 0 and one product by 2^-256 in field 1.
//
// Fold, k_fold_levels.  The pairs are adjacent, so a tile of kFoldTile = 2^10 consecutive rows of
// level s holds what levels s + 1 .. s + 10 need of it: 512, 256, .. 1 rows, row j of level s + d
// of tile T being row T 2^(10-d) + j of that level.  A lane loads four consecutive rows (128
// bytes) and makes two rows of the next level and one of the level after in registers; the 256
// rows of that level go to LDS and the other eight levels are halved there, 256 -> 128 -> .. -> 1.
// Rows past len_s are loaded as zero, and since len_{s+d} = ceil(len_s / 2^d) a row of level s + d
// is stored exactly when it is below len_{s+d}: the odd ends need nothing else.  Every row is
// stored once, element form and scalar form in the same pass, to its level's place.  Launch j
// reads level 10 j (P_0 from `polynomial`, the others from `folded`) and writes levels 10 j + 1 ..
// min(10 j + 10, l); level l is `evaluation`.  A call is ceil(l / 10) launches whatever n is; a
// launch is min(kFoldBlocks, tiles) workgroups that walk the tiles grid-stride, one workgroup once
// the level fits a tile.  P_0 is read once, levels 10, 20 are read once, everything else never.
//
// Evaluate, k_evaluate_partials and k_evaluate_finish.  The rows of all l levels are cut into
// chunks of C = kTileRows ceil(ceil(n / kTileRows) / kChunkBlocks) rows, level i into
// ceil(len_i / C) of them; one workgroup per chunk, at most 2 kChunkBlocks + l.  A workgroup walks
// its chunk's tiles of kTileRows = 1024 rows from the top: a lane runs Horner over kLaneRows = 4
// consecutive rows for each of the t points (the t accumulators in registers) and carries its own
// sum from tile to tile with u^1024; after the last tile the lanes are combined through LDS with
// u^(4 2^s), s = 0 .. 7, made once per workgroup.  The partial, sum_j P_i[start + j] u^j, goes to
// the workspace; the finish, one workgroup per level and point, multiplies partial c by u^(c C)
// and stores the l t sums.  Every row is read once for all points.
//
// Batch and divide.  B[m] = sum_i q^i P_i[m] is made on the fly, in launches (a) and (c), from the
// levels that reach row m (two on average), the q^i in LDS: 2 x (2 n + l) x 32 bytes read, t n x
// 32 written, against 3 n + 2 n + t n with B written to a workspace of n x 32 bytes.  With
// H(j) = sum_{m >= j} B[m] u^(m-j), h[j] = H(j + 1) and H(0) the remainder:
//   (a) k_quotient_sums: chunks of C rows of B as above (ceil(n / C) <= kChunkBlocks workgroups),
//       the chunk's own sum, by the code of k_evaluate_partials over another source of rows;
//   (b) k_quotient_carries: one workgroup, 256 chunks a pass from the top in a loop, a suffix scan
//       in LDS with u^(C 2^s): carry[c] = H(end of chunk c), and H(0) to `remainders`;
//   (c) k_quotients: a workgroup walks its chunk's tiles from the top; per tile the lanes' sums,
//       with the carry added to the top lane's, are scanned in LDS (u^(4 2^s)), which gives every
//       lane its own carry; the lane runs h[m] = H(m + 1), H(m) = B[m] + u H(m + 1) down its four
//       rows, which it kept in registers, and stores them in scalar form.
// Three launches whatever n is.  No kernel waits on another workgroup: what crosses workgroups
// crosses a launch.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; field 0 / field 1; no kernel
// uses scratch memory):
//                          VGPRs      LDS bytes   waves per SIMD
//   k_fold_levels          112 / 128   18984       4 / 4
//   k_evaluate_partials    201 / 186   10656       2 / 2
//   k_evaluate_finish       76 / 70     4608       6 / 7
//   k_quotient_sums        209 / 202   11736       2 / 2
//   k_quotient_carries      63 / 54     9540       7 / 7
//   k_quotients            178 / 171   39536       2 / 2
// The three wide kernels are bound by their field products, not by bytes; the
// "max-ilp" scheduling strategy was measured on this file and lost.
#include "blitzar_amd/csrc/proof/univariate_opening.h"

#include <cstring>
#include <type_traits>

#include "blitzar_amd/csrc/proof/host_call.h"
#include "blitzar_amd/csrc/proof/sumcheck_rows.h"

namespace bz::proof {
namespace {
constexpr u32 kFoldLevels = 10;
constexpr u32 kFoldTile = 1u << kFoldLevels;
constexpr u32 kFoldThreads = 256;
constexpr u32 kFoldBlocks = 1024; // 4 workgroups per CU

constexpr u32 kLaneRows = 4;
constexpr u32 kTileThreads = 256;
constexpr u32 kTileRows = kLaneRows * kTileThreads;
constexpr u32 kTileSteps = 8;      // log2(kTileThreads): the steps of a tree or scan over the lanes
constexpr u32 kChunkBlocks = 1024; // chunks of a level of n rows at most
constexpr u32 kCarryPass = 256;    // chunks one pass of k_quotient_carries scans

//--------------------------------------------------------------------------------------------------
// rows, shared by the host forms and the kernels
//--------------------------------------------------------------------------------------------------
// the raw residue of row i: normalised, V < 4
template <class F> BZ_HD typename F::fe raw_row(const u64* rows, u64 i) {
  u64 w[4];
#pragma unroll
  for (u32 k = 0; k < 4; ++k) w[k] = rows[4 * i + k];
  return F::reduce(F::from_words(w));
}
// element form of a raw residue (normalised): canonical
template <class F> BZ_HD void store_row(u64* rows, u64 i, const typename F::fe& v) {
  u64 w[4];
  F::to_words(w, F::canonical(v));
#pragma unroll
  for (u32 k = 0; k < 4; ++k) rows[4 * i + k] = w[k];
}
template <class F> BZ_HD void store_element(u8* bytes, const typename F::fe& v) {
  u64 w[4];
  F::to_words(w, F::canonical(v));
#pragma unroll
  for (u32 k = 0; k < 4; ++k) {
#pragma unroll
    for (u32 j = 0; j < 8; ++j) bytes[8 * k + j] = static_cast<u8>(w[k] >> (8 * j));
  }
}
// the raw residue of the plain integer: x 2^256 -> x is the product with 2^-256 R = 2^5 (field 1)
template <class E> BZ_HD typename E::F::fe scalar_of(const typename E::F::fe& v) {
  using F = typename E::F;
  if constexpr (std::is_same_v<E, grumpkin_elements>) {
    typename F::fe c = F::zero();
    c.v[0] = 1u << (F::LB * F::N - 256);
    return F::mul(v, c);
  } else {
    return v;
  }
}
// a + x (b - a): a, b raw (V < 4), x engine form
template <class F>
BZ_HD typename F::fe fold_pair(const typename F::fe& a, const typename F::fe& b,
                               const typename F::fe& x) {
  return fadd<F>(a, F::mul(x, fsub<F>(b, a)));
}
// base^e, engine form
template <class F> BZ_HD typename F::fe fpow(const typename F::fe& base, u64 e) {
  typename F::fe out = F::one(), b = base;
  for (; e != 0; e >>= 1) {
    if ((e & 1) != 0) out = F::mul(out, b);
    b = F::sqr(b);
  }
  return out;
}
// len_i and off_i (off_0 and off_1: 0)
struct level_place {
  u64 len, off;
};
BZ_HD level_place place_of(u64 n, u32 level) {
  level_place p{n, 0};
  for (u32 j = 1; j <= level; ++j) {
    if (j > 1) p.off += p.len;
    p.len = (p.len + 1) / 2;
  }
  return p;
}
// rows of a chunk (a multiple of kTileRows) and chunks of a level of `len` rows
BZ_HD u64 chunk_rows_of(u64 n) {
  const u64 tiles = (n + kTileRows - 1) / kTileRows;
  return kTileRows * ((tiles + kChunkBlocks - 1) / kChunkBlocks);
}
BZ_HD u64 chunks_of(u64 len, u64 chunk_rows) { return (len + chunk_rows - 1) / chunk_rows; }
// chunks of all levels 0 .. l - 1
u32 evaluate_chunks(u64 n, u32 num_variables) {
  const u64 chunk_rows = chunk_rows_of(n);
  u64 total = 0, len = n;
  for (u32 i = 0; i < num_variables; ++i) {
    total += chunks_of(len, chunk_rows);
    len = (len + 1) / 2;
  }
  return static_cast<u32>(total);
}

//--------------------------------------------------------------------------------------------------
// device kernels
//--------------------------------------------------------------------------------------------------
// one row of level first + d, row j of it, where it belongs (level l: the evaluation)
template <class E>
BZ_DEV void emit_folded(u64* folded, u64* scalars, u8* evaluation, u32 level, u32 num_variables,
                        u64 len, u64 off, u64 j, const typename E::F::fe& v) {
  using F = typename E::F;
  if (level == num_variables) {
    if (j == 0 && evaluation != nullptr) store_element<F>(evaluation, v);
    return;
  }
  if (j >= len) return;
  store_row<F>(folded, off + j, v);
  if (scalars != nullptr) store_row<F>(scalars, off + j, scalar_of<E>(v));
}

// levels first + 1 .. min(first + kFoldLevels, l) from level `first`
template <class E>
__global__ void __launch_bounds__(kFoldThreads)
    k_fold_levels(u64* folded, u64* scalars, u8* evaluation, const u64* polynomial,
                  const u8* __restrict__ point, u64 n, u32 num_variables, u32 first) {
  using F = typename E::F;
  using fe = typename F::fe;
  __shared__ fe xs[kFoldLevels];            // the challenge of level first + 1 + d
  __shared__ u64 lens[kFoldLevels + 1], offs[kFoldLevels + 1]; // of level first + d
  __shared__ fe halves[2][kFoldThreads];
  const u32 t = threadIdx.x;
  const u32 count = num_variables - first < kFoldLevels ? num_variables - first : kFoldLevels;
  if (t < count) xs[t] = E::load(point + 32 * (num_variables - (first + 1 + t)));
  if (t == 0) {
    level_place p = place_of(n, first);
    for (u32 d = 0; d <= count; ++d) {
      lens[d] = p.len;
      offs[d] = p.off;
      if (first + d >= 1) p.off += p.len;
      p.len = (p.len + 1) / 2;
    }
  }
  __syncthreads();
  const u64* source = first == 0 ? polynomial : folded + 4 * offs[0];
  const u64 source_len = lens[0];
  const u64 tiles = (source_len + kFoldTile - 1) / kFoldTile;
  for (u64 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const u64 base = tile * kFoldTile + 4 * t;
    fe a[4];
#pragma unroll
    for (u32 e = 0; e < 4; ++e) {
      a[e] = base + e < source_len ? raw_row<F>(source, base + e) : F::zero();
    }
    const fe b0 = fold_pair<F>(a[0], a[1], xs[0]);
    const fe b1 = fold_pair<F>(a[2], a[3], xs[0]);
    emit_folded<E>(folded, scalars, evaluation, first + 1, num_variables, lens[1], offs[1],
                   tile * (kFoldTile / 2) + 2 * t, b0);
    emit_folded<E>(folded, scalars, evaluation, first + 1, num_variables, lens[1], offs[1],
                   tile * (kFoldTile / 2) + 2 * t + 1, b1);
    if (count >= 2) {
      const fe c = fold_pair<F>(b0, b1, xs[1]);
      emit_folded<E>(folded, scalars, evaluation, first + 2, num_variables, lens[2], offs[2],
                     tile * (kFoldTile / 4) + t, c);
      halves[0][t] = c;
    }
    __syncthreads();
    u32 from = 0;
    for (u32 d = 3; d <= count; ++d) {
      const u32 width = kFoldTile >> d;
      if (t < width) {
        const fe v = fold_pair<F>(halves[from][2 * t], halves[from][2 * t + 1], xs[d - 1]);
        emit_folded<E>(folded, scalars, evaluation, first + d, num_variables, lens[d], offs[d],
                       tile * width + t, v);
        halves[from ^ 1][t] = v;
      }
      from ^= 1;
      __syncthreads();
    }
  }
}

// where a chunk's rows come from: row(m), zero past the end
template <class F> struct level_rows {
  const u64* rows;
  u64 len;
  BZ_DEV typename F::fe row(u64 m) const { return m < len ? raw_row<F>(rows, m) : F::zero(); }
};
// B[m] = sum_{i : m < len_i} q^i P_i[m]; qpow: q^i, engine form, in LDS
template <class F> struct batched_rows {
  const u64* polynomial;
  const u64* folded;
  u64 n;
  u32 num_variables;
  const typename F::fe* qpow;
  BZ_DEV typename F::fe row(u64 m) const {
    if (m >= n) return F::zero();
    typename F::fe acc = raw_row<F>(polynomial, m);
    u64 len = n, off = 0;
    for (u32 i = 1; i < num_variables; ++i) {
      if (i > 1) off += len;
      len = (len + 1) / 2;
      if (m >= len) break;
      acc = fadd<F>(acc, F::mul(qpow[i], raw_row<F>(folded, off + m)));
    }
    return acc;
  }
};

// the points of a call in LDS: us[k] = u_k and steps[k][s] = u_k^(kLaneRows 2^s), s <= kTileSteps
// (the last: u^kTileRows), engine form
template <class F> struct point_powers {
  typename F::fe us[kMaxOpeningPoints];
  typename F::fe steps[kMaxOpeningPoints][kTileSteps + 1];
};
template <class E>
BZ_DEV void load_point_powers(point_powers<typename E::F>& pp, const u8* points, u32 num_points) {
  using F = typename E::F;
  if (threadIdx.x < num_points) {
    const u32 k = threadIdx.x;
    const typename F::fe u = E::load(points + 32 * k);
    pp.us[k] = u;
    typename F::fe p = F::sqr(F::sqr(u));
    static_assert(kLaneRows == 4);
    for (u32 s = 0; s <= kTileSteps; ++s) {
      pp.steps[k][s] = p;
      p = F::sqr(p);
    }
  }
}
// fn(constant k) for k = 0 .. Count - 1, expanded at compile time: whatever fn indexes with k is
// indexed by a constant and stays in registers
template <class Fn, u32... K> BZ_HD void for_each_constant(std::integer_sequence<u32, K...>, Fn&& fn) {
  (fn(std::integral_constant<u32, K>{}), ...);
}
template <u32 Count, class Fn> BZ_HD void for_each_constant(Fn&& fn) {
  for_each_constant(std::make_integer_sequence<u32, Count>{}, fn);
}
template <class Fn> BZ_HD void for_each_point(Fn&& fn) { for_each_constant<kMaxOpeningPoints>(fn); }

// r[0] + r[1] u + r[2] u^2 + r[3] u^3
template <class F>
BZ_DEV typename F::fe lane_horner(const typename F::fe* r, const typename F::fe& u) {
  static_assert(kLaneRows == 4);
  typename F::fe acc = fadd<F>(F::mul(u, r[3]), r[2]);
  acc = fadd<F>(F::mul(u, acc), r[1]);
  return fadd<F>(F::mul(u, acc), r[0]);
}

// partials[k * stride] = sum_{begin <= m < end} src.row(m) u_k^(m - begin), k < num_points
template <class F, class Source>
BZ_DEV void chunk_sums(typename F::fe* partials, u64 stride, const Source& src, u64 begin, u64 end,
                       const point_powers<F>& pp, u32 num_points, typename F::fe* tree) {
  using fe = typename F::fe;
  const u32 t = threadIdx.x;
  fe acc[kMaxOpeningPoints];
  for_each_point([&](auto k) { acc[k] = F::zero(); });
  const u64 tiles = (end - begin + kTileRows - 1) / kTileRows;
  for (u64 tile = tiles; tile-- > 0;) {
    const u64 m0 = begin + tile * kTileRows + kLaneRows * t;
    fe r[kLaneRows];
    for_each_constant<kLaneRows>(
        [&](auto e) { r[e] = m0 + e < end ? src.row(m0 + e) : F::zero(); });
    for_each_point([&](auto k) {
      if (k < num_points) {
        acc[k] = fadd<F>(F::mul(pp.steps[k][kTileSteps], acc[k]), lane_horner<F>(r, pp.us[k]));
      }
    });
  }
  for_each_point([&](auto k) {
    if (k < num_points) {
      tree[t] = acc[k];
      __syncthreads();
      for (u32 s = 0; s < kTileSteps; ++s) {
        const u32 stride_lanes = 1u << s;
        if (t % (2 * stride_lanes) == 0) {
          tree[t] = fadd<F>(tree[t], F::mul(pp.steps[k][s], tree[t + stride_lanes]));
        }
        __syncthreads();
      }
      if (t == 0) partials[k * stride] = tree[0];
      __syncthreads();
    }
  });
}

// partials[k * gridDim.x + block]: the sum of the block's chunk, relative to the chunk's first row
template <class E>
__global__ void __launch_bounds__(kTileThreads)
    k_evaluate_partials(typename E::F::fe* __restrict__ partials, const u64* __restrict__ polynomial,
                        const u64* __restrict__ folded, u64 n, u32 num_variables,
                        const u8* __restrict__ points, u32 num_points, u64 chunk_rows) {
  using F = typename E::F;
  __shared__ point_powers<F> pp;
  __shared__ typename F::fe tree[kTileThreads];
  load_point_powers<E>(pp, points, num_points);
  __syncthreads();
  // the block's level and its chunk of it
  u64 chunk = blockIdx.x, len = n, off = 0;
  u32 level = 0;
  for (; level + 1 < num_variables; ++level) {
    const u64 chunks = chunks_of(len, chunk_rows);
    if (chunk < chunks) break;
    chunk -= chunks;
    if (level >= 1) off += len;
    len = (len + 1) / 2;
  }
  const level_rows<F> src{level == 0 ? polynomial : folded + 4 * off, len};
  const u64 begin = chunk * chunk_rows;
  const u64 end = begin + chunk_rows < len ? begin + chunk_rows : len;
  chunk_sums<F>(partials + blockIdx.x, gridDim.x, src, begin, end, pp, num_points, tree);
}

// evaluations[k * l + i] = sum_c partials[k][first chunk of level i + c] u_k^(c chunk_rows); one
// workgroup per level and point
template <class E>
__global__ void __launch_bounds__(kRoundThreads)
    k_evaluate_finish(u8* __restrict__ evaluations, const typename E::F::fe* __restrict__ partials,
                      u32 total_chunks, u64 n, u32 num_variables, const u8* __restrict__ points,
                      u64 chunk_rows) {
  using F = typename E::F;
  using fe = typename F::fe;
  __shared__ fe tree[kRoundThreads];
  const u32 level = blockIdx.x % num_variables, k = blockIdx.x / num_variables;
  u64 first = 0, len = n;
  for (u32 i = 0; i < level; ++i) {
    first += chunks_of(len, chunk_rows);
    len = (len + 1) / 2;
  }
  const u64 chunks = chunks_of(len, chunk_rows);
  const fe step = fpow<F>(E::load(points + 32 * k), chunk_rows);
  fe sum = F::zero();
  for (u64 c = threadIdx.x; c < chunks; c += kRoundThreads) {
    sum = fadd<F>(sum, F::mul(fpow<F>(step, c), partials[static_cast<u64>(k) * total_chunks + first + c]));
  }
  sum = block_sum<F>(tree, sum);
  if (threadIdx.x == 0) store_element<F>(evaluations + 32 * static_cast<u64>(blockIdx.x), sum);
}

// qpow[i] = q^i, i < l, engine form, by thread 0
template <class E>
BZ_DEV void load_q_powers(typename E::F::fe* qpow, const u8* q, u32 num_variables) {
  using F = typename E::F;
  if (threadIdx.x == 0) {
    const typename F::fe base = E::load(q);
    typename F::fe p = F::one();
    for (u32 i = 0; i < num_variables; ++i) {
      qpow[i] = p;
      p = F::mul(p, base);
    }
  }
}

// (a) sums[k * gridDim.x + chunk] = sum_{m in chunk} B[m] u_k^(m - chunk's first row)
template <class E>
__global__ void __launch_bounds__(kTileThreads)
    k_quotient_sums(typename E::F::fe* __restrict__ sums, const u64* __restrict__ polynomial,
                    const u64* __restrict__ folded, u64 n, u32 num_variables,
                    const u8* __restrict__ q, const u8* __restrict__ points, u32 num_points,
                    u64 chunk_rows) {
  using F = typename E::F;
  __shared__ point_powers<F> pp;
  __shared__ typename F::fe qpow[kMaxOpeningVariables];
  __shared__ typename F::fe tree[kTileThreads];
  load_point_powers<E>(pp, points, num_points);
  load_q_powers<E>(qpow, q, num_variables);
  __syncthreads();
  const batched_rows<F> src{polynomial, folded, n, num_variables, qpow};
  const u64 begin = blockIdx.x * chunk_rows;
  const u64 end = begin + chunk_rows < n ? begin + chunk_rows : n;
  chunk_sums<F>(sums + blockIdx.x, gridDim.x, src, begin, end, pp, num_points, tree);
}

// v[t] <- sum_{j >= t} v[j] base^(j - t) over the workgroup's kTileThreads entries; steps[s] =
// base^(2^s), s < kTileSteps.  Ends behind a barrier
template <class F> BZ_DEV void suffix_scan(typename F::fe* v, const typename F::fe* steps) {
  const u32 t = threadIdx.x;
  for (u32 s = 0; s < kTileSteps; ++s) {
    const u32 stride = 1u << s;
    typename F::fe add = F::zero();
    if (t + stride < kTileThreads) add = F::mul(steps[s], v[t + stride]);
    __syncthreads();
    v[t] = fadd<F>(v[t], add);
    __syncthreads();
  }
}

// (b) carries[k * chunks + c] = H_k(first row behind chunk c), and remainders[k] = H_k(0); one
// workgroup, kCarryPass chunks a pass from the top
template <class E>
__global__ void __launch_bounds__(kTileThreads)
    k_quotient_carries(typename E::F::fe* __restrict__ carries, u8* __restrict__ remainders,
                       const typename E::F::fe* __restrict__ sums, u32 chunks,
                       const u8* __restrict__ points, u32 num_points, u64 chunk_rows) {
  using F = typename E::F;
  using fe = typename F::fe;
  static_assert(kCarryPass == kTileThreads);
  __shared__ fe v[kTileThreads];
  __shared__ fe steps[kTileSteps]; // u^(chunk_rows 2^s)
  __shared__ fe running;           // H at the first row of the chunks done so far
  const u32 t = threadIdx.x;
  for (u32 k = 0; k < num_points; ++k) {
    if (t == 0) {
      fe p = fpow<F>(E::load(points + 32 * k), chunk_rows);
      for (u32 s = 0; s < kTileSteps; ++s) {
        steps[s] = p;
        p = F::sqr(p);
      }
      running = F::zero();
    }
    __syncthreads();
    const fe* mine = sums + static_cast<u64>(k) * chunks;
    fe* out = carries + static_cast<u64>(k) * chunks;
    for (u32 hi = chunks; hi > 0;) {
      const u32 count = hi < kCarryPass ? hi : kCarryPass;
      const u32 lo = hi - count;
      const fe above = running;
      fe own = t < count ? mine[lo + t] : F::zero();
      if (t == count - 1) own = fadd<F>(own, F::mul(steps[0], above));
      v[t] = own;
      __syncthreads();
      suffix_scan<F>(v, steps);
      if (t < count) {
        // (a conditional expression over `above` and the LDS entry would select between two
        // addresses and put `above` into scratch memory)
        fe behind = above;
        if (t + 1 < count) behind = v[t + 1];
        out[lo + t] = behind;
      }
      if (t == 0) running = v[0];
      __syncthreads();
      hi = lo;
    }
    if (t == 0 && remainders != nullptr) store_element<F>(remainders + 32 * k, running);
    __syncthreads();
  }
}

// (c) quotients[k * n + m] = H_k(m + 1), scalar form, for the rows of the block's chunk
template <class E>
__global__ void __launch_bounds__(kTileThreads)
    k_quotients(u64* __restrict__ quotients, const typename E::F::fe* __restrict__ carries,
                const u64* __restrict__ polynomial, const u64* __restrict__ folded, u64 n,
                u32 num_variables, const u8* __restrict__ q, const u8* __restrict__ points,
                u32 num_points, u64 chunk_rows) {
  using F = typename E::F;
  using fe = typename F::fe;
  __shared__ point_powers<F> pp;
  __shared__ fe qpow[kMaxOpeningVariables];
  __shared__ fe v[kMaxOpeningPoints][kTileThreads];
  __shared__ fe carry[kMaxOpeningPoints]; // H at the first row behind the tile
  const u32 t = threadIdx.x;
  load_point_powers<E>(pp, points, num_points);
  load_q_powers<E>(qpow, q, num_variables);
  if (t < num_points) carry[t] = carries[static_cast<u64>(t) * gridDim.x + blockIdx.x];
  __syncthreads();
  const batched_rows<F> src{polynomial, folded, n, num_variables, qpow};
  const u64 begin = blockIdx.x * chunk_rows;
  const u64 end = begin + chunk_rows < n ? begin + chunk_rows : n;
  const u64 tiles = (end - begin + kTileRows - 1) / kTileRows;
  for (u64 tile = tiles; tile-- > 0;) {
    const u64 m0 = begin + tile * kTileRows + kLaneRows * t;
    fe r[kLaneRows];
    for_each_constant<kLaneRows>(
        [&](auto e) { r[e] = m0 + e < end ? src.row(m0 + e) : F::zero(); });
    for_each_point([&](auto k) {
      if (k < num_points) {
        fe own = lane_horner<F>(r, pp.us[k]);
        if (t == kTileThreads - 1) own = fadd<F>(own, F::mul(pp.steps[k][0], carry[k]));
        v[k][t] = own;
      }
    });
    __syncthreads();
    // v[k][t] <- H_k(m0)
    for (u32 k = 0; k < num_points; ++k) suffix_scan<F>(v[k], pp.steps[k]);
    for_each_point([&](auto k) {
      if (k < num_points) {
        fe h = v[k][t == kTileThreads - 1 ? 0 : t + 1]; // H_k(m0 + kLaneRows)
        if (t == kTileThreads - 1) h = carry[k];
        u64* out = quotients + 4 * (static_cast<u64>(k) * n);
        for_each_constant<kLaneRows>([&](auto down) {
          constexpr u32 e = kLaneRows - 1 - down;
          if (m0 + e < end) store_row<F>(out, m0 + e, scalar_of<E>(h));
          h = fadd<F>(r[e], F::mul(pp.us[k], h));
        });
      }
    });
    __syncthreads();
    if (t < num_points) carry[t] = v[t][0];
    __syncthreads();
  }
}

//--------------------------------------------------------------------------------------------------
// checks
//--------------------------------------------------------------------------------------------------
void check_disjoint(std::initializer_list<byte_range> outputs,
                    std::initializer_list<byte_range> inputs) {
  for (const byte_range& out : outputs) {
    for (const byte_range& in : inputs) {
      BZ_RELEASE_ASSERT(!overlap(out, in), "an output overlaps an input of the same call");
    }
  }
}
bool aligned8(const void* p) { return reinterpret_cast<uintptr_t>(p) % 8 == 0; }

u64 folded_rows(u64 n, u32 num_variables) {
  const level_place last = place_of(n, num_variables - 1);
  return num_variables == 1 ? 0 : last.off + last.len;
}

void check_sizes(const univariate_opening& o) {
  BZ_RELEASE_ASSERT(o.num_variables >= 1 && o.num_variables <= kMaxOpeningVariables,
                    "a univariate opening needs 1 <= num_variables <= 30");
  BZ_RELEASE_ASSERT(o.n >= 1 && o.n <= (u64{1} << o.num_variables),
                    "a univariate opening needs 1 <= n <= 2^num_variables");
  BZ_RELEASE_ASSERT(o.polynomial != nullptr && o.points != nullptr &&
                        (o.folded != nullptr || o.num_variables == 1),
                    "null argument to a univariate opening");
  BZ_RELEASE_ASSERT(aligned8(o.polynomial) && aligned8(o.folded),
                    "the polynomials of a univariate opening must be 8-byte aligned");
}
void check_points(const univariate_opening& o) {
  BZ_RELEASE_ASSERT(o.num_points >= 1 && o.num_points <= kMaxOpeningPoints,
                    "a univariate opening needs 1 <= num_points <= 4");
}
bool sizes_supported(unsigned field_id, u64 n, u32 num_variables, u32 num_points) {
  return field_id <= 1 && num_variables >= 1 && num_variables <= kMaxOpeningVariables && n >= 1 &&
         n <= (u64{1} << num_variables) && num_points >= 1 && num_points <= kMaxOpeningPoints;
}

void check_fold(const void* scalars, const void* evaluation, const univariate_opening& o) {
  check_sizes(o);
  BZ_RELEASE_ASSERT(aligned8(scalars), "the scalars of a fold must be 8-byte aligned");
  const u64 rows = 32 * folded_rows(o.n, o.num_variables);
  check_disjoint({{o.folded, rows}, {scalars, rows}, {evaluation, 32}},
                 {{o.polynomial, 32 * o.n}, {o.points, u64{32} * o.num_variables}});
}
void check_evaluate(const void* evaluations, const univariate_opening& o, const void* workspace,
                    u64 workspace_bytes) {
  check_sizes(o);
  check_points(o);
  BZ_RELEASE_ASSERT(evaluations != nullptr, "null argument to a univariate opening");
  check_disjoint({{evaluations, u64{32} * o.num_variables * o.num_points},
                  {workspace, workspace_bytes}},
                 {{o.polynomial, 32 * o.n},
                  {o.folded, 32 * folded_rows(o.n, o.num_variables)},
                  {o.points, u64{32} * o.num_points}});
}
void check_quotients(const void* quotients, const void* remainders, const univariate_opening& o,
                     const void* q, const void* workspace, u64 workspace_bytes) {
  check_sizes(o);
  check_points(o);
  BZ_RELEASE_ASSERT(quotients != nullptr && q != nullptr, "null argument to a univariate opening");
  BZ_RELEASE_ASSERT(aligned8(quotients), "the quotients must be 8-byte aligned");
  check_disjoint({{quotients, 32 * o.n * o.num_points},
                  {remainders, u64{32} * o.num_points},
                  {workspace, workspace_bytes}},
                 {{o.polynomial, 32 * o.n},
                  {o.folded, 32 * folded_rows(o.n, o.num_variables)},
                  {o.points, u64{32} * o.num_points},
                  {q, 32}});
}

// the caller's workspaces
template <class F> struct evaluate_layout {
  size_t partials, total;
  u32 chunks;
  evaluate_layout(u64 n, u32 num_variables, u32 num_points) {
    workspace_carver carve;
    chunks = evaluate_chunks(n, num_variables);
    // what no smaller n needs more than: the chunks grow with n while a chunk is one tile
    const u32 room = n <= u64{kTileRows} * kChunkBlocks ? chunks : 2 * kChunkBlocks + num_variables + 1;
    partials = carve.take(sizeof(typename F::fe) * room * num_points);
    total = carve.total();
  }
};
template <class F> struct quotient_layout {
  size_t sums, carries, total;
  u32 chunks;
  quotient_layout(u64 n, u32 num_points) {
    workspace_carver carve;
    chunks = static_cast<u32>(chunks_of(n, chunk_rows_of(n)));
    // what no smaller n needs more than
    const u32 room = n <= u64{kTileRows} * kChunkBlocks ? chunks : kChunkBlocks;
    sums = carve.take(sizeof(typename F::fe) * room * num_points);
    carries = carve.take(sizeof(typename F::fe) * room * num_points);
    total = carve.total();
  }
};

//--------------------------------------------------------------------------------------------------
// host backend: plain loops over the same row arithmetic
//--------------------------------------------------------------------------------------------------
template <class E>
void fold_host(u64* folded, u64* scalars, u8* evaluation, const u64* polynomial, u64 n,
               const u8* point, u32 num_variables) {
  using F = typename E::F;
  using fe = typename F::fe;
  std::vector<fe> level(n);
  for (u64 j = 0; j < n; ++j) level[j] = raw_row<F>(polynomial, j);
  u64 off = 0;
  for (u32 i = 1; i <= num_variables; ++i) {
    const fe x = E::load(point + 32 * (num_variables - i));
    const u64 len = (level.size() + 1) / 2;
    std::vector<fe> next(len);
    for (u64 j = 0; j < len; ++j) {
      const fe high = 2 * j + 1 < level.size() ? level[2 * j + 1] : F::zero();
      next[j] = fold_pair<F>(level[2 * j], high, x);
    }
    if (i == num_variables) {
      if (evaluation != nullptr) store_element<F>(evaluation, next[0]);
      break;
    }
    for (u64 j = 0; j < len; ++j) {
      store_row<F>(folded, off + j, next[j]);
      if (scalars != nullptr) store_row<F>(scalars, off + j, scalar_of<E>(next[j]));
    }
    off += len;
    level.swap(next);
  }
}

// rows of level i: P_0 from o.polynomial, the others from o.folded
const u64* level_rows_of(const univariate_opening& o, u32 level, u64& len) {
  const level_place p = place_of(o.n, level);
  len = p.len;
  return level == 0 ? static_cast<const u64*>(o.polynomial)
                    : static_cast<const u64*>(o.folded) + 4 * p.off;
}

template <class E> void evaluate_host(u8* evaluations, const univariate_opening& o) {
  using F = typename E::F;
  using fe = typename F::fe;
  const u8* points = static_cast<const u8*>(o.points);
  for (u32 k = 0; k < o.num_points; ++k) {
    const fe u = E::load(points + 32 * k);
    for (u32 i = 0; i < o.num_variables; ++i) {
      u64 len;
      const u64* rows = level_rows_of(o, i, len);
      fe acc = F::zero();
      for (u64 j = len; j-- > 0;) acc = fadd<F>(F::mul(u, acc), raw_row<F>(rows, j));
      store_element<F>(evaluations + static_cast<size_t>(32) * (k * o.num_variables + i), acc);
    }
  }
}

template <class E>
void quotients_host(u64* quotients, u8* remainders, const univariate_opening& o, const u8* q) {
  using F = typename E::F;
  using fe = typename F::fe;
  std::vector<fe> batched(o.n, F::zero());
  const fe base = E::load(q);
  fe power = F::one();
  for (u32 i = 0; i < o.num_variables; ++i) {
    u64 len;
    const u64* rows = level_rows_of(o, i, len);
    for (u64 m = 0; m < len; ++m) {
      const fe row = raw_row<F>(rows, m);
      batched[m] = i == 0 ? row : fadd<F>(batched[m], F::mul(power, row));
    }
    power = F::mul(power, base);
  }
  const u8* points = static_cast<const u8*>(o.points);
  for (u32 k = 0; k < o.num_points; ++k) {
    const fe u = E::load(points + 32 * k);
    fe h = F::zero();
    for (u64 m = o.n; m-- > 0;) {
      store_row<F>(quotients + 4 * (static_cast<u64>(k) * o.n), m, scalar_of<E>(h));
      h = fadd<F>(batched[m], F::mul(u, h));
    }
    if (remainders != nullptr) store_element<F>(remainders + 32 * k, h);
  }
}

//--------------------------------------------------------------------------------------------------
// device forms: enqueue only
//--------------------------------------------------------------------------------------------------
// ceil(l / kFoldLevels) launches
template <class E>
void fold_enqueue(void* scalars, void* evaluation, const univariate_opening& o, hipStream_t stream) {
  for (u32 first = 0; first < o.num_variables; first += kFoldLevels) {
    const u64 len = place_of(o.n, first).len;
    const u64 tiles = (len + kFoldTile - 1) / kFoldTile;
    const u32 blocks = static_cast<u32>(std::min<u64>(kFoldBlocks, tiles));
    hipLaunchKernelGGL((k_fold_levels<E>), dim3(blocks), dim3(kFoldThreads), 0, stream,
                       static_cast<u64*>(o.folded), static_cast<u64*>(scalars),
                       static_cast<u8*>(evaluation), static_cast<const u64*>(o.polynomial),
                       static_cast<const u8*>(o.points), o.n, o.num_variables, first);
    BZ_HIP_CHECK(hipGetLastError());
    g_kernel_launches += 1;
  }
}

// two launches
template <class E>
void evaluate_enqueue(void* evaluations, const univariate_opening& o, void* workspace,
                      u64 workspace_bytes, hipStream_t stream) {
  using fe = typename E::F::fe;
  const evaluate_layout<typename E::F> layout{o.n, o.num_variables, o.num_points};
  BZ_RELEASE_ASSERT(workspace != nullptr && workspace_bytes >= layout.total,
                    "the polynomial evaluation workspace is too small");
  fe* d_partials = reinterpret_cast<fe*>(workspace_carver::aligned(workspace) + layout.partials);
  const u64 chunk_rows = chunk_rows_of(o.n);
  hipLaunchKernelGGL((k_evaluate_partials<E>), dim3(layout.chunks), dim3(kTileThreads), 0, stream,
                     d_partials, static_cast<const u64*>(o.polynomial),
                     static_cast<const u64*>(o.folded), o.n, o.num_variables,
                     static_cast<const u8*>(o.points), o.num_points, chunk_rows);
  BZ_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL((k_evaluate_finish<E>), dim3(o.num_variables * o.num_points),
                     dim3(kRoundThreads), 0, stream, static_cast<u8*>(evaluations), d_partials,
                     layout.chunks, o.n, o.num_variables, static_cast<const u8*>(o.points),
                     chunk_rows);
  BZ_HIP_CHECK(hipGetLastError());
  g_kernel_launches += 2;
}

// three launches
template <class E>
void quotients_enqueue(void* quotients, void* remainders, const univariate_opening& o,
                       const void* q, void* workspace, u64 workspace_bytes, hipStream_t stream) {
  using fe = typename E::F::fe;
  const quotient_layout<typename E::F> layout{o.n, o.num_points};
  BZ_RELEASE_ASSERT(workspace != nullptr && workspace_bytes >= layout.total,
                    "the quotient workspace is too small");
  u8* base = workspace_carver::aligned(workspace);
  fe* d_sums = reinterpret_cast<fe*>(base + layout.sums);
  fe* d_carries = reinterpret_cast<fe*>(base + layout.carries);
  const u64 chunk_rows = chunk_rows_of(o.n);
  const u64* polynomial = static_cast<const u64*>(o.polynomial);
  const u64* folded = static_cast<const u64*>(o.folded);
  const u8* points = static_cast<const u8*>(o.points);
  hipLaunchKernelGGL((k_quotient_sums<E>), dim3(layout.chunks), dim3(kTileThreads), 0, stream,
                     d_sums, polynomial, folded, o.n, o.num_variables, static_cast<const u8*>(q),
                     points, o.num_points, chunk_rows);
  BZ_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL((k_quotient_carries<E>), dim3(1), dim3(kTileThreads), 0, stream, d_carries,
                     static_cast<u8*>(remainders), d_sums, layout.chunks, points, o.num_points,
                     chunk_rows);
  BZ_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL((k_quotients<E>), dim3(layout.chunks), dim3(kTileThreads), 0, stream,
                     static_cast<u64*>(quotients), d_carries, polynomial, folded, o.n,
                     o.num_variables, static_cast<const u8*>(q), points, o.num_points, chunk_rows);
  BZ_HIP_CHECK(hipGetLastError());
  g_kernel_launches += 3;
}
} // namespace

std::vector<std::pair<u64, u64>> folded_layout(u64 n, u32 num_variables) {
  std::vector<std::pair<u64, u64>> out;
  for (u32 i = 1; i < num_variables; ++i) {
    const level_place p = place_of(n, i);
    out.emplace_back(p.off, p.len);
  }
  return out;
}

void fold_polynomial_device(void* scalars, void* evaluation, unsigned field_id,
                            const univariate_opening& o, hipStream_t stream) {
  check_fold(scalars, evaluation, o);
  with_elements(field_id, [&](auto elements) {
    fold_enqueue<decltype(elements)>(scalars, evaluation, o, stream);
  });
}

void fold_polynomial(api_state& st, void* scalars, void* evaluation, unsigned field_id,
                     const univariate_opening& o) {
  check_fold(scalars, evaluation, o);
  with_elements(field_id, [&](auto elements) {
    using E = decltype(elements);
    if (st.backend != 2) {
      fold_host<E>(static_cast<u64*>(o.folded), static_cast<u64*>(scalars),
                   static_cast<u8*>(evaluation), static_cast<const u64*>(o.polynomial), o.n,
                   static_cast<const u8*>(o.points), o.num_variables);
      return;
    }
    // the polynomial and the point up, the device form, the levels down
    host_call call{st};
    const size_t folded_bytes = static_cast<size_t>(32) * folded_rows(o.n, o.num_variables);
    univariate_opening on_device = o;
    void *d_scalars, *d_evaluation;
    call.input(&on_device.polynomial, o.polynomial, static_cast<size_t>(32) * o.n);
    call.output(&on_device.folded, o.folded, folded_bytes);
    call.input(&on_device.points, o.points, static_cast<size_t>(32) * o.num_variables);
    call.output(&d_scalars, scalars, folded_bytes);
    call.output(&d_evaluation, evaluation, 32);
    call.allocate();
    fold_enqueue<E>(d_scalars, d_evaluation, on_device, call.stream());
    call.finish();
  });
}

u64 evaluate_polynomials_workspace_bytes(unsigned field_id, u64 n, u32 num_variables,
                                         u32 num_points) {
  if (!sizes_supported(field_id, n, num_variables, num_points)) return 0;
  return with_elements(field_id, [&](auto elements) -> u64 {
    return evaluate_layout<typename decltype(elements)::F>{n, num_variables, num_points}.total;
  });
}

void check_evaluate_polynomials_device(const void* evaluations, unsigned field_id,
                                       const univariate_opening& o, const void* workspace,
                                       u64 workspace_bytes) {
  check_evaluate(evaluations, o, workspace, workspace_bytes);
  BZ_RELEASE_ASSERT(workspace != nullptr &&
                        workspace_bytes >= evaluate_polynomials_workspace_bytes(
                                               field_id, o.n, o.num_variables, o.num_points),
                    "the polynomial evaluation workspace is too small");
}

void evaluate_polynomials_device(void* evaluations, unsigned field_id, const univariate_opening& o,
                                 void* workspace, u64 workspace_bytes, hipStream_t stream) {
  check_evaluate_polynomials_device(evaluations, field_id, o, workspace, workspace_bytes);
  with_elements(field_id, [&](auto elements) {
    evaluate_enqueue<decltype(elements)>(evaluations, o, workspace, workspace_bytes, stream);
  });
}

void evaluate_polynomials(api_state& st, void* evaluations, unsigned field_id,
                          const univariate_opening& o) {
  check_evaluate(evaluations, o, nullptr, 0);
  with_elements(field_id, [&](auto elements) {
    using E = decltype(elements);
    if (st.backend != 2) {
      evaluate_host<E>(static_cast<u8*>(evaluations), o);
      return;
    }
    // the levels and the points up, the device form, the evaluations down
    host_call call{st};
    const size_t workspace_bytes =
        evaluate_layout<typename E::F>{o.n, o.num_variables, o.num_points}.total;
    univariate_opening on_device = o;
    void *d_evaluations, *d_workspace;
    call.input(&on_device.polynomial, o.polynomial, static_cast<size_t>(32) * o.n);
    call.input(&on_device.folded, o.folded,
               static_cast<size_t>(32) * folded_rows(o.n, o.num_variables));
    call.input(&on_device.points, o.points, static_cast<size_t>(32) * o.num_points);
    call.output(&d_evaluations, evaluations,
                static_cast<size_t>(32) * o.num_variables * o.num_points);
    call.scratch(&d_workspace, workspace_bytes);
    call.allocate();
    evaluate_enqueue<E>(d_evaluations, on_device, d_workspace, workspace_bytes, call.stream());
    call.finish();
  });
}

u64 batch_quotients_workspace_bytes(unsigned field_id, u64 n, u32 num_variables, u32 num_points) {
  if (!sizes_supported(field_id, n, num_variables, num_points)) return 0;
  return with_elements(field_id, [&](auto elements) -> u64 {
    return quotient_layout<typename decltype(elements)::F>{n, num_points}.total;
  });
}

void check_batch_quotients_device(const void* quotients, const void* remainders, unsigned field_id,
                                  const univariate_opening& o, const void* q,
                                  const void* workspace, u64 workspace_bytes) {
  check_quotients(quotients, remainders, o, q, workspace, workspace_bytes);
  BZ_RELEASE_ASSERT(workspace != nullptr &&
                        workspace_bytes >= batch_quotients_workspace_bytes(
                                               field_id, o.n, o.num_variables, o.num_points),
                    "the quotient workspace is too small");
}

void batch_quotients_device(void* quotients, void* remainders, unsigned field_id,
                            const univariate_opening& o, const void* q, void* workspace,
                            u64 workspace_bytes, hipStream_t stream) {
  check_batch_quotients_device(quotients, remainders, field_id, o, q, workspace, workspace_bytes);
  with_elements(field_id, [&](auto elements) {
    quotients_enqueue<decltype(elements)>(quotients, remainders, o, q, workspace, workspace_bytes,
                                          stream);
  });
}

void batch_quotients(api_state& st, void* quotients, void* remainders, unsigned field_id,
                     const univariate_opening& o, const void* q) {
  check_quotients(quotients, remainders, o, q, nullptr, 0);
  with_elements(field_id, [&](auto elements) {
    using E = decltype(elements);
    if (st.backend != 2) {
      quotients_host<E>(static_cast<u64*>(quotients), static_cast<u8*>(remainders), o,
                        static_cast<const u8*>(q));
      return;
    }
    // the levels, the points and q up, the device form, the quotients and remainders down
    host_call call{st};
    const size_t workspace_bytes = quotient_layout<typename E::F>{o.n, o.num_points}.total;
    univariate_opening on_device = o;
    void *d_quotients, *d_remainders, *d_q, *d_workspace;
    call.input(&on_device.polynomial, o.polynomial, static_cast<size_t>(32) * o.n);
    call.input(&on_device.folded, o.folded,
               static_cast<size_t>(32) * folded_rows(o.n, o.num_variables));
    call.input(&on_device.points, o.points, static_cast<size_t>(32) * o.num_points);
    call.output(&d_quotients, quotients, static_cast<size_t>(32) * o.n * o.num_points);
    call.output(&d_remainders, remainders, static_cast<size_t>(32) * o.num_points);
    call.input(&d_q, q, 32);
    call.scratch(&d_workspace, workspace_bytes);
    call.allocate();
    quotients_enqueue<E>(d_quotients, d_remainders, on_device, d_q, d_workspace, workspace_bytes,
                         call.stream());
    call.finish();
  });
}
} // namespace bz::proof
