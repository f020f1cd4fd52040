// Test-only device hooks: the product's field / curve headers, unchanged, wrapped in gfx950 kernels
// so that tests/test_device_arith.py can run single primitives on the GPU -- the lane-spread
// arithmetic of curve/ed16_wave.h, curve/sw_wave.h and curve/sw29_coop.h, which has no host build,
// and the device compile of the headers tests/native/hooks.cpp covers on the host.
//
// This file is compiled once per (unit, flag set) by tests/device_hooks.py with the flags of the
// product translation unit that instantiates the code (blitzar_amd/build.py FLAGS + TU_FLAGS):
//     -DBZ_DH_TAG=<name>      namespace of the object and suffix of its entry point bz_dh_run_<name>
//     -DBZ_DH_ED=1            curve25519: f29 / ed29 per-lane ops, ed16w and the ed25519_msm wave ops
//     -DBZ_DH_SW=<msm trait> -DBZ_DH_G=<sw29 curve>   a Weierstrass curve: mont29 / sw29 per-lane ops
//     -DBZ_DH_ED_WAVE=1 / -DBZ_DH_SW_WAVE=1   also the wave ops (ed16w, sww::wave, add_coop4, the traits'
//                             wave members), in the object built like the TU that instantiates them
//     -DBZ_DH_SW_BLS=1        bls12-381: the define its product translation units set
//     -DBZ_DH_PROOF=1         the proof kernels' pieces: the wavefront's Keccak / Merlin of
//                             proof/transcript.h, the scalar arithmetic of proof/scalar25.h and the element
//                             conversions of proof/sumcheck_rows.h as the kernels use them, and the protocol
//                             steps of proof/sumcheck_protocol.h and proof/inner_product_protocol.h
// and the objects are linked into tests/native/_build/libbz_device_hooks.so.  Not part of
// libblitzar_amd.so.
//
// Entry point:  int bz_dh_run_<tag>(op, in, in_words, out, out_words, cases, params[4])
// with host pointers; it allocates, copies, launches, synchronises and returns the HIP status
// (negative: -1 unknown op, -2 sizes do not match the op's record layout, -3 parameters out of range).
// Every case is one fixed-size record of 32-bit words; record sizes depend on the op and on the
// validated `params` only, never on the data, and no kernel forms an address from input data: the
// few record fields that index memory (a transcript's position, fold digits and their count) are
// checked on the host before the launch (-3) and clamped in the kernel.
//   per-lane ops: one case per thread, blocks of 64
//   wave ops:     one case per 64-thread workgroup, with the product's wave_scratch()
#if defined(BZ_DH_SW_BLS)
#define BZ_MONT29_MAD_MODE 1 // as msm_bls12_381.hip / msm_bls12_381_accumulate.hip
#endif
#include <hip/hip_runtime.h>

#include <cstring>

#include "blitzar_amd/csrc/msm/curve_traits.h"
#if defined(BZ_DH_PROOF)
#include "blitzar_amd/csrc/proof/inner_product_protocol.h"
#include "blitzar_amd/csrc/proof/scalar25.h"
#include "blitzar_amd/csrc/proof/sumcheck_protocol.h"
#include "blitzar_amd/csrc/proof/sumcheck_rows.h"
#include "blitzar_amd/csrc/proof/transcript.h"
#endif

#define BZ_DH_CAT2(a, b) a##b
#define BZ_DH_CAT(a, b) BZ_DH_CAT2(a, b)

namespace bz {
namespace BZ_DH_CAT(dh_, BZ_DH_TAG) {

constexpr u32 kMaxWindows = 17;   // window sums of a Horner chain / slices of a wave_chain
constexpr u32 kMaxWindowBits = 16;
constexpr u32 kMaxChain = 512;    // steps of a fed-back chain
constexpr u32 kMaxCases = 4096;

struct params4 {
  u32 v[4];
};

template <class T> __device__ __forceinline__ T load_as(const u32* in) {
  static_assert(sizeof(T) % 4 == 0);
  T t;
  u32* w = reinterpret_cast<u32*>(&t);
  for (u32 i = 0; i < sizeof(T) / 4; ++i) w[i] = in[i];
  return t;
}
template <class T> __device__ __forceinline__ void store_as(u32* out, const T& t) {
  static_assert(sizeof(T) % 4 == 0);
  const u32* w = reinterpret_cast<const u32*>(&t);
  for (u32 i = 0; i < sizeof(T) / 4; ++i) out[i] = w[i];
}
template <class T> constexpr u32 words_of() { return sizeof(T) / 4; }

template <class Op>
__global__ void __launch_bounds__(64) k_lane(const u32* in, u32* out, u32 cases, params4 pr) {
  const u32 t = blockIdx.x * 64 + threadIdx.x;
  if (t >= cases) return;
  Op::run(in + static_cast<size_t>(t) * Op::in_words(pr), out + static_cast<size_t>(t) * Op::out_words(pr),
          pr);
}
// grid = cases
template <class Op> __global__ void __launch_bounds__(64) k_wave(const u32* in, u32* out, params4 pr) {
  const u32 b = blockIdx.x;
  Op::run(in + static_cast<size_t>(b) * Op::in_words(pr), out + static_cast<size_t>(b) * Op::out_words(pr),
          pr);
}

// valid_records: the record fields a kernel indexes memory with, checked before the launch
struct op_base {
  static constexpr bool wave = false;
  static bool valid(const params4&) { return true; }
  static bool valid_records(const u32*, u32, const params4&) { return true; }
};
struct wave_op_base {
  static constexpr bool wave = true;
  static bool valid(const params4&) { return true; }
  static bool valid_records(const u32*, u32, const params4&) { return true; }
};
#define BZ_DH_IO(IN, OUT)                                                                          \
  __host__ __device__ static constexpr u32 in_words(const params4&) { return IN; }                 \
  __host__ __device__ static constexpr u32 out_words(const params4&) { return OUT; }

#if defined(BZ_DH_ED)
//--------------------------------------------------------------------------------------------------
// f29 / ed29, one case per lane (twins of tests/native/hooks.cpp)
//--------------------------------------------------------------------------------------------------
constexpr u32 kFe = 9, kEd = 40 /* ed_point: 4 x 5 x u64 */, kP29 = 36 /* ed29_point */;

struct f29_mul : op_base {
  BZ_DH_IO(18, 9)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    store_as(out, f29::mul(load_as<fe29>(in), load_as<fe29>(in + 9)));
  }
};
struct f29_sq : op_base {
  BZ_DH_IO(9, 9)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    store_as(out, f29::sq(load_as<fe29>(in)));
  }
};
struct f29_sub : op_base {
  BZ_DH_IO(18, 9)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    store_as(out, f29::sub(load_as<fe29>(in), load_as<fe29>(in + 9)));
  }
};
struct f29_weak_reduce : op_base {
  BZ_DH_IO(9, 9)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    store_as(out, f29::weak_reduce(load_as<fe29>(in)));
  }
};
struct f29_invert : op_base {
  BZ_DH_IO(9, 9)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    store_as(out, f29::invert(load_as<fe29>(in)));
  }
};
struct f29_pow22523 : op_base {
  BZ_DH_IO(9, 9)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    store_as(out, f29::pow22523(load_as<fe29>(in)));
  }
};
struct f29_from_fe51 : op_base {
  BZ_DH_IO(10, 9)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    store_as(out, f29::from_fe51(load_as<fe51>(in)));
  }
};
struct f29_to_words : op_base {
  BZ_DH_IO(9, 8)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    u64 w[4];
    f29::to_words(w, load_as<fe29>(in));
    for (int i = 0; i < 4; ++i) out[2 * i] = static_cast<u32>(w[i]), out[2 * i + 1] = static_cast<u32>(w[i] >> 32);
  }
};
struct f29_pack_words : op_base {
  BZ_DH_IO(9, 8)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    u32 w[8];
    ed29::pack_words(w, load_as<fe29>(in));
    for (int i = 0; i < 8; ++i) out[i] = w[i];
  }
};
struct f29_unpack_words : op_base {
  BZ_DH_IO(8, 9)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    u32 w[8];
    for (int i = 0; i < 8; ++i) w[i] = in[i];
    store_as(out, ed29::unpack_words(w));
  }
};
// record: a, b (ed_point), negate
struct ed29_add : op_base {
  BZ_DH_IO(2 * kEd + 1, kEd)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    const ed29_point r = ed29::add_cached(ed29::from_ed(load_as<ed_point>(in)),
                                          ed29::cached_from_ed(load_as<ed_point>(in + kEd)), in[2 * kEd] != 0);
    store_as(out, ed29::to_ed(r));
  }
};
struct ed29_add_general : op_base {
  BZ_DH_IO(2 * kEd, kEd)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    store_as(out, ed29::to_ed(ed29::add(ed29::from_ed(load_as<ed_point>(in)),
                                        ed29::from_ed(load_as<ed_point>(in + kEd)))));
  }
};
struct ed29_add_gathered : op_base {
  BZ_DH_IO(2 * kEd + 1, kEd)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    const bool negate = in[2 * kEd] != 0;
    const ed29_cached_packed row[1] = {ed29::pack(ed29::cached_from_ed(load_as<ed_point>(in + kEd)))};
    const ed29_cached_packed g = ed29::gather_signed(row, 0, negate);
    store_as(out, ed29::to_ed(ed29::add_cached_presigned(ed29::from_ed(load_as<ed_point>(in)),
                                                         ed29::unpack(g), negate)));
  }
};
// record: a (ed_point), k
struct ed29_dbl_n : op_base {
  BZ_DH_IO(kEd + 1, kEd)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    const u32 k = in[kEd] > 64 ? 64 : in[kEd];
    store_as(out, ed29::to_ed(ed29::dbl_n(ed29::from_ed(load_as<ed_point>(in)), static_cast<int>(k))));
  }
};
// params: {n, form}; record: n x (ed_point, negate).  form 0: add_cached chain, 1: add_niels chain,
// 2 / 3: the first entry loaded (from_cached_presigned / from_niels), the others added
struct ed29_chain : op_base {
#if defined(BZ_DH_ED_NIELS)
  static bool valid(const params4& p) { return p.v[0] >= 1 && p.v[0] <= 64 && (p.v[1] == 1 || p.v[1] == 3); }
#else
  static bool valid(const params4& p) { return p.v[0] >= 1 && p.v[0] <= 64 && p.v[1] <= 3; }
#endif
  __host__ __device__ static constexpr u32 in_words(const params4& p) { return p.v[0] * (kEd + 1); }
  __host__ __device__ static constexpr u32 out_words(const params4&) { return kEd; }
  __device__ static void run(const u32* in, u32* out, const params4& pr) {
    const u32 n = pr.v[0] > 64 ? 64 : pr.v[0], form = pr.v[1];
    ed29_point acc = ed29::identity();
    for (u32 i = 0; i < n; ++i) {
      const ed_point q = load_as<ed_point>(in + i * (kEd + 1));
      const bool neg = in[i * (kEd + 1) + kEd] != 0;
      if (form == 1) {
        acc = ed29::add_niels(acc, ed29::to_niels(ed29::from_ed(q)), neg);
      } else if (form == 3) {
        const ed29_niels row = ed29::to_niels(ed29::from_ed(q));
        acc = i == 0 ? ed29::from_niels(row, neg) : ed29::add_niels(acc, row, neg);
      }
#if !defined(BZ_DH_ED_NIELS)
      else if (form == 0) {
        acc = ed29::add_cached(acc, ed29::cached_from_ed(q), neg);
      } else {
        const ed29_cached_packed row[1] = {ed29::pack(ed29::cached_from_ed(q))};
        const ed29_cached g = ed29::unpack(ed29::gather_signed(row, 0, neg));
        acc = i == 0 ? ed29::from_cached_presigned(g, neg) : ed29::add_cached_presigned(acc, g, neg);
      }
#endif
    }
    store_as(out, ed29::to_ed(acc));
  }
};
struct ed29_ristretto_encode : op_base {
  BZ_DH_IO(kEd, 8)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    u64 w[4];
    ristretto29::encode_words(w, ed29::from_ed(load_as<ed_point>(in)));
    for (int i = 0; i < 4; ++i) out[2 * i] = static_cast<u32>(w[i]), out[2 * i + 1] = static_cast<u32>(w[i] >> 32);
  }
};

#if defined(BZ_DH_ED_WAVE)
//--------------------------------------------------------------------------------------------------
// ed16w and the wave members of ed25519_msm, one case per workgroup of 64
//--------------------------------------------------------------------------------------------------
// every lane holds the point; lane 0 writes it
__device__ __forceinline__ void put_point(u32* out, const ed29_point& p) {
  if ((threadIdx.x & 63) == 0) store_as(out, p);
}
// record: u lane words, v lane words -> product lane words
struct ed16w_fmul : wave_op_base {
  BZ_DH_IO(128, 64)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    const ed16w::lane_ctx c = ed16w::make_ctx(ed16w::wave_scratch());
    out[c.lane] = ed16w::fmul(c, in[c.lane], in[64 + c.lane]);
  }
};
// record: state lane words -> state lane words, store_point of them
struct ed16w_dbl : wave_op_base {
  BZ_DH_IO(64, 64 + kP29)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    const ed16w::lane_ctx c = ed16w::make_ctx(ed16w::wave_scratch());
    const u32 st = ed16w::dbl(c, in[c.lane]);
    out[c.lane] = st;
    put_point(out + 64, ed16w::store_point(c, st));
  }
};
struct ed16w_add_cached : wave_op_base {
  BZ_DH_IO(128, 64 + kP29)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    const ed16w::lane_ctx c = ed16w::make_ctx(ed16w::wave_scratch());
    const u32 st = ed16w::add_cached(c, in[c.lane], in[64 + c.lane]);
    out[c.lane] = st;
    put_point(out + 64, ed16w::store_point(c, st));
  }
};
// params: {n}; record: state, cached; step k: add_cached when k is a multiple of 3, else dbl; the raw
// state is fed back
struct ed16w_chain : wave_op_base {
  static bool valid(const params4& p) { return p.v[0] <= kMaxChain; }
  BZ_DH_IO(128, 64 + kP29)
  __device__ static void run(const u32* in, u32* out, const params4& pr) {
    const ed16w::lane_ctx c = ed16w::make_ctx(ed16w::wave_scratch());
    const u32 n = pr.v[0] > kMaxChain ? kMaxChain : pr.v[0];
    u32 st = in[c.lane];
    const u32 q = in[64 + c.lane];
#pragma unroll 1
    for (u32 k = 0; k < n; ++k) st = (k % 3 == 0) ? ed16w::add_cached(c, st, q) : ed16w::dbl(c, st);
    out[c.lane] = st;
    put_point(out + 64, ed16w::store_point(c, st));
  }
};
// record: ed29_point -> load_point lane words, store_point of them
struct ed16w_roundtrip : wave_op_base {
  BZ_DH_IO(kP29, 64 + kP29)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    const ed16w::lane_ctx c = ed16w::make_ctx(ed16w::wave_scratch());
    const u32 st = ed16w::load_point(c, load_as<ed29_point>(in));
    out[c.lane] = st;
    put_point(out + 64, ed16w::store_point(c, st));
  }
};
// record: raw lane words -> store_point (gather_row of each row)
struct ed16w_gather : wave_op_base {
  BZ_DH_IO(64, kP29)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    const ed16w::lane_ctx c = ed16w::make_ctx(ed16w::wave_scratch());
    put_point(out, ed16w::store_point(c, in[c.lane]));
  }
};
struct ed16w_pow22523 : wave_op_base {
  BZ_DH_IO(kFe, kFe)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    const ed16w::lane_ctx c = ed16w::make_ctx(ed16w::wave_scratch());
    const fe29 r = ed16w::pow22523(c, load_as<fe29>(in));
    if (c.lane == 0) store_as(out, r);
  }
};
struct ed_batch_wave_invert : wave_op_base {
  BZ_DH_IO(kFe, kFe)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    const fe29 r = ed25519_msm::batch_wave_invert(load_as<fe29>(in));
    if ((threadIdx.x & 63) == 0) store_as(out, r);
  }
};
struct ed_wave_encode : wave_op_base {
  BZ_DH_IO(kP29, 8)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    ed25519_msm::wave_encode(reinterpret_cast<u8*>(out), load_as<ed29_point>(in));
  }
};
// params: {num_windows, window_bits, have_acc}; record: acc, num_windows window sums (ed29_point)
struct ed_wave_horner : wave_op_base {
  static bool valid(const params4& p) {
    return p.v[0] >= 1 && p.v[0] <= kMaxWindows && p.v[1] >= 1 && p.v[1] <= kMaxWindowBits && p.v[2] <= 1;
  }
  __host__ __device__ static constexpr u32 in_words(const params4& p) { return (1 + p.v[0]) * kP29; }
  __host__ __device__ static constexpr u32 out_words(const params4&) { return kP29; }
  __device__ static void run(const u32* in, u32* out, const params4& pr) {
    __shared__ alignas(16) ed29_point sums[kMaxWindows]; // (slots are rewritten as 16-byte aligned rows)
    const u32 nw = pr.v[0] > kMaxWindows ? kMaxWindows : pr.v[0];
    const u32 bits = pr.v[1] > kMaxWindowBits ? kMaxWindowBits : pr.v[1];
    for (u32 w = threadIdx.x; w < nw; w += 64) sums[w] = load_as<ed29_point>(in + (1 + w) * kP29);
    __syncthreads();
    put_point(out, ed25519_msm::wave_horner(load_as<ed29_point>(in), pr.v[2] != 0, sums, 1, nw, bits));
  }
};
// record: v, s (ed29_point), m (non-zero: the contract of wave_add_multiple)
struct ed_wave_add_multiple : wave_op_base {
  BZ_DH_IO(2 * kP29 + 1, kP29)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    const u32 m = in[2 * kP29] == 0 ? 1u : in[2 * kP29];
    put_point(out, ed25519_msm::wave_add_multiple(load_as<ed29_point>(in), load_as<ed29_point>(in + kP29), m));
  }
};
// params: {windows, bits}; record: g -> windows points
struct ed_wave_chain : wave_op_base {
  static bool valid(const params4& p) {
    return p.v[0] >= 1 && p.v[0] <= kMaxWindows && p.v[1] >= 1 && p.v[1] <= kMaxWindowBits;
  }
  __host__ __device__ static constexpr u32 in_words(const params4&) { return kP29; }
  __host__ __device__ static constexpr u32 out_words(const params4& p) { return p.v[0] * kP29; }
  __device__ static void run(const u32* in, u32* out, const params4& pr) {
    const u32 nw = pr.v[0] > kMaxWindows ? kMaxWindows : pr.v[0];
    const u32 bits = pr.v[1] > kMaxWindowBits ? kMaxWindowBits : pr.v[1];
    ed25519_msm::wave_chain(reinterpret_cast<ed29_point*>(out), 1, load_as<ed29_point>(in), nw, bits);
  }
};
#endif // BZ_DH_ED_WAVE

#define BZ_DH_OPS_F29(X)                                                                           \
  X(f29_mul) X(f29_sq) X(f29_sub) X(f29_weak_reduce) X(f29_invert) X(f29_pow22523) X(f29_from_fe51) \
  X(f29_to_words) X(f29_pack_words) X(f29_unpack_words)
#define BZ_DH_OPS_ED_LANE(X)                                                                       \
  BZ_DH_OPS_F29(X)                                                                                 \
  X(ed29_add) X(ed29_add_general) X(ed29_add_gathered) X(ed29_dbl_n) X(ed29_chain) X(ed29_ristretto_encode)
#if defined(BZ_DH_ED_NIELS)
// the object built like msm_curve25519_niels_accumulate.hip holds what that translation unit
// instantiates: the field and the Z = 1 addition forms (ed29_chain forms 1 and 3)
#define BZ_DH_OPS(X) BZ_DH_OPS_F29(X) X(ed29_chain)
#elif defined(BZ_DH_ED_WAVE)
#define BZ_DH_OPS(X)                                                                               \
  BZ_DH_OPS_ED_LANE(X)                                                                             \
  X(ed16w_fmul) X(ed16w_dbl) X(ed16w_add_cached) X(ed16w_chain) X(ed16w_roundtrip) X(ed16w_gather) \
  X(ed16w_pow22523) X(ed_batch_wave_invert) X(ed_wave_encode) X(ed_wave_horner)                    \
  X(ed_wave_add_multiple) X(ed_wave_chain)
#else
#define BZ_DH_OPS(X) BZ_DH_OPS_ED_LANE(X)
#endif
#endif // BZ_DH_ED

#if defined(BZ_DH_SW)
//--------------------------------------------------------------------------------------------------
// mont29 / sw29, one case per lane.  ABI-form ops are twins of tests/native/hooks.cpp; raw ops take
// and return the N limbs of the engine's form so that loose operands can be injected
//--------------------------------------------------------------------------------------------------
using C = BZ_DH_SW;
using G = BZ_DH_G;
using F = G::F;
using fe = F::fe;
using point = G::point;
using point64 = G::G64::point;
constexpr u32 kN = F::N, kW64 = 2 * F::N64 /* words of an ABI-form element */, kPt = 3 * kN, kPt64 = 3 * kW64;

__device__ __forceinline__ bool same_limbs(const fe& a, const fe& b) {
  u32 d = 0;
  for (u32 i = 0; i < kN; ++i) d |= a.v[i] ^ b.v[i];
  return d == 0;
}
__device__ __forceinline__ bool same_limbs(const point& a, const point& b) {
  return same_limbs(a.X, b.X) && same_limbs(a.Y, b.Y) && same_limbs(a.Z, b.Z);
}
__device__ __forceinline__ fe from_m64(const u32* in) {
  u64 w[F::N64];
  for (int i = 0; i < F::N64; ++i) w[i] = in[2 * i] | (static_cast<u64>(in[2 * i + 1]) << 32);
  return F::from_mont64(w);
}
__device__ __forceinline__ void to_m64(u32* out, const fe& a) {
  u64 w[F::N64];
  F::to_mont64(w, a);
  for (int i = 0; i < F::N64; ++i) out[2 * i] = static_cast<u32>(w[i]), out[2 * i + 1] = static_cast<u32>(w[i] >> 32);
}
// out: product (ABI form), 1 when mul_pinned gave the same limbs
struct m29_mul : op_base {
  BZ_DH_IO(2 * kW64, kW64 + 1)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    const fe a = from_m64(in), b = from_m64(in + kW64);
    const fe slow = F::mul(a, b), fast = F::mul_pinned(a, b);
    to_m64(out, slow);
    out[kW64] = same_limbs(slow, fast) ? 1 : 0;
  }
};
struct m29_roundtrip : op_base {
  BZ_DH_IO(kW64, kW64)
  __device__ static void run(const u32* in, u32* out, const params4&) { to_m64(out, from_m64(in)); }
};
struct m29_invert : op_base {
  BZ_DH_IO(kW64, kW64)
  __device__ static void run(const u32* in, u32* out, const params4&) { to_m64(out, F::invert(from_m64(in))); }
};
// (2a) b + c (3d), one reduction; out: value, 1 when mul2_pinned gave the same limbs
struct m29_mul2 : op_base {
  BZ_DH_IO(4 * kW64, kW64 + 1)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    const fe a = from_m64(in), b = from_m64(in + kW64), c = from_m64(in + 2 * kW64), d = from_m64(in + 3 * kW64);
    const fe a2 = F::add(a, a), d3 = F::add(F::add(d, d), d);
    const fe lhs = F::mul2(a2, b, c, d3), scan = F::mul2_pinned(a2, b, c, d3);
    to_m64(out, lhs);
    out[kW64] = same_limbs(lhs, scan) ? 1 : 0;
  }
};
// raw limbs: out = mul, mul_pinned
struct m29_raw_mul : op_base {
  BZ_DH_IO(2 * kN, 2 * kN)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    const fe a = load_as<fe>(in), b = load_as<fe>(in + kN);
    store_as(out, F::mul(a, b));
    store_as(out + kN, F::mul_pinned(a, b));
  }
};
struct m29_raw_norm : op_base {
  BZ_DH_IO(kN, kN)
  __device__ static void run(const u32* in, u32* out, const params4&) { store_as(out, F::norm(load_as<fe>(in))); }
};
// out: sub<2>, sub<4>, sub<8>, neg<2>(b), neg<4>(b), neg<8>(b)
struct m29_raw_sub : op_base {
  BZ_DH_IO(2 * kN, 6 * kN)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    const fe a = load_as<fe>(in), b = load_as<fe>(in + kN);
    store_as(out, F::template sub<2>(a, b));
    store_as(out + kN, F::template sub<4>(a, b));
    store_as(out + 2 * kN, F::template sub<8>(a, b));
    store_as(out + 3 * kN, F::template neg<2>(b));
    store_as(out + 4 * kN, F::template neg<4>(b));
    store_as(out + 5 * kN, F::template neg<8>(b));
  }
};
struct m29_raw_mul_b3 : op_base {
  BZ_DH_IO(kN, kN)
  __device__ static void run(const u32* in, u32* out, const params4&) { store_as(out, G::mul_b3(load_as<fe>(in))); }
};
struct sw29_add : op_base {
  BZ_DH_IO(2 * kPt64, kPt64)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    store_as(out, G::to_point64(G::add(G::from_point64(load_as<point64>(in)),
                                       G::from_point64(load_as<point64>(in + kPt64)))));
  }
};
struct sw29_dbl_n : op_base {
  BZ_DH_IO(kPt64 + 1, kPt64)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    const u32 k = in[kPt64] > 64 ? 64 : in[kPt64];
    store_as(out, G::to_point64(G::dbl_n(G::from_point64(load_as<point64>(in)), static_cast<int>(k))));
  }
};
// params: {n, lifted}; record: start (ABI projective), n x (affine x, y ABI form, negate).
// lifted 0: out = start + sum (+-) q_i through add_mixed, then 1 when add_mixed<true>, add_mixed_acc<false>
// and add_mixed_acc<true> agreed with it at every step (limbs, limbs, canonical result);
// lifted 1: k_accumulate's lane: the first entry lifted (lift_acc), the others add_mixed_acc<true>
struct sw29_chain : op_base {
  static bool valid(const params4& p) { return p.v[0] >= 1 && p.v[0] <= 64 && p.v[1] <= 1; }
  __host__ __device__ static constexpr u32 in_words(const params4& p) { return kPt64 + p.v[0] * (2 * kW64 + 1); }
  __host__ __device__ static constexpr u32 out_words(const params4&) { return kPt64 + 1; }
  __device__ static void run(const u32* in, u32* out, const params4& pr) {
    const u32 n = pr.v[0] > 64 ? 64 : pr.v[0];
    const bool lifted = pr.v[1] != 0;
    point acc = lifted ? G::identity() : G::from_point64(load_as<point64>(in));
    point tight = acc;
    bool same = true;
    for (u32 i = 0; i < n; ++i) {
      const u32* rec = in + kPt64 + i * (2 * kW64 + 1);
      G::affine q{from_m64(rec), from_m64(rec + kW64)};
      const bool neg = rec[2 * kW64] != 0;
      if (lifted) {
        acc = i == 0 ? G::lift_acc(q, neg) : G::template add_mixed_acc<true>(acc, q, neg);
      } else {
        const point fast = G::template add_mixed<true>(acc, q, neg);
        acc = G::add_mixed(acc, q, neg);
        same = same && same_limbs(fast, acc);
        const point tight_slow = G::template add_mixed_acc<false>(tight, q, neg);
        tight = G::template add_mixed_acc<true>(tight, q, neg);
        same = same && same_limbs(tight_slow, tight);
      }
    }
    const point64 r = G::to_point64(acc);
    store_as(out, r);
    if (!lifted) {
      const point64 rt = G::to_point64(tight);
      const u32* x = reinterpret_cast<const u32*>(&r);
      const u32* y = reinterpret_cast<const u32*>(&rt);
      for (u32 i = 0; i < kPt64; ++i) same = same && x[i] == y[i];
    }
    out[kPt64] = same ? 1 : 0;
  }
};

#if defined(BZ_DH_SW_WAVE)
//--------------------------------------------------------------------------------------------------
// sww::wave<G>, the wave members of the curve's trait and add_coop4
//--------------------------------------------------------------------------------------------------
using W = sww::wave<G>;
__device__ __forceinline__ void put_point(u32* out, const point& p) {
  if ((threadIdx.x & 63) == 0) store_as(out, p);
}
struct sww_fmul : wave_op_base {
  BZ_DH_IO(128, 64)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    const typename W::ctx c = W::make_ctx(sww::wave_scratch());
    out[c.lane] = W::fmul(c, in[c.lane], in[64 + c.lane]);
  }
};
struct sww_dbl : wave_op_base {
  BZ_DH_IO(64, 64 + kPt)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    const typename W::ctx c = W::make_ctx(sww::wave_scratch());
    const u32 st = W::dbl(c, in[c.lane]);
    out[c.lane] = st;
    put_point(out + 64, W::store_point(c, st));
  }
};
struct sww_add : wave_op_base {
  BZ_DH_IO(128, 64 + kPt)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    const typename W::ctx c = W::make_ctx(sww::wave_scratch());
    const u32 st = W::add(c, in[c.lane], in[64 + c.lane]);
    out[c.lane] = st;
    put_point(out + 64, W::store_point(c, st));
  }
};
// params: {n}; step k: add(q) when k is a multiple of 3, else dbl; the raw state is fed back
struct sww_chain : wave_op_base {
  static bool valid(const params4& p) { return p.v[0] <= kMaxChain; }
  BZ_DH_IO(128, 64 + kPt)
  __device__ static void run(const u32* in, u32* out, const params4& pr) {
    const typename W::ctx c = W::make_ctx(sww::wave_scratch());
    const u32 n = pr.v[0] > kMaxChain ? kMaxChain : pr.v[0];
    u32 st = in[c.lane];
    const u32 q = in[64 + c.lane];
#pragma unroll 1
    for (u32 k = 0; k < n; ++k) st = (k % 3 == 0) ? W::add(c, st, q) : W::dbl(c, st);
    out[c.lane] = st;
    put_point(out + 64, W::store_point(c, st));
  }
};
// record: point (engine limbs) -> load_point_value lane words, store_point of them
struct sww_roundtrip : wave_op_base {
  BZ_DH_IO(kPt, 64 + kPt)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    const typename W::ctx c = W::make_ctx(sww::wave_scratch());
    const u32 st = W::load_point_value(c, load_as<point>(in));
    out[c.lane] = st;
    put_point(out + 64, W::store_point(c, st));
  }
};
// params: {num_windows, window_bits, have_acc}; record: acc, num_windows window sums (engine limbs)
struct sww_horner : wave_op_base {
  static bool valid(const params4& p) {
    return p.v[0] >= 1 && p.v[0] <= kMaxWindows && p.v[1] >= 1 && p.v[1] <= kMaxWindowBits && p.v[2] <= 1;
  }
  __host__ __device__ static constexpr u32 in_words(const params4& p) { return (1 + p.v[0]) * kPt; }
  __host__ __device__ static constexpr u32 out_words(const params4&) { return kPt; }
  __device__ static void run(const u32* in, u32* out, const params4& pr) {
    __shared__ point sums[kMaxWindows];
    const u32 nw = pr.v[0] > kMaxWindows ? kMaxWindows : pr.v[0];
    const u32 bits = pr.v[1] > kMaxWindowBits ? kMaxWindowBits : pr.v[1];
    for (u32 w = threadIdx.x; w < nw; w += 64) sums[w] = load_as<point>(in + (1 + w) * kPt);
    __syncthreads();
    put_point(out, C::wave_horner(load_as<point>(in), pr.v[2] != 0, sums, 1, nw, bits));
  }
};
struct sww_add_multiple : wave_op_base {
  BZ_DH_IO(2 * kPt + 1, kPt)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    const u32 m = in[2 * kPt] == 0 ? 1u : in[2 * kPt];
    put_point(out, C::wave_add_multiple(load_as<point>(in), load_as<point>(in + kPt), m));
  }
};
struct sww_wave_chain : wave_op_base {
  static bool valid(const params4& p) {
    return p.v[0] >= 1 && p.v[0] <= kMaxWindows && p.v[1] >= 1 && p.v[1] <= kMaxWindowBits;
  }
  __host__ __device__ static constexpr u32 in_words(const params4&) { return kPt; }
  __host__ __device__ static constexpr u32 out_words(const params4& p) { return p.v[0] * kPt; }
  __device__ static void run(const u32* in, u32* out, const params4& pr) {
    const u32 nw = pr.v[0] > kMaxWindows ? kMaxWindows : pr.v[0];
    const u32 bits = pr.v[1] > kMaxWindowBits ? kMaxWindowBits : pr.v[1];
    C::wave_chain(reinterpret_cast<point*>(out), 1, load_as<point>(in), nw, bits);
  }
};
// record: 16 x (p, q), one pair per quad of the wavefront -> the result as every lane holds it
struct sw29_coop4 : wave_op_base {
  BZ_DH_IO(16 * 2 * kPt, 64 * kPt)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    const u32 lane = threadIdx.x & 63, quad = lane >> 2;
    const point p = load_as<point>(in + quad * 2 * kPt), q = load_as<point>(in + quad * 2 * kPt + kPt);
    store_as(out + lane * kPt, C::add_coop4(p, q, lane & 3));
  }
};
#endif // BZ_DH_SW_WAVE

#define BZ_DH_OPS_SW_LANE(X)                                                                       \
  X(m29_mul) X(m29_roundtrip) X(m29_invert) X(m29_mul2) X(m29_raw_mul) X(m29_raw_norm)             \
  X(m29_raw_sub) X(m29_raw_mul_b3) X(sw29_add) X(sw29_dbl_n) X(sw29_chain)
#if defined(BZ_DH_SW_WAVE)
#define BZ_DH_OPS(X)                                                                               \
  BZ_DH_OPS_SW_LANE(X)                                                                             \
  X(sww_fmul) X(sww_dbl) X(sww_add) X(sww_chain) X(sww_roundtrip) X(sww_horner) X(sww_add_multiple) \
  X(sww_wave_chain) X(sw29_coop4)
#else
#define BZ_DH_OPS(X) BZ_DH_OPS_SW_LANE(X)
#endif
#endif // BZ_DH_SW

#if defined(BZ_DH_PROOF)
//--------------------------------------------------------------------------------------------------
// proof/: the wavefront's sponge and Merlin, one case per workgroup of 64 with the state in LDS as
// the product kernels hold it (8-byte aligned); the scalar and element arithmetic, one case per
// lane, each op the expression a product kernel evaluates
//--------------------------------------------------------------------------------------------------
using namespace proof;
using sponge_strobe = strobe128_over<wave_sponge>;
constexpr u32 kRate = sponge_strobe::kRate;
constexpr u32 kTr = 51 /* the 203 bytes of a transcript and one of padding */, kS = 8 /* 32 bytes */;
constexpr u32 kMaxLabel = 16, kMaxMessage = 512, kMaxChallenge = 256;

__device__ __forceinline__ void wave_copy_in(u8* lds, const u32* in, u32 bytes) {
  const u8* b = reinterpret_cast<const u8*>(in);
  for (u32 i = wave_sponge::lane(); i < bytes; i += 64) lds[i] = b[i];
}
__device__ __forceinline__ void wave_copy_out(u32* out, const u8* lds, u32 bytes) {
  u8* b = reinterpret_cast<u8*>(out);
  for (u32 i = wave_sponge::lane(); i < bytes; i += 64) b[i] = lds[i];
}
// the caller's transcript into LDS; `pos` indexes the state: validated on the host, clamped here
__device__ __forceinline__ void load_checked_transcript(transcript_state& t, const u32* in) {
  wave_load_transcript(t, reinterpret_cast<const u8*>(in));
  if (wave_sponge::lane() == 0 && t.pos >= kRate) t.pos = kRate - 1;
  wave_sponge::sync();
}
// every record starts with a transcript: pos < kRate
template <class Op> bool transcripts_valid(const u32* in, u32 cases, const params4& pr) {
  for (u32 c = 0; c < cases; ++c) {
    const u8* t = reinterpret_cast<const u8*>(in + static_cast<size_t>(c) * Op::in_words(pr));
    if (t[200] >= kRate) return false;
  }
  return true;
}

// params: {permutations 1 .. 2}; record: 200 state bytes -> 200 state bytes
struct keccak_wave : wave_op_base {
  static bool valid(const params4& p) { return p.v[0] >= 1 && p.v[0] <= 2; }
  BZ_DH_IO(50, 50)
  __device__ static void run(const u32* in, u32* out, const params4& pr) {
    __shared__ alignas(8) u8 state[200];
    wave_copy_in(state, in, 200);
    wave_sponge::sync();
    wave_sponge::permute(state);
    if (pr.v[0] >= 2) wave_sponge::permute(state);
    wave_copy_out(out, state, 200);
  }
};
// params: {label bytes 1 .. 16, message bytes 0 .. 512, challenge bytes 1 .. 256, form};
// record: transcript, label, message -> transcript, challenge.  form 0: append_message(label,
// message), form 1 (message bytes = 8): append_u64(label, the message's 8 bytes as an integer);
// then challenge_bytes(label)
struct merlin_wave : wave_op_base {
  static bool valid(const params4& p) {
    return p.v[0] >= 1 && p.v[0] <= kMaxLabel && p.v[1] <= kMaxMessage && p.v[2] >= 1 &&
           p.v[2] <= kMaxChallenge && (p.v[3] == 0 || (p.v[3] == 1 && p.v[1] == 8));
  }
  static bool valid_records(const u32* in, u32 cases, const params4& pr) {
    return transcripts_valid<merlin_wave>(in, cases, pr);
  }
  BZ_DH_IO(kTr + kMaxLabel / 4 + kMaxMessage / 4, kTr + kMaxChallenge / 4)
  struct alignas(8) lds_state {
    transcript_state t;
    u8 pad[5];
    u8 message[kMaxMessage];
    u8 challenge[kMaxChallenge];
    char name[kMaxLabel];
  };
  __device__ static void run(const u32* in, u32* out, const params4& pr) {
    __shared__ lds_state w;
    const u32 label_bytes = pr.v[0] > kMaxLabel ? kMaxLabel : pr.v[0];
    const u32 message_bytes = pr.v[1] > kMaxMessage ? kMaxMessage : pr.v[1];
    const u32 challenge_bytes = pr.v[2] > kMaxChallenge ? kMaxChallenge : pr.v[2];
    load_checked_transcript(w.t, in);
    wave_copy_in(reinterpret_cast<u8*>(w.name), in + kTr, kMaxLabel);
    wave_copy_in(w.message, in + kTr + kMaxLabel / 4, kMaxMessage);
    wave_sponge::sync();
    const label_view name{w.name, label_bytes};
    transcript_over<wave_sponge> tr{&w.t};
    if (pr.v[3] == 0) {
      tr.append_message(name, w.message, message_bytes);
    } else {
      const u32* m = in + kTr + kMaxLabel / 4;
      tr.append_u64(name, m[0] | (static_cast<u64>(m[1]) << 32));
    }
    tr.challenge_bytes(w.challenge, challenge_bytes, name);
    wave_store_transcript(reinterpret_cast<u8*>(out), w.t);
    wave_copy_out(out + kTr, w.challenge, challenge_bytes);
  }
};

__device__ __forceinline__ const u8* bytes_of(const u32* in) { return reinterpret_cast<const u8*>(in); }
__device__ __forceinline__ u8* bytes_of(u32* out) { return reinterpret_cast<u8*>(out); }

// round_challenge and the scalar challenge::make: any 256-bit integer to its canonical residue
struct s25_reduce : op_base {
  BZ_DH_IO(kS, kS)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    s25::store(bytes_of(out), s25::from_mont(s25::to_mont(s25::load(bytes_of(in)))));
  }
};
// k_fold_scalars; record: m_low, m_high, u, v
struct s25_fold : op_base {
  BZ_DH_IO(4 * kS, kS)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    const s25::fe m_low = s25::to_mont(s25::load(bytes_of(in)));
    const s25::fe m_high = s25::to_mont(s25::load(bytes_of(in + kS)));
    s25::store(bytes_of(out), s25::add(s25::F::mul(m_low, s25::load(bytes_of(in + 2 * kS))),
                                       s25::F::mul(m_high, s25::load(bytes_of(in + 3 * kS)))));
  }
};
// k_inner_product with k_cross_finish; params: {n 1 .. 64}; record: n x (a_i, b_i)
struct s25_dot : op_base {
  static bool valid(const params4& p) { return p.v[0] >= 1 && p.v[0] <= 64; }
  __host__ __device__ static constexpr u32 in_words(const params4& p) { return p.v[0] * 2 * kS; }
  __host__ __device__ static constexpr u32 out_words(const params4&) { return kS; }
  __device__ static void run(const u32* in, u32* out, const params4& pr) {
    const u32 n = pr.v[0] > 64 ? 64 : pr.v[0];
    s25::fe acc = s25::F::zero();
    for (u32 i = 0; i < n; ++i) {
      acc = s25::add(acc, s25::F::mul(s25::load(bytes_of(in + 2 * kS * i)),
                                      s25::load(bytes_of(in + 2 * kS * i + kS))));
    }
    s25::store(bytes_of(out), s25::F::mul(acc, s25::r2()));
  }
};
// k_round_challenge's 1 / x (zero for zero)
struct s25_invert : op_base {
  BZ_DH_IO(kS, kS)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    s25::store(bytes_of(out), s25::from_mont(s25::F::invert(s25::to_mont(s25::load(bytes_of(in))))));
  }
};
// the element conversions of proof/sumcheck_rows.h, E = scalar25519_elements (sc_) / grumpkin_elements (gk_)
template <class E> struct el_roundtrip : op_base {
  BZ_DH_IO(kS, kS)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    E::store(bytes_of(out), E::load(bytes_of(in)));
  }
};
// record: four 64-bit words, element
template <class E> struct el_convert : op_base {
  BZ_DH_IO(kS + 1, kS)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    u64 w[4];
    for (int i = 0; i < 4; ++i) w[i] = in[2 * i] | (static_cast<u64>(in[2 * i + 1]) << 32);
    E::store(bytes_of(out), E::convert(w, in[kS] != 0));
  }
};
// wave_round's 1 - r
template <class E> struct el_one_minus : op_base {
  BZ_DH_IO(kS, kS)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    using F = typename E::F;
    E::store(bytes_of(out), fsub<F>(F::one(), E::load(bytes_of(in))));
  }
};
// record: x -> r_bytes, E::store of the returned engine form
template <class E> struct el_challenge_make : op_base {
  BZ_DH_IO(kS, 2 * kS)
  __device__ static void run(const u32* in, u32* out, const params4&) {
    const typename E::F::fe r = challenge<E>::make(bytes_of(out), bytes_of(in));
    E::store(bytes_of(out + kS), r);
  }
};
struct sc_roundtrip : el_roundtrip<scalar25519_elements> {};
struct gk_roundtrip : el_roundtrip<grumpkin_elements> {};
struct sc_convert : el_convert<scalar25519_elements> {};
struct gk_convert : el_convert<grumpkin_elements> {};
struct sc_one_minus : el_one_minus<scalar25519_elements> {};
struct gk_one_minus : el_one_minus<grumpkin_elements> {};
struct sc_challenge_make : el_challenge_make<scalar25519_elements> {};
struct gk_challenge_make : el_challenge_make<grumpkin_elements> {};

// params: {field_id 0 .. 1, length 2 .. 9}; record: transcript, polynomial (9 x 32 bytes) ->
// transcript, x, r in the caller's representation, E::store of the returned engine form
struct sumcheck_round_wave : wave_op_base {
  static bool valid(const params4& p) { return p.v[0] <= 1 && p.v[1] >= 2 && p.v[1] <= kMaxDegree + 1; }
  static bool valid_records(const u32* in, u32 cases, const params4& pr) {
    return transcripts_valid<sumcheck_round_wave>(in, cases, pr);
  }
  BZ_DH_IO(kTr + (kMaxDegree + 1) * kS, kTr + 3 * kS)
  struct alignas(8) lds_state { // proof/sumcheck_transcript.hip wave_transcript
    transcript_state t;
    u8 pad[5];
    u8 message[(kMaxDegree + 1) * 32];
    u8 x[32], r[32], engine[32];
  };
  template <class E> __device__ static void round(lds_state& w, u32 length) {
    const typename E::F::fe r = transcript_round<E, wave_sponge>(w.r, w.x, &w.t, w.message, length);
    wave_sponge::sync();
    if (wave_sponge::lane() == 0) E::store(w.engine, r);
    wave_sponge::sync();
  }
  __device__ static void run(const u32* in, u32* out, const params4& pr) {
    __shared__ lds_state w;
    const u32 length = pr.v[1] > kMaxDegree + 1 ? kMaxDegree + 1 : pr.v[1];
    load_checked_transcript(w.t, in);
    wave_copy_in(w.message, in + kTr, (kMaxDegree + 1) * 32);
    wave_sponge::sync();
    if (pr.v[0] == 0) {
      round<scalar25519_elements>(w, length);
    } else {
      round<grumpkin_elements>(w, length);
    }
    wave_store_transcript(bytes_of(out), w.t);
    wave_copy_out(out + kTr, w.x, 32);
    wave_copy_out(out + kTr + kS, w.r, 32);
    wave_copy_out(out + kTr + 2 * kS, w.engine, 32);
  }
};
// k_round_challenge's transcript step; params: {init 0 .. 1}; record: transcript, L, R, n (64 bits)
// -> transcript, x, the returned x mod l as store(from_mont(.))
struct ip_round_wave : wave_op_base {
  static bool valid(const params4& p) { return p.v[0] <= 1; }
  static bool valid_records(const u32* in, u32 cases, const params4& pr) {
    return transcripts_valid<ip_round_wave>(in, cases, pr);
  }
  BZ_DH_IO(kTr + 2 * kS + 2, kTr + 2 * kS)
  struct alignas(8) lds_state { // proof/inner_product.hip wave_state
    transcript_state t;
    u8 pad[5];
    u8 l[32], r[32], x[32], reduced[32];
  };
  __device__ static void run(const u32* in, u32* out, const params4& pr) {
    __shared__ lds_state w;
    load_checked_transcript(w.t, in);
    wave_copy_in(w.l, in + kTr, 32);
    wave_copy_in(w.r, in + kTr + kS, 32);
    wave_sponge::sync();
    const u64 n = in[kTr + 2 * kS] | (static_cast<u64>(in[kTr + 2 * kS + 1]) << 32);
    if (pr.v[0] != 0) init_transcript<wave_sponge>(&w.t, n);
    const s25::fe x = round_challenge<wave_sponge>(w.x, &w.t, w.l, w.r);
    wave_sponge::sync();
    if (wave_sponge::lane() == 0) s25::store(w.reduced, s25::from_mont(x));
    wave_sponge::sync();
    wave_store_transcript(bytes_of(out), w.t);
    wave_copy_out(out + kTr, w.x, 32);
    wave_copy_out(out + kTr + kS, w.reduced, 32);
  }
};
// a lane of k_fold_generators over the terms of k_fold_terms; record: 256 digit bytes, count, g_lo,
// g_hi (ed_point) -> m_low g_lo + m_high g_hi (ed_point).  Digits pick one of three terms and the
// count bounds the walk: at most 3 and kScalarBits, validated on the host, clamped here
struct ip_fold_point : op_base {
  static constexpr u32 kEdPoint = 40;
  BZ_DH_IO(65 + 2 * kEdPoint, kEdPoint)
  static bool valid_records(const u32* in, u32 cases, const params4& pr) {
    for (u32 c = 0; c < cases; ++c) {
      const u32* rec = in + static_cast<size_t>(c) * in_words(pr);
      if (rec[64] > kScalarBits) return false;
      const u8* d = reinterpret_cast<const u8*>(rec);
      for (u32 i = 0; i < 256; ++i) {
        if (d[i] > 3) return false;
      }
    }
    return true;
  }
  __device__ static void run(const u32* in, u32* out, const params4&) {
    fold_digits digits;
    for (u32 i = 0; i < 256; ++i) digits.d[i] = bytes_of(in)[i] & 3;
    digits.count = in[64] > kScalarBits ? kScalarBits : in[64];
    const ed29_point lo = ed29::from_ed(load_as<ed_point>(in + 65));
    const ed29_point hi = ed29::from_ed(load_as<ed_point>(in + 65 + kEdPoint));
    const ed29_cached_packed terms[3] = {ed29::pack(ed29::to_cached(lo)), ed29::pack(ed29::to_cached(hi)),
                                         ed29::pack(ed29::to_cached(ed29::add(lo, hi)))};
    const ed29_point r = fold_point(digits, [&](u32 k) { return ed29::unpack(terms[k > 2 ? 2 : k]); });
    store_as(out, ed29::to_ed(r));
  }
};

#define BZ_DH_OPS(X)                                                                               \
  X(keccak_wave) X(merlin_wave) X(s25_reduce) X(s25_fold) X(s25_dot) X(s25_invert)                 \
  X(sc_roundtrip) X(gk_roundtrip) X(sc_convert) X(gk_convert) X(sc_one_minus) X(gk_one_minus)      \
  X(sc_challenge_make) X(gk_challenge_make) X(sumcheck_round_wave) X(ip_round_wave) X(ip_fold_point)
#endif // BZ_DH_PROOF

template <class Op>
int launch(const u32* in, u64 in_words, u32* out, u64 out_words, u32 cases, const params4& pr) {
  if (!Op::valid(pr)) return -3;
  if (cases == 0 || cases > kMaxCases) return -3;
  if (in_words != static_cast<u64>(cases) * Op::in_words(pr)) return -2;
  if (out_words != static_cast<u64>(cases) * Op::out_words(pr)) return -2;
  if (!Op::valid_records(in, cases, pr)) return -3;
  u32 *din = nullptr, *dout = nullptr;
  hipError_t e = hipMalloc(&din, in_words * 4);
  if (e != hipSuccess) return static_cast<int>(e);
  e = hipMalloc(&dout, out_words * 4);
  if (e == hipSuccess) e = hipMemcpy(din, in, in_words * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dout, 0, out_words * 4);
  if (e == hipSuccess) {
    if constexpr (Op::wave) {
      hipLaunchKernelGGL((k_wave<Op>), dim3(cases), dim3(64), 0, 0, din, dout, pr);
    } else {
      hipLaunchKernelGGL((k_lane<Op>), dim3((cases + 63) / 64), dim3(64), 0, 0, din, dout, cases, pr);
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, out_words * 4, hipMemcpyDeviceToHost);
  (void)hipFree(din);
  (void)hipFree(dout);
  return static_cast<int>(e);
}

inline int run(const char* op, const u32* in, u64 in_words, u32* out, u64 out_words, u32 cases,
               const u32* params) {
  params4 pr;
  for (int i = 0; i < 4; ++i) pr.v[i] = params[i];
#define BZ_DH_DISPATCH(NAME) \
  if (std::strcmp(op, #NAME) == 0) return launch<NAME>(in, in_words, out, out_words, cases, pr);
  BZ_DH_OPS(BZ_DH_DISPATCH)
#undef BZ_DH_DISPATCH
  return -1;
}
} // namespace dh_<tag>
} // namespace bz

extern "C" int BZ_DH_CAT(bz_dh_run_, BZ_DH_TAG)(const char* op, const bz::u32* in, bz::u64 in_words,
                                                bz::u32* out, bz::u64 out_words, bz::u32 cases,
                                                const bz::u32* params) {
  return bz::BZ_DH_CAT(dh_, BZ_DH_TAG)::run(op, in, in_words, out, out_words, cases, params);
}
