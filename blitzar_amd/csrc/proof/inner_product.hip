// Inner-product argument prover / verifier (proof/inner_product.h).
//
// Protocol (reference: sxt/proof/inner_product/proof_computation.cc:54-155): with np = 2^k >= n,
// generators g_0 .. g_{np-1}, Q = g_np, vectors a, b padded with zeros to np; per round
//   L = <a_lo, g_hi> + <a_lo, b_hi> Q,   R = <a_hi, g_lo> + <a_hi, b_lo> Q,
//   x = challenge(L, R),
//   a' = x a_lo + x^-1 a_hi,  b' = x^-1 b_lo + x b_hi,  g' = x^-1 g_lo + x g_hi,
// until one element is left.  Proof bytes (compressed L, R; the last a) are canonical encodings
// of group elements / scalars, so any correct evaluation order reproduces the reference's bytes.
//
// The host backend runs the round loop on host loops.  On the device a proof is a chain of kernels
// enqueued on one stream that never returns to the host: everything lives in
// the caller's workspace as
//   scalars     S = [c_l | a_0 .. a_{size-1} | c_r]      (a zero-padded to np; size halves per round)
//   generators  G = [g_lo (mid) | Q | g_hi (mid)]
// so that ONE call of the MSM engine with two columns and per-column generator offsets yields
//   L = rows S[0 .. mid]          over G[mid ..]  = c_l Q + <a_lo, g_hi>,
//   R = rows S[mid + 1 .. size+1] over G[0 ..]    = <a_hi, g_lo> + c_r Q:
// the two c Q products are one more row of each column, not a serial double-and-add.  a stays at
// S + 1 through every fold (in place: entry i is read by its own lane only), c_r moves down to the
// end of the halved a; the generator fold writes through the terms buffer and re-places Q between
// the halves of the folded generators.  The transcript step of a round (Merlin on wavefront 0,
// x mod l, 1 / x, the joint fold digits) is one workgroup that leaves its results in a workspace
// slot for the fold kernels.
#include "blitzar_amd/csrc/proof/inner_product.h"

#include <algorithm>
#include <vector>

#include "blitzar_amd/csrc/curve/ed29.h"
#include "blitzar_amd/csrc/proof/inner_product_protocol.h"
#include "blitzar_amd/csrc/proof/scalar25.h"
#include "blitzar_amd/csrc/proof/transcript.h"

namespace bz::proof {
namespace {
using s25::scalar;
// k * p on the host (253-bit double-and-add on the ABI-form arithmetic)
ed_point scalar_multiply(const ed_point& p, const u8 k[32]) {
  ed_point acc = ed::identity();
  bool started = false;
  for (int bit = 255; bit >= 0; --bit) {
    if (started) acc = ed::dbl(acc);
    if ((k[bit >> 3] >> (bit & 7)) & 1) {
      acc = started ? ed::add(acc, p) : p;
      started = true;
    }
  }
  return acc;
}

//--------------------------------------------------------------------------------------------------
// the transcript of the protocol (proof/inner_product_protocol.h) on the host
//--------------------------------------------------------------------------------------------------
scalar host_round_challenge(void* transcript_bytes, const u8* l_value, const u8* r_value) {
  u8 x[32];
  return {round_challenge<host_sponge>(x, static_cast<transcript_state*>(transcript_bytes), l_value,
                                       r_value)};
}

//--------------------------------------------------------------------------------------------------
// device kernels
//--------------------------------------------------------------------------------------------------
constexpr u32 kPartialBlocks = 256; // workgroups of k_inner_product, at most

// Before the first round: a and b into the workspace zero-padded to np (a behind the c_l row), the
// caller's np + 1 generators into [g_lo | Q | g_hi] (nullptr: the built-in ones were derived in
// place before this kernel), Q aside for the generator folds.
__global__ void __launch_bounds__(256)
    k_load(u64* __restrict__ s, u64* __restrict__ b_out, ed_point* g, ed_point* __restrict__ q,
           const u8* __restrict__ a, const u8* __restrict__ b, const ed_point* generators, u32 n,
           u32 np) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  const u32 mid = np / 2;
  if (i == 0) *q = generators != nullptr ? generators[np] : g[mid];
  if (i >= np) return;
  // the caller's scalars are bytes: no alignment is promised
  const bool aligned = ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 7) == 0;
  for (int k = 0; k < 4; ++k) {
    u64 wa = 0, wb = 0;
    if (i < n) {
      const u64 at = 32 * static_cast<u64>(i) + 8 * k;
      if (aligned) {
        wa = *reinterpret_cast<const u64*>(a + at);
        wb = *reinterpret_cast<const u64*>(b + at);
      } else {
        for (int j = 7; j >= 0; --j) {
          wa = (wa << 8) | a[at + j];
          wb = (wb << 8) | b[at + j];
        }
      }
    }
    s[4 * (static_cast<u64>(i) + 1) + k] = wa;
    b_out[4 * static_cast<u64>(i) + k] = wb;
  }
  if (generators != nullptr) {
    g[i < mid ? i : i + 1] = generators[i];
    if (i == 0) g[mid] = generators[np];
  }
}

// what a wavefront keeps in LDS for a transcript step
struct alignas(8) wave_state {
  transcript_state t;
  u8 pad[5];
  u8 l[32], r[32], x[32];
};

// n = 1: the transcript's init, and ap = a[0] verbatim
__global__ void __launch_bounds__(64)
    k_single_element(u8* __restrict__ ap, u8* transcript, const u8* __restrict__ a) {
  __shared__ wave_state w;
  wave_load_transcript(w.t, transcript);
  init_transcript<wave_sponge>(&w.t, 1);
  wave_store_transcript(transcript, w.t);
  if (threadIdx.x < 32) ap[threadIdx.x] = a[threadIdx.x];
}

// out[i] = m_low x[i] + m_high x[mid + i] (canonical), i < mid (fold.cc:30-45); (m_low, m_high) =
// (x, x^-1) for a, (x^-1, x) for b, from the slot in Montgomery form; the vector is plain: the
// products are plain.  In place (out == in) is safe: entry i is only read by its own lane, entries
// >= mid are not written.  The last fold of a (mid = 1) goes to the caller as `last`.
__global__ void __launch_bounds__(256)
    k_fold_scalars(u64* out, u8* last, const u64* in, const fold_slot* __restrict__ slot,
                   int low_is_x, u32 mid) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= mid) return;
  const s25::fe m_low = low_is_x ? slot->x : slot->x_inv;
  const s25::fe m_high = low_is_x ? slot->x_inv : slot->x;
  const s25::fe r =
      s25::add(s25::F::mul(m_low, s25::load_words(in + 4 * static_cast<u64>(i))),
               s25::F::mul(m_high, s25::load_words(in + 4 * (static_cast<u64>(mid) + i))));
  if (last != nullptr) {
    s25::store(last, r);
    return;
  }
  u64 w[4];
  s25::store_words(w, r);
  for (int k = 0; k < 4; ++k) out[4 * static_cast<u64>(i) + k] = w[k];
}

// partials[block] = sum over the block's share of a[i] b[i] / R (plain inputs; k_cross_finish adds
// the partials and multiplies by R^2): grid-stride products, LDS tree
__global__ void __launch_bounds__(256)
    k_inner_product(s25::fe* __restrict__ partials, const u64* __restrict__ a,
                    const u64* __restrict__ b, u32 count) {
  __shared__ s25::fe tree[256];
  s25::fe acc = s25::F::zero();
  for (u64 i = blockIdx.x * 256u + threadIdx.x; i < count; i += static_cast<u64>(gridDim.x) * 256u) {
    acc = s25::add(acc, s25::F::mul(s25::load_words(a + 4 * i), s25::load_words(b + 4 * i)));
  }
  tree[threadIdx.x] = acc;
  __syncthreads();
  for (u32 stride = 128; stride > 0; stride >>= 1) {
    if (threadIdx.x < stride) {
      tree[threadIdx.x] = s25::add(tree[threadIdx.x], tree[threadIdx.x + stride]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = tree[0];
}

// One workgroup: c_l and c_r (canonical) from the `blocks` partials of each, which lie
// kPartialBlocks apart, into their rows of the scalar columns (c_r == nullptr: c_l alone)
__global__ void __launch_bounds__(kPartialBlocks)
    k_cross_finish(u64* __restrict__ c_l, u64* __restrict__ c_r,
                   const s25::fe* __restrict__ partials, u32 blocks) {
  __shared__ s25::fe tree[kPartialBlocks];
  const u32 sides = c_r != nullptr ? 2 : 1;
  for (u32 side = 0; side < sides; ++side) {
    tree[threadIdx.x] =
        threadIdx.x < blocks ? partials[side * kPartialBlocks + threadIdx.x] : s25::F::zero();
    __syncthreads();
    for (u32 stride = kPartialBlocks / 2; stride > 0; stride >>= 1) {
      if (threadIdx.x < stride) {
        tree[threadIdx.x] = s25::add(tree[threadIdx.x], tree[threadIdx.x + stride]);
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      u64 w[4];
      s25::store_words(w, s25::F::mul(tree[0], s25::r2()));
      u64* c = side == 0 ? c_l : c_r;
      for (int k = 0; k < 4; ++k) c[k] = w[k];
    }
    __syncthreads();
  }
}

// terms[k * mid + i], k = 0, 1, 2: g_i, g_{mid + 1 + i} (Q lies between the halves) and their sum
// as packed cached addends
__global__ void __launch_bounds__(256)
    k_fold_terms(ed29_cached_packed* __restrict__ terms, const ed_point* __restrict__ g, u32 mid) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= mid) return;
  const ed29_point lo = ed29::from_ed(g[i]), hi = ed29::from_ed(g[static_cast<u64>(mid) + 1 + i]);
  terms[i] = ed29::pack(ed29::to_cached(lo));
  terms[mid + i] = ed29::pack(ed29::to_cached(hi));
  terms[2 * static_cast<u64>(mid) + i] = ed29::pack(ed29::to_cached(ed29::add(lo, hi)));
}

// g'_i = x^-1 g_i + x g_{mid + i}, written in the next round's layout [g'_lo | Q | g'_hi]: every
// lane walks the SAME digit sequence (the slot's: wave-uniform loads, uniform control flow),
// gathering its own three terms.  It reads the terms only, so writing over g is safe.  mid >= 2.
__global__ void __launch_bounds__(256)
    k_fold_generators(ed_point* __restrict__ out, const ed29_cached_packed* __restrict__ terms,
                      const fold_slot* __restrict__ slot, const ed_point* __restrict__ q, u32 mid) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= mid) return;
  const ed29_point r = fold_point(slot->digits, [&](u32 k) {
    return ed29::unpack(terms[static_cast<u64>(k) * mid + i]);
  });
  const u32 half = mid / 2;
  out[i < half ? i : i + 1] = ed29::to_ed(r);
  if (i == 0) out[half] = *q;
}

// The transcript step of a round, one wavefront: L and R (the engine's encodings, `lr`) go to the
// caller and into the transcript (round 0, `n` != 0: its init first); x mod l, 1 / x (zero for
// zero, as scalar::inverse) and the joint digits of (x^-1, x) go to the slot.  Every lane computes
// the same scalars; the digits are spread over the lanes.
__global__ void __launch_bounds__(64)
    k_round_challenge(u8* __restrict__ l_value, u8* __restrict__ r_value,
                      fold_slot* __restrict__ slot, u8* transcript, const u8* __restrict__ lr, u64 n) {
  __shared__ wave_state w;
  const u32 lane = threadIdx.x;
  wave_load_transcript(w.t, transcript);
  if (lane < 32) {
    w.l[lane] = lr[lane];
    w.r[lane] = lr[32 + lane];
    l_value[lane] = lr[lane];
    r_value[lane] = lr[32 + lane];
  }
  wave_sponge::sync();
  if (n != 0) init_transcript<wave_sponge>(&w.t, n);
  const s25::fe x = round_challenge<wave_sponge>(w.x, &w.t, w.l, w.r);
  wave_store_transcript(transcript, w.t);
  const s25::fe x_inv = s25::F::invert(x);
  u64 lo[4], hi[4];
  s25::store_words(lo, s25::from_mont(x_inv));
  s25::store_words(hi, s25::from_mont(x));
  u32 count = 0;
#pragma unroll
  for (u32 k = 0; k < 4; ++k) {
    const u32 bit = 64 * k + lane;
    const u32 d = static_cast<u32>((lo[k] >> lane) & 1) + 2 * static_cast<u32>((hi[k] >> lane) & 1);
    slot->digits.d[bit] = static_cast<u8>(bit < kScalarBits ? d : 0);
    const u64 any = lo[k] | hi[k];
    if (any != 0) count = 64 * k + 64 - static_cast<u32>(__builtin_clzll(any));
  }
  if (lane == 0) {
    slot->x = x;
    slot->x_inv = x_inv;
    slot->digits.count = count < kScalarBits ? count : kScalarBits;
  }
}

//--------------------------------------------------------------------------------------------------
// the chain
//--------------------------------------------------------------------------------------------------
u64 ceil_log2(u64 n) {
  u64 k = 0;
  while ((u64{1} << k) < n) ++k;
  return k;
}

// the caller's workspace, for np = 2^ceil_log2(n)
struct workspace_layout {
  size_t scalars, b, generators, terms, partials, slot, q, lr, total;
  explicit workspace_layout(u64 np) {
    workspace_carver carve;
    scalars = carve.take(32 * (np + 2));
    b = carve.take(32 * np);
    generators = carve.take(sizeof(ed_point) * (np + 1));
    terms = carve.take(sizeof(ed29_cached_packed) * 3 * (np / 2));
    partials = carve.take(sizeof(s25::fe) * 2 * kPartialBlocks);
    slot = carve.take(sizeof(fold_slot));
    q = carve.take(sizeof(ed_point));
    lr = carve.take(64);
    total = carve.total();
  }
};

void enqueue_chain(msm_context& ctx, u8* l_vector, u8* r_vector, u8* ap_value, u8* transcript, u64 n,
                   u64 generators_offset, const ed_point* generators, const u8* a_vector,
                   const u8* b_vector, void* workspace, u64 workspace_bytes, hipStream_t stream) {
  if (n == 1) {
    hipLaunchKernelGGL(k_single_element, dim3(1), dim3(64), 0, stream, ap_value, transcript, a_vector);
    BZ_HIP_CHECK(hipGetLastError());
    g_kernel_launches += 1;
    return;
  }
  const u64 rounds = ceil_log2(n), np = u64{1} << rounds;
  const workspace_layout layout{np};
  BZ_RELEASE_ASSERT(workspace != nullptr && workspace_bytes >= layout.total,
                    "the inner-product workspace is too small");
  u8* base = workspace_carver::aligned(workspace);
  u64* d_s = reinterpret_cast<u64*>(base + layout.scalars);
  u64* d_a = d_s + 4; // behind the c_l row
  u64* d_b = reinterpret_cast<u64*>(base + layout.b);
  ed_point* d_g = reinterpret_cast<ed_point*>(base + layout.generators);
  auto* d_terms = reinterpret_cast<ed29_cached_packed*>(base + layout.terms);
  auto* d_partials = reinterpret_cast<s25::fe*>(base + layout.partials);
  auto* d_slot = reinterpret_cast<fold_slot*>(base + layout.slot);
  ed_point* d_q = reinterpret_cast<ed_point*>(base + layout.q);
  u8* d_lr = base + layout.lr;

  if (generators == nullptr) {
    builtin_generators_enqueue(d_g, generators_offset, np / 2, stream);
    builtin_generators_enqueue(d_g + np / 2, generators_offset + np, 1, stream);
    builtin_generators_enqueue(d_g + np / 2 + 1, generators_offset + np / 2, np / 2, stream);
    g_kernel_launches += 3;
  }
  hipLaunchKernelGGL(k_load, dim3(static_cast<u32>((np + 255) / 256)), dim3(256), 0, stream, d_s,
                     d_b, d_g, d_q, a_vector, b_vector, generators, static_cast<u32>(n),
                     static_cast<u32>(np));
  BZ_HIP_CHECK(hipGetLastError());
  g_kernel_launches += 1;

  const curve_vtable& vt = curve25519_vtable();
  u64 round = 0;
  for (u64 size = np; size > 1; size /= 2, ++round) {
    const u32 mid = static_cast<u32>(size / 2);
    const u32 blocks = (mid + 255) / 256;
    const u32 partial_blocks = std::min(kPartialBlocks, blocks);
    // c_l = <a_lo, b_hi> into row 0, c_r = <a_hi, b_lo> into the row behind a
    hipLaunchKernelGGL(k_inner_product, dim3(partial_blocks), dim3(256), 0, stream, d_partials, d_a,
                       d_b + 4 * static_cast<u64>(mid), mid);
    hipLaunchKernelGGL(k_inner_product, dim3(partial_blocks), dim3(256), 0, stream,
                       d_partials + kPartialBlocks, d_a + 4 * static_cast<u64>(mid), d_b, mid);
    hipLaunchKernelGGL(k_cross_finish, dim3(1), dim3(kPartialBlocks), 0, stream, d_s,
                       d_a + 4 * size, d_partials, partial_blocks);
    g_kernel_launches += 3;
    if (mid > 1) { // does not depend on x: ahead of the engine's kernels
      hipLaunchKernelGGL(k_fold_terms, dim3(blocks), dim3(256), 0, stream, d_terms, d_g, mid);
      g_kernel_launches += 1;
    }
    BZ_HIP_CHECK(hipGetLastError());
    // L and R in one call of the engine: generators and scalars are resident
    host_column col_l = byte_column(reinterpret_cast<const u8*>(d_s), mid + 1, 32, false);
    col_l.generator_offset = mid;
    const host_column col_r =
        byte_column(reinterpret_cast<const u8*>(d_a + 4 * static_cast<u64>(mid)), mid + 1, 32, false);
    vt.msm(ctx, d_lr, 32, false, {col_l, col_r}, nullptr, d_g, stream, false);
    hipLaunchKernelGGL(k_round_challenge, dim3(1), dim3(64), 0, stream, l_vector + 32 * round,
                       r_vector + 32 * round, d_slot, transcript, d_lr, round == 0 ? n : u64{0});
    hipLaunchKernelGGL(k_fold_scalars, dim3(blocks), dim3(256), 0, stream, d_a,
                       mid == 1 ? ap_value : nullptr, d_a, d_slot, 1, mid);
    g_kernel_launches += 2;
    if (mid > 1) {
      hipLaunchKernelGGL(k_fold_scalars, dim3(blocks), dim3(256), 0, stream, d_b,
                         static_cast<u8*>(nullptr), d_b, d_slot, 0, mid);
      hipLaunchKernelGGL(k_fold_generators, dim3(blocks), dim3(256), 0, stream, d_g, d_terms, d_slot,
                         d_q, mid);
      g_kernel_launches += 2;
    }
    BZ_HIP_CHECK(hipGetLastError());
  }
}

// the GPU backend's form on host operands: upload, the chain on the primary stream, download, one
// synchronise
void prove_uploaded(api_state& st, u8* l_vector, u8* r_vector, u8* ap_value, void* transcript, u64 n,
                    u64 generators_offset, const u8* a_vector, const u8* b_vector) {
  device_state& ds = st.primary();
  ds.activate();
  const u64 rounds = ceil_log2(n);
  const workspace_layout layout{u64{1} << rounds};
  ds.io.reset(2 * device_arena::padded(32 * n) + 2 * device_arena::padded(32 * rounds) +
                  device_arena::padded(32) + device_arena::padded(sizeof(transcript_state)) +
                  layout.total + 256,
              ds.stream);
  u8* d_a = ds.io.take<u8>(32 * n);
  u8* d_b = ds.io.take<u8>(32 * n);
  u8* d_l = ds.io.take<u8>(32 * rounds);
  u8* d_r = ds.io.take<u8>(32 * rounds);
  u8* d_ap = ds.io.take<u8>(32);
  u8* d_transcript = ds.io.take<u8>(sizeof(transcript_state));
  u8* d_workspace = ds.io.take<u8>(layout.total);
  BZ_HIP_CHECK(hipMemcpyAsync(d_a, a_vector, 32 * n, hipMemcpyHostToDevice, ds.stream));
  BZ_HIP_CHECK(hipMemcpyAsync(d_b, b_vector, 32 * n, hipMemcpyHostToDevice, ds.stream));
  BZ_HIP_CHECK(hipMemcpyAsync(d_transcript, transcript, sizeof(transcript_state),
                              hipMemcpyHostToDevice, ds.stream));
  enqueue_chain(*ds.ctx, d_l, d_r, d_ap, d_transcript, n, generators_offset, nullptr, d_a, d_b,
                d_workspace, layout.total, ds.stream);
  BZ_HIP_CHECK(hipMemcpyAsync(l_vector, d_l, 32 * rounds, hipMemcpyDeviceToHost, ds.stream));
  BZ_HIP_CHECK(hipMemcpyAsync(r_vector, d_r, 32 * rounds, hipMemcpyDeviceToHost, ds.stream));
  BZ_HIP_CHECK(hipMemcpyAsync(ap_value, d_ap, 32, hipMemcpyDeviceToHost, ds.stream));
  BZ_HIP_CHECK(hipMemcpyAsync(transcript, d_transcript, sizeof(transcript_state),
                              hipMemcpyDeviceToHost, ds.stream));
  BZ_HIP_CHECK(hipStreamSynchronize(ds.stream));
}

//--------------------------------------------------------------------------------------------------
// the host backend's round loop (reference: prfip::cpu_driver, cpu_driver.cc)
//--------------------------------------------------------------------------------------------------
// current vector shapes: g has `size` entries, a and b have min(size, their original length) --
// only round 0 can be ragged
struct fold_shape {
  u64 size, a_len, b_len;
  u64 mid() const { return size / 2; }
  void advance() {
    size = mid();
    a_len = size;
    b_len = size;
  }
};

class host_fold_backend {
public:
  host_fold_backend(api_state& st, u64 n, u64 np, u64 offset, const u8* a, const u8* b)
      : st_{st}, shape_{np, n, n}, a_(a, a + 32 * n), b_(b, b + 32 * n), g_(np) {
    host_builtin_generators_unlocked(st, g_.data(), np, offset);
  }

  // c_l = <a_lo, b_hi>, c_r = <a_hi, b_lo> (canonical bytes); l_p = <a_lo, g_hi>, r_p = <a_hi, g_lo>
  void commit_to_fold(u8 c_l[32], u8 c_r[32], ed_point& l_p, ed_point& r_p) {
    const u64 mid = shape_.mid();
    inner_product(c_l, a_.data(), b_.data() + 32 * mid, std::min(mid, shape_.b_len - mid));
    inner_product(c_r, a_.data() + 32 * mid, b_.data(), std::min(shape_.a_len - mid, mid));
    l_p = msm(a_.data(), mid, g_.data() + mid);
    r_p = msm(a_.data() + 32 * mid, shape_.a_len - mid, g_.data());
  }

  // a' = x a_lo + x^-1 a_hi; unless one element is left: b' = x^-1 b_lo + x b_hi,
  // g' = x^-1 g_lo + x g_hi
  void fold(const scalar& x, const scalar& x_inv) {
    const u64 mid = shape_.mid();
    fold_scalars(a_, x, x_inv, mid, shape_.a_len);
    if (mid > 1) {
      fold_scalars(b_, x_inv, x, mid, shape_.b_len);
      u8 lo[32], hi[32];
      x_inv.to_bytes(lo);
      x.to_bytes(hi);
      const fold_digits digits = decompose_fold(lo, hi);
      for (u64 i = 0; i < mid; ++i) {
        const ed29_point g_lo = ed29::from_ed(g_[i]), g_hi = ed29::from_ed(g_[mid + i]);
        const ed29_cached terms[3] = {ed29::to_cached(g_lo), ed29::to_cached(g_hi),
                                      ed29::to_cached(ed29::add(g_lo, g_hi))};
        g_[i] = ed29::to_ed(fold_point(digits, [&](u32 k) { return terms[k]; }));
      }
    }
    shape_.advance();
  }

  void first_a(u8 out[32]) { std::memcpy(out, a_.data(), 32); }

private:
  api_state& st_;
  fold_shape shape_;
  std::vector<u8> a_, b_;
  std::vector<ed_point> g_;

  static void inner_product(u8 out[32], const u8* a, const u8* b, u64 count) {
    s25::fe acc = s25::F::zero();
    for (u64 i = 0; i < count; ++i) {
      acc = s25::add(acc, s25::F::mul(s25::load(a + 32 * i), s25::load(b + 32 * i)));
    }
    s25::store(out, s25::F::mul(acc, s25::r2()));
  }
  static void fold_scalars(std::vector<u8>& x, const scalar& m_low, const scalar& m_high, u64 mid,
                           u64 len) {
    for (u64 i = 0; i < mid; ++i) {
      s25::fe r = s25::F::mul(m_low.m, s25::load(x.data() + 32 * i));
      if (mid + i < len) {
        r = s25::add(r, s25::F::mul(m_high.m, s25::load(x.data() + 32 * (mid + i))));
      }
      s25::store(x.data() + 32 * i, r);
    }
  }
  ed_point msm(const u8* scalars, u64 count, const ed_point* generators) {
    ed_point r = ed::identity();
    if (count == 0) return r;
    const std::vector<host_column> cols{byte_column(scalars, count, 32, false)};
    curve25519_vtable().msm_host(reinterpret_cast<u8*>(&r), sizeof(ed_point), true, cols,
                                 generators, false, count);
    return r;
  }
};
} // namespace

void prove_inner_product(api_state& st, u8* l_vector, u8* r_vector, u8* ap_value,
                         void* transcript_bytes, u64 n, u64 generators_offset, const u8* a_vector,
                         const u8* b_vector) {
  if (st.backend == 2 && n > 1) {
    prove_uploaded(st, l_vector, r_vector, ap_value, transcript_bytes, n, generators_offset, a_vector,
                   b_vector);
    return;
  }
  init_transcript<host_sponge>(static_cast<transcript_state*>(transcript_bytes), n);
  if (n == 1) {
    std::memcpy(ap_value, a_vector, 32); // verbatim, as proof_computation.cc:83-86
    return;
  }
  const u64 np = u64{1} << ceil_log2(n);
  ed_point q;
  host_builtin_generators_unlocked(st, &q, 1, generators_offset + np);
  host_fold_backend backend{st, n, np, generators_offset, a_vector, b_vector};
  u64 round = 0;
  for (u64 size = np; size > 1; size /= 2, ++round) {
    u8 c_l[32], c_r[32];
    ed_point l_p, r_p;
    backend.commit_to_fold(c_l, c_r, l_p, r_p);
    l_p = ed::add(l_p, scalar_multiply(q, c_l));
    r_p = ed::add(r_p, scalar_multiply(q, c_r));
    u8* l_value = l_vector + 32 * round;
    u8* r_value = r_vector + 32 * round;
    ristretto::encode(l_value, l_p);
    ristretto::encode(r_value, r_p);
    const scalar x = host_round_challenge(transcript_bytes, l_value, r_value);
    backend.fold(x, x.inverse());
  }
  backend.first_a(ap_value);
}

u64 inner_product_workspace_bytes(u64 n) {
  if (n == 0 || n > (u64{1} << 30)) return 0;
  return workspace_layout{u64{1} << ceil_log2(n)}.total;
}

void prove_inner_product_device(msm_context& ctx, u8* l_vector, u8* r_vector, u8* ap_value,
                                void* transcript, u64 n, u64 generators_offset,
                                const void* generators, const u8* a_vector, const u8* b_vector,
                                void* workspace, u64 workspace_bytes, hipStream_t stream) {
  enqueue_chain(ctx, l_vector, r_vector, ap_value, static_cast<u8*>(transcript), n,
                generators_offset, static_cast<const ed_point*>(generators), a_vector, b_vector,
                workspace, workspace_bytes, stream);
}

//--------------------------------------------------------------------------------------------------
// the verifier's chain, for num_proofs proofs of one length over ONE
// generator set: everything in the caller's workspace as
//   generators  G = [Q | g_0 .. g_{np-1} | (a_commit_i | L_i,0 .. | R_i,0 ..) for i < num_proofs]
//   shared column i   [e_Q,i - product_i | e_i,0 .. e_i,np-1]   at generator offset 0
//   own column i      [1 | x_i,j^2 .. | x_i,j^-2 ..]            at offset np + 1 + i (1 + 2 rounds)
// so that ONE call of the MSM engine with 2 num_proofs columns yields both sides of
//   (e_Q - product) Q + <e, g>  ==  a_commit + sum_j x_j^2 L_j + x_j^-2 R_j,
// the reference's equation with the per-proof terms moved to the right: the big part of G is
// shared by every proof.  Proof i is accepted when its two encodings are equal and every one of its
// L and R decoded.  The single form is the batch of one.
//--------------------------------------------------------------------------------------------------
namespace {
constexpr u32 kMaxRounds = 30; // n <= 2^30
constexpr u32 kMaxProofPartials = 1024; // workgroups of k_verify_expand per proof, at most

// what the challenge kernel leaves for the expansion, and the decode kernel for the verdict; one
// per proof
struct verify_slot {
  s25::fe seed;             // ap prod x_i^-1, plain
  s25::fe x_sq[kMaxRounds]; // Montgomery form
  u32 undecodable[2 * kMaxRounds];
};

// One wavefront per proof (blockIdx.x): the whole transcript of the proof (init, a challenge per
// round, stored back), then lane j < rounds turns x_j into the own column's rows x_j^2 and x_j^-2
// and x_sq[j]; lane 0 multiplies the inverses up into the seed.  The own column's row [1] and
// a_commit's place in G are filled here as well.  rounds = 0 (n = 1): the shared column is
// [b_0 ap - product | ap].  Every operand is read bytewise: the proofs lie back to back.
__global__ void __launch_bounds__(64)
    k_verify_challenges(u8* __restrict__ shared_rows, u8* __restrict__ own_rows,
                        verify_slot* __restrict__ slots, ed_point* __restrict__ g_own,
                        u8* transcripts, const u8* __restrict__ l_vectors,
                        const u8* __restrict__ r_vectors, const u8* __restrict__ ap_values,
                        const u8* __restrict__ products, const u8* __restrict__ b_vectors,
                        const u8* __restrict__ a_commits, u64 n, u32 rounds) {
  __shared__ wave_state w;
  __shared__ s25::fe inverses[kMaxRounds];
  const u32 lane = threadIdx.x;
  const u64 proof = blockIdx.x;
  const u64 np = u64{1} << rounds;
  u8* transcript = transcripts + sizeof(transcript_state) * proof;
  const u8* l_vector = l_vectors + 32 * rounds * proof;
  const u8* r_vector = r_vectors + 32 * rounds * proof;
  verify_slot* slot = slots + proof;
  u8* own = own_rows + 32 * (1 + 2 * u64{rounds}) * proof;
  u8* shared = shared_rows + 32 * (np + 1) * proof;

  wave_load_transcript(w.t, transcript);
  init_transcript<wave_sponge>(&w.t, n);
  s25::fe mine = s25::F::zero();
  for (u32 i = 0; i < rounds; ++i) {
    if (lane < 32) {
      w.l[lane] = l_vector[32 * i + lane];
      w.r[lane] = r_vector[32 * i + lane];
    }
    wave_sponge::sync();
    const s25::fe x = round_challenge<wave_sponge>(w.x, &w.t, w.l, w.r);
    if (lane == i) mine = x;
  }
  wave_store_transcript(transcript, w.t);

  if (lane < 32) own[lane] = lane == 0 ? 1 : 0;
  {
    u8* to = reinterpret_cast<u8*>(g_own + (1 + 2 * u64{rounds}) * proof);
    const u8* from = a_commits + sizeof(ed_point) * proof;
    for (u32 i = lane; i < sizeof(ed_point); i += 64) to[i] = from[i];
  }
  const s25::fe ap = s25::load(ap_values + 32 * proof);
  if (rounds == 0) {
    if (lane == 0) {
      const s25::fe product = s25::from_mont(s25::to_mont(s25::load(products + 32 * proof)));
      const s25::fe e_q = s25::F::mul(s25::to_mont(s25::load(b_vectors + 32 * proof)), ap);
      s25::store(shared, s25::add(e_q, s25::neg(product)));
      s25::store(shared + 32, s25::from_mont(s25::to_mont(ap)));
    }
    return;
  }
  if (lane < rounds) {
    const s25::fe x_inv = s25::F::invert(mine); // zero for zero, as scalar::inverse
    const s25::fe x_sq = s25::F::mul(mine, mine);
    s25::store(own + 32 * (1 + lane), s25::from_mont(x_sq));
    s25::store(own + 32 * (1 + rounds + lane), s25::from_mont(s25::F::mul(x_inv, x_inv)));
    slot->x_sq[lane] = x_sq;
    inverses[lane] = x_inv;
  }
  wave_sponge::sync();
  if (lane == 0) {
    s25::fe all = inverses[0];
    for (u32 i = 1; i < rounds; ++i) all = s25::F::mul(all, inverses[i]);
    slot->seed = s25::F::mul(all, ap); // Montgomery form times plain: plain
  }
}

// One lane per L / R point of the batch, 2 rounds of them per proof: its place in G = the decoded
// point, or the identity and a raised flag for an encoding ristretto::decode rejects -- the chain
// runs on whatever the proofs hold
__global__ void __launch_bounds__(256)
    k_verify_decode(ed_point* __restrict__ g_own, verify_slot* __restrict__ slots,
                    const u8* __restrict__ l_vectors, const u8* __restrict__ r_vectors, u32 rounds,
                    u32 num_proofs) {
  const u64 at = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (at >= 2 * u64{rounds} * num_proofs) return;
  const u64 proof = at / (2 * rounds);
  const u32 i = static_cast<u32>(at % (2 * rounds));
  const u8* bytes = i < rounds ? l_vectors + 32 * (rounds * proof + i)
                               : r_vectors + 32 * (rounds * proof + (i - rounds));
  ed_point p;
  const bool ok = ristretto29::decode(p, bytes);
  g_own[(1 + 2 * u64{rounds}) * proof + 1 + i] = ok ? p : ed::identity();
  slots[proof].undecodable[i] = ok ? 0 : 1;
}

// the caller's np + 1 generators, the last one Q, into [Q | g_0 .. g_{np-1}]; by words where the
// caller's pointer allows it
__global__ void __launch_bounds__(256)
    k_verify_generators(ed_point* __restrict__ g, const u8* __restrict__ generators, u32 np) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > np) return;
  const u8* from = generators + sizeof(ed_point) * static_cast<u64>(i);
  ed_point* to = g + (i == np ? 0 : i + 1);
  if ((reinterpret_cast<uintptr_t>(generators) & 7) == 0) {
    *to = *reinterpret_cast<const ed_point*>(from);
  } else {
    u8* bytes = reinterpret_cast<u8*>(to);
    for (u32 k = 0; k < sizeof(ed_point); ++k) bytes[k] = from[k];
  }
}

// The expansion fused with <e, b>:
//   e_k = seed prod_{j : bit j of k set} x_sq[rounds - 1 - j],  k < np,
// the closed form of the reference's doubling loop (verification_computation.cc:77-91).  A lane
// writes the canonical row of its e_k into the proof's shared column and, for k < n, multiplies it
// by b_k while it holds it; the workgroup adds the products up (LDS tree) into one partial.
//
// (proof, k) to lanes, rounds >= 1:
//   np >= 256: a proof has `partials` = np / (256 items) workgroups, items = max(1, np / 2^18), so
//     that no proof has more than kMaxProofPartials partials; workgroup blockIdx.x works for proof
//     blockIdx.x / partials on the rows [(chunk items + t) 256 + lane, t < items): coalesced.
//   np < 256: the flat index proof np + k is cut into workgroups, 256 / np whole proofs each, so
//     that a batch of short proofs fills its workgroups; the tree stops at the proof's np lanes.
// b is read by words where the caller's pointer is 8-byte aligned (32 n i keeps that), bytewise
// otherwise.
__global__ void __launch_bounds__(256)
    k_verify_expand(u8* __restrict__ shared_rows, s25::fe* __restrict__ partials,
                    const verify_slot* __restrict__ slots, const u8* __restrict__ b_vectors, u32 n,
                    u32 rounds, u32 items, u32 proof_partials, u32 num_proofs) {
  __shared__ s25::fe x_sq[128]; // np < 256: (256 >> rounds) rounds <= 128; else rounds <= 30
  __shared__ s25::fe tree[256];
  const u32 np = 1u << rounds;
  const u32 lanes = np < 256 ? np : 256; // of one proof in this workgroup
  const u32 proofs_here = 256 / lanes;
  const u32 local = threadIdx.x / lanes;
  u32 first, chunk;
  if (np < 256) {
    first = blockIdx.x * proofs_here;
    chunk = 0;
  } else {
    first = blockIdx.x / proof_partials;
    chunk = blockIdx.x % proof_partials;
  }
  if (threadIdx.x < proofs_here * rounds) {
    const u32 p = first + threadIdx.x / rounds;
    if (p < num_proofs) x_sq[threadIdx.x] = slots[p].x_sq[threadIdx.x % rounds];
  }
  __syncthreads();
  const u32 proof = first + local;
  s25::fe sum = s25::F::zero();
  if (proof < num_proofs) {
    const s25::fe seed = slots[proof].seed;
    const s25::fe* mine = x_sq + local * rounds;
    u64* rows = reinterpret_cast<u64*>(shared_rows + 32 * (static_cast<u64>(np) + 1) * proof + 32);
    const u8* b = b_vectors + 32 * static_cast<u64>(n) * proof;
    const bool aligned = (reinterpret_cast<uintptr_t>(b_vectors) & 7) == 0;
    for (u32 t = 0; t < items; ++t) {
      const u32 k = (chunk * items + t) * 256 + (threadIdx.x & (lanes - 1));
      s25::fe e = seed;
      for (u32 j = 0; j < rounds; ++j) {
        if ((k >> j) & 1) e = s25::F::mul(mine[rounds - 1 - j], e);
      }
      u64 words[4];
      s25::store_words(words, e);
      for (int q = 0; q < 4; ++q) rows[4 * static_cast<u64>(k) + q] = words[q];
      if (k < n) {
        const u8* at = b + 32 * static_cast<u64>(k);
        const s25::fe b_k =
            aligned ? s25::load_words(reinterpret_cast<const u64*>(at)) : s25::load(at);
        sum = s25::add(sum, s25::F::mul(e, b_k));
      }
    }
  }
  tree[threadIdx.x] = sum;
  __syncthreads();
  for (u32 stride = lanes / 2; stride > 0; stride >>= 1) {
    if ((threadIdx.x & (lanes - 1)) < stride) {
      tree[threadIdx.x] = s25::add(tree[threadIdx.x], tree[threadIdx.x + stride]);
    }
    __syncthreads();
  }
  if ((threadIdx.x & (lanes - 1)) == 0 && proof < num_proofs) {
    partials[static_cast<u64>(proof) * proof_partials + chunk] = tree[threadIdx.x];
  }
}

// One wavefront per proof: e_Q - product (canonical) from the proof's partials (sums of e_k b_k / R)
// into row 0 of its shared column
__global__ void __launch_bounds__(64)
    k_verify_finish(u8* __restrict__ shared_rows, const s25::fe* __restrict__ partials,
                    const u8* __restrict__ products, u32 proof_partials, u32 np) {
  __shared__ s25::fe tree[64];
  const u64 proof = blockIdx.x;
  s25::fe sum = s25::F::zero();
  for (u32 t = threadIdx.x; t < proof_partials; t += 64) {
    sum = s25::add(sum, partials[proof * proof_partials + t]);
  }
  tree[threadIdx.x] = sum;
  __syncthreads();
  for (u32 stride = 32; stride > 0; stride >>= 1) {
    if (threadIdx.x < stride) {
      tree[threadIdx.x] = s25::add(tree[threadIdx.x], tree[threadIdx.x + stride]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const s25::fe product = s25::from_mont(s25::to_mont(s25::load(products + 32 * proof)));
    const s25::fe e_q = s25::F::mul(tree[0], s25::r2());
    s25::store(shared_rows + 32 * (static_cast<u64>(np) + 1) * proof,
               s25::add(e_q, s25::neg(product)));
  }
}

// One wavefront per proof, four to a workgroup: accepted when the engine's two encodings of the
// proof are equal and none of its points failed to decode.  The word is stored bytewise: verdicts
// need no alignment.
__global__ void __launch_bounds__(256)
    k_verify_verdict(u8* __restrict__ verdicts, const u8* __restrict__ encodings,
                     const verify_slot* __restrict__ slots, u32 rounds, u32 num_proofs) {
  const u32 lane = threadIdx.x & 63;
  const u32 proof = blockIdx.x * 4 + threadIdx.x / 64;
  if (proof >= num_proofs) return; // the whole wavefront
  bool ok = true;
  if (lane < 32) {
    ok = encodings[32 * static_cast<u64>(proof) + lane] ==
         encodings[32 * (static_cast<u64>(num_proofs) + proof) + lane];
  }
  if (lane < 2 * rounds) ok = ok && slots[proof].undecodable[lane] == 0;
  const bool all = __all(ok) != 0;
  if (lane < 4) verdicts[4 * static_cast<u64>(proof) + lane] = lane == 0 && all ? 1 : 0;
}

// the caller's workspace of the batch verifier, for np = 2^rounds
struct verify_batch_layout {
  size_t generators, shared_rows, own_rows, partials, slots, encodings, total;
  u32 items, proof_partials; // k_verify_expand's geometry
  verify_batch_layout(u64 np, u64 rounds, u64 num_proofs) {
    items = static_cast<u32>(std::max<u64>(1, np / (256 * u64{kMaxProofPartials})));
    proof_partials = np < 256 ? 1 : static_cast<u32>(np / (256 * u64{items}));
    workspace_carver carve;
    generators = carve.take(sizeof(ed_point) * (np + 1 + num_proofs * (1 + 2 * rounds)));
    shared_rows = carve.take(32 * (np + 1) * num_proofs);
    own_rows = carve.take(32 * (1 + 2 * rounds) * num_proofs);
    partials = carve.take(sizeof(s25::fe) * proof_partials * num_proofs);
    slots = carve.take(sizeof(verify_slot) * num_proofs);
    encodings = carve.take(64 * num_proofs);
    total = carve.total();
  }
};

// the single form's workspace, as it was before it became the batch of one (a b copy beside the
// exponents); the batch of one fits into it at every np, which the chain asserts
struct verify_layout {
  size_t total;
  verify_layout(u64 np, u64 rounds) {
    workspace_carver carve;
    carve.take(sizeof(ed_point) * (2 + np + 2 * rounds));
    carve.take(32 * (3 + np + 2 * rounds));
    carve.take(32 * np);
    carve.take(sizeof(s25::fe) * kPartialBlocks);
    carve.take(sizeof(verify_slot));
    carve.take(64);
    total = carve.total();
  }
};

bool verify_batch_in_limits(u64 n, u64 num_proofs) {
  if (n == 0 || n > (u64{1} << 30) || num_proofs == 0 || num_proofs > (u64{1} << 28)) return false;
  return num_proofs * (u64{1} << ceil_log2(n)) <= (u64{1} << 28);
}

void enqueue_verify_chain(msm_context& ctx, u8* verdicts, u8* transcripts, u64 n, u64 num_proofs,
                          u64 generators_offset, const u8* generators, const u8* b_vectors,
                          const u8* products, const u8* a_commits, const u8* l_vectors,
                          const u8* r_vectors, const u8* ap_values, void* workspace,
                          u64 workspace_bytes, hipStream_t stream) {
  const u64 rounds = ceil_log2(n), np = u64{1} << rounds;
  const verify_batch_layout layout{np, rounds, num_proofs};
  BZ_RELEASE_ASSERT(workspace != nullptr && workspace_bytes >= layout.total,
                    "the inner-product verifier's workspace is too small");
  u8* base = workspace_carver::aligned(workspace);
  ed_point* d_g = reinterpret_cast<ed_point*>(base + layout.generators);
  ed_point* d_g_own = d_g + np + 1;
  u8* d_shared = base + layout.shared_rows;
  u8* d_own = base + layout.own_rows;
  auto* d_partials = reinterpret_cast<s25::fe*>(base + layout.partials);
  auto* d_slots = reinterpret_cast<verify_slot*>(base + layout.slots);
  u8* d_encodings = base + layout.encodings;
  const u32 proofs = static_cast<u32>(num_proofs), r = static_cast<u32>(rounds);
  const u64 own_rows = 1 + 2 * rounds;

  // G: nothing here depends on the challenges, and [Q | g] is written once for the batch
  if (generators == nullptr) {
    builtin_generators_enqueue(d_g, generators_offset + np, 1, stream);
    builtin_generators_enqueue(d_g + 1, generators_offset, np, stream);
    g_kernel_launches += 2;
  } else {
    hipLaunchKernelGGL(k_verify_generators, dim3(static_cast<u32>((np + 256) / 256)), dim3(256), 0,
                       stream, d_g, generators, static_cast<u32>(np));
    g_kernel_launches += 1;
  }
  if (rounds != 0) {
    hipLaunchKernelGGL(k_verify_decode, dim3(static_cast<u32>((2 * rounds * num_proofs + 255) / 256)),
                       dim3(256), 0, stream, d_g_own, d_slots, l_vectors, r_vectors, r, proofs);
    g_kernel_launches += 1;
  }
  hipLaunchKernelGGL(k_verify_challenges, dim3(proofs), dim3(64), 0, stream, d_shared, d_own,
                     d_slots, d_g_own, transcripts, l_vectors, r_vectors, ap_values, products,
                     b_vectors, a_commits, n, r);
  g_kernel_launches += 1;
  if (rounds != 0) {
    const u64 blocks = np < 256 ? (num_proofs * np + 255) / 256 : num_proofs * layout.proof_partials;
    hipLaunchKernelGGL(k_verify_expand, dim3(static_cast<u32>(blocks)), dim3(256), 0, stream,
                       d_shared, d_partials, d_slots, b_vectors, static_cast<u32>(n), r, layout.items,
                       layout.proof_partials, proofs);
    hipLaunchKernelGGL(k_verify_finish, dim3(proofs), dim3(64), 0, stream, d_shared, d_partials,
                       products, layout.proof_partials, static_cast<u32>(np));
    g_kernel_launches += 2;
  }
  BZ_HIP_CHECK(hipGetLastError());
  // shared columns first, then own columns: encodings[i] against encodings[num_proofs + i].  The
  // engine cuts a call into batches of its own where the columns exceed a launch grid.
  std::vector<host_column> cols(2 * num_proofs);
  for (u64 i = 0; i < num_proofs; ++i) {
    cols[i] = byte_column(d_shared + 32 * (np + 1) * i, np + 1, 32, false);
    cols[num_proofs + i] = byte_column(d_own + 32 * own_rows * i, own_rows, 32, false);
    cols[num_proofs + i].generator_offset = np + 1 + own_rows * i;
  }
  curve25519_vtable().msm(ctx, d_encodings, 32, false, cols, nullptr, d_g, stream, false);
  hipLaunchKernelGGL(k_verify_verdict, dim3((proofs + 3) / 4), dim3(256), 0, stream, verdicts,
                     d_encodings, d_slots, r, proofs);
  BZ_HIP_CHECK(hipGetLastError());
  g_kernel_launches += 1;
}

} // namespace

u64 inner_product_verify_workspace_bytes(u64 n) {
  if (n == 0 || n > (u64{1} << 30)) return 0;
  const u64 rounds = ceil_log2(n);
  return verify_layout{u64{1} << rounds, rounds}.total;
}

u64 inner_product_verify_batch_workspace_bytes(u64 n, u64 num_proofs) {
  if (!verify_batch_in_limits(n, num_proofs)) return 0;
  const u64 rounds = ceil_log2(n);
  return verify_batch_layout{u64{1} << rounds, rounds, num_proofs}.total;
}

void verify_inner_product_device(msm_context& ctx, void* verdict, void* transcript, u64 n,
                                 u64 generators_offset, const void* generators, const u8* b_vector,
                                 const u8* product, const void* a_commit, const u8* l_vector,
                                 const u8* r_vector, const u8* ap_value, void* workspace,
                                 u64 workspace_bytes, hipStream_t stream) {
  // the batch of one, in the workspace this entry point has always asked for
  BZ_RELEASE_ASSERT(workspace != nullptr &&
                        workspace_bytes >= inner_product_verify_workspace_bytes(n),
                    "the inner-product verifier's workspace is too small");
  enqueue_verify_chain(ctx, static_cast<u8*>(verdict), static_cast<u8*>(transcript), n, 1,
                       generators_offset, static_cast<const u8*>(generators), b_vector, product,
                       static_cast<const u8*>(a_commit), l_vector, r_vector, ap_value, workspace,
                       workspace_bytes, stream);
}

void verify_inner_product_batch_device(msm_context& ctx, void* verdicts, void* transcripts, u64 n,
                                       u64 num_proofs, u64 generators_offset,
                                       const void* generators, const u8* b_vectors,
                                       const u8* products, const void* a_commits,
                                       const u8* l_vectors, const u8* r_vectors,
                                       const u8* ap_values, void* workspace, u64 workspace_bytes,
                                       hipStream_t stream) {
  BZ_RELEASE_ASSERT(verify_batch_in_limits(n, num_proofs),
                    "1 <= n <= 2^30, 1 <= num_proofs and num_proofs x np <= 2^28");
  enqueue_verify_chain(ctx, static_cast<u8*>(verdicts), static_cast<u8*>(transcripts), n, num_proofs,
                       generators_offset, static_cast<const u8*>(generators), b_vectors, products,
                       static_cast<const u8*>(a_commits), l_vectors, r_vectors, ap_values, workspace,
                       workspace_bytes, stream);
}

bool verify_inner_product(api_state& st, void* transcript_bytes, u64 n, u64 generators_offset,
                          const u8* b_vector, const u8* product, const void* a_commit,
                          const u8* l_vector, const u8* r_vector, const u8* ap_value) {
  const u64 rounds = ceil_log2(n), np = u64{1} << rounds;
  init_transcript<host_sponge>(static_cast<transcript_state*>(transcript_bytes), n);
  std::vector<scalar> x(rounds);
  for (u64 i = 0; i < rounds; ++i) {
    x[i] = host_round_challenge(transcript_bytes, l_vector + 32 * i, r_vector + 32 * i);
  }

  // exponents of [Q, g_0 .. g_{np-1}, L_0 .., R_0 ..] (verification_computation.cc:30-121)
  const u64 count = 1 + np + 2 * rounds;
  std::vector<u8> exponents(32 * count);
  const scalar ap = scalar::from_bytes(ap_value);
  std::vector<scalar> g_exponents(np);
  if (n == 1) {
    (scalar::from_bytes(b_vector) * ap).to_bytes(exponents.data());
    g_exponents[0] = ap;
  } else {
    std::vector<scalar> x_sq(rounds);
    scalar all_inv = x[0].inverse();
    x_sq[0] = x[0] * x[0];
    (-(all_inv * all_inv)).to_bytes(exponents.data() + 32 * (1 + np + rounds));
    for (u64 i = 1; i < rounds; ++i) {
      const scalar xi_inv = x[i].inverse();
      all_inv = all_inv * xi_inv;
      x_sq[i] = x[i] * x[i];
      (-(xi_inv * xi_inv)).to_bytes(exponents.data() + 32 * (1 + np + rounds + i));
    }
    g_exponents[0] = all_inv * ap;
    u64 a = 1, b = 2, next = rounds;
    while (a != np) {
      const scalar multiplier = x_sq[--next];
      for (u64 i = a; i < b; ++i) g_exponents[i] = multiplier * g_exponents[i - a];
      a = b;
      b = 2 * a;
    }
    s25::fe acc = s25::F::zero(); // <g_exponents, b> over the n entries of b
    for (u64 i = 0; i < n; ++i) {
      acc = s25::add(acc, s25::F::mul(g_exponents[i].m, s25::load(b_vector + 32 * i)));
    }
    s25::store(exponents.data(), acc);
    for (u64 i = 0; i < rounds; ++i) (-x_sq[i]).to_bytes(exponents.data() + 32 * (1 + np + i));
  }
  for (u64 i = 0; i < np; ++i) g_exponents[i].to_bytes(exponents.data() + 32 * (1 + i));

  std::vector<ed_point> generators(count);
  host_builtin_generators_unlocked(st, generators.data(), 1, generators_offset + np);
  host_builtin_generators_unlocked(st, generators.data() + 1, np, generators_offset);
  for (u64 i = 0; i < rounds; ++i) {
    // an invalid encoding cannot be part of a valid proof
    if (!ristretto::decode(generators[1 + np + i], l_vector + 32 * i)) return false;
    if (!ristretto::decode(generators[1 + np + rounds + i], r_vector + 32 * i)) return false;
  }
  u8 expected[32], commit[32];
  commit_column_unlocked(st, expected, exponents.data(), count, generators.data());
  // product * Q + a_commit (proof_computation.cc:146-153)
  ed_point a_point;
  std::memcpy(&a_point, a_commit, sizeof(a_point));
  ristretto::encode(commit, ed::add(scalar_multiply(generators[0], product), a_point));
  return std::memcmp(commit, expected, 32) == 0;
}
} // namespace bz::proof
