// What the proof operations on host operands share (proof/column_inverse.hip, multiplicities.hip,
// word_columns.hip, mle_opening.hip, univariate_opening.hip, sumcheck_transcript.hip): the overlap
// test of their argument checks, and the staging of a blocking call on the GPU backend.  Such a
// call declares its buffers, allocates once, enqueues its device form on the staged pointers and
// finishes:
//
//   host_call call{st};
//   call.input(&d_point, point, point_bytes);
//   call.output(&d_vector, vector, vector_bytes);
//   call.allocate();                               // one allocation, the uploads
//   evaluation_vector_enqueue<E>(d_vector, d_point, ..., call.stream());
//   call.finish();                                 // the downloads, one synchronise, the free
//
// Every buffer lies at a multiple of 256 bytes of the allocation, in the order of the declarations;
// uploads and downloads run in that order too.  The declaration decides what is copied and what a
// null operand means; no caller adds up sizes.
#pragma once

#include <vector>

#include "blitzar_amd/csrc/proof/sumcheck.h"

namespace bz::proof {
struct byte_range {
  const void* at;
  u64 bytes;
};
inline bool overlap(const byte_range& a, const byte_range& b) {
  if (a.at == nullptr || b.at == nullptr || a.bytes == 0 || b.bytes == 0) return false;
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a.at), b0 = reinterpret_cast<uintptr_t>(b.at);
  return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

class host_call {
public:
  // on the primary device, which becomes the current one
  explicit host_call(api_state& st) : stream_{st.primary().stream} {
    BZ_HIP_CHECK(hipSetDevice(st.primary().device));
  }
  host_call(const host_call&) = delete;
  host_call& operator=(const host_call&) = delete;
  ~host_call() {
    if (base_ != nullptr) (void)hipFree(base_);
  }

  // Declarations: `*slot` (a pointer of any type) holds the device pointer once allocate() has run;
  // a slot that stays null is null at once.
  // uploaded; a null `host` has no memory and a null pointer
  template <class P> void input(P* slot, const void* host, size_t bytes) {
    if (host == nullptr) {
      *slot = nullptr;
    } else {
      declare(slot, bytes, host, nullptr);
    }
  }
  // downloaded by finish(); a null `host` has a null pointer and no download, but keeps its place:
  // what a call allocates depends on its shapes alone, not on which results are asked for
  template <class P> void output(P* slot, void* host, size_t bytes) {
    if (host == nullptr) {
      *slot = nullptr;
      (void)carve_.take(bytes);
    } else {
      declare(slot, bytes, nullptr, host);
    }
  }
  // uploaded, and downloaded by finish()
  template <class P> void in_out(P* slot, void* host, size_t bytes) {
    declare(slot, bytes, host, host);
  }
  // neither
  template <class P> void scratch(P* slot, size_t bytes) { declare(slot, bytes, nullptr, nullptr); }
  // *staged = the `count` columns with `data` at copies of their own width; a column of no rows has
  // a pointer of its own and no copy.  `staged` must not change its size afterwards.
  void columns(std::vector<sumcheck_column>* staged, const sumcheck_column* columns, u32 count) {
    staged->assign(columns, columns + count);
    for (sumcheck_column& c : *staged) declare(&c.data, c.n * c.nbytes, c.data, nullptr);
  }

  // one allocation for everything declared, then the uploads
  void allocate() {
    BZ_HIP_CHECK(hipMalloc(&base_, carve_.end()));
    for (const buffer& b : buffers_) {
      b.set(b.slot, static_cast<u8*>(base_) + b.offset);
      if (b.from != nullptr && b.bytes != 0) {
        BZ_HIP_CHECK(hipMemcpyAsync(static_cast<u8*>(base_) + b.offset, b.from, b.bytes,
                                    hipMemcpyHostToDevice, stream_));
      }
    }
  }
  // the sum of the declared buffers, each padded to a multiple of 256: what allocate() asks for
  size_t bytes() const { return carve_.end(); }
  hipStream_t stream() const { return stream_; }

  // the downloads, one synchronise, the memory given back
  void finish() {
    for (const buffer& b : buffers_) {
      if (b.to != nullptr && b.bytes != 0) {
        BZ_HIP_CHECK(hipMemcpyAsync(b.to, static_cast<const u8*>(base_) + b.offset, b.bytes,
                                    hipMemcpyDeviceToHost, stream_));
      }
    }
    BZ_HIP_CHECK(hipStreamSynchronize(stream_));
    BZ_HIP_CHECK(hipFree(base_));
    base_ = nullptr;
  }

private:
  struct buffer {
    void* slot;
    void (*set)(void* slot, u8* at);
    size_t offset, bytes;
    const void* from; // host memory to upload, or null
    void* to;         // host memory to download to, or null
  };
  template <class P> void declare(P* slot, size_t bytes, const void* from, void* to) {
    buffers_.push_back({slot, [](void* s, u8* at) { *static_cast<P*>(s) = reinterpret_cast<P>(at); },
                        carve_.take(bytes), bytes, from, to});
  }

  hipStream_t stream_;
  workspace_carver carve_;
  std::vector<buffer> buffers_;
  void* base_ = nullptr;
};
} // namespace bz::proof
