// Native driver of the caller tables (include/blitzar_amd.h: bzamd_prepare_tiles_converted) for A/B
// runs on the GPU box, in the manner of pipeline_bench.cc: a sequence of bzamd_msm_device calls in
// throughput mode, one 32-byte column of 2^log2n 252-bit scalars against curve25519 caller
// generators, in two legs:
//
//   same       every call reads the same generator array (a service's case: after the first call
//              nothing is converted);
//   alternate  before every call the array is overwritten, on the caller's stream, with the other of
//              two generator sets (the built-in sequence from 0 and from n): every tile changes every
//              time, so every call hashes AND converts -- the table's worst case.  The copy is part of
//              the step in both builds.
//
//   caller_table_bench [--log2n 20] [--steps 200] [--warmup 10]
//
// Prints one JSON line per leg: ms per step, tiles converted during the timed steps (-1 with a
// library that has no counter: the driver runs against older builds for the comparison) and a hash
// of the commitments (the legs of two builds must print the same hashes).
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "blitzar_amd.h"

#define CHECK(expr)                                                                      \
  do {                                                                                   \
    hipError_t e__ = (expr);                                                             \
    if (e__ != hipSuccess) {                                                             \
      std::fprintf(stderr, "%s failed: %s\n", #expr, hipGetErrorString(e__));            \
      std::exit(2);                                                                      \
    }                                                                                    \
  } while (0)

static double now_ms() {
  using clock = std::chrono::steady_clock;
  return std::chrono::duration<double, std::milli>(clock::now().time_since_epoch()).count();
}

int main(int argc, char** argv) {
  unsigned log2n = 20, steps = 200, warmup = 10;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    auto next = [&] { return static_cast<unsigned>(std::atoi(argv[++i])); };
    if (a == "--log2n") log2n = next();
    else if (a == "--steps") steps = next();
    else if (a == "--warmup") warmup = next();
    else {
      std::fprintf(stderr, "unknown argument %s\n", a.c_str());
      return 2;
    }
  }
  const uint64_t n = uint64_t{1} << log2n;
  const sxt_config config{SXT_GPU_BACKEND, 0};
  if (sxt_init(&config) != 0) return 2;
  using counter_fn = uint64_t (*)();
  const counter_fn converted =
      reinterpret_cast<counter_fn>(dlsym(RTLD_DEFAULT, "bzamd_prepare_tiles_converted"));
  hipStream_t stream = nullptr;
  CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));

  std::vector<uint8_t> host(n * 32);
  uint64_t x = 0x9e3779b97f4a7c15ull;
  for (size_t i = 0; i + 8 <= host.size(); i += 8) {
    x ^= x >> 12; x ^= x << 25; x ^= x >> 27;
    const uint64_t v = x * 0x2545f4914f6cdd1dull;
    std::memcpy(&host[i], &v, 8);
  }
  for (size_t r = 0; r < n; ++r) host[r * 32 + 31] &= 0x0f;
  uint8_t* d_scalars = nullptr;
  CHECK(hipMalloc(&d_scalars, host.size()));
  CHECK(hipMemcpy(d_scalars, host.data(), host.size(), hipMemcpyHostToDevice));
  const size_t gen_bytes = 160 * n;
  uint8_t *d_sets[2] = {nullptr, nullptr}, *d_gens = nullptr;
  for (int k = 0; k < 2; ++k) {
    CHECK(hipMalloc(&d_sets[k], gen_bytes));
    bzamd_ristretto255_generators_device(reinterpret_cast<sxt_ristretto255*>(d_sets[k]), k * n, n,
                                         stream);
  }
  CHECK(hipMalloc(&d_gens, gen_bytes));
  CHECK(hipMemcpyAsync(d_gens, d_sets[0], gen_bytes, hipMemcpyDeviceToDevice, stream));
  CHECK(hipStreamSynchronize(stream));
  const sxt_sequence_descriptor desc{32, n, d_scalars, 0};
  const unsigned slots = steps > warmup ? steps : warmup;
  uint8_t* d_out = nullptr;
  CHECK(hipMalloc(&d_out, 32 * slots));
  std::vector<uint8_t> outs(32 * slots);

  int rc = 0;
  for (int leg = 0; leg < 2; ++leg) {
    const bool alternate = leg == 1;
    unsigned turn = 0;
    auto run = [&](unsigned count) {
      for (unsigned k = 0; k < count; ++k, ++turn) {
        if (alternate) {
          CHECK(hipMemcpyAsync(d_gens, d_sets[turn & 1], gen_bytes, hipMemcpyDeviceToDevice, stream));
        }
        bzamd_pipeline_next();
        bzamd_msm_device(0, d_out + 32 * k, 1, &desc, d_gens, stream);
      }
      bzamd_pipeline_flush(stream);
      CHECK(hipDeviceSynchronize());
    };
    CHECK(hipMemset(d_out, 0, 32 * slots));
    run(warmup + (warmup & 1)); // (an even count: the timed steps start at set 0 again)
    const uint64_t before = converted != nullptr ? converted() : 0;
    const double t0 = now_ms();
    run(steps);
    const double ms = (now_ms() - t0) / steps;
    const long long tiles = converted != nullptr ? static_cast<long long>(converted() - before) : -1;
    CHECK(hipMemcpy(outs.data(), d_out, outs.size(), hipMemcpyDeviceToHost));
    // same: every step commits to set 0; alternate: even steps to set 0, odd steps to set 1
    bool agree = true;
    for (unsigned k = 2; k < steps; ++k) {
      agree = agree && std::memcmp(&outs[32 * k], &outs[32 * (alternate ? k & 1 : 0)], 32) == 0;
    }
    agree = agree && (steps < 2 || (std::memcmp(&outs[0], &outs[32], 32) == 0) == !alternate);
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < 64 && i < outs.size(); ++i) h = (h ^ outs[i]) * 0x100000001b3ull;
    std::printf("{\"leg\": \"%s\", \"log2n\": %u, \"steps\": %u, \"ms_per_step\": %.4f, "
                "\"tiles_converted\": %lld, \"outputs_agree\": %s, \"hash\": \"%016llx\"}\n",
                alternate ? "alternate" : "same", log2n, steps, ms, tiles, agree ? "true" : "false",
                static_cast<unsigned long long>(h));
    std::fflush(stdout);
    if (!agree) rc = 1;
    // (leave set 0 in the array for the next leg)
    CHECK(hipMemcpy(d_gens, d_sets[0], gen_bytes, hipMemcpyDeviceToDevice));
  }
  return rc;
}
