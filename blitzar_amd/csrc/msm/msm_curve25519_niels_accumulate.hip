// gfx950 code object of k_accumulate for curve25519 generators in their Z = 1 form (resident sets,
// built-in generators, fixed-base handles, caller tables): a translation unit of its own because
// this loop, unlike the 8-product one, fits three waves per SIMD under the iterative-ilp scheduling
// strategy.  Its rows arrive by wavefront through LDS (kernels.h, accumulate_lds_gather) and are
// stored halved (curve/ed29.h, add_niels): 164 VGPRs, no spill, 28 672 bytes of LDS per workgroup,
// 1188 instructions per addition of which 52 s_nop (blitzar_amd/build.py, TU_FLAGS;
// tests/test_accumulate_lds_gather_resources.py).  The kernel holds the loop twice, with 32-bit and
// with 64-bit piece offsets; the counts are those of the 32-bit copy.
#include "blitzar_amd/csrc/msm/curve_traits.h"
#include "blitzar_amd/csrc/msm/kernels.h"

namespace bz {
BZ_ACCUMULATE_INSTANCE(, ed25519_niels_msm);
} // namespace bz
