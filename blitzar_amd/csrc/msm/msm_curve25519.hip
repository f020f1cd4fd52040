// gfx950 code object for the curve25519 MSM kernels (see curve_tu.h / kernels.h).
#include "blitzar_amd/csrc/msm/curve_tu.h"

namespace bz {
BZ_ACCUMULATE_INSTANCE(extern, ed25519_msm); // msm_curve25519_accumulate.hip
BZ_ACCUMULATE_INSTANCE(extern, ed25519_niels_msm); // msm_curve25519_niels_accumulate.hip
// Caller generators that are converted on every call keep the projective (Y+X, Y-X, Z, 2dT)
// addends: normalising a whole array to Z = 1 per call (k_prepare_addends_batched, one shared
// inversion per 1024 generators) makes k_accumulate 8 % faster (0.72 -> 0.66 ms at config 2) but the
// shared inversion is a 50-80 us dependent chain that every workgroup of the launch waits for at the
// same time: +0.25 ms of prepare, only partly hidden beside recode + sort (measured A/B on MI355X,
// profiles/round2_ab.md: 1.90 -> 1.79 ms with, 1.70 ms without the normalisation on the same kind of
// box).  What is normalised once is kept in the Z = 1 form: resident generator sets (the batched
// kernel) and the caller table of a keyed pointer, whose tiles are normalised when their bytes
// change (k_prepare_addends_staged<ed25519_niels_msm, true>; curve_tu.h, msm).
const curve_vtable& curve25519_vtable() { return curve_tu<ed25519_msm, ed25519_niels_msm, ed25519_msm>::vtable(); }
} // namespace bz
