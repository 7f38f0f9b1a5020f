// The instantiations of prop_pool_kernel without STOP_PHOTONS_ON_DETECTION (prop_pool_kernel.hip.h: KEEP = true,
// SetStopDetectedPhotons(false) -- the reference class's default, OpenCL.cxx:86) as a translation unit of their own: compiled in
// parallel with the others and with the same code generation (Makefile: POOL_CODEGEN).
#include "prop_pool_kernel.hip.h"

namespace clsimhip {

hipError_t launch_pool_keep_kernel(const KParams &P, const KVariant &v, hipStream_t stream)
{
    if (P.n_steps == 0) return hipSuccess;
    if (check_lengths(P, v) != hipSuccess) return hipErrorInvalidValue;
    if (P.history_n != 0 || v.tabulate || !v.keep_detected) return hipErrorInvalidValue;
    if (P.num_layers >= (1 << 14)) return hipErrorInvalidValue;          // (a ring entry keeps the carried layer index in 14 bits: pool_kernel_fits() says so first)
    if (P.n_steps > kPoolIndexMask) return hipErrorInvalidValue;          // (a pending entry keeps the step index in 23 bits: Converter::pooled_for() says so first)
    const bool fast = v.fast && !v.generic_only;       // (as launch_pool_kernel)
    return dispatch_variant(v, fast, [&](auto med, auto tilt, auto aniso, auto flasher, auto fast_tag) {
        return launch_pool_variant<med(), tilt(), aniso(), flasher(), fast_tag(), true>(P, stream, v.grid, v.launched, v.baked);
    });
}

} // namespace clsimhip
