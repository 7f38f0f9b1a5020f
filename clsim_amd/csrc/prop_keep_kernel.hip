// The instantiations of prop_kernel without STOP_PHOTONS_ON_DETECTION (prop_kernel.hip.h: TAB = 3, SetStopDetectedPhotons(false))
// as a translation unit of their own: compiled in parallel with the others, with the propagation kernels' code generation (Makefile:
// KERNEL_CODEGEN) and four waves per SIMD (the search that saves every DOM on the way holds a hit sink and its masks on top of the photon).
#include "prop_kernel.hip.h"

namespace clsimhip {

hipError_t launch_keep_kernel(const KParams &P, const KVariant &v, hipStream_t stream)
{
    if (P.n_steps == 0) return hipSuccess;
    if (!v.keep_detected || v.tabulate) return hipErrorInvalidValue;
    if (check_lengths(P, v) != hipSuccess) return hipErrorInvalidValue;
    const bool fast = v.fast && P.history_n == 0 && !v.generic_only;       // (as launch_prop_kernel)
    return dispatch_variant(v, fast, [&](auto med, auto tilt, auto aniso, auto flasher, auto fast_tag) {
        return launch_variant<med(), tilt(), aniso(), flasher(), 3, fast_tag()>(P, stream, v.grid, v.launched);
    });
}

} // namespace clsimhip
