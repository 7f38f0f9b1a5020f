// The pooled propagation kernels with STOP_PHOTONS_ON_DETECTION (prop_pool_kernel.hip.h: KEEP = false) as a translation unit, compiled
// with the pooled kernel's code generation (Makefile: POOL_CODEGEN), and what the host asks about the pooled kernel's limits.
#include "prop_pool_kernel.hip.h"

namespace clsimhip {

hipError_t launch_pool_kernel(const KParams &P, const KVariant &v, hipStream_t stream)
{
    if (P.n_steps == 0) return hipSuccess;
    if (check_lengths(P, v) != hipSuccess) return hipErrorInvalidValue;
    if (P.history_n != 0 || v.tabulate || v.keep_detected) return hipErrorInvalidValue;
    if (P.num_layers >= (1 << 14)) return hipErrorInvalidValue;          // (a ring entry keeps the carried layer index in 14 bits: pool_kernel_fits() says so first)
    if (P.n_steps > kPoolIndexMask) return hipErrorInvalidValue;          // (a pending entry keeps the step index in 23 bits: Converter::pooled_for() says so first)
    // clsimhip_set_tuning("generic_kernels", 1): the generic instantiation also where Compile() found every proof (tests compare the two)
    const bool fast = v.fast && !v.generic_only;
    return dispatch_variant(v, fast, [&](auto med, auto tilt, auto aniso, auto flasher, auto fast_tag) {
        return launch_pool_variant<med(), tilt(), aniso(), flasher(), fast_tag(), false>(P, stream, v.grid, v.launched, v.baked);
    });
}

// the largest bunch the pooled kernel's 23-bit step index can address (clsimhip_set_tuning("pool_max_steps") lowers the GUARD for tests:
// larger bunches then take the classic kernel, exactly what a bunch beyond 2^23 - 1 does)
size_t pool_kernel_max_steps() { return (size_t{1} << kPoolIndexBits) - 1; }
// does the pooled kernel pay for this table image (its waves need at least kPoolWorthwhileReady ring entries)?  keep_strings: the
// number of strings when the converter runs without STOP_PHOTONS_ON_DETECTION (the search's string masks share the pool's LDS), else 0
bool pool_kernel_fits(uint32_t table_words, uint32_t keep_strings, int num_layers)
{
    if (num_layers >= (1 << 14)) return false;
    static_assert(kPoolWorthwhileReady >= kPoolMinReady, "an image the pooled kernel is chosen for must be one it can run");
    return pool_ring_that_fits(table_words, keep_strings) >= kPoolWorthwhileReady;
}

} // namespace clsimhip
