// The TABULATE instantiations of prop_kernel (the table maker, prop_kernel.hip.h: TAB = 1, 2) as a translation unit of their
// own: they are compiled with the compiler's default code generation -- the table maker's limit is its fp64 atomics, and it
// loses 3 % under the settings that the propagation instantiations gain 8-12 % from (Makefile: KERNEL_CODEGEN) -- and in
// parallel with them.
// (threads per workgroup of the table maker's kernels; the propagation kernels' 256 unless the build says otherwise)
#ifdef CLSIMHIP_TAB_BLOCK
#define CLSIMHIP_BLOCK CLSIMHIP_TAB_BLOCK
#endif
#include "prop_kernel.hip.h"

namespace clsimhip {

// FLASHER is always compiled in (the source type is looked at per step)
hipError_t launch_tab_kernel(const KParams &P, const KVariant &v, hipStream_t stream)
{
    if (P.n_steps == 0) return hipSuccess;
    if (!v.tabulate || !P.tab_bins || !P.has_fixed_abs) return hipErrorInvalidValue;
    if (check_lengths(P, v) != hipSuccess) return hipErrorInvalidValue;
    if (P.tab_ndim != 4 && P.tab_ndim != 5) return hipErrorInvalidValue;
    // (round 4) FAST: the instantiation without the wave-uniform tests of the medium's proofs, as in the propagation kernels.  Built, tested
    // (tests/test_tabulator.py) and measured -- 200x36x100x105 table: 2.15e7 photons/s against 2.24e7 for the generic instantiation, the
    // impact-angle table 1.92e7 both (profiles/r04/tab_fast_vs_generic.txt): this kernel waits for its memory-side fp64 atomics in 55 % of
    // its wave cycles and issues vector instructions in 37 % of the slots, fewer scalar branches buy nothing and the other register
    // allocation costs.  So the generic instantiation runs; clsimhip_tabulator_set_tuning("fast_kernels", 1) selects the other one.
    const bool fast = v.fast && v.tab_fast;
    return dispatch_variant<true>(v, fast, [&](auto med, auto tilt, auto aniso, auto flasher, auto fast_tag) {
        return (P.tab_ndim > 4) ? launch_variant<med(), tilt(), aniso(), flasher(), 2, fast_tag()>(P, stream, v.grid, v.launched)
                                : launch_variant<med(), tilt(), aniso(), flasher(), 1, fast_tag()>(P, stream, v.grid, v.launched);
    });
}

} // namespace clsimhip
