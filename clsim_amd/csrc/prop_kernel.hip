// The classic propagation kernels (prop_kernel.hip.h: TAB = 0, one photon per lane, STOP_PHOTONS_ON_DETECTION) as a translation unit,
// compiled with the propagation kernels' code generation (Makefile: KERNEL_CODEGEN), and what the host asks about their geometry.
#include "prop_kernel.hip.h"

namespace clsimhip {

hipError_t launch_prop_kernel(const KParams &P, const KVariant &v, hipStream_t stream)
{
    if (P.n_steps == 0) return hipSuccess;
    if (check_lengths(P, v) != hipSuccess) return hipErrorInvalidValue;
    const bool fast = v.fast && P.history_n == 0 && !v.generic_only;
    return dispatch_variant(v, fast, [&](auto med, auto tilt, auto aniso, auto flasher, auto fast_tag) {
        return launch_variant<med(), tilt(), aniso(), flasher(), 0, fast_tag()>(P, stream, v.grid, v.launched);
    });
}

size_t prop_kernel_lds_bytes(uint32_t table_words) { return (size_t)(table_words + kWavesPerBlock * kStageRecords * kStubWords + kBlock) * 4; }
int prop_kernel_block_size() { return kBlock; }
// upper bound of the lanes of one launch (persistent grid: at most 2048 resident threads per CU)
size_t prop_kernel_max_lanes()
{
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    return (size_t)cus * 2048u;
}
// LDS bytes one workgroup may use so that the intended number of workgroups fits the CU's 160 KB
size_t prop_kernel_lds_budget() { return (size_t)(160 * 1024) / (size_t)((kMinWavesPerSimd * 256) / kBlock) - 1024; }

} // namespace clsimhip
