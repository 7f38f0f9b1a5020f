// The exhaustive probe of the run-time compiled kernel's table index (detmath.hip.h: clamp_index_of), a unit of its own so that the
// machine code of the kernels in prop_aux_kernels.hip stays what it was.  Reached through launch_check_math (what = 20).
#include <hip/hip_runtime.h>

#include "detmath.hip.h"
#include "prop_launch.h"

namespace clsimhip {

// dm::clamp_index_of<HI> (the run-time compiled kernel's two-instruction table index, round 10) against the form it replaces,
// clampi((int)f, 0, HI): every one of the 2^32 bit patterns (512 per thread) x the six bounds the kernels bake in or could (0 and 1: the
// smallest tables; 0xa8, 0xaa, 0x1ff: C2's tilt rows, layers and string map; 0x3fff: beyond the inline constants and every real table).
// result[0] = mismatches, result[1..] = bit patterns of the first few mismatching arguments.
template <int HI>
DM void check_index_clamp_one(float f, uint32_t *result, uint32_t result_cap)
{
    const int hi = __builtin_amdgcn_readfirstlane(HI);                 // (the spelled-out form with its bound in a register, as it was)
    const int v = (int)f, lo = (v > 0) ? v : 0, want = (lo < hi) ? lo : hi;         // clampi((int)f, 0, hi) of prop_device.hip.h
    if (dm::clamp_index_of<HI>(f) != want) {
        const uint32_t k = atomicAdd(result, 1u);
        if (k + 1u < result_cap) result[k + 1u] = dm::f2u(f);
    }
}
__global__ void check_index_clamp_kernel(uint32_t *result, uint32_t result_cap)
{
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= (1u << 23)) return;
    for (uint32_t k = 0; k < 512u; ++k) {
        const float f = dm::u2f((m << 9) | k);
        check_index_clamp_one<0>(f, result, result_cap);
        check_index_clamp_one<1>(f, result, result_cap);
        check_index_clamp_one<0xa8>(f, result, result_cap);
        check_index_clamp_one<0xaa>(f, result, result_cap);
        check_index_clamp_one<0x1ff>(f, result, result_cap);
        check_index_clamp_one<0x3fff>(f, result, result_cap);
    }
}

hipError_t launch_check_index_clamp(uint32_t *result, uint32_t result_cap, hipStream_t stream)
{
    hipLaunchKernelGGL(check_index_clamp_kernel, dim3((1u << 23) / 256), dim3(256), 0, stream, result, result_cap);
    return hipGetLastError();
}

} // namespace clsimhip
