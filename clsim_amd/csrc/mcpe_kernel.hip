// MCPE kernel: the hit maker of mcpe.h over the photon records of one bunch, one lane per record.
//
// Traffic is the algorithm's own: 80 B read per record (five 16-byte loads per lane; neighbouring lanes read neighbouring
// records, so every cache line fetched is used whole), 16 B written per accepted MCPE.  Everything else is wave-uniform:
// the parameters come from the kernel argument segment (scalar loads), the acceptance tables are copied into LDS once per
// block (43 doubles for IceCube), the DOM -> class table is a few tens of KiB read through the caches.  Accepted MCPEs
// leave through a wave-aggregated append -- ballot, population count, one atomic per wave -- as flush_hit_stubs does for
// photons (prop_device.hip.h).
#include "mcpe.h"

namespace clsimhip {

__global__ void __launch_bounds__(256) mcpe_kernel(const McpeParams P)
{
    __shared__ double lds_values[kMcpeMaxTableValues];
    for (uint32_t i = threadIdx.x; i < P.num_values; i += 256u) lds_values[i] = P.values[i];
    __syncthreads();
    const uint32_t counted = *P.hit_count;
    const uint32_t n = counted < P.capacity ? counted : P.capacity;
    const uint32_t lane = threadIdx.x & 63u;
    const uint4 *records = reinterpret_cast<const uint4 *>(P.photons);
    // `first` is the same in all 64 lanes of a wave: they make the same number of trips and meet in every ballot
    for (uint64_t first = blockIdx.x * 256u + (threadIdx.x & ~63u); first < n; first += gridDim.x * 256u) {     // (64 bits: n may be close to 2^32)
        const uint64_t i = first + lane;
        int code = MCPE_DROPPED;
        clsimhip_mcpe m;
        m.identifier = 0u; m.string_id = 0; m.om_id = 0; m.time = 0.;
        if (i < n) {
            uint32_t w[20];
#pragma unroll
            for (uint32_t q = 0; q < 5u; ++q) {
                const uint4 v = records[i * 5u + q];
                w[4u * q] = v.x; w[4u * q + 1u] = v.y; w[4u * q + 2u] = v.z; w[4u * q + 3u] = v.w;
            }
            code = mcpe_make(P, lds_values, w, m);
        }
        const uint64_t accepted = __ballot(code == MCPE_ACCEPTED);
        if (accepted != 0u) {
            uint32_t base = 0u;
            if (lane == 0u) base = atomicAdd(P.counters, (uint32_t)__popcll(accepted));
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(accepted >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)accepted, 0u));
            // the counter keeps counting; only the first out_capacity arrivals are stored (the photon counter's rule, c.cl:329-334)
            if (code == MCPE_ACCEPTED && (uint64_t)base + rank < (uint64_t)P.out_capacity) {
                uint64_t *slot = reinterpret_cast<uint64_t *>(P.out + (size_t)(base + rank));
                slot[0] = (uint64_t)m.identifier | ((uint64_t)(uint16_t)m.string_id << 32) | ((uint64_t)m.om_id << 48);
                slot[1] = __builtin_bit_cast(uint64_t, m.time);
            }
        }
#pragma unroll
        for (int c = MCPE_NEGATIVE_WEIGHT; c <= MCPE_PROBABILITY_ABOVE_ONE; ++c) {
            const uint64_t met = __ballot(code == c);
            if (met != 0u && lane == 0u) atomicAdd(P.counters + c, (uint32_t)__popcll(met));
        }
    }
}

hipError_t launch_mcpe_kernel(const McpeParams &P, hipStream_t stream)
{
    // one lane per record up to 1024 blocks (262 144 records in one pass; a full IceCube bunch delivers ~184 000), a stride loop beyond
    uint32_t blocks = (P.capacity + 255u) / 256u;
    if (P.capacity > 0xffffff00u) blocks = 1024u;
    if (blocks > 1024u) blocks = 1024u;
    if (blocks == 0u) blocks = 1u;
    hipLaunchKernelGGL(mcpe_kernel, dim3(blocks), dim3(256), 0, stream, P);
    return hipGetLastError();
}

} // namespace clsimhip
