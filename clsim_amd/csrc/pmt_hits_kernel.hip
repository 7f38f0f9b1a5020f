// Multi-PMT hit kernel: the hit maker of pmt_hits.h over the photon records of one bunch, one lane per record.
//
// Traffic as in mcpe_kernel: 80 B read per record (five 16-byte loads per lane, neighbouring lanes read neighbouring records), 24 B
// written per hit.  The parameters come by value in the kernel argument segment.  The PMT tables of all module types (72 B per PMT)
// and the function values are copied into LDS once per block -- the launch asks for exactly the bytes the generator holds, 2.5 KiB
// for one type of 31 PMTs with three short tables, 60 KiB at the limits -- and every lane of a wave that looks at the same PMT reads
// the same LDS address (a broadcast; lanes of modules of different types diverge, the loop runs per lane).  A module's rotation and
// type sit in a global table behind the hash lookup (88 B per module, read once per record, through the caches).  The loop is
// binary64 throughout: 31 PMTs are about 1 900 operations per record, 0.35 GFLOP for a full IceCube-sized bunch -- microseconds at
// the vector binary64 rate, so one block size serves: 256 lanes, at most two blocks' worth of LDS per CU at the limits.  Accepted
// hits leave through the wave-aggregated append of mcpe_kernel -- ballot, population count, one atomic per wave.
#include "pmt_hits.h"

namespace clsimhip {

__global__ void __launch_bounds__(256) pmt_hits_kernel(const PmtHitParams P)
{
    extern __shared__ uint64_t lds_words[];             // [num_pmts x 9] PMT tables, [num_values] function values
    const uint32_t pmt_words = P.num_pmts * 9u;
    {
        const uint64_t *from = reinterpret_cast<const uint64_t *>(P.pmts);
        for (uint32_t i = threadIdx.x; i < pmt_words; i += 256u) lds_words[i] = from[i];
        from = reinterpret_cast<const uint64_t *>(P.values);
        for (uint32_t i = threadIdx.x; i < P.num_values; i += 256u) lds_words[pmt_words + i] = from[i];
    }
    __syncthreads();
    const PmtEntry *lds_pmts = reinterpret_cast<const PmtEntry *>(lds_words);
    const double *lds_values = reinterpret_cast<const double *>(lds_words + pmt_words);
    const uint32_t counted = *P.hit_count;
    const uint32_t n = counted < P.capacity ? counted : P.capacity;
    const uint32_t lane = threadIdx.x & 63u;
    const uint4 *records = reinterpret_cast<const uint4 *>(P.photons);
    // `first` is the same in all 64 lanes of a wave: they make the same number of trips and meet in every ballot
    for (uint64_t first = blockIdx.x * 256u + (threadIdx.x & ~63u); first < n; first += gridDim.x * 256u) {     // (64 bits: n may be close to 2^32)
        const uint64_t i = first + lane;
        int code = PMT_DROPPED;
        bool off_surface = false;
        clsimhip_pmt_hit hit;
        hit.identifier = 0u; hit.string_id = 0; hit.om_id = 0; hit.pmt = 0u; hit.reserved = 0u; hit.time = 0.;
        if (i < n) {
            uint32_t w[20];
#pragma unroll
            for (uint32_t q = 0; q < 5u; ++q) {
                const uint4 v = records[i * 5u + q];
                w[4u * q] = v.x; w[4u * q + 1u] = v.y; w[4u * q + 2u] = v.z; w[4u * q + 3u] = v.w;
            }
            code = pmt_make(P, lds_values, lds_pmts, w, hit, off_surface);
        }
        const uint64_t accepted = __ballot(code == PMT_ACCEPTED);
        if (accepted != 0u) {
            uint32_t base = 0u;
            if (lane == 0u) base = atomicAdd(P.counters, (uint32_t)__popcll(accepted));
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(accepted >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)accepted, 0u));
            // the counter keeps counting; only the first out_capacity arrivals are stored (the photon counter's rule, c.cl:329-334)
            if (code == PMT_ACCEPTED && (uint64_t)base + rank < (uint64_t)P.out_capacity) {
                uint64_t *slot = reinterpret_cast<uint64_t *>(P.out + (size_t)(base + rank));
                slot[0] = (uint64_t)hit.identifier | ((uint64_t)(uint16_t)hit.string_id << 32) | ((uint64_t)hit.om_id << 48);
                slot[1] = (uint64_t)hit.pmt;
                slot[2] = __builtin_bit_cast(uint64_t, hit.time);
            }
        }
#pragma unroll
        for (int c = PMT_UNKNOWN_MODULE; c <= PMT_PROBABILITY_ABOVE_ONE; ++c) {
            const uint64_t met = __ballot(code == c);
            if (met != 0u && lane == 0u) atomicAdd(P.counters + c, (uint32_t)__popcll(met));
        }
        const uint64_t off = __ballot(off_surface);
        if (off != 0u && lane == 0u) atomicAdd(P.counters + 3, (uint32_t)__popcll(off));
    }
}

hipError_t launch_pmt_hits_kernel(const PmtHitParams &P, hipStream_t stream)
{
    // one lane per record up to 1024 blocks, a stride loop beyond (mcpe_kernel's grid)
    uint32_t blocks = (P.capacity + 255u) / 256u;
    if (P.capacity > 0xffffff00u) blocks = 1024u;
    if (blocks > 1024u) blocks = 1024u;
    if (blocks == 0u) blocks = 1u;
    hipLaunchKernelGGL(pmt_hits_kernel, dim3(blocks), dim3(256), pmt_hits_lds_bytes(P), stream, P);
    return hipGetLastError();
}

} // namespace clsimhip
