// Event statistics on the device: the definition of event_stats.h as a stage behind the upload and behind assemble_hits_kernel, for
// gfx950 (wave64).
//
//   event_stats_steps_kernel     grid-stride over the bunch's steps, one lane per record: the dwords at offsets 32, 36, 40 of the 48-byte
//                                record (num_photons, weight, identifier) -> the record of its particle (direct index into a
//                                consecutive table, binary search otherwise) and the generated term
//   event_stats_photons_kernel   grid-stride over min(*photon_count, capacity) photon records: the dwords at offsets 36, 40, 44 of the
//                                80-byte record (weight, identifier, string ID | OM ID << 16) -> particle, mask, the at-DOM term
//   both, per wave               (wave_accumulate) steps and photons of one particle come in long runs: the wave takes the record of
//                                its first pending lane (a ballot, a readlane), and over the lanes that name it a ballot per sign and
//                                limb position tells which positions any of them touches; each touched position is summed across
//                                the 64 lanes in 64 bits with DPP moves and ONE lane issues one 64-bit atomicAdd for it, one for the
//                                count, one per kind of non-finite term.  A wave whose lanes all name one particle makes one trip;
//                                otherwise one trip per distinct particle, at most 64.
//   event_stats_close_kernel     one lane per record: carries propagated, positive minus negative accumulator, the 144-byte record;
//                                lane 0 writes the counters
//
// The photon count comes from device memory: nothing waits for the host.  Atomics only add integers to deferred-carry slots, which
// cannot overflow (event_stats.h), so no result depends on their order.
#include "event_stats.h"

namespace clsimhip {

namespace {

constexpr uint32_t kEventStatsMaxBlocks = 1024u;        // of the two grid-stride kernels: 4 per CU

// v of every lane + v of the lane CONTROL names, where ROWS lets the row write (a lane without a source adds 0)
template <int CONTROL, int ROWS>
__device__ __forceinline__ uint64_t dpp_add(uint64_t v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CONTROL, ROWS, 0xf, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CONTROL, ROWS, 0xf, false);
    return v + (((uint64_t)hi << 32) | lo);
}

// the sum over the 64 lanes, all of them active, as a wave-uniform value: four shifts within the rows of 16 (row_shr:1, 2, 4, 8)
// leave a row's sum in its last lane, two broadcasts (row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3) the wave's in
// lane 63
__device__ __forceinline__ uint64_t wave_sum(uint64_t v)
{
    v = dpp_add<0x111, 0xf>(v);
    v = dpp_add<0x112, 0xf>(v);
    v = dpp_add<0x114, 0xf>(v);
    v = dpp_add<0x118, 0xf>(v);
    v = dpp_add<0x142, 0xa>(v);
    v = dpp_add<0x143, 0xc>(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ void add_to(uint64_t *slot, uint64_t v) { atomicAdd(reinterpret_cast<unsigned long long *>(slot), (unsigned long long)v); }

// All 64 lanes of the wave are here.  `valid`: the lane has a term for `record` (< A.records); `count`: what it adds to the side's count.
template <uint32_t SIDE>
__device__ __forceinline__ void wave_accumulate(uint64_t *__restrict__ slots, uint32_t lane, bool valid, uint32_t record, const EventStatsTerm &t, uint32_t count)
{
    uint64_t todo = __ballot(valid);
    while (todo != 0u) {                                                    // one trip per distinct record: at most 64
        const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
        const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)record, (int)leader);
        const bool mine = valid && record == r;
        todo &= ~__ballot(mine);                                            // (the leader is one of them: the loop ends)
        uint64_t *acc = slots + (size_t)r * kEventStatsSlots;
        const uint64_t counted = wave_sum(mine ? (uint64_t)count : 0u);
        if (lane == 0u && counted != 0u) add_to(acc + kEventStatsCounts + SIDE, counted);
        const bool finite = mine && t.kind == ES_FINITE;
        if (__ballot(mine && !finite) != 0u) {
#pragma unroll
            for (uint32_t k = 1; k <= 3u; ++k) {
                const uint64_t of_kind = __ballot(mine && t.kind == k);
                if (lane == 0u && of_kind != 0u) add_to(acc + kEventStatsSpecial + 3u * SIDE + (k - 1u), (uint64_t)__popcll(of_kind));
            }
        }
#pragma unroll
        for (uint32_t negative = 0; negative < 2u; ++negative) {
            const bool signed_so = finite && t.negative == negative;
            if (__ballot(signed_so) == 0u) continue;
#pragma unroll
            for (uint32_t position = 0; position < 10u; ++position) {      // a term's limbs lie at 0 ... 9
                const uint32_t k = position - t.position;
                const uint32_t limb = !signed_so ? 0u : k == 0u ? t.limb[0] : k == 1u ? t.limb[1] : k == 2u ? t.limb[2] : 0u;
                if (__ballot(limb != 0u) == 0u) continue;                  // no lane touches this position
                const uint64_t sum = wave_sum((uint64_t)limb);
                if (lane == 0u) add_to(acc + event_stats_limb_slot(SIDE, negative, position), sum);
            }
        }
    }
}

__device__ __forceinline__ int64_t record_of(const EventStatsDeviceArgs &A, uint32_t identifier)
{
    if (!A.particles) return 0;
    return series_find_particle(A.particles, A.n_particles, A.consecutive != 0u, identifier);
}

__global__ void __launch_bounds__(256) event_stats_steps_kernel(const EventStatsDeviceArgs A)
{
    const uint32_t n = A.n_steps, lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    // `first` is the same in all 64 lanes of a wave
    for (uint64_t first = (uint64_t)blockIdx.x * 256u + (threadIdx.x & ~63u); first < n; first += stride) {
        const uint64_t i = first + lane;
        const bool have = i < n;
        uint32_t num_photons = 0u, weight = 0u, identifier = 0u;
        if (have) {
            const uint32_t *w = reinterpret_cast<const uint32_t *>(A.steps + i);        // i < n_steps
            num_photons = w[8]; weight = w[9]; identifier = w[10];
        }
        const int64_t record = have ? record_of(A, identifier) : -1;
        const uint64_t unknown = __ballot(have && record < 0);
        if (lane == 0u && unknown != 0u) atomicAdd(A.header + CLSIMHIP_EVENT_STATISTICS_UNKNOWN_STEP_PARTICLE, (uint32_t)__popcll(unknown));
        EventStatsTerm t;
        event_stats_term(weight, num_photons, true, t);
        wave_accumulate<ES_GENERATED>(A.slots, lane, record >= 0, (uint32_t)record, t, num_photons);
    }
}

__global__ void __launch_bounds__(256) event_stats_photons_kernel(const EventStatsDeviceArgs A)
{
    const uint32_t arrived = *A.photon_count;
    const uint32_t n = arrived < A.capacity ? arrived : A.capacity, lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t first = (uint64_t)blockIdx.x * 256u + (threadIdx.x & ~63u); first < n; first += stride) {
        const uint64_t i = first + lane;
        const bool have = i < n;
        uint32_t weight = 0u, identifier = 0u, word = 0u;
        if (have) {
            const uint32_t *w = reinterpret_cast<const uint32_t *>(A.photons + i);      // i < min(*photon_count, capacity)
            weight = w[9]; identifier = w[10]; word = w[11];
        }
        const int64_t record = have ? record_of(A, identifier) : -1;
        bool counted = record >= 0;
        if (counted) {
            const uint32_t frame_rank = A.particles ? A.particles[record].frame_rank : 0u;
            if (event_stats_is_masked(A.masked, A.n_masked, ((uint64_t)frame_rank << 32) | word)) counted = false;
        }
        const uint64_t unknown = __ballot(have && record < 0), masked = __ballot(record >= 0 && !counted);
        if (lane == 0u && unknown != 0u) atomicAdd(A.header + CLSIMHIP_EVENT_STATISTICS_UNKNOWN_PARTICLE, (uint32_t)__popcll(unknown));
        if (lane == 0u && masked != 0u) atomicAdd(A.header + CLSIMHIP_EVENT_STATISTICS_MASKED, (uint32_t)__popcll(masked));
        EventStatsTerm t;
        event_stats_term(weight, 1u, false, t);
        wave_accumulate<ES_AT_DOMS>(A.slots, lane, counted, (uint32_t)record, t, 1u);
    }
}

__global__ void __launch_bounds__(256) event_stats_close_kernel(const EventStatsDeviceArgs A)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r == 0u) {
#pragma unroll
        for (uint32_t k = 0; k < 3u; ++k) A.counters[k] = A.header[k];
        A.counters[3] = A.records;
    }
    if (r >= A.records) return;
    uint32_t identifier = 0u, frame = 0u;
    if (A.particles) {
        identifier = A.particles[r].identifier;
        frame = A.frames[A.particles[r].frame_rank];                       // a rank of the table's: < its frames
    }
    clsimhip_event_statistics record;
    event_stats_close(A.slots + r * kEventStatsSlots, identifier, frame, record);
    A.out[r] = record;
}

} // namespace

hipError_t launch_event_stats(const EventStatsDeviceArgs &A, hipStream_t stream)
{
    // header and accumulators lie together
    const size_t zeroed = kEventStatsHeaderWords * sizeof(uint32_t) + (size_t)(A.records ? A.records : 1u) * kEventStatsSlots * sizeof(uint64_t);
    hipError_t e = hipMemsetAsync(A.header, 0, zeroed, stream);
    if (e != hipSuccess) return e;
    const auto blocks_for = [](uint64_t records) {
        const uint64_t blocks = (records + 255u) / 256u;
        return (uint32_t)(blocks < kEventStatsMaxBlocks ? blocks : kEventStatsMaxBlocks);
    };
    if (A.n_steps) hipLaunchKernelGGL(event_stats_steps_kernel, dim3(blocks_for(A.n_steps)), dim3(256), 0, stream, A);
    if (A.capacity) hipLaunchKernelGGL(event_stats_photons_kernel, dim3(blocks_for(A.capacity)), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(event_stats_close_kernel, dim3((uint32_t)(((uint64_t)(A.records ? A.records : 1u) + 255u) / 256u)), dim3(256), 0, stream, A);
    return hipGetLastError();
}

} // namespace clsimhip
