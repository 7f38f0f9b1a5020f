// Cable shadow on the device: the definition of cable_shadow.h as a filtering stage behind assemble_hits_kernel, for gfx950 (wave64).
//
//   cable_shadow_flag_kernel     one lane per record: groups 0 and 1 of the record -> its segment, made once (cable_segment), then the
//                                cylinder table from its first record to its last, two records a trip.  The table is the same for
//                                every lane: the loop counter and the table's address are wave-uniform and nothing is stored before
//                                the loop, so a cylinder's 64 bytes come through the scalar cache into scalar registers and cost
//                                the vector unit no load and no register.  A lane that has hit stops testing; a wave leaves the
//                                loop when all its lanes have hit.  It writes the flag byte and adds the wave's lit records to the
//                                count of their tile of 2 048 records (one atomic per wave; a wave's 64 records lie in one tile).
//   launch_series_tile_scan      the MCPE series stage's single-workgroup scan, unchanged, on a header of this stage:
//                                [SH_KEPT] = the records tested, the total -- the lit records -- in [SH_SERIES]
//   cable_shadow_compact_kernel  per tile: every wave walks its 512 flags in index order, 64 at a time; a lit record's place is the
//                                tile's scanned count, the lit records of the waves before, and the lit lanes below in the ballot.
//                                The record moves as five 16-byte loads and stores.  Output order = input order.  It writes the
//                                count block: lit, tested, shadowed.
//
// Everything reads its sizes from device memory: nothing waits for the host, and a workgroup with nothing to do leaves at once.
// Atomics only count; no position in the output comes from the arrival order of an atomic.  The work of a launch is bounded by
// capacity x 16 384 tests (cable_shadow.h: kCableShadowMaxCylinders).
#include "cable_shadow.h"

namespace clsimhip {

namespace {

__device__ __forceinline__ uint32_t lanes_below(uint64_t mask)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__global__ void __launch_bounds__(256) cable_shadow_flag_kernel(const CableShadowDeviceArgs A, const CableCylinder *__restrict__ cylinders)
{
    const uint32_t counted = *A.in_count;
    const uint32_t n = counted < A.capacity ? counted : A.capacity;
    // `first` is the same in all 64 lanes of a wave
    const uint64_t first = (uint64_t)blockIdx.x * 256u + (threadIdx.x & ~63u);
    if (first >= n) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = first + lane;
    const bool have = i < n;
    CableSegment s;
    s.P0[0] = 0.; s.P0[1] = 0.; s.P0[2] = 0.; s.d[0] = 0.; s.d[1] = 0.; s.d[2] = 0.; s.dd = 0.;
    if (have) {
        const uint4 *g = reinterpret_cast<const uint4 *>(A.in + i);        // i < min(*in_count, capacity)
        const uint4 g0 = g[0], g1 = g[1];                                   // x y z time, theta phi wavelength cherenkov_dist
        cable_segment(__builtin_bit_cast(float, g0.x), __builtin_bit_cast(float, g0.y), __builtin_bit_cast(float, g0.z), __builtin_bit_cast(float, g1.x),
                      __builtin_bit_cast(float, g1.y), A.distance, s);
    }
    bool testing = have;                                                    // a record, and no cylinder has hit it yet
    // Two cylinders a trip, carried from one trip to the next so that both loads are issued together at the top of the trip: the
    // table comes from the L2, a wave waits for it once per pair, not once per cylinder (and not once per part of a cylinder, as
    // when the loads are left to sink into the branches that use them).  Scalar loads return in any order, so the wait for this
    // trip's pair is also the wait for the pair just asked for: the loads of one trip do not overlap the tests of the trip before.
    // An index beyond the table names its last record again (n_cylinders >= 1), which changes nothing.
    const uint32_t n_cylinders = A.n_cylinders, last = n_cylinders - 1u;
    CableCylinder next0 = cylinders[0], next1 = cylinders[1u < last ? 1u : last];
    for (uint32_t c = 0; c < n_cylinders; c += 2u) {
        if (__ballot(testing) == 0u) break;
        const CableCylinder cylinder0 = next0, cylinder1 = next1;
        next0 = cylinders[c + 2u < last ? c + 2u : last];                   // wave-uniform, <= last
        next1 = cylinders[c + 3u < last ? c + 3u : last];
        if (testing && cable_hit(s, cylinder0)) testing = false;
        if (testing && cable_hit(s, cylinder1)) testing = false;
    }
    const uint64_t lit = __ballot(testing);
    if (have) A.flags[i] = testing ? (uint8_t)0u : (uint8_t)1u;
    if (lane == 0u && lit != 0u) atomicAdd(A.tile_counts + first / kCableShadowTile, (uint32_t)__popcll(lit));     // first < capacity: a tile of it
    if (blockIdx.x == 0u && threadIdx.x == 0u) A.header[SH_KEPT] = n;       // (n = 0: the header was zeroed)
}

__global__ void __launch_bounds__(256) cable_shadow_compact_kernel(const CableShadowDeviceArgs A)
{
    const uint32_t n = A.header[SH_KEPT];
    if (blockIdx.x == 0u && threadIdx.x == 0u) {
        const uint32_t lit = A.header[SH_SERIES];                           // <= n
        A.counts[0] = lit; A.counts[1] = n; A.counts[2] = n - lit;
    }
    const uint64_t start = (uint64_t)blockIdx.x * kCableShadowTile;
    if (start >= n) return;
    __shared__ uint32_t wave_lit[4];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint64_t keep[8];
    uint32_t total = 0u;
#pragma unroll
    for (uint32_t r = 0; r < 8u; ++r) {
        const uint64_t i = start + wave * 512u + r * 64u + lane;
        keep[r] = __ballot(i < n && A.flags[i] == 0u);
        total += (uint32_t)__popcll(keep[r]);
    }
    if (lane == 0u) wave_lit[wave] = total;
    __syncthreads();
    uint32_t at = A.tile_counts[blockIdx.x];            // scanned: the lit records of the tiles before
    for (uint32_t w = 0; w < wave; ++w) at += wave_lit[w];
#pragma unroll
    for (uint32_t r = 0; r < 8u; ++r) {
        if ((keep[r] >> lane) & 1u) {
            const uint64_t i = start + wave * 512u + r * 64u + lane;       // < n
            const uint4 *from = reinterpret_cast<const uint4 *>(A.in + i);
            uint4 *to = reinterpret_cast<uint4 *>(A.lit + (size_t)(at + lanes_below(keep[r])));     // < lit <= n <= capacity
            const uint4 g0 = from[0], g1 = from[1], g2 = from[2], g3 = from[3], g4 = from[4];
            to[0] = g0; to[1] = g1; to[2] = g2; to[3] = g3; to[4] = g4;
        }
        at += (uint32_t)__popcll(keep[r]);
    }
}

} // namespace

hipError_t launch_cable_shadow(const CableShadowDeviceArgs &A, hipStream_t stream)
{
    uint32_t tiles = (uint32_t)(((uint64_t)A.capacity + kCableShadowTile - 1u) / kCableShadowTile);
    if (tiles == 0u) tiles = 1u;
    uint32_t blocks = (uint32_t)(((uint64_t)A.capacity + 255u) / 256u);
    if (blocks == 0u) blocks = 1u;
    // header and tile counts lie together
    hipError_t e = hipMemsetAsync(A.header, 0, (kSeriesHeaderWords + (size_t)tiles) * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    SeriesDeviceArgs scan{};                // what the MCPE series stage's tile scan reads
    scan.capacity = A.capacity;
    scan.header = A.header;
    scan.tile_counts = A.tile_counts;
    hipLaunchKernelGGL(cable_shadow_flag_kernel, dim3(blocks), dim3(256), 0, stream, A, A.cylinders);
    launch_series_tile_scan(scan, stream);
    hipLaunchKernelGGL(cable_shadow_compact_kernel, dim3(tiles), dim3(256), 0, stream, A);
    return hipGetLastError();
}

} // namespace clsimhip
