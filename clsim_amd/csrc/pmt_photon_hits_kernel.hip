// PMT photon hits on the device: the definition of pmt_photon_hits.h as a sorting stage over stored frame photons, for gfx950
// (wave64).  The shape is photon_hits_kernel.hip's.
//
//   pmt_photon_hits_key_kernel     one lane per record: three 16-byte loads, the series search, the module's slot, its rotation and type
//                                  from the global module table (88 B per module, through the caches), the PMT loop per lane -> 16-byte
//                                  key (series x 64 + PMT, time key, identifier), appended per wave (ballot, population count, one atomic
//                                  per wave; the append order is arbitrary and the sort removes it).  The PMT tables of all types (72 B
//                                  per PMT) and the function values are copied into dynamic LDS once per workgroup, as pmt_hits_kernel
//                                  stages them: exactly the bytes the generator holds, 60 KiB at its limits.  That is ALL the LDS of
//                                  this kernel: no launch of the stage asks for more than 64 KiB per workgroup.
//   pmt_photon_hits_digits_kernel  the 16 x 256 digit histograms of the kept keys (one 16-byte read per key), 16 KiB of LDS in a
//                                  kernel of its own for that reason.  For the bytes of the group no key of this launch can differ
//                                  in, the count goes to bin 0, one addition per pass.
//   launch_series_sort             the MCPE series stage's plan and stable LSD radix passes (mcpe_series_kernel.hip), unchanged.
//   pmt_photon_hits_heads_kernel / launch_series_tile_scan / pmt_photon_hits_emit_kernel / pmt_photon_hits_close_kernel
//                                  a key whose group differs from its predecessor's starts a series; the hits are rebuilt from the
//                                  keys (identifier, the IDs of the input's series entry, PMT = group mod 64, the time of the time key
//                                  bit for bit: equal keys are equal hits).
//
// Everything reads its sizes from device memory (the input's two counts, the kept count): nothing waits for the host, and a workgroup
// with nothing to do leaves at once.  Atomics only count; no position in the output comes from the arrival order of an atomic.
#include "pmt_photon_hits.h"

namespace clsimhip {

namespace {

constexpr int kNone = PMT_PHOTON_HIT_DROPPED;   // code of a lane without a record
constexpr uint32_t kPerType = (uint32_t)kPmtMaxPerType;

__device__ __forceinline__ uint32_t lanes_below(uint64_t mask)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__device__ __forceinline__ SeriesKey load_key(const SeriesKey *p)
{
    const uint4 v = *reinterpret_cast<const uint4 *>(p);
    SeriesKey k;
    k.group = v.x; k.t_hi = v.y; k.t_lo = v.z; k.identifier = v.w;
    return k;
}
__device__ __forceinline__ void store_key(SeriesKey *p, const SeriesKey &k)
{
    *reinterpret_cast<uint4 *>(p) = make_uint4(k.group, k.t_hi, k.t_lo, k.identifier);
}

__device__ __forceinline__ uint32_t at_most(uint32_t counted, uint32_t capacity) { return counted < capacity ? counted : capacity; }

__global__ void __launch_bounds__(256) pmt_photon_hits_key_kernel(const PmtPhotonHitsDeviceArgs A)
{
    extern __shared__ uint64_t lds_words[];             // [num_pmts x 9] PMT tables, [num_values] function values
    const uint32_t pmt_words = A.P.num_pmts * 9u;
    {
        const uint64_t *from = reinterpret_cast<const uint64_t *>(A.P.pmts);
        for (uint32_t i = threadIdx.x; i < pmt_words; i += 256u) lds_words[i] = from[i];
        from = reinterpret_cast<const uint64_t *>(A.P.values);
        for (uint32_t i = threadIdx.x; i < A.P.num_values; i += 256u) lds_words[pmt_words + i] = from[i];
    }
    __syncthreads();
    const PmtEntry *lds_pmts = reinterpret_cast<const PmtEntry *>(lds_words);
    const double *lds_values = reinterpret_cast<const double *>(lds_words + pmt_words);
    const uint32_t n = at_most(A.in_counts[0], A.capacity);
    PmtPhotonHitLookup L;
    L.series = A.in_series;
    L.n_series = at_most(A.in_counts[1], A.capacity);
    L.reserved = 0u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint4 *records = reinterpret_cast<const uint4 *>(A.in);
    // `first` is the same in all 64 lanes of a wave: they make the same number of trips and meet in every ballot
    for (uint64_t first = blockIdx.x * 256u + (threadIdx.x & ~63u); first < n; first += gridDim.x * 256u) {
        const uint64_t i = first + lane;
        int code = kNone;
        bool off_surface = false;
        uint32_t pmt = 0u;
        SeriesKey key;
        key.group = 0u; key.t_hi = 0u; key.t_lo = 0u; key.identifier = 0u;
        if (i < n) {
            uint32_t w[12];
#pragma unroll
            for (uint32_t q = 0; q < 3u; ++q) {
                const uint4 v = records[i * 3u + q];
                w[4u * q] = v.x; w[4u * q + 1u] = v.y; w[4u * q + 2u] = v.z; w[4u * q + 3u] = v.w;
            }
            code = pmt_photon_hit_make(L, A.P, lds_values, lds_pmts, (uint32_t)i, w, key, pmt, off_surface);
        }
        const uint64_t kept = __ballot(code == PMT_PHOTON_HIT_KEPT);
        if (kept != 0u) {
            uint32_t base = 0u;
            if (lane == 0u) base = atomicAdd(A.header + SH_KEPT, (uint32_t)__popcll(kept));
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            if (code == PMT_PHOTON_HIT_KEPT) store_key(A.keys[0] + (size_t)(base + lanes_below(kept)), key);        // kept <= n <= capacity
        }
#pragma unroll
        for (int c = PMT_PHOTON_HIT_UNCOVERED; c <= PMT_PHOTON_HIT_OFF_SURFACE; ++c) {
            const uint64_t met = __ballot(c == PMT_PHOTON_HIT_OFF_SURFACE ? off_surface : code == c);
            if (met != 0u && lane == 0u) atomicAdd(A.header + PPH_COUNTERS + c, (uint32_t)__popcll(met));
        }
    }
}

__global__ void __launch_bounds__(256) pmt_photon_hits_digits_kernel(const PmtPhotonHitsDeviceArgs A)
{
    const uint32_t n = A.header[SH_KEPT];
    if ((uint64_t)blockIdx.x * 256u >= n) return;       // (the workgroup's first key: block 0 leaves too when nothing was kept)
    __shared__ uint32_t hist[16u * 256u];
    for (uint32_t i = threadIdx.x; i < 16u * 256u; i += 256u) hist[i] = 0u;
    __syncthreads();
    const uint32_t counted_passes = 12u + A.group_passes;
    const SeriesKey *keys = A.keys[0];
    for (uint64_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const SeriesKey key = load_key(keys + i);
#pragma unroll
        for (uint32_t p = 0; p < 16u; ++p)
            if (p < counted_passes) atomicAdd(&hist[p * 256u + series_digit(key, p)], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 16u * 256u; i += 256u)
        if (hist[i] != 0u) atomicAdd(A.histogram + i, hist[i]);
    // the group's upper bytes are zero in every key of this launch (group < capacity x 64): bin 0, one addition per pass
    if (blockIdx.x == 0u && threadIdx.x >= counted_passes && threadIdx.x < 16u) atomicAdd(A.histogram + threadIdx.x * 256u, n);
}

__global__ void __launch_bounds__(256) pmt_photon_hits_heads_kernel(const PmtPhotonHitsDeviceArgs A)
{
    const uint32_t n = A.header[SH_KEPT];
    const uint64_t start = (uint64_t)blockIdx.x * kSeriesTile;
    if (start >= n) return;
    __shared__ uint32_t heads;
    if (threadIdx.x == 0u) heads = 0u;
    __syncthreads();
    const SeriesKey *keys = A.keys[A.header[SH_FINAL]];
    uint32_t mine = 0u;
#pragma unroll
    for (uint32_t r = 0; r < 8u; ++r) {
        const uint64_t i = start + r * 256u + threadIdx.x;
        if (i < n && (i == 0u || keys[i].group != keys[i - 1u].group)) ++mine;
    }
    if (mine != 0u) atomicAdd(&heads, mine);
    __syncthreads();
    if (threadIdx.x == 0u) A.tile_counts[blockIdx.x] = heads;
}

__global__ void __launch_bounds__(256) pmt_photon_hits_emit_kernel(const PmtPhotonHitsDeviceArgs A)
{
    const uint32_t n = A.header[SH_KEPT];
    const uint64_t start = (uint64_t)blockIdx.x * kSeriesTile;
    if (start >= n) return;
    __shared__ uint32_t wave_heads[4];
    const SeriesKey *keys = A.keys[A.header[SH_FINAL]];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    SeriesKey key[8];
    uint64_t heads[8];
    uint32_t total = 0u;
#pragma unroll
    for (uint32_t r = 0; r < 8u; ++r) {
        const uint64_t i = start + wave * 512u + r * 64u + lane;
        bool head = false;
        if (i < n) {
            key[r] = load_key(keys + i);
            head = i == 0u || key[r].group != keys[i - 1u].group;
        }
        heads[r] = __ballot(head);
        total += (uint32_t)__popcll(heads[r]);
    }
    if (lane == 0u) wave_heads[wave] = total;
    __syncthreads();
    uint32_t index = A.tile_counts[blockIdx.x];         // scanned: the series the tile's first head starts
    for (uint32_t w = 0; w < wave; ++w) index += wave_heads[w];
    const uint2 *entries = reinterpret_cast<const uint2 *>(A.in_series);
#pragma unroll
    for (uint32_t r = 0; r < 8u; ++r) {
        const uint64_t i = start + wave * 512u + r * 64u + lane;
        if (i < n) {
            const SeriesKey &k = key[r];
            const uint32_t pmt = k.group % kPerType;
            const uint2 entry = entries[2u * (size_t)(k.group / kPerType)];    // frame, string ID | OM ID << 16 (a kept key's series is an entry in use)
            uint64_t *record = reinterpret_cast<uint64_t *>(A.out + i);
            record[0] = (uint64_t)k.identifier | ((uint64_t)entry.y << 32);
            record[1] = (uint64_t)pmt;
            record[2] = pmt_photon_hit_time_bits(k);
            if ((heads[r] >> lane) & 1u) {
                const uint32_t s = index + lanes_below(heads[r]);       // < series <= n
                uint64_t *out_entry = reinterpret_cast<uint64_t *>(A.series + s);
                out_entry[0] = (uint64_t)entry.x | ((uint64_t)entry.y << 32);
                out_entry[1] = (uint64_t)pmt | ((uint64_t)(uint32_t)i << 32);
                out_entry[2] = 0u;                                      // count: pmt_photon_hits_close_kernel; reserved 0
            }
        }
        index += (uint32_t)__popcll(heads[r]);
    }
}

__global__ void __launch_bounds__(256) pmt_photon_hits_close_kernel(const PmtPhotonHitsDeviceArgs A)
{
    const uint32_t n = A.header[SH_KEPT], n_series = A.header[SH_SERIES];
    for (uint64_t s = blockIdx.x * 256u + threadIdx.x; s < n_series; s += gridDim.x * 256u) {
        const uint32_t next = s + 1u < n_series ? A.series[s + 1u].first : n;
        A.series[s].count = next - A.series[s].first;
    }
    if (blockIdx.x == 0u) {
        if (threadIdx.x < 2u) A.counts[threadIdx.x] = A.header[threadIdx.x];
        else if (threadIdx.x < 2u + (uint32_t)kPmtPhotonHitCounters) A.counts[threadIdx.x] = A.header[PPH_COUNTERS + threadIdx.x - 2u];
    }
}

} // namespace

hipError_t launch_pmt_photon_hits(const PmtPhotonHitsDeviceArgs &A, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(A.header, 0, (kSeriesHeaderWords + 16u * 256u) * sizeof(uint32_t), stream);     // header and histogram lie together
    if (e != hipSuccess) return e;
    uint32_t lanes = (A.capacity + 255u) / 256u;
    if (lanes > 1024u) lanes = 1024u;
    if (lanes == 0u) lanes = 1u;
    uint32_t tiles = (uint32_t)(((uint64_t)A.capacity + kSeriesTile - 1u) / kSeriesTile);
    if (tiles == 0u) tiles = 1u;
    SeriesDeviceArgs S{};                               // what the MCPE series stage's sort passes and tile scan read
    S.capacity = A.capacity;
    S.header = A.header;
    S.histogram = A.histogram;
    S.tile_counts = A.tile_counts;
    S.keys[0] = A.keys[0];
    S.keys[1] = A.keys[1];
    hipLaunchKernelGGL(pmt_photon_hits_key_kernel, dim3(lanes), dim3(256), pmt_hits_lds_bytes(A.P), stream, A);
    e = hipGetLastError();                              // (a launch the runtime refuses -- its LDS, its arguments -- is an error return here)
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pmt_photon_hits_digits_kernel, dim3(lanes), dim3(256), 0, stream, A);
    launch_series_sort(S, stream);
    hipLaunchKernelGGL(pmt_photon_hits_heads_kernel, dim3(tiles), dim3(256), 0, stream, A);
    launch_series_tile_scan(S, stream);
    hipLaunchKernelGGL(pmt_photon_hits_emit_kernel, dim3(tiles), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(pmt_photon_hits_close_kernel, dim3(lanes), dim3(256), 0, stream, A);
    return hipGetLastError();
}

} // namespace clsimhip
