// PMT series on the device: the definition of pmt_series.h as a sorting stage behind pmt_hits_kernel, for gfx950 (wave64).
//
//   pmt_series_key_kernel  one lane per hit: the record's three 8-byte words, module slot -> rank and channel base, particle lookup,
//                          mask, time shift -> 16-byte key, appended per wave (ballot, population count, one atomic per wave; the
//                          append order is arbitrary and the sort removes it); the same pass counts the 16 x 256 digit histograms of
//                          the kept keys (LDS, then one atomic per non-empty bin).
//   launch_series_sort     the MCPE series stage's plan and stable LSD radix passes (mcpe_series_kernel.hip), unchanged: the key is
//                          its SeriesKey.
//   pmt_series_heads_kernel / launch_series_tile_scan / pmt_series_emit_kernel / pmt_series_close_kernel
//                          a key whose group differs from its predecessor's starts a series; the records are rebuilt from the keys
//                          (group -> frame rank and channel, channel -> module rank by a binary search over the channel bases, PMT =
//                          channel - base, time of the time key: equal keys are equal records).
//
// Everything reads its sizes from device memory (the hit counter, the kept count): nothing waits for the host, and a workgroup with
// nothing to do leaves at once.  Atomics only count; no position in the output comes from the arrival order of an atomic.
#include "pmt_series.h"

namespace clsimhip {

namespace {

constexpr uint32_t kNone = 3u;              // code of a lane without a record

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

__global__ void __launch_bounds__(256) pmt_series_key_kernel(const PmtSeriesDeviceArgs A)
{
    __shared__ uint32_t hist[16u * 256u];
    for (uint32_t i = threadIdx.x; i < 16u * 256u; i += 256u) hist[i] = 0u;
    __syncthreads();
    const uint32_t counted = *A.in_count;
    const uint32_t n = counted < A.capacity ? counted : A.capacity;
    const uint32_t lane = threadIdx.x & 63u;
    // `first` is the same in all 64 lanes of a wave: they make the same number of trips and meet in every ballot
    for (uint64_t first = blockIdx.x * 256u + (threadIdx.x & ~63u); first < n; first += gridDim.x * 256u) {
        const uint64_t i = first + lane;
        int code = (int)kNone;
        SeriesKey key;
        key.group = 0u; key.t_hi = 0u; key.t_lo = 0u; key.identifier = 0u;
        if (i < n) {
            const uint64_t *rec = reinterpret_cast<const uint64_t *>(A.in + i);
            const uint64_t ids = rec[0], pmt = rec[1];
            code = pmt_series_make_key(A.lookup, (uint32_t)ids, (uint32_t)(ids >> 32), (uint32_t)pmt, __builtin_bit_cast(double, rec[2]), key);
        }
        const uint64_t kept = __ballot(code == PMT_SERIES_KEPT);
        if (kept != 0u) {
            uint32_t base = 0u;
            if (lane == 0u) base = atomicAdd(A.header + SH_KEPT, (uint32_t)__popcll(kept));
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            if (code == PMT_SERIES_KEPT) {
                store_key(A.keys[0] + (size_t)(base + lanes_below(kept)), key);     // kept <= n <= capacity
#pragma unroll
                for (uint32_t p = 0; p < 16u; ++p) atomicAdd(&hist[p * 256u + series_digit(key, p)], 1u);
            }
        }
#pragma unroll
        for (int c = PMT_SERIES_UNKNOWN_PARTICLE; c <= PMT_SERIES_UNKNOWN_CHANNEL; ++c) {
            const uint64_t met = __ballot(code == c);
            if (met != 0u && lane == 0u) atomicAdd(A.header + SH_COUNTERS + c, (uint32_t)__popcll(met));
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 16u * 256u; i += 256u)
        if (hist[i] != 0u) atomicAdd(A.histogram + i, hist[i]);
}

__global__ void __launch_bounds__(256) pmt_series_heads_kernel(const PmtSeriesDeviceArgs A)
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

__global__ void __launch_bounds__(256) pmt_series_emit_kernel(const PmtSeriesDeviceArgs A)
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
    const uint32_t n_channels = A.lookup.n_channels, n_modules = A.lookup.n_modules;
#pragma unroll
    for (uint32_t r = 0; r < 8u; ++r) {
        const uint64_t i = start + wave * 512u + r * 64u + lane;
        if (i < n) {
            const SeriesKey &k = key[r];
            const uint32_t frame_rank = k.group / n_channels;           // (a kept key: there is a channel)
            const uint32_t channel = k.group - frame_rank * n_channels;
            const uint32_t rank = pmt_series_rank_of_channel(A.lookup.base, n_modules, channel);
            const uint32_t module = A.module_of_rank[rank];
            const uint32_t pmt = channel - A.lookup.base[rank];
            uint64_t *record = reinterpret_cast<uint64_t *>(A.out + i);
            record[0] = (uint64_t)k.identifier | ((uint64_t)module << 32);
            record[1] = (uint64_t)pmt;                                  // reserved = 0
            record[2] = __builtin_bit_cast(uint64_t, series_time_of(((uint64_t)k.t_hi << 32) | k.t_lo));
            if ((heads[r] >> lane) & 1u) {
                const uint32_t s = index + lanes_below(heads[r]);       // < series <= n
                uint64_t *entry = reinterpret_cast<uint64_t *>(A.series + s);
                entry[0] = (uint64_t)A.frames[frame_rank] | ((uint64_t)module << 32);
                entry[1] = (uint64_t)pmt | ((uint64_t)(uint32_t)i << 32);
                entry[2] = 0u;                                          // count: pmt_series_close_kernel; reserved = 0
            }
        }
        index += (uint32_t)__popcll(heads[r]);
    }
}

__global__ void __launch_bounds__(256) pmt_series_close_kernel(const PmtSeriesDeviceArgs A)
{
    const uint32_t n = A.header[SH_KEPT], n_series = A.header[SH_SERIES];
    for (uint64_t s = blockIdx.x * 256u + threadIdx.x; s < n_series; s += gridDim.x * 256u) {
        const uint32_t next = s + 1u < n_series ? A.series[s + 1u].first : n;
        A.series[s].count = next - A.series[s].first;
    }
    if (blockIdx.x == 0u && threadIdx.x < 5u) A.counts[threadIdx.x] = A.header[threadIdx.x];
}

} // namespace

hipError_t launch_pmt_series(const PmtSeriesDeviceArgs &A, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(A.header, 0, (kSeriesHeaderWords + 16u * 256u) * sizeof(uint32_t), stream);     // header and histogram lie together
    if (e != hipSuccess) return e;
    uint32_t lanes = (A.capacity + 255u) / 256u;
    if (A.capacity > 0xffffff00u || lanes > 1024u) lanes = 1024u;
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
    hipLaunchKernelGGL(pmt_series_key_kernel, dim3(lanes), dim3(256), 0, stream, A);
    launch_series_sort(S, stream);
    hipLaunchKernelGGL(pmt_series_heads_kernel, dim3(tiles), dim3(256), 0, stream, A);
    launch_series_tile_scan(S, stream);
    hipLaunchKernelGGL(pmt_series_emit_kernel, dim3(tiles), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(pmt_series_close_kernel, dim3(lanes), dim3(256), 0, stream, A);
    return hipGetLastError();
}

} // namespace clsimhip
