// MCPE merging on the device: the definition of mcpe_merge.h as a stage behind the series stage, for gfx950 (wave64), and its host
// side (workspace, argument checks, launches).
//
//   merge_open_kernel      a wave owns a grid-stride share of the series table and walks each of its series 64 records per round.
//                          With the current opener's time T wave-uniform it ballots merge_opens(t, T, window) over the lanes behind
//                          the opener; the lowest set lane is the next opener, and it repeats within the round until the ballot is
//                          empty: one ballot per group plus one per round, whatever the length of the series.  The next round's
//                          times are loaded before this round's ballots.  Per record: one flag word, and the series it belongs to.
//   merge_count_kernel / scan / merge_group_kernel / merge_close_kernel
//                          openers per tile of 2048 records, exclusive scan (the series stage's, one workgroup), then every
//                          record's group index from ballots over the flags; an opener writes its merged record and its own
//                          position, npe is the distance to the next opener (series are contiguous and each starts with an opener),
//                          and the merged series table comes from the group index at each series' first record.
//   merge_parent_key_kernel / the series stage's sort passes / merge_parent_count_kernel / scan / merge_parent_emit_kernel /
//   merge_finish_kernel    per record the key (series, identifier, group within the series, 0) in the 16-byte SeriesKey layout,
//                          sorted by the series stage's stable LSD radix passes (its plan skips the constant digits); a key that
//                          differs from its predecessor is a distinct (identifier, group) pair of its series, a key whose series
//                          differs starts that series' range.
//
// Everything reads its sizes from device memory (the series stage's counts): nothing waits for the host.  Atomics only count; no
// position comes from the arrival order of an atomic.
#include "mcpe_merge.h"

#include <string>

#include "hip_resources.h"

namespace clsimhip {

namespace {

__device__ __forceinline__ uint32_t lanes_below(uint64_t mask)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// t of lane `from`, which is the same in all lanes
__device__ __forceinline__ double time_of_lane(double t, uint32_t from)
{
    const uint64_t b = __builtin_bit_cast(uint64_t, t);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, (int)from);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), (int)from);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ uint4 load_words(const SeriesKey *p) { return *reinterpret_cast<const uint4 *>(p); }

__global__ void __launch_bounds__(256) merge_open_kernel(const MergeDeviceArgs A)
{
    const uint32_t stored = A.series_counts[0], tabled = A.series_counts[1];
    const uint32_t n = stored < A.capacity ? stored : A.capacity;
    const uint32_t n_series = tabled < A.capacity ? tabled : A.capacity;
    if (blockIdx.x == 0u && threadIdx.x == 0u) {
        A.header[SH_KEPT] = n;
        A.header[MH_SERIES] = n_series;
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves = gridDim.x * 4u;
    // `s` is the same in all 64 lanes of a wave, and so is every loop below: the lanes meet in every ballot
    for (uint32_t s = blockIdx.x * 4u + (threadIdx.x >> 6); s < n_series; s += waves) {
        const uint32_t at = A.series[s].first, count = A.series[s].count;
        const uint64_t first = at < n ? at : n;                                         // (a table that partitions the records: no clamp bites)
        const uint64_t end = first + count < n ? first + count : n;
        double T = 0.;
        double ahead = first + lane < end ? A.in[first + lane].time : 0.;
        for (uint64_t base = first; base < end; base += 64u) {
            const uint64_t i = base + lane;
            const bool have = i < end;
            const double t = ahead;
            if (i + 64u < end) ahead = A.in[i + 64u].time;                              // in flight during this round's ballots
            uint64_t behind = __ballot(have);                                           // the lanes behind the current opener
            uint64_t opened = 0u;
            if (base == first) {                                                        // the first record of the series
                opened = 1u;
                T = time_of_lane(t, 0u);
                behind &= ~1ull;
            }
            for (;;) {
                const uint64_t open = __ballot(((behind >> lane) & 1u) != 0u && merge_opens(t, T, A.window));
                if (open == 0u) break;
                const uint32_t next = (uint32_t)__ffsll((unsigned long long)open) - 1u;
                opened |= 1ull << next;
                T = time_of_lane(t, next);
                behind &= ~((2ull << next) - 1ull);                                     // (next = 63: 2 << 63 = 0, nobody is left)
            }
            if (have) {
                A.opens[i] = (uint32_t)(opened >> lane) & 1u;
                A.owner[i] = s;
            }
        }
    }
}

__global__ void __launch_bounds__(256) merge_count_kernel(const MergeDeviceArgs A)
{
    const uint32_t n = A.header[SH_KEPT];
    const uint64_t start = (uint64_t)blockIdx.x * kSeriesTile;
    if (start >= n) return;
    __shared__ uint32_t openers;
    if (threadIdx.x == 0u) openers = 0u;
    __syncthreads();
    uint32_t mine = 0u;
#pragma unroll
    for (uint32_t r = 0; r < 8u; ++r) {
        const uint64_t i = start + r * 256u + threadIdx.x;
        if (i < n && A.opens[i] != 0u) ++mine;
    }
    if (mine != 0u) atomicAdd(&openers, mine);
    __syncthreads();
    if (threadIdx.x == 0u) A.tile_counts[blockIdx.x] = openers;
}

__global__ void __launch_bounds__(256) merge_group_kernel(const MergeDeviceArgs A)
{
    const uint32_t n = A.header[SH_KEPT];
    const uint64_t start = (uint64_t)blockIdx.x * kSeriesTile;
    if (start >= n) return;
    __shared__ uint32_t wave_openers[4];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint64_t openers[8];
    uint32_t total = 0u;
#pragma unroll
    for (uint32_t r = 0; r < 8u; ++r) {
        const uint64_t i = start + wave * 512u + r * 64u + lane;
        openers[r] = __ballot(i < n && A.opens[i] != 0u);
        total += (uint32_t)__popcll(openers[r]);
    }
    if (lane == 0u) wave_openers[wave] = total;
    __syncthreads();
    uint32_t index = A.tile_counts[blockIdx.x];         // scanned: the group the tile's first opener starts
    for (uint32_t w = 0; w < wave; ++w) index += wave_openers[w];
#pragma unroll
    for (uint32_t r = 0; r < 8u; ++r) {
        const uint64_t i = start + wave * 512u + r * 64u + lane;
        if (i < n) {
            const uint32_t before = index + lanes_below(openers[r]);                    // openers in front of this record
            if ((openers[r] >> lane) & 1u) {
                A.group[i] = before;                                                    // < openers <= n <= capacity
                A.position[before] = (uint32_t)i;
                const uint64_t *record = reinterpret_cast<const uint64_t *>(A.in + i);
                uint64_t *merged = reinterpret_cast<uint64_t *>(A.merged + before);
                merged[0] = record[0] & 0xffffffff00000000ull;                          // npe: merge_close_kernel; string ID, OM ID
                merged[1] = record[1];                                                  // the opener's time
            } else {
                A.group[i] = before != 0u ? before - 1u : 0u;                           // (the first record of a series is an opener)
            }
        }
        index += (uint32_t)__popcll(openers[r]);
    }
}

__global__ void __launch_bounds__(256) merge_close_kernel(const MergeDeviceArgs A)
{
    const uint32_t n = A.header[SH_KEPT], n_series = A.header[MH_SERIES], n_merged = A.header[SH_SERIES];
    for (uint64_t g = blockIdx.x * 256u + threadIdx.x; g < n_merged; g += gridDim.x * 256u) {
        const uint32_t next = g + 1u < n_merged ? A.position[g + 1u] : n;
        A.merged[g].npe = next - A.position[g];
    }
    for (uint64_t s = blockIdx.x * 256u + threadIdx.x; s < n_series; s += gridDim.x * 256u) {
        clsimhip_mcpe_series entry = A.series[s];
        const uint32_t first = entry.first < n ? A.group[entry.first] : n_merged;
        uint32_t next = n_merged;
        if (s + 1u < n_series) {
            const uint32_t at = A.series[s + 1u].first;
            if (at < n) next = A.group[at];
        }
        entry.first = first;
        entry.count = next - first;
        A.merged_series[s] = entry;
    }
    if (blockIdx.x == 0u && threadIdx.x == 0u) A.header[MH_MERGED] = n_merged;          // (SH_SERIES receives the parents' total next)
}

__global__ void __launch_bounds__(256) merge_parent_key_kernel(const MergeDeviceArgs A)
{
    __shared__ uint32_t hist[12u * 256u];               // digits 4 ... 15; digits 0 ... 3 are those of the constant word
    for (uint32_t i = threadIdx.x; i < 12u * 256u; i += 256u) hist[i] = 0u;
    __syncthreads();
    const uint32_t n = A.header[SH_KEPT];
    for (uint64_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint32_t s = A.owner[i];                                                  // < series, or 0: zeroed, then merge_open_kernel's
        const uint32_t at = A.series[s].first;
        SeriesKey key;
        key.group = s;
        key.t_hi = A.in[i].identifier;
        key.t_lo = A.group[i] - (at < n ? A.group[at] : 0u);
        key.identifier = 0u;
        *reinterpret_cast<uint4 *>(A.keys[0] + i) = make_uint4(key.group, key.t_hi, key.t_lo, key.identifier);
#pragma unroll
        for (uint32_t p = 4u; p < 16u; ++p) atomicAdd(&hist[(p - 4u) * 256u + series_digit(key, p)], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 12u * 256u; i += 256u)
        if (hist[i] != 0u) atomicAdd(A.histogram + 4u * 256u + i, hist[i]);
    if (blockIdx.x == 0u && threadIdx.x < 4u) A.histogram[threadIdx.x * 256u] = n;     // the constant word: every key has digit 0
}

__device__ __forceinline__ bool differ(const uint4 &a, const uint4 &b) { return a.x != b.x || a.y != b.y || a.z != b.z || a.w != b.w; }

__global__ void __launch_bounds__(256) merge_parent_count_kernel(const MergeDeviceArgs A)
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
        if (i < n && (i == 0u || differ(load_words(keys + i), load_words(keys + i - 1u)))) ++mine;
    }
    if (mine != 0u) atomicAdd(&heads, mine);
    __syncthreads();
    if (threadIdx.x == 0u) A.tile_counts[blockIdx.x] = heads;
}

__global__ void __launch_bounds__(256) merge_parent_emit_kernel(const MergeDeviceArgs A)
{
    const uint32_t n = A.header[SH_KEPT], n_series = A.header[MH_SERIES];
    const uint64_t start = (uint64_t)blockIdx.x * kSeriesTile;
    if (start >= n) return;
    __shared__ uint32_t wave_heads[4];
    const SeriesKey *keys = A.keys[A.header[SH_FINAL]];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint4 key[8];
    uint64_t heads[8];
    bool starts[8];                                     // the key's series differs from its predecessor's
    uint32_t total = 0u;
#pragma unroll
    for (uint32_t r = 0; r < 8u; ++r) {
        const uint64_t i = start + wave * 512u + r * 64u + lane;
        bool head = false;
        starts[r] = false;
        if (i < n) {
            key[r] = load_words(keys + i);
            if (i == 0u) head = starts[r] = true;
            else {
                const uint4 before = load_words(keys + i - 1u);
                head = differ(key[r], before);
                starts[r] = key[r].x != before.x;
            }
        }
        heads[r] = __ballot(head);
        total += (uint32_t)__popcll(heads[r]);
    }
    if (lane == 0u) wave_heads[wave] = total;
    __syncthreads();
    uint32_t index = A.tile_counts[blockIdx.x];         // scanned: the entry the tile's first head makes
    for (uint32_t w = 0; w < wave; ++w) index += wave_heads[w];
#pragma unroll
    for (uint32_t r = 0; r < 8u; ++r) {
        if ((heads[r] >> lane) & 1u) {
            const uint32_t p = index + lanes_below(heads[r]);                           // < heads <= n <= capacity
            *reinterpret_cast<uint64_t *>(A.parents + p) = (uint64_t)key[r].y | ((uint64_t)key[r].z << 32);   // identifier, index
            if (starts[r] && key[r].x < n_series) A.ranges[key[r].x].first = p;         // count: merge_finish_kernel
        }
        index += (uint32_t)__popcll(heads[r]);
    }
}

__global__ void __launch_bounds__(256) merge_finish_kernel(const MergeDeviceArgs A)
{
    const uint32_t n_series = A.header[MH_SERIES], n_parents = A.header[SH_SERIES];
    for (uint64_t s = blockIdx.x * 256u + threadIdx.x; s < n_series; s += gridDim.x * 256u) {
        const uint32_t next = s + 1u < n_series ? A.ranges[s + 1u].first : n_parents;
        A.ranges[s].count = next - A.ranges[s].first;
    }
    if (blockIdx.x == 0u && threadIdx.x == 0u) {
        A.counts[0] = A.header[MH_MERGED];
        A.counts[1] = n_parents;
    }
}

size_t round16(size_t v) { return (v + 15u) & ~size_t{15}; }

// the workspace: header and histogram (zeroed together by every call), tile counts, two key buffers, then four words per record:
// flag and series (zeroed together), group, and per group the opener's position
struct MergeWorkspace {
    size_t histogram, tile_counts, keys0, keys1, opens, owner, group, position, bytes;
    explicit MergeWorkspace(size_t capacity)
    {
        const size_t tiles = std::max<size_t>((capacity + kSeriesTile - 1u) / kSeriesTile, 1u);
        const size_t records = std::max<size_t>(capacity, 1u);
        histogram = kSeriesHeaderWords * sizeof(uint32_t);
        tile_counts = histogram + 16u * 256u * sizeof(uint32_t);
        keys0 = round16(tile_counts + 256u * tiles * sizeof(uint32_t));
        keys1 = keys0 + records * sizeof(SeriesKey);
        opens = keys1 + records * sizeof(SeriesKey);
        owner = opens + round16(records * sizeof(uint32_t));
        group = owner + round16(records * sizeof(uint32_t));
        position = group + round16(records * sizeof(uint32_t));
        bytes = position + round16(records * sizeof(uint32_t));
    }
};

hipError_t launch_mcpe_merge(const MergeDeviceArgs &A, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(A.header, 0, (kSeriesHeaderWords + 16u * 256u) * sizeof(uint32_t), stream);     // header and histogram lie together
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(A.opens, 0, reinterpret_cast<uint8_t *>(A.group) - reinterpret_cast<uint8_t *>(A.opens), stream);     // flags and series
    if (e != hipSuccess) return e;
    uint32_t lanes = (A.capacity + 255u) / 256u;
    if (A.capacity > 0xffffff00u || lanes > 1024u) lanes = 1024u;
    if (lanes == 0u) lanes = 1u;
    uint32_t tiles = (uint32_t)(((uint64_t)A.capacity + kSeriesTile - 1u) / kSeriesTile);
    if (tiles == 0u) tiles = 1u;
    SeriesDeviceArgs S{};                               // what the series stage's sort passes and tile scan read
    S.capacity = A.capacity;
    S.header = A.header;
    S.histogram = A.histogram;
    S.tile_counts = A.tile_counts;
    S.keys[0] = A.keys[0];
    S.keys[1] = A.keys[1];
    hipLaunchKernelGGL(merge_open_kernel, dim3(lanes), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(merge_count_kernel, dim3(tiles), dim3(256), 0, stream, A);
    launch_series_tile_scan(S, stream);
    hipLaunchKernelGGL(merge_group_kernel, dim3(tiles), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(merge_close_kernel, dim3(lanes), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(merge_parent_key_kernel, dim3(lanes), dim3(256), 0, stream, A);
    launch_series_sort(S, stream);
    hipLaunchKernelGGL(merge_parent_count_kernel, dim3(tiles), dim3(256), 0, stream, A);
    launch_series_tile_scan(S, stream);
    hipLaunchKernelGGL(merge_parent_emit_kernel, dim3(tiles), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(merge_finish_kernel, dim3(lanes), dim3(256), 0, stream, A);
    return hipGetLastError();
}

} // namespace

size_t mcpe_merge_workspace_bytes(size_t capacity) { return MergeWorkspace(capacity).bytes; }

void mcpe_merge_device(int device, const void *d_records, const void *d_series, const void *d_series_counts, size_t capacity, double window,
                       void *d_merged, void *d_merged_series, void *d_parents, void *d_ranges, void *d_counts, void *d_workspace,
                       size_t workspace_bytes, hipStream_t stream)
{
    if (!merge_window_ok(window)) throw Error(CLSIMHIP_ERR_ARGUMENT, "MCPE merging: the window must be a number with 0 <= window < +inf");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) throw Error(CLSIMHIP_ERR_DEVICE, "no HIP device available (MCPE merging's device path has no CPU fallback)");
    if (device < 0 || device >= count) throw Error(CLSIMHIP_ERR_ARGUMENT, "device ordinal out of range");
    if (!d_series_counts || !d_counts || !d_workspace) throw Error(CLSIMHIP_ERR_ARGUMENT, "device pointers are (null)");
    if (capacity && (!d_records || !d_series || !d_merged || !d_merged_series || !d_parents || !d_ranges))
        throw Error(CLSIMHIP_ERR_ARGUMENT, "d_records / d_series / d_merged / d_merged_series / d_parents / d_ranges is (null)");
    if (capacity > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "capacity beyond 2^32 - 1 records");
    auto at = [](const void *p) { return reinterpret_cast<uintptr_t>(p); };
    if ((at(d_records) & 7u) || (at(d_series) & 7u) || (at(d_merged) & 7u) || (at(d_merged_series) & 7u) || (at(d_parents) & 7u) || (at(d_ranges) & 7u) ||
        (at(d_workspace) & 15u) || (at(d_counts) & 3u) || (at(d_series_counts) & 3u))
        throw Error(CLSIMHIP_ERR_ARGUMENT, "d_records, d_series and the four outputs must be aligned to 8 bytes, d_workspace to 16, d_series_counts and d_counts to 4");
    const MergeWorkspace W(capacity);
    if (workspace_bytes < W.bytes) throw Error(CLSIMHIP_ERR_ARGUMENT, "the MCPE merging workspace holds " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(W.bytes) + " are needed");
    DeviceGuard on_device(device);
    uint8_t *ws = static_cast<uint8_t *>(d_workspace);
    MergeDeviceArgs A{};
    A.in = static_cast<const clsimhip_mcpe *>(d_records);
    A.series = static_cast<const clsimhip_mcpe_series *>(d_series);
    A.series_counts = static_cast<const uint32_t *>(d_series_counts);
    A.capacity = static_cast<uint32_t>(capacity);
    A.window = window;
    A.header = reinterpret_cast<uint32_t *>(ws);
    A.histogram = reinterpret_cast<uint32_t *>(ws + W.histogram);
    A.tile_counts = reinterpret_cast<uint32_t *>(ws + W.tile_counts);
    A.keys[0] = reinterpret_cast<SeriesKey *>(ws + W.keys0);
    A.keys[1] = reinterpret_cast<SeriesKey *>(ws + W.keys1);
    A.opens = reinterpret_cast<uint32_t *>(ws + W.opens);
    A.owner = reinterpret_cast<uint32_t *>(ws + W.owner);
    A.group = reinterpret_cast<uint32_t *>(ws + W.group);
    A.position = reinterpret_cast<uint32_t *>(ws + W.position);
    A.merged = static_cast<clsimhip_mcpe_merged *>(d_merged);
    A.merged_series = static_cast<clsimhip_mcpe_series *>(d_merged_series);
    A.parents = static_cast<clsimhip_mcpe_parent *>(d_parents);
    A.ranges = static_cast<clsimhip_mcpe_parent_range *>(d_ranges);
    A.counts = static_cast<uint32_t *>(d_counts);
    const hipError_t e = launch_mcpe_merge(A, stream);
    if (e != hipSuccess) throw Error(CLSIMHIP_ERR_DEVICE, std::string("MCPE merging kernel launch: ") + hipGetErrorString(e));
}

} // namespace clsimhip
