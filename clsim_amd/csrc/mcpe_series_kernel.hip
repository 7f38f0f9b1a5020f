// MCPE series on the device: the definition of mcpe_series.h as a sorting stage behind mcpe_kernel, for gfx950 (wave64).
//
//   series_key_kernel      one lane per MCPE: DOM rank, particle lookup, mask, time shift -> 16-byte key, appended per wave (ballot,
//                          population count, one atomic per wave; the append order is arbitrary and the sort removes it); the same
//                          pass counts the 16 x 256 digit histograms of the kept keys (LDS, then one atomic per non-empty bin).
//   series_plan_kernel     a digit that is the same in every key needs no pass: which passes are live, and which of the two key
//                          buffers each one reads.  Frame, DOM rank and identifier rarely fill their 32 bits, times share their
//                          exponent bytes.
//   per live pass (stable LSD radix sort, 8-bit digits, least significant first):
//     series_count_kernel  digit counts of every tile of 2048 keys
//     series_scan_kernel   exclusive scan over (digit, tile), digit major: where each tile's keys of each digit start
//     series_scatter_kernel every wave walks its 512 keys of the tile in index order, 64 at a time; a key's place among the keys of
//                          its digit in that round comes from ballots over the digit's bits (the lanes with the same digit, and how
//                          many of them sit below), the digit's running offset from the lowest such lane.  No position comes from
//                          the arrival order of an atomic: atomics only count.
//   series_heads_kernel / series_scan_kernel / series_emit_kernel / series_close_kernel
//                          a key whose group differs from its predecessor's starts a series; the records are rebuilt from the keys
//                          (identifier, DOM of the rank, time of the time key: equal keys are equal records).
//
// Everything reads its sizes from device memory (the MCPE counter, the kept count): nothing waits for the host, and a workgroup
// with nothing to do leaves at once.  A pass moves 16 B in and 16 B out per key plus the tile counts; the keys of one tile are read
// once and held in registers between counting and scattering.
#include "mcpe_series.h"

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

__global__ void __launch_bounds__(256) series_key_kernel(const SeriesDeviceArgs A)
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
            const uint64_t ids = rec[0];
            code = series_make_key(A.lookup, (uint32_t)ids, (uint32_t)(ids >> 32), __builtin_bit_cast(double, rec[1]), key);
        }
        const uint64_t kept = __ballot(code == SERIES_KEPT);
        if (kept != 0u) {
            uint32_t base = 0u;
            if (lane == 0u) base = atomicAdd(A.header + SH_KEPT, (uint32_t)__popcll(kept));
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            if (code == SERIES_KEPT) {
                store_key(A.keys[0] + (size_t)(base + lanes_below(kept)), key);     // kept <= n <= capacity
#pragma unroll
                for (uint32_t p = 0; p < 16u; ++p) atomicAdd(&hist[p * 256u + series_digit(key, p)], 1u);
            }
        }
#pragma unroll
        for (int c = SERIES_UNKNOWN_PARTICLE; c <= SERIES_UNKNOWN_DOM; ++c) {
            const uint64_t met = __ballot(code == c);
            if (met != 0u && lane == 0u) atomicAdd(A.header + SH_COUNTERS + c, (uint32_t)__popcll(met));
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 16u * 256u; i += 256u)
        if (hist[i] != 0u) atomicAdd(A.histogram + i, hist[i]);
}

__global__ void __launch_bounds__(64) series_plan_kernel(const SeriesDeviceArgs A)
{
    __shared__ uint32_t constant[16];
    const uint32_t kept = A.header[SH_KEPT];
    if (threadIdx.x < 16u) {
        uint32_t all_in_one = 0u;
        for (uint32_t d = 0; d < 256u; ++d) all_in_one |= (A.histogram[threadIdx.x * 256u + d] == kept) ? 1u : 0u;
        constant[threadIdx.x] = all_in_one;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t current = 0u;
        for (uint32_t p = 0; p < 16u; ++p) {
            const uint32_t live = (constant[p] == 0u && kept > 1u) ? 1u : 0u;
            A.header[SH_LIVE + p] = live;
            A.header[SH_SOURCE + p] = current;
            current ^= live;
        }
        A.header[SH_FINAL] = current;
    }
}

__global__ void __launch_bounds__(256) series_count_kernel(const SeriesDeviceArgs A, const uint32_t pass)
{
    if (A.header[SH_LIVE + pass] == 0u) return;
    const uint32_t n = A.header[SH_KEPT];
    const uint64_t start = (uint64_t)blockIdx.x * kSeriesTile;
    if (start >= n) return;
    __shared__ uint32_t count[256];
    count[threadIdx.x] = 0u;
    __syncthreads();
    const SeriesKey *src = A.keys[A.header[SH_SOURCE + pass]];
#pragma unroll
    for (uint32_t r = 0; r < 8u; ++r) {
        const uint64_t i = start + r * 256u + threadIdx.x;
        if (i < n) atomicAdd(&count[series_digit(load_key(src + i), pass)], 1u);
    }
    __syncthreads();
    const uint32_t tiles = (n + kSeriesTile - 1u) / kSeriesTile;
    A.tile_counts[(size_t)threadIdx.x * tiles + blockIdx.x] = count[threadIdx.x];
}

// in-place exclusive scan of tile_counts[0 .. per_tile x tiles in use), one workgroup that walks the array 1024 entries at a time
// (neighbouring lanes touch neighbouring words) and carries the sum along; which = 0 ... 15: the counts of that pass (256 per
// tile), 16: the series heads (one per tile; the total is the number of series)
__global__ void __launch_bounds__(1024) series_scan_kernel(const SeriesDeviceArgs A, const uint32_t which)
{
    if (which < 16u && A.header[SH_LIVE + which] == 0u) return;
    const uint32_t n = A.header[SH_KEPT];
    const uint32_t tiles = (n + kSeriesTile - 1u) / kSeriesTile;
    const uint64_t total = (uint64_t)tiles * (which < 16u ? 256u : 1u);
    __shared__ uint32_t wave_sum[16];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t carry = 0u;                        // the same in every lane
    for (uint64_t base = 0; base < total; base += 1024u) {
        const uint64_t i = base + threadIdx.x;
        const uint32_t v = i < total ? A.tile_counts[i] : 0u;
        uint32_t inclusive = v;
#pragma unroll
        for (uint32_t step = 1u; step < 64u; step *= 2u) {
            const uint32_t below = __shfl_up(inclusive, step);
            if (lane >= step) inclusive += below;
        }
        if (lane == 63u) wave_sum[wave] = inclusive;
        __syncthreads();
        uint32_t before = 0u, all = 0u;
        for (uint32_t w = 0; w < 16u; ++w) {
            const uint32_t s = wave_sum[w];
            before += w < wave ? s : 0u;
            all += s;
        }
        if (i < total) A.tile_counts[i] = carry + before + (inclusive - v);
        carry += all;
        __syncthreads();                        // (wave_sum is written again in the next round)
    }
    if (which == 16u && threadIdx.x == 0u) A.header[SH_SERIES] = carry;
}

__global__ void __launch_bounds__(256) series_scatter_kernel(const SeriesDeviceArgs A, const uint32_t pass)
{
    if (A.header[SH_LIVE + pass] == 0u) return;
    const uint32_t n = A.header[SH_KEPT];
    const uint64_t start = (uint64_t)blockIdx.x * kSeriesTile;
    if (start >= n) return;
    __shared__ uint32_t offset[4][256];         // per wave and digit: first the count, then the running output position
    for (uint32_t w = 0; w < 4u; ++w) offset[w][threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t source = A.header[SH_SOURCE + pass];
    const SeriesKey *src = A.keys[source];
    SeriesKey *dst = A.keys[source ^ 1u];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    // the tile in index order: wave w holds keys [512 w, 512 w + 512), round r of it keys [64 r, 64 r + 64), one per lane
    SeriesKey key[8];
    uint32_t digit[8];
#pragma unroll
    for (uint32_t r = 0; r < 8u; ++r) {
        const uint64_t i = start + wave * 512u + r * 64u + lane;
        digit[r] = 256u;                        // no key
        if (i < n) {
            key[r] = load_key(src + i);
            digit[r] = series_digit(key[r], pass);
            atomicAdd(&offset[wave][digit[r]], 1u);
        }
    }
    __syncthreads();
    {
        const uint32_t tiles = (n + kSeriesTile - 1u) / kSeriesTile;
        uint32_t position = A.tile_counts[(size_t)threadIdx.x * tiles + blockIdx.x];       // scanned: the tile's first key of this digit
        for (uint32_t w = 0; w < 4u; ++w) {
            const uint32_t c = offset[w][threadIdx.x];
            offset[w][threadIdx.x] = position;
            position += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < 8u; ++r) {
        const bool have = digit[r] < 256u;
        const uint32_t d = digit[r] & 255u;
        uint64_t peers = __ballot(have);        // the lanes of this round with the same digit
#pragma unroll
        for (uint32_t bit = 0; bit < 8u; ++bit) {
            const bool set = ((d >> bit) & 1u) != 0u;
            const uint64_t m = __ballot(set);
            peers &= set ? m : ~m;
        }
        const uint32_t leader = have ? (uint32_t)__ffsll((unsigned long long)peers) - 1u : lane;
        uint32_t base = 0u;
        if (have && lane == leader) {           // one lane per digit touches the digit's offset: no two lanes meet in LDS
            base = offset[wave][d];
            offset[wave][d] = base + (uint32_t)__popcll(peers);
        }
        base = (uint32_t)__shfl((int)base, (int)leader);
        if (have) store_key(dst + (size_t)(base + lanes_below(peers)), key[r]);    // < n: the scanned counts partition [0, n)
        // the next round's leader of a digit may be another lane: its read comes after this write
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

__device__ __forceinline__ bool is_head(const SeriesKey *keys, uint64_t i)
{
    return i == 0u || keys[i].group != keys[i - 1u].group;
}

__global__ void __launch_bounds__(256) series_heads_kernel(const SeriesDeviceArgs A)
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
        if (i < n && is_head(keys, i)) ++mine;
    }
    if (mine != 0u) atomicAdd(&heads, mine);
    __syncthreads();
    if (threadIdx.x == 0u) A.tile_counts[blockIdx.x] = heads;
}

__global__ void __launch_bounds__(256) series_emit_kernel(const SeriesDeviceArgs A)
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
    const uint32_t n_doms = A.lookup.n_doms;
#pragma unroll
    for (uint32_t r = 0; r < 8u; ++r) {
        const uint64_t i = start + wave * 512u + r * 64u + lane;
        if (i < n) {
            const SeriesKey &k = key[r];
            const uint32_t frame_rank = k.group / n_doms;
            const uint32_t dom = A.dom_of_rank[k.group - frame_rank * n_doms];
            uint64_t *record = reinterpret_cast<uint64_t *>(A.out + i);
            record[0] = (uint64_t)k.identifier | ((uint64_t)dom << 32);
            record[1] = __builtin_bit_cast(uint64_t, series_time_of(((uint64_t)k.t_hi << 32) | k.t_lo));
            if ((heads[r] >> lane) & 1u) {
                const uint32_t s = index + lanes_below(heads[r]);       // < series <= n
                uint64_t *entry = reinterpret_cast<uint64_t *>(A.series + s);
                entry[0] = (uint64_t)(A.frames ? A.frames[frame_rank] : 0u) | ((uint64_t)dom << 32);
                entry[1] = (uint64_t)(uint32_t)i;                       // count: series_close_kernel
            }
        }
        index += (uint32_t)__popcll(heads[r]);
    }
}

__global__ void __launch_bounds__(256) series_close_kernel(const SeriesDeviceArgs A)
{
    const uint32_t n = A.header[SH_KEPT], n_series = A.header[SH_SERIES];
    for (uint64_t s = blockIdx.x * 256u + threadIdx.x; s < n_series; s += gridDim.x * 256u) {
        const uint32_t next = s + 1u < n_series ? A.series[s + 1u].first : n;
        A.series[s].count = next - A.series[s].first;
    }
    if (blockIdx.x == 0u && threadIdx.x < 5u) A.counts[threadIdx.x] = A.header[threadIdx.x];
}

} // namespace

namespace {
uint32_t tiles_of(uint32_t capacity)
{
    const uint32_t tiles = (uint32_t)(((uint64_t)capacity + kSeriesTile - 1u) / kSeriesTile);
    return tiles == 0u ? 1u : tiles;
}
} // namespace

void launch_series_sort(const SeriesDeviceArgs &A, hipStream_t stream)
{
    const uint32_t tiles = tiles_of(A.capacity);
    hipLaunchKernelGGL(series_plan_kernel, dim3(1), dim3(64), 0, stream, A);
    for (uint32_t pass = 0; pass < 16u; ++pass) {
        hipLaunchKernelGGL(series_count_kernel, dim3(tiles), dim3(256), 0, stream, A, pass);
        hipLaunchKernelGGL(series_scan_kernel, dim3(1), dim3(1024), 0, stream, A, pass);
        hipLaunchKernelGGL(series_scatter_kernel, dim3(tiles), dim3(256), 0, stream, A, pass);
    }
}

void launch_series_tile_scan(const SeriesDeviceArgs &A, hipStream_t stream)
{
    hipLaunchKernelGGL(series_scan_kernel, dim3(1), dim3(1024), 0, stream, A, 16u);
}

hipError_t launch_mcpe_series(const SeriesDeviceArgs &A, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(A.header, 0, (kSeriesHeaderWords + 16u * 256u) * sizeof(uint32_t), stream);     // header and histogram lie together
    if (e != hipSuccess) return e;
    uint32_t lanes = (A.capacity + 255u) / 256u;
    if (A.capacity > 0xffffff00u || lanes > 1024u) lanes = 1024u;
    if (lanes == 0u) lanes = 1u;
    const uint32_t tiles = tiles_of(A.capacity);
    hipLaunchKernelGGL(series_key_kernel, dim3(lanes), dim3(256), 0, stream, A);
    launch_series_sort(A, stream);
    hipLaunchKernelGGL(series_heads_kernel, dim3(tiles), dim3(256), 0, stream, A);
    launch_series_tile_scan(A, stream);
    hipLaunchKernelGGL(series_emit_kernel, dim3(tiles), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(series_close_kernel, dim3(lanes), dim3(256), 0, stream, A);
    return hipGetLastError();
}

} // namespace clsimhip
