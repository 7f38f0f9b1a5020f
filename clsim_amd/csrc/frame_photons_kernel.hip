// Frame photons on the device: the definition of frame_photons.h as a sorting stage behind assemble_hits_kernel, for gfx950 (wave64).
//
// The MCPE series stage's radix passes (mcpe_series_kernel.hip) sort 128-bit keys and carry nothing.  A photon is not described by such
// a key, so they run twice, through launch_series_sort, with the record's index as the key's fourth word.  The sort is a stable LSD
// radix sort: round B keeps round A's order among its ties.
//
//   frame_photons_key_a_kernel   one lane per photon: groups 0 and 2 of the record -> DOM rank, particle lookup, mask, time shift
//                                (series_make_key); a kept photon's groups 1 and 4 -> h.  Appended per wave (ballot, population
//                                count, one atomic per wave): round A's key (identifier, h, 0, append position) and, at the append
//                                position, (group, t_hi, t_lo, source index).  The histogram it counts holds every kept key in bin 0 of
//                                passes 0-3: the plan kernel finds those digits constant, so the index takes no part in the sort.
//   launch_series_sort           round A: ascending in (identifier, h); ties in append order
//   frame_photons_key_b_kernel   in round A's output order: (group, t_hi, t_lo, source index), and round B's histogram likewise
//   launch_series_sort           round B: ascending in (group, tkey), then (identifier, h); ties in append order
//   frame_photons_heads_kernel   per tile: the records whose group differs from their predecessor's (series heads) and those that
//                                differ in (group, tkey, identifier, h) (run heads); launch_series_tile_scan, once for each
//   frame_photons_emit_kernel    gathers the 48-byte record through the source index, writes the series entries, every run's first
//                                record, and marks a run in which two neighbours differ in content
//   frame_photons_tie_kernel     one workgroup per marked run at a time: a run of more than kFramePhotonsTieBound members is counted,
//                                every member of a shorter one finds its rank by comparison within the run (content, then position:
//                                equal contents are equal records) and writes its record there.  Every loop is bounded by 2 048.
//   frame_photons_close_kernel   the series' counts and the count block
//
// Everything reads its sizes from device memory: nothing waits for the host, and a workgroup with nothing to do leaves at once.
// Atomics only count; no position in the output comes from the arrival order of an atomic.  Propagated photons differ in their
// times: runs of more than one record are rare, marked runs need crafted input, and the tie kernel then reads one word per run.
#include "frame_photons.h"

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
__device__ __forceinline__ void store_key(SeriesKey *p, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    *reinterpret_cast<uint4 *>(p) = make_uint4(a, b, c, d);
}

__device__ __forceinline__ const uint4 *groups_of(const FramePhotonsDeviceArgs &A, uint32_t source)
{
    return reinterpret_cast<const uint4 *>(A.in + source);         // source < min(*in_count, capacity)
}

// identifier, module word and content of record `source`: groups 0, 1, 2 and 4
__device__ __forceinline__ void load_content(const FramePhotonsDeviceArgs &A, uint32_t source, uint32_t &identifier, uint32_t &module, FramePhotonContent &c)
{
    const uint4 *g = groups_of(A, source);
    const uint4 g0 = g[0], g1 = g[1], g2 = g[2], g4 = g[4];
    const uint32_t a0[4] = {g0.x, g0.y, g0.z, g0.w}, a1[4] = {g1.x, g1.y, g1.z, g1.w}, a2[4] = {g2.x, g2.y, g2.z, g2.w}, a4[4] = {g4.x, g4.y, g4.z, g4.w};
    frame_photons_content(a0, a1, a2, a4, c);
    identifier = g2.z;
    module = g2.w;
}

// two neighbours of the sorted keys: 0 = another run, 1 = the same run and the same content, 2 = the same run, contents differ
__device__ __forceinline__ uint32_t relation(const FramePhotonsDeviceArgs &A, const SeriesKey &before, const SeriesKey &k)
{
    if (before.group != k.group || before.t_hi != k.t_hi || before.t_lo != k.t_lo) return 0u;
    uint32_t ia, ib, module;
    FramePhotonContent a, b;
    load_content(A, before.identifier, ia, module, a);
    load_content(A, k.identifier, ib, module, b);
    if (ia != ib || frame_photons_mix(a) != frame_photons_mix(b)) return 0u;
    return frame_photons_compare(a, b) == 0 ? 1u : 2u;
}

// the wave's share of a pass over kept keys: every kept key in bin 0 of passes [0, constant_passes), by digit above
__device__ __forceinline__ void count_digits(uint32_t *hist, const SeriesKey &key, bool have, uint64_t kept, uint32_t lane, uint32_t constant_passes)
{
    if (lane == 0u)
        for (uint32_t p = 0; p < constant_passes; ++p) atomicAdd(&hist[p * 256u], (uint32_t)__popcll(kept));
    if (have)
        for (uint32_t p = constant_passes; p < 16u; ++p) atomicAdd(&hist[p * 256u + series_digit(key, p)], 1u);
}

__global__ void __launch_bounds__(256) frame_photons_key_a_kernel(const FramePhotonsDeviceArgs A)
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
        uint4 g0 = make_uint4(0u, 0u, 0u, 0u), g2 = g0;
        if (i < n) {
            const uint4 *g = groups_of(A, (uint32_t)i);
            g0 = g[0]; g2 = g[2];
            code = series_make_key(A.lookup, g2.z, g2.w, (double)__builtin_bit_cast(float, g0.w), key);
        }
        const uint64_t kept = __ballot(code == FRAME_PHOTONS_KEPT);
        if (kept != 0u) {
            uint32_t base = 0u;
            if (lane == 0u) base = atomicAdd(A.header + SH_KEPT, (uint32_t)__popcll(kept));
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            SeriesKey a;
            a.group = 0u; a.t_hi = 0u; a.t_lo = 0u; a.identifier = 0u;
            if (code == FRAME_PHOTONS_KEPT) {
                const uint4 *g = groups_of(A, (uint32_t)i);
                const uint4 g1 = g[1], g4 = g[4];
                const uint32_t a0[4] = {g0.x, g0.y, g0.z, g0.w}, a1[4] = {g1.x, g1.y, g1.z, g1.w}, a2[4] = {g2.x, g2.y, g2.z, g2.w}, a4[4] = {g4.x, g4.y, g4.z, g4.w};
                FramePhotonContent c;
                frame_photons_content(a0, a1, a2, a4, c);
                const uint32_t at = base + lanes_below(kept);               // kept <= n <= capacity
                a.group = g2.z; a.t_hi = frame_photons_mix(c); a.identifier = at;
                store_key(A.keys[0] + (size_t)at, a.group, a.t_hi, 0u, at);
                store_key(A.placed + (size_t)at, key.group, key.t_hi, key.t_lo, (uint32_t)i);
            }
            count_digits(hist, a, code == FRAME_PHOTONS_KEPT, kept, lane, 8u);      // (the index and the zero word)
        }
#pragma unroll
        for (int c = FRAME_PHOTONS_UNKNOWN_PARTICLE; c <= FRAME_PHOTONS_UNKNOWN_DOM; ++c) {
            const uint64_t met = __ballot(code == c);
            if (met != 0u && lane == 0u) atomicAdd(A.header + SH_COUNTERS + c, (uint32_t)__popcll(met));
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 16u * 256u; i += 256u)
        if (hist[i] != 0u) atomicAdd(A.histogram[0] + i, hist[i]);
}

__global__ void __launch_bounds__(256) frame_photons_key_b_kernel(const FramePhotonsDeviceArgs A)
{
    const uint32_t n = A.header[SH_KEPT];
    if ((uint64_t)blockIdx.x * 256u >= n) return;
    __shared__ uint32_t hist[16u * 256u];
    for (uint32_t i = threadIdx.x; i < 16u * 256u; i += 256u) hist[i] = 0u;
    __syncthreads();
    if (blockIdx.x == 0u && threadIdx.x == 0u) A.header[FH_RUNS + SH_KEPT] = n;
    const SeriesKey *sorted = A.keys[A.header[SH_FINAL]];                   // round A's output: keys[0] or keys[1]
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t first = blockIdx.x * 256u + (threadIdx.x & ~63u); first < n; first += gridDim.x * 256u) {
        const uint64_t j = first + lane;
        SeriesKey key;
        key.group = 0u; key.t_hi = 0u; key.t_lo = 0u; key.identifier = 0u;
        if (j < n) {
            const uint32_t at = load_key(sorted + j).identifier;            // < kept: key A wrote it
            key = load_key(A.placed + at);
            store_key(A.keys[2] + j, key.group, key.t_hi, key.t_lo, key.identifier);
            A.run_mixed[j] = 0u;                                            // (runs <= kept)
        }
        count_digits(hist, key, j < n, __ballot(j < n), lane, 4u);          // (the index)
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 16u * 256u; i += 256u)
        if (hist[i] != 0u) atomicAdd(A.histogram[1] + i, hist[i]);
}

// (round B sorted in keys[2] and keys[0])
__device__ __forceinline__ const SeriesKey *sorted_keys(const FramePhotonsDeviceArgs &A) { return A.header[SH_FINAL] ? A.keys[0] : A.keys[2]; }

__global__ void __launch_bounds__(256) frame_photons_heads_kernel(const FramePhotonsDeviceArgs A)
{
    const uint32_t n = A.header[SH_KEPT];
    const uint64_t start = (uint64_t)blockIdx.x * kSeriesTile;
    if (start >= n) return;
    __shared__ uint32_t heads, runs;
    if (threadIdx.x == 0u) { heads = 0u; runs = 0u; }
    __syncthreads();
    const SeriesKey *keys = sorted_keys(A);
    uint32_t my_heads = 0u, my_runs = 0u;
#pragma unroll
    for (uint32_t r = 0; r < 8u; ++r) {
        const uint64_t i = start + r * 256u + threadIdx.x;
        if (i < n) {
            if (i == 0u) { ++my_heads; ++my_runs; continue; }
            const SeriesKey k = load_key(keys + i), before = load_key(keys + i - 1u);
            if (k.group != before.group) ++my_heads;
            if (relation(A, before, k) == 0u) ++my_runs;
        }
    }
    if (my_heads != 0u) atomicAdd(&heads, my_heads);
    if (my_runs != 0u) atomicAdd(&runs, my_runs);
    __syncthreads();
    if (threadIdx.x == 0u) { A.tile_counts[blockIdx.x] = heads; A.run_counts[blockIdx.x] = runs; }
}

__global__ void __launch_bounds__(256) frame_photons_emit_kernel(const FramePhotonsDeviceArgs A)
{
    const uint32_t n = A.header[SH_KEPT];
    const uint64_t start = (uint64_t)blockIdx.x * kSeriesTile;
    if (start >= n) return;
    __shared__ uint32_t wave_heads[4], wave_runs[4];
    const SeriesKey *keys = sorted_keys(A);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    SeriesKey key[8];
    uint64_t heads[8], runs[8], mixed[8];
    uint32_t total_heads = 0u, total_runs = 0u;
#pragma unroll
    for (uint32_t r = 0; r < 8u; ++r) {
        const uint64_t i = start + wave * 512u + r * 64u + lane;
        bool head = false, run = false, differs = false;
        if (i < n) {
            key[r] = load_key(keys + i);
            if (i == 0u) {
                head = true; run = true;
            } else {
                const SeriesKey before = load_key(keys + i - 1u);
                head = key[r].group != before.group;
                const uint32_t rel = relation(A, before, key[r]);
                run = rel == 0u;
                differs = rel == 2u;
            }
        }
        heads[r] = __ballot(head);
        runs[r] = __ballot(run);
        mixed[r] = __ballot(differs);
        total_heads += (uint32_t)__popcll(heads[r]);
        total_runs += (uint32_t)__popcll(runs[r]);
    }
    if (lane == 0u) { wave_heads[wave] = total_heads; wave_runs[wave] = total_runs; }
    __syncthreads();
    uint32_t index = A.tile_counts[blockIdx.x];         // scanned: the series the tile's first head starts
    uint32_t run_index = A.run_counts[blockIdx.x];      // scanned: the run the tile's first run head starts
    for (uint32_t w = 0; w < wave; ++w) { index += wave_heads[w]; run_index += wave_runs[w]; }
    const uint32_t n_doms = A.lookup.n_doms;
#pragma unroll
    for (uint32_t r = 0; r < 8u; ++r) {
        const uint64_t i = start + wave * 512u + r * 64u + lane;
        if (i < n) {
            const SeriesKey &k = key[r];
            uint32_t identifier, module;
            FramePhotonContent c;
            load_content(A, k.identifier, identifier, module, c);
            const uint64_t t = __builtin_bit_cast(uint64_t, series_time_of(((uint64_t)k.t_hi << 32) | k.t_lo));
            uint4 *record = reinterpret_cast<uint4 *>(A.out + i);
            record[0] = make_uint4(identifier, module, (uint32_t)t, (uint32_t)(t >> 32));
            record[1] = make_uint4(c.w[0], c.w[1], c.w[2], c.w[3]);
            record[2] = make_uint4(c.w[4], c.w[5], c.w[6], c.w[7]);
            if ((heads[r] >> lane) & 1u) {
                const uint32_t s = index + lanes_below(heads[r]);           // < series <= n
                const uint32_t frame_rank = k.group / n_doms;               // (a kept key: there is a DOM)
                *reinterpret_cast<uint4 *>(A.series + s) = make_uint4(A.frames[frame_rank], module, (uint32_t)i, 0u);      // count: close
            }
            // the run this record is in: the heads up to and including its own lane, minus one
            const uint32_t run = run_index + (uint32_t)__popcll(runs[r] & (~0ull >> (63u - lane))) - 1u;       // < runs <= n
            if ((runs[r] >> lane) & 1u) A.run_first[run] = (uint32_t)i;
            if ((mixed[r] >> lane) & 1u) A.run_mixed[run] = 1u;             // (every writer writes 1)
        }
        index += (uint32_t)__popcll(heads[r]);
        run_index += (uint32_t)__popcll(runs[r]);
    }
}

__global__ void __launch_bounds__(256) frame_photons_tie_kernel(const FramePhotonsDeviceArgs A)
{
    const uint32_t n = A.header[SH_KEPT], n_runs = A.header[FH_RUNS + SH_SERIES];
    if ((uint64_t)blockIdx.x * 256u >= n_runs) return;
    __shared__ uint32_t found[256];
    __shared__ uint32_t n_found;
    const SeriesKey *keys = sorted_keys(A);
    // (the same number of trips in every lane of the workgroup: they meet at the barriers)
    for (uint64_t first = (uint64_t)blockIdx.x * 256u; first < n_runs; first += (uint64_t)gridDim.x * 256u) {
        if (threadIdx.x == 0u) n_found = 0u;
        __syncthreads();
        const uint64_t run = first + threadIdx.x;
        if (run < n_runs && A.run_mixed[run] != 0u) found[atomicAdd(&n_found, 1u)] = (uint32_t)run;     // in any order: each is handled alike
        __syncthreads();
        const uint32_t todo = n_found;                                      // <= 256
        for (uint32_t f = 0; f < todo; ++f) {
            const uint32_t which = found[f];
            const uint32_t begin = A.run_first[which];
            const uint32_t end = which + 1u < n_runs ? A.run_first[which + 1u] : n;
            const uint32_t members = end - begin;
            if (members > kFramePhotonsTieBound) {
                if (threadIdx.x == 0u) atomicAdd(A.header + FH_TIE_OVERFLOW, members);
                continue;
            }
            for (uint32_t m = threadIdx.x; m < members; m += 256u) {        // <= 8 trips
                const SeriesKey k = load_key(keys + begin + m);
                uint32_t identifier, module, other_identifier, other_module;
                FramePhotonContent mine, other;
                load_content(A, k.identifier, identifier, module, mine);
                uint32_t rank = 0u;
                for (uint32_t j = 0; j < members; ++j) {                    // <= 2 048 trips
                    load_content(A, keys[begin + j].identifier, other_identifier, other_module, other);
                    const int order = frame_photons_compare(other, mine);
                    rank += (order < 0 || (order == 0 && j < m)) ? 1u : 0u;
                }
                const uint64_t t = __builtin_bit_cast(uint64_t, series_time_of(((uint64_t)k.t_hi << 32) | k.t_lo));
                uint4 *record = reinterpret_cast<uint4 *>(A.out + (size_t)(begin + rank));     // the ranks are a permutation of the run
                record[0] = make_uint4(identifier, module, (uint32_t)t, (uint32_t)(t >> 32));
                record[1] = make_uint4(mine.w[0], mine.w[1], mine.w[2], mine.w[3]);
                record[2] = make_uint4(mine.w[4], mine.w[5], mine.w[6], mine.w[7]);
            }
        }
        __syncthreads();                                                    // (found is written again in the next trip)
    }
}

__global__ void __launch_bounds__(256) frame_photons_close_kernel(const FramePhotonsDeviceArgs A)
{
    const uint32_t n = A.header[SH_KEPT], n_series = A.header[SH_SERIES];
    for (uint64_t s = blockIdx.x * 256u + threadIdx.x; s < n_series; s += gridDim.x * 256u) {
        const uint32_t next = s + 1u < n_series ? A.series[s + 1u].first : n;
        A.series[s].count = next - A.series[s].first;
    }
    if (blockIdx.x == 0u && threadIdx.x < 6u) {
        const uint32_t overflow = A.header[FH_TIE_OVERFLOW];
        uint32_t v = threadIdx.x < 5u ? A.header[threadIdx.x] : overflow;
        if (threadIdx.x < 2u && overflow != 0u) v = 0u;                     // no records from a bunch that met the bound
        A.counts[threadIdx.x] = v;
    }
}

} // namespace

hipError_t launch_frame_photons(const FramePhotonsDeviceArgs &A, hipStream_t stream)
{
    // header and both histograms lie together
    hipError_t e = hipMemsetAsync(A.header, 0, (kSeriesHeaderWords + 2u * 16u * 256u) * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    uint32_t lanes = (A.capacity + 255u) / 256u;
    if (A.capacity > 0xffffff00u || lanes > 1024u) lanes = 1024u;
    if (lanes == 0u) lanes = 1u;
    uint32_t tiles = (uint32_t)(((uint64_t)A.capacity + kSeriesTile - 1u) / kSeriesTile);
    if (tiles == 0u) tiles = 1u;
    SeriesDeviceArgs round_a{}, round_b{}, run_scan{};      // what the MCPE series stage's sort passes and tile scan read
    round_a.capacity = A.capacity;
    round_a.header = A.header;
    round_a.histogram = A.histogram[0];
    round_a.tile_counts = A.tile_counts;
    round_a.keys[0] = A.keys[0];
    round_a.keys[1] = A.keys[1];
    round_b = round_a;
    round_b.histogram = A.histogram[1];
    round_b.keys[0] = A.keys[2];
    round_b.keys[1] = A.keys[0];
    run_scan = round_a;
    run_scan.header = A.header + FH_RUNS;
    run_scan.tile_counts = A.run_counts;
    hipLaunchKernelGGL(frame_photons_key_a_kernel, dim3(lanes), dim3(256), 0, stream, A);
    launch_series_sort(round_a, stream);
    hipLaunchKernelGGL(frame_photons_key_b_kernel, dim3(lanes), dim3(256), 0, stream, A);
    launch_series_sort(round_b, stream);
    hipLaunchKernelGGL(frame_photons_heads_kernel, dim3(tiles), dim3(256), 0, stream, A);
    launch_series_tile_scan(round_b, stream);
    launch_series_tile_scan(run_scan, stream);
    hipLaunchKernelGGL(frame_photons_emit_kernel, dim3(tiles), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(frame_photons_tie_kernel, dim3(lanes), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(frame_photons_close_kernel, dim3(lanes), dim3(256), 0, stream, A);
    return hipGetLastError();
}

} // namespace clsimhip
