// Event statistics frame store on the device: the definition of event_stats_store.h as three stages and the device store, for gfx950
// (wave64).  A record is nine 16-byte quarters; no kernel reads or writes it in smaller pieces except its key (the first 8 bytes).
//
// CANON
//   canon_keys_kernel        one lane per record, nine 16-byte loads: empty or not, the identifier behind the map (bisection), and the
//                            pair (key, index | empty << 31).  Only pairs are sorted; EMPTY_DROPPED and RELABELLED are counted per wave.
//   canon_sort_*_kernel      a bitonic network on the pairs, all comparators ascending, for any length: positions beyond the input count
//                            as +infinity.  Distances below the tile are done in LDS (one kernel per stage), the others in HBM.  The
//                            order is (empty, key, index): total, so the result does not depend on how the network is scheduled.
//   canon_heads_kernel / launch_series_tile_scan / canon_runs_kernel
//                            a pair whose key differs from its predecessor's opens a run; per tile the heads are counted, scanned, and
//                            every run's first position is written.
//   canon_sum_kernel         a wave takes 64 runs.  A run shorter than kEventStatsLongRun is summed by one lane; every longer one by the
//                            whole wave: lanes stride over the run, gather each record once and add its 32-bit limbs into uint64
//                            deferred-carry slots (at most 2^31 limbs below 2^32: no overflow), the slots are summed across the wave
//                            and carries are propagated once, modulo 2^384.
// COMBINE
//   combine_check_kernel / combine_plan_kernel / combine_partition_kernel
//                            the local checks of both forms, the effective sizes, and the merge path's diagonal per tile of the merged
//                            sequence (ties: A first), as in the frame stores' union.
//   combine_heads_kernel / launch_series_tile_scan / combine_fit_kernel / combine_emit_kernel
//                            a tile holds its keys of A and B in LDS; a record of B whose key A holds (in the tile, or A's last record
//                            in front of it) is no head: it is added to A's record.  Output positions come from the scan over the heads.
//                            A result that does not fit is A alone.
// SPLIT
//   split_plan_kernel / split_copy_kernel   a bisection on the frame, then copies by quarters.
//
// Everything reads its sizes from device memory: nothing waits for the host.  Atomics only count.  Every loop is bounded by a capacity
// and every index is clamped to one, whatever bytes the inputs hold.  Plain vector stores only.
#include "event_stats_store.h"

#include "series_union_device.hip.h"

namespace clsimhip {

namespace {

static_assert(kEventStatsStoreTile == kSeriesTile, "the tile scan of the series stage walks tiles of kSeriesTile");
constexpr uint32_t kTile = kEventStatsStoreTile;
constexpr uint32_t kWords = kEventStatsRecordWords, kQuads = kEventStatsRecordQuads;
constexpr uint32_t kEmptyBit = 0x80000000u;

// header words beside SH_KEPT (the pairs that are not empty / the merged length) and SH_SERIES (the scan's total: runs / output records)
enum StoreHeader : uint32_t { EH_RELABELLED = 2, EH_EMPTY = 3, EH_MALFORMED_A = 2, EH_MALFORMED_B = 3, EH_OVERFLOW = 4, EH_RECORDS = 5,
                              EH_N = 40 /* CANON: the input's records */, EH_N_A = 40 /* COMBINE: the effective sizes */, EH_N_B = 41, EH_IN_A = 42, EH_IN_B = 43 };

struct EventStatsTag {};                                                // names store_note_kernel's launch in a trace

// ---- records ----
__device__ __forceinline__ void load_words(const uint4 *records, uint32_t i, uint32_t w[kWords])
{
    const uint4 *p = records + (size_t)i * kQuads;
#pragma unroll
    for (uint32_t q = 0; q < kQuads; ++q) {
        const uint4 v = p[q];
        w[4u * q] = v.x; w[4u * q + 1u] = v.y; w[4u * q + 2u] = v.z; w[4u * q + 3u] = v.w;
    }
}
__device__ __forceinline__ void store_words(uint4 *records, uint32_t i, const uint32_t w[kWords])
{
    uint4 *p = records + (size_t)i * kQuads;
#pragma unroll
    for (uint32_t q = 0; q < kQuads; ++q) p[q] = make_uint4(w[4u * q], w[4u * q + 1u], w[4u * q + 2u], w[4u * q + 3u]);
}
__device__ __forceinline__ uint64_t key_at(const uint4 *records, uint32_t i)
{
    const uint2 v = *reinterpret_cast<const uint2 *>(records + (size_t)i * kQuads);
    return event_stats_store_key(v.x, v.y);
}
// a += b on words, by ADD
__device__ __forceinline__ void add_words(uint32_t a[kWords], const uint32_t b[kWords])
{
    clsimhip_event_statistics ra, rb;
    __builtin_memcpy(&ra, a, sizeof ra);
    __builtin_memcpy(&rb, b, sizeof rb);
    event_stats_add(ra, rb);
    __builtin_memcpy(a, &ra, sizeof ra);
}

// ---- deferred-carry accumulators of one run ----
struct RunSum {
    uint64_t limb[24];                                                  // generated_sum's twelve, at_doms_sum's twelve
    uint64_t count[2];
    uint32_t special[6];
};
__device__ __forceinline__ void run_clear(RunSum &s)
{
#pragma unroll
    for (uint32_t k = 0; k < 24u; ++k) s.limb[k] = 0u;
    s.count[0] = 0u; s.count[1] = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 6u; ++k) s.special[k] = 0u;
}
__device__ __forceinline__ void run_add(RunSum &s, const uint32_t w[kWords])
{
#pragma unroll
    for (uint32_t k = 0; k < 24u; ++k) s.limb[k] += w[6u + k];
    s.count[0] += (uint64_t)w[2] | ((uint64_t)w[3] << 32);
    s.count[1] += (uint64_t)w[4] | ((uint64_t)w[5] << 32);
#pragma unroll
    for (uint32_t k = 0; k < 6u; ++k) s.special[k] += w[30u + k];
}
// the sum over the wave's 64 lanes, all of them here, in every lane
__device__ __forceinline__ void run_wave_sum(RunSum &s)
{
#pragma unroll
    for (int step = 1; step < 64; step *= 2) {
#pragma unroll
        for (uint32_t k = 0; k < 24u; ++k) s.limb[k] += __shfl_xor((unsigned long long)s.limb[k], step);
        s.count[0] += __shfl_xor((unsigned long long)s.count[0], step);
        s.count[1] += __shfl_xor((unsigned long long)s.count[1], step);
#pragma unroll
        for (uint32_t k = 0; k < 6u; ++k) s.special[k] += __shfl_xor(s.special[k], step);
    }
}
// carries propagated once, the carry out of limb 11 dropped: modulo 2^384
__device__ __forceinline__ void run_close(const RunSum &s, uint64_t key, uint32_t w[kWords])
{
    w[0] = (uint32_t)key; w[1] = (uint32_t)(key >> 32);
    w[2] = (uint32_t)s.count[0]; w[3] = (uint32_t)(s.count[0] >> 32);
    w[4] = (uint32_t)s.count[1]; w[5] = (uint32_t)(s.count[1] >> 32);
#pragma unroll
    for (uint32_t side = 0; side < 2u; ++side) {
        uint64_t carry = 0u;
#pragma unroll
        for (uint32_t k = 0; k < 12u; ++k) {
            const uint64_t v = s.limb[12u * side + k] + carry;          // slot < 2^63, carry < 2^32
            w[6u + 12u * side + k] = (uint32_t)v;
            carry = v >> 32;
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < 6u; ++k) w[30u + k] = s.special[k];
}

// ---- a tile's flags -> how many are set in front of each element, in element order (element e = round x 256 + lane of the workgroup) ----
__device__ __forceinline__ void tile_scan(const bool flag[kRounds], uint32_t *cnt /* LDS, 4 x kRounds */, uint32_t before[kRounds], uint32_t &total)
{
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint64_t ballots[kRounds];
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        ballots[r] = __ballot(flag[r]);
        if (lane == 0u) cnt[r * 4u + wave] = (uint32_t)__popcll(ballots[r]);
    }
    __syncthreads();
    uint32_t run = 0u;
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
#pragma unroll
        for (uint32_t w = 0; w < 4u; ++w) {
            if (w == wave) before[r] = run + lanes_below(ballots[r]);
            run += cnt[r * 4u + w];
        }
    }
    total = run;
    __syncthreads();                                                    // (cnt may be written again)
}

// first index in keys[0, n) whose key is not below `key`
__device__ __forceinline__ uint32_t lower_bound_lds(const uint64_t *keys, uint32_t n, uint64_t key)
{
    uint32_t lo = 0u, hi = n;
    while (lo < hi) {                                                   // at most 12 trips: n <= kTile
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (keys[mid] < key) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// =====================================================================================================================================
// CANON
// =====================================================================================================================================
struct CanonArgs {
    const uint4 *records;
    const uint32_t *count;                  // records = min(*count, capacity)
    uint32_t capacity;
    const clsimhip_relabel *map;            // device memory
    uint32_t n_map;
    uint32_t *header;                       // kSeriesHeaderWords
    uint32_t *tile_counts;                  // heads per tile, scanned in place
    uint64_t *keys;                         // per record
    uint32_t *index;                        // per record: its place in the input | empty << 31
    uint32_t *run_first;                    // by run: the first of its pairs; capacity + 1
    uint4 *out;
    uint32_t out_capacity;
    uint32_t *out_counts;                   // five: records, 0, RELABELLED, EMPTY_DROPPED, overflow
    const uint32_t *head_counts;            // (may be null) the counts of the split that made the input: its overflow is passed on
};

__global__ void __launch_bounds__(256) canon_keys_kernel(const CanonArgs A)
{
    const uint32_t n = min_u32(*A.count, A.capacity), lane = threadIdx.x & 63u;
    if (blockIdx.x == 0u && threadIdx.x == 0u) A.header[EH_N] = n;
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t first = (uint64_t)blockIdx.x * 256u + (threadIdx.x & ~63u); first < n; first += stride) {      // the same in a wave's lanes
        const uint64_t i = first + lane;
        bool empty = false, hit = false;
        if (i < n) {
            uint32_t w[kWords];
            load_words(A.records, (uint32_t)i, w);                      // i < n <= capacity
            empty = event_stats_store_words_empty(w);
            const uint32_t identifier = empty ? w[0] : event_stats_store_relabel(A.map, A.n_map, w[0], &hit);
            A.keys[i] = event_stats_store_key(identifier, w[1]);
            A.index[i] = (uint32_t)i | (empty ? kEmptyBit : 0u);        // i < 2^31
        }
        const uint64_t empties = __ballot(empty), hits = __ballot(hit);
        if (lane == 0u && empties != 0u) atomicAdd(A.header + EH_EMPTY, (uint32_t)__popcll(empties));
        if (lane == 0u && hits != 0u) atomicAdd(A.header + EH_RELABELLED, (uint32_t)__popcll(hits));
    }
}

// the order of the pairs: the empty ones last, then the key, then the place in the input
__device__ __forceinline__ bool pair_less(uint64_t key_a, uint32_t index_a, uint64_t key_b, uint32_t index_b)
{
    const uint32_t empty_a = index_a >> 31, empty_b = index_b >> 31;
    if (empty_a != empty_b) return empty_a < empty_b;
    if (key_a != key_b) return key_a < key_b;
    return index_a < index_b;
}

// comparator t of a step: the lower position i and the higher one l.  j = 0: the stage's first step, i against its mirror image in
// the block of k; else i against i | j.
__device__ __forceinline__ void comparator(uint64_t t, uint64_t k, uint64_t j, uint64_t &i, uint64_t &l)
{
    const uint64_t d = j ? j : k >> 1;
    i = ((t & ~(d - 1u)) << 1) | (t & (d - 1u));
    l = j ? (i | j) : (i ^ (k - 1u));
}

// one step whose distance reaches beyond a tile, in HBM; stage k is idle when the input fits one sorted block of k / 2
__global__ void __launch_bounds__(256) canon_sort_global_kernel(const CanonArgs A, const uint64_t k, const uint64_t j)
{
    const uint32_t n = A.header[EH_N];
    if ((k >> 1) >= n) return;
    for (uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x; t < n; t += (uint64_t)gridDim.x * 256u) {
        uint64_t i, l;
        comparator(t, k, j, i, l);
        if (i >= n) break;                                              // (i grows with t)
        if (l >= n) continue;                                           // +infinity stays where it is
        const uint64_t key_i = A.keys[i], key_l = A.keys[l];            // i < l < n <= capacity
        const uint32_t index_i = A.index[i], index_l = A.index[l];
        if (pair_less(key_l, index_l, key_i, index_i)) {
            A.keys[i] = key_l; A.index[i] = index_l;
            A.keys[l] = key_i; A.index[l] = index_i;
        }
    }
}

// the steps whose distance stays inside a tile, in LDS.  k = 0: every stage up to the tile (the tile is sorted); else the steps
// j = kTile / 2 ... 1 of stage k.
__global__ void __launch_bounds__(256) canon_sort_local_kernel(const CanonArgs A, const uint64_t k)
{
    const uint32_t n = A.header[EH_N];
    const uint64_t base = (uint64_t)blockIdx.x * kTile;
    if (base >= n || (k != 0u && (k >> 1) >= n)) return;
    __shared__ uint64_t keys[kTile];
    __shared__ uint32_t index[kTile];
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t e = r * 256u + threadIdx.x;
        const bool have = base + e < n;
        keys[e] = have ? A.keys[base + e] : ~0ull;                      // +infinity: nothing is above it
        index[e] = have ? A.index[base + e] : ~0u;
    }
    __syncthreads();
    const auto step = [&](uint32_t kk, uint32_t jj) {
#pragma unroll
        for (uint32_t r = 0; r < kRounds / 2u; ++r) {                   // kTile / 2 comparators
            uint64_t i, l;
            comparator(r * 256u + threadIdx.x, kk, jj, i, l);           // i < l < kTile
            if (pair_less(keys[l], index[l], keys[i], index[i])) {
                const uint64_t key = keys[i];
                const uint32_t at = index[i];
                keys[i] = keys[l]; index[i] = index[l];
                keys[l] = key; index[l] = at;
            }
        }
        __syncthreads();
    };
    if (k == 0u) {
        for (uint32_t kk = 2u; kk <= kTile; kk *= 2u) {
            step(kk, 0u);
            for (uint32_t jj = kk / 4u; jj >= 1u; jj /= 2u) step(kk, jj);
        }
    } else {
        for (uint32_t jj = kTile / 2u; jj >= 1u; jj /= 2u) step(kTile, jj);
    }
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t e = r * 256u + threadIdx.x;
        if (base + e < n) { A.keys[base + e] = keys[e]; A.index[base + e] = index[e]; }
    }
}

__global__ void __launch_bounds__(64) canon_plan_kernel(const CanonArgs A)
{
    if (threadIdx.x != 0u) return;
    const uint32_t n = A.header[EH_N], empty = min_u32(A.header[EH_EMPTY], n);
    A.header[SH_KEPT] = n - empty;                                      // the sorted pairs that carry a record
}

// whether pair p of the m that carry a record opens a run
__device__ __forceinline__ bool canon_is_head(const CanonArgs &A, uint64_t p, uint32_t m)
{
    if (p >= m) return false;
    return p == 0u || A.keys[p] != A.keys[p - 1u];
}

__global__ void __launch_bounds__(256) canon_heads_kernel(const CanonArgs A)
{
    const uint32_t m = A.header[SH_KEPT];
    const uint64_t base = (uint64_t)blockIdx.x * kTile;
    if (base >= m) return;
    __shared__ uint32_t cnt[4u * kRounds];
    bool flag[kRounds];
    uint32_t before[kRounds], total;
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) flag[r] = canon_is_head(A, base + r * 256u + threadIdx.x, m);
    tile_scan(flag, cnt, before, total);
    if (threadIdx.x == 0u) A.tile_counts[blockIdx.x] = total;           // blockIdx.x < tiles(m) <= tiles(capacity)
}

__global__ void __launch_bounds__(256) canon_runs_kernel(const CanonArgs A)
{
    const uint32_t m = A.header[SH_KEPT];
    const uint64_t base = (uint64_t)blockIdx.x * kTile;
    if (blockIdx.x == 0u && threadIdx.x == 0u) A.run_first[min_u32(A.header[SH_SERIES], A.capacity)] = m;      // where the last run ends
    if (base >= m) return;
    __shared__ uint32_t cnt[4u * kRounds];
    bool flag[kRounds];
    uint32_t before[kRounds], total;
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) flag[r] = canon_is_head(A, base + r * 256u + threadIdx.x, m);
    tile_scan(flag, cnt, before, total);
    const uint32_t offset = A.tile_counts[blockIdx.x];
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r)
        if (flag[r]) A.run_first[min_u32(offset + before[r], A.capacity)] = (uint32_t)(base + r * 256u + threadIdx.x);
}

__global__ void __launch_bounds__(256) canon_sum_kernel(const CanonArgs A)
{
    const uint32_t n = A.header[EH_N], m = A.header[SH_KEPT], runs = min_u32(A.header[SH_SERIES], m);
    if (runs > A.out_capacity) return;                                  // does not fit: nothing is delivered
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t group = (uint64_t)blockIdx.x * 256u + (threadIdx.x & ~63u); group < runs; group += stride) {    // the same in a wave's lanes
        const uint64_t r = group + lane;
        uint32_t first = 0u, end = 0u;
        if (r < runs) {                                                 // r + 1 <= runs <= capacity
            first = min_u32(A.run_first[r], m);
            end = min_u32(A.run_first[r + 1u], m);
            if (end < first) end = first;
        }
        const uint32_t length = end - first;
        RunSum sum;
        uint32_t w[kWords];
        if (length != 0u && length < kEventStatsLongRun) {              // a short run: this lane alone
            run_clear(sum);
            for (uint32_t p = first; p < end; ++p) {
                load_words(A.records, min_u32(A.index[p] & ~kEmptyBit, n - 1u), w);
                run_add(sum, w);
            }
            run_close(sum, A.keys[first], w);
            store_words(A.out, (uint32_t)r, w);                         // r < runs <= out_capacity
        }
        uint64_t todo = __ballot(length >= kEventStatsLongRun);
        while (todo != 0u) {                                            // a long run: the whole wave
            const int leader = __builtin_ctzll(todo);
            todo &= todo - 1u;
            const uint32_t from = __shfl(first, leader), to = __shfl(end, leader);
            run_clear(sum);
            for (uint64_t p = (uint64_t)from + lane; p < to; p += 64u) {
                load_words(A.records, min_u32(A.index[p] & ~kEmptyBit, n - 1u), w);
                run_add(sum, w);
            }
            run_wave_sum(sum);
            if (lane == 0u) {
                run_close(sum, A.keys[from], w);
                store_words(A.out, (uint32_t)(group + (uint32_t)leader), w);
            }
        }
    }
}

__global__ void __launch_bounds__(64) canon_close_kernel(const CanonArgs A)
{
    if (threadIdx.x != 0u) return;
    const uint32_t runs = min_u32(A.header[SH_SERIES], A.header[SH_KEPT]);
    const bool fits = runs <= A.out_capacity;
    A.out_counts[0] = fits ? runs : 0u;
    A.out_counts[1] = 0u;
    A.out_counts[ESC_RELABELLED] = A.header[EH_RELABELLED];
    A.out_counts[ESC_EMPTY_DROPPED] = A.header[EH_EMPTY];
    A.out_counts[ESC_OVERFLOW] = fits ? (A.head_counts ? A.head_counts[ESC_OVERFLOW] : 0u) : runs;
}

// the workspace of all three stages: header, one word per tile and one per tile boundary of capacity_a + capacity_b records, then per
// record of A a key, an index and a run start (and one more), and eight bytes per record of B (CANON: per map entry)
struct StoreWorkspace {
    size_t tile_counts, partition, keys, index, run_first, map, bytes;
    StoreWorkspace(size_t capacity_a, size_t capacity_b)
    {
        const size_t tiles = tiles_of(capacity_a + capacity_b);
        tile_counts = kSeriesHeaderWords * sizeof(uint32_t);
        partition = tile_counts + round16(tiles * sizeof(uint32_t));
        keys = partition + round16((tiles + 1u) * sizeof(uint32_t));
        index = keys + round16(std::max<size_t>(capacity_a, 1u) * sizeof(uint64_t));
        run_first = index + round16(std::max<size_t>(capacity_a, 1u) * sizeof(uint32_t));
        map = run_first + round16((capacity_a + 1u) * sizeof(uint32_t));
        bytes = map + round16(std::max<size_t>(capacity_b, 1u) * sizeof(clsimhip_relabel));
    }
};

hipError_t launch_canon(const CanonArgs &A, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(A.header, 0, kSeriesHeaderWords * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const uint32_t tiles = tiles_of(A.capacity), lanes = lanes_of(A.capacity);
    SeriesDeviceArgs S{};                                               // what the series stage's tile scan reads
    S.capacity = A.capacity;
    S.header = A.header;
    S.tile_counts = A.tile_counts;
    hipLaunchKernelGGL(canon_keys_kernel, dim3(lanes), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(canon_plan_kernel, dim3(1), dim3(64), 0, stream, A);
    hipLaunchKernelGGL(canon_sort_local_kernel, dim3(tiles), dim3(256), 0, stream, A, (uint64_t)0u);
    for (uint64_t k = 2u * kTile; (k >> 1) < A.capacity; k *= 2u) {
        hipLaunchKernelGGL(canon_sort_global_kernel, dim3(lanes), dim3(256), 0, stream, A, k, (uint64_t)0u);
        for (uint64_t j = k / 4u; j >= kTile; j /= 2u) hipLaunchKernelGGL(canon_sort_global_kernel, dim3(lanes), dim3(256), 0, stream, A, k, j);
        hipLaunchKernelGGL(canon_sort_local_kernel, dim3(tiles), dim3(256), 0, stream, A, k);
    }
    hipLaunchKernelGGL(canon_heads_kernel, dim3(tiles), dim3(256), 0, stream, A);
    launch_series_tile_scan(S, stream);
    hipLaunchKernelGGL(canon_runs_kernel, dim3(tiles), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(canon_sum_kernel, dim3(lanes), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(canon_close_kernel, dim3(1), dim3(64), 0, stream, A);
    return hipGetLastError();
}

// =====================================================================================================================================
// COMBINE
// =====================================================================================================================================
struct CombineArgs {
    const uint4 *a, *b;
    const uint32_t *a_count, *b_count;      // records = min(*count, capacity)
    uint32_t capacity_a, capacity_b, out_capacity;
    uint32_t *header;                       // kSeriesHeaderWords
    uint32_t *tile_counts;                  // heads per tile of the merged sequence, scanned in place
    uint32_t *partition;                    // per tile boundary: records of A in front of it
    uint4 *out;
    uint32_t *out_counts;                   // five: records, 0, MALFORMED in A, MALFORMED in B, overflow
};

// record i of a form of n: not empty, and above its predecessor in the key
__device__ __forceinline__ bool form_record_ok(const uint4 *records, uint32_t i)
{
    uint32_t w[kWords];
    load_words(records, i, w);
    if (event_stats_store_words_empty(w)) return false;
    return i == 0u || key_at(records, i - 1u) < event_stats_store_key(w[0], w[1]);
}

__global__ void __launch_bounds__(256) combine_check_kernel(const CombineArgs C)
{
    const uint32_t n_a = min_u32(*C.a_count, C.capacity_a), n_b = min_u32(*C.b_count, C.capacity_b);
    if (blockIdx.x == 0u && threadIdx.x == 0u) { C.header[EH_IN_A] = n_a; C.header[EH_IN_B] = n_b; }
    const uint64_t start = (uint64_t)blockIdx.x * 256u + threadIdx.x, stride = (uint64_t)gridDim.x * 256u;
    uint32_t bad_a = 0u, bad_b = 0u;
    for (uint64_t i = start; i < n_a; i += stride) bad_a += form_record_ok(C.a, (uint32_t)i) ? 0u : 1u;
    for (uint64_t i = start; i < n_b; i += stride) bad_b += form_record_ok(C.b, (uint32_t)i) ? 0u : 1u;
    if (bad_a != 0u) atomicAdd(C.header + EH_MALFORMED_A, bad_a);
    if (bad_b != 0u) atomicAdd(C.header + EH_MALFORMED_B, bad_b);
}

__global__ void __launch_bounds__(64) combine_plan_kernel(const CombineArgs C)
{
    if (threadIdx.x != 0u) return;
    uint32_t n_a = C.header[EH_IN_A], n_b = C.header[EH_IN_B], overflow = 0u;
    if (C.header[EH_MALFORMED_A] != 0u) {
        n_a = 0u; n_b = 0u;
    } else if (C.header[EH_MALFORMED_B] != 0u) {
        n_b = 0u;
    } else if ((uint64_t)n_a + n_b > 0xffffffffull) {                   // a merged sequence no 32-bit position walks
        overflow = 0xffffffffu;
        n_b = 0u;
    }
    if (n_a > C.out_capacity) {                                         // A alone does not fit either: nothing
        if (overflow == 0u) overflow = n_a;
        n_a = 0u; n_b = 0u;
    }
    C.header[EH_N_A] = n_a;
    C.header[EH_N_B] = n_b;
    C.header[EH_OVERFLOW] = overflow;
    C.header[SH_KEPT] = n_a + n_b;                                      // the merged sequence the tiles walk
}

__global__ void __launch_bounds__(256) combine_partition_kernel(const CombineArgs C)
{
    const uint32_t n_a = C.header[EH_N_A], n_b = C.header[EH_N_B];
    const uint32_t n = n_a + n_b;
    const uint32_t tiles = (uint32_t)(((uint64_t)n + kTile - 1u) / kTile);
    for (uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x; t <= tiles; t += (uint64_t)gridDim.x * 256u) {
        const uint64_t reach = t * kTile;
        const uint32_t diagonal = reach < n ? (uint32_t)reach : n;
        // the records of A among the first `diagonal` of the merged sequence: the first i with B[diagonal - i - 1] < A[i]
        uint32_t lo = diagonal > n_b ? diagonal - n_b : 0u, hi = diagonal < n_a ? diagonal : n_a;
        while (lo < hi) {                                               // at most 32 trips; mid < n_a, 0 <= diagonal - mid - 1 < n_b
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (key_at(C.b, diagonal - mid - 1u) < key_at(C.a, mid)) hi = mid; else lo = mid + 1u;
        }
        C.partition[t] = lo;                                            // t <= tiles(capacity_a + capacity_b)
    }
}

// what a tile of the merged sequence holds: A[i0, i0 + la) and B[j0, j0 + lb), la + lb <= kTile, every index below its form's size
struct CombineTile { uint32_t i0, la, j0, lb; };

__device__ __forceinline__ CombineTile combine_tile(const CombineArgs &C, uint32_t n_a, uint32_t n_b)
{
    const uint32_t n = n_a + n_b;
    const uint64_t d0 = (uint64_t)blockIdx.x * kTile;
    const uint32_t length = (uint32_t)(d0 + kTile < n ? kTile : n - d0);
    CombineTile T;
    T.i0 = min_u32(min_u32(C.partition[blockIdx.x], n_a), (uint32_t)d0);
    const uint32_t i1 = min_u32(C.partition[blockIdx.x + 1u], n_a);
    T.la = i1 > T.i0 ? min_u32(i1 - T.i0, length) : 0u;
    T.j0 = min_u32((uint32_t)d0 - T.i0, n_b);
    T.lb = min_u32(length - T.la, n_b - T.j0);
    return T;
}

// the tile's keys into LDS: A's first, then B's
__device__ __forceinline__ void combine_tile_keys(const CombineArgs &C, const CombineTile &T, uint64_t *keys)
{
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t e = r * 256u + threadIdx.x;
        if (e < T.la) keys[e] = key_at(C.a, T.i0 + e);
        else if (e < T.la + T.lb) keys[e] = key_at(C.b, T.j0 + (e - T.la));
    }
    __syncthreads();
}

// whether A holds the key of the tile's record b of B: in the tile, or -- for the first one -- as A's last record in front of the tile
__device__ __forceinline__ bool combine_b_matched(const CombineArgs &C, const CombineTile &T, const uint64_t *keys, uint32_t b)
{
    const uint64_t key = keys[T.la + b];
    const uint32_t at = lower_bound_lds(keys, T.la, key);
    if (at < T.la && keys[at] == key) return true;
    return b == 0u && T.i0 > 0u && key_at(C.a, T.i0 - 1u) == key;
}

__global__ void __launch_bounds__(256) combine_heads_kernel(const CombineArgs C)
{
    const uint32_t n_a = C.header[EH_N_A], n_b = C.header[EH_N_B];
    if ((uint64_t)blockIdx.x * kTile >= (uint64_t)n_a + n_b) return;
    __shared__ uint64_t keys[kTile];
    __shared__ uint32_t cnt[4u * kRounds];
    const CombineTile T = combine_tile(C, n_a, n_b);
    combine_tile_keys(C, T, keys);
    bool flag[kRounds];
    uint32_t before[kRounds], total;
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t b = r * 256u + threadIdx.x;
        flag[r] = b < T.lb && !combine_b_matched(C, T, keys, b);
    }
    tile_scan(flag, cnt, before, total);
    if (threadIdx.x == 0u) C.tile_counts[blockIdx.x] = T.la + total;    // every record of A is a head
}

// behind the scan: whether the result fits, and the output counts
__global__ void __launch_bounds__(64) combine_fit_kernel(const CombineArgs C)
{
    if (threadIdx.x != 0u) return;
    uint32_t overflow = C.header[EH_OVERFLOW], records = C.header[SH_SERIES];
    if (overflow == 0u && records > C.out_capacity) overflow = records;
    if (overflow != 0u) records = C.header[EH_N_A];                     // A alone (the plan has seen that it fits)
    C.header[EH_OVERFLOW] = overflow;
    C.header[EH_RECORDS] = records;
    C.out_counts[0] = records;
    C.out_counts[1] = 0u;
    C.out_counts[ESC_MALFORMED_A] = C.header[EH_MALFORMED_A];
    C.out_counts[ESC_MALFORMED_B] = C.header[EH_MALFORMED_B];
    C.out_counts[ESC_OVERFLOW] = overflow;
}

__global__ void __launch_bounds__(256) combine_emit_kernel(const CombineArgs C)
{
    const uint32_t n_a = C.header[EH_N_A], n_b = C.header[EH_N_B];
    if (C.header[EH_OVERFLOW] != 0u) {                                  // A alone, by quarters
        const uint64_t quads = (uint64_t)min_u32(C.header[EH_RECORDS], min_u32(n_a, C.out_capacity)) * kQuads;
        for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < quads; q += (uint64_t)gridDim.x * 256u) C.out[q] = C.a[q];
        return;
    }
    if ((uint64_t)blockIdx.x * kTile >= (uint64_t)n_a + n_b) return;
    __shared__ uint64_t keys[kTile];
    __shared__ uint32_t heads_before[kTile + 1u];                       // of B's records in the tile: the heads among those in front
    __shared__ uint32_t cnt[4u * kRounds];
    const CombineTile T = combine_tile(C, n_a, n_b);
    combine_tile_keys(C, T, keys);
    bool flag[kRounds];
    uint32_t before[kRounds], total;
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t b = r * 256u + threadIdx.x;
        flag[r] = b < T.lb && !combine_b_matched(C, T, keys, b);
    }
    tile_scan(flag, cnt, before, total);
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t b = r * 256u + threadIdx.x;
        if (b < T.lb) heads_before[b] = before[r];
    }
    if (threadIdx.x == 0u) heads_before[T.lb] = total;
    __syncthreads();
    const uint32_t offset = C.tile_counts[blockIdx.x];
    uint32_t w[kWords];
#pragma unroll 1
    for (uint32_t r = 0; r < kRounds; ++r) {                            // A's records: heads all, each with B's record of its key added
        const uint32_t a = r * 256u + threadIdx.x;
        if (a >= T.la) continue;
        const uint64_t key = keys[a];
        const uint32_t rank = lower_bound_lds(keys + T.la, T.lb, key);  // B's records of the tile below it
        const uint32_t j = T.j0 + rank;                                 // B's first record that is not below: in the tile, or the next tile's first
        const bool matched = rank < T.lb ? keys[T.la + rank] == key : (j < n_b && key_at(C.b, j) == key);
        load_words(C.a, T.i0 + a, w);
        if (matched) {
            uint32_t other[kWords];
            load_words(C.b, j, other);
            add_words(w, other);
        }
        const uint32_t to = offset + a + heads_before[rank];
        if (to < C.out_capacity) store_words(C.out, to, w);
    }
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {                            // B's records whose key A does not hold
        if (!flag[r]) continue;
        const uint32_t b = r * 256u + threadIdx.x;                      // < T.lb
        const uint32_t rank = lower_bound_lds(keys, T.la, keys[T.la + b]);
        load_words(C.b, T.j0 + b, w);
        const uint32_t to = offset + rank + before[r];
        if (to < C.out_capacity) store_words(C.out, to, w);
    }
}

hipError_t launch_combine(const CombineArgs &C, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(C.header, 0, kSeriesHeaderWords * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const uint64_t both = (uint64_t)C.capacity_a + C.capacity_b;
    const uint32_t tiles = tiles_of(both);
    SeriesDeviceArgs S{};                                               // what the series stage's tile scan reads
    S.capacity = both > 0xffffffffull ? 0xffffffffu : (uint32_t)both;
    S.header = C.header;
    S.tile_counts = C.tile_counts;
    hipLaunchKernelGGL(combine_check_kernel, dim3(lanes_of(std::max<uint64_t>(C.capacity_a, C.capacity_b))), dim3(256), 0, stream, C);
    hipLaunchKernelGGL(combine_plan_kernel, dim3(1), dim3(64), 0, stream, C);
    hipLaunchKernelGGL(combine_partition_kernel, dim3(lanes_of((uint64_t)tiles + 1u)), dim3(256), 0, stream, C);
    hipLaunchKernelGGL(combine_heads_kernel, dim3(tiles), dim3(256), 0, stream, C);
    launch_series_tile_scan(S, stream);
    hipLaunchKernelGGL(combine_fit_kernel, dim3(1), dim3(64), 0, stream, C);
    hipLaunchKernelGGL(combine_emit_kernel, dim3(tiles), dim3(256), 0, stream, C);
    return hipGetLastError();
}

// =====================================================================================================================================
// SPLIT
// =====================================================================================================================================
struct SplitArgs {
    const uint4 *records;
    const uint32_t *count;                  // records = min(*count, capacity)
    uint32_t capacity, last_frame;
    const uint32_t *blocked;                // (may be null) five words: any nonzero -> nothing is drained
    uint4 *head;                            // (null: the head is dropped -- the store's own plan)
    uint32_t *head_counts;                  // five: records, 0, 0, 0, overflow
    uint32_t head_capacity;
    uint4 *tail;
    uint32_t *tail_counts;                  // five: records, 0, 0, 0, 0
};

__global__ void __launch_bounds__(64) split_plan_kernel(const SplitArgs S)
{
    if (threadIdx.x != 0u) return;
    const uint32_t n = min_u32(*S.count, S.capacity);
    const uint4 *records = S.records;
    uint32_t head = event_stats_store_split_point([records](uint32_t i) { return key_at(records, i); }, n, S.last_frame);
    uint32_t overflow = 0u;
    if (head > S.head_capacity) {                                       // a head that does not fit drains nothing
        overflow = head;
        head = 0u;
    }
    if (S.blocked) {
        uint32_t any = 0u;
        for (uint32_t k = 0; k < 5u; ++k) any |= S.blocked[k];
        if (any != 0u) head = 0u;
    }
    S.head_counts[0] = head; S.head_counts[1] = 0u; S.head_counts[2] = 0u; S.head_counts[3] = 0u; S.head_counts[4] = overflow;
    S.tail_counts[0] = n - head; S.tail_counts[1] = 0u; S.tail_counts[2] = 0u; S.tail_counts[3] = 0u; S.tail_counts[4] = 0u;
}

__global__ void __launch_bounds__(256) split_copy_kernel(const SplitArgs S)
{
    const uint32_t n = min_u32(*S.count, S.capacity);
    const uint32_t head = min_u32(min_u32(S.head_counts[0], n), S.head ? S.head_capacity : n);
    const uint64_t quads = (uint64_t)n * kQuads, head_quads = (uint64_t)head * kQuads;
    for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < quads; q += (uint64_t)gridDim.x * 256u) {
        const uint4 v = S.records[q];                                   // q < 9 x capacity
        if (q >= head_quads) S.tail[q - head_quads] = v;                // the tail holds `capacity` records
        else if (S.head) S.head[q] = v;                                 // q < 9 x head_capacity
    }
}

hipError_t launch_split(const SplitArgs &S, hipStream_t stream)
{
    hipLaunchKernelGGL(split_plan_kernel, dim3(1), dim3(64), 0, stream, S);
    hipLaunchKernelGGL(split_copy_kernel, dim3(lanes_of((uint64_t)S.capacity * kQuads)), dim3(256), 0, stream, S);
    return hipGetLastError();
}

// =====================================================================================================================================
// the host side
// =====================================================================================================================================
const std::string kStore = "event statistics store";
constexpr size_t kRecordBytes = sizeof(clsimhip_event_statistics);

uintptr_t at(const void *p) { return reinterpret_cast<uintptr_t>(p); }
bool overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) { return a_bytes && b_bytes && at(a) < at(b) + b_bytes && at(b) < at(a) + a_bytes; }

void capacity_check(size_t capacity)
{
    if (capacity > kFrameStoreMaxCapacity) throw Error(CLSIMHIP_ERR_ARGUMENT, kStore + ": capacity beyond 2^31 records");
}

void workspace_check(size_t workspace_bytes, size_t needed)
{
    if (workspace_bytes < needed)
        throw Error(CLSIMHIP_ERR_ARGUMENT, "the " + kStore + " workspace holds " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(needed) + " are needed");
}

// CANON's arguments; the map lies wherever `d_map` says, the workspace is laid out for (capacity, layout_b)
CanonArgs canon_args(const void *d_records, const void *d_count, size_t capacity, const clsimhip_relabel *d_map, size_t n_map, void *d_out, void *d_out_counts,
                     size_t out_capacity, void *d_workspace, size_t workspace_bytes, size_t layout_b)
{
    if (!d_count || !d_out_counts || !d_workspace) throw Error(CLSIMHIP_ERR_ARGUMENT, "device pointers are (null)");
    if ((capacity && !d_records) || (out_capacity && !d_out)) throw Error(CLSIMHIP_ERR_ARGUMENT, "d_records / d_out is (null)");
    capacity_check(std::max(capacity, out_capacity));
    if (misaligned(15u, d_records, d_out, d_workspace) || misaligned(3u, d_count, d_out_counts))
        throw Error(CLSIMHIP_ERR_ARGUMENT, "records and d_workspace must be aligned to 16 bytes, the counts to 4");
    if (overlap(d_records, capacity * kRecordBytes, d_out, out_capacity * kRecordBytes)) throw Error(CLSIMHIP_ERR_ARGUMENT, kStore + ": the output must not overlap an input");
    const StoreWorkspace W(capacity, layout_b);
    workspace_check(workspace_bytes, W.bytes);
    uint8_t *ws = static_cast<uint8_t *>(d_workspace);
    CanonArgs A{};
    A.records = static_cast<const uint4 *>(d_records);
    A.count = static_cast<const uint32_t *>(d_count);
    A.capacity = static_cast<uint32_t>(capacity);
    A.map = d_map;
    A.n_map = static_cast<uint32_t>(n_map);
    A.header = reinterpret_cast<uint32_t *>(ws);
    A.tile_counts = reinterpret_cast<uint32_t *>(ws + W.tile_counts);
    A.keys = reinterpret_cast<uint64_t *>(ws + W.keys);
    A.index = reinterpret_cast<uint32_t *>(ws + W.index);
    A.run_first = reinterpret_cast<uint32_t *>(ws + W.run_first);
    A.out = static_cast<uint4 *>(d_out);
    A.out_capacity = static_cast<uint32_t>(out_capacity);
    A.out_counts = static_cast<uint32_t *>(d_out_counts);
    return A;
}

CombineArgs combine_args(const void *d_a, const void *d_a_count, size_t capacity_a, const void *d_b, const void *d_b_count, size_t capacity_b, void *d_out,
                         void *d_out_counts, size_t out_capacity, void *d_workspace, size_t workspace_bytes)
{
    if (!d_a_count || !d_b_count || !d_out_counts || !d_workspace) throw Error(CLSIMHIP_ERR_ARGUMENT, "device pointers are (null)");
    if ((capacity_a && !d_a) || (capacity_b && !d_b) || (out_capacity && !d_out)) throw Error(CLSIMHIP_ERR_ARGUMENT, "d_a / d_b / d_out is (null)");
    capacity_check(std::max({capacity_a, capacity_b, out_capacity}));
    if (misaligned(15u, d_a, d_b, d_out, d_workspace) || misaligned(3u, d_a_count, d_b_count, d_out_counts))
        throw Error(CLSIMHIP_ERR_ARGUMENT, "records and d_workspace must be aligned to 16 bytes, the counts to 4");
    if (overlap(d_a, capacity_a * kRecordBytes, d_out, out_capacity * kRecordBytes) || overlap(d_b, capacity_b * kRecordBytes, d_out, out_capacity * kRecordBytes))
        throw Error(CLSIMHIP_ERR_ARGUMENT, kStore + ": the output must not overlap an input");
    const StoreWorkspace W(capacity_a, capacity_b);
    workspace_check(workspace_bytes, W.bytes);
    uint8_t *ws = static_cast<uint8_t *>(d_workspace);
    CombineArgs C{};
    C.a = static_cast<const uint4 *>(d_a);
    C.b = static_cast<const uint4 *>(d_b);
    C.a_count = static_cast<const uint32_t *>(d_a_count);
    C.b_count = static_cast<const uint32_t *>(d_b_count);
    C.capacity_a = static_cast<uint32_t>(capacity_a);
    C.capacity_b = static_cast<uint32_t>(capacity_b);
    C.out_capacity = static_cast<uint32_t>(out_capacity);
    C.header = reinterpret_cast<uint32_t *>(ws);
    C.tile_counts = reinterpret_cast<uint32_t *>(ws + W.tile_counts);
    C.partition = reinterpret_cast<uint32_t *>(ws + W.partition);
    C.out = static_cast<uint4 *>(d_out);
    C.out_counts = static_cast<uint32_t *>(d_out_counts);
    return C;
}

SplitArgs split_args(const void *d_records, const void *d_count, size_t capacity, uint32_t last_frame, void *d_head, void *d_head_counts, size_t head_capacity,
                     void *d_tail, void *d_tail_counts, size_t tail_capacity, bool head_may_be_dropped)
{
    if (!d_count || !d_head_counts || !d_tail_counts) throw Error(CLSIMHIP_ERR_ARGUMENT, "device pointers are (null)");
    if (capacity && (!d_records || !d_tail)) throw Error(CLSIMHIP_ERR_ARGUMENT, "d_records / d_tail is (null)");
    if (!head_may_be_dropped && head_capacity && !d_head) throw Error(CLSIMHIP_ERR_ARGUMENT, "d_head is (null)");
    capacity_check(std::max(capacity, head_capacity));
    if (tail_capacity < capacity)
        throw Error(CLSIMHIP_ERR_ARGUMENT, kStore + ": the tail's capacity must not be below the input's (a bound that drains nothing leaves everything in the tail)");
    if (misaligned(15u, d_records, d_head, d_tail) || misaligned(3u, d_count, d_head_counts, d_tail_counts))
        throw Error(CLSIMHIP_ERR_ARGUMENT, "records must be aligned to 16 bytes, the counts to 4");
    if (overlap(d_records, capacity * kRecordBytes, d_head, head_capacity * kRecordBytes) || overlap(d_records, capacity * kRecordBytes, d_tail, tail_capacity * kRecordBytes))
        throw Error(CLSIMHIP_ERR_ARGUMENT, kStore + ": the output must not overlap an input");
    SplitArgs S{};
    S.records = static_cast<const uint4 *>(d_records);
    S.count = static_cast<const uint32_t *>(d_count);
    S.capacity = static_cast<uint32_t>(capacity);
    S.last_frame = last_frame;
    S.head = static_cast<uint4 *>(d_head);
    S.head_counts = static_cast<uint32_t *>(d_head_counts);
    S.head_capacity = static_cast<uint32_t>(head_capacity);
    S.tail = static_cast<uint4 *>(d_tail);
    S.tail_counts = static_cast<uint32_t *>(d_tail_counts);
    return S;
}

// Page-locked staging of the stand-alone CANON's map (series_bunch.h), one buffer per device, for the life of the process
std::mutex g_call_mutex, g_map_mutex;
SeriesStaging &staging()
{
    static SeriesStaging *s = new SeriesStaging(&g_map_mutex);
    return *s;
}

// ---- the device store ----
// Two record buffers: an add or a drain reads the current one and writes the other.  event_ marks the last work issued on the store's
// buffers, on whichever stream; every call makes its stream wait for it before it touches them.
class DeviceEventStatsStore final : public EventStatsStore {
public:
    using Record = clsimhip_event_statistics;

    DeviceEventStatsStore(int device, size_t capacity) : device_(device), capacity_(capacity)
    {
        need_device(device, "a device " + kStore);
        DeviceGuard on_device(device);
        for (int k = 0; k < 2; ++k) records_[k].alloc(capacity, named("records").c_str());
        canon_.alloc(capacity, named("bunch form").c_str());
        counts_.alloc(kSlots * 8u, named("counts").c_str());
        workspace_bytes_ = StoreWorkspace(capacity, capacity).bytes;
        workspace_.alloc(workspace_bytes_, named("workspace").c_str());
        sticky_.alloc(8u, named("counters").c_str());                   // page-locked: the device writes them, the host reads them without a copy
        std::memset(sticky_.get(), 0, 8u * sizeof(uint32_t));
        void *d = nullptr;
        hip_check(hipHostGetDevicePointer(&d, sticky_.get(), 0), "hipHostGetDevicePointer");
        d_sticky_ = static_cast<uint32_t *>(d);
        plan_.alloc(16u, named("plan").c_str());
        stream_.create(named("stream").c_str());
        event_.create_untimed(named("event").c_str());
        uploaded_.create_untimed(named("event").c_str());
        map_uploaded_.create_untimed(named("event").c_str());
        hip_check(hipMemsetAsync(counts_.get(), 0, kSlots * 8u * sizeof(uint32_t), stream_.get()), "hipMemsetAsync");
        hip_check(hipEventRecord(event_.get(), stream_.get()), "hipEventRecord");
        hip_check(hipEventRecord(uploaded_.get(), stream_.get()), "hipEventRecord");
        hip_check(hipEventRecord(map_uploaded_.get(), stream_.get()), "hipEventRecord");
    }
    ~DeviceEventStatsStore() override
    {
        DeviceGuard on_device(device_, std::nothrow);
        (void)hipEventSynchronize(event_.get());                        // nothing of the store's is in flight when its memory goes
    }
    bool on_device() const override { return true; }

    void add_host(const Record *records, size_t n, const clsimhip_relabel *map, size_t n_map) override
    {
        if (n && !records) throw Error(CLSIMHIP_ERR_ARGUMENT, "records is (null)");
        relabel_map_check(map, n_map);
        if (n > capacity_) throw Error(CLSIMHIP_ERR_ARGUMENT, kStore + ": a bunch of " + std::to_string(n) + " records does not fit a store of " + std::to_string(capacity_));
        std::lock_guard<std::mutex> lk(mutex_);
        DeviceGuard on_device(device_);
        if (!bunch_) {
            bunch_.alloc(capacity_, named("bunch").c_str());
            staged_.alloc(std::max<size_t>(capacity_, 1u), named("staging").c_str());
            staged_count_.alloc(8u, named("staging").c_str());
        }
        hip_check(hipEventSynchronize(uploaded_.get()), "hipEventSynchronize");         // the previous bunch has left the staging buffers
        if (n) std::memcpy(staged_.get(), records, n * sizeof(Record));
        staged_count_.get()[0] = static_cast<uint32_t>(n);
        hipStream_t s = stream_.get();
        hip_check(hipStreamWaitEvent(s, event_.get(), 0), "hipStreamWaitEvent");        // (the previous add has read the bunch buffer)
        if (n) hip_check(hipMemcpyAsync(bunch_.get(), staged_.get(), n * sizeof(Record), hipMemcpyHostToDevice, s), "upload event statistics bunch");
        hip_check(hipMemcpyAsync(counts_of(kBunch), staged_count_.get(), sizeof(uint32_t), hipMemcpyHostToDevice, s), "upload event statistics bunch");
        hip_check(hipEventRecord(uploaded_.get(), s), "hipEventRecord");
        fold(bunch_.get(), counts_of(kBunch), capacity_, map, n_map, s);
    }

    void add_device(const void *d_records, const void *d_count, size_t capacity, const clsimhip_relabel *map, size_t n_map, hipStream_t stream) override
    {
        relabel_map_check(map, n_map);
        if (capacity > capacity_)
            throw Error(CLSIMHIP_ERR_ARGUMENT, kStore + ": a bunch buffer of " + std::to_string(capacity) + " records is beyond the store's capacity of " + std::to_string(capacity_));
        std::lock_guard<std::mutex> lk(mutex_);
        DeviceGuard on_device(device_);
        hip_check(hipStreamWaitEvent(stream, event_.get(), 0), "hipStreamWaitEvent");
        fold(d_records, d_count, capacity, map, n_map, stream);
    }

    void drain_device(uint32_t last_frame, const clsimhip_relabel *map, size_t n_map, void *d_out, void *d_counts, size_t capacity, hipStream_t stream) override
    {
        relabel_map_check(map, n_map);
        std::lock_guard<std::mutex> lk(mutex_);
        refuse_when_sticky();
        DeviceGuard on_device(device_);
        hip_check(hipStreamWaitEvent(stream, event_.get(), 0), "hipStreamWaitEvent");
        drain_into(last_frame, map, n_map, d_out, d_counts, capacity, stream);
    }

    void drain_host(uint32_t last_frame, const clsimhip_relabel *map, size_t n_map, Record *out, size_t capacity, size_t *n) override
    {
        relabel_map_check(map, n_map);
        std::lock_guard<std::mutex> lk(mutex_);
        DeviceGuard on_device(device_);
        const size_t head = plan(last_frame);
        if (head > capacity)
            throw Error(CLSIMHIP_ERR_ARGUMENT, kStore + ": the frames up to " + std::to_string(last_frame) + " hold " + std::to_string(head) + " records, the output " +
                                                   std::to_string(capacity));
        if (head && !out) throw Error(CLSIMHIP_ERR_ARGUMENT, "out is (null)");
        if (!drained_) drained_.alloc(capacity_, named("drained frames").c_str());
        hipStream_t s = stream_.get();
        drain_into(last_frame, map, n_map, drained_.get(), counts_of(kDrained), capacity_, s);
        hip_check(hipMemcpyAsync(plan_.get(), counts_of(kDrained), 5u * sizeof(uint32_t), hipMemcpyDeviceToHost, s), ("download " + kStore + " counts").c_str());
        hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        const size_t made = std::min<size_t>(plan_.get()[0], head);
        if (made) hip_check(hipMemcpyAsync(out, drained_.get(), made * sizeof(Record), hipMemcpyDeviceToHost, s), ("download " + kStore + " frames").c_str());
        hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        if (n) *n = made;
    }

    void size(uint32_t last_frame, size_t *n) override
    {
        std::lock_guard<std::mutex> lk(mutex_);
        DeviceGuard on_device(device_);
        const size_t head = plan(last_frame);
        if (n) *n = head;
    }

private:
    // count words, eight per slot: the two record buffers, an uploaded bunch, its canonical form, a plan, a drained head before and behind
    // the map, and what a plan would leave
    enum Slot : int { kBunch = 2, kCanon = 3, kPlan = 4, kHead = 5, kDrained = 6, kScratch = 7, kSlots = 8 };
    uint32_t *counts_of(int which) const { return counts_.get() + 8 * which; }

    // what an allocation, a stream or an event of the store is called when HIP refuses it
    std::string named(const char *what) const { return kStore + " " + what; }

    void refuse_when_sticky() const
    {
        const volatile uint32_t *c = sticky_.get();
        const uint32_t v[5] = {c[0], c[1], c[2], c[3], c[4]};
        if ((v[0] | v[1] | v[2] | v[3] | v[4]) == 0u) return;
        throw Error(CLSIMHIP_ERR_DEVICE, kStore + ": data was dropped on the device and nothing is delivered -- " + std::to_string(v[FS_MALFORMED_BUNCHES]) +
                                             " malformed bunches (" + std::to_string(v[FS_MALFORMED_ELEMENTS]) + " malformed elements), " +
                                             std::to_string(v[FS_OVERFLOWED_BUNCHES]) + " bunches that did not fit (" + std::to_string(v[FS_OVERFLOWED_RECORDS]) + " records), " +
                                             std::to_string(v[FS_MALFORMED_STORE]) + " malformed elements in the store itself");
    }

    // the map in device memory behind everything issued on `stream` so far (the caller has made the stream wait for the store's event)
    const clsimhip_relabel *upload_map(const clsimhip_relabel *map, size_t n_map, hipStream_t stream)
    {
        if (n_map == 0) return nullptr;
        if (n_map > map_capacity_) {
            hip_check(hipEventSynchronize(event_.get()), "hipEventSynchronize");        // nothing reads the old one any more
            hip_check(hipEventSynchronize(map_uploaded_.get()), "hipEventSynchronize");
            d_map_.alloc(n_map, named("map").c_str());
            staged_map_.alloc(n_map, named("map staging").c_str());
            map_capacity_ = n_map;
        }
        hip_check(hipEventSynchronize(map_uploaded_.get()), "hipEventSynchronize");     // the previous map has left the staging buffer
        std::memcpy(staged_map_.get(), map, n_map * sizeof(clsimhip_relabel));
        hip_check(hipMemcpyAsync(d_map_.get(), staged_map_.get(), n_map * sizeof(clsimhip_relabel), hipMemcpyHostToDevice, stream), "upload event statistics map");
        hip_check(hipEventRecord(map_uploaded_.get(), stream), "hipEventRecord");
        return d_map_.get();
    }

    // COMBINE(store, CANON(bunch, map)) into the other buffer, behind the store's event on `stream`
    void fold(const void *d_records, const void *d_count, size_t capacity, const clsimhip_relabel *map, size_t n_map, hipStream_t stream)
    {
        const int other = current_ ^ 1;
        const clsimhip_relabel *d_map = upload_map(map, n_map, stream);
        const CanonArgs A = canon_args(d_records, d_count, capacity, d_map, n_map, canon_.get(), counts_of(kCanon), capacity_, workspace_.get(), workspace_bytes_, 0);
        const CombineArgs C = combine_args(records_[current_].get(), counts_of(current_), capacity_, canon_.get(), counts_of(kCanon), capacity_, records_[other].get(),
                                           counts_of(other), capacity_, workspace_.get(), workspace_bytes_);
        launched(launch_canon(A, stream), kStore + " canonical form");
        launched(launch_combine(C, stream), kStore + " combination");
        hipLaunchKernelGGL(store_note_kernel<EventStatsTag>, dim3(1), dim3(64), 0, stream, static_cast<const uint32_t *>(counts_of(other)),
                           static_cast<const uint32_t *>(d_count), static_cast<uint32_t>(capacity), d_sticky_);
        launched(hipGetLastError(), kStore + " combination");
        current_ = other;
        hip_check(hipEventRecord(event_.get(), stream), "hipEventRecord");
    }

    // CANON(head of SPLIT, map) into the caller's buffer, the tail into the other buffer, behind the store's event on `stream`.  Without
    // a map the head is canonical as it stands and goes straight out.
    void drain_into(uint32_t last_frame, const clsimhip_relabel *map, size_t n_map, void *d_out, void *d_counts, size_t capacity, hipStream_t stream)
    {
        const int other = current_ ^ 1;
        if (n_map == 0) {
            SplitArgs S = split_args(records_[current_].get(), counts_of(current_), capacity_, last_frame, d_out, d_counts, capacity, records_[other].get(), counts_of(other),
                                     capacity_, false);
            S.blocked = d_sticky_;
            launched(launch_split(S, stream), kStore + " drain");
        } else {
            if (!d_counts) throw Error(CLSIMHIP_ERR_ARGUMENT, "device pointers are (null)");
            if (!head_) head_.alloc(capacity_, named("head").c_str());
            const clsimhip_relabel *d_map = upload_map(map, n_map, stream);
            SplitArgs S = split_args(records_[current_].get(), counts_of(current_), capacity_, last_frame, head_.get(), counts_of(kHead), std::min(capacity, capacity_),
                                     records_[other].get(), counts_of(other), capacity_, false);
            S.blocked = d_sticky_;
            CanonArgs A = canon_args(head_.get(), counts_of(kHead), capacity_, d_map, n_map, d_out, d_counts, capacity, workspace_.get(), workspace_bytes_, 0);
            A.head_counts = counts_of(kHead);
            launched(launch_split(S, stream), kStore + " drain");
            launched(launch_canon(A, stream), kStore + " drain");
        }
        current_ = other;
        hip_check(hipEventRecord(event_.get(), stream), "hipEventRecord");
    }

    // waits for everything issued, refuses when data was dropped, and reads what a drain up to last_frame would take
    size_t plan(uint32_t last_frame)
    {
        hipStream_t s = stream_.get();
        hip_check(hipStreamWaitEvent(s, event_.get(), 0), "hipStreamWaitEvent");
        hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        refuse_when_sticky();
        const SplitArgs S = split_args(records_[current_].get(), counts_of(current_), capacity_, last_frame, nullptr, counts_of(kPlan), capacity_, records_[current_ ^ 1].get(),
                                       counts_of(kScratch), capacity_, true);
        hipLaunchKernelGGL(split_plan_kernel, dim3(1), dim3(64), 0, s, S);
        launched(hipGetLastError(), kStore + " plan");
        hip_check(hipMemcpyAsync(plan_.get(), counts_of(kPlan), 5u * sizeof(uint32_t), hipMemcpyDeviceToHost, s), ("download " + kStore + " plan").c_str());
        hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        return plan_.get()[0];
    }

    int device_;
    size_t capacity_, workspace_bytes_ = 0, map_capacity_ = 0;
    std::mutex mutex_;
    DeviceBuffer<Record> records_[2], canon_, bunch_, head_, drained_;
    DeviceBuffer<uint32_t> counts_;
    DeviceBuffer<uint8_t> workspace_;
    DeviceBuffer<clsimhip_relabel> d_map_;
    PinnedBuffer<uint32_t> sticky_, plan_, staged_count_;
    PinnedBuffer<Record> staged_;
    PinnedBuffer<clsimhip_relabel> staged_map_;
    uint32_t *d_sticky_ = nullptr;
    Stream stream_;
    Event event_, uploaded_, map_uploaded_;
    int current_ = 0;
};

} // namespace

size_t event_stats_store_workspace_bytes(size_t capacity_a, size_t capacity_b) { return StoreWorkspace(capacity_a, capacity_b).bytes; }

void event_stats_canonical_device(int device, const void *d_records, const void *d_count, size_t capacity, const clsimhip_relabel *map, size_t n_map, void *d_out,
                                  void *d_out_counts, size_t out_capacity, void *d_workspace, size_t workspace_bytes, hipStream_t stream)
{
    need_device(device, "the " + kStore + "'s canonical form on the device");
    relabel_map_check(map, n_map);
    const StoreWorkspace W(capacity, n_map);
    const clsimhip_relabel *d_map = d_workspace ? reinterpret_cast<const clsimhip_relabel *>(static_cast<uint8_t *>(d_workspace) + W.map) : nullptr;
    const CanonArgs A = canon_args(d_records, d_count, capacity, d_map, n_map, d_out, d_out_counts, out_capacity, d_workspace, workspace_bytes, n_map);
    DeviceGuard on_device(device);
    std::lock_guard<std::mutex> one_call(g_call_mutex);
    if (n_map) {                                                        // copied before the call returns; the upload is asynchronous
        uint8_t *pinned = staging().acquire(device, n_map * sizeof(clsimhip_relabel), "event statistics store");
        std::memcpy(pinned, map, n_map * sizeof(clsimhip_relabel));
        hip_check(hipMemcpyAsync(static_cast<uint8_t *>(d_workspace) + W.map, pinned, n_map * sizeof(clsimhip_relabel), hipMemcpyHostToDevice, stream),
                  "hipMemcpyAsync (event statistics map)");
        hip_check(hipEventRecord(staging().done(device), stream), "hipEventRecord (event statistics map)");
    }
    launched(launch_canon(A, stream), kStore + " canonical form");
}

void event_stats_combine_device(int device, const void *d_a, const void *d_a_count, size_t capacity_a, const void *d_b, const void *d_b_count, size_t capacity_b,
                                void *d_out, void *d_out_counts, size_t out_capacity, void *d_workspace, size_t workspace_bytes, hipStream_t stream)
{
    need_device(device, "the " + kStore + "'s combination on the device");
    const CombineArgs C = combine_args(d_a, d_a_count, capacity_a, d_b, d_b_count, capacity_b, d_out, d_out_counts, out_capacity, d_workspace, workspace_bytes);
    DeviceGuard on_device(device);
    launched(launch_combine(C, stream), kStore + " combination");
}

void event_stats_split_device(int device, const void *d_records, const void *d_count, size_t capacity, uint32_t last_frame, void *d_head, void *d_head_counts,
                              size_t head_capacity, void *d_tail, void *d_tail_counts, size_t tail_capacity, hipStream_t stream)
{
    need_device(device, "the " + kStore + "'s split on the device");
    const SplitArgs S = split_args(d_records, d_count, capacity, last_frame, d_head, d_head_counts, head_capacity, d_tail, d_tail_counts, tail_capacity, false);
    DeviceGuard on_device(device);
    launched(launch_split(S, stream), kStore + " split");
}

std::unique_ptr<EventStatsStore> make_device_event_stats_store(int device, size_t capacity)
{
    capacity_check(capacity);
    return std::unique_ptr<EventStatsStore>(new DeviceEventStatsStore(device, capacity));
}

} // namespace clsimhip
