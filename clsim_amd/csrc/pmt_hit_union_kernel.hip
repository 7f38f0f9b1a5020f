// PMT hit frame store on the device: the definition of pmt_hit_union.h as a merge of two sorted runs, for gfx950 (wave64), the split,
// their host side (workspace, argument checks, launches) and the device store.  The stage has the MCPE union's shape
// (mcpe_union_kernel.hip); what differs is the record and the table entry (24 bytes each, 8-byte aligned) and the key (6 words).
//
//   ph_union_check_kernel      one lane per entry and per record of both inputs: the local checks of a series form of PMT hits (a
//                              record finds its entry by bisection over `first`), MALFORMED elements counted per input, and per record
//                              its entry's frame.
//   ph_union_plan_kernel       one workgroup: the effective sizes -- A malformed: nothing; B malformed or a union that does not fit: A alone.
//   ph_union_partition_kernel  one lane per output tile boundary: how many records of A lie in front of it, by bisection along the merge
//                              path's diagonal on the key (ties: A first).
//   ph_union_merge_kernel      one workgroup per output tile of 2048 records, whatever the lengths of the series.  LDS holds the WHOLE
//                              key of the tile (six arrays of 2048 words, 48 KiB: three workgroups per compute unit).  A lane loads
//                              its eight records (three 8-byte loads each), keeps their keys in registers and ranks each in the other
//                              run by bisection in LDS: a lane of A counts B's elements strictly less, a lane of B counts A's less or
//                              equal -- a permutation for two series forms, clamped below the tile's fill for anything else.  The keys
//                              are then permuted in LDS, and because a record is a function of its key the output is REBUILT from the
//                              sorted keys, not moved: the tile's output is 3 x fill 8-byte words, and lane q writes word q, q + 256 ...
//                              so that a wave's stores are 512 contiguous bytes (24 is no multiple of 16; a lane that stored its own
//                              record would scatter three 8-byte stores to a permuted place).  A head is a record whose
//                              (frame, DOM code, pmt) differs from its LDS neighbour's, the tile's first record's predecessor being the
//                              larger of A[i-1] and B[j-1].
//   launch_series_tile_scan / ph_union_emit_kernel / ph_union_close_kernel
//                              the series stage's scan over the heads per tile, then the table, as in the MCPE union.
//   ph_split_plan_kernel / ph_split_copy_kernel
//                              the entries with frame <= last_frame by bisection, then a grid-stride copy of 8-byte words; the tail's
//                              `first` rebased.
//   ph_store_note_kernel       the store's bookkeeping behind a union.
//
// Everything reads its sizes from device memory: nothing waits for the host.  Atomics only count.  Every loop is bounded by a
// capacity and every index is clamped to one, whatever bytes the inputs hold.
#include "pmt_hit_union.h"

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "hip_resources.h"

namespace clsimhip {

namespace {

using UArgs = PmtHitUnionDeviceArgs;
using SArgs = PmtHitSplitDeviceArgs;

__device__ __forceinline__ uint32_t lanes_below(uint64_t mask)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__device__ __forceinline__ uint32_t min_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }

// a record's or an entry's six words by three 8-byte loads (records and tables are 8-byte aligned: the callers check the base)
__device__ __forceinline__ void load_words(const void *base, uint64_t i, uint32_t (&w)[6])
{
    const uint64_t *p = static_cast<const uint64_t *>(base) + 3u * i;
    const uint64_t g0 = p[0], g1 = p[1], g2 = p[2];
    w[0] = (uint32_t)g0; w[1] = (uint32_t)(g0 >> 32);
    w[2] = (uint32_t)g1; w[3] = (uint32_t)(g1 >> 32);
    w[4] = (uint32_t)g2; w[5] = (uint32_t)(g2 >> 32);
}

__global__ void __launch_bounds__(256) ph_union_check_kernel(const UArgs U)
{
    const uint32_t n_a = min_u32(U.a_counts[0], U.capacity_a), s_a = min_u32(U.a_counts[1], U.capacity_a);
    const uint32_t n_b = min_u32(U.b_counts[0], U.capacity_b), s_b = min_u32(U.b_counts[1], U.capacity_b);
    if (blockIdx.x == 0u && threadIdx.x == 0u) {
        U.header[UH_IN_A] = n_a; U.header[UH_SERIES_A] = s_a;
        U.header[UH_IN_B] = n_b; U.header[UH_SERIES_B] = s_b;
    }
    const uint64_t start = (uint64_t)blockIdx.x * 256u + threadIdx.x, stride = (uint64_t)gridDim.x * 256u;
    uint32_t bad_a = 0u, bad_b = 0u;
    for (uint64_t s = start; s < s_a; s += stride) bad_a += pmt_hit_union_entry_ok(U.a_series, s_a, n_a, (uint32_t)s) ? 0u : 1u;
    for (uint64_t s = start; s < s_b; s += stride) bad_b += pmt_hit_union_entry_ok(U.b_series, s_b, n_b, (uint32_t)s) ? 0u : 1u;
    for (uint64_t i = start; i < n_a; i += stride) {
        uint32_t frame;
        bad_a += pmt_hit_union_record_ok(U.a_records, U.a_series, s_a, (uint32_t)i, &frame) ? 0u : 1u;
        U.a_frames[i] = frame;                                          // i < n_a <= capacity_a
    }
    for (uint64_t i = start; i < n_b; i += stride) {
        uint32_t frame;
        bad_b += pmt_hit_union_record_ok(U.b_records, U.b_series, s_b, (uint32_t)i, &frame) ? 0u : 1u;
        U.b_frames[i] = frame;
    }
    if (bad_a != 0u) atomicAdd(U.header + UH_MALFORMED_A, bad_a);
    if (bad_b != 0u) atomicAdd(U.header + UH_MALFORMED_B, bad_b);
}

__global__ void __launch_bounds__(64) ph_union_plan_kernel(const UArgs U)
{
    if (threadIdx.x != 0u) return;
    uint32_t n_a = U.header[UH_IN_A], n_b = U.header[UH_IN_B];
    const uint64_t both = (uint64_t)n_a + n_b;
    uint32_t overflow = 0u;
    if (U.header[UH_MALFORMED_A] != 0u) {
        n_a = 0u; n_b = 0u;
    } else if (U.header[UH_MALFORMED_B] != 0u) {
        n_b = 0u;
    } else if (both > U.out_capacity) {
        overflow = both > 0xffffffffull ? 0xffffffffu : (uint32_t)both;
        n_b = 0u;
    }
    if (n_a > U.out_capacity) {                                         // A alone does not fit either: nothing
        if (overflow == 0u) overflow = n_a;
        n_a = 0u;
    }
    U.header[UH_N_A] = n_a;
    U.header[UH_N_B] = n_b;
    U.header[UH_OVERFLOW] = overflow;
    U.header[SH_KEPT] = n_a + n_b;                                      // <= out_capacity
}

__device__ __forceinline__ PmtHitKey key_at(const clsimhip_pmt_hit *records, const uint32_t *frames, uint32_t i)
{
    uint32_t rec[kPmtHitRecordWords];
    load_words(records, i, rec);
    return pmt_hit_union_make_key(frames[i], rec);
}

__global__ void __launch_bounds__(256) ph_union_partition_kernel(const UArgs U)
{
    const uint32_t n_a = U.header[UH_N_A], n_b = U.header[UH_N_B];
    const uint32_t n = n_a + n_b;
    const uint32_t tiles = (uint32_t)(((uint64_t)n + kSeriesTile - 1u) / kSeriesTile);
    for (uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x; t <= tiles; t += (uint64_t)gridDim.x * 256u) {
        const uint64_t reach = t * kSeriesTile;
        const uint32_t diagonal = reach < n ? (uint32_t)reach : n;
        // the records of A among the first `diagonal` of the output: the first i with B[diagonal - i - 1] < A[i]
        uint32_t lo = diagonal > n_b ? diagonal - n_b : 0u, hi = diagonal < n_a ? diagonal : n_a;
        while (lo < hi) {                                               // at most 32 trips; mid < n_a, 0 <= diagonal - mid - 1 < n_b
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (pmt_hit_union_key_less(key_at(U.b_records, U.b_frames, diagonal - mid - 1u), key_at(U.a_records, U.a_frames, mid))) hi = mid; else lo = mid + 1u;
        }
        U.partition[t] = lo;                                            // t <= tiles(capacity_a + capacity_b)
    }
}

constexpr uint32_t kRounds = kSeriesTile / 256u;                        // 8 elements per lane

// how many of the tile's elements [from, to), an ascending run, go in front of `key`: those less than it, and with kAfterEqual those
// equal to it too
template <bool kAfterEqual>
__device__ __forceinline__ uint32_t rank_in(uint32_t (*keys)[kSeriesTile], uint32_t from, uint32_t to, const uint32_t (&key)[kPmtHitKeyWords])
{
    uint32_t lo = from, hi = to;
    while (lo < hi) {                                                   // at most 11 trips: to - from <= 2048
        const uint32_t mid = lo + (hi - lo) / 2u;
        bool less = false, greater = false, decided = false;            // keys[mid] < key, keys[mid] > key
#pragma unroll
        for (uint32_t k = 0; k < kPmtHitKeyWords; ++k) {
            const uint32_t w = keys[k][mid];
            if (!decided && w != key[k]) { decided = true; less = w < key[k]; greater = !less; }
        }
        const bool before = kAfterEqual ? !greater : less;              // the element at mid goes in front of `key`
        if (before) lo = mid + 1u; else hi = mid;
    }
    return lo - from;
}

__global__ void __launch_bounds__(256) ph_union_merge_kernel(const UArgs U)
{
    const uint32_t n_a = U.header[UH_N_A], n_b = U.header[UH_N_B];
    const uint32_t n = n_a + n_b;
    const uint64_t start = (uint64_t)blockIdx.x * kSeriesTile;
    if (start >= n) return;
    __shared__ uint32_t keys[kPmtHitKeyWords][kSeriesTile];             // 48 KiB, structure of arrays
    __shared__ uint32_t heads;
    const uint32_t total = n - start < kSeriesTile ? (uint32_t)(n - start) : kSeriesTile;
    // the tile's share of both runs; the clamps bite for no pair of series forms
    uint32_t i0 = min_u32(U.partition[blockIdx.x], n_a), i1 = min_u32(U.partition[blockIdx.x + 1u], n_a);
    if (i0 > start) i0 = (uint32_t)start;
    const uint32_t j0 = min_u32((uint32_t)start - i0, n_b);
    uint32_t in_a = i1 > i0 ? min_u32(i1 - i0, total) : 0u;
    if (total - in_a > n_b - j0) in_a = total - (n_b - j0);             // (then in_a <= n_a - i0 unless the partition is none: clamped next)
    if (in_a > n_a - i0) in_a = n_a - i0;
    const uint32_t in_b = min_u32(total - in_a, n_b - j0);
    const uint32_t filled = in_a + in_b;                                // = total for two series forms; never above it
    if (threadIdx.x == 0u) heads = 0u;
    // tile position e is A[i0 + e] for e < in_a and B[j0 + e - in_a] behind
    uint32_t key[kRounds][kPmtHitKeyWords];
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t e = r * 256u + threadIdx.x;
        if (e < filled) {
            const bool from_a = e < in_a;
            const uint32_t at = from_a ? i0 + e : j0 + (e - in_a);     // < n_a, < n_b
            const PmtHitKey k = key_at(from_a ? U.a_records : U.b_records, from_a ? U.a_frames : U.b_frames, at);
#pragma unroll
            for (uint32_t w = 0; w < kPmtHitKeyWords; ++w) { key[r][w] = k.w[w]; keys[w][e] = k.w[w]; }
        }
    }
    __syncthreads();
    uint32_t rank[kRounds];
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t e = r * 256u + threadIdx.x;
        rank[r] = 0u;
        if (e < in_a) rank[r] = e + rank_in<false>(keys, in_a, filled, key[r]);                     // the records of B in front: strictly less
        else if (e < filled) rank[r] = (e - in_a) + rank_in<true>(keys, 0u, in_a, key[r]);          // the records of A in front: less or equal
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t e = r * 256u + threadIdx.x;
        if (e < filled) {
            const uint32_t p = min_u32(rank[r], filled - 1u);           // (a permutation of [0, filled) for sorted runs)
#pragma unroll
            for (uint32_t w = 0; w < kPmtHitKeyWords; ++w) keys[w][p] = key[r][w];
        }
    }
    __syncthreads();
    // the predecessor of the tile's first record: the larger of A[i0 - 1] and B[j0 - 1] in (frame, DOM code, pmt)
    uint32_t before[kPmtHitChannelWords] = {0u, 0u, 0u};
    bool have_before = false;
    if (i0 > 0u) {
        const PmtHitKey k = key_at(U.a_records, U.a_frames, i0 - 1u);
        before[0] = k.w[0]; before[1] = k.w[1]; before[2] = k.w[2];
        have_before = true;
    }
    if (j0 > 0u) {
        const PmtHitKey k = key_at(U.b_records, U.b_frames, j0 - 1u);
        if (!have_before || union_words_less(before, k.w, kPmtHitChannelWords)) { before[0] = k.w[0]; before[1] = k.w[1]; before[2] = k.w[2]; }
        have_before = true;
    }
    uint32_t mine = 0u;
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t e = r * 256u + threadIdx.x;                      // an output position now
        if (e < filled) {
            const uint32_t frame = keys[0][e], dom = keys[1][e], pmt = keys[2][e];
            U.out_frames[start + e] = frame;                            // start + e < n <= out_capacity
            bool head;
            if (e > 0u) head = keys[0][e - 1u] != frame || keys[1][e - 1u] != dom || keys[2][e - 1u] != pmt;
            else head = !have_before || before[0] != frame || before[1] != dom || before[2] != pmt;
            mine += head ? 1u : 0u;
        }
    }
    // the records, rebuilt from the sorted keys: word q of the tile's 3 x filled 8-byte words is part q % 3 of record q / 3
    uint64_t *const out = reinterpret_cast<uint64_t *>(U.out_records) + 3u * start;
    const uint32_t out_words = 3u * filled;
#pragma unroll
    for (uint32_t r = 0; r < 3u * kRounds; ++r) {
        const uint32_t q = r * 256u + threadIdx.x;
        if (q < out_words) {
            const uint32_t e = q / 3u, part = q - 3u * e;               // e < filled
            // the two LDS words the part is made of: (identifier, DOM code), (pmt, -), (tkey high, tkey low)
            const uint32_t x = part == 0u ? keys[5][e] : part == 1u ? keys[2][e] : keys[3][e];
            const uint32_t y = part == 0u ? keys[1][e] : part == 1u ? 0u : keys[4][e];
            uint32_t k[kPmtHitKeyWords] = {0u, 0u, 0u, 0u, 0u, 0u}, rec[kPmtHitRecordWords];
            if (part == 2u) { k[3] = x; k[4] = y; } else { k[5] = x; k[1] = y; k[2] = x; }
            pmt_hit_union_record_of(k, rec);                            // the one definition of key -> record; each part uses its two words
            const uint32_t low = part == 0u ? rec[0] : part == 1u ? rec[2] : rec[4], high = part == 0u ? rec[1] : part == 1u ? rec[3] : rec[5];
            out[q] = (uint64_t)low | ((uint64_t)high << 32);            // 3 * (start + e) + part < 3 * out_capacity
        }
    }
    if (mine != 0u) atomicAdd(&heads, mine);
    __syncthreads();
    if (threadIdx.x == 0u) U.tile_counts[blockIdx.x] = heads;
}

__global__ void __launch_bounds__(256) ph_union_emit_kernel(const UArgs U)
{
    const uint32_t n = U.header[SH_KEPT];
    const uint64_t start = (uint64_t)blockIdx.x * kSeriesTile;
    if (start >= n) return;
    __shared__ uint32_t wave_heads[4];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t frame[kRounds], dom[kRounds], pmt[kRounds];
    uint64_t heads[kRounds];
    uint32_t total = 0u;
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint64_t i = start + wave * 512u + r * 64u + lane;
        bool head = false;
        if (i < n) {
            const uint32_t *rec = pmt_hit_union_words(U.out_records, i);
            frame[r] = U.out_frames[i];
            dom[r] = rec[1];
            pmt[r] = rec[2];
            if (i == 0u) head = true;
            else {
                const uint32_t *prev = pmt_hit_union_words(U.out_records, i - 1u);
                head = frame[r] != U.out_frames[i - 1u] || dom[r] != prev[1] || pmt[r] != prev[2];
            }
        }
        heads[r] = __ballot(head);
        total += (uint32_t)__popcll(heads[r]);
    }
    if (lane == 0u) wave_heads[wave] = total;
    __syncthreads();
    uint32_t index = U.tile_counts[blockIdx.x];         // scanned: the series the tile's first head starts
    for (uint32_t w = 0; w < wave; ++w) index += wave_heads[w];
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint64_t i = start + wave * 512u + r * 64u + lane;
        if (i < n && ((heads[r] >> lane) & 1u)) {
            const uint32_t s = index + lanes_below(heads[r]);           // < series <= n <= out_capacity
            if (s < U.out_capacity) {
                uint64_t *entry = reinterpret_cast<uint64_t *>(U.out_series + s);
                entry[0] = (uint64_t)frame[r] | ((uint64_t)dom[r] << 32);
                entry[1] = (uint64_t)pmt[r] | ((uint64_t)(uint32_t)i << 32);        // pmt, first
                entry[2] = 0u;                                                      // count: ph_union_close_kernel; reserved = 0
            }
        }
        index += (uint32_t)__popcll(heads[r]);
    }
}

__global__ void __launch_bounds__(256) ph_union_close_kernel(const UArgs U)
{
    const uint32_t n = U.header[SH_KEPT], n_series = min_u32(U.header[SH_SERIES], U.out_capacity);
    for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < n_series; s += (uint64_t)gridDim.x * 256u) {
        const uint32_t next = s + 1u < n_series ? U.out_series[s + 1u].first : n;
        U.out_series[s].count = next - U.out_series[s].first;
    }
    if (blockIdx.x == 0u && threadIdx.x < 5u) U.out_counts[threadIdx.x] = threadIdx.x == 1u ? n_series : U.header[threadIdx.x];
}

__global__ void __launch_bounds__(64) ph_split_plan_kernel(const SArgs S)
{
    if (threadIdx.x != 0u) return;
    const uint32_t n = min_u32(S.counts[0], S.capacity), n_series = min_u32(S.counts[1], S.capacity);
    uint32_t entries = pmt_hit_union_split_entries(S.series, n_series, S.last_frame);
    uint32_t head = entries < n_series ? min_u32(S.series[entries].first, n) : n;
    if (entries == 0u) head = 0u;
    uint32_t overflow = 0u;
    if (head > S.head_capacity || entries > S.head_capacity) {          // a head that does not fit drains nothing
        overflow = head > entries ? head : entries;
        head = 0u; entries = 0u;
    }
    if (S.blocked) {
        uint32_t any = 0u;
        for (uint32_t k = 0; k < 5u; ++k) any |= S.blocked[k];
        if (any != 0u) { head = 0u; entries = 0u; }
    }
    S.head_counts[0] = head; S.head_counts[1] = entries; S.head_counts[2] = 0u; S.head_counts[3] = 0u; S.head_counts[4] = overflow;
    S.tail_counts[0] = n - head; S.tail_counts[1] = n_series - entries; S.tail_counts[2] = 0u; S.tail_counts[3] = 0u; S.tail_counts[4] = 0u;
}

__global__ void __launch_bounds__(256) ph_split_copy_kernel(const SArgs S)
{
    const uint32_t head = S.head_counts[0], entries = S.head_counts[1];             // <= head_capacity
    const uint32_t n = min_u32(S.counts[0], S.capacity), n_series = min_u32(S.counts[1], S.capacity);
    const uint64_t start = (uint64_t)blockIdx.x * 256u + threadIdx.x, stride = (uint64_t)gridDim.x * 256u;
    // the records as 8-byte words: word q belongs to record q / 3, and both outputs keep a record's words together
    const uint64_t *in = reinterpret_cast<const uint64_t *>(S.records);
    uint64_t *head_out = reinterpret_cast<uint64_t *>(S.head_records), *tail_out = reinterpret_cast<uint64_t *>(S.tail_records);
    const uint64_t words = 3ull * n, head_words = 3ull * head;
    for (uint64_t q = start; q < words; q += stride) {
        const uint64_t w = in[q];
        if (q < head_words) {
            if (head_out) head_out[q] = w;                                          // < 3 * head_capacity
        } else
            tail_out[q - head_words] = w;                                           // < 3 * (n - head) <= 3 * capacity <= the tail's
    }
    for (uint64_t s = start; s < n_series; s += stride) {
        const uint64_t *entry = reinterpret_cast<const uint64_t *>(S.series + s);
        const uint64_t e0 = entry[0], e1 = entry[1], e2 = entry[2];
        if (s < entries) {
            if (S.head_series) {
                uint64_t *out = reinterpret_cast<uint64_t *>(S.head_series + s);
                out[0] = e0; out[1] = e1; out[2] = e2;
            }
        } else {
            uint64_t *out = reinterpret_cast<uint64_t *>(S.tail_series + (s - entries));
            out[0] = e0;
            out[1] = (uint64_t)(uint32_t)e1 | ((uint64_t)((uint32_t)(e1 >> 32) - head) << 32);     // first
            out[2] = e2;
        }
    }
}

// the store's bookkeeping behind a union: what the union dropped goes into the sticky counters (one lane; plain stores)
__global__ void __launch_bounds__(64) ph_store_note_kernel(const uint32_t *union_counts, const uint32_t *bunch_counts, uint32_t bunch_capacity, uint32_t *sticky)
{
    if (threadIdx.x != 0u) return;
    if (union_counts[2] != 0u) sticky[FS_MALFORMED_STORE] += union_counts[2];
    else if (union_counts[3] != 0u) { sticky[FS_MALFORMED_BUNCHES] += 1u; sticky[FS_MALFORMED_ELEMENTS] += union_counts[3]; }
    else if (union_counts[4] != 0u) { sticky[FS_OVERFLOWED_BUNCHES] += 1u; sticky[FS_OVERFLOWED_RECORDS] += min_u32(bunch_counts[0], bunch_capacity); }
}

size_t round16(size_t v) { return (v + 15u) & ~size_t{15}; }

uint32_t tiles_of(uint64_t records)
{
    const uint64_t tiles = (records + kSeriesTile - 1u) / kSeriesTile;
    return tiles == 0u ? 1u : (uint32_t)tiles;
}

uint32_t lanes_of(uint64_t records)
{
    const uint64_t lanes = (records + 255u) / 256u;
    return lanes == 0u ? 1u : lanes > 1024u ? 1024u : (uint32_t)lanes;
}

// the workspace: header, heads per output tile, the partition, then one word per record of A, of B and of the output
struct UnionWorkspace {
    size_t tile_counts, partition, a_frames, b_frames, out_frames, bytes;
    UnionWorkspace(size_t capacity_a, size_t capacity_b)
    {
        const size_t tiles = tiles_of(capacity_a + capacity_b);
        tile_counts = kSeriesHeaderWords * sizeof(uint32_t);
        partition = tile_counts + round16(tiles * sizeof(uint32_t));
        a_frames = partition + round16((tiles + 1u) * sizeof(uint32_t));
        b_frames = a_frames + round16(std::max<size_t>(capacity_a, 1u) * sizeof(uint32_t));
        out_frames = b_frames + round16(std::max<size_t>(capacity_b, 1u) * sizeof(uint32_t));
        bytes = out_frames + round16(std::max<size_t>(capacity_a + capacity_b, 1u) * sizeof(uint32_t));
    }
};

hipError_t launch_union(const UArgs &U, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(U.header, 0, kSeriesHeaderWords * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const uint64_t both = (uint64_t)U.capacity_a + U.capacity_b;
    const uint64_t out = both < U.out_capacity ? both : U.out_capacity;
    const uint32_t tiles = tiles_of(out);
    SeriesDeviceArgs S{};                               // what the series stage's tile scan reads
    S.capacity = (uint32_t)out;
    S.header = U.header;
    S.tile_counts = U.tile_counts;
    hipLaunchKernelGGL(ph_union_check_kernel, dim3(lanes_of(std::max<uint64_t>(U.capacity_a, U.capacity_b))), dim3(256), 0, stream, U);
    hipLaunchKernelGGL(ph_union_plan_kernel, dim3(1), dim3(64), 0, stream, U);
    hipLaunchKernelGGL(ph_union_partition_kernel, dim3(lanes_of((uint64_t)tiles + 1u)), dim3(256), 0, stream, U);
    hipLaunchKernelGGL(ph_union_merge_kernel, dim3(tiles), dim3(256), 0, stream, U);
    launch_series_tile_scan(S, stream);
    hipLaunchKernelGGL(ph_union_emit_kernel, dim3(tiles), dim3(256), 0, stream, U);
    hipLaunchKernelGGL(ph_union_close_kernel, dim3(lanes_of(out)), dim3(256), 0, stream, U);
    return hipGetLastError();
}

hipError_t launch_split(const SArgs &S, hipStream_t stream)
{
    hipLaunchKernelGGL(ph_split_plan_kernel, dim3(1), dim3(64), 0, stream, S);
    hipLaunchKernelGGL(ph_split_copy_kernel, dim3(lanes_of(3ull * S.capacity)), dim3(256), 0, stream, S);
    return hipGetLastError();
}

void need_device(int device, const char *what)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) throw Error(CLSIMHIP_ERR_DEVICE, std::string("no HIP device available (") + what + " has no CPU fallback)");
    if (device < 0 || device >= count) throw Error(CLSIMHIP_ERR_ARGUMENT, "device ordinal out of range");
}

uintptr_t at(const void *p) { return reinterpret_cast<uintptr_t>(p); }

UArgs union_args(const void *d_a_records, const void *d_a_series, const void *d_a_counts, size_t capacity_a, const void *d_b_records, const void *d_b_series,
                 const void *d_b_counts, size_t capacity_b, void *d_out_records, void *d_out_series, void *d_out_counts, size_t out_capacity, void *d_workspace,
                 size_t workspace_bytes)
{
    if (!d_a_counts || !d_b_counts || !d_out_counts || !d_workspace) throw Error(CLSIMHIP_ERR_ARGUMENT, "device pointers are (null)");
    if ((capacity_a && (!d_a_records || !d_a_series)) || (capacity_b && (!d_b_records || !d_b_series)) || (out_capacity && (!d_out_records || !d_out_series)))
        throw Error(CLSIMHIP_ERR_ARGUMENT, "d_a_records / d_a_series / d_b_records / d_b_series / d_out_records / d_out_series is (null)");
    if (capacity_a > kFrameStoreMaxCapacity || capacity_b > kFrameStoreMaxCapacity || out_capacity > kFrameStoreMaxCapacity)
        throw Error(CLSIMHIP_ERR_ARGUMENT, "PMT hit frame store: capacity beyond 2^31 records");
    if ((at(d_a_records) & 7u) || (at(d_a_series) & 7u) || (at(d_b_records) & 7u) || (at(d_b_series) & 7u) || (at(d_out_records) & 7u) || (at(d_out_series) & 7u) ||
        (at(d_workspace) & 15u) || (at(d_a_counts) & 3u) || (at(d_b_counts) & 3u) || (at(d_out_counts) & 3u))
        throw Error(CLSIMHIP_ERR_ARGUMENT, "records and series tables must be aligned to 8 bytes, d_workspace to 16, the counts to 4");
    const UnionWorkspace W(capacity_a, capacity_b);
    if (workspace_bytes < W.bytes)
        throw Error(CLSIMHIP_ERR_ARGUMENT, "the PMT hit union workspace holds " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(W.bytes) + " are needed");
    uint8_t *ws = static_cast<uint8_t *>(d_workspace);
    UArgs U{};
    U.a_records = static_cast<const clsimhip_pmt_hit *>(d_a_records);
    U.a_series = static_cast<const clsimhip_pmt_series *>(d_a_series);
    U.a_counts = static_cast<const uint32_t *>(d_a_counts);
    U.b_records = static_cast<const clsimhip_pmt_hit *>(d_b_records);
    U.b_series = static_cast<const clsimhip_pmt_series *>(d_b_series);
    U.b_counts = static_cast<const uint32_t *>(d_b_counts);
    U.capacity_a = static_cast<uint32_t>(capacity_a);
    U.capacity_b = static_cast<uint32_t>(capacity_b);
    U.out_capacity = static_cast<uint32_t>(out_capacity);
    U.header = reinterpret_cast<uint32_t *>(ws);
    U.tile_counts = reinterpret_cast<uint32_t *>(ws + W.tile_counts);
    U.partition = reinterpret_cast<uint32_t *>(ws + W.partition);
    U.a_frames = reinterpret_cast<uint32_t *>(ws + W.a_frames);
    U.b_frames = reinterpret_cast<uint32_t *>(ws + W.b_frames);
    U.out_frames = reinterpret_cast<uint32_t *>(ws + W.out_frames);
    U.out_records = static_cast<clsimhip_pmt_hit *>(d_out_records);
    U.out_series = static_cast<clsimhip_pmt_series *>(d_out_series);
    U.out_counts = static_cast<uint32_t *>(d_out_counts);
    return U;
}

SArgs split_args(const void *d_records, const void *d_series, const void *d_counts, size_t capacity, uint32_t last_frame, void *d_head_records, void *d_head_series,
                 void *d_head_counts, size_t head_capacity, void *d_tail_records, void *d_tail_series, void *d_tail_counts, size_t tail_capacity,
                 bool head_may_be_dropped)
{
    if (!d_counts || !d_head_counts || !d_tail_counts) throw Error(CLSIMHIP_ERR_ARGUMENT, "device pointers are (null)");
    if (capacity && (!d_records || !d_series || !d_tail_records || !d_tail_series)) throw Error(CLSIMHIP_ERR_ARGUMENT, "d_records / d_series / d_tail_records / d_tail_series is (null)");
    if (!head_may_be_dropped && head_capacity && (!d_head_records || !d_head_series)) throw Error(CLSIMHIP_ERR_ARGUMENT, "d_head_records / d_head_series is (null)");
    if (capacity > kFrameStoreMaxCapacity || head_capacity > kFrameStoreMaxCapacity) throw Error(CLSIMHIP_ERR_ARGUMENT, "PMT hit frame store: capacity beyond 2^31 records");
    if (tail_capacity < capacity) throw Error(CLSIMHIP_ERR_ARGUMENT, "PMT hit frame store: the tail's capacity must not be below the input's (a bound that drains nothing leaves everything in the tail)");
    if ((at(d_records) & 7u) || (at(d_series) & 7u) || (at(d_head_records) & 7u) || (at(d_head_series) & 7u) || (at(d_tail_records) & 7u) || (at(d_tail_series) & 7u) ||
        (at(d_counts) & 3u) || (at(d_head_counts) & 3u) || (at(d_tail_counts) & 3u))
        throw Error(CLSIMHIP_ERR_ARGUMENT, "records and series tables must be aligned to 8 bytes, the counts to 4");
    SArgs S{};
    S.records = static_cast<const clsimhip_pmt_hit *>(d_records);
    S.series = static_cast<const clsimhip_pmt_series *>(d_series);
    S.counts = static_cast<const uint32_t *>(d_counts);
    S.capacity = static_cast<uint32_t>(capacity);
    S.last_frame = last_frame;
    S.head_records = static_cast<clsimhip_pmt_hit *>(d_head_records);
    S.head_series = static_cast<clsimhip_pmt_series *>(d_head_series);
    S.head_counts = static_cast<uint32_t *>(d_head_counts);
    S.head_capacity = static_cast<uint32_t>(head_capacity);
    S.tail_records = static_cast<clsimhip_pmt_hit *>(d_tail_records);
    S.tail_series = static_cast<clsimhip_pmt_series *>(d_tail_series);
    S.tail_counts = static_cast<uint32_t *>(d_tail_counts);
    return S;
}

void launched(hipError_t e, const char *what)
{
    if (e != hipSuccess) throw Error(CLSIMHIP_ERR_DEVICE, std::string(what) + " kernel launch: " + hipGetErrorString(e));
}

} // namespace

size_t pmt_hits_union_workspace_bytes(size_t capacity_a, size_t capacity_b) { return UnionWorkspace(capacity_a, capacity_b).bytes; }

void pmt_hits_union_device(int device, const void *d_a_records, const void *d_a_series, const void *d_a_counts, size_t capacity_a, const void *d_b_records,
                           const void *d_b_series, const void *d_b_counts, size_t capacity_b, void *d_out_records, void *d_out_series, void *d_out_counts,
                           size_t out_capacity, void *d_workspace, size_t workspace_bytes, hipStream_t stream)
{
    need_device(device, "the PMT hit union's device path");
    const UArgs U = union_args(d_a_records, d_a_series, d_a_counts, capacity_a, d_b_records, d_b_series, d_b_counts, capacity_b, d_out_records, d_out_series, d_out_counts,
                               out_capacity, d_workspace, workspace_bytes);
    DeviceGuard on_device(device);
    launched(launch_union(U, stream), "PMT hit union");
}

void pmt_hits_split_device(int device, const void *d_records, const void *d_series, const void *d_counts, size_t capacity, uint32_t last_frame,
                           void *d_head_records, void *d_head_series, void *d_head_counts, size_t head_capacity, void *d_tail_records, void *d_tail_series,
                           void *d_tail_counts, size_t tail_capacity, hipStream_t stream)
{
    need_device(device, "the PMT hit split's device path");
    const SArgs S = split_args(d_records, d_series, d_counts, capacity, last_frame, d_head_records, d_head_series, d_head_counts, head_capacity, d_tail_records,
                               d_tail_series, d_tail_counts, tail_capacity, false);
    DeviceGuard on_device(device);
    launched(launch_split(S, stream), "PMT hit split");
}

// ---- the device store ----
namespace {

class DevicePmtHitStore final : public PmtHitStore {
public:
    DevicePmtHitStore(int device, size_t capacity) : device_(device), capacity_(capacity)
    {
        need_device(device, "a device PMT hit frame store");
        DeviceGuard on_device(device);
        for (int k = 0; k < 2; ++k) {
            records_[k].alloc(capacity, "PMT hit frame store records");
            series_[k].alloc(capacity, "PMT hit frame store table");
        }
        counts_.alloc(4u * 8u, "PMT hit frame store counts");           // two for the buffers, one of the bunch, one of a plan; eight words each
        workspace_bytes_ = pmt_hits_union_workspace_bytes(capacity, capacity);
        workspace_.alloc(workspace_bytes_, "PMT hit frame store workspace");
        sticky_.alloc(8u, "PMT hit frame store counters");              // page-locked: the device writes them, the host reads them without a copy
        std::memset(sticky_.get(), 0, 8u * sizeof(uint32_t));
        void *d = nullptr;
        hip_check(hipHostGetDevicePointer(&d, sticky_.get(), 0), "hipHostGetDevicePointer");
        d_sticky_ = static_cast<uint32_t *>(d);
        plan_.alloc(16u, "PMT hit frame store plan");
        stream_.create("PMT hit frame store stream");
        event_.create_untimed("PMT hit frame store event");
        uploaded_.create_untimed("PMT hit frame store event");
        hip_check(hipMemsetAsync(counts_.get(), 0, 4u * 8u * sizeof(uint32_t), stream_.get()), "hipMemsetAsync");
        hip_check(hipEventRecord(event_.get(), stream_.get()), "hipEventRecord");
        hip_check(hipEventRecord(uploaded_.get(), stream_.get()), "hipEventRecord");
    }
    ~DevicePmtHitStore() override
    {
        DeviceGuard on_device(device_, std::nothrow);
        (void)hipEventSynchronize(event_.get());                        // nothing of the store's is in flight when its memory goes
    }
    bool on_device() const override { return true; }

    void add_host(const clsimhip_pmt_hit *records, size_t n, const clsimhip_pmt_series *series, size_t n_series) override
    {
        pmt_hits_form_check("the bunch", records, n, series, n_series);
        if (n > capacity_) throw Error(CLSIMHIP_ERR_ARGUMENT, "PMT hit frame store: a bunch of " + std::to_string(n) + " records does not fit a store of " + std::to_string(capacity_));
        std::lock_guard<std::mutex> lk(mutex_);
        DeviceGuard on_device(device_);
        if (!bunch_records_) {
            bunch_records_.alloc(capacity_, "PMT hit frame store bunch");
            bunch_series_.alloc(capacity_, "PMT hit frame store bunch");
            staged_records_.alloc(std::max<size_t>(capacity_, 1u), "PMT hit frame store staging");
            staged_series_.alloc(std::max<size_t>(capacity_, 1u), "PMT hit frame store staging");
            staged_counts_.alloc(8u, "PMT hit frame store staging");
        }
        hip_check(hipEventSynchronize(uploaded_.get()), "hipEventSynchronize");         // the previous bunch has left the staging buffers
        if (n) std::memcpy(staged_records_.get(), records, n * sizeof(clsimhip_pmt_hit));
        if (n_series) std::memcpy(staged_series_.get(), series, n_series * sizeof(clsimhip_pmt_series));
        uint32_t *c = staged_counts_.get();
        c[0] = static_cast<uint32_t>(n); c[1] = static_cast<uint32_t>(n_series); c[2] = c[3] = c[4] = 0u;
        hipStream_t s = stream_.get();
        hip_check(hipStreamWaitEvent(s, event_.get(), 0), "hipStreamWaitEvent");        // (the previous union has read the bunch buffers)
        if (n) hip_check(hipMemcpyAsync(bunch_records_.get(), staged_records_.get(), n * sizeof(clsimhip_pmt_hit), hipMemcpyHostToDevice, s), "upload PMT hit bunch");
        if (n_series) hip_check(hipMemcpyAsync(bunch_series_.get(), staged_series_.get(), n_series * sizeof(clsimhip_pmt_series), hipMemcpyHostToDevice, s), "upload PMT hit bunch");
        hip_check(hipMemcpyAsync(counts_of(2), c, 5u * sizeof(uint32_t), hipMemcpyHostToDevice, s), "upload PMT hit bunch");
        hip_check(hipEventRecord(uploaded_.get(), s), "hipEventRecord");
        fold(bunch_records_.get(), bunch_series_.get(), counts_of(2), capacity_, s);
    }

    void add_device(const void *d_records, const void *d_series, const void *d_series_counts, size_t capacity, hipStream_t stream) override
    {
        if (capacity > capacity_)
            throw Error(CLSIMHIP_ERR_ARGUMENT, "PMT hit frame store: a bunch buffer of " + std::to_string(capacity) + " records is beyond the store's capacity of " + std::to_string(capacity_));
        std::lock_guard<std::mutex> lk(mutex_);
        DeviceGuard on_device(device_);
        hip_check(hipStreamWaitEvent(stream, event_.get(), 0), "hipStreamWaitEvent");
        fold(d_records, d_series, d_series_counts, capacity, stream);
    }

    void drain_device(uint32_t last_frame, void *d_records, void *d_series, void *d_counts, size_t capacity, hipStream_t stream) override
    {
        std::lock_guard<std::mutex> lk(mutex_);
        refuse_when_sticky();
        DeviceGuard on_device(device_);
        SArgs S = split_args(records_[current_].get(), series_[current_].get(), counts_of(current_), capacity_, last_frame, d_records, d_series, d_counts, capacity,
                             records_[current_ ^ 1].get(), series_[current_ ^ 1].get(), counts_of(current_ ^ 1), capacity_, false);
        S.blocked = d_sticky_;
        hip_check(hipStreamWaitEvent(stream, event_.get(), 0), "hipStreamWaitEvent");
        launched(launch_split(S, stream), "PMT hit frame store drain");
        current_ ^= 1;
        hip_check(hipEventRecord(event_.get(), stream), "hipEventRecord");
    }

    void drain_host(uint32_t last_frame, clsimhip_pmt_hit *records, clsimhip_pmt_series *series, size_t capacity, size_t *n, size_t *n_series) override
    {
        std::lock_guard<std::mutex> lk(mutex_);
        DeviceGuard on_device(device_);
        size_t head = 0, entries = 0;
        const SArgs S = plan(last_frame, &head, &entries);
        if (head > capacity || entries > capacity)
            throw Error(CLSIMHIP_ERR_ARGUMENT, "PMT hit frame store: the frames up to " + std::to_string(last_frame) + " hold " + std::to_string(head) + " records, the output " +
                                                   std::to_string(capacity));
        if ((head && !records) || (entries && !series)) throw Error(CLSIMHIP_ERR_ARGUMENT, "records / series is (null)");
        hipStream_t s = stream_.get();
        if (head) hip_check(hipMemcpyAsync(records, records_[current_].get(), head * sizeof(clsimhip_pmt_hit), hipMemcpyDeviceToHost, s), "download PMT hit frames");
        if (entries) hip_check(hipMemcpyAsync(series, series_[current_].get(), entries * sizeof(clsimhip_pmt_series), hipMemcpyDeviceToHost, s), "download PMT hit frames");
        hipLaunchKernelGGL(ph_split_copy_kernel, dim3(lanes_of(3ull * S.capacity)), dim3(256), 0, s, S);     // the tail becomes the store; the head has gone to the host
        launched(hipGetLastError(), "PMT hit frame store drain");
        current_ ^= 1;
        hip_check(hipEventRecord(event_.get(), s), "hipEventRecord");
        hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        if (n) *n = head;
        if (n_series) *n_series = entries;
    }

    void size(uint32_t last_frame, size_t *n, size_t *n_series) override
    {
        std::lock_guard<std::mutex> lk(mutex_);
        DeviceGuard on_device(device_);
        size_t head = 0, entries = 0;
        (void)plan(last_frame, &head, &entries);
        if (n) *n = head;
        if (n_series) *n_series = entries;
    }

private:
    uint32_t *counts_of(int which) const { return counts_.get() + 8 * which; }

    void refuse_when_sticky() const
    {
        const volatile uint32_t *c = sticky_.get();
        const uint32_t v[5] = {c[0], c[1], c[2], c[3], c[4]};
        if ((v[0] | v[1] | v[2] | v[3] | v[4]) == 0u) return;
        throw Error(CLSIMHIP_ERR_DEVICE, "PMT hit frame store: data was dropped on the device and nothing is delivered -- " + std::to_string(v[FS_MALFORMED_BUNCHES]) +
                                             " malformed bunches (" + std::to_string(v[FS_MALFORMED_ELEMENTS]) + " malformed elements), " +
                                             std::to_string(v[FS_OVERFLOWED_BUNCHES]) + " bunches that did not fit (" + std::to_string(v[FS_OVERFLOWED_RECORDS]) + " records), " +
                                             std::to_string(v[FS_MALFORMED_STORE]) + " malformed elements in the store itself");
    }

    // the union of the store and a bunch into the other pair of buffers, behind the store's event on `stream` (the caller has made
    // the stream wait for it)
    void fold(const void *d_records, const void *d_series, const void *d_series_counts, size_t capacity, hipStream_t stream)
    {
        const int other = current_ ^ 1;
        const UArgs U = union_args(records_[current_].get(), series_[current_].get(), counts_of(current_), capacity_, d_records, d_series, d_series_counts, capacity,
                                   records_[other].get(), series_[other].get(), counts_of(other), capacity_, workspace_.get(), workspace_bytes_);
        launched(launch_union(U, stream), "PMT hit frame store union");
        hipLaunchKernelGGL(ph_store_note_kernel, dim3(1), dim3(64), 0, stream, static_cast<const uint32_t *>(counts_of(other)), static_cast<const uint32_t *>(d_series_counts),
                           static_cast<uint32_t>(capacity), d_sticky_);
        launched(hipGetLastError(), "PMT hit frame store union");
        current_ = other;
        hip_check(hipEventRecord(event_.get(), stream), "hipEventRecord");
    }

    // waits for everything issued, refuses when data was dropped, and reads what a drain up to last_frame would take; the plan is
    // left in the counts of the other buffers, where ph_split_copy_kernel reads it
    SArgs plan(uint32_t last_frame, size_t *head, size_t *entries)
    {
        hipStream_t s = stream_.get();
        hip_check(hipStreamWaitEvent(s, event_.get(), 0), "hipStreamWaitEvent");
        hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        refuse_when_sticky();
        SArgs S = split_args(records_[current_].get(), series_[current_].get(), counts_of(current_), capacity_, last_frame, nullptr, nullptr, counts_of(3), capacity_,
                             records_[current_ ^ 1].get(), series_[current_ ^ 1].get(), counts_of(current_ ^ 1), capacity_, true);
        hipLaunchKernelGGL(ph_split_plan_kernel, dim3(1), dim3(64), 0, s, S);
        launched(hipGetLastError(), "PMT hit frame store plan");
        hip_check(hipMemcpyAsync(plan_.get(), counts_of(3), 5u * sizeof(uint32_t), hipMemcpyDeviceToHost, s), "download PMT hit frame store plan");
        hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        *head = plan_.get()[0];
        *entries = plan_.get()[1];
        return S;
    }

    int device_;
    size_t capacity_, workspace_bytes_ = 0;
    std::mutex mutex_;
    DeviceBuffer<clsimhip_pmt_hit> records_[2], bunch_records_;
    DeviceBuffer<clsimhip_pmt_series> series_[2], bunch_series_;
    DeviceBuffer<uint32_t> counts_;
    DeviceBuffer<uint8_t> workspace_;
    PinnedBuffer<uint32_t> sticky_, plan_, staged_counts_;
    PinnedBuffer<clsimhip_pmt_hit> staged_records_;
    PinnedBuffer<clsimhip_pmt_series> staged_series_;
    uint32_t *d_sticky_ = nullptr;
    Stream stream_;
    Event event_, uploaded_;
    int current_ = 0;
};

} // namespace

std::unique_ptr<PmtHitStore> make_device_pmt_hit_store(int device, size_t capacity)
{
    if (capacity > kFrameStoreMaxCapacity) throw Error(CLSIMHIP_ERR_ARGUMENT, "PMT hit frame store: capacity beyond 2^31 records");
    return std::unique_ptr<PmtHitStore>(new DevicePmtHitStore(device, capacity));
}

} // namespace clsimhip
