// PMT hit frame store on the device: what moves a 24-byte PMT hit and its 24-byte table entry (8-byte aligned both) through the stage
// of series_union_device.hip.h, and that stage's instantiation over PmtHitUnion under the names pmt_hit_union.h exports.
//
//   ph_union_merge_kernel      LDS holds the WHOLE key of the tile (six arrays of 2048 words, 48 KiB: three workgroups per
//                              compute unit).  A lane loads its eight records (three 8-byte loads each), keeps their keys in
//                              registers and ranks each in the other run by bisection in LDS: a lane of A counts B's elements
//                              strictly less, a lane of B counts A's less or equal -- a permutation for two series forms, clamped
//                              below the tile's fill for anything else.  The keys are then permuted in LDS, and because a record is
//                              a function of its key the output is REBUILT from the sorted keys, not moved: the tile's output is
//                              3 x fill 8-byte words, and lane q writes word q, q + 256 ... so that a wave's stores are 512
//                              contiguous bytes (24 is no multiple of 16; a lane that stored its own record would scatter three
//                              8-byte stores to a permuted place).  A head is a record whose (frame, DOM code, pmt) differs from its
//                              LDS neighbour's.
//   ph_union_emit_kernel       a table entry is three 8-byte words.
//   ph_split_copy_kernel       a grid-stride copy of 8-byte words, three per record.
#include "pmt_hit_union.h"

#include "series_union_device.hip.h"

namespace clsimhip {

namespace {

using UArgs = UnionDeviceArgs<PmtHitUnion>;
using SArgs = SplitDeviceArgs<PmtHitUnion>;

// a record's or an entry's six words by three 8-byte loads (records and tables are 8-byte aligned: the callers check the base)
__device__ __forceinline__ void load_words(const void *base, uint64_t i, uint32_t (&w)[6])
{
    const uint64_t *p = static_cast<const uint64_t *>(base) + 3u * i;
    const uint64_t g0 = p[0], g1 = p[1], g2 = p[2];
    w[0] = (uint32_t)g0; w[1] = (uint32_t)(g0 >> 32);
    w[2] = (uint32_t)g1; w[3] = (uint32_t)(g1 >> 32);
    w[4] = (uint32_t)g2; w[5] = (uint32_t)(g2 >> 32);
}

__device__ __forceinline__ PmtHitKey key_at(const clsimhip_pmt_hit *records, const uint32_t *frames, uint32_t i)
{
    uint32_t rec[kPmtHitRecordWords];
    load_words(records, i, rec);
    return pmt_hit_union_make_key(frames[i], rec);
}

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
                entry[2] = 0u;                                                      // count: union_close_kernel   ; reserved = 0
            }
        }
        index += (uint32_t)__popcll(heads[r]);
    }
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

} // namespace

// the stage's own kernels and key loader, as series_union_device.hip.h launches and calls them
template <>
struct UnionMovers<PmtHitUnion> {
    static constexpr uint32_t kCopyItemsPerRecord = 3u                  /* 8-byte words */;
    static constexpr auto merge = ph_union_merge_kernel, emit = ph_union_emit_kernel;
    static constexpr auto split_copy = ph_split_copy_kernel;
    static __device__ __forceinline__ PmtHitKey key_at(const clsimhip_pmt_hit *records, const uint32_t *frames, uint32_t i) { return clsimhip::key_at(records, frames, i); }
};

size_t pmt_hits_union_workspace_bytes(size_t capacity_a, size_t capacity_b) { return union_workspace_bytes(capacity_a, capacity_b); }

void pmt_hits_union_device(int device, const void *d_a_records, const void *d_a_series, const void *d_a_counts, size_t capacity_a, const void *d_b_records,
                           const void *d_b_series, const void *d_b_counts, size_t capacity_b, void *d_out_records, void *d_out_series, void *d_out_counts,
                           size_t out_capacity, void *d_workspace, size_t workspace_bytes, hipStream_t stream)
{
    series_union_device<PmtHitUnion>(device, d_a_records, d_a_series, d_a_counts, capacity_a, d_b_records, d_b_series, d_b_counts, capacity_b, d_out_records, d_out_series,
                                     d_out_counts, out_capacity, d_workspace, workspace_bytes, stream);
}

void pmt_hits_split_device(int device, const void *d_records, const void *d_series, const void *d_counts, size_t capacity, uint32_t last_frame,
                           void *d_head_records, void *d_head_series, void *d_head_counts, size_t head_capacity, void *d_tail_records, void *d_tail_series,
                           void *d_tail_counts, size_t tail_capacity, hipStream_t stream)
{
    series_split_device<PmtHitUnion>(device, d_records, d_series, d_counts, capacity, last_frame, d_head_records, d_head_series, d_head_counts, head_capacity,
                                     d_tail_records, d_tail_series, d_tail_counts, tail_capacity, stream);
}

std::unique_ptr<PmtHitStore> make_device_pmt_hit_store(int device, size_t capacity) { return make_device_frame_store_of<PmtHitUnion>(device, capacity); }

} // namespace clsimhip
