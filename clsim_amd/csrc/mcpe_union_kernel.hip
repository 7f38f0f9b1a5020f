// MCPE frame store on the device: what moves a 16-byte MCPE through the stage of series_union_device.hip.h, and that stage's
// instantiation over McpeUnion under the names mcpe_union.h exports.
//
//   union_merge_kernel             one 16-byte load per record, the tile's keys in LDS (five arrays of 2048 words, 40 KiB), every
//                                  element ranked in the other run by bisection there, the keys permuted in LDS, one 16-byte store
//                                  per record rebuilt from its key (equal keys are equal records); a head is a record whose
//                                  (frame, DOM) differs from its predecessor's.
//   union_emit_kernel              a table entry is two 8-byte words.
//   split_copy_kernel              a record and an entry are one 16-byte word each.
#include "mcpe_union.h"

#include "series_union_device.hip.h"

namespace clsimhip {

namespace {

__device__ __forceinline__ UnionKey key_at(const clsimhip_mcpe *records, const uint32_t *frames, uint32_t i)
{
    const uint64_t *rec = reinterpret_cast<const uint64_t *>(records + i);
    return union_make_key(frames[i], rec[0], rec[1]);
}

// how many of the LDS keys [from, to), an ascending run, go in front of `key`: those less than it, and with kAfterEqual those equal to it too
template <bool kAfterEqual>
__device__ __forceinline__ uint32_t rank_in(uint32_t (*keys)[kSeriesTile], uint32_t from, uint32_t to, const UnionKey &key)
{
    uint32_t lo = from, hi = to;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        bool less = false, decided = false;                             // keys[mid] < key
        bool greater = false;
#pragma unroll
        for (uint32_t k = 0; k < kUnionKeyWords; ++k) {
            const uint32_t w = keys[k][mid];
            if (!decided && w != key.w[k]) { decided = true; less = w < key.w[k]; greater = !less; }
        }
        const bool before = kAfterEqual ? !greater : less;              // the element at mid goes in front of `key`
        if (before) lo = mid + 1u; else hi = mid;
    }
    return lo - from;
}

__global__ void __launch_bounds__(256) union_merge_kernel(const UnionDeviceArgs<McpeUnion> U)
{
    const uint32_t n_a = U.header[UH_N_A], n_b = U.header[UH_N_B];
    const uint32_t n = n_a + n_b;
    const uint64_t start = (uint64_t)blockIdx.x * kSeriesTile;
    if (start >= n) return;
    __shared__ uint32_t keys[kUnionKeyWords][kSeriesTile];              // 40 KiB, structure of arrays
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
    const uint32_t filled = in_a + in_b;                                // = total
    if (threadIdx.x == 0u) heads = 0u;
    UnionKey key[kRounds];
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t e = r * 256u + threadIdx.x;
        if (e < filled) {
            const bool from_a = e < in_a;
            const uint32_t at = from_a ? i0 + e : j0 + (e - in_a);
            const uint4 rec = *reinterpret_cast<const uint4 *>((from_a ? U.a_records : U.b_records) + at);
            const uint32_t frame = (from_a ? U.a_frames : U.b_frames)[at];
            key[r] = union_make_key(frame, (uint64_t)rec.x | ((uint64_t)rec.y << 32), (uint64_t)rec.z | ((uint64_t)rec.w << 32));
#pragma unroll
            for (uint32_t k = 0; k < kUnionKeyWords; ++k) keys[k][e] = key[r].w[k];
        }
    }
    __syncthreads();
    uint32_t rank[kRounds];
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t e = r * 256u + threadIdx.x;
        rank[r] = 0u;
        if (e < in_a) rank[r] = e + rank_in<false>(keys, in_a, filled, key[r]);                 // the records of B in front: strictly less
        else if (e < filled) rank[r] = (e - in_a) + rank_in<true>(keys, 0u, in_a, key[r]);      // the records of A in front: less or equal
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t e = r * 256u + threadIdx.x;
        if (e < filled) {
            const uint32_t p = min_u32(rank[r], filled - 1u);           // (a permutation of [0, filled) for sorted runs)
#pragma unroll
            for (uint32_t k = 0; k < kUnionKeyWords; ++k) keys[k][p] = key[r].w[k];
        }
    }
    __syncthreads();
    // the predecessor of the tile's first record
    uint32_t before_frame = 0u, before_dom = 0u;
    bool have_before = false;
    if (i0 > 0u) {
        const UnionKey k = key_at(U.a_records, U.a_frames, i0 - 1u);
        before_frame = k.w[0]; before_dom = k.w[1]; have_before = true;
    }
    if (j0 > 0u) {
        const UnionKey k = key_at(U.b_records, U.b_frames, j0 - 1u);
        if (!have_before || k.w[0] > before_frame || (k.w[0] == before_frame && k.w[1] > before_dom)) { before_frame = k.w[0]; before_dom = k.w[1]; }
        have_before = true;
    }
    uint32_t mine = 0u;
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t p = r * 256u + threadIdx.x;
        if (p < filled) {
            const uint32_t frame = keys[0][p], dom = keys[1][p];
            const uint64_t t = ((uint64_t)keys[2][p] << 32) | keys[3][p];
            const uint64_t bits = __builtin_bit_cast(uint64_t, series_time_of(t));
            const uint64_t g = start + p;                               // < n <= out_capacity
            *reinterpret_cast<uint4 *>(U.out_records + g) = make_uint4(keys[4][p], union_dom_word(dom), (uint32_t)bits, (uint32_t)(bits >> 32));
            U.out_frames[g] = frame;
            bool head;
            if (p > 0u) head = keys[0][p - 1u] != frame || keys[1][p - 1u] != dom;
            else head = !have_before || before_frame != frame || before_dom != dom;
            mine += head ? 1u : 0u;
        }
    }
    if (mine != 0u) atomicAdd(&heads, mine);
    __syncthreads();
    if (threadIdx.x == 0u) U.tile_counts[blockIdx.x] = heads;
}

__global__ void __launch_bounds__(256) union_emit_kernel(const UnionDeviceArgs<McpeUnion> U)
{
    const uint32_t n = U.header[SH_KEPT];
    const uint64_t start = (uint64_t)blockIdx.x * kSeriesTile;
    if (start >= n) return;
    __shared__ uint32_t wave_heads[4];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t frame[kRounds], dom[kRounds];
    uint64_t heads[kRounds];
    uint32_t total = 0u;
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint64_t i = start + wave * 512u + r * 64u + lane;
        bool head = false;
        if (i < n) {
            frame[r] = U.out_frames[i];
            dom[r] = (uint32_t)(reinterpret_cast<const uint64_t *>(U.out_records + i)[0] >> 32);
            head = i == 0u || frame[r] != U.out_frames[i - 1u] || dom[r] != (uint32_t)(reinterpret_cast<const uint64_t *>(U.out_records + (i - 1u))[0] >> 32);
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
                entry[1] = (uint64_t)(uint32_t)i;                       // count: union_close_kernel
            }
        }
        index += (uint32_t)__popcll(heads[r]);
    }
}

__global__ void __launch_bounds__(256) split_copy_kernel(const SplitDeviceArgs<McpeUnion> S)
{
    const uint32_t head = S.head_counts[0], entries = S.head_counts[1];             // <= head_capacity
    const uint32_t n = min_u32(S.counts[0], S.capacity), n_series = min_u32(S.counts[1], S.capacity);
    const uint64_t start = (uint64_t)blockIdx.x * 256u + threadIdx.x, stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t i = start; i < n; i += stride) {
        const uint4 rec = *reinterpret_cast<const uint4 *>(S.records + i);
        if (i < head) {
            if (S.head_records) *reinterpret_cast<uint4 *>(S.head_records + i) = rec;
        } else
            *reinterpret_cast<uint4 *>(S.tail_records + (i - head)) = rec;          // < n - head <= capacity <= the tail's
    }
    for (uint64_t s = start; s < n_series; s += stride) {
        uint4 entry = *reinterpret_cast<const uint4 *>(S.series + s);
        if (s < entries) {
            if (S.head_series) *reinterpret_cast<uint4 *>(S.head_series + s) = entry;
        } else {
            entry.z -= head;                                                        // first
            *reinterpret_cast<uint4 *>(S.tail_series + (s - entries)) = entry;
        }
    }
}

} // namespace

// the stage's own kernels and key loader, as series_union_device.hip.h launches and calls them
template <>
struct UnionMovers<McpeUnion> {
    static constexpr uint32_t kCopyItemsPerRecord = 1u;
    static constexpr auto merge = union_merge_kernel, emit = union_emit_kernel;
    static constexpr auto split_copy = split_copy_kernel;
    static __device__ __forceinline__ UnionKey key_at(const clsimhip_mcpe *records, const uint32_t *frames, uint32_t i) { return clsimhip::key_at(records, frames, i); }
};

size_t mcpe_union_workspace_bytes(size_t capacity_a, size_t capacity_b) { return union_workspace_bytes(capacity_a, capacity_b); }

void mcpe_union_device(int device, const void *d_a_records, const void *d_a_series, const void *d_a_counts, size_t capacity_a, const void *d_b_records,
                       const void *d_b_series, const void *d_b_counts, size_t capacity_b, void *d_out_records, void *d_out_series, void *d_out_counts,
                       size_t out_capacity, void *d_workspace, size_t workspace_bytes, hipStream_t stream)
{
    series_union_device<McpeUnion>(device, d_a_records, d_a_series, d_a_counts, capacity_a, d_b_records, d_b_series, d_b_counts, capacity_b, d_out_records, d_out_series,
                                   d_out_counts, out_capacity, d_workspace, workspace_bytes, stream);
}

void mcpe_split_device(int device, const void *d_records, const void *d_series, const void *d_counts, size_t capacity, uint32_t last_frame,
                       void *d_head_records, void *d_head_series, void *d_head_counts, size_t head_capacity, void *d_tail_records, void *d_tail_series,
                       void *d_tail_counts, size_t tail_capacity, hipStream_t stream)
{
    series_split_device<McpeUnion>(device, d_records, d_series, d_counts, capacity, last_frame, d_head_records, d_head_series, d_head_counts, head_capacity,
                                   d_tail_records, d_tail_series, d_tail_counts, tail_capacity, stream);
}

std::unique_ptr<FrameStore> make_device_frame_store(int device, size_t capacity) { return make_device_frame_store_of<McpeUnion>(device, capacity); }

} // namespace clsimhip
