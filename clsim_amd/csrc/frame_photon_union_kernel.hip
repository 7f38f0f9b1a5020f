// Frame photon store on the device: what moves a 48-byte frame photon through the stage of series_union_device.hip.h, and that
// stage's instantiation over FramePhotonUnion under the names frame_photon_union.h exports.  The record is moved, not rebuilt from its
// key, and the key has 14 words.
//
//   fp_union_merge_kernel      a lane loads its eight records once (three 16-byte loads each) and keeps them in registers.
//                              LDS holds the SIX LEADING key words of the tile (frame, DOM code, tkey high, tkey low, identifier, h:
//                              six arrays of 2048 words, 48 KiB); a full 14-word tile would be 112 KiB.  Every element is ranked in
//                              the other run by bisection there; where the six words tie -- and only there -- the probe's eight
//                              content words are read from the records in global memory (two 16-byte loads that hit L2: the tile has
//                              just been read).  That second read is what keeps LDS under 64 KiB; it is bounded by 11 probes per
//                              element, whatever the tie run's length or contents, so there is no tie bound.  The record then goes
//                              from its registers to its place (three 16-byte stores): loaded once, stored once, and no source index
//                              is kept.  (frame, DOM code) are permuted in LDS for the heads: a head is a record whose (frame, DOM)
//                              differs from its predecessor's.
//   fp_union_emit_kernel       a table entry is two 8-byte words.
//   fp_split_copy_kernel       three 16-byte loads and stores per record, one per entry.
#include "frame_photon_union.h"

#include "series_union_device.hip.h"

namespace clsimhip {

namespace {

using UArgs = UnionDeviceArgs<FramePhotonUnion>;
using SArgs = SplitDeviceArgs<FramePhotonUnion>;

// a record's twelve words by three 16-byte loads (records are 16-byte aligned: the callers check the base)
__device__ __forceinline__ void load_record(const clsimhip_frame_photon *records, uint32_t i, uint32_t (&rec)[kFramePhotonRecordWords])
{
    const uint4 *p = reinterpret_cast<const uint4 *>(records + i);
    const uint4 g0 = p[0], g1 = p[1], g2 = p[2];
    rec[0] = g0.x; rec[1] = g0.y; rec[2] = g0.z; rec[3] = g0.w;
    rec[4] = g1.x; rec[5] = g1.y; rec[6] = g1.z; rec[7] = g1.w;
    rec[8] = g2.x; rec[9] = g2.y; rec[10] = g2.z; rec[11] = g2.w;
}

__device__ __forceinline__ FramePhotonKey key_at(const clsimhip_frame_photon *records, const uint32_t *frames, uint32_t i)
{
    uint32_t rec[kFramePhotonRecordWords];
    load_record(records, i, rec);
    return frame_photon_union_make_key(frames[i], rec);
}

constexpr uint32_t kLeadingWords = 6u;                                  // frame, DOM code, tkey high, tkey low, identifier, h

// how many of the tile's elements [from, to), an ascending run, go in front of the element with the leading words `lead` and the
// content rec[4 .. 11]: those less than it, and with kAfterEqual those equal to it too.  The leading words of the run are in LDS;
// the content of the element at tile position e is in `base` at e - base_at (global memory), read where the leading words tie.
template <bool kAfterEqual>
__device__ __forceinline__ uint32_t rank_in(uint32_t (*keys)[kSeriesTile], uint32_t from, uint32_t to, const uint32_t (&lead)[kLeadingWords],
                                            const uint32_t (&rec)[kFramePhotonRecordWords], const clsimhip_frame_photon *base, uint32_t base_at)
{
    uint32_t lo = from, hi = to;
    while (lo < hi) {                                                   // at most 11 trips: to - from <= 2048
        const uint32_t mid = lo + (hi - lo) / 2u;
        bool less = false, decided = false;                             // keys[mid] < key
        bool greater = false;
#pragma unroll
        for (uint32_t k = 0; k < kLeadingWords; ++k) {
            const uint32_t w = keys[k][mid];
            if (!decided && w != lead[k]) { decided = true; less = w < lead[k]; greater = !less; }
        }
        if (!decided) {                                                 // a content tie: w0 ... w7 of the element at mid
            const uint4 *p = reinterpret_cast<const uint4 *>(base + (mid - base_at));       // from <= mid < to: inside the tile's share of the run
            const uint4 c0 = p[1], c1 = p[2];
            const uint32_t w[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
#pragma unroll
            for (uint32_t k = 0; k < 8u; ++k)
                if (!decided && w[k] != rec[4u + k]) { decided = true; less = w[k] < rec[4u + k]; greater = !less; }
        }
        const bool before = kAfterEqual ? !greater : less;              // the element at mid goes in front of `key`
        if (before) lo = mid + 1u; else hi = mid;
    }
    return lo - from;
}

__global__ void __launch_bounds__(256) fp_union_merge_kernel(const UArgs U)
{
    const uint32_t n_a = U.header[UH_N_A], n_b = U.header[UH_N_B];
    const uint32_t n = n_a + n_b;
    const uint64_t start = (uint64_t)blockIdx.x * kSeriesTile;
    if (start >= n) return;
    __shared__ uint32_t keys[kLeadingWords][kSeriesTile];               // 48 KiB, structure of arrays
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
    // tile position e is A[i0 + e] for e < in_a and B[j0 + e - in_a] behind
    const clsimhip_frame_photon *const a_base = U.a_records + i0, *const b_base = U.b_records + j0;
    uint32_t rec[kRounds][kFramePhotonRecordWords], lead[kRounds][kLeadingWords];
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t e = r * 256u + threadIdx.x;
        if (e < filled) {
            const bool from_a = e < in_a;
            const uint32_t at = from_a ? i0 + e : j0 + (e - in_a);     // < n_a, < n_b
            load_record(from_a ? U.a_records : U.b_records, at, rec[r]);
            const FramePhotonKey key = frame_photon_union_make_key((from_a ? U.a_frames : U.b_frames)[at], rec[r]);
#pragma unroll
            for (uint32_t k = 0; k < kLeadingWords; ++k) { lead[r][k] = key.w[k]; keys[k][e] = key.w[k]; }
        }
    }
    __syncthreads();
    uint32_t rank[kRounds];
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t e = r * 256u + threadIdx.x;
        rank[r] = 0u;
        if (e < in_a) rank[r] = e + rank_in<false>(keys, in_a, filled, lead[r], rec[r], b_base, in_a);          // the records of B in front: strictly less
        else if (e < filled) rank[r] = (e - in_a) + rank_in<true>(keys, 0u, in_a, lead[r], rec[r], a_base, 0u); // the records of A in front: less or equal
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t e = r * 256u + threadIdx.x;
        if (e < filled) {
            rank[r] = min_u32(rank[r], filled - 1u);                    // (a permutation of [0, filled) for sorted runs)
            keys[0][rank[r]] = lead[r][0];
            keys[1][rank[r]] = lead[r][1];
        }
    }
    __syncthreads();
    // the predecessor of the tile's first record
    uint32_t before_frame = 0u, before_dom = 0u;
    bool have_before = false;
    if (i0 > 0u) {
        before_frame = U.a_frames[i0 - 1u];
        before_dom = union_dom_code(reinterpret_cast<const uint32_t *>(U.a_records + (i0 - 1u))[1]);
        have_before = true;
    }
    if (j0 > 0u) {
        const uint32_t frame = U.b_frames[j0 - 1u], dom = union_dom_code(reinterpret_cast<const uint32_t *>(U.b_records + (j0 - 1u))[1]);
        if (!have_before || frame > before_frame || (frame == before_frame && dom > before_dom)) { before_frame = frame; before_dom = dom; }
        have_before = true;
    }
    uint32_t mine = 0u;
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t e = r * 256u + threadIdx.x;
        if (e < filled) {
            const uint32_t p = rank[r];
            const uint64_t g = start + p;                               // < n <= out_capacity
            uint4 *out = reinterpret_cast<uint4 *>(U.out_records + g);
            out[0] = make_uint4(rec[r][0], rec[r][1], rec[r][2], rec[r][3]);
            out[1] = make_uint4(rec[r][4], rec[r][5], rec[r][6], rec[r][7]);
            out[2] = make_uint4(rec[r][8], rec[r][9], rec[r][10], rec[r][11]);
            U.out_frames[g] = lead[r][0];
            bool head;
            if (p > 0u) head = keys[0][p - 1u] != lead[r][0] || keys[1][p - 1u] != lead[r][1];
            else head = !have_before || before_frame != lead[r][0] || before_dom != lead[r][1];
            mine += head ? 1u : 0u;
        }
    }
    if (mine != 0u) atomicAdd(&heads, mine);
    __syncthreads();
    if (threadIdx.x == 0u) U.tile_counts[blockIdx.x] = heads;
}

__global__ void __launch_bounds__(256) fp_union_emit_kernel(const UArgs U)
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
            dom[r] = reinterpret_cast<const uint32_t *>(U.out_records + i)[1];
            head = i == 0u || frame[r] != U.out_frames[i - 1u] || dom[r] != reinterpret_cast<const uint32_t *>(U.out_records + (i - 1u))[1];
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

__global__ void __launch_bounds__(256) fp_split_copy_kernel(const SArgs S)
{
    const uint32_t head = S.head_counts[0], entries = S.head_counts[1];             // <= head_capacity
    const uint32_t n = min_u32(S.counts[0], S.capacity), n_series = min_u32(S.counts[1], S.capacity);
    const uint64_t start = (uint64_t)blockIdx.x * 256u + threadIdx.x, stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t i = start; i < n; i += stride) {
        const uint4 *in = reinterpret_cast<const uint4 *>(S.records + i);
        const uint4 g0 = in[0], g1 = in[1], g2 = in[2];
        uint4 *out = nullptr;
        if (i < head) {
            if (S.head_records) out = reinterpret_cast<uint4 *>(S.head_records + i);
        } else
            out = reinterpret_cast<uint4 *>(S.tail_records + (i - head));           // < n - head <= capacity <= the tail's
        if (out) { out[0] = g0; out[1] = g1; out[2] = g2; }
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
struct UnionMovers<FramePhotonUnion> {
    static constexpr uint32_t kCopyItemsPerRecord = 1u;
    static constexpr auto merge = fp_union_merge_kernel, emit = fp_union_emit_kernel;
    static constexpr auto split_copy = fp_split_copy_kernel;
    static __device__ __forceinline__ FramePhotonKey key_at(const clsimhip_frame_photon *records, const uint32_t *frames, uint32_t i) { return clsimhip::key_at(records, frames, i); }
};

size_t frame_photons_union_workspace_bytes(size_t capacity_a, size_t capacity_b) { return union_workspace_bytes(capacity_a, capacity_b); }

void frame_photons_union_device(int device, const void *d_a_records, const void *d_a_series, const void *d_a_counts, size_t capacity_a, const void *d_b_records,
                                const void *d_b_series, const void *d_b_counts, size_t capacity_b, void *d_out_records, void *d_out_series, void *d_out_counts,
                                size_t out_capacity, void *d_workspace, size_t workspace_bytes, hipStream_t stream)
{
    series_union_device<FramePhotonUnion>(device, d_a_records, d_a_series, d_a_counts, capacity_a, d_b_records, d_b_series, d_b_counts, capacity_b, d_out_records,
                                          d_out_series, d_out_counts, out_capacity, d_workspace, workspace_bytes, stream);
}

void frame_photons_split_device(int device, const void *d_records, const void *d_series, const void *d_counts, size_t capacity, uint32_t last_frame,
                                void *d_head_records, void *d_head_series, void *d_head_counts, size_t head_capacity, void *d_tail_records, void *d_tail_series,
                                void *d_tail_counts, size_t tail_capacity, hipStream_t stream)
{
    series_split_device<FramePhotonUnion>(device, d_records, d_series, d_counts, capacity, last_frame, d_head_records, d_head_series, d_head_counts, head_capacity,
                                          d_tail_records, d_tail_series, d_tail_counts, tail_capacity, stream);
}

std::unique_ptr<FramePhotonStore> make_device_frame_photon_store(int device, size_t capacity) { return make_device_frame_store_of<FramePhotonUnion>(device, capacity); }

} // namespace clsimhip
