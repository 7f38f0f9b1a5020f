// Frame stores on the device (series_union.h): the union as a merge of two sorted runs, for gfx950 (wave64), the split, their host
// side (workspace, argument checks, launches) and the device store, stated once over a traits type T.  mcpe_union_kernel.hip,
// frame_photon_union_kernel.hip and pmt_hit_union_kernel.hip include this header, state what moves their records, and instantiate the
// rest under their exported names.
//
//   union_check_kernel     one lane per entry and per record of both inputs: the local checks of a series form (a record finds its
//                          entry by bisection over `first`), MALFORMED elements counted per input, and per record its entry's frame.
//   union_plan_kernel      one workgroup: the effective sizes -- A malformed: nothing; B malformed or a union that does not fit: A alone.
//   union_partition_kernel one lane per output tile boundary: how many records of A lie in front of it, by bisection along the merge
//                          path's diagonal on the full key (ties: A first).
//   UnionMovers<T>::merge  the stage's own: one workgroup per output tile of 2048 records, whatever the lengths of the series;
//                          every element is ranked in the other run by bisection in LDS.  What LDS holds and how a record reaches
//                          its place is the record's own matter.  A head is a record whose channel differs from its predecessor's,
//                          the tile's first record's predecessor being the larger of A[i-1] and B[j-1].
//   launch_series_tile_scan / UnionMovers<T>::emit (the stage's own: it writes table entries) / union_close_kernel
//                          the series stage's scan over the heads per tile, then the table, as in the PMT series stage.
//   split_plan_kernel / UnionMovers<T>::split_copy (the stage's own: it moves records and entries)
//                          the entries with frame <= last_frame by bisection, then copies; the tail's `first` rebased.
//   store_note_kernel      the store's bookkeeping behind a union.
//
// The per-type kernels are the stage's own, named to this header by its specialisation of UnionMovers<T>: the widths of their loads
// and stores are the point of them.  Everything reads its sizes from device memory: nothing waits for the
// host.  Atomics only count.  Every loop is bounded by a capacity and every index is clamped to one, whatever bytes the inputs hold.
#pragma once
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "hip_resources.h"
#include "mcpe_series.h"
#include "series_bunch.h"
#include "series_union_host.h"

namespace clsimhip {

__device__ __forceinline__ uint32_t lanes_below(uint64_t mask)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__device__ __forceinline__ uint32_t min_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }

constexpr uint32_t kRounds = kSeriesTile / 256u;                        // 8 elements per lane

// ---- what a stage states itself: a specialisation with ----
//   merge, emit, split_copy   its three own kernels (pointers to __global__ functions taking UnionDeviceArgs<T>, UnionDeviceArgs<T>
//                             and SplitDeviceArgs<T>), launched here with the geometry the comment at the head gives
//   kCopyItemsPerRecord       the items split_copy strides over, per record
//   static __device__ Key key_at(const Record *records, const uint32_t *frames, uint32_t i)
//                             the key of record i, by the loads the record's size and alignment allow
template <class T> struct UnionMovers;

// ---- what no record changes ----
template <class T>
__global__ void __launch_bounds__(256) union_check_kernel(const UnionDeviceArgs<T> U)
{
    const uint32_t n_a = min_u32(U.a_counts[0], U.capacity_a), s_a = min_u32(U.a_counts[1], U.capacity_a);
    const uint32_t n_b = min_u32(U.b_counts[0], U.capacity_b), s_b = min_u32(U.b_counts[1], U.capacity_b);
    if (blockIdx.x == 0u && threadIdx.x == 0u) {
        U.header[UH_IN_A] = n_a; U.header[UH_SERIES_A] = s_a;
        U.header[UH_IN_B] = n_b; U.header[UH_SERIES_B] = s_b;
    }
    const uint64_t start = (uint64_t)blockIdx.x * 256u + threadIdx.x, stride = (uint64_t)gridDim.x * 256u;
    uint32_t bad_a = 0u, bad_b = 0u;
    for (uint64_t s = start; s < s_a; s += stride) bad_a += T::entry_ok(U.a_series, s_a, n_a, (uint32_t)s) ? 0u : 1u;
    for (uint64_t s = start; s < s_b; s += stride) bad_b += T::entry_ok(U.b_series, s_b, n_b, (uint32_t)s) ? 0u : 1u;
    for (uint64_t i = start; i < n_a; i += stride) {
        uint32_t frame;
        bad_a += T::record_ok(U.a_records, U.a_series, s_a, (uint32_t)i, &frame) ? 0u : 1u;
        U.a_frames[i] = frame;                                          // i < n_a <= capacity_a
    }
    for (uint64_t i = start; i < n_b; i += stride) {
        uint32_t frame;
        bad_b += T::record_ok(U.b_records, U.b_series, s_b, (uint32_t)i, &frame) ? 0u : 1u;
        U.b_frames[i] = frame;
    }
    if (bad_a != 0u) atomicAdd(U.header + UH_MALFORMED_A, bad_a);
    if (bad_b != 0u) atomicAdd(U.header + UH_MALFORMED_B, bad_b);
}

template <class T>
__global__ void __launch_bounds__(64) union_plan_kernel(const UnionDeviceArgs<T> U)
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

template <class T>
__global__ void __launch_bounds__(256) union_partition_kernel(const UnionDeviceArgs<T> U)
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
            if (union_key_less<T>(UnionMovers<T>::key_at(U.b_records, U.b_frames, diagonal - mid - 1u), UnionMovers<T>::key_at(U.a_records, U.a_frames, mid))) hi = mid;
            else lo = mid + 1u;
        }
        U.partition[t] = lo;                                            // t <= tiles(capacity_a + capacity_b)
    }
}

template <class T>
__global__ void __launch_bounds__(256) union_close_kernel(const UnionDeviceArgs<T> U)
{
    const uint32_t n = U.header[SH_KEPT], n_series = min_u32(U.header[SH_SERIES], U.out_capacity);
    for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < n_series; s += (uint64_t)gridDim.x * 256u) {
        const uint32_t next = s + 1u < n_series ? U.out_series[s + 1u].first : n;
        U.out_series[s].count = next - U.out_series[s].first;
    }
    if (blockIdx.x == 0u && threadIdx.x < 5u) U.out_counts[threadIdx.x] = threadIdx.x == 1u ? n_series : U.header[threadIdx.x];
}

template <class T>
__global__ void __launch_bounds__(64) split_plan_kernel(const SplitDeviceArgs<T> S)
{
    if (threadIdx.x != 0u) return;
    const uint32_t n = min_u32(S.counts[0], S.capacity), n_series = min_u32(S.counts[1], S.capacity);
    uint32_t entries = union_split_entries(S.series, n_series, S.last_frame);
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

// the store's bookkeeping behind a union: what the union dropped goes into the sticky counters (one lane; plain stores).  It touches
// no record: T gives every stage's launch its own name in a trace.
template <class T>
__global__ void __launch_bounds__(64) store_note_kernel(const uint32_t *union_counts, const uint32_t *bunch_counts, uint32_t bunch_capacity, uint32_t *sticky)
{
    if (threadIdx.x != 0u) return;
    if (union_counts[2] != 0u) sticky[FS_MALFORMED_STORE] += union_counts[2];
    else if (union_counts[3] != 0u) { sticky[FS_MALFORMED_BUNCHES] += 1u; sticky[FS_MALFORMED_ELEMENTS] += union_counts[3]; }
    else if (union_counts[4] != 0u) { sticky[FS_OVERFLOWED_BUNCHES] += 1u; sticky[FS_OVERFLOWED_RECORDS] += min_u32(bunch_counts[0], bunch_capacity); }
}

// ---- the host side (round16: series_bunch.h) ----
inline uint32_t tiles_of(uint64_t records)
{
    const uint64_t tiles = (records + kSeriesTile - 1u) / kSeriesTile;
    return tiles == 0u ? 1u : (uint32_t)tiles;
}

inline uint32_t lanes_of(uint64_t records)
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

template <class T>
hipError_t launch_union(const UnionDeviceArgs<T> &U, hipStream_t stream)
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
    hipLaunchKernelGGL(union_check_kernel<T>, dim3(lanes_of(std::max<uint64_t>(U.capacity_a, U.capacity_b))), dim3(256), 0, stream, U);
    hipLaunchKernelGGL(union_plan_kernel<T>, dim3(1), dim3(64), 0, stream, U);
    hipLaunchKernelGGL(union_partition_kernel<T>, dim3(lanes_of((uint64_t)tiles + 1u)), dim3(256), 0, stream, U);
    hipLaunchKernelGGL(UnionMovers<T>::merge, dim3(tiles), dim3(256), 0, stream, U);
    launch_series_tile_scan(S, stream);
    hipLaunchKernelGGL(UnionMovers<T>::emit, dim3(tiles), dim3(256), 0, stream, U);
    hipLaunchKernelGGL(union_close_kernel<T>, dim3(lanes_of(out)), dim3(256), 0, stream, U);
    return hipGetLastError();
}

template <class T>
hipError_t launch_split_copy(const SplitDeviceArgs<T> &S, hipStream_t stream)
{
    hipLaunchKernelGGL(UnionMovers<T>::split_copy, dim3(lanes_of((uint64_t)UnionMovers<T>::kCopyItemsPerRecord * S.capacity)), dim3(256), 0, stream, S);
    return hipGetLastError();
}

template <class T>
hipError_t launch_split(const SplitDeviceArgs<T> &S, hipStream_t stream)
{
    hipLaunchKernelGGL(split_plan_kernel<T>, dim3(1), dim3(64), 0, stream, S);
    return launch_split_copy(S, stream);
}

inline void need_device(int device, const std::string &what)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) throw Error(CLSIMHIP_ERR_DEVICE, "no HIP device available (" + what + " has no CPU fallback)");
    if (device < 0 || device >= count) throw Error(CLSIMHIP_ERR_ARGUMENT, "device ordinal out of range");
}

inline void launched(hipError_t e, const std::string &what)
{
    if (e != hipSuccess) throw Error(CLSIMHIP_ERR_DEVICE, what + " kernel launch: " + hipGetErrorString(e));
}

// whether any of the addresses has one of the mask's bits set
template <class... P>
bool misaligned(uintptr_t mask, const P *...p) { return (((reinterpret_cast<uintptr_t>(p)) | ...) & mask) != 0u; }

template <class T>
UnionDeviceArgs<T> union_args(const void *d_a_records, const void *d_a_series, const void *d_a_counts, size_t capacity_a, const void *d_b_records, const void *d_b_series,
                              const void *d_b_counts, size_t capacity_b, void *d_out_records, void *d_out_series, void *d_out_counts, size_t out_capacity,
                              void *d_workspace, size_t workspace_bytes)
{
    using Record = typename T::Record;
    using Entry = typename T::Entry;
    if (!d_a_counts || !d_b_counts || !d_out_counts || !d_workspace) throw Error(CLSIMHIP_ERR_ARGUMENT, "device pointers are (null)");
    if ((capacity_a && (!d_a_records || !d_a_series)) || (capacity_b && (!d_b_records || !d_b_series)) || (out_capacity && (!d_out_records || !d_out_series)))
        throw Error(CLSIMHIP_ERR_ARGUMENT, "d_a_records / d_a_series / d_b_records / d_b_series / d_out_records / d_out_series is (null)");
    frame_store_capacity_check<T>(std::max({capacity_a, capacity_b, out_capacity}));
    if (misaligned(T::kAlign - 1u, d_a_records, d_a_series, d_b_records, d_b_series, d_out_records, d_out_series) || misaligned(15u, d_workspace) ||
        misaligned(3u, d_a_counts, d_b_counts, d_out_counts))
        throw Error(CLSIMHIP_ERR_ARGUMENT, T::kAlign == 16u ? "records, series tables and d_workspace must be aligned to 16 bytes, the counts to 4"
                                                            : "records and series tables must be aligned to 8 bytes, d_workspace to 16, the counts to 4");
    const UnionWorkspace W(capacity_a, capacity_b);
    if (workspace_bytes < W.bytes)
        throw Error(CLSIMHIP_ERR_ARGUMENT, std::string("the ") + T::kName + " union workspace holds " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(W.bytes) +
                                               " are needed");
    uint8_t *ws = static_cast<uint8_t *>(d_workspace);
    UnionDeviceArgs<T> U{};
    U.a_records = static_cast<const Record *>(d_a_records);
    U.a_series = static_cast<const Entry *>(d_a_series);
    U.a_counts = static_cast<const uint32_t *>(d_a_counts);
    U.b_records = static_cast<const Record *>(d_b_records);
    U.b_series = static_cast<const Entry *>(d_b_series);
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
    U.out_records = static_cast<Record *>(d_out_records);
    U.out_series = static_cast<Entry *>(d_out_series);
    U.out_counts = static_cast<uint32_t *>(d_out_counts);
    return U;
}

template <class T>
SplitDeviceArgs<T> split_args(const void *d_records, const void *d_series, const void *d_counts, size_t capacity, uint32_t last_frame, void *d_head_records,
                              void *d_head_series, void *d_head_counts, size_t head_capacity, void *d_tail_records, void *d_tail_series, void *d_tail_counts,
                              size_t tail_capacity, bool head_may_be_dropped)
{
    using Record = typename T::Record;
    using Entry = typename T::Entry;
    if (!d_counts || !d_head_counts || !d_tail_counts) throw Error(CLSIMHIP_ERR_ARGUMENT, "device pointers are (null)");
    if (capacity && (!d_records || !d_series || !d_tail_records || !d_tail_series)) throw Error(CLSIMHIP_ERR_ARGUMENT, "d_records / d_series / d_tail_records / d_tail_series is (null)");
    if (!head_may_be_dropped && head_capacity && (!d_head_records || !d_head_series)) throw Error(CLSIMHIP_ERR_ARGUMENT, "d_head_records / d_head_series is (null)");
    frame_store_capacity_check<T>(std::max(capacity, head_capacity));
    if (tail_capacity < capacity)
        throw Error(CLSIMHIP_ERR_ARGUMENT, std::string(T::kStore) + ": the tail's capacity must not be below the input's (a bound that drains nothing leaves everything in the tail)");
    if (misaligned(T::kAlign - 1u, d_records, d_series, d_head_records, d_head_series, d_tail_records, d_tail_series) || misaligned(3u, d_counts, d_head_counts, d_tail_counts))
        throw Error(CLSIMHIP_ERR_ARGUMENT, "records and series tables must be aligned to " + std::to_string(T::kAlign) + " bytes, the counts to 4");
    SplitDeviceArgs<T> S{};
    S.records = static_cast<const Record *>(d_records);
    S.series = static_cast<const Entry *>(d_series);
    S.counts = static_cast<const uint32_t *>(d_counts);
    S.capacity = static_cast<uint32_t>(capacity);
    S.last_frame = last_frame;
    S.head_records = static_cast<Record *>(d_head_records);
    S.head_series = static_cast<Entry *>(d_head_series);
    S.head_counts = static_cast<uint32_t *>(d_head_counts);
    S.head_capacity = static_cast<uint32_t>(head_capacity);
    S.tail_records = static_cast<Record *>(d_tail_records);
    S.tail_series = static_cast<Entry *>(d_tail_series);
    S.tail_counts = static_cast<uint32_t *>(d_tail_counts);
    return S;
}

inline size_t union_workspace_bytes(size_t capacity_a, size_t capacity_b) { return UnionWorkspace(capacity_a, capacity_b).bytes; }

template <class T>
void series_union_device(int device, const void *d_a_records, const void *d_a_series, const void *d_a_counts, size_t capacity_a, const void *d_b_records,
                         const void *d_b_series, const void *d_b_counts, size_t capacity_b, void *d_out_records, void *d_out_series, void *d_out_counts,
                         size_t out_capacity, void *d_workspace, size_t workspace_bytes, hipStream_t stream)
{
    need_device(device, std::string("the ") + T::kName + " union's device path");
    const UnionDeviceArgs<T> U = union_args<T>(d_a_records, d_a_series, d_a_counts, capacity_a, d_b_records, d_b_series, d_b_counts, capacity_b, d_out_records,
                                               d_out_series, d_out_counts, out_capacity, d_workspace, workspace_bytes);
    DeviceGuard on_device(device);
    launched(launch_union(U, stream), std::string(T::kName) + " union");
}

template <class T>
void series_split_device(int device, const void *d_records, const void *d_series, const void *d_counts, size_t capacity, uint32_t last_frame, void *d_head_records,
                         void *d_head_series, void *d_head_counts, size_t head_capacity, void *d_tail_records, void *d_tail_series, void *d_tail_counts,
                         size_t tail_capacity, hipStream_t stream)
{
    need_device(device, std::string("the ") + T::kName + " split's device path");
    const SplitDeviceArgs<T> S = split_args<T>(d_records, d_series, d_counts, capacity, last_frame, d_head_records, d_head_series, d_head_counts, head_capacity,
                                               d_tail_records, d_tail_series, d_tail_counts, tail_capacity, false);
    DeviceGuard on_device(device);
    launched(launch_split(S, stream), std::string(T::kName) + " split");
}

// ---- the device store ----
// Two pairs of buffers: a union or a drain reads the current pair and writes the other.  event_ marks the last work issued on the
// store's buffers, on whichever stream; every call makes its stream wait for it before it touches them.
template <class T>
class DeviceFrameStoreOf final : public FrameStoreOf<T> {
public:
    using Record = typename T::Record;
    using Entry = typename T::Entry;

    DeviceFrameStoreOf(int device, size_t capacity) : device_(device), capacity_(capacity)
    {
        need_device(device, "a device " + store_);
        DeviceGuard on_device(device);
        for (int k = 0; k < 2; ++k) {
            records_[k].alloc(capacity, named("records").c_str());
            series_[k].alloc(capacity, named("table").c_str());
        }
        counts_.alloc(4u * 8u, named("counts").c_str());                        // two for the buffers, one of the bunch, one of a plan; eight words each
        workspace_bytes_ = union_workspace_bytes(capacity, capacity);
        workspace_.alloc(workspace_bytes_, named("workspace").c_str());
        sticky_.alloc(8u, named("counters").c_str());                           // page-locked: the device writes them, the host reads them without a copy
        std::memset(sticky_.get(), 0, 8u * sizeof(uint32_t));
        void *d = nullptr;
        hip_check(hipHostGetDevicePointer(&d, sticky_.get(), 0), "hipHostGetDevicePointer");
        d_sticky_ = static_cast<uint32_t *>(d);
        plan_.alloc(16u, named("plan").c_str());
        stream_.create(named("stream").c_str());
        event_.create_untimed(named("event").c_str());
        uploaded_.create_untimed(named("event").c_str());
        hip_check(hipMemsetAsync(counts_.get(), 0, 4u * 8u * sizeof(uint32_t), stream_.get()), "hipMemsetAsync");
        hip_check(hipEventRecord(event_.get(), stream_.get()), "hipEventRecord");
        hip_check(hipEventRecord(uploaded_.get(), stream_.get()), "hipEventRecord");
    }
    ~DeviceFrameStoreOf() override
    {
        DeviceGuard on_device(device_, std::nothrow);
        (void)hipEventSynchronize(event_.get());                        // nothing of the store's is in flight when its memory goes
    }
    bool on_device() const override { return true; }

    void add_host(const Record *records, size_t n, const Entry *series, size_t n_series) override
    {
        series_form_check<T>("the bunch", records, n, series, n_series);
        if (n > capacity_) throw Error(CLSIMHIP_ERR_ARGUMENT, store_ + ": a bunch of " + std::to_string(n) + " records does not fit a store of " + std::to_string(capacity_));
        std::lock_guard<std::mutex> lk(mutex_);
        DeviceGuard on_device(device_);
        if (!bunch_records_) {
            bunch_records_.alloc(capacity_, named("bunch").c_str());
            bunch_series_.alloc(capacity_, named("bunch").c_str());
            staged_records_.alloc(std::max<size_t>(capacity_, 1u), named("staging").c_str());
            staged_series_.alloc(std::max<size_t>(capacity_, 1u), named("staging").c_str());
            staged_counts_.alloc(8u, named("staging").c_str());
        }
        const std::string upload = std::string("upload ") + T::kName + " bunch";
        hip_check(hipEventSynchronize(uploaded_.get()), "hipEventSynchronize");         // the previous bunch has left the staging buffers
        if (n) std::memcpy(staged_records_.get(), records, n * sizeof(Record));
        if (n_series) std::memcpy(staged_series_.get(), series, n_series * sizeof(Entry));
        uint32_t *c = staged_counts_.get();
        c[0] = static_cast<uint32_t>(n); c[1] = static_cast<uint32_t>(n_series); c[2] = c[3] = c[4] = 0u;
        hipStream_t s = stream_.get();
        hip_check(hipStreamWaitEvent(s, event_.get(), 0), "hipStreamWaitEvent");        // (the previous union has read the bunch buffers)
        if (n) hip_check(hipMemcpyAsync(bunch_records_.get(), staged_records_.get(), n * sizeof(Record), hipMemcpyHostToDevice, s), upload.c_str());
        if (n_series) hip_check(hipMemcpyAsync(bunch_series_.get(), staged_series_.get(), n_series * sizeof(Entry), hipMemcpyHostToDevice, s), upload.c_str());
        hip_check(hipMemcpyAsync(counts_of(2), c, 5u * sizeof(uint32_t), hipMemcpyHostToDevice, s), upload.c_str());
        hip_check(hipEventRecord(uploaded_.get(), s), "hipEventRecord");
        fold(bunch_records_.get(), bunch_series_.get(), counts_of(2), capacity_, s);
    }

    void add_device(const void *d_records, const void *d_series, const void *d_series_counts, size_t capacity, hipStream_t stream) override
    {
        if (capacity > capacity_)
            throw Error(CLSIMHIP_ERR_ARGUMENT, store_ + ": a bunch buffer of " + std::to_string(capacity) + " records is beyond the store's capacity of " + std::to_string(capacity_));
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
        SplitDeviceArgs<T> S = split_args<T>(records_[current_].get(), series_[current_].get(), counts_of(current_), capacity_, last_frame, d_records, d_series, d_counts,
                                             capacity, records_[current_ ^ 1].get(), series_[current_ ^ 1].get(), counts_of(current_ ^ 1), capacity_, false);
        S.blocked = d_sticky_;
        hip_check(hipStreamWaitEvent(stream, event_.get(), 0), "hipStreamWaitEvent");
        launched(launch_split(S, stream), store_ + " drain");
        current_ ^= 1;
        hip_check(hipEventRecord(event_.get(), stream), "hipEventRecord");
    }

    void drain_host(uint32_t last_frame, Record *records, Entry *series, size_t capacity, size_t *n, size_t *n_series) override
    {
        std::lock_guard<std::mutex> lk(mutex_);
        DeviceGuard on_device(device_);
        size_t head = 0, entries = 0;
        const SplitDeviceArgs<T> S = plan(last_frame, &head, &entries);
        if (head > capacity || entries > capacity)
            throw Error(CLSIMHIP_ERR_ARGUMENT, store_ + ": the frames up to " + std::to_string(last_frame) + " hold " + std::to_string(head) + " records, the output " +
                                                   std::to_string(capacity));
        if ((head && !records) || (entries && !series)) throw Error(CLSIMHIP_ERR_ARGUMENT, "records / series is (null)");
        const std::string download = std::string("download ") + T::kName + " frames";
        hipStream_t s = stream_.get();
        if (head) hip_check(hipMemcpyAsync(records, records_[current_].get(), head * sizeof(Record), hipMemcpyDeviceToHost, s), download.c_str());
        if (entries) hip_check(hipMemcpyAsync(series, series_[current_].get(), entries * sizeof(Entry), hipMemcpyDeviceToHost, s), download.c_str());
        launched(launch_split_copy(S, s), store_ + " drain");           // the tail becomes the store; the head has gone to the host
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

    // what an allocation, a stream or an event of the store is called when HIP refuses it
    std::string named(const char *what) const { return store_ + " " + what; }

    void refuse_when_sticky() const
    {
        const volatile uint32_t *c = sticky_.get();
        const uint32_t v[5] = {c[0], c[1], c[2], c[3], c[4]};
        if ((v[0] | v[1] | v[2] | v[3] | v[4]) == 0u) return;
        throw Error(CLSIMHIP_ERR_DEVICE, store_ + ": data was dropped on the device and nothing is delivered -- " + std::to_string(v[FS_MALFORMED_BUNCHES]) +
                                             " malformed bunches (" + std::to_string(v[FS_MALFORMED_ELEMENTS]) + " malformed elements), " +
                                             std::to_string(v[FS_OVERFLOWED_BUNCHES]) + " bunches that did not fit (" + std::to_string(v[FS_OVERFLOWED_RECORDS]) + " records), " +
                                             std::to_string(v[FS_MALFORMED_STORE]) + " malformed elements in the store itself");
    }

    // the union of the store and a bunch into the other pair of buffers, behind the store's event on `stream` (the caller has made
    // the stream wait for it)
    void fold(const void *d_records, const void *d_series, const void *d_series_counts, size_t capacity, hipStream_t stream)
    {
        const int other = current_ ^ 1;
        const UnionDeviceArgs<T> U = union_args<T>(records_[current_].get(), series_[current_].get(), counts_of(current_), capacity_, d_records, d_series, d_series_counts,
                                                   capacity, records_[other].get(), series_[other].get(), counts_of(other), capacity_, workspace_.get(), workspace_bytes_);
        launched(launch_union(U, stream), store_ + " union");
        hipLaunchKernelGGL(store_note_kernel<T>, dim3(1), dim3(64), 0, stream, static_cast<const uint32_t *>(counts_of(other)), static_cast<const uint32_t *>(d_series_counts),
                           static_cast<uint32_t>(capacity), d_sticky_);
        launched(hipGetLastError(), store_ + " union");
        current_ = other;
        hip_check(hipEventRecord(event_.get(), stream), "hipEventRecord");
    }

    // waits for everything issued, refuses when data was dropped, and reads what a drain up to last_frame would take; the plan is
    // left in the counts of the other buffers, where the split copy kernel reads it
    SplitDeviceArgs<T> plan(uint32_t last_frame, size_t *head, size_t *entries)
    {
        hipStream_t s = stream_.get();
        hip_check(hipStreamWaitEvent(s, event_.get(), 0), "hipStreamWaitEvent");
        hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        refuse_when_sticky();
        SplitDeviceArgs<T> S = split_args<T>(records_[current_].get(), series_[current_].get(), counts_of(current_), capacity_, last_frame, nullptr, nullptr, counts_of(3),
                                             capacity_, records_[current_ ^ 1].get(), series_[current_ ^ 1].get(), counts_of(current_ ^ 1), capacity_, true);
        hipLaunchKernelGGL(split_plan_kernel<T>, dim3(1), dim3(64), 0, s, S);
        launched(hipGetLastError(), store_ + " plan");
        hip_check(hipMemcpyAsync(plan_.get(), counts_of(3), 5u * sizeof(uint32_t), hipMemcpyDeviceToHost, s), ("download " + store_ + " plan").c_str());
        hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        *head = plan_.get()[0];
        *entries = plan_.get()[1];
        return S;
    }

    const std::string store_ = T::kStore;
    int device_;
    size_t capacity_, workspace_bytes_ = 0;
    std::mutex mutex_;
    DeviceBuffer<Record> records_[2], bunch_records_;
    DeviceBuffer<Entry> series_[2], bunch_series_;
    DeviceBuffer<uint32_t> counts_;
    DeviceBuffer<uint8_t> workspace_;
    PinnedBuffer<uint32_t> sticky_, plan_, staged_counts_;
    PinnedBuffer<Record> staged_records_;
    PinnedBuffer<Entry> staged_series_;
    uint32_t *d_sticky_ = nullptr;
    Stream stream_;
    Event event_, uploaded_;
    int current_ = 0;
};

template <class T>
std::unique_ptr<FrameStoreOf<T>> make_device_frame_store_of(int device, size_t capacity)
{
    frame_store_capacity_check<T>(capacity);
    return std::unique_ptr<FrameStoreOf<T>>(new DeviceFrameStoreOf<T>(device, capacity));
}

} // namespace clsimhip
