// Series relabel on the device: the definition of series_relabel.h for gfx950 (wave64), one template over the two record types, and
// its host side (workspace, the map's staging, argument checks, launches).
//
//   relabel_copy_kernel    a fixed grid of workgroups, each walking tiles of 2048 records (256 lanes x 8, lane-strided so that a wave's
//                          loads and stores are contiguous).  The map's upper levels -- 256 pivots, every pivot_stride-th `from` -- are
//                          read into LDS once per workgroup; a record bisects them there and the stretch below its pivot in HBM.  Per
//                          record: one load, the lookup, one store with the new identifier; its predecessor's first 16 bytes (a cache
//                          hit) say whether it opens a run, and only a record that does not looks further: its predecessor's new
//                          identifier and content, for "descends".  Run heads are counted per tile, descents and RELABELLED in the header.
//                          The series table is copied by the same lanes.
//   launch_series_tile_scan  the series stage's scan over the heads per tile: where each tile's runs start, and how many runs there are.
//   relabel_runs_kernel    only with a descent anywhere (else every workgroup returns at once, as in the two below): per tile, every
//                          record's run by a scan over the head flags; heads write run_first, descents mark their run.
//   relabel_sort_kernel    a fixed grid walks the runs 256 at a time; a marked run of at most 2048 records is sorted by one workgroup:
//                          new identifiers (and h) in LDS, 16 KiB, every member ranked by counting the members that go in front of it
//                          (ties in (identifier, h) compare the contents in HBM; equal keys are equal bytes, the source index breaks
//                          them), then each record moves once, from the input to its place.  A longer one adds its length to TIE_OVERFLOW.
//   relabel_close_kernel   the five output counts.
//
// Everything reads its sizes from device memory: nothing waits for the host.  Atomics only count and mark.  Every loop is bounded by a
// capacity and every index is clamped to one, whatever bytes the inputs hold.
#include "series_relabel.h"

#include <cstring>
#include <mutex>
#include <string>

#include "hip_resources.h"
#include "series_bunch.h"

namespace clsimhip {

namespace {

__device__ __forceinline__ uint32_t min_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }

constexpr uint32_t kRounds = kSeriesTile / 256u;                        // 8 records per lane and tile

template <uint32_t kWords>
__device__ __forceinline__ void load_words(const void *records, uint32_t i, uint32_t (&w)[kWords])
{
    const uint4 *p = reinterpret_cast<const uint4 *>(records) + (size_t)i * (kWords / 4u);
#pragma unroll
    for (uint32_t q = 0; q < kWords / 4u; ++q) {
        const uint4 v = p[q];
        w[4u * q] = v.x; w[4u * q + 1u] = v.y; w[4u * q + 2u] = v.z; w[4u * q + 3u] = v.w;
    }
}

template <uint32_t kWords>
__device__ __forceinline__ void store_words(void *records, uint32_t i, const uint32_t (&w)[kWords])
{
    uint4 *p = reinterpret_cast<uint4 *>(records) + (size_t)i * (kWords / 4u);
#pragma unroll
    for (uint32_t q = 0; q < kWords / 4u; ++q) p[q] = make_uint4(w[4u * q], w[4u * q + 1u], w[4u * q + 2u], w[4u * q + 3u]);
}

// the map's entry for `identifier`, or -1: the pivots in LDS, then at most pivot_stride entries in HBM
__device__ __forceinline__ int64_t lookup(const clsimhip_relabel *map, uint32_t n_map, uint32_t stride, const uint32_t *pivots, uint32_t n_pivots, uint32_t identifier)
{
    uint32_t lo = 0u, hi = n_pivots;                                    // first pivot > identifier
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (pivots[mid] <= identifier) lo = mid + 1u; else hi = mid;
    }
    if (lo == 0u) return -1;
    const uint32_t from = (lo - 1u) * stride;                           // < n_map
    const uint64_t to = (uint64_t)from + stride;
    return relabel_find(map, from, to < n_map ? (uint32_t)to : n_map, identifier);
}

__device__ __forceinline__ uint32_t load_pivots(const clsimhip_relabel *map, uint32_t n_map, uint32_t stride, uint32_t *pivots)
{
    const uint32_t n_pivots = stride == 0u ? 0u : min_u32((uint32_t)(((uint64_t)n_map + stride - 1u) / stride), kRelabelPivots);
    for (uint32_t k = threadIdx.x; k < n_pivots; k += blockDim.x) pivots[k] = map[(size_t)k * stride].from;     // k x stride < n_map
    __syncthreads();
    return n_pivots;
}

template <class T>
__global__ void __launch_bounds__(256) relabel_copy_kernel(const RelabelDeviceArgs<T> A)
{
    __shared__ uint32_t pivots[kRelabelPivots];
    __shared__ uint32_t wave_heads[4];
    const uint32_t n = min_u32(A.counts[0], A.capacity), n_series = min_u32(A.counts[1], A.capacity);
    if (blockIdx.x == 0u && threadIdx.x == 0u) { A.header[SH_KEPT] = n; A.header[RH_N_SERIES] = n_series; }
    for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < n_series; s += (uint64_t)gridDim.x * 256u) A.out_series[s] = A.series[s];     // s < capacity
    const uint32_t n_pivots = load_pivots(A.map, A.n_map, A.pivot_stride, pivots);
    const uint32_t tiles = (uint32_t)(((uint64_t)n + kSeriesTile - 1u) / kSeriesTile);
    uint32_t relabelled = 0u, descents = 0u;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        uint32_t heads = 0u;
#pragma unroll 2
        for (uint32_t r = 0; r < kRounds; ++r) {
            const uint64_t at = (uint64_t)tile * kSeriesTile + r * 256u + threadIdx.x;
            if (at >= n) continue;
            const uint32_t i = (uint32_t)at;
            uint32_t rec[T::kWords], before[4] = {0u, 0u, 0u, 0u};
            load_words<T::kWords>(A.records, i, rec);
            if (i > 0u) {
                const uint4 v = reinterpret_cast<const uint4 *>(A.records + (i - 1u))[0];
                before[0] = v.x; before[1] = v.y; before[2] = v.z; before[3] = v.w;
            }
            const int64_t k = lookup(A.map, A.n_map, A.pivot_stride, pivots, n_pivots, rec[0]);
            if (k >= 0) { rec[0] = A.map[k].to; ++relabelled; }
            if (relabel_is_head(rec, before, A.series, n_series, i)) {
                ++heads;
            } else {                                                    // rare: equal times at one DOM
                uint32_t full[T::kWords];
                load_words<T::kWords>(A.records, i - 1u, full);
                const int64_t kb = lookup(A.map, A.n_map, A.pivot_stride, pivots, n_pivots, full[0]);
                const uint32_t id_before = kb >= 0 ? A.map[kb].to : full[0];
                if (T::rest_less(rec[0], rec, id_before, full)) ++descents;
            }
            store_words<T::kWords>(A.out_records, i, rec);                // i < n <= capacity
        }
        // the tile's heads: a sum over the workgroup
        for (uint32_t step = 32u; step > 0u; step >>= 1) heads += __shfl_down(heads, step);
        if ((threadIdx.x & 63u) == 0u) wave_heads[threadIdx.x >> 6] = heads;
        __syncthreads();
        if (threadIdx.x == 0u) A.tile_counts[tile] = wave_heads[0] + wave_heads[1] + wave_heads[2] + wave_heads[3];     // tile < tiles(capacity)
        __syncthreads();
    }
    if (relabelled != 0u) atomicAdd(A.header + RH_RELABELLED, relabelled);
    if (descents != 0u) atomicAdd(A.header + RH_DESCENTS, descents);
}

template <class T>
__global__ void __launch_bounds__(256) relabel_runs_kernel(const RelabelDeviceArgs<T> A)
{
    if (A.header[RH_DESCENTS] == 0u) return;
    __shared__ uint32_t lane_heads[256];
    const uint32_t n = A.header[SH_KEPT], n_series = A.header[RH_N_SERIES];
    const uint32_t n_runs = min_u32(A.header[SH_SERIES], n);
    const uint64_t base = (uint64_t)blockIdx.x * kSeriesTile + (uint64_t)threadIdx.x * kRounds;      // a lane's 8 records are neighbours
    if ((uint64_t)blockIdx.x * kSeriesTile >= n) return;
    // the records as the copy kernel wrote them: in the input's order, with their new identifiers
    uint32_t head_bits = 0u, descent_bits = 0u;
    for (uint32_t r = 0; r < kRounds; ++r) {
        if (base + r >= n) break;
        const uint32_t i = (uint32_t)(base + r);
        uint32_t rec[T::kWords], before[T::kWords];
        load_words<T::kWords>(A.out_records, i, rec);
        if (i > 0u) load_words<T::kWords>(A.out_records, i - 1u, before);
        else for (uint32_t k = 0; k < T::kWords; ++k) before[k] = 0u;
        if (relabel_is_head(rec, before, A.series, n_series, i)) head_bits |= 1u << r;
        else if (T::rest_less(rec[0], rec, before[0], before)) descent_bits |= 1u << r;
    }
    lane_heads[threadIdx.x] = __popc(head_bits);
    __syncthreads();
    uint32_t run = A.tile_counts[blockIdx.x];                           // the heads in front of this tile ...
    for (uint32_t t = 0; t < threadIdx.x; ++t) run += lane_heads[t];    // ... and in front of this lane
    for (uint32_t r = 0; r < kRounds; ++r) {
        if (base + r >= n) break;
        if (head_bits & (1u << r)) {
            if (run < n_runs) A.run_first[run] = (uint32_t)(base + r);  // n_runs <= n <= capacity
            ++run;
        } else if ((descent_bits & (1u << r)) && run >= 1u && run - 1u < n_runs) {
            atomicOr(A.run_disturbed + (run - 1u), 1u);
        }
    }
}

template <class T>
__global__ void __launch_bounds__(256) relabel_clear_kernel(const RelabelDeviceArgs<T> A)
{
    if (A.header[RH_DESCENTS] == 0u) return;
    const uint32_t n = A.header[SH_KEPT];
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) A.run_disturbed[i] = 0u;
}

template <class T>
__global__ void __launch_bounds__(256) relabel_sort_kernel(const RelabelDeviceArgs<T> A)
{
    if (A.header[RH_DESCENTS] == 0u) return;
    __shared__ uint32_t ids[kRelabelRunBound], mixes[kRelabelRunBound];
    __shared__ uint32_t marked[256];
    __shared__ uint32_t n_marked;
    const uint32_t n = A.header[SH_KEPT];
    const uint32_t n_runs = min_u32(A.header[SH_SERIES], n);
    for (uint64_t chunk = (uint64_t)blockIdx.x * 256u; chunk < n_runs; chunk += (uint64_t)gridDim.x * 256u) {
        if (threadIdx.x == 0u) n_marked = 0u;
        __syncthreads();
        const uint64_t mine = chunk + threadIdx.x;
        if (mine < n_runs && A.run_disturbed[mine] != 0u) marked[atomicAdd(&n_marked, 1u)] = (uint32_t)mine;     // at most 256
        __syncthreads();
        const uint32_t listed = n_marked;
        for (uint32_t m = 0; m < listed; ++m) {
            const uint32_t run = marked[m];
            const uint32_t first = min_u32(A.run_first[run], n);
            const uint32_t end = run + 1u < n_runs ? min_u32(A.run_first[run + 1u], n) : n;
            const uint32_t len = end > first ? end - first : 0u;
            if (len > kRelabelRunBound) {
                if (threadIdx.x == 0u) atomicAdd(A.header + RH_TIE_OVERFLOW, len);
                continue;
            }
            for (uint32_t e = threadIdx.x; e < len; e += 256u) {
                uint32_t rec[T::kWords];
                load_words<T::kWords>(A.out_records, first + e, rec);   // (still in the input's order)
                ids[e] = rec[0];
                if (T::kWords > 4u) {
                    FramePhotonContent c;
#pragma unroll
                    for (uint32_t k = 0; k < 8u; ++k) c.w[k] = rec[(4u + k) % T::kWords];
                    mixes[e] = frame_photons_mix(c);
                }
            }
            __syncthreads();
            uint32_t rank[kRounds];
#pragma unroll
            for (uint32_t r = 0; r < kRounds; ++r) {
                const uint32_t e = r * 256u + threadIdx.x;
                rank[r] = 0u;
                if (e >= len) continue;
                const uint32_t id = ids[e], mix = T::kWords > 4u ? mixes[e] : 0u;
                uint32_t in_front = 0u;
                for (uint32_t j = 0; j < len; ++j) {
                    const uint32_t id_j = ids[j];
                    bool front;                                         // member j goes in front of member e
                    if (id_j != id) front = id_j < id;
                    else if (T::kWords == 4u) front = j < e;
                    else if (mixes[j] != mix) front = mixes[j] < mix;
                    else {                                              // rare: the contents decide, then the source index
                        const uint32_t *a = reinterpret_cast<const uint32_t *>(A.records + (first + j)), *b = reinterpret_cast<const uint32_t *>(A.records + (first + e));
                        int c = 0;
                        for (uint32_t k = 4u; k < T::kWords && c == 0; ++k) c = a[k] != b[k] ? (a[k] < b[k] ? -1 : 1) : 0;
                        front = c != 0 ? c < 0 : j < e;
                    }
                    in_front += front ? 1u : 0u;
                }
                rank[r] = in_front;                                     // < len: a permutation of the run
            }
            __syncthreads();                                            // (every read of out_records in this run is over)
#pragma unroll
            for (uint32_t r = 0; r < kRounds; ++r) {
                const uint32_t e = r * 256u + threadIdx.x;
                if (e >= len) continue;
                uint32_t rec[T::kWords];
                load_words<T::kWords>(A.records, first + e, rec);
                rec[0] = ids[e];
                store_words<T::kWords>(A.out_records, first + min_u32(rank[r], len - 1u), rec);      // < end <= n <= capacity
            }
            __syncthreads();                                            // (ids and mixes are written again for the next run)
        }
        __syncthreads();
    }
}

template <class T>
__global__ void __launch_bounds__(64) relabel_close_kernel(const RelabelDeviceArgs<T> A)
{
    if (threadIdx.x != 0u) return;
    const uint32_t overflow = A.header[RH_TIE_OVERFLOW];
    A.out_counts[0] = overflow ? 0u : A.header[SH_KEPT];
    A.out_counts[1] = overflow ? 0u : A.header[RH_N_SERIES];
    A.out_counts[2] = A.header[RH_RELABELLED];
    A.out_counts[3] = 0u;
    A.out_counts[4] = overflow;
}

uint32_t tiles_of(uint64_t records)
{
    const uint64_t tiles = (records + kSeriesTile - 1u) / kSeriesTile;
    return tiles == 0u ? 1u : (uint32_t)tiles;
}

// the workspace: header, heads per tile, then one word per record (and one more) for the runs' starts, one per record for their marks,
// and the map
struct RelabelWorkspace {
    size_t tile_counts, run_first, run_disturbed, map, bytes;
    RelabelWorkspace(size_t capacity, size_t n_map)
    {
        tile_counts = kSeriesHeaderWords * sizeof(uint32_t);
        run_first = tile_counts + round16(tiles_of(capacity) * sizeof(uint32_t));
        run_disturbed = run_first + round16((capacity + 1u) * sizeof(uint32_t));
        map = run_disturbed + round16(std::max<size_t>(capacity, 1u) * sizeof(uint32_t));
        bytes = map + round16(std::max<size_t>(n_map, 1u) * sizeof(clsimhip_relabel));
    }
};

template <class T>
hipError_t launch_relabel(const RelabelDeviceArgs<T> &A, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(A.header, 0, kSeriesHeaderWords * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const uint32_t tiles = tiles_of(A.capacity);
    const uint32_t walkers = std::min<uint32_t>(tiles, 2048u);          // 8 workgroups per CU: the pivots are read once per workgroup
    SeriesDeviceArgs S{};                                               // what the series stage's tile scan reads
    S.capacity = A.capacity;
    S.header = A.header;
    S.tile_counts = A.tile_counts;
    hipLaunchKernelGGL(relabel_copy_kernel<T>, dim3(walkers), dim3(256), 0, stream, A);
    launch_series_tile_scan(S, stream);
    hipLaunchKernelGGL(relabel_clear_kernel<T>, dim3(std::min<uint32_t>(tiles, 1024u)), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(relabel_runs_kernel<T>, dim3(tiles), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(relabel_sort_kernel<T>, dim3(std::min<uint32_t>(tiles, 1024u)), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(relabel_close_kernel<T>, dim3(1), dim3(64), 0, stream, A);
    return hipGetLastError();
}

// Page-locked staging of the map (series_bunch.h), one buffer per device, for the life of the process: the calls have no object of their
// own to keep it in, and a static's destructor would run behind the HIP runtime's.
std::mutex g_call_mutex, g_map_mutex;
SeriesStaging &staging()
{
    static SeriesStaging *s = new SeriesStaging(&g_map_mutex);
    return *s;
}

uintptr_t at(const void *p) { return reinterpret_cast<uintptr_t>(p); }

template <class T>
void relabel_device(const char *stage, int device, const void *d_records, const void *d_series, const void *d_counts, size_t capacity, const clsimhip_relabel *map,
                    size_t n_map, void *d_out_records, void *d_out_series, void *d_out_counts, void *d_workspace, size_t workspace_bytes, hipStream_t stream)
{
    using Record = typename T::Record;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) throw Error(CLSIMHIP_ERR_DEVICE, std::string("no HIP device available (") + stage + " has no CPU fallback)");
    if (device < 0 || device >= count) throw Error(CLSIMHIP_ERR_ARGUMENT, "device ordinal out of range");
    if (!d_counts || !d_out_counts || !d_workspace) throw Error(CLSIMHIP_ERR_ARGUMENT, "device pointers are (null)");
    if (capacity && (!d_records || !d_series || !d_out_records || !d_out_series)) throw Error(CLSIMHIP_ERR_ARGUMENT, "d_records / d_series / d_out_records / d_out_series is (null)");
    if (capacity > kFrameStoreMaxCapacity) throw Error(CLSIMHIP_ERR_ARGUMENT, "series relabel: capacity beyond 2^31 records");
    if ((at(d_records) & 15u) || (at(d_series) & 15u) || (at(d_out_records) & 15u) || (at(d_out_series) & 15u) || (at(d_workspace) & 15u) || (at(d_counts) & 3u) ||
        (at(d_out_counts) & 3u))
        throw Error(CLSIMHIP_ERR_ARGUMENT, "records, series tables and d_workspace must be aligned to 16 bytes, the counts to 4");
    const auto overlap = [](const void *a, size_t a_bytes, const void *b, size_t b_bytes) { return a_bytes && b_bytes && at(a) < at(b) + b_bytes && at(b) < at(a) + a_bytes; };
    if (overlap(d_records, capacity * sizeof(Record), d_out_records, capacity * sizeof(Record)) ||
        overlap(d_series, capacity * sizeof(clsimhip_mcpe_series), d_out_series, capacity * sizeof(clsimhip_mcpe_series)))
        throw Error(CLSIMHIP_ERR_ARGUMENT, "series relabel: the output must not overlap the input");
    relabel_map_check(map, n_map);
    const RelabelWorkspace W(capacity, n_map);
    if (workspace_bytes < W.bytes)
        throw Error(CLSIMHIP_ERR_ARGUMENT, "the series relabel workspace holds " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(W.bytes) + " are needed");
    uint8_t *ws = static_cast<uint8_t *>(d_workspace);
    RelabelDeviceArgs<T> A{};
    A.records = static_cast<const Record *>(d_records);
    A.series = static_cast<const clsimhip_mcpe_series *>(d_series);
    A.counts = static_cast<const uint32_t *>(d_counts);
    A.capacity = static_cast<uint32_t>(capacity);
    A.map = reinterpret_cast<const clsimhip_relabel *>(ws + W.map);
    A.n_map = static_cast<uint32_t>(n_map);
    A.pivot_stride = static_cast<uint32_t>((n_map + kRelabelPivots - 1u) / kRelabelPivots);
    A.header = reinterpret_cast<uint32_t *>(ws);
    A.tile_counts = reinterpret_cast<uint32_t *>(ws + W.tile_counts);
    A.run_first = reinterpret_cast<uint32_t *>(ws + W.run_first);
    A.run_disturbed = reinterpret_cast<uint32_t *>(ws + W.run_disturbed);
    A.out_records = static_cast<Record *>(d_out_records);
    A.out_series = static_cast<clsimhip_mcpe_series *>(d_out_series);
    A.out_counts = static_cast<uint32_t *>(d_out_counts);
    DeviceGuard on_device(device);
    std::lock_guard<std::mutex> one_call(g_call_mutex);
    if (n_map) {                                                        // copied before the call returns; the upload is asynchronous
        uint8_t *pinned = staging().acquire(device, n_map * sizeof(clsimhip_relabel), stage);
        std::memcpy(pinned, map, n_map * sizeof(clsimhip_relabel));
        hip_check(hipMemcpyAsync(ws + W.map, pinned, n_map * sizeof(clsimhip_relabel), hipMemcpyHostToDevice, stream), "hipMemcpyAsync (relabel map)");
        hip_check(hipEventRecord(staging().done(device), stream), "hipEventRecord (relabel map)");
    }
    const hipError_t e = launch_relabel(A, stream);
    if (e != hipSuccess) throw Error(CLSIMHIP_ERR_DEVICE, std::string(stage) + " kernel launch: " + hipGetErrorString(e));
}

} // namespace

size_t series_relabel_workspace_bytes(size_t capacity, size_t n_map, size_t record_bytes)
{
    if (record_bytes != sizeof(clsimhip_mcpe) && record_bytes != sizeof(clsimhip_frame_photon)) return 0u;
    return RelabelWorkspace(capacity, n_map).bytes;
}

void mcpe_series_relabel_device(int device, const void *d_records, const void *d_series, const void *d_counts, size_t capacity, const clsimhip_relabel *map, size_t n_map,
                                void *d_out_records, void *d_out_series, void *d_out_counts, void *d_workspace, size_t workspace_bytes, hipStream_t stream)
{
    relabel_device<RelabelMcpe>("the MCPE series relabel's device path", device, d_records, d_series, d_counts, capacity, map, n_map, d_out_records, d_out_series,
                                d_out_counts, d_workspace, workspace_bytes, stream);
}

void frame_photons_relabel_device(int device, const void *d_records, const void *d_series, const void *d_counts, size_t capacity, const clsimhip_relabel *map, size_t n_map,
                                  void *d_out_records, void *d_out_series, void *d_out_counts, void *d_workspace, size_t workspace_bytes, hipStream_t stream)
{
    relabel_device<RelabelFramePhoton>("the frame photons relabel's device path", device, d_records, d_series, d_counts, capacity, map, n_map, d_out_records,
                                       d_out_series, d_out_counts, d_workspace, workspace_bytes, stream);
}

} // namespace clsimhip
