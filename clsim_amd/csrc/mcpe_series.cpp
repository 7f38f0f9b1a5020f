// MCPE series (mcpe_series.h): what a bunch's particle table and mask become before any record is looked at, the host twin, and
// the host side of the device stage.  The kernels are in mcpe_series_kernel.hip.
#include "mcpe_series.h"

#include <algorithm>
#include <cstring>

#include "mcpe.h"

namespace clsimhip {

namespace {
size_t round16(size_t v) { return (v + 15u) & ~size_t{15}; }

// the workspace: header and histogram (zeroed together by every call), tile counts, two key buffers, the bunch's blob
struct SeriesWorkspace {
    size_t histogram, tile_counts, keys0, keys1, blob, bytes;
    SeriesWorkspace(size_t capacity, size_t blob_bytes)
    {
        const size_t tiles = std::max<size_t>((capacity + kSeriesTile - 1u) / kSeriesTile, 1u);
        histogram = kSeriesHeaderWords * sizeof(uint32_t);
        tile_counts = histogram + 16u * 256u * sizeof(uint32_t);
        keys0 = round16(tile_counts + 256u * tiles * sizeof(uint32_t));
        keys1 = keys0 + std::max<size_t>(capacity, 1u) * sizeof(SeriesKey);
        blob = keys1 + std::max<size_t>(capacity, 1u) * sizeof(SeriesKey);
        bytes = blob + round16(blob_bytes);
    }
};

bool key_less(const SeriesKey &a, const SeriesKey &b)
{
    if (a.group != b.group) return a.group < b.group;
    if (a.t_hi != b.t_hi) return a.t_hi < b.t_hi;
    if (a.t_lo != b.t_lo) return a.t_lo < b.t_lo;
    return a.identifier < b.identifier;
}
} // namespace

size_t mcpe_series_blob_bytes(size_t n_particles, size_t n_masked)
{
    return round16(n_particles * sizeof(SeriesParticle)) + round16(std::max<size_t>(n_particles, 1u) * sizeof(uint32_t)) + round16(n_masked * sizeof(uint32_t)) + 16u;
}

size_t mcpe_series_workspace_bytes(size_t capacity, size_t n_particles, size_t n_masked)
{
    return SeriesWorkspace(capacity, mcpe_series_blob_bytes(n_particles, n_masked)).bytes;
}

SeriesBunch McpeGenerator::prepare_series(const clsimhip_mcpe_particle *particles, size_t n_particles, const clsimhip_mcpe_mask *masked, size_t n_masked,
                                          uint8_t *blob) const
{
    if (n_particles && !particles) throw Error(CLSIMHIP_ERR_ARGUMENT, "particles is (null)");
    if (n_masked && !masked) throw Error(CLSIMHIP_ERR_ARGUMENT, "masked is (null)");
    if (!blob) throw Error(CLSIMHIP_ERR_ARGUMENT, "blob is (null)");
    if (n_particles > 0xffffffffull || n_masked > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "more than 2^32 - 1 particles or masked modules");
    SeriesBunch B;
    B.have_table = particles != nullptr;
    B.n_particles = static_cast<uint32_t>(n_particles);
    B.frames_offset = round16(n_particles * sizeof(SeriesParticle));
    B.masked_offset = B.frames_offset + round16(std::max<size_t>(n_particles, 1u) * sizeof(uint32_t));
    B.bytes = mcpe_series_blob_bytes(n_particles, n_masked);
    SeriesParticle *table = reinterpret_cast<SeriesParticle *>(blob);
    uint32_t *frames = reinterpret_cast<uint32_t *>(blob + B.frames_offset);
    uint32_t *groups = reinterpret_cast<uint32_t *>(blob + B.masked_offset);
    // frames: the distinct frame IDs, ascending; a table entry carries its frame's rank
    size_t n_frames = 1;
    frames[0] = 0u;
    if (n_particles > 0) {
        for (size_t i = 0; i < n_particles; ++i) {
            if (i > 0 && !(particles[i].identifier > particles[i - 1].identifier))
                throw Error(CLSIMHIP_ERR_ARGUMENT, "the particle table is not strictly increasing in identifier (entry " + std::to_string(i) + ")");
            frames[i] = particles[i].frame;
        }
        std::sort(frames, frames + n_particles);
        n_frames = static_cast<size_t>(std::unique(frames, frames + n_particles) - frames);
        for (size_t i = 0; i < n_particles; ++i) {
            table[i].identifier = particles[i].identifier;
            table[i].frame_rank = static_cast<uint32_t>(std::lower_bound(frames, frames + n_frames, particles[i].frame) - frames);
            table[i].time_shift = particles[i].time_shift;
        }
        B.consecutive = static_cast<uint64_t>(particles[n_particles - 1].identifier) - particles[0].identifier + 1u == n_particles;
    }
    const uint64_t n_doms = num_doms();
    if (static_cast<uint64_t>(n_frames) * std::max<uint64_t>(n_doms, 1u) >= (uint64_t{1} << 32))
        throw Error(CLSIMHIP_ERR_CONFIG, "MCPE series: " + std::to_string(n_frames) + " frames x " + std::to_string(n_doms) + " DOMs do not fit 32 bits");
    B.n_frames = static_cast<uint32_t>(n_frames);
    // mask: the groups it names, ascending and distinct; what names no frame of the table or no DOM of the generator is ignored
    size_t kept = 0;
    for (size_t i = 0; i < n_masked; ++i) {
        const uint32_t *f = std::lower_bound(frames, frames + n_frames, masked[i].frame);
        if (f == frames + n_frames || *f != masked[i].frame || (B.have_table && n_particles == 0)) continue;
        const uint32_t word = static_cast<uint32_t>(static_cast<uint16_t>(masked[i].string_id)) | (static_cast<uint32_t>(masked[i].om_id) << 16);
        const int64_t rank = series_dom_rank(dom_table_.data(), dom_ranks_.data(), params_.dom_mask, word);
        if (rank < 0) continue;
        groups[kept++] = static_cast<uint32_t>(f - frames) * static_cast<uint32_t>(n_doms) + static_cast<uint32_t>(rank);
    }
    std::sort(groups, groups + kept);
    B.n_masked = static_cast<uint32_t>(std::unique(groups, groups + kept) - groups);
    return B;
}

void McpeGenerator::series_host(const clsimhip_mcpe *in, size_t n, const clsimhip_mcpe_particle *particles, size_t n_particles,
                                const clsimhip_mcpe_mask *masked, size_t n_masked, clsimhip_mcpe *out, clsimhip_mcpe_series *series, size_t *n_kept,
                                size_t *n_series, uint64_t counters[3]) const
{
    if (n && (!in || !out || !series)) throw Error(CLSIMHIP_ERR_ARGUMENT, "mcpes / out / series is (null)");
    if (n > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "more than 2^32 - 1 records");
    std::vector<SeriesParticle> aligned((mcpe_series_blob_bytes(n_particles, n_masked) + sizeof(SeriesParticle) - 1u) / sizeof(SeriesParticle));
    uint8_t *blob = reinterpret_cast<uint8_t *>(aligned.data());
    const SeriesBunch B = prepare_series(particles, n_particles, masked, n_masked, blob);
    SeriesLookup L{};
    L.particles = B.have_table ? reinterpret_cast<const SeriesParticle *>(blob) : nullptr;
    L.masked_groups = reinterpret_cast<const uint32_t *>(blob + B.masked_offset);
    L.dom_table = dom_table_.data();
    L.dom_ranks = dom_ranks_.data();
    L.n_particles = B.n_particles; L.n_masked = B.n_masked; L.dom_mask = params_.dom_mask;
    L.n_doms = static_cast<uint32_t>(num_doms());
    L.consecutive = B.consecutive ? 1u : 0u;
    const uint32_t *frames = reinterpret_cast<const uint32_t *>(blob + B.frames_offset);
    std::vector<SeriesKey> keys;
    keys.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        SeriesKey k;
        const uint32_t word = static_cast<uint32_t>(static_cast<uint16_t>(in[i].string_id)) | (static_cast<uint32_t>(in[i].om_id) << 16);
        const int code = series_make_key(L, in[i].identifier, word, in[i].time, k);
        if (code == SERIES_KEPT) keys.push_back(k);
        else if (counters) ++counters[code];
    }
    std::sort(keys.begin(), keys.end(), key_less);
    size_t made = 0;
    for (size_t i = 0; i < keys.size(); ++i) {
        const SeriesKey &k = keys[i];
        const uint32_t frame_rank = k.group / L.n_doms;
        const uint32_t word = dom_of_rank_[k.group - frame_rank * L.n_doms];
        clsimhip_mcpe &m = out[i];
        m.identifier = k.identifier;
        m.string_id = static_cast<int16_t>(word & 0xffffu);
        m.om_id = static_cast<uint16_t>(word >> 16);
        m.time = series_time_of((static_cast<uint64_t>(k.t_hi) << 32) | k.t_lo);
        if (i == 0 || keys[i - 1].group != k.group) {
            clsimhip_mcpe_series &s = series[made++];
            s.frame = frames[frame_rank];
            s.string_id = m.string_id; s.om_id = m.om_id;
            s.first = static_cast<uint32_t>(i);
            s.count = 0u;
        }
        ++series[made - 1].count;
    }
    if (n_kept) *n_kept = keys.size();
    if (n_series) *n_series = made;
}

void McpeGenerator::series_device(int device, const void *d_mcpes, const void *d_count, size_t capacity, const clsimhip_mcpe_particle *particles,
                                  size_t n_particles, const clsimhip_mcpe_mask *masked, size_t n_masked, void *d_out, void *d_series, void *d_counts,
                                  void *d_workspace, size_t workspace_bytes, hipStream_t stream)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) throw Error(CLSIMHIP_ERR_DEVICE, "no HIP device available (the MCPE series' device path has no CPU fallback)");
    if (device < 0 || device >= count) throw Error(CLSIMHIP_ERR_ARGUMENT, "device ordinal out of range");
    DeviceGuard on_device(device);
    const size_t bytes = mcpe_series_blob_bytes(n_particles, n_masked);
    // one call at a time per generator and device prepares its bunch in the staging buffer: the previous call's copy has to be over
    std::lock_guard<std::mutex> lk(series_mutex_);
    SeriesStage &stage = stages_[device];
    if (stage.done.get()) hip_check(hipEventSynchronize(stage.done.get()), "MCPE series: previous upload");
    else stage.done.create_untimed("hipEventCreate");
    if (stage.bytes < bytes) {
        stage.buffer.reset();
        stage.buffer.alloc(bytes, "pinned MCPE series bunch");
        stage.bytes = bytes;
    }
    uint8_t *blob = stage.buffer.get();
    const SeriesBunch B = prepare_series(particles, n_particles, masked, n_masked, blob);
    // (the event is recorded right behind the copy, in front of the kernels: the next call waits for the copy, not for the stage)
    series_device_prepared(device, d_mcpes, d_count, capacity, B, blob, d_out, d_series, d_counts, d_workspace, workspace_bytes, stream, stage.done.get());
}

void McpeGenerator::series_device_prepared(int device, const void *d_mcpes, const void *d_count, size_t capacity, const SeriesBunch &B, const uint8_t *h_blob,
                                           void *d_out, void *d_series, void *d_counts, void *d_workspace, size_t workspace_bytes, hipStream_t stream,
                                           hipEvent_t uploaded)
{
    if (!d_count || !d_counts || !d_workspace) throw Error(CLSIMHIP_ERR_ARGUMENT, "device pointers are (null)");
    if (capacity && (!d_mcpes || !d_out || !d_series)) throw Error(CLSIMHIP_ERR_ARGUMENT, "d_mcpes / d_out / d_series is (null)");
    if (capacity > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "capacity beyond 2^32 - 1 records");
    if ((reinterpret_cast<uintptr_t>(d_mcpes) & 7u) || (reinterpret_cast<uintptr_t>(d_out) & 7u) || (reinterpret_cast<uintptr_t>(d_series) & 7u) ||
        (reinterpret_cast<uintptr_t>(d_workspace) & 15u) || (reinterpret_cast<uintptr_t>(d_counts) & 3u) || (reinterpret_cast<uintptr_t>(d_count) & 3u))
        throw Error(CLSIMHIP_ERR_ARGUMENT, "d_mcpes, d_out and d_series must be aligned to 8 bytes, d_workspace to 16, d_count and d_counts to 4");
    const SeriesWorkspace W(capacity, B.bytes);
    if (workspace_bytes < W.bytes) throw Error(CLSIMHIP_ERR_ARGUMENT, "the MCPE series workspace holds " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(W.bytes) + " are needed");
    DeviceGuard on_device(device);
    const DeviceImage im = image_on(device);
    uint8_t *ws = static_cast<uint8_t *>(d_workspace);
    hip_check(hipMemcpyAsync(ws + W.blob, h_blob, B.bytes, hipMemcpyHostToDevice, stream), "upload MCPE series bunch");
    if (uploaded) hip_check(hipEventRecord(uploaded, stream), "event");
    SeriesDeviceArgs A{};
    A.lookup.particles = B.have_table ? reinterpret_cast<const SeriesParticle *>(ws + W.blob) : nullptr;
    A.lookup.masked_groups = reinterpret_cast<const uint32_t *>(ws + W.blob + B.masked_offset);
    A.lookup.dom_table = im.dom_table;
    A.lookup.dom_ranks = im.dom_ranks;
    A.lookup.n_particles = B.n_particles; A.lookup.n_masked = B.n_masked; A.lookup.dom_mask = params_.dom_mask;
    A.lookup.n_doms = static_cast<uint32_t>(num_doms());
    A.lookup.consecutive = B.consecutive ? 1u : 0u;
    A.frames = reinterpret_cast<const uint32_t *>(ws + W.blob + B.frames_offset);
    A.dom_of_rank = im.dom_of_rank;
    A.in = static_cast<const clsimhip_mcpe *>(d_mcpes);
    A.in_count = static_cast<const uint32_t *>(d_count);
    A.capacity = static_cast<uint32_t>(capacity);
    A.header = reinterpret_cast<uint32_t *>(ws);
    A.histogram = reinterpret_cast<uint32_t *>(ws + W.histogram);
    A.tile_counts = reinterpret_cast<uint32_t *>(ws + W.tile_counts);
    A.keys[0] = reinterpret_cast<SeriesKey *>(ws + W.keys0);
    A.keys[1] = reinterpret_cast<SeriesKey *>(ws + W.keys1);
    A.out = static_cast<clsimhip_mcpe *>(d_out);
    A.series = static_cast<clsimhip_mcpe_series *>(d_series);
    A.counts = static_cast<uint32_t *>(d_counts);
    const hipError_t e = launch_mcpe_series(A, stream);
    if (e != hipSuccess) throw Error(CLSIMHIP_ERR_DEVICE, std::string("MCPE series kernel launch: ") + hipGetErrorString(e));
}

} // namespace clsimhip
