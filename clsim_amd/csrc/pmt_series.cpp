// PMT series (pmt_series.h): the generator's rank and channel tables, what a bunch's particle table and mask become before any
// record is looked at, the host twin, and the host side of the device stage.  The kernels are in pmt_series_kernel.hip.
#include "pmt_series.h"

#include <algorithm>
#include <cstring>

namespace clsimhip {

namespace {
size_t round16(size_t v) { return (v + 15u) & ~size_t{15}; }

// the workspace: header and histogram (zeroed together by every call), tile counts, two key buffers, the bunch's blob
struct PmtSeriesWorkspace {
    size_t histogram, tile_counts, keys0, keys1, blob, bytes;
    PmtSeriesWorkspace(size_t capacity, size_t blob_bytes)
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

uint32_t record_word(int16_t string_id, uint16_t om_id) { return static_cast<uint32_t>(static_cast<uint16_t>(string_id)) | (static_cast<uint32_t>(om_id) << 16); }
} // namespace

// (the blob has the MCPE series' layout: table, frame IDs by rank, masked keys)
size_t pmt_series_blob_bytes(size_t n_particles, size_t n_masked)
{
    return round16(n_particles * sizeof(SeriesParticle)) + round16(std::max<size_t>(n_particles, 1u) * sizeof(uint32_t)) + round16(n_masked * sizeof(uint32_t)) + 16u;
}

size_t pmt_series_workspace_bytes(size_t capacity, size_t n_particles, size_t n_masked)
{
    return PmtSeriesWorkspace(capacity, pmt_series_blob_bytes(n_particles, n_masked)).bytes;
}

SeriesBunch PmtHitGenerator::prepare_series(const clsimhip_mcpe_particle *particles, size_t n_particles, const clsimhip_mcpe_mask *masked, size_t n_masked,
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
    B.bytes = pmt_series_blob_bytes(n_particles, n_masked);
    SeriesParticle *table = reinterpret_cast<SeriesParticle *>(blob);
    uint32_t *frames = reinterpret_cast<uint32_t *>(blob + B.frames_offset);
    uint32_t *keys = reinterpret_cast<uint32_t *>(blob + B.masked_offset);
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
    const uint64_t n_channels = num_channels();
    if (static_cast<uint64_t>(n_frames) * std::max<uint64_t>(n_channels, 1u) >= (uint64_t{1} << 32))
        throw Error(CLSIMHIP_ERR_CONFIG, "PMT series: " + std::to_string(n_frames) + " frames x " + std::to_string(n_channels) + " channels do not fit 32 bits");
    B.n_frames = static_cast<uint32_t>(n_frames);
    // mask: the (frame, module) pairs it names, ascending and distinct; what names no frame of the table or no module of the
    // generator is ignored
    size_t kept = 0;
    for (size_t i = 0; i < n_masked; ++i) {
        const uint32_t *f = std::lower_bound(frames, frames + n_frames, masked[i].frame);
        if (f == frames + n_frames || *f != masked[i].frame || (B.have_table && n_particles == 0)) continue;
        const int64_t slot = pmt_series_module_slot(module_table_.data(), params_.module_mask, record_word(masked[i].string_id, masked[i].om_id));
        if (slot < 0) continue;
        keys[kept++] = static_cast<uint32_t>(f - frames) * static_cast<uint32_t>(num_modules()) + module_ranks_[slot];
    }
    std::sort(keys, keys + kept);
    B.n_masked = static_cast<uint32_t>(std::unique(keys, keys + kept) - keys);
    return B;
}

void PmtHitGenerator::series_host(const clsimhip_pmt_hit *in, size_t n, const clsimhip_mcpe_particle *particles, size_t n_particles,
                                  const clsimhip_mcpe_mask *masked, size_t n_masked, clsimhip_pmt_hit *out, clsimhip_pmt_series *series, size_t *n_kept,
                                  size_t *n_series, uint64_t counters[3]) const
{
    if (n && (!in || !out || !series)) throw Error(CLSIMHIP_ERR_ARGUMENT, "hits / out / series is (null)");
    if (n > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "more than 2^32 - 1 records");
    std::vector<SeriesParticle> aligned((pmt_series_blob_bytes(n_particles, n_masked) + sizeof(SeriesParticle) - 1u) / sizeof(SeriesParticle));
    uint8_t *blob = reinterpret_cast<uint8_t *>(aligned.data());
    const SeriesBunch B = prepare_series(particles, n_particles, masked, n_masked, blob);
    PmtSeriesLookup L{};
    L.particles = B.have_table ? reinterpret_cast<const SeriesParticle *>(blob) : nullptr;
    L.masked_modules = reinterpret_cast<const uint32_t *>(blob + B.masked_offset);
    L.module_table = module_table_.data();
    L.module_ranks = module_ranks_.data();
    L.channel_bases = channel_bases_.data();
    L.base = base_.data();
    L.n_particles = B.n_particles; L.n_masked = B.n_masked; L.module_mask = params_.module_mask;
    L.n_modules = static_cast<uint32_t>(num_modules());
    L.n_channels = static_cast<uint32_t>(num_channels());
    L.consecutive = B.consecutive ? 1u : 0u;
    const uint32_t *frames = reinterpret_cast<const uint32_t *>(blob + B.frames_offset);
    std::vector<SeriesKey> keys;
    keys.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        SeriesKey k;
        const int code = pmt_series_make_key(L, in[i].identifier, record_word(in[i].string_id, in[i].om_id), in[i].pmt, in[i].time, k);
        if (code == PMT_SERIES_KEPT) keys.push_back(k);
        else if (counters) ++counters[code];
    }
    std::sort(keys.begin(), keys.end(), key_less);
    size_t made = 0;
    for (size_t i = 0; i < keys.size(); ++i) {
        const SeriesKey &k = keys[i];
        const uint32_t frame_rank = k.group / L.n_channels;
        const uint32_t channel = k.group - frame_rank * L.n_channels;
        const uint32_t rank = pmt_series_rank_of_channel(L.base, L.n_modules, channel);
        const uint32_t word = module_of_rank_[rank];
        clsimhip_pmt_hit &h = out[i];
        h.identifier = k.identifier;
        h.string_id = static_cast<int16_t>(word & 0xffffu);
        h.om_id = static_cast<uint16_t>(word >> 16);
        h.pmt = channel - L.base[rank];
        h.reserved = 0u;
        h.time = series_time_of((static_cast<uint64_t>(k.t_hi) << 32) | k.t_lo);
        if (i == 0 || keys[i - 1].group != k.group) {
            clsimhip_pmt_series &s = series[made++];
            s.frame = frames[frame_rank];
            s.string_id = h.string_id; s.om_id = h.om_id;
            s.pmt = h.pmt;
            s.first = static_cast<uint32_t>(i);
            s.count = 0u;
            s.reserved = 0u;
        }
        ++series[made - 1].count;
    }
    if (n_kept) *n_kept = keys.size();
    if (n_series) *n_series = made;
}

// page-locked staging of the stand-alone series call's bunch, one per device, reused once its upload has been passed
struct PmtSeriesStage { Event done; PinnedBuffer<uint8_t> buffer; size_t bytes = 0; };

struct PmtHitGenerator::SeriesState {
    std::map<int, SeriesImage> images;
    std::map<int, PmtSeriesStage> stages;
    ~SeriesState()
    {
        for (auto &kv : images) {
            DeviceGuard on_device(kv.first, std::nothrow);
            DeviceBuffer<uint32_t> ranks(kv.second.module_ranks), bases(kv.second.channel_bases), base(kv.second.base), of_rank(kv.second.module_of_rank);
        }
        // (a stage exists from the first series call on a device on, whether or not that call got as far as the device's image)
        for (auto &kv : stages) {
            DeviceGuard on_device(kv.first, std::nothrow);
            kv.second = PmtSeriesStage();
        }
    }
};

PmtHitGenerator::SeriesState &PmtHitGenerator::series_state()
{
    if (!series_state_) series_state_ = std::make_shared<SeriesState>();
    return *series_state_;
}

PmtHitGenerator::SeriesImage PmtHitGenerator::series_image_on(int device)
{
    std::lock_guard<std::mutex> lk(device_mutex_);
    SeriesState &state = series_state();
    auto it = state.images.find(device);
    if (it != state.images.end()) return it->second;
    DeviceBuffer<uint32_t> ranks(module_ranks_.size(), "PMT module ranks"), bases(channel_bases_.size(), "PMT channel bases");
    DeviceBuffer<uint32_t> base(base_.size(), "PMT channels by module rank"), of_rank(std::max<size_t>(module_of_rank_.size(), 1u), "PMT modules by rank");
    hip_check(hipMemcpy(ranks.get(), module_ranks_.data(), module_ranks_.size() * sizeof(uint32_t), hipMemcpyHostToDevice), "PMT module ranks");
    hip_check(hipMemcpy(bases.get(), channel_bases_.data(), channel_bases_.size() * sizeof(uint32_t), hipMemcpyHostToDevice), "PMT channel bases");
    hip_check(hipMemcpy(base.get(), base_.data(), base_.size() * sizeof(uint32_t), hipMemcpyHostToDevice), "PMT channels by module rank");
    if (!module_of_rank_.empty())
        hip_check(hipMemcpy(of_rank.get(), module_of_rank_.data(), module_of_rank_.size() * sizeof(uint32_t), hipMemcpyHostToDevice), "PMT modules by rank");
    const SeriesImage im{ranks.release(), bases.release(), base.release(), of_rank.release()};
    state.images[device] = im;
    return im;
}

void PmtHitGenerator::series_device(int device, const void *d_hits, const void *d_count, size_t capacity, const clsimhip_mcpe_particle *particles,
                                    size_t n_particles, const clsimhip_mcpe_mask *masked, size_t n_masked, void *d_out, void *d_series, void *d_counts,
                                    void *d_workspace, size_t workspace_bytes, hipStream_t stream)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) throw Error(CLSIMHIP_ERR_DEVICE, "no HIP device available (the PMT series' device path has no CPU fallback)");
    if (device < 0 || device >= count) throw Error(CLSIMHIP_ERR_ARGUMENT, "device ordinal out of range");
    DeviceGuard on_device(device);
    const size_t bytes = pmt_series_blob_bytes(n_particles, n_masked);
    // one call at a time per generator and device prepares its bunch in the staging buffer: the previous call's copy has to be over
    std::lock_guard<std::mutex> lk(series_mutex_);
    PmtSeriesStage *staged = nullptr;
    {
        std::lock_guard<std::mutex> state_lock(device_mutex_);
        staged = &series_state().stages[device];
    }
    PmtSeriesStage &stage = *staged;
    if (stage.done.get()) hip_check(hipEventSynchronize(stage.done.get()), "PMT series: previous upload");
    else stage.done.create_untimed("hipEventCreate");
    if (stage.bytes < bytes) {
        stage.buffer.reset();
        stage.buffer.alloc(bytes, "pinned PMT series bunch");
        stage.bytes = bytes;
    }
    uint8_t *blob = stage.buffer.get();
    const SeriesBunch B = prepare_series(particles, n_particles, masked, n_masked, blob);
    // (the event is recorded right behind the copy, in front of the kernels: the next call waits for the copy, not for the stage)
    series_device_prepared(device, d_hits, d_count, capacity, B, blob, d_out, d_series, d_counts, d_workspace, workspace_bytes, stream, stage.done.get());
}

void PmtHitGenerator::series_device_prepared(int device, const void *d_hits, const void *d_count, size_t capacity, const SeriesBunch &B, const uint8_t *h_blob,
                                             void *d_out, void *d_series, void *d_counts, void *d_workspace, size_t workspace_bytes, hipStream_t stream,
                                             hipEvent_t uploaded)
{
    if (!d_count || !d_counts || !d_workspace) throw Error(CLSIMHIP_ERR_ARGUMENT, "device pointers are (null)");
    if (capacity && (!d_hits || !d_out || !d_series)) throw Error(CLSIMHIP_ERR_ARGUMENT, "d_hits / d_out / d_series is (null)");
    if (capacity > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "capacity beyond 2^32 - 1 records");
    if ((reinterpret_cast<uintptr_t>(d_hits) & 7u) || (reinterpret_cast<uintptr_t>(d_out) & 7u) || (reinterpret_cast<uintptr_t>(d_series) & 7u) ||
        (reinterpret_cast<uintptr_t>(d_workspace) & 15u) || (reinterpret_cast<uintptr_t>(d_counts) & 3u) || (reinterpret_cast<uintptr_t>(d_count) & 3u))
        throw Error(CLSIMHIP_ERR_ARGUMENT, "d_hits, d_out and d_series must be aligned to 8 bytes, d_workspace to 16, d_count and d_counts to 4");
    const PmtSeriesWorkspace W(capacity, B.bytes);
    if (workspace_bytes < W.bytes) throw Error(CLSIMHIP_ERR_ARGUMENT, "the PMT series workspace holds " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(W.bytes) + " are needed");
    DeviceGuard on_device(device);
    const DeviceImage im = image_on(device);
    const SeriesImage sim = series_image_on(device);
    uint8_t *ws = static_cast<uint8_t *>(d_workspace);
    hip_check(hipMemcpyAsync(ws + W.blob, h_blob, B.bytes, hipMemcpyHostToDevice, stream), "upload PMT series bunch");
    if (uploaded) hip_check(hipEventRecord(uploaded, stream), "event");
    PmtSeriesDeviceArgs A{};
    A.lookup.particles = B.have_table ? reinterpret_cast<const SeriesParticle *>(ws + W.blob) : nullptr;
    A.lookup.masked_modules = reinterpret_cast<const uint32_t *>(ws + W.blob + B.masked_offset);
    A.lookup.module_table = im.module_table;
    A.lookup.module_ranks = sim.module_ranks;
    A.lookup.channel_bases = sim.channel_bases;
    A.lookup.base = sim.base;
    A.lookup.n_particles = B.n_particles; A.lookup.n_masked = B.n_masked; A.lookup.module_mask = params_.module_mask;
    A.lookup.n_modules = static_cast<uint32_t>(num_modules());
    A.lookup.n_channels = static_cast<uint32_t>(num_channels());
    A.lookup.consecutive = B.consecutive ? 1u : 0u;
    A.frames = reinterpret_cast<const uint32_t *>(ws + W.blob + B.frames_offset);
    A.module_of_rank = sim.module_of_rank;
    A.in = static_cast<const clsimhip_pmt_hit *>(d_hits);
    A.in_count = static_cast<const uint32_t *>(d_count);
    A.capacity = static_cast<uint32_t>(capacity);
    A.header = reinterpret_cast<uint32_t *>(ws);
    A.histogram = reinterpret_cast<uint32_t *>(ws + W.histogram);
    A.tile_counts = reinterpret_cast<uint32_t *>(ws + W.tile_counts);
    A.keys[0] = reinterpret_cast<SeriesKey *>(ws + W.keys0);
    A.keys[1] = reinterpret_cast<SeriesKey *>(ws + W.keys1);
    A.out = static_cast<clsimhip_pmt_hit *>(d_out);
    A.series = static_cast<clsimhip_pmt_series *>(d_series);
    A.counts = static_cast<uint32_t *>(d_counts);
    const hipError_t e = launch_pmt_series(A, stream);
    if (e != hipSuccess) throw Error(CLSIMHIP_ERR_DEVICE, std::string("PMT series kernel launch: ") + hipGetErrorString(e));
}

} // namespace clsimhip
