// PMT series (pmt_series.h): the generator's rank and channel tables, what a bunch's particle table and mask become before any
// record is looked at, the host twin, and the host side of the device stage.  The kernels are in pmt_series_kernel.hip.
#include "pmt_series.h"

#include <algorithm>
#include <cstring>

namespace clsimhip {

// (the blob and the workspace have the MCPE series' layout: series_bunch.h)
size_t pmt_series_blob_bytes(size_t n_particles, size_t n_masked) { return series_blob_bytes(n_particles, n_masked); }

size_t pmt_series_workspace_bytes(size_t capacity, size_t n_particles, size_t n_masked)
{
    return SeriesWorkspaceLayout(capacity, series_blob_bytes(n_particles, n_masked)).bytes;
}

SeriesBunch PmtHitGenerator::prepare_series(const clsimhip_mcpe_particle *particles, size_t n_particles, const clsimhip_mcpe_mask *masked, size_t n_masked,
                                            uint8_t *blob) const
{
    // a frame has as many groups as the generator has channels, but the mask names modules: its keys are frame rank x modules + module rank
    const uint32_t n_modules = static_cast<uint32_t>(num_modules());
    return prepare_series_bunch(particles, n_particles, masked, n_masked, blob, num_channels(), "PMT series", "channels", [&](uint32_t frame_rank, uint32_t word) -> int64_t {
        const int64_t slot = pmt_series_module_slot(module_table_.data(), params_.module_mask, word);
        return slot < 0 ? -1 : static_cast<int64_t>(frame_rank * n_modules + module_ranks_[slot]);
    });
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
    set_series_lookup(L, B, blob);
    L.masked_modules = reinterpret_cast<const uint32_t *>(blob + B.masked_offset);
    L.module_table = module_table_.data();
    L.module_ranks = module_ranks_.data();
    L.channel_bases = channel_bases_.data();
    L.base = base_.data();
    L.module_mask = params_.module_mask;
    L.n_modules = static_cast<uint32_t>(num_modules());
    L.n_channels = static_cast<uint32_t>(num_channels());
    const uint32_t *frames = reinterpret_cast<const uint32_t *>(blob + B.frames_offset);
    std::vector<SeriesKey> keys;
    keys.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        SeriesKey k;
        const int code = pmt_series_make_key(L, in[i].identifier, record_word(in[i].string_id, in[i].om_id), in[i].pmt, in[i].time, k);
        if (code == PMT_SERIES_KEPT) keys.push_back(k);
        else if (counters) ++counters[code];
    }
    std::sort(keys.begin(), keys.end(), series_key_less);
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

struct PmtHitGenerator::SeriesState {
    std::map<int, SeriesImage> images;
    SeriesStaging staging;                  // of the stand-alone series call's bunch (series_bunch.h): calls under series_mutex_, its map under device_mutex_
    explicit SeriesState(std::mutex *device_mutex) : staging(device_mutex) {}
    ~SeriesState()
    {
        for (auto &kv : images) {
            DeviceGuard on_device(kv.first, std::nothrow);
            DeviceBuffer<uint32_t> ranks(kv.second.module_ranks), bases(kv.second.channel_bases), base(kv.second.base), of_rank(kv.second.module_of_rank);
        }
    }
};

PmtHitGenerator::SeriesState &PmtHitGenerator::series_state()
{
    if (!series_state_) series_state_ = std::make_shared<SeriesState>(&device_mutex_);
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
    // one call at a time per generator and device prepares its bunch in the staging buffer: the previous call's copy has to be over
    std::lock_guard<std::mutex> lk(series_mutex_);
    SeriesStaging *staging = nullptr;
    {
        std::lock_guard<std::mutex> state_lock(device_mutex_);
        staging = &series_state().staging;
    }
    uint8_t *blob = staging->acquire(device, series_blob_bytes(n_particles, n_masked), "PMT series");
    const SeriesBunch B = prepare_series(particles, n_particles, masked, n_masked, blob);
    series_device_prepared(device, d_hits, d_count, capacity, B, blob, d_out, d_series, d_counts, d_workspace, workspace_bytes, stream, staging->done(device));
}

void PmtHitGenerator::series_device_prepared(int device, const void *d_hits, const void *d_count, size_t capacity, const SeriesBunch &B, const uint8_t *h_blob,
                                             void *d_out, void *d_series, void *d_counts, void *d_workspace, size_t workspace_bytes, hipStream_t stream,
                                             hipEvent_t uploaded)
{
    const SeriesWorkspaceLayout W(capacity, B.bytes);
    check_series_device_args("PMT series", "d_hits", 8u, d_hits, d_count, capacity, d_out, d_series, d_counts, d_workspace, workspace_bytes, W.bytes);
    DeviceGuard on_device(device);
    const DeviceImage im = image_on(device);
    const SeriesImage sim = series_image_on(device);
    uint8_t *ws = static_cast<uint8_t *>(d_workspace);
    hip_check(hipMemcpyAsync(ws + W.blob, h_blob, B.bytes, hipMemcpyHostToDevice, stream), "upload PMT series bunch");
    if (uploaded) hip_check(hipEventRecord(uploaded, stream), "event");
    PmtSeriesDeviceArgs A{};
    set_series_lookup(A.lookup, B, ws + W.blob);
    A.lookup.masked_modules = reinterpret_cast<const uint32_t *>(ws + W.blob + B.masked_offset);
    A.lookup.module_table = im.module_table;
    A.lookup.module_ranks = sim.module_ranks;
    A.lookup.channel_bases = sim.channel_bases;
    A.lookup.base = sim.base;
    A.lookup.module_mask = params_.module_mask;
    A.lookup.n_modules = static_cast<uint32_t>(num_modules());
    A.lookup.n_channels = static_cast<uint32_t>(num_channels());
    A.frames = reinterpret_cast<const uint32_t *>(ws + W.blob + B.frames_offset);
    A.module_of_rank = sim.module_of_rank;
    A.in = static_cast<const clsimhip_pmt_hit *>(d_hits);
    A.in_count = static_cast<const uint32_t *>(d_count);
    A.capacity = static_cast<uint32_t>(capacity);
    set_series_workspace(A, ws, W);
    A.out = static_cast<clsimhip_pmt_hit *>(d_out);
    A.series = static_cast<clsimhip_pmt_series *>(d_series);
    A.counts = static_cast<uint32_t *>(d_counts);
    const hipError_t e = launch_pmt_series(A, stream);
    if (e != hipSuccess) throw Error(CLSIMHIP_ERR_DEVICE, std::string("PMT series kernel launch: ") + hipGetErrorString(e));
}

} // namespace clsimhip
