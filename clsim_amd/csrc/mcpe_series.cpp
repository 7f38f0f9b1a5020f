// MCPE series (mcpe_series.h): what a bunch's particle table and mask become before any record is looked at, the host twin, and
// the host side of the device stage.  The kernels are in mcpe_series_kernel.hip.
#include "mcpe_series.h"

#include <algorithm>
#include <cstring>

#include "mcpe.h"

namespace clsimhip {

size_t mcpe_series_blob_bytes(size_t n_particles, size_t n_masked) { return series_blob_bytes(n_particles, n_masked); }

size_t mcpe_series_workspace_bytes(size_t capacity, size_t n_particles, size_t n_masked)
{
    return SeriesWorkspaceLayout(capacity, series_blob_bytes(n_particles, n_masked)).bytes;
}

SeriesBunch McpeGenerator::prepare_series(const clsimhip_mcpe_particle *particles, size_t n_particles, const clsimhip_mcpe_mask *masked, size_t n_masked,
                                          uint8_t *blob) const
{
    // a masked entry's key is its group: frame rank x DOMs + DOM rank
    const uint32_t n_doms = static_cast<uint32_t>(num_doms());
    return prepare_series_bunch(particles, n_particles, masked, n_masked, blob, num_doms(), "MCPE series", "DOMs", [&](uint32_t frame_rank, uint32_t word) -> int64_t {
        const int64_t rank = series_dom_rank(dom_table_.data(), dom_ranks_.data(), params_.dom_mask, word);
        return rank < 0 ? -1 : static_cast<int64_t>(frame_rank * n_doms + static_cast<uint32_t>(rank));
    });
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
    set_series_lookup(L, B, blob);
    L.masked_groups = reinterpret_cast<const uint32_t *>(blob + B.masked_offset);
    L.dom_table = dom_table_.data();
    L.dom_ranks = dom_ranks_.data();
    L.dom_mask = params_.dom_mask;
    L.n_doms = static_cast<uint32_t>(num_doms());
    const uint32_t *frames = reinterpret_cast<const uint32_t *>(blob + B.frames_offset);
    std::vector<SeriesKey> keys;
    keys.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        SeriesKey k;
        const int code = series_make_key(L, in[i].identifier, record_word(in[i].string_id, in[i].om_id), in[i].time, k);
        if (code == SERIES_KEPT) keys.push_back(k);
        else if (counters) ++counters[code];
    }
    std::sort(keys.begin(), keys.end(), series_key_less);
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
    // one call at a time per generator and device prepares its bunch in the staging buffer: the previous call's copy has to be over
    std::lock_guard<std::mutex> lk(series_mutex_);
    uint8_t *blob = staging_.acquire(device, series_blob_bytes(n_particles, n_masked), "MCPE series");
    const SeriesBunch B = prepare_series(particles, n_particles, masked, n_masked, blob);
    series_device_prepared(device, d_mcpes, d_count, capacity, B, blob, d_out, d_series, d_counts, d_workspace, workspace_bytes, stream, staging_.done(device));
}

void McpeGenerator::series_device_prepared(int device, const void *d_mcpes, const void *d_count, size_t capacity, const SeriesBunch &B, const uint8_t *h_blob,
                                           void *d_out, void *d_series, void *d_counts, void *d_workspace, size_t workspace_bytes, hipStream_t stream,
                                           hipEvent_t uploaded)
{
    const SeriesWorkspaceLayout W(capacity, B.bytes);
    check_series_device_args("MCPE series", "d_mcpes", 8u, d_mcpes, d_count, capacity, d_out, d_series, d_counts, d_workspace, workspace_bytes, W.bytes);
    DeviceGuard on_device(device);
    const DeviceImage im = image_on(device);
    uint8_t *ws = static_cast<uint8_t *>(d_workspace);
    hip_check(hipMemcpyAsync(ws + W.blob, h_blob, B.bytes, hipMemcpyHostToDevice, stream), "upload MCPE series bunch");
    if (uploaded) hip_check(hipEventRecord(uploaded, stream), "event");
    SeriesDeviceArgs A{};
    set_series_lookup(A.lookup, B, ws + W.blob);
    A.lookup.masked_groups = reinterpret_cast<const uint32_t *>(ws + W.blob + B.masked_offset);
    A.lookup.dom_table = im.dom_table;
    A.lookup.dom_ranks = im.dom_ranks;
    A.lookup.dom_mask = params_.dom_mask;
    A.lookup.n_doms = static_cast<uint32_t>(num_doms());
    A.frames = reinterpret_cast<const uint32_t *>(ws + W.blob + B.frames_offset);
    A.dom_of_rank = im.dom_of_rank;
    A.in = static_cast<const clsimhip_mcpe *>(d_mcpes);
    A.in_count = static_cast<const uint32_t *>(d_count);
    A.capacity = static_cast<uint32_t>(capacity);
    set_series_workspace(A, ws, W);
    A.out = static_cast<clsimhip_mcpe *>(d_out);
    A.series = static_cast<clsimhip_mcpe_series *>(d_series);
    A.counts = static_cast<uint32_t *>(d_counts);
    const hipError_t e = launch_mcpe_series(A, stream);
    if (e != hipSuccess) throw Error(CLSIMHIP_ERR_DEVICE, std::string("MCPE series kernel launch: ") + hipGetErrorString(e));
}

} // namespace clsimhip
