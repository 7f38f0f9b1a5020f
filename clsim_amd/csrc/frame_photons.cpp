// Frame photons (frame_photons.h): the stage's DOM list, what a bunch's particle table and mask become before any record is looked at,
// the host twin, and the host side of the device stage.  The kernels are in frame_photons_kernel.hip.
#include "frame_photons.h"

#include <algorithm>
#include <cstring>

namespace clsimhip {

namespace {
// the workspace: header and the two histograms (zeroed together by every call), tile counts, run counts, three key buffers, the
// records' places, the runs, the bunch's blob
struct FramePhotonsWorkspace {
    size_t histogram_a, histogram_b, tile_counts, run_counts, keys0, keys1, keys2, placed, run_first, run_mixed, blob, bytes;
    FramePhotonsWorkspace(size_t capacity, size_t blob_bytes)
    {
        const size_t tiles = std::max<size_t>((capacity + kSeriesTile - 1u) / kSeriesTile, 1u), records = std::max<size_t>(capacity, 1u);
        histogram_a = kSeriesHeaderWords * sizeof(uint32_t);
        histogram_b = histogram_a + 16u * 256u * sizeof(uint32_t);
        tile_counts = histogram_b + 16u * 256u * sizeof(uint32_t);
        run_counts = tile_counts + 256u * tiles * sizeof(uint32_t);
        keys0 = round16(run_counts + tiles * sizeof(uint32_t));
        keys1 = keys0 + records * sizeof(SeriesKey);
        keys2 = keys1 + records * sizeof(SeriesKey);
        placed = keys2 + records * sizeof(SeriesKey);
        run_first = placed + records * sizeof(SeriesKey);
        run_mixed = run_first + round16(records * sizeof(uint32_t));
        blob = run_mixed + round16(records * sizeof(uint32_t));
        bytes = blob + round16(blob_bytes);
    }
};

// what the twin sorts: the key of the two rounds and the content
struct Kept { SeriesKey key; uint32_t h; FramePhotonContent content; };

bool same_run(const Kept &a, const Kept &b)
{
    return a.key.group == b.key.group && a.key.t_hi == b.key.t_hi && a.key.t_lo == b.key.t_lo && a.key.identifier == b.key.identifier && a.h == b.h;
}
bool kept_less(const Kept &a, const Kept &b)
{
    if (a.key.group != b.key.group) return a.key.group < b.key.group;
    if (a.key.t_hi != b.key.t_hi) return a.key.t_hi < b.key.t_hi;
    if (a.key.t_lo != b.key.t_lo) return a.key.t_lo < b.key.t_lo;
    if (a.key.identifier != b.key.identifier) return a.key.identifier < b.key.identifier;
    if (a.h != b.h) return a.h < b.h;
    return frame_photons_compare(a.content, b.content) < 0;
}
} // namespace

// (the blob has the MCPE series' layout: series_bunch.h)
size_t frame_photons_blob_bytes(size_t n_particles, size_t n_masked) { return series_blob_bytes(n_particles, n_masked); }

size_t frame_photons_workspace_bytes(size_t capacity, size_t n_particles, size_t n_masked)
{
    return FramePhotonsWorkspace(capacity, series_blob_bytes(n_particles, n_masked)).bytes;
}

FramePhotonDoms::FramePhotonDoms(const int32_t *string_ids, const uint32_t *om_ids, size_t n)
{
    if (n && (!string_ids || !om_ids)) throw Error(CLSIMHIP_ERR_ARGUMENT, "string_ids / om_ids is (null)");
    if (n > (size_t{1} << 24)) throw Error(CLSIMHIP_ERR_ARGUMENT, "more than 2^24 DOMs");
    size_t slots = 2;
    while (slots < 2u * n) slots *= 2u;
    dom_mask_ = static_cast<uint32_t>(slots - 1u);
    dom_table_.assign(slots, 0u);
    for (size_t i = 0; i < n; ++i) {
        if (string_ids[i] < -32768 || string_ids[i] > 32767 || om_ids[i] > 65535u)
            throw Error(CLSIMHIP_ERR_ARGUMENT, "string ID " + std::to_string(string_ids[i]) + " / OM ID " + std::to_string(om_ids[i]) + " does not fit the photon record");
        const uint32_t word = record_word(string_ids[i], om_ids[i]);
        uint32_t slot = ((word * 2654435761u) >> 7) & dom_mask_;            // series_dom_rank's
        while (dom_table_[slot] != 0u && static_cast<uint32_t>(dom_table_[slot]) != word) slot = (slot + 1u) & dom_mask_;
        if (dom_table_[slot] == 0u) dom_of_rank_.push_back(word);           // (a DOM named twice is one DOM)
        dom_table_[slot] = static_cast<uint64_t>(word) | (uint64_t{1} << 32);
    }
    std::sort(dom_of_rank_.begin(), dom_of_rank_.end(), [](uint32_t a, uint32_t b) {
        const int16_t sa = static_cast<int16_t>(a & 0xffffu), sb = static_cast<int16_t>(b & 0xffffu);
        return sa != sb ? sa < sb : (a >> 16) < (b >> 16);
    });
    dom_ranks_.assign(slots, 0u);
    for (size_t r = 0; r < dom_of_rank_.size(); ++r) {
        uint32_t slot = ((dom_of_rank_[r] * 2654435761u) >> 7) & dom_mask_;
        while (static_cast<uint32_t>(dom_table_[slot]) != dom_of_rank_[r] || dom_table_[slot] == 0u) slot = (slot + 1u) & dom_mask_;
        dom_ranks_[slot] = static_cast<uint32_t>(r);
    }
}

FramePhotonDoms::~FramePhotonDoms()
{
    for (auto &kv : images_) {
        DeviceGuard on_device(kv.first, std::nothrow);
        DeviceBuffer<uint64_t> table(kv.second.dom_table);
        DeviceBuffer<uint32_t> ranks(kv.second.dom_ranks);
    }
}

SeriesBunch FramePhotonDoms::prepare(const clsimhip_mcpe_particle *particles, size_t n_particles, const clsimhip_mcpe_mask *masked, size_t n_masked,
                                     uint8_t *blob) const
{
    // a masked entry's key is its group: frame rank x DOMs + DOM rank
    const uint32_t n_doms = static_cast<uint32_t>(num_doms());
    return prepare_series_bunch(particles, n_particles, masked, n_masked, blob, num_doms(), "frame photons", "DOMs", [&](uint32_t frame_rank, uint32_t word) -> int64_t {
        const int64_t rank = series_dom_rank(dom_table_.data(), dom_ranks_.data(), dom_mask_, word);
        return rank < 0 ? -1 : static_cast<int64_t>(frame_rank * n_doms + static_cast<uint32_t>(rank));
    });
}

void FramePhotonDoms::host(const clsimhip_photon *in, size_t n, const clsimhip_mcpe_particle *particles, size_t n_particles, const clsimhip_mcpe_mask *masked,
                           size_t n_masked, clsimhip_frame_photon *out, clsimhip_mcpe_series *series, size_t *n_kept, size_t *n_series, uint64_t counters[4]) const
{
    if (n && (!in || !out || !series)) throw Error(CLSIMHIP_ERR_ARGUMENT, "photons / out / series is (null)");
    if (n > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "more than 2^32 - 1 records");
    std::vector<SeriesParticle> aligned((frame_photons_blob_bytes(n_particles, n_masked) + sizeof(SeriesParticle) - 1u) / sizeof(SeriesParticle));
    uint8_t *blob = reinterpret_cast<uint8_t *>(aligned.data());
    const SeriesBunch B = prepare(particles, n_particles, masked, n_masked, blob);
    SeriesLookup L{};
    set_series_lookup(L, B, blob);
    L.masked_groups = reinterpret_cast<const uint32_t *>(blob + B.masked_offset);
    L.dom_table = dom_table_.data();
    L.dom_ranks = dom_ranks_.data();
    L.dom_mask = dom_mask_;
    L.n_doms = static_cast<uint32_t>(num_doms());
    const uint32_t *frames = reinterpret_cast<const uint32_t *>(blob + B.frames_offset);
    std::vector<Kept> kept;
    kept.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        uint32_t g[20];                                                     // (the record is packed: no word of it is read in place)
        std::memcpy(g, in + i, sizeof g);
        float time;
        std::memcpy(&time, g + 3, sizeof time);
        Kept k;
        const int code = series_make_key(L, g[10], g[11], static_cast<double>(time), k.key);
        if (code != FRAME_PHOTONS_KEPT) {
            if (counters) ++counters[code];
            continue;
        }
        frame_photons_content(g, g + 4, g + 8, g + 16, k.content);
        k.h = frame_photons_mix(k.content);
        kept.push_back(k);
    }
    std::sort(kept.begin(), kept.end(), kept_less);
    // the bound: a run with two distinct contents (sorted: its first and last differ) and more than kFramePhotonsTieBound members
    uint64_t overflow = 0;
    for (size_t begin = 0; begin < kept.size();) {
        size_t end = begin + 1u;
        while (end < kept.size() && same_run(kept[begin], kept[end])) ++end;
        if (end - begin > kFramePhotonsTieBound && frame_photons_compare(kept[begin].content, kept[end - 1u].content) != 0) overflow += end - begin;
        begin = end;
    }
    if (counters) counters[FRAME_PHOTONS_TIE_OVERFLOW] += overflow;
    if (overflow) kept.clear();                                             // no records from a bunch that met the bound
    size_t made = 0;
    for (size_t i = 0; i < kept.size(); ++i) {
        const Kept &k = kept[i];
        const uint32_t frame_rank = k.key.group / L.n_doms;
        const uint32_t word = dom_of_rank_[k.key.group - frame_rank * L.n_doms];
        clsimhip_frame_photon &p = out[i];
        p.identifier = k.key.identifier;
        p.string_id = static_cast<int16_t>(word & 0xffffu);
        p.om_id = static_cast<uint16_t>(word >> 16);
        p.time = series_time_of((static_cast<uint64_t>(k.key.t_hi) << 32) | k.key.t_lo);
        std::memcpy(&p.weight, k.content.w, sizeof k.content.w);            // the eight floats, bit for bit
        if (i == 0 || kept[i - 1].key.group != k.key.group) {
            clsimhip_mcpe_series &s = series[made++];
            s.frame = frames[frame_rank];
            s.string_id = p.string_id; s.om_id = p.om_id;
            s.first = static_cast<uint32_t>(i);
            s.count = 0u;
        }
        ++series[made - 1].count;
    }
    if (n_kept) *n_kept = kept.size();
    if (n_series) *n_series = made;
}

FramePhotonDoms::Image FramePhotonDoms::image_on(int device)
{
    std::lock_guard<std::mutex> lk(device_mutex_);
    auto it = images_.find(device);
    if (it != images_.end()) return it->second;
    DeviceBuffer<uint64_t> table(dom_table_.size(), "frame photons: DOM table");
    DeviceBuffer<uint32_t> ranks(dom_ranks_.size(), "frame photons: DOM ranks");
    hip_check(hipMemcpy(table.get(), dom_table_.data(), dom_table_.size() * sizeof(uint64_t), hipMemcpyHostToDevice), "frame photons: DOM table");
    hip_check(hipMemcpy(ranks.get(), dom_ranks_.data(), dom_ranks_.size() * sizeof(uint32_t), hipMemcpyHostToDevice), "frame photons: DOM ranks");
    const Image im{table.release(), ranks.release()};
    images_[device] = im;
    return im;
}

void FramePhotonDoms::device(int device, const void *d_photons, const void *d_count, size_t capacity, const clsimhip_mcpe_particle *particles, size_t n_particles,
                             const clsimhip_mcpe_mask *masked, size_t n_masked, void *d_out, void *d_series, void *d_counts, void *d_workspace,
                             size_t workspace_bytes, hipStream_t stream)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) throw Error(CLSIMHIP_ERR_DEVICE, "no HIP device available (the frame photons' device path has no CPU fallback)");
    if (device < 0 || device >= count) throw Error(CLSIMHIP_ERR_ARGUMENT, "device ordinal out of range");
    DeviceGuard on_device(device);
    // one call at a time per object prepares its bunch in the staging buffer: the previous call's copy has to be over
    std::lock_guard<std::mutex> lk(call_mutex_);
    uint8_t *blob = staging_.acquire(device, series_blob_bytes(n_particles, n_masked), "frame photons");
    const SeriesBunch B = prepare(particles, n_particles, masked, n_masked, blob);
    device_prepared(device, d_photons, d_count, capacity, B, blob, d_out, d_series, d_counts, d_workspace, workspace_bytes, stream, staging_.done(device));
}

void FramePhotonDoms::device_prepared(int device, const void *d_photons, const void *d_count, size_t capacity, const SeriesBunch &B, const uint8_t *h_blob,
                                      void *d_out, void *d_series, void *d_counts, void *d_workspace, size_t workspace_bytes, hipStream_t stream, hipEvent_t uploaded)
{
    const FramePhotonsWorkspace W(capacity, B.bytes);
    check_series_device_args("frame photons", "d_photons", 16u, d_photons, d_count, capacity, d_out, d_series, d_counts, d_workspace, workspace_bytes, W.bytes);
    DeviceGuard on_device(device);
    const Image im = image_on(device);
    uint8_t *ws = static_cast<uint8_t *>(d_workspace);
    hip_check(hipMemcpyAsync(ws + W.blob, h_blob, B.bytes, hipMemcpyHostToDevice, stream), "upload frame photons bunch");
    if (uploaded) hip_check(hipEventRecord(uploaded, stream), "event");
    FramePhotonsDeviceArgs A{};
    set_series_lookup(A.lookup, B, ws + W.blob);
    A.lookup.masked_groups = reinterpret_cast<const uint32_t *>(ws + W.blob + B.masked_offset);
    A.lookup.dom_table = im.dom_table;
    A.lookup.dom_ranks = im.dom_ranks;
    A.lookup.dom_mask = dom_mask_;
    A.lookup.n_doms = static_cast<uint32_t>(num_doms());
    A.frames = reinterpret_cast<const uint32_t *>(ws + W.blob + B.frames_offset);
    A.in = static_cast<const clsimhip_photon *>(d_photons);
    A.in_count = static_cast<const uint32_t *>(d_count);
    A.capacity = static_cast<uint32_t>(capacity);
    A.header = reinterpret_cast<uint32_t *>(ws);
    A.histogram[0] = reinterpret_cast<uint32_t *>(ws + W.histogram_a);
    A.histogram[1] = reinterpret_cast<uint32_t *>(ws + W.histogram_b);
    A.tile_counts = reinterpret_cast<uint32_t *>(ws + W.tile_counts);
    A.run_counts = reinterpret_cast<uint32_t *>(ws + W.run_counts);
    A.keys[0] = reinterpret_cast<SeriesKey *>(ws + W.keys0);
    A.keys[1] = reinterpret_cast<SeriesKey *>(ws + W.keys1);
    A.keys[2] = reinterpret_cast<SeriesKey *>(ws + W.keys2);
    A.placed = reinterpret_cast<SeriesKey *>(ws + W.placed);
    A.run_first = reinterpret_cast<uint32_t *>(ws + W.run_first);
    A.run_mixed = reinterpret_cast<uint32_t *>(ws + W.run_mixed);
    A.out = static_cast<clsimhip_frame_photon *>(d_out);
    A.series = static_cast<clsimhip_mcpe_series *>(d_series);
    A.counts = static_cast<uint32_t *>(d_counts);
    const hipError_t e = launch_frame_photons(A, stream);
    if (e != hipSuccess) throw Error(CLSIMHIP_ERR_DEVICE, std::string("frame photons kernel launch: ") + hipGetErrorString(e));
}

} // namespace clsimhip
