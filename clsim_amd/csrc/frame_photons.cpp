// Frame photons (frame_photons.h): the stage's DOM list, what a bunch's particle table and mask become before any record is looked at,
// the host twin, and the host side of the device stage.  The kernels are in frame_photons_kernel.hip.
#include "frame_photons.h"

#include <algorithm>
#include <cstring>

namespace clsimhip {

namespace {
size_t round16(size_t v) { return (v + 15u) & ~size_t{15}; }

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

uint32_t record_word(int32_t string_id, uint32_t om_id) { return static_cast<uint32_t>(static_cast<uint16_t>(string_id)) | (om_id << 16); }

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

// (the blob has the MCPE series' layout: table, frame IDs by rank, masked groups)
size_t frame_photons_blob_bytes(size_t n_particles, size_t n_masked)
{
    return round16(n_particles * sizeof(SeriesParticle)) + round16(std::max<size_t>(n_particles, 1u) * sizeof(uint32_t)) + round16(n_masked * sizeof(uint32_t)) + 16u;
}

size_t frame_photons_workspace_bytes(size_t capacity, size_t n_particles, size_t n_masked)
{
    return FramePhotonsWorkspace(capacity, frame_photons_blob_bytes(n_particles, n_masked)).bytes;
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
    for (auto &kv : stages_) {
        DeviceGuard on_device(kv.first, std::nothrow);
        kv.second = Stage();
    }
}

SeriesBunch FramePhotonDoms::prepare(const clsimhip_mcpe_particle *particles, size_t n_particles, const clsimhip_mcpe_mask *masked, size_t n_masked,
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
    B.bytes = frame_photons_blob_bytes(n_particles, n_masked);
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
        throw Error(CLSIMHIP_ERR_CONFIG, "frame photons: " + std::to_string(n_frames) + " frames x " + std::to_string(n_doms) + " DOMs do not fit 32 bits");
    B.n_frames = static_cast<uint32_t>(n_frames);
    // mask: the (frame, module) pairs it names, ascending and distinct; what names no frame of the table or no DOM of the list is
    // ignored
    size_t kept = 0;
    for (size_t i = 0; i < n_masked; ++i) {
        const uint32_t *f = std::lower_bound(frames, frames + n_frames, masked[i].frame);
        if (f == frames + n_frames || *f != masked[i].frame || (B.have_table && n_particles == 0)) continue;
        const int64_t rank = series_dom_rank(dom_table_.data(), dom_ranks_.data(), dom_mask_, record_word(masked[i].string_id, masked[i].om_id));
        if (rank < 0) continue;
        groups[kept++] = static_cast<uint32_t>(f - frames) * static_cast<uint32_t>(n_doms) + static_cast<uint32_t>(rank);
    }
    std::sort(groups, groups + kept);
    B.n_masked = static_cast<uint32_t>(std::unique(groups, groups + kept) - groups);
    return B;
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
    L.particles = B.have_table ? reinterpret_cast<const SeriesParticle *>(blob) : nullptr;
    L.masked_groups = reinterpret_cast<const uint32_t *>(blob + B.masked_offset);
    L.dom_table = dom_table_.data();
    L.dom_ranks = dom_ranks_.data();
    L.n_particles = B.n_particles; L.n_masked = B.n_masked; L.dom_mask = dom_mask_;
    L.n_doms = static_cast<uint32_t>(num_doms());
    L.consecutive = B.consecutive ? 1u : 0u;
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
    const size_t bytes = frame_photons_blob_bytes(n_particles, n_masked);
    // one call at a time per object prepares its bunch in the staging buffer: the previous call's copy has to be over
    std::lock_guard<std::mutex> lk(call_mutex_);
    Stage *staged = nullptr;
    {
        std::lock_guard<std::mutex> state_lock(device_mutex_);
        staged = &stages_[device];
    }
    Stage &stage = *staged;
    if (stage.done.get()) hip_check(hipEventSynchronize(stage.done.get()), "frame photons: previous upload");
    else stage.done.create_untimed("hipEventCreate");
    if (stage.bytes < bytes) {
        stage.buffer.reset();
        stage.buffer.alloc(bytes, "pinned frame photons bunch");
        stage.bytes = bytes;
    }
    uint8_t *blob = stage.buffer.get();
    const SeriesBunch B = prepare(particles, n_particles, masked, n_masked, blob);
    // (the event is recorded right behind the copy, in front of the kernels: the next call waits for the copy, not for the stage)
    device_prepared(device, d_photons, d_count, capacity, B, blob, d_out, d_series, d_counts, d_workspace, workspace_bytes, stream, stage.done.get());
}

void FramePhotonDoms::device_prepared(int device, const void *d_photons, const void *d_count, size_t capacity, const SeriesBunch &B, const uint8_t *h_blob,
                                      void *d_out, void *d_series, void *d_counts, void *d_workspace, size_t workspace_bytes, hipStream_t stream, hipEvent_t uploaded)
{
    if (!d_count || !d_counts || !d_workspace) throw Error(CLSIMHIP_ERR_ARGUMENT, "device pointers are (null)");
    if (capacity && (!d_photons || !d_out || !d_series)) throw Error(CLSIMHIP_ERR_ARGUMENT, "d_photons / d_out / d_series is (null)");
    if (capacity > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "capacity beyond 2^32 - 1 records");
    if ((reinterpret_cast<uintptr_t>(d_photons) & 15u) || (reinterpret_cast<uintptr_t>(d_out) & 15u) || (reinterpret_cast<uintptr_t>(d_series) & 15u) ||
        (reinterpret_cast<uintptr_t>(d_workspace) & 15u) || (reinterpret_cast<uintptr_t>(d_counts) & 3u) || (reinterpret_cast<uintptr_t>(d_count) & 3u))
        throw Error(CLSIMHIP_ERR_ARGUMENT, "d_photons, d_out, d_series and d_workspace must be aligned to 16 bytes, d_count and d_counts to 4");
    const FramePhotonsWorkspace W(capacity, B.bytes);
    if (workspace_bytes < W.bytes)
        throw Error(CLSIMHIP_ERR_ARGUMENT, "the frame photons workspace holds " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(W.bytes) + " are needed");
    DeviceGuard on_device(device);
    const Image im = image_on(device);
    uint8_t *ws = static_cast<uint8_t *>(d_workspace);
    hip_check(hipMemcpyAsync(ws + W.blob, h_blob, B.bytes, hipMemcpyHostToDevice, stream), "upload frame photons bunch");
    if (uploaded) hip_check(hipEventRecord(uploaded, stream), "event");
    FramePhotonsDeviceArgs A{};
    A.lookup.particles = B.have_table ? reinterpret_cast<const SeriesParticle *>(ws + W.blob) : nullptr;
    A.lookup.masked_groups = reinterpret_cast<const uint32_t *>(ws + W.blob + B.masked_offset);
    A.lookup.dom_table = im.dom_table;
    A.lookup.dom_ranks = im.dom_ranks;
    A.lookup.n_particles = B.n_particles; A.lookup.n_masked = B.n_masked; A.lookup.dom_mask = dom_mask_;
    A.lookup.n_doms = static_cast<uint32_t>(num_doms());
    A.lookup.consecutive = B.consecutive ? 1u : 0u;
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
