// What the three series stages (mcpe_series.h, pmt_series.h, frame_photons.h) have in common on the host: the form a bunch's particle
// table and mask are brought into before any record is looked at (the "blob": table, frame IDs by rank, masked keys), the workspace
// of the two stages that share mcpe_series_kernel.hip's radix passes, the page-locked staging of the stand-alone *_device calls, and
// the checks the *_device_prepared calls open with.  Header-only on purpose: each stage's .cpp links without the others'.
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <mutex>
#include <string>

#include "hip_resources.h"
#include "host_model.h"
#include "mcpe_series.h"

namespace clsimhip {

inline size_t round16(size_t v) { return (v + 15u) & ~size_t{15}; }

// string ID | OM ID << 16, as in the records
inline uint32_t record_word(int32_t string_id, uint32_t om_id) { return static_cast<uint32_t>(static_cast<uint16_t>(string_id)) | (om_id << 16); }

inline bool series_key_less(const SeriesKey &a, const SeriesKey &b)
{
    if (a.group != b.group) return a.group < b.group;
    if (a.t_hi != b.t_hi) return a.t_hi < b.t_hi;
    if (a.t_lo != b.t_lo) return a.t_lo < b.t_lo;
    return a.identifier < b.identifier;
}

// the blob: table, frame IDs by rank, masked keys, each rounded up to 16 bytes
inline size_t series_blob_bytes(size_t n_particles, size_t n_masked)
{
    return round16(n_particles * sizeof(SeriesParticle)) + round16(std::max<size_t>(n_particles, 1u) * sizeof(uint32_t)) + round16(n_masked * sizeof(uint32_t)) + 16u;
}

// the workspace of the MCPE and the PMT series stage: header and histogram (zeroed together by every call), tile counts, two key
// buffers, the bunch's blob
struct SeriesWorkspaceLayout {
    size_t histogram, tile_counts, keys0, keys1, blob, bytes;
    SeriesWorkspaceLayout(size_t capacity, size_t blob_bytes)
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

// ... and where its pieces are, for SeriesDeviceArgs and PmtSeriesDeviceArgs
template <class Args>
void set_series_workspace(Args &A, uint8_t *ws, const SeriesWorkspaceLayout &W)
{
    A.header = reinterpret_cast<uint32_t *>(ws);
    A.histogram = reinterpret_cast<uint32_t *>(ws + W.histogram);
    A.tile_counts = reinterpret_cast<uint32_t *>(ws + W.tile_counts);
    A.keys[0] = reinterpret_cast<SeriesKey *>(ws + W.keys0);
    A.keys[1] = reinterpret_cast<SeriesKey *>(ws + W.keys1);
}

// the bunch's part of a SeriesLookup or PmtSeriesLookup, with the blob wherever it lives (the masked keys are at blob + masked_offset)
template <class Lookup>
void set_series_lookup(Lookup &L, const SeriesBunch &B, const uint8_t *blob)
{
    L.particles = B.have_table ? reinterpret_cast<const SeriesParticle *>(blob) : nullptr;
    L.n_particles = B.n_particles; L.n_masked = B.n_masked;
    L.consecutive = B.consecutive ? 1u : 0u;
}

// One bunch's particle table and mask, checked and written to `blob` (series_blob_bytes(n_particles, n_masked) bytes, 16-byte
// aligned).  A frame has `groups_per_frame` groups (`unit`: what the stage calls them); group_of(frame rank, record word) is the
// masked entry's key, or negative for a module that is not the stage's.
template <class GroupOf>
SeriesBunch prepare_series_bunch(const clsimhip_mcpe_particle *particles, size_t n_particles, const clsimhip_mcpe_mask *masked, size_t n_masked, uint8_t *blob,
                                 uint64_t groups_per_frame, const char *stage, const char *unit, GroupOf group_of)
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
    B.bytes = series_blob_bytes(n_particles, n_masked);
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
    if (static_cast<uint64_t>(n_frames) * std::max<uint64_t>(groups_per_frame, 1u) >= (uint64_t{1} << 32))
        throw Error(CLSIMHIP_ERR_CONFIG, std::string(stage) + ": " + std::to_string(n_frames) + " frames x " + std::to_string(groups_per_frame) + " " + unit + " do not fit 32 bits");
    B.n_frames = static_cast<uint32_t>(n_frames);
    // mask: the keys it names, ascending and distinct; what names no frame of the table or no module of the stage is ignored
    size_t kept = 0;
    for (size_t i = 0; i < n_masked; ++i) {
        const uint32_t *f = std::lower_bound(frames, frames + n_frames, masked[i].frame);
        if (f == frames + n_frames || *f != masked[i].frame || (B.have_table && n_particles == 0)) continue;
        const int64_t key = group_of(static_cast<uint32_t>(f - frames), record_word(masked[i].string_id, masked[i].om_id));
        if (key >= 0) keys[kept++] = static_cast<uint32_t>(key);
    }
    std::sort(keys, keys + kept);
    B.n_masked = static_cast<uint32_t>(std::unique(keys, keys + kept) - keys);
    return B;
}

// Page-locked staging of a stand-alone *_device call's bunch, one buffer per device, reused once its upload has been passed.  The
// owner lets one call at a time in (McpeGenerator and PmtHitGenerator: series_mutex_, FramePhotonDoms: call_mutex_); `map_mutex`, if
// given, is the owner's mutex for its per-device maps and is held while this one is looked into, not while a call waits or allocates.
class SeriesStaging {
public:
    explicit SeriesStaging(std::mutex *map_mutex = nullptr) : map_mutex_(map_mutex) {}
    SeriesStaging(const SeriesStaging &) = delete;
    SeriesStaging &operator=(const SeriesStaging &) = delete;
    ~SeriesStaging()
    {
        for (auto &kv : entries_) {
            DeviceGuard on_device(kv.first, std::nothrow);
            kv.second = Entry();
        }
    }
    // the device's buffer, at least `bytes` long, once the previous call's copy out of it is over (the caller has made `device` current)
    uint8_t *acquire(int device, size_t bytes, const char *stage)
    {
        Entry &e = entry(device);
        if (e.done.get()) hip_check(hipEventSynchronize(e.done.get()), (std::string(stage) + ": previous upload").c_str());
        else e.done.create_untimed("hipEventCreate");
        if (e.bytes < bytes) {
            e.buffer.reset();
            e.buffer.alloc(bytes, ("pinned " + std::string(stage) + " bunch").c_str());
            e.bytes = bytes;
        }
        return e.buffer.get();
    }
    // what the call records right behind its copy, in front of the kernels: the next call waits for the copy, not for the stage
    hipEvent_t done(int device) { return entry(device).done.get(); }

private:
    struct Entry { Event done; PinnedBuffer<uint8_t> buffer; size_t bytes = 0; };
    Entry &entry(int device)
    {
        if (!map_mutex_) return entries_[device];
        std::lock_guard<std::mutex> lk(*map_mutex_);
        return entries_[device];
    }
    std::mutex *map_mutex_;
    std::map<int, Entry> entries_;
};

// what every *_device_prepared call checks first; `records`: the input pointer's name, `align`: what it, d_out and d_series are
// aligned to (8, or 16 like the workspace)
inline void check_series_device_args(const char *stage, const char *records, unsigned align, const void *d_records, const void *d_count, size_t capacity,
                                     const void *d_out, const void *d_series, const void *d_counts, const void *d_workspace, size_t workspace_bytes, size_t needed_bytes)
{
    const auto off = [](const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) != 0u; };
    const std::string in(records);
    if (!d_count || !d_counts || !d_workspace) throw Error(CLSIMHIP_ERR_ARGUMENT, "device pointers are (null)");
    if (capacity && (!d_records || !d_out || !d_series)) throw Error(CLSIMHIP_ERR_ARGUMENT, in + " / d_out / d_series is (null)");
    if (capacity > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "capacity beyond 2^32 - 1 records");
    if (off(d_records, align) || off(d_out, align) || off(d_series, align) || off(d_workspace, 16u) || off(d_counts, 4u) || off(d_count, 4u))
        throw Error(CLSIMHIP_ERR_ARGUMENT, align == 16u ? in + ", d_out, d_series and d_workspace must be aligned to 16 bytes, d_count and d_counts to 4"
                                                        : in + ", d_out and d_series must be aligned to 8 bytes, d_workspace to 16, d_count and d_counts to 4");
    if (workspace_bytes < needed_bytes)
        throw Error(CLSIMHIP_ERR_ARGUMENT, "the " + std::string(stage) + " workspace holds " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(needed_bytes) + " are needed");
}

} // namespace clsimhip
