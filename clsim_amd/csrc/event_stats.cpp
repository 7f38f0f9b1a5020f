// Event statistics (event_stats.h): what a bunch's particle table and mask become before any record is looked at, the host twin, the
// weight helper of the C ABI, and the host side of the device stage.  The kernels are in event_stats_kernel.hip.
#include "event_stats.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "series_bunch.h"

namespace clsimhip {

namespace {
// the workspace: header and accumulators (zeroed together by every call), the bunch's blob
struct EventStatsWorkspace {
    size_t slots, blob, bytes;
    EventStatsWorkspace(size_t n_particles, size_t blob_bytes)
    {
        slots = kEventStatsHeaderWords * sizeof(uint32_t);
        blob = round16(slots + std::max<size_t>(n_particles, 1u) * kEventStatsSlots * sizeof(uint64_t));
        bytes = blob + round16(blob_bytes);
    }
};

// the table part of the blob is the series stages', without a mask
size_t table_bytes(size_t n_particles) { return round16(series_blob_bytes(n_particles, 0)); }

// where the stage's inputs are, with the blob wherever it lives
void set_lookup(EventStatsDeviceArgs &A, const SeriesBunch &B, const uint8_t *blob)
{
    A.particles = B.have_table ? reinterpret_cast<const SeriesParticle *>(blob) : nullptr;
    A.frames = reinterpret_cast<const uint32_t *>(blob + B.frames_offset);
    A.masked = reinterpret_cast<const uint64_t *>(blob + B.masked_offset);
    A.n_particles = B.n_particles; A.n_masked = B.n_masked;
    A.consecutive = B.consecutive ? 1u : 0u;
    A.records = B.have_table ? B.n_particles : 1u;
}

// what every device call checks first, in the style of series_bunch.h's check_series_device_args: pointers, alignment, the workspace
void check_device_args(const void *d_steps, size_t n_steps, const void *d_photons, const void *d_count, size_t capacity, size_t records, const void *d_out,
                       const void *d_counters, const void *d_workspace, size_t workspace_bytes, size_t needed_bytes)
{
    const auto off = [](const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) != 0u; };
    if (!d_count || !d_counters || !d_workspace) throw Error(CLSIMHIP_ERR_ARGUMENT, "device pointers are (null)");
    if ((n_steps && !d_steps) || (capacity && !d_photons) || (records && !d_out)) throw Error(CLSIMHIP_ERR_ARGUMENT, "d_steps / d_photons / d_out is (null)");
    if (n_steps > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "more than 2^32 - 1 steps");
    if (capacity > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "capacity beyond 2^32 - 1 records");
    if (off(d_steps, 4u) || off(d_photons, 4u) || off(d_out, 8u) || off(d_workspace, 16u) || off(d_counters, 4u) || off(d_count, 4u))
        throw Error(CLSIMHIP_ERR_ARGUMENT, "d_steps and d_photons must be aligned to 4 bytes, d_out to 8, d_workspace to 16, d_count and d_counters to 4");
    if (workspace_bytes < needed_bytes)
        throw Error(CLSIMHIP_ERR_ARGUMENT, "the event statistics workspace holds " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(needed_bytes) + " are needed");
}

// the stand-alone call's staging (series_bunch.h), one call at a time
std::mutex g_call_mutex, g_map_mutex;
SeriesStaging &staging()
{
    static SeriesStaging *s = new SeriesStaging(&g_map_mutex);     // (lives as long as the process: no HIP call at exit)
    return *s;
}
} // namespace

size_t event_stats_blob_bytes(size_t n_particles, size_t n_masked) { return table_bytes(n_particles) + round16(n_masked * sizeof(uint64_t)) + 16u; }

size_t event_stats_workspace_bytes(size_t n_particles, size_t n_masked)
{
    return EventStatsWorkspace(n_particles, event_stats_blob_bytes(n_particles, n_masked)).bytes;
}

SeriesBunch event_stats_prepare(const clsimhip_mcpe_particle *particles, size_t n_particles, const clsimhip_mcpe_mask *masked, size_t n_masked, uint8_t *blob)
{
    if (n_masked && !masked) throw Error(CLSIMHIP_ERR_ARGUMENT, "masked is (null)");
    if (n_masked > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "more than 2^32 - 1 particles or masked modules");
    // the table part: checked, ranked by frame (one group per frame: the 32-bit bound is on the frames alone)
    SeriesBunch B = prepare_series_bunch(particles, n_particles, nullptr, 0, blob, 1u, "event statistics", "groups", [](uint32_t, uint32_t) -> int64_t { return -1; });
    // the mask: frame rank << 32 | record word, ascending and distinct; what names no frame of the table is ignored
    const uint32_t *frames = reinterpret_cast<const uint32_t *>(blob + B.frames_offset);
    B.masked_offset = table_bytes(n_particles);
    B.bytes = event_stats_blob_bytes(n_particles, n_masked);
    uint64_t *keys = reinterpret_cast<uint64_t *>(blob + B.masked_offset);
    size_t kept = 0;
    for (size_t i = 0; i < n_masked; ++i) {
        const uint32_t *f = std::lower_bound(frames, frames + B.n_frames, masked[i].frame);
        if (f == frames + B.n_frames || *f != masked[i].frame || (B.have_table && n_particles == 0)) continue;
        keys[kept++] = (static_cast<uint64_t>(f - frames) << 32) | record_word(masked[i].string_id, masked[i].om_id);
    }
    std::sort(keys, keys + kept);
    B.n_masked = static_cast<uint32_t>(std::unique(keys, keys + kept) - keys);
    return B;
}

void event_stats_host(const clsimhip_step *steps, size_t n_steps, const clsimhip_photon *photons, size_t n_photons, const clsimhip_mcpe_particle *particles,
                      size_t n_particles, const clsimhip_mcpe_mask *masked, size_t n_masked, clsimhip_event_statistics *out, uint64_t counters[3])
{
    if ((n_steps && !steps) || (n_photons && !photons)) throw Error(CLSIMHIP_ERR_ARGUMENT, "steps / photons is (null)");
    if (n_steps > 0xffffffffull || n_photons > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "more than 2^32 - 1 records");
    std::vector<SeriesParticle> aligned((event_stats_blob_bytes(n_particles, n_masked) + sizeof(SeriesParticle) - 1u) / sizeof(SeriesParticle));
    uint8_t *blob = reinterpret_cast<uint8_t *>(aligned.data());
    const SeriesBunch B = event_stats_prepare(particles, n_particles, masked, n_masked, blob);
    EventStatsDeviceArgs A{};
    set_lookup(A, B, blob);
    if (A.records && !out) throw Error(CLSIMHIP_ERR_ARGUMENT, "out is (null)");
    std::vector<uint64_t> slots(static_cast<size_t>(A.records) * kEventStatsSlots, 0u);
    uint64_t counts[3] = {0, 0, 0};
    const auto record_of = [&](uint32_t identifier) -> int64_t {
        return A.particles ? series_find_particle(A.particles, A.n_particles, A.consecutive != 0u, identifier) : 0;
    };
    const auto add = [&](uint32_t side, int64_t record, const EventStatsTerm &t, uint64_t count) {
        uint64_t *acc = slots.data() + static_cast<size_t>(record) * kEventStatsSlots;
        acc[kEventStatsCounts + side] += count;
        if (t.kind != ES_FINITE) { ++acc[kEventStatsSpecial + 3u * side + (t.kind - 1u)]; return; }
        for (uint32_t k = 0; k < 3u; ++k) acc[event_stats_limb_slot(side, t.negative, t.position + k)] += t.limb[k];
    };
    for (size_t i = 0; i < n_steps; ++i) {
        uint32_t w[12];                                                     // (the record is packed: no word of it is read in place)
        std::memcpy(w, steps + i, sizeof w);
        const int64_t record = record_of(w[10]);
        if (record < 0) { ++counts[CLSIMHIP_EVENT_STATISTICS_UNKNOWN_STEP_PARTICLE]; continue; }      // ClientModule.cxx:514
        EventStatsTerm t;
        event_stats_term(w[9], w[8], true, t);
        add(ES_GENERATED, record, t, w[8]);
    }
    for (size_t i = 0; i < n_photons; ++i) {
        uint32_t w[20];
        std::memcpy(w, photons + i, sizeof w);
        const int64_t record = record_of(w[10]);
        if (record < 0) { ++counts[CLSIMHIP_EVENT_STATISTICS_UNKNOWN_PARTICLE]; continue; }           // :388-390
        const uint32_t frame_rank = A.particles ? A.particles[record].frame_rank : 0u;
        if (event_stats_is_masked(A.masked, A.n_masked, (static_cast<uint64_t>(frame_rank) << 32) | w[11])) {     // :399
            ++counts[CLSIMHIP_EVENT_STATISTICS_MASKED];
            continue;
        }
        EventStatsTerm t;
        event_stats_term(w[9], 1u, false, t);
        add(ES_AT_DOMS, record, t, 1u);
    }
    for (uint32_t r = 0; r < A.records; ++r) {
        uint32_t identifier = 0u, frame = 0u;
        if (A.particles) { identifier = A.particles[r].identifier; frame = A.frames[A.particles[r].frame_rank]; }
        std::memset(out + r, 0, sizeof out[r]);
        event_stats_close(slots.data() + static_cast<size_t>(r) * kEventStatsSlots, identifier, frame, out[r]);
    }
    if (counters) std::memcpy(counters, counts, sizeof counts);
}

double event_stats_weight(const uint64_t words[6], const uint32_t special[3])
{
    if (!words || !special || special[2] != 0u || (special[0] != 0u && special[1] != 0u)) return std::numeric_limits<double>::quiet_NaN();     // 0x7ff8000000000000
    if (special[0] != 0u) return std::numeric_limits<double>::infinity();
    if (special[1] != 0u) return -std::numeric_limits<double>::infinity();
    // the magnitude
    const bool negative = (words[5] >> 63) != 0u;
    uint64_t mag[6];
    uint64_t carry = negative ? 1u : 0u;
    for (int k = 0; k < 6; ++k) {
        const uint64_t v = negative ? ~words[k] : words[k];
        mag[k] = v + carry;
        carry = (carry && mag[k] == 0u) ? 1u : 0u;
    }
    int top = -1;                                                           // its highest set bit
    for (int k = 5; k >= 0 && top < 0; --k)
        if (mag[k]) top = 64 * k + 63 - __builtin_clzll(mag[k]);
    if (top < 0) return 0.0;
    const auto bit = [&](int i) { return (mag[i >> 6] >> (i & 63)) & 1u; };
    // the top 53 bits, then one rounding to nearest, ties to even, on the bit below them and everything below that
    const int low = top > 52 ? top - 52 : 0;
    uint64_t q = 0u;
    for (int i = top; i >= low; --i) q = (q << 1) | bit(i);
    if (low > 0) {
        bool sticky = false;
        for (int i = low - 2; i >= 0 && !sticky; --i) sticky = bit(i) != 0u;
        if (bit(low - 1) && (sticky || (q & 1u))) ++q;                      // (2^53 is a binary64 too)
    }
    const double value = std::ldexp(static_cast<double>(q), low - 149);    // exact: q <= 2^53, exponents within [-149, 234]
    return negative ? -value : value;
}

void event_stats_device(int device, const void *d_steps, size_t n_steps, const void *d_photons, const void *d_count, size_t capacity,
                        const clsimhip_mcpe_particle *particles, size_t n_particles, const clsimhip_mcpe_mask *masked, size_t n_masked, void *d_out, void *d_counters,
                        void *d_workspace, size_t workspace_bytes, hipStream_t stream)
{
    // (what can be refused without a device is refused first)
    if (n_particles > 0xffffffffull || n_masked > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "more than 2^32 - 1 particles or masked modules");
    if (n_particles && !particles) throw Error(CLSIMHIP_ERR_ARGUMENT, "particles is (null)");
    if (n_masked && !masked) throw Error(CLSIMHIP_ERR_ARGUMENT, "masked is (null)");
    check_device_args(d_steps, n_steps, d_photons, d_count, capacity, particles ? n_particles : 1u, d_out, d_counters, d_workspace, workspace_bytes,
                      event_stats_workspace_bytes(n_particles, n_masked));
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) throw Error(CLSIMHIP_ERR_DEVICE, "no HIP device available (the event statistics' device path has no CPU fallback)");
    if (device < 0 || device >= count) throw Error(CLSIMHIP_ERR_ARGUMENT, "device ordinal out of range");
    DeviceGuard on_device(device);
    // one call at a time prepares its bunch in the staging buffer: the previous call's copy has to be over
    std::lock_guard<std::mutex> lk(g_call_mutex);
    uint8_t *blob = staging().acquire(device, event_stats_blob_bytes(n_particles, n_masked), "event statistics");
    const SeriesBunch B = event_stats_prepare(particles, n_particles, masked, n_masked, blob);
    event_stats_device_prepared(device, d_steps, n_steps, d_photons, d_count, capacity, B, blob, d_out, d_counters, d_workspace, workspace_bytes, stream,
                                staging().done(device));
}

void event_stats_device_prepared(int device, const void *d_steps, size_t n_steps, const void *d_photons, const void *d_count, size_t capacity, const SeriesBunch &B,
                                 const uint8_t *h_blob, void *d_out, void *d_counters, void *d_workspace, size_t workspace_bytes, hipStream_t stream, hipEvent_t uploaded)
{
    const EventStatsWorkspace W(B.n_particles, B.bytes);
    const size_t records = B.have_table ? B.n_particles : 1u;
    check_device_args(d_steps, n_steps, d_photons, d_count, capacity, records, d_out, d_counters, d_workspace, workspace_bytes, W.bytes);
    DeviceGuard on_device(device);
    uint8_t *ws = static_cast<uint8_t *>(d_workspace);
    hip_check(hipMemcpyAsync(ws + W.blob, h_blob, B.bytes, hipMemcpyHostToDevice, stream), "upload event statistics bunch");
    if (uploaded) hip_check(hipEventRecord(uploaded, stream), "event");
    EventStatsDeviceArgs A{};
    set_lookup(A, B, ws + W.blob);
    A.steps = static_cast<const clsimhip_step *>(d_steps);
    A.n_steps = static_cast<uint32_t>(n_steps);
    A.photons = static_cast<const clsimhip_photon *>(d_photons);
    A.photon_count = static_cast<const uint32_t *>(d_count);
    A.capacity = static_cast<uint32_t>(capacity);
    A.header = reinterpret_cast<uint32_t *>(ws);
    A.slots = reinterpret_cast<uint64_t *>(ws + W.slots);
    A.out = static_cast<clsimhip_event_statistics *>(d_out);
    A.counters = static_cast<uint32_t *>(d_counters);
    const hipError_t e = launch_event_stats(A, stream);
    if (e != hipSuccess) throw Error(CLSIMHIP_ERR_DEVICE, std::string("event statistics kernel launch: ") + hipGetErrorString(e));
}

} // namespace clsimhip
