// Frame photons: the detected photons of one bunch -> for every frame, for every module in OMKey order, a sorted series of compressed
// photons (include/clsimhip.h: "Frame photons").  The definition lives here ONCE, as functions both the host twin (frame_photons.cpp)
// and the HIP kernels (frame_photons_kernel.hip) compile.  It restates what the reference does with every photon on a host thread:
//   I3CLSimClientModule::AddPhotonsToFrames        private/clsim/I3CLSimClientModule.cxx:359-439  (particle lookup :388-390,
//                                                   ignoreModules :399, (*frame->photons)[ModuleKey] :407-415)
//   Emit<I3CompressedPhoton>                       :327-349  (the time shift :334, the fields an I3CompressedPhoton keeps)
// Per record: DOM rank in the stage's DOM list (none: UNKNOWN_DOM), particle lookup (UNKNOWN_PARTICLE), mask (MASKED),
// time' = (double)time + shift, one binary64 addition -- mcpe_series.h's series_make_key, on the photon's widened time.  The other
// eight fields are copied bit for bit.
//
// The order.  The reference appends to each (frame, ModuleKey) vector in arrival order, which no two runs repeat.  Here the kept
// records come out ascending in
//     frame rank, module rank, tkey(time'), identifier, h, w0 ... w7
// with w0 ... w7 the eight float fields as uint32 bit patterns in declared order (weight, wavelength, group velocity, x, y, z, theta,
// phi) and h = frame_photons_mix(w), FNV-1a over their 32 bytes.  h decides order, so it is part of the contract.  Records equal in
// all of that are byte-identical: the output is a function of the input as a multiset.
//
// The bound.  A run of records equal in (frame, module, tkey, identifier, h) that holds at least two distinct contents is put in
// order by comparison within the run.  If such a run has more than kFramePhotonsTieBound members, each member is counted as
// TIE_OVERFLOW and the call delivers no records (kept = series = 0).  A run of identical records of any length is fine.
#pragma once
#include <map>
#include <mutex>
#include <vector>

#include "hip_resources.h"
#include "host_model.h"
#include "mcpe_series.h"
#include "series_bunch.h"

namespace clsimhip {

enum FramePhotonsCode : int {
    FRAME_PHOTONS_KEPT = -1, FRAME_PHOTONS_UNKNOWN_PARTICLE = 0, FRAME_PHOTONS_MASKED = 1, FRAME_PHOTONS_UNKNOWN_DOM = 2, FRAME_PHOTONS_TIE_OVERFLOW = 3
};
static_assert((int)FRAME_PHOTONS_KEPT == (int)SERIES_KEPT && (int)FRAME_PHOTONS_UNKNOWN_PARTICLE == (int)SERIES_UNKNOWN_PARTICLE &&
                  (int)FRAME_PHOTONS_MASKED == (int)SERIES_MASKED && (int)FRAME_PHOTONS_UNKNOWN_DOM == (int)SERIES_UNKNOWN_DOM,
              "series_make_key's codes are this stage's");

constexpr uint32_t kFramePhotonsTieBound = 2048u;

// the 80-byte record as five 16-byte groups of four words; the stage reads groups 0, 1, 2 and 4
//   0: x y z time   1: theta phi wavelength cherenkov_dist   2: num_scatters weight identifier (string ID | OM ID << 16)
//   3: start x y z time   4: start_theta start_phi group_velocity dist_in_abs_lens
struct FramePhotonContent { uint32_t w[8]; };

SERIES_HD void frame_photons_content(const uint32_t g0[4], const uint32_t g1[4], const uint32_t g2[4], const uint32_t g4[4], FramePhotonContent &c)
{
    c.w[0] = g2[1]; c.w[1] = g1[2]; c.w[2] = g4[2];             // weight, wavelength, group velocity
    c.w[3] = g0[0]; c.w[4] = g0[1]; c.w[5] = g0[2];             // x, y, z
    c.w[6] = g1[0]; c.w[7] = g1[1];                             // theta, phi
}

// FNV-1a over the 32 bytes of w0 ... w7, each word least significant byte first
SERIES_HD uint32_t frame_photons_mix(const FramePhotonContent &c)
{
    uint32_t h = 2166136261u;
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k) {
#pragma unroll
        for (uint32_t b = 0; b < 4u; ++b) {
            h ^= (c.w[k] >> (8u * b)) & 255u;
            h *= 16777619u;
        }
    }
    return h;
}

// -1 / 0 / +1: a before b, equal, after -- w0 first
SERIES_HD int frame_photons_compare(const FramePhotonContent &a, const FramePhotonContent &b)
{
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k)
        if (a.w[k] != b.w[k]) return a.w[k] < b.w[k] ? -1 : 1;
    return 0;
}

// ---- the device stage (frame_photons_kernel.hip) ----
// header words beside mcpe_series.h's SH_*: the fourth counter, and a second (kept, total) pair for the tile scan over the runs
enum FramePhotonsHeader : uint32_t { FH_TIE_OVERFLOW = 6, FH_RUNS = 40 /* [SH_KEPT]: kept again, [SH_SERIES]: runs */ };

struct FramePhotonsDeviceArgs {
    SeriesLookup lookup;                    // device pointers
    const uint32_t *frames;                 // frame ID by frame rank
    const clsimhip_photon *in;              // 16-byte aligned
    const uint32_t *in_count;               // records = min(*in_count, capacity)
    uint32_t capacity;
    uint32_t *header;                       // kSeriesHeaderWords
    uint32_t *histogram[2];                 // 16 x 256 each: round A's, round B's
    uint32_t *tile_counts;                  // 256 x tiles(capacity)
    uint32_t *run_counts;                   // tiles(capacity): run heads per tile
    SeriesKey *keys[3];                     // round A sorts in 0 and 1, round B in 2 and 0
    SeriesKey *placed;                      // by append position: (group, t_hi, t_lo, source index)
    uint32_t *run_first;                    // by run: its first record
    uint32_t *run_mixed;                    // by run: 1 when two neighbours of it differ in content
    clsimhip_frame_photon *out;
    clsimhip_mcpe_series *series;
    uint32_t *counts;                       // six: kept, series, the four counters
};

// all kernels of the stage, asynchronous on `stream`
hipError_t launch_frame_photons(const FramePhotonsDeviceArgs &A, hipStream_t stream);

// ---- the host side (frame_photons.cpp) ----
size_t frame_photons_blob_bytes(size_t n_particles, size_t n_masked);
size_t frame_photons_workspace_bytes(size_t capacity, size_t n_particles, size_t n_masked);

// The stage's DOM list: the modules a photon may have been detected at, ranked in ascending (string ID signed, OM ID) order -- an
// open-addressing table with the MCPE generator's layout and hash (mcpe_series.h: series_dom_rank), at most half full.
class FramePhotonDoms {
public:
    FramePhotonDoms(const int32_t *string_ids, const uint32_t *om_ids, size_t n);
    ~FramePhotonDoms();
    FramePhotonDoms(const FramePhotonDoms &) = delete;
    FramePhotonDoms &operator=(const FramePhotonDoms &) = delete;
    size_t num_doms() const { return dom_of_rank_.size(); }
    // One bunch's particle table and mask, checked and brought into the form the stage reads (frame_photons_blob_bytes(n_particles,
    // n_masked) bytes at `blob`, 16-byte aligned: table, frame IDs by rank, masked groups -- the MCPE series' layout)
    SeriesBunch prepare(const clsimhip_mcpe_particle *particles, size_t n_particles, const clsimhip_mcpe_mask *masked, size_t n_masked, uint8_t *blob) const;
    // the host twin: std::sort with the full comparator
    void host(const clsimhip_photon *in, size_t n, const clsimhip_mcpe_particle *particles, size_t n_particles, const clsimhip_mcpe_mask *masked,
              size_t n_masked, clsimhip_frame_photon *out, clsimhip_mcpe_series *series, size_t *n_kept, size_t *n_series, uint64_t counters[4]) const;
    // the kernels; the table and the mask are prepared in a page-locked buffer of the object's (one call at a time per object)
    void device(int device, const void *d_photons, const void *d_count, size_t capacity, const clsimhip_mcpe_particle *particles, size_t n_particles,
                const clsimhip_mcpe_mask *masked, size_t n_masked, void *d_out, void *d_series, void *d_counts, void *d_workspace, size_t workspace_bytes,
                hipStream_t stream);
    // the same with a bunch prepared earlier; h_blob must stay as it is until the copy queued on `stream` is over (`uploaded`, if
    // given, is recorded right behind it)
    void device_prepared(int device, const void *d_photons, const void *d_count, size_t capacity, const SeriesBunch &bunch, const uint8_t *h_blob, void *d_out,
                         void *d_series, void *d_counts, void *d_workspace, size_t workspace_bytes, hipStream_t stream, hipEvent_t uploaded = nullptr);

private:
    struct Image { uint64_t *dom_table = nullptr; uint32_t *dom_ranks = nullptr; };
    Image image_on(int device);
    std::vector<uint64_t> dom_table_;       // record word (string ID | OM ID << 16) | 1 << 32; 0 = empty
    std::vector<uint32_t> dom_ranks_;       // beside dom_table_, slot by slot
    std::vector<uint32_t> dom_of_rank_;
    uint32_t dom_mask_ = 0;
    std::mutex device_mutex_, call_mutex_;
    std::map<int, Image> images_;
    SeriesStaging staging_{&device_mutex_}; // of the stand-alone call's bunch (series_bunch.h): calls under call_mutex_, its map under device_mutex_
};

} // namespace clsimhip
