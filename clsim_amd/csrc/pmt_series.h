// PMT series: the hits of one bunch -> for every frame, for every module in OMKey order, for every PMT in ascending number, a
// time-ordered series (include/clsimhip.h: "PMT series").  The definition lives here ONCE, as functions both the host twin
// (pmt_series.cpp) and the HIP kernels (pmt_series_kernel.hip) compile.  It restates what the reference does with every hit on host
// threads:
//   I3CLSimClientModule::AddPhotonsToFrames        private/clsim/I3CLSimClientModule.cxx:359-439  (particle lookup, ignoreModules,
//                                                   time shift)
//   I3PhotonToMCHitConverterForMultiPMT::DAQ       private/clsim/dom/I3PhotonToMCHitConverterForMultiPMT.cxx:291-292, 365
//                                                   ((*outputMap)[omkey][pmt]: I3MCHitSeriesMultiOMMap, a map of maps)
//   std::sort per PMT                              :387-395
// Per record: module rank and channel = base[module rank] + pmt (no module, or pmt >= the type's PMTs: UNKNOWN_CHANNEL, which the hit
// maker's records cannot meet), particle lookup (UNKNOWN_PARTICLE), mask per (frame, module) (MASKED), time' = time + shift (one
// binary64 addition), key = (group, tkey, identifier) with group = frame rank x channels + channel: mcpe_series.h's SeriesKey, so the
// radix passes are mcpe_series_kernel.hip's; the output is ascending in that 128-bit integer key and a function of the input as a
// multiset.
#pragma once
#include "mcpe_series.h"
#include "pmt_hits.h"

namespace clsimhip {

enum PmtSeriesCode : int { PMT_SERIES_KEPT = -1, PMT_SERIES_UNKNOWN_PARTICLE = 0, PMT_SERIES_MASKED = 1, PMT_SERIES_UNKNOWN_CHANNEL = 2 };

struct PmtSeriesLookup {                    // one bunch's prepared inputs, wherever they live
    const SeriesParticle *particles;        // null: no table -- every identifier is frame rank 0, shift 0
    const uint32_t *masked_modules;         // frame rank x modules + module rank, ascending, distinct
    const uint64_t *module_table;           // the generator's (pmt_hits.h)
    const uint32_t *module_ranks;           // beside the table slot by slot: rank in ascending (string ID signed, OM ID) order
    const uint32_t *channel_bases;          // beside the table slot by slot: base[rank]
    const uint32_t *base;                   // by module rank, modules + 1 entries: exclusive prefix sum of the types' PMT counts
    uint32_t n_particles, n_masked, module_mask, n_modules;
    uint32_t n_channels, consecutive;
};

// slot of the module in the generator's open-addressing table, or -1.  `word` = string ID | OM ID << 16, as in the records.
SERIES_HD int64_t pmt_series_module_slot(const uint64_t *table, uint32_t mask, uint32_t word)
{
    uint32_t slot = mcpe_dom_slot(word, mask);
    for (;;) {                                                          // (at most half full: an empty entry ends every probe)
        const uint64_t e = table[slot];
        if (e == 0u) return -1;
        if ((uint32_t)e == word) return (int64_t)slot;
        slot = (slot + 1u) & mask;
    }
}

// module rank of a channel: the last rank whose base is <= channel (base[0] = 0, base[n_modules] = channels > channel)
SERIES_HD uint32_t pmt_series_rank_of_channel(const uint32_t *base, uint32_t n_modules, uint32_t channel)
{
    uint32_t lo = 0u, hi = n_modules;                                   // first rank whose base is > channel, in (0, n_modules]
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (base[mid] <= channel) lo = mid + 1u; else hi = mid;
    }
    return lo - 1u;
}

// one hit -> PMT_SERIES_KEPT and its key, or the counter it belongs to
SERIES_HD int pmt_series_make_key(const PmtSeriesLookup &L, uint32_t identifier, uint32_t module_word, uint32_t pmt, double time, SeriesKey &key)
{
    const int64_t slot = pmt_series_module_slot(L.module_table, L.module_mask, module_word);
    if (slot < 0) return PMT_SERIES_UNKNOWN_CHANNEL;
    const uint32_t rank = L.module_ranks[slot], first = L.channel_bases[slot];
    if (pmt >= L.base[rank + 1u] - first) return PMT_SERIES_UNKNOWN_CHANNEL;
    uint32_t frame_rank = 0u;
    double shift = 0.;
    if (L.particles) {
        const int64_t p = series_find_particle(L.particles, L.n_particles, L.consecutive != 0u, identifier);
        if (p < 0) return PMT_SERIES_UNKNOWN_PARTICLE;                  // ClientModule.cxx:388-390
        frame_rank = L.particles[p].frame_rank;
        shift = L.particles[p].time_shift;
    }
    // (both products < 2^32: checked when the bunch is prepared, and modules <= channels)
    if (series_is_masked(L.masked_modules, L.n_masked, frame_rank * L.n_modules + rank)) return PMT_SERIES_MASKED;      // :399
    const uint64_t t = series_tkey(time + shift);                       // :334
    key.group = frame_rank * L.n_channels + (first + pmt);
    key.t_hi = (uint32_t)(t >> 32);
    key.t_lo = (uint32_t)t;
    key.identifier = identifier;
    return PMT_SERIES_KEPT;
}

// ---- the device stage (pmt_series_kernel.hip) ----
struct PmtSeriesDeviceArgs {
    PmtSeriesLookup lookup;                 // device pointers
    const uint32_t *frames;                 // frame ID by frame rank
    const uint32_t *module_of_rank;         // record word (string ID | OM ID << 16) by module rank
    const clsimhip_pmt_hit *in;
    const uint32_t *in_count;               // records = min(*in_count, capacity)
    uint32_t capacity;
    uint32_t *header;                       // kSeriesHeaderWords (mcpe_series.h: SH_*)
    uint32_t *histogram;                    // 16 x 256
    uint32_t *tile_counts;                  // 256 x tiles(capacity)
    SeriesKey *keys[2];
    clsimhip_pmt_hit *out;
    clsimhip_pmt_series *series;
    uint32_t *counts;                       // five: kept, series, the three counters
};

// all kernels of the stage, asynchronous on `stream`
hipError_t launch_pmt_series(const PmtSeriesDeviceArgs &A, hipStream_t stream);

} // namespace clsimhip
