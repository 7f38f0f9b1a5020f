// MCPE series: the MCPEs of one bunch -> for every frame, for every DOM in OMKey order, a time-ordered series
// (include/clsimhip.h: "MCPE series").  The definition lives here ONCE, as functions both the host twin (mcpe_series.cpp) and the
// HIP kernels (mcpe_series_kernel.hip) compile.  It restates what the reference's client module does with every MCPE on a host
// thread:
//   I3CLSimClientModule::AddPhotonsToFrames        private/clsim/I3CLSimClientModule.cxx:359-439  (particle lookup, ignoreModules,
//                                                   time shift, (*frame->hits)[omkey])
//   std::sort(hits, MCPETimeLess)                  private/clsim/dom/I3PhotonToMCPEConverter.cxx:524-526
//   I3MCPESeriesMap in key order                   I3CLSimClientModule.cxx:710-719
// Per record: DOM rank (no rank: UNKNOWN_DOM, which the hit maker's records cannot meet), particle lookup (UNKNOWN_PARTICLE), mask
// (MASKED), time' = time + shift (one binary64 addition), key = (group, tkey, identifier) with group = frame rank x DOMs + DOM
// rank; the output is ascending in that 128-bit integer key, so it is a function of the input as a multiset.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/clsimhip.h"

namespace clsimhip {

#define SERIES_HD __host__ __device__ __forceinline__

enum SeriesCode : int { SERIES_KEPT = -1, SERIES_UNKNOWN_PARTICLE = 0, SERIES_MASKED = 1, SERIES_UNKNOWN_DOM = 2 };

// what one bunch's particle table and mask become before any record is looked at (built on the host, in the caller's thread)
struct SeriesParticle { uint32_t identifier, frame_rank; double time_shift; };      // ascending in identifier

struct alignas(16) SeriesKey { uint32_t group; uint32_t t_hi, t_lo; uint32_t identifier; };        // most significant first; 16 bytes

// the order-preserving image of a binary64: a total order on bit patterns (-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN)
SERIES_HD uint64_t series_tkey(double t)
{
    const uint64_t b = __builtin_bit_cast(uint64_t, t);
    return b ^ ((b >> 63) ? ~0ull : (1ull << 63));
}
SERIES_HD double series_time_of(uint64_t tkey)
{
    const uint64_t b = tkey ^ ((tkey >> 63) ? (1ull << 63) : ~0ull);
    return __builtin_bit_cast(double, b);
}

// digit `pass` (0 = least significant byte) of the 128-bit key
SERIES_HD uint32_t series_digit(const SeriesKey &k, uint32_t pass)
{
    const uint32_t word = pass < 4u ? k.identifier : pass < 8u ? k.t_lo : pass < 12u ? k.t_hi : k.group;
    return (word >> ((pass & 3u) * 8u)) & 255u;
}

// rank of the DOM in ascending (string ID signed, OM ID) order, from the generator's open-addressing table (mcpe.h: dom_table) and
// the ranks stored beside it slot by slot; -1: the generator has no such DOM.  `word` = string ID | OM ID << 16, as in the records.
SERIES_HD int64_t series_dom_rank(const uint64_t *table, const uint32_t *ranks, uint32_t mask, uint32_t word)
{
    uint32_t slot = ((word * 2654435761u) >> 7) & mask;                 // mcpe_dom_slot
    for (;;) {
        const uint64_t e = table[slot];
        if (e == 0u) return -1;
        if ((uint32_t)e == word) return (int64_t)ranks[slot];
        slot = (slot + 1u) & mask;
    }
}

// index of `identifier` in the table, or -1.  consecutive: identifiers first, first + 1, ... (the client module's), one subtraction
SERIES_HD int64_t series_find_particle(const SeriesParticle *table, uint32_t n, bool consecutive, uint32_t identifier)
{
    if (n == 0u) return -1;
    if (consecutive) {
        const uint32_t k = identifier - table[0].identifier;
        return k < n ? (int64_t)k : -1;
    }
    uint32_t lo = 0u, hi = n;                                           // first entry >= identifier
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (table[mid].identifier < identifier) lo = mid + 1u; else hi = mid;
    }
    return (lo < n && table[lo].identifier == identifier) ? (int64_t)lo : -1;
}

SERIES_HD bool series_is_masked(const uint32_t *masked_groups, uint32_t n, uint32_t group)     // ascending, distinct
{
    uint32_t lo = 0u, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (masked_groups[mid] < group) lo = mid + 1u; else hi = mid;
    }
    return lo < n && masked_groups[lo] == group;
}

struct SeriesLookup {                       // one bunch's prepared inputs, wherever they live
    const SeriesParticle *particles;        // null: no table -- every identifier is frame rank 0, shift 0
    const uint32_t *masked_groups;
    const uint64_t *dom_table;
    const uint32_t *dom_ranks;
    uint32_t n_particles, n_masked, dom_mask, n_doms;
    uint32_t consecutive, reserved;
};

// one MCPE -> SERIES_KEPT and its key, or the counter it belongs to
SERIES_HD int series_make_key(const SeriesLookup &L, uint32_t identifier, uint32_t dom_word, double time, SeriesKey &key)
{
    const int64_t rank = series_dom_rank(L.dom_table, L.dom_ranks, L.dom_mask, dom_word);
    if (rank < 0) return SERIES_UNKNOWN_DOM;
    uint32_t frame_rank = 0u;
    double shift = 0.;
    if (L.particles) {
        const int64_t p = series_find_particle(L.particles, L.n_particles, L.consecutive != 0u, identifier);
        if (p < 0) return SERIES_UNKNOWN_PARTICLE;                      // ClientModule.cxx:388-390
        frame_rank = L.particles[p].frame_rank;
        shift = L.particles[p].time_shift;
    }
    const uint32_t group = frame_rank * L.n_doms + (uint32_t)rank;      // (< 2^32: checked when the bunch is prepared)
    if (series_is_masked(L.masked_groups, L.n_masked, group)) return SERIES_MASKED;     // :399
    const uint64_t t = series_tkey(time + shift);                       // :334
    key.group = group;
    key.t_hi = (uint32_t)(t >> 32);
    key.t_lo = (uint32_t)t;
    key.identifier = identifier;
    return SERIES_KEPT;
}

// ---- the device stage (mcpe_series_kernel.hip) ----
constexpr uint32_t kSeriesTile = 2048u;     // keys per workgroup and digit pass: 256 lanes x 8
constexpr uint32_t kSeriesHeaderWords = 64u;
// header words (uint32) at the start of the workspace
enum SeriesHeader : uint32_t {
    SH_KEPT = 0, SH_SERIES = 1, SH_COUNTERS = 2 /* 3 of them */, SH_FINAL = 5 /* 0 / 1: the buffer the sorted keys are in */,
    SH_LIVE = 8 /* 16: pass is live */, SH_SOURCE = 24 /* 16: the buffer pass p reads */
};

struct SeriesDeviceArgs {
    SeriesLookup lookup;                    // device pointers
    const uint32_t *frames;                 // frame ID by frame rank (null: frame 0)
    const uint32_t *dom_of_rank;            // record word (string ID | OM ID << 16) by DOM rank
    const clsimhip_mcpe *in;
    const uint32_t *in_count;               // records = min(*in_count, capacity)
    uint32_t capacity;
    uint32_t *header;                       // kSeriesHeaderWords
    uint32_t *histogram;                    // 16 x 256
    uint32_t *tile_counts;                  // 256 x tiles(capacity), digit major over the tiles in use
    SeriesKey *keys[2];
    clsimhip_mcpe *out;
    clsimhip_mcpe_series *series;
    uint32_t *counts;                       // five: kept, series, the three counters
};

// all kernels of the stage, asynchronous on `stream`
hipError_t launch_mcpe_series(const SeriesDeviceArgs &A, hipStream_t stream);

// Two pieces of the stage the MCPE merging stage (mcpe_merge.h) uses on keys of its own, with header, histogram, tile_counts, keys
// and capacity of A filled in: header[SH_KEPT] keys in keys[0] and their 16 x 256 digit histogram -> the plan and all live passes
// (the sorted keys are in keys[header[SH_FINAL]]); one count per tile of header[SH_KEPT] keys in tile_counts -> their exclusive
// scan, the total in header[SH_SERIES].
void launch_series_sort(const SeriesDeviceArgs &A, hipStream_t stream);
void launch_series_tile_scan(const SeriesDeviceArgs &A, hipStream_t stream);

} // namespace clsimhip
