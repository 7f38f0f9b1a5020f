// PMT photon hits: stored frame photons (include/clsimhip.h: clsimhip_frame_photon with a series table) -> per-frame, per-module,
// per-PMT time-sorted hits of segmented modules.  The multi-PMT counterpart of photon_hits.h: photons are propagated once and stored,
// hits are made from them as often as needed, with another quantum efficiency, collection efficiency or angular acceptance each time.
// The definition lives here ONCE, as a function both the host twin (pmt_photon_hits.cpp) and the HIP kernels
// (pmt_photon_hits_kernel.hip) compile: binary64 + - * / in the order written, no contraction (-ffp-contract=off, Makefile), so x86-64
// and gfx950 give the same bits.  It restates
//   I3PhotonToMCHitConverterForMultiPMT::DAQ        private/clsim/dom/I3PhotonToMCHitConverterForMultiPMT.cxx:244-407
//     the stored I3PhotonSeriesMap, module by module :262-283      FindHitPMT                         :111-227
//     the probability and the draw                   :319-353      the hit under OMKey and PMT number :362-382
//     the per-PMT time sort                          :387-395
// with pmt_hits.h's tables and generator, mcpe.h's sin / cos pair, hash, table evaluation and module lookup and mcpe_series.h's time
// key, which it includes and does not repeat.
//
// The geometry and the probability are pmt_make's (pmt_hits.h:83-123), on the frame record's fields.  They are stated a second time
// here, in pmt_photon_hit_probability, and NOT shared with pmt_make: with the body factored out of pmt_make into one inline function,
// pmt_hits_kernel compiled to other instructions (1 306 against 1 354), and that kernel is to keep its code.  The tests hold the two
// together: for draw-free input the online path and this one give the same hits (tests/test_pmt_photon_hits.py, the bridge).
// The NaN rules are pmt_make's: comparisons with a NaN are false, a NaN direction skips no PMT and ends on the type's last one, a NaN
// weight or P passes both P > 1 and P <= u and yields a hit.
//
// What differs from the reference, on purpose:
//   the draw:     the reference takes one number per photon from an I3RandomService in arrival order (:353).  Here u is a hash of
//                 the record's 48 bytes and the generator's seed: the result does not depend on the order of the input, and with one
//                 seed the hits made at a lower collection efficiency are a subset of those made at a higher one;
//   the order:    std::sort(MCHitTimeLess) leaves hits with equal times in any order (:387-395).  Here the kept hits are ascending in
//                 (series, PMT, tkey(time), identifier) -- mcpe_series.h's total order on the time's bit pattern -- and hits equal in
//                 that are byte-identical;
//   glass / gel:  the path-length argument of GetGlassGelSurvivalProbability (:328) is not modelled, as in pmt_hits.h;
//   the MCTree:   the lookup of the photon's particle in the MCTree (:356-360) is the caller's: the hit carries the identifier;
//   the time:     the hit's time is the record's, bit for bit (:372).  It already carries the particle's shift.
#pragma once
#include "mcpe.h"
#include "mcpe_series.h"
#include "pmt_hits.h"
#include "photon_hits.h"        // photon_hit_series_of

namespace clsimhip {

// result of one record: a key (KEPT), nothing (DROPPED: no PMT met from the front, or the draw), or the counter it belongs to, in
// the order of include/clsimhip.h's CLSIMHIP_PMT_PHOTON_HITS_*.  OFF_SURFACE is not a result: the record goes on.
enum PmtPhotonHitCode : int {
    PMT_PHOTON_HIT_KEPT = -1, PMT_PHOTON_HIT_UNCOVERED = 0, PMT_PHOTON_HIT_SERIES_MISMATCH = 1, PMT_PHOTON_HIT_UNKNOWN_MODULE = 2,
    PMT_PHOTON_HIT_PROBABILITY_ABOVE_ONE = 3, PMT_PHOTON_HIT_OFF_SURFACE = 4, PMT_PHOTON_HIT_DROPPED = 5
};
constexpr int kPmtPhotonHitCounters = 5;
// group = series x 64 + PMT number must fit 32 bits
constexpr uint64_t kPmtPhotonHitMaxSeries = uint64_t{1} << 26;
static_assert(kPmtMaxPerType == 64, "a key's group is series x 64 + PMT number");

struct PmtPhotonHitLookup {                 // the input's series table, wherever it lives
    const clsimhip_mcpe_series *series;
    uint32_t n_series, reserved;
};

// pmt_make's lines 83-123 on the fields of a record at the module M of type T (position relative to the module centre) ->
// PMT_ACCEPTED with the PMT `found` and the probability `prob` for the draw, PMT_DROPPED or PMT_PROBABILITY_ABOVE_ONE.
// off_surface: the record reached the surface check (:139) and is outside the window.
template <class Values, class Pmts>
MCPE_HD int pmt_photon_hit_probability(const PmtHitParams &P, Values values, Pmts pmts, const PmtModule &M, const PmtType &T, float x, float y, float z,
                                       float theta, float phi, float wavelength, float weight, int &found, double &prob, bool &off_surface)
{
    const double px = (double)x, py = (double)y, pz = (double)z;
    float st, ct, sp, cp;
    mcpe_sincos(theta, st, ct);
    mcpe_sincos(phi, sp, cp);
    const double dx = (double)st * (double)cp, dy = (double)st * (double)sp, dz = (double)ct;
    const double dot = px * dx + py * dy + pz * dz;                     // :132
    if (dot > 0.) return PMT_DROPPED;                                   // :133-136: the photon is leaving
    const double pr2 = px * px + py * py + pz * pz;
    off_surface = !(T.lo2 <= pr2 && pr2 <= T.hi2);                      // :139-145, without the square root; goes on
    found = -1;
    double path = 0., rx = 0., ry = 0., rz = 0.;
    for (int i = 0; i < T.count; ++i) {
        const PmtEntry &E = pmts[T.first + i];
        const double nx = (M.m[0] * E.n[0] + M.m[1] * E.n[1]) + M.m[2] * E.n[2];       // :167
        const double ny = (M.m[3] * E.n[0] + M.m[4] * E.n[1]) + M.m[5] * E.n[2];
        const double nz = (M.m[6] * E.n[0] + M.m[7] * E.n[1]) + M.m[8] * E.n[2];
        const double denom = dx * nx + dy * ny + dz * nz;               // :175
        if (denom >= 1e-8) continue;                                    // :177: towards the PMT's back
        const double ax = (M.m[0] * E.a[0] + M.m[1] * E.a[1]) + M.m[2] * E.a[2];       // :185
        const double ay = (M.m[3] * E.a[0] + M.m[4] * E.a[1]) + M.m[5] * E.a[2];
        const double az = (M.m[6] * E.a[0] + M.m[7] * E.a[1]) + M.m[8] * E.a[2];
        const double mu = ((ax - px) * nx + (ay - py) * ny + (az - pz) * nz) / denom;  // :193
        if (mu < 0.) continue;                                          // :195: moving away from the PMT
        const double ex = ax - px - mu * dx, ey = ay - py - mu * dy, ez = az - pz - mu * dz;
        const double dist2 = ex * ex + ey * ey + ez * ez;               // :199-202
        if (dist2 > E.radius2) continue;                                // :204
        // :207-217: a later intersection replaces an earlier one only if it is closer (or the earlier path length is a NaN)
        if (found >= 0 && !(path != path || mu < path)) continue;
        found = i; path = mu;
        rx = nx; ry = ny; rz = nz;
    }
    if (found < 0) return PMT_DROPPED;                                  // :308
    const double c = -(rx * dx + ry * dy + rz * dz);                    // :319-321, the cosine of hit_angle
    if (c <= 0.) return PMT_DROPPED;                                    // :323: a flat disc cannot be hit from behind
    const PmtEntry &E = pmts[T.first + found];
    const double wlen = (double)wavelength;
    prob = (double)weight;                                              // :343-346
    prob *= mcpe_acceptance(P.functions[T.g], values, wlen);
    prob *= mcpe_acceptance(P.functions[E.q], values, wlen) * E.ce;
    prob *= mcpe_acceptance(P.functions[E.acceptance], values, c) / c;
    if (prob > 1.) return PMT_PROBABILITY_ABOVE_ONE;                    // :348-351
    return PMT_ACCEPTED;
}

// Record i (its 12 words: identifier, string ID | OM ID << 16, the time's two words, then weight, wavelength, group velocity, x, y,
// z, theta, phi) -> PmtPhotonHitCode; `key` and `pmt` are written when the code is PMT_PHOTON_HIT_KEPT (the hit is {w[0], the
// entry's IDs, pmt, 0, the record's time}: the key holds all of it).  P: the generator's functions, types, module table and seed;
// `values` / `pmts`: the function values and PMT tables, wherever the caller keeps them (LDS in the kernel).
template <class Values, class Pmts>
MCPE_HD int pmt_photon_hit_make(const PmtPhotonHitLookup &L, const PmtHitParams &P, Values values, Pmts pmts, uint32_t i, const uint32_t *w, SeriesKey &key,
                                uint32_t &pmt, bool &off_surface)
{
    off_surface = false;
    const int64_t s = photon_hit_series_of(L.series, L.n_series, i);
    if (s < 0) return PMT_PHOTON_HIT_UNCOVERED;
    const clsimhip_mcpe_series &entry = L.series[s];
    if (i - entry.first >= entry.count) return PMT_PHOTON_HIT_UNCOVERED;                // (first <= i: no wrap)
    const uint32_t word = (uint32_t)(uint16_t)entry.string_id | ((uint32_t)entry.om_id << 16);
    if (w[1] != word) return PMT_PHOTON_HIT_SERIES_MISMATCH;
    const int module = mcpe_class_of(P.module_table, P.module_mask, word);
    if (module < 0) return PMT_PHOTON_HIT_UNKNOWN_MODULE;                               // :281-283
    const PmtModule &M = P.modules[module];
    int found = -1;
    double prob = 0.;
    const int code = pmt_photon_hit_probability(P, values, pmts, M, P.types[M.type], mcpe_f(w[7]), mcpe_f(w[8]), mcpe_f(w[9]), mcpe_f(w[10]), mcpe_f(w[11]),
                                                mcpe_f(w[5]), mcpe_f(w[4]), found, prob, off_surface);
    if (code == PMT_PROBABILITY_ABOVE_ONE) return PMT_PHOTON_HIT_PROBABILITY_ABOVE_ONE;
    if (code != PMT_ACCEPTED) return PMT_PHOTON_HIT_DROPPED;
    uint64_t h = P.seed;
    for (int j = 0; j < 6; ++j) h = mcpe_splitmix64(h ^ ((uint64_t)w[2 * j] | ((uint64_t)w[2 * j + 1] << 32)));
    const double u = (double)(h >> 11) * 0x1p-53;
    if (prob <= u) return PMT_PHOTON_HIT_DROPPED;                                       // :353
    // the time is the record's own, bit for bit (:372): no arithmetic, so a NaN keeps its payload on both targets
    const uint64_t bits = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
    const uint64_t t = bits ^ ((bits >> 63) ? ~0ull : (1ull << 63));                    // series_tkey, on the bits
    pmt = (uint32_t)found;
    key.group = (uint32_t)s * (uint32_t)kPmtMaxPerType + pmt;                           // (s < 2^26: checked by the callers)
    key.t_hi = (uint32_t)(t >> 32);
    key.t_lo = (uint32_t)t;
    key.identifier = w[0];
    return PMT_PHOTON_HIT_KEPT;
}

// the time of a key, bit for bit (series_time_of returns a double, which a target may quiet on its way)
MCPE_HD uint64_t pmt_photon_hit_time_bits(const SeriesKey &k)
{
    const uint64_t t = ((uint64_t)k.t_hi << 32) | k.t_lo;
    return t ^ ((t >> 63) ? (1ull << 63) : ~0ull);
}

// ---- the device stage (pmt_photon_hits_kernel.hip) ----
// header words beside mcpe_series.h's SH_*: the five counters
enum PmtPhotonHitsHeader : uint32_t { PPH_COUNTERS = 48 };

struct PmtPhotonHitsDeviceArgs {
    PmtHitParams P;                         // the generator's, with device pointers (its per-launch members are not read)
    const clsimhip_mcpe_series *in_series;  // 16-byte aligned
    const clsimhip_frame_photon *in;        // 16-byte aligned
    const uint32_t *in_counts;              // records = min(in_counts[0], capacity), series = min(in_counts[1], capacity)
    uint32_t capacity;
    uint32_t group_passes;                  // digit passes 12 ... 12 + group_passes - 1 can be live: a group is below capacity x 64
    uint32_t *header;                       // kSeriesHeaderWords
    uint32_t *histogram;                    // 16 x 256
    uint32_t *tile_counts;
    SeriesKey *keys[2];
    clsimhip_pmt_hit *out;
    clsimhip_pmt_series *series;
    uint32_t *counts;                       // seven: kept, series, the five counters
};
static_assert(sizeof(PmtPhotonHitsDeviceArgs) <= 4096, "passed by value in the kernel argument segment");

// all kernels of the stage, asynchronous on `stream`
hipError_t launch_pmt_photon_hits(const PmtPhotonHitsDeviceArgs &A, hipStream_t stream);

size_t pmt_photon_hits_workspace_bytes(size_t capacity);

static_assert((int)PMT_PHOTON_HIT_UNCOVERED == CLSIMHIP_PMT_PHOTON_HITS_UNCOVERED && (int)PMT_PHOTON_HIT_SERIES_MISMATCH == CLSIMHIP_PMT_PHOTON_HITS_SERIES_MISMATCH &&
                  (int)PMT_PHOTON_HIT_UNKNOWN_MODULE == CLSIMHIP_PMT_PHOTON_HITS_UNKNOWN_MODULE &&
                  (int)PMT_PHOTON_HIT_PROBABILITY_ABOVE_ONE == CLSIMHIP_PMT_PHOTON_HITS_PROBABILITY_ABOVE_ONE &&
                  (int)PMT_PHOTON_HIT_OFF_SURFACE == CLSIMHIP_PMT_PHOTON_HITS_OFF_SURFACE,
              "the counters' order is the C ABI's");

} // namespace clsimhip
