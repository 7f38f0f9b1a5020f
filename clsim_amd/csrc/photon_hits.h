// Photon hits: stored frame photons (include/clsimhip.h: clsimhip_frame_photon with a series table) -> per-frame, per-DOM,
// time-sorted MCPEs, with the calibration look-ups of the reference's older module.  The second half of the reference's two-step
// workflow (python/traysegments/I3CLSimMakeHitsFromPhotons.py): photons are propagated once, hits are made from them as often as
// needed.  The definition lives here ONCE, as a function both the host twin (photon_hits.cpp) and the HIP kernels
// (photon_hits_kernel.hip) compile: binary64 + - * / in the order written, no contraction (-ffp-contract=off, Makefile), so x86-64
// and gfx950 give the same bits.  It restates
//   I3PhotonToMCPEConverter::DAQ                    private/clsim/dom/I3PhotonToMCPEConverter.cxx:257-539
//     DOMs without a status entry or with pmtHV == 0 :288-292      the DOM's own orientation          :315-320, :409-412
//     the relative DOM efficiency x SPE compensation :327-388      (resolved per DOM when the maker is made: photon_hits.cpp)
//     the surface check, pancake factor 1 only       :417-453      the probability's three factors    :466-474
//     the arrival time correction                    :512-518      the per-DOM time sort              :524-526
// with mcpe.h's wavelength acceptance, polynomial, sin / cos pair and hash, which it includes and does not repeat.
//
// Comparisons with a NaN are false, as in mcpe.h.  Step by step:
//   weight:       a NaN weight is neither < 0 nor == 0 and goes on;
//   cosine:       a NaN -(dir . D) clamps to 1 (the first select takes 1 when c < 1 is false);
//   surface:      a NaN r^2 is OFF_SURFACE (the window test is written as !(lo2 <= r2 && r2 <= hi2); the reference's
//                 abs(sqrt(r2) - oversize R) > 3 cm would let it pass);
//   probability:  a NaN P passes both P > 1 and P <= u and yields a record; a NaN wavelength reads the table's last bin;
//   time:         the formula's value, infinities included; a NaN, however it came about, is stored as 0x7ff8000000000000.
//
// What differs from the reference, on purpose:
//   the draw:     the reference takes one number per photon from an I3RandomService in arrival order (:507).  Here u is a hash of
//                 the record's 48 bytes and a seed: the result does not depend on the order of the input, and with one seed the
//                 hits made at a lower efficiency are a subset of those made at a higher one (common random numbers);
//   the order:    std::sort(MCPETimeLess) leaves records with equal times in any order (:526).  Here the kept records of a series
//                 are ascending in (tkey(time), identifier) -- mcpe_series.h's total order on the time's bit pattern -- and records
//                 equal in that are byte-identical;
//   CheckSanity:  (:455) inspects fields of an I3Photon that an I3CompressedPhoton does not carry; it does not apply;
//   merging:      (:531-532) MCHitMerging lies outside the reference.  The caller applies the MCPE merging stage (mcpe_merge.h) to this
//                 stage's output, which has the form that stage reads;
//   geometry:     the cross-checks between I3OMGeo and I3ModuleGeo (:301-325) are the caller's configuration: the DOM table carries
//                 one direction per DOM, and positions are relative to the module, as the frame photons stage stores them.
#pragma once
#include "mcpe.h"
#include "mcpe_series.h"

namespace clsimhip {

// result of one record: a key (KEPT), nothing (DROPPED: weight 0 or the draw), or the counter it belongs to, in the order of
// include/clsimhip.h's CLSIMHIP_PHOTON_HITS_*.  OFF_SURFACE is also counted for a record that only_warn_off_surface lets go on.
enum PhotonHitCode : int {
    PHOTON_HIT_KEPT = -1, PHOTON_HIT_UNCOVERED = 0, PHOTON_HIT_SERIES_MISMATCH = 1, PHOTON_HIT_UNKNOWN_DOM = 2, PHOTON_HIT_INACTIVE = 3,
    PHOTON_HIT_NEGATIVE_WEIGHT = 4, PHOTON_HIT_OFF_SURFACE = 5, PHOTON_HIT_PROBABILITY_ABOVE_ONE = 6, PHOTON_HIT_DROPPED = 7
};
constexpr int kPhotonHitCounters = 7;

constexpr uint32_t kPhotonHitIgnoreInactive = 1u, kPhotonHitOnlyWarn = 2u, kPhotonHitCheckSurface = 4u;    // PhotonHitLookup::switches
constexpr uint32_t kPhotonHitHasStatus = 1u, kPhotonHitInCalibration = 2u;                                  // a DOM's flags

// DOM table: open addressing with mcpe.h's hash, at most half full.  Entry: record word (string ID | OM ID << 16) | (class + 1) << 32
// | flags << 40; 0 = empty.  Beside it, slot by slot, four doubles: the resolved efficiency and the DOM's direction.
struct PhotonHitLookup {                    // wherever the tables live
    const clsimhip_mcpe_series *series;     // the input's series table
    const uint64_t *dom_table;
    const double *dom_values;               // 4 per slot: efficiency, Dx, Dy, Dz
    uint32_t n_series, dom_mask;
    uint32_t switches, reserved;
};

// slot of the DOM, or -1
MCPE_HD int64_t photon_hit_dom_slot(const uint64_t *table, uint32_t mask, uint32_t word)
{
    uint32_t slot = mcpe_dom_slot(word, mask);
    for (;;) {                                          // (the table is at most half full: an empty entry ends every probe)
        const uint64_t e = table[slot];
        if (e == 0u) return -1;
        if ((uint32_t)e == word) return (int64_t)slot;
        slot = (slot + 1u) & mask;
    }
}

// the last entry with first <= i, or -1.  (Nothing checks that `first` ascends: the walk below is the definition.)
MCPE_HD int64_t photon_hit_series_of(const clsimhip_mcpe_series *series, uint32_t n, uint32_t i)
{
    uint32_t lo = 0u, hi = n;                           // first entry with first > i
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (series[mid].first <= i) lo = mid + 1u; else hi = mid;
    }
    return (int64_t)lo - 1;
}

// Record i (its 12 words: identifier, string ID | OM ID << 16, the time's two words, then weight, wavelength, group velocity, x, y,
// z, theta, phi) -> PhotonHitCode; `key` is written when the code is PHOTON_HIT_KEPT.  off_surface: the record failed the surface
// check, whatever became of it then.  P: the maker's acceptances, polynomial, surface window, time factor and seed; `values`: the
// classes' table values, wherever the caller keeps them.
template <class Values>
MCPE_HD int photon_hit_make(const PhotonHitLookup &L, const McpeParams &P, Values values, uint32_t i, const uint32_t *w, SeriesKey &key, bool &off_surface)
{
    off_surface = false;
    const int64_t s = photon_hit_series_of(L.series, L.n_series, i);
    if (s < 0) return PHOTON_HIT_UNCOVERED;
    const clsimhip_mcpe_series &entry = L.series[s];
    if (i - entry.first >= entry.count) return PHOTON_HIT_UNCOVERED;                   // (first <= i: no wrap)
    const uint32_t word = (uint32_t)(uint16_t)entry.string_id | ((uint32_t)entry.om_id << 16);
    if (w[1] != word) return PHOTON_HIT_SERIES_MISMATCH;
    const int64_t slot = photon_hit_dom_slot(L.dom_table, L.dom_mask, word);
    if (slot < 0) return PHOTON_HIT_UNKNOWN_DOM;                                        // :295-298
    const uint32_t upper = (uint32_t)(L.dom_table[slot] >> 32);
    if ((L.switches & kPhotonHitIgnoreInactive) != 0u && ((upper >> 8) & kPhotonHitHasStatus) == 0u) return PHOTON_HIT_INACTIVE;     // :288-292
    const double W = (double)mcpe_f(w[4]);
    if (W < 0.) return PHOTON_HIT_NEGATIVE_WEIGHT;                                      // :398
    if (W == 0.) return PHOTON_HIT_DROPPED;                                             // :399
    const double *dom = L.dom_values + 4u * (size_t)slot;
    const double efficiency = dom[0], Dx = dom[1], Dy = dom[2], Dz = dom[3];
    float st, ct, sp, cp;
    mcpe_sincos(mcpe_f(w[10]), st, ct);
    mcpe_sincos(mcpe_f(w[11]), sp, cp);
    const double dx = (double)st * (double)cp, dy = (double)st * (double)sp, dz = (double)ct;
    double c = -(dx * Dx + dy * Dy + dz * Dz);                                          // :409-411; D as given
    c = c < 1. ? c : 1.;                                                                // :412
    c = c > -1. ? c : -1.;
    const double x = (double)mcpe_f(w[7]), y = (double)mcpe_f(w[8]), z = (double)mcpe_f(w[9]);
    if ((L.switches & kPhotonHitCheckSurface) != 0u) {                                  // :417: pancake factor 1 only
        const double r2 = x * x + y * y + z * z;
        if (!(P.lo2 <= r2 && r2 <= P.hi2)) {                                            // :420, without the square root
            off_surface = true;
            if ((L.switches & kPhotonHitOnlyWarn) == 0u) return PHOTON_HIT_OFF_SURFACE;
        }
    }
    const int k = (int)(upper & 255u) - 1;
    double prob = W * mcpe_acceptance(P.classes[k], values, (double)mcpe_f(w[5]));      // :466
    prob = prob * mcpe_polynomial(P, c);                                                // :470
    prob = prob * efficiency;                                                           // :474
    if (prob > 1.) return PHOTON_HIT_PROBABILITY_ABOVE_ONE;                             // :478-504
    uint64_t h = P.seed;
    for (int j = 0; j < 6; ++j) h = mcpe_splitmix64(h ^ ((uint64_t)w[2 * j] | ((uint64_t)w[2 * j + 1] << 32)));
    const double u = (double)(h >> 11) * 0x1p-53;
    if (prob <= u) return PHOTON_HIT_DROPPED;                                           // :507
    const double dot = (-x) * dx + (-y) * dy + (-z) * dz;                               // :515
    double time = __builtin_bit_cast(double, (uint64_t)w[2] | ((uint64_t)w[3] << 32)) + dot * P.time_factor / (double)mcpe_f(w[6]);    // :516-517
    // (one NaN pattern, as in mcpe_make: which of two NaN operands an addition passes on differs between the targets)
    if (time != time) time = __builtin_bit_cast(double, (uint64_t)0x7ff8000000000000ull);
    const uint64_t t = series_tkey(time);
    key.group = (uint32_t)s;
    key.t_hi = (uint32_t)(t >> 32);
    key.t_lo = (uint32_t)t;
    key.identifier = w[0];
    return PHOTON_HIT_KEPT;
}

// ---- the device stage (photon_hits_kernel.hip) ----
// header words beside mcpe_series.h's SH_*: the seven counters
enum PhotonHitsHeader : uint32_t { PH_COUNTERS = 48 };

struct PhotonHitsDeviceArgs {
    PhotonHitLookup lookup;                 // device pointers; n_series is read from in_counts
    const McpeParams *params;               // the maker's, in device memory (copied into LDS with the table values)
    const double *values;
    uint32_t num_values;
    uint32_t group_passes;                  // digit passes 12 ... 12 + group_passes - 1 can be live: a group is below `capacity`
    const clsimhip_frame_photon *in;        // 16-byte aligned
    const uint32_t *in_counts;              // records = min(in_counts[0], capacity), series = min(in_counts[1], capacity)
    uint32_t capacity;
    uint32_t *header;                       // kSeriesHeaderWords
    uint32_t *histogram;                    // 16 x 256
    uint32_t *tile_counts;
    SeriesKey *keys[2];
    clsimhip_mcpe *out;
    clsimhip_mcpe_series *series;
    uint32_t *counts;                       // nine: kept, series, the seven counters
};

// all kernels of the stage, asynchronous on `stream`
hipError_t launch_photon_hits(const PhotonHitsDeviceArgs &A, hipStream_t stream);

// ---- the host side (photon_hits.cpp) ----
using PhotonHitDom = clsimhip_photon_hit_dom;
using PhotonHitConfig = clsimhip_photon_hit_config;
static_assert(kPhotonHitHasStatus == CLSIMHIP_PHOTON_HITS_FLAG_HAS_STATUS && kPhotonHitInCalibration == CLSIMHIP_PHOTON_HITS_FLAG_IN_CALIBRATION &&
                  (int)PHOTON_HIT_PROBABILITY_ABOVE_ONE == CLSIMHIP_PHOTON_HITS_PROBABILITY_ABOVE_ONE,
              "the flags and the counters' order are the C ABI's");

size_t photon_hits_workspace_bytes(size_t capacity);

// The maker object: configuration, host twin, and its tables on every device it has been used on
class PhotonHitMaker {
public:
    PhotonHitMaker(const std::vector<FunctionData> &classes, const clsimhip_polynomial &angular, const PhotonHitDom *doms, size_t n_doms, const PhotonHitConfig &config);
    ~PhotonHitMaker();
    PhotonHitMaker(const PhotonHitMaker &) = delete;
    PhotonHitMaker &operator=(const PhotonHitMaker &) = delete;

    // the resolved efficiency of a DOM of the table (CLSIMHIP_ERR_ARGUMENT for any other)
    double efficiency(int32_t string_id, uint32_t om_id) const;
    // host twin: out holds n entries, out_series n_series; counters[7] += the conditions met
    void host(const clsimhip_frame_photon *records, size_t n, const clsimhip_mcpe_series *series, size_t n_series, clsimhip_mcpe *out,
              clsimhip_mcpe_series *out_series, size_t *n_kept, size_t *n_series_out, uint64_t counters[7]) const;
    // the kernels on `stream` of `device`
    void device(int device, const void *d_records, const void *d_series, const void *d_in_counts, size_t capacity, void *d_out, void *d_out_series,
                void *d_counts, void *d_workspace, size_t workspace_bytes, hipStream_t stream);

private:
    McpeParams params_{};
    uint32_t switches_ = 0u;
    std::vector<double> values_;
    std::vector<uint64_t> dom_table_;
    std::vector<double> dom_values_;        // beside dom_table_, slot by slot: efficiency, Dx, Dy, Dz
    struct Image { McpeParams *params = nullptr; double *values = nullptr; uint64_t *dom_table = nullptr; double *dom_values = nullptr; };
    std::mutex device_mutex_;
    std::map<int, Image> images_;
    Image image_on(int device);
};

} // namespace clsimhip
