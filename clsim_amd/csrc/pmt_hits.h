// Multi-PMT hit maker: one delivered photon record -> zero or one hit on one PMT of a segmented module (include/clsimhip.h:
// clsimhip_pmt_generator).  As in mcpe.h the definition lives here ONCE, as a function both the host twin (pmt_hits.cpp) and the
// HIP kernel (pmt_hits_kernel.hip) compile: binary64 + - * / in the order written, no contraction (-ffp-contract=off, Makefile),
// so x86-64 and gfx950 give the same bits.  The sin / cos pairs, the record hash, the FromTable / Constant evaluation and the
// module hash table are mcpe.h's.  It restates
//   FindHitPMT                                     private/clsim/dom/I3PhotonToMCHitConverterForMultiPMT.cxx:111-227
//   I3PhotonToMCHitConverterForMultiPMT::DAQ       :297-382, the body of the loop over one module's photons
// What differs from the reference, on purpose:
//   * hit_angle >= 90 deg (:319-323) is stated on the cosine, c = -(n . d) <= 0, so that no acos is needed; the angular acceptance
//     factor is tabulated over c, and |cos(hit_angle)| in :340 is c (it is > 0 where it is used).
//   * the path-length argument of GetGlassGelSurvivalProbability (:328) is NOT modelled: it needs an exp whose definition the
//     reference does not hold (I3OMTypeInfo is outside it).  G is a function of the wavelength alone.
//   * the reference computes travelTimeInOM (:314) and then gives the hit the photon's own time (:372); so does this.
//   * the 3 cm surface check (:139-145) only warns in the reference; here it is counted (OFF_SURFACE) and the record goes on.  The
//     window is squared, as in mcpe_make.
//   * I3Orientation is outside the reference: a module carries the rotation as nine doubles, row-major, module frame -> detector
//     frame, applied as (m0 v0 + m1 v1) + m2 v2 per row.  The two log_fatal checks on the rotation (:172, :189) and the one on the
//     PMT position (:191) depend on the configuration alone and are made once, when the generator is created.
//   * the draw is the record hash of mcpe_make (the reference takes one number per photon from an I3RandomService, :353).
#pragma once
#include "mcpe.h"

namespace clsimhip {

constexpr int kPmtMaxTypes = 8;
constexpr int kPmtMaxPerType = 64;
constexpr int kPmtMaxFunctions = 64;
// LDS of the kernel, sized per launch by what the generator holds: the PMT tables of all types (72 B per PMT: 36 KiB for 8 x 64) and
// the function values, a budget of their own (24 KiB) so that the largest generator asks for 60 KiB per block
constexpr uint32_t kPmtMaxTableValues = 3072;

// result of one record (OFF_SURFACE is not a result: the record goes on, pmt_make reports it beside the code)
enum PmtCode : int { PMT_ACCEPTED = 0, PMT_UNKNOWN_MODULE = 1, PMT_PROBABILITY_ABOVE_ONE = 2, PMT_DROPPED = 3 };

struct PmtEntry {                   // one PMT of a type, in the module's frame
    double n[3], a[3];              // axis (unit), centre of the disc [m]
    double radius2, ce;             // disc radius squared, collection efficiency
    int32_t q, acceptance;          // function indices: quantum efficiency over the wavelength, angular acceptance factor over c
};
static_assert(sizeof(PmtEntry) == 72, "PmtEntry is staged in LDS as nine 8-byte words");

struct PmtType {
    double lo2, hi2;                // the surface window, squared: max(R - 0.03, 0)^2 <= r^2 <= (R + 0.03)^2
    int32_t first, count;           // its PMTs in PmtHitParams::pmts
    int32_t g, reserved;            // function index: glass / gel survival over the wavelength
};

struct PmtModule {                  // behind the hash lookup (global memory in the kernel)
    double m[9];                    // row-major, module frame -> detector frame
    int32_t type, reserved;
};

// kernel parameters (passed by value) and the host twin's configuration
struct PmtHitParams {
    McpeClass functions[kPmtMaxFunctions];
    PmtType types[kPmtMaxTypes];
    uint64_t seed;
    const double *values;           // the functions' table values, one after the other (num_values of them)
    const PmtEntry *pmts;           // the types' PMTs, one type after the other (num_pmts of them)
    const uint64_t *module_table;   // mcpe.h's scheme: record word 11 | (module index + 1) << 32; 0 = empty
    const PmtModule *modules;
    uint32_t num_values, num_pmts, module_mask;
    int32_t num_types, num_functions;
    // per launch
    const uint32_t *photons;        // 20 words per record
    const uint32_t *hit_count;      // records = min(*hit_count, capacity)
    clsimhip_pmt_hit *out;
    uint32_t *counters;             // [0] accepted (keeps counting past out_capacity), [1] UNKNOWN_MODULE, [2] PROBABILITY_ABOVE_ONE, [3] OFF_SURFACE
    uint32_t capacity, out_capacity;
};

// one record (its 20 words; position words 0-2 relative to the module centre, as saveHit writes them) -> PmtCode; `out` is
// written when the code is PMT_ACCEPTED; off_surface: the record reached the surface check (:139) and is outside the window.
// `values` / `pmts`: the function values and PMT tables, wherever the caller keeps them (LDS in the kernel).
template <class Values, class Pmts>
MCPE_HD int pmt_make(const PmtHitParams &P, Values values, Pmts pmts, const uint32_t *w, clsimhip_pmt_hit &out, bool &off_surface)
{
    off_surface = false;
    const int module = mcpe_class_of(P.module_table, P.module_mask, w[11]);
    if (module < 0) return PMT_UNKNOWN_MODULE;                          // :281-283
    const PmtModule &M = P.modules[module];
    const PmtType &T = P.types[M.type];
    const double px = (double)mcpe_f(w[0]), py = (double)mcpe_f(w[1]), pz = (double)mcpe_f(w[2]);
    float st, ct, sp, cp;
    mcpe_sincos(mcpe_f(w[4]), st, ct);
    mcpe_sincos(mcpe_f(w[5]), sp, cp);
    const double dx = (double)st * (double)cp, dy = (double)st * (double)sp, dz = (double)ct;
    const double dot = px * dx + py * dy + pz * dz;                     // :132
    if (dot > 0.) return PMT_DROPPED;                                   // :133-136: the photon is leaving
    const double pr2 = px * px + py * py + pz * pz;
    off_surface = !(T.lo2 <= pr2 && pr2 <= T.hi2);                      // :139-145, without the square root; goes on
    int found = -1;
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
    const double wlen = (double)mcpe_f(w[6]);
    double prob = (double)mcpe_f(w[9]);                                 // :343-346
    prob *= mcpe_acceptance(P.functions[T.g], values, wlen);
    prob *= mcpe_acceptance(P.functions[E.q], values, wlen) * E.ce;
    prob *= mcpe_acceptance(P.functions[E.acceptance], values, c) / c;
    if (prob > 1.) return PMT_PROBABILITY_ABOVE_ONE;                    // :348-351
    uint64_t h = P.seed;
    for (int j = 0; j < 10; ++j) h = mcpe_splitmix64(h ^ ((uint64_t)w[2 * j] | ((uint64_t)w[2 * j + 1] << 32)));
    const double u = (double)(h >> 11) * 0x1p-53;
    if (prob <= u) return PMT_DROPPED;                                  // :353
    out.identifier = w[10];
    out.string_id = (int16_t)(w[11] & 0xffffu);
    out.om_id = (uint16_t)(w[11] >> 16);
    out.pmt = (uint32_t)found;
    out.reserved = 0u;
    out.time = (double)mcpe_f(w[3]);                                    // :372 (not :314)
    return PMT_ACCEPTED;
}

// bytes of LDS a launch with these parameters asks for (the PMT tables, then the function values: pmt_hits_kernel's layout)
inline size_t pmt_hits_lds_bytes(const PmtHitParams &P) { return (size_t)P.num_values * sizeof(double) + (size_t)P.num_pmts * sizeof(PmtEntry); }

// pmt_hits_kernel.hip: P.values / P.pmts / P.module_table / P.modules in device memory; asynchronous on `stream`
hipError_t launch_pmt_hits_kernel(const PmtHitParams &P, hipStream_t stream);

// The generator object: configuration, host twin, and its tables on every device it has been used on
class PmtHitGenerator {
public:
    PmtHitGenerator(const std::vector<FunctionData> &functions, const clsimhip_pmt_type *types, size_t n_types, const clsimhip_pmt *pmts, size_t n_pmts,
                    const clsimhip_pmt_module *modules, size_t n_modules, uint64_t seed);
    ~PmtHitGenerator();
    PmtHitGenerator(const PmtHitGenerator &) = delete;
    PmtHitGenerator &operator=(const PmtHitGenerator &) = delete;

    // host twin: input order is kept; counters[3] += UNKNOWN_MODULE, PROBABILITY_ABOVE_ONE, OFF_SURFACE
    void convert_host(const clsimhip_photon *photons, size_t n, clsimhip_pmt_hit *out, size_t capacity, size_t *n_out, uint64_t counters[3]) const;
    // the kernel on `stream` of `device`; zeroes d_counters[0..3] first (in stream order)
    void convert_device(int device, const void *d_photons, const void *d_hit_count, size_t capacity, void *d_hits, size_t hit_capacity, void *d_counters,
                        hipStream_t stream);
    bool has_module(int32_t string_id, uint32_t om_id) const;
    // the sphere radii of the types modules use (Compile() compares them with the radius the converter records photons at)
    const std::vector<double> &used_sphere_radii() const { return used_radii_; }

    // ---- PMT series (pmt_series.h; pmt_series.cpp) ----
    size_t num_modules() const { return module_of_rank_.size(); }
    size_t num_channels() const { return base_.back(); }                // PMTs of all modules together
    // One bunch's particle table and mask, checked and brought into the form the stage reads (pmt_series_blob_bytes(n_particles,
    // n_masked) bytes at `blob`, 16-byte aligned): CLSIMHIP_ERR_ARGUMENT for a table that is not strictly increasing in
    // `identifier`, CLSIMHIP_ERR_CONFIG for frames x channels >= 2^32.  particles = nullptr: no table.
    SeriesBunch prepare_series(const clsimhip_mcpe_particle *particles, size_t n_particles, const clsimhip_mcpe_mask *masked, size_t n_masked,
                               uint8_t *blob) const;
    // host twin: out and series hold n entries each; counters[3] += UNKNOWN_PARTICLE, MASKED, UNKNOWN_CHANNEL
    void series_host(const clsimhip_pmt_hit *in, size_t n, const clsimhip_mcpe_particle *particles, size_t n_particles, const clsimhip_mcpe_mask *masked,
                     size_t n_masked, clsimhip_pmt_hit *out, clsimhip_pmt_series *series, size_t *n_kept, size_t *n_series, uint64_t counters[3]) const;
    // the kernels on `stream` of `device`, over min(*d_count, capacity) records; d_counts: five uint32 (kept, series, the counters)
    void series_device(int device, const void *d_hits, const void *d_count, size_t capacity, const clsimhip_mcpe_particle *particles,
                       size_t n_particles, const clsimhip_mcpe_mask *masked, size_t n_masked, void *d_out, void *d_series, void *d_counts,
                       void *d_workspace, size_t workspace_bytes, hipStream_t stream);
    // the same for a bunch prepared into page-locked memory that stays as it is until the stream has passed the copy this call
    // begins with; `uploaded` (may be null) is recorded behind that copy
    void series_device_prepared(int device, const void *d_hits, const void *d_count, size_t capacity, const SeriesBunch &bunch, const uint8_t *h_blob,
                                void *d_out, void *d_series, void *d_counts, void *d_workspace, size_t workspace_bytes, hipStream_t stream,
                                hipEvent_t uploaded = nullptr);

    // ---- PMT photon hits (pmt_photon_hits.h; pmt_photon_hits.cpp) ----
    // host twin: out and out_series hold n entries each; counters[5] += the conditions met
    void photon_hits_host(const clsimhip_frame_photon *records, size_t n, const clsimhip_mcpe_series *series, size_t n_series, clsimhip_pmt_hit *out,
                          clsimhip_pmt_series *out_series, size_t *n_kept, size_t *n_series_out, uint64_t counters[5]) const;
    // the kernels on `stream` of `device`, with the device image convert_device uses
    void photon_hits_device(int device, const void *d_records, const void *d_series, const void *d_in_counts, size_t capacity, void *d_out, void *d_out_series,
                            void *d_counts, void *d_workspace, size_t workspace_bytes, hipStream_t stream);

private:
    PmtHitParams params_{};
    std::vector<double> values_;
    std::vector<PmtEntry> pmts_;
    std::vector<uint64_t> module_table_;
    std::vector<PmtModule> modules_;
    std::vector<double> used_radii_;
    struct DeviceImage { double *values = nullptr; PmtEntry *pmts = nullptr; uint64_t *module_table = nullptr; PmtModule *modules = nullptr; };
    std::mutex device_mutex_;
    std::map<int, DeviceImage> images_;
    DeviceImage image_on(int device);
    // PMT series: beside module_table_ slot by slot the module's rank in ascending (string ID, OM ID) order and its first channel;
    // by rank the first channel (one entry more: the number of channels) and the record word (string ID | OM ID << 16)
    std::vector<uint32_t> module_ranks_, channel_bases_, base_, module_of_rank_;
    void build_series_tables();
    // what the stage keeps on the devices it has run on: these tables, and the page-locked staging of the stand-alone call's bunch
    // (pmt_series.cpp; made by the first device call, so that the generator and its host twin need nothing of the HIP runtime)
    struct SeriesImage { uint32_t *module_ranks = nullptr, *channel_bases = nullptr, *base = nullptr, *module_of_rank = nullptr; };
    struct SeriesState;
    std::mutex series_mutex_;
    std::shared_ptr<SeriesState> series_state_;
    SeriesState &series_state();
    SeriesImage series_image_on(int device);
};

// pmt_series.cpp: the sizes that go with a bunch's particle table and mask (a SeriesBunch of host_model.h, as for the MCPE series)
size_t pmt_series_blob_bytes(size_t n_particles, size_t n_masked);
size_t pmt_series_workspace_bytes(size_t capacity, size_t n_particles, size_t n_masked);

} // namespace clsimhip
