// Hit maker: one delivered photon record -> zero or one MCPE (include/clsimhip.h: clsimhip_mcpe_generator).
// The definition lives here ONCE, as a function both the host twin (mcpe.cpp) and the HIP kernel (mcpe_kernel.hip)
// compile: binary64 + - * / in the order written, no contraction (-ffp-contract=off, Makefile), so x86-64 and gfx950
// give the same bits.  It restates
//   I3CLSimPhotonToMCPEConverterForDOMs::Convert   private/clsim/dom/I3PhotonToMCPEConverter.cxx:602-669
//   the older module's arrival time correction     :512-518  (zero when pancake factor = oversize factor)
//   I3CLSimFunctionFromTable::GetValue             private/clsim/function/I3CLSimFunctionFromTable.cxx:106-124
//   I3CLSimFunctionPolynomial::GetValue            private/clsim/function/I3CLSimFunctionPolynomial.cxx:85-101
// The reference's one random number per photon comes from an I3RandomService in arrival order, which is not reproducible
// (hits arrive in atomic order); here it is a hash of the record and a seed, so the result does not depend on the schedule.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "detmath.hip.h"
#include "hip_resources.h"
#include "host_model.h"
#include "series_bunch.h"

namespace clsimhip {

#define MCPE_HD __host__ __device__ __forceinline__

constexpr int kMcpeMaxClasses = 8;
constexpr int kMcpeMaxCoefficients = 32;
constexpr uint32_t kMcpeMaxTableValues = 4096;      // all classes together: 32 KiB of LDS in the kernel

// result of one record: an MCPE, nothing (weight 0 or the draw), or one of the four conditions the reference ends the run on
enum McpeCode : int {
    MCPE_ACCEPTED = 0, MCPE_NEGATIVE_WEIGHT = 1, MCPE_OFF_SURFACE = 2, MCPE_UNKNOWN_DOM = 3, MCPE_PROBABILITY_ABOVE_ONE = 4,
    MCPE_DROPPED = 5
};

struct McpeClass {                  // one wavelength acceptance: FromTable with equal spacing, or Constant
    int32_t kind, n;
    uint32_t offset, reserved;      // first of its n values in McpeParams::values
    double start, step, value;
};

// kernel parameters (passed by value: wave-uniform, read with scalar loads) and the host twin's configuration
struct McpeParams {
    McpeClass classes[kMcpeMaxClasses];
    double coefficients[kMcpeMaxCoefficients];
    double range_min, range_max, underflow, overflow;
    double lo2, hi2;                // the surface window, squared: max(R - 0.03, 0)^2 <= r^2 <= (R + 0.03)^2
    double time_factor;             // 1 - pancake / oversize
    uint64_t seed;
    const double *values;           // the classes' table values, one after the other (num_values of them)
    const uint64_t *dom_table;      // open addressing, dom_mask + 1 entries: record word 11 | (class + 1) << 32; 0 = empty
    uint32_t num_values, dom_mask;
    int32_t num_classes, num_coefficients;
    // per launch
    const uint32_t *photons;        // 20 words per record
    const uint32_t *hit_count;      // records = min(*hit_count, capacity)
    clsimhip_mcpe *out;
    uint32_t *counters;             // [0] accepted (keeps counting past out_capacity), [1..4] the conditions
    uint32_t capacity, out_capacity;
};

// The Cephes branch's quadrant count as an int32, for EVERY float: what gfx950's conversion instruction gives for dm::sincos_cephes_'s
// (int32_t)k -- it saturates, and a NaN gives 0.  (The C++ conversion is undefined outside int32, and x86-64 yields INT32_MIN there.)
inline int32_t mcpe_quadrant_host(float k)
{
    if (k != k) return 0;
    if (k >= 2147483648.0f) return INT32_MAX;
    if (k <= -2147483648.0f) return INT32_MIN;
    return (int32_t)k;
}

// ---- dm::sincos_ on the host: the same operations on the same constants (detmath.hip.h: sincos_2pi_with_, sincos_cephes_) ----
// Total: an angle beyond the int32 quadrant range (|x| from about 3.37e9, infinities, NaNs) takes the saturated count above.  There
// the reduced argument is meaningless (huge, or a NaN for an infinite or NaN angle); the results are what the operations give.
inline void mcpe_sincos_host(float x, float &s, float &c)
{
    if (x >= 0.0f && x <= dm::SINCOS_2PI_MAX) {
        const float kf = __builtin_fmaf(x, MT_SC_16OPI, 12582912.0f);
        const float k = kf - 12582912.0f;
        float r = __builtin_fmaf(-k, MT_SC_H1, x);
        r = __builtin_fmaf(-k, MT_SC_H2, r);
        const float z = r * r;
        const float sp = __builtin_fmaf(z, MT_SIN_S1, MT_SIN_S0) * z;
        const float sr = __builtin_fmaf(sp, r, r);
        const float cm = __builtin_fmaf(z, MT_COS_C1, -0.5f) * z;
        const uint32_t row = __builtin_bit_cast(uint32_t, kf) - 0x4b400000u;      // 0 ... 32
        const float S = dm::kScTableHost[2u * row], C = dm::kScTableHost[2u * row + 1u];
        s = S + __builtin_fmaf(S, cm, C * sr);
        c = C + __builtin_fmaf(C, cm, -(S * sr));
        return;
    }
    const float k = __builtin_rintf(x * dm::TWO_O_PI);
    float r = __builtin_fmaf(-k, dm::PIO2_1, x);
    r = __builtin_fmaf(-k, dm::PIO2_2, r);
    r = __builtin_fmaf(-k, dm::PIO2_3, r);
    const float z = r * r;
    float ps = -1.9515295891e-4f;
    ps = __builtin_fmaf(ps, z, 8.3321608736e-3f);
    ps = __builtin_fmaf(ps, z, -1.6666654611e-1f);
    ps = __builtin_fmaf(ps * z, r, r);
    float pc = 2.443315711809948e-5f;
    pc = __builtin_fmaf(pc, z, -1.388731625493765e-3f);
    pc = __builtin_fmaf(pc, z, 4.166664568298827e-2f);
    pc = pc * (z * z);
    pc = __builtin_fmaf(-0.5f, z, pc);
    pc = pc + 1.0f;
    const uint32_t q = (uint32_t)mcpe_quadrant_host(k);                 // (unsigned: q + 1 wraps at INT32_MAX, as the device's add does)
    const float a = (q & 1u) ? pc : ps;
    const float b = (q & 1u) ? ps : pc;
    s = (q & 2u) ? -a : a;
    c = ((q + 1u) & 2u) ? -b : b;
}

MCPE_HD void mcpe_sincos(float x, float &s, float &c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    dm::sincos_(x, s, c);
#else
    mcpe_sincos_host(x, s, c);
#endif
}

MCPE_HD float mcpe_f(uint32_t u) { return __builtin_bit_cast(float, u); }

MCPE_HD uint64_t mcpe_splitmix64(uint64_t state)        // rng.cpp: splitmix64, one step from `state`
{
    uint64_t z = state + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

MCPE_HD uint32_t mcpe_dom_slot(uint32_t key, uint32_t mask) { return ((key * 2654435761u) >> 7) & mask; }     // (25 bits: tables of up to 2^25 entries)

// class index of the (string ID, OM ID) pair in record word 11, or -1
MCPE_HD int mcpe_class_of(const uint64_t *table, uint32_t mask, uint32_t key)
{
    uint32_t slot = mcpe_dom_slot(key, mask);
    for (;;) {                                          // (the table is at most half full: an empty entry ends every probe)
        const uint64_t e = table[slot];
        if (e == 0u) return -1;
        if ((uint32_t)e == key) return (int)(e >> 32) - 1;
        slot = (slot + 1u) & mask;
    }
}

// FromTable.cxx:106-124 (equal spacing): modf, clamp to the first / last bin, mix(min, max, t) = min + (max - min) * t.
// `values`: the class's table, wherever the caller keeps it.
template <class Values>
MCPE_HD double mcpe_acceptance(const McpeClass &k, Values values, double wlen)
{
    if (k.kind == CLSIMHIP_FUNCTION_CONSTANT) return k.value;
    const double q = (wlen - k.start) / k.step;
    double fbin = __builtin_trunc(q);
    double fraction = q - fbin;                         // modf: exact
    const double last = (double)(k.n - 1);
    if (fbin < 0. || (fbin == 0. && fraction < 0.)) { fbin = 0.; fraction = 0.; }
    else if (!(fbin < last)) { fbin = last - 1.; fraction = 1.; }        // (a NaN wavelength ends here too)
    const uint32_t bin = k.offset + (uint32_t)fbin;
    const double lo = values[bin], hi = values[bin + 1u];
    return lo + (hi - lo) * fraction;
}

// Polynomial.cxx:85-101: the running-multiplier form, sum += c_i * multiplier (NOT Horner: the bits differ)
MCPE_HD double mcpe_polynomial(const McpeParams &P, double x)
{
    if (P.num_coefficients == 0) return 0.;
    if (x < P.range_min) return P.underflow;
    if (x > P.range_max) return P.overflow;
    double sum = P.coefficients[0], multiplier = 1.;
    for (int i = 1; i < P.num_coefficients; ++i) {
        multiplier *= x;
        sum += P.coefficients[i] * multiplier;
    }
    return sum;
}

// one record (its 20 words, string and OM IDs in w[11]) -> McpeCode; `out` is written when the code is MCPE_ACCEPTED
template <class Values>
MCPE_HD int mcpe_make(const McpeParams &P, Values values, const uint32_t *w, clsimhip_mcpe &out)
{
    const double W = (double)mcpe_f(w[9]);
    if (W < 0.) return MCPE_NEGATIVE_WEIGHT;                            // :606
    if (W == 0.) return MCPE_DROPPED;                                   // :607
    const double x = (double)mcpe_f(w[0]), y = (double)mcpe_f(w[1]), z = (double)mcpe_f(w[2]);
    const double r2 = x * x + y * y + z * z;
    if (!(P.lo2 <= r2 && r2 <= P.hi2)) return MCPE_OFF_SURFACE;         // :610-622, without the square root
    float st, ct, sp, cp;
    mcpe_sincos(mcpe_f(w[4]), st, ct);
    mcpe_sincos(mcpe_f(w[5]), sp, cp);
    const double dx = (double)st * (double)cp, dy = (double)st * (double)sp, dz = (double)ct;
    double c = -dz;                                                     // :624-625
    c = c < 1. ? c : 1.;
    c = c > -1. ? c : -1.;
    const int k = mcpe_class_of(P.dom_table, P.dom_mask, w[11]);
    if (k < 0) return MCPE_UNKNOWN_DOM;                                 // :628-630
    double prob = W * mcpe_acceptance(P.classes[k], values, (double)mcpe_f(w[6]));
    prob = prob * mcpe_polynomial(P, c);
    if (prob > 1.) return MCPE_PROBABILITY_ABOVE_ONE;                   // :639-661
    uint64_t h = P.seed;
    for (int j = 0; j < 10; ++j) h = mcpe_splitmix64(h ^ ((uint64_t)w[2 * j] | ((uint64_t)w[2 * j + 1] << 32)));
    const double u = (double)(h >> 11) * 0x1p-53;
    if (prob <= u) return MCPE_DROPPED;                                 // :664
    const double dot = (-x) * dx + (-y) * dy + (-z) * dz;               // :512-518
    out.identifier = w[10];
    out.string_id = (int16_t)(w[11] & 0xffffu);
    out.om_id = (uint16_t)(w[11] >> 16);
    double time = (double)mcpe_f(w[3]) + dot * P.time_factor / (double)mcpe_f(w[18]);
    // a NaN time has ONE bit pattern: which of two NaN operands an addition passes on is the target's (and the compiler's) business --
    // measured: x86-64 and gfx950 differ there, while both generate 0xfff8000000000000 -- and the series stage orders records by the time's bits
    if (time != time) time = __builtin_bit_cast(double, (uint64_t)0x7ff8000000000000ull);
    out.time = time;
    return MCPE_ACCEPTED;
}

// mcpe_kernel.hip: P.values / P.dom_table in device memory; asynchronous on `stream`
hipError_t launch_mcpe_kernel(const McpeParams &P, hipStream_t stream);

// The generator object: configuration, host twin, and its tables on every device it has been used on
class McpeGenerator {
public:
    McpeGenerator(const std::vector<FunctionData> &classes, size_t n_doms, const int32_t *string_ids, const uint32_t *om_ids,
                  const int32_t *class_index, const clsimhip_polynomial &angular, double dom_radius, double oversize, double pancake,
                  uint64_t seed);
    ~McpeGenerator();
    McpeGenerator(const McpeGenerator &) = delete;
    McpeGenerator &operator=(const McpeGenerator &) = delete;

    // host twin: input order is kept; counters[4] += the conditions met
    void convert_host(const clsimhip_photon *photons, size_t n, clsimhip_mcpe *out, size_t capacity, size_t *n_out, uint64_t counters[4]) const;
    // the kernel on `stream` of `device`; zeroes d_counters[0..4] first (in stream order)
    void convert_device(int device, const void *d_photons, const void *d_hit_count, size_t capacity, void *d_mcpes, size_t mcpe_capacity,
                        void *d_counters, hipStream_t stream);
    bool has_class(int32_t string_id, uint32_t om_id) const;
    double pancake() const { return pancake_; }

    // ---- MCPE series (mcpe_series.h; mcpe_series.cpp) ----
    size_t num_doms() const { return dom_of_rank_.size(); }             // distinct (string ID, OM ID) pairs
    // One bunch's particle table and mask, checked and brought into the form the stage reads (mcpe_series_blob_bytes(n_particles,
    // n_masked) bytes at `blob`, 16-byte aligned): CLSIMHIP_ERR_ARGUMENT for a table that is not strictly increasing in
    // `identifier`, CLSIMHIP_ERR_CONFIG for frames x DOMs >= 2^32.  particles = nullptr: no table.
    SeriesBunch prepare_series(const clsimhip_mcpe_particle *particles, size_t n_particles, const clsimhip_mcpe_mask *masked, size_t n_masked,
                               uint8_t *blob) const;
    // host twin: out and series hold n entries each; counters[3] += UNKNOWN_PARTICLE, MASKED, UNKNOWN_DOM
    void series_host(const clsimhip_mcpe *in, size_t n, const clsimhip_mcpe_particle *particles, size_t n_particles, const clsimhip_mcpe_mask *masked,
                     size_t n_masked, clsimhip_mcpe *out, clsimhip_mcpe_series *series, size_t *n_kept, size_t *n_series, uint64_t counters[3]) const;
    // the kernels on `stream` of `device`, over min(*d_count, capacity) records; d_counts: five uint32 (kept, series, the counters)
    void series_device(int device, const void *d_mcpes, const void *d_count, size_t capacity, const clsimhip_mcpe_particle *particles,
                       size_t n_particles, const clsimhip_mcpe_mask *masked, size_t n_masked, void *d_out, void *d_series, void *d_counts,
                       void *d_workspace, size_t workspace_bytes, hipStream_t stream);
    // the same for a bunch prepared into page-locked memory that stays as it is until the stream has passed the copy this call
    // begins with; `uploaded` (may be null) is recorded behind that copy
    void series_device_prepared(int device, const void *d_mcpes, const void *d_count, size_t capacity, const SeriesBunch &bunch, const uint8_t *h_blob,
                                void *d_out, void *d_series, void *d_counts, void *d_workspace, size_t workspace_bytes, hipStream_t stream,
                                hipEvent_t uploaded = nullptr);

private:
    McpeParams params_{};
    std::vector<double> values_;
    std::vector<uint64_t> dom_table_;
    double pancake_ = 1.;
    std::vector<uint32_t> dom_ranks_;       // beside dom_table_, slot by slot: the DOM's rank in ascending (string ID, OM ID) order
    std::vector<uint32_t> dom_of_rank_;     // record word 11 (string ID | OM ID << 16) by rank
    struct DeviceImage { double *values = nullptr; uint64_t *dom_table = nullptr; uint32_t *dom_ranks = nullptr, *dom_of_rank = nullptr; };
    std::mutex device_mutex_, series_mutex_;
    std::map<int, DeviceImage> images_;
    SeriesStaging staging_;                 // of the stand-alone series call's bunch (series_bunch.h; under series_mutex_)
    DeviceImage image_on(int device);
};

} // namespace clsimhip
