// C++ adapter: the reference's converter interface implemented on the C ABI.
//
// `I3CLSimStepToPhotonConverterHIP` has the member functions of
// I3CLSimStepToPhotonConverter (public/clsim/I3CLSimStepToPhotonConverter.h:67-192)
// and the concrete setters the canonical caller uses
// (public/clsim/I3CLSimStepToPhotonConverterOpenCL.h:78-258,
// private/clsim/I3CLSimModuleHelper.cxx:303-372), with the same names, argument
// meaning and error behaviour (I3CLSimStepToPhotonConverter_exception).
//
// Two builds of the same class:
//  * -DCLSIMHIP_WITH_ICETRAY (inside IceTray): derives from the REAL interface -- the four configuration setters
//    take I3CLSimRandomValueConstPtr / I3CLSimFunctionConstPtr / I3CLSimMediumPropertiesConstPtr /
//    I3CLSimSimpleGeometryConstPtr exactly as public/clsim/I3CLSimStepToPhotonConverter.h:91-124 declares them and
//    translate through I3CLSimStepToPhotonConverterHIPGlue.h; the constructor takes the I3RandomService that seeds the
//    streams (OpenCL.cxx:68-69), SetDevice takes the HIP device ordinal (OpenCL.h:102 takes an I3CLSimOpenCLDevice).
//    This repository compiles and runs that build against tests/stubs/ (tests/test_icetray_adapter.py).
//  * stand-alone (no IceTray headers at all): derives from the minimal interface below, which has the same virtual
//    functions in the same order, and takes the C descriptors directly.
#pragma once
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/clsimhip.h"

#ifdef CLSIMHIP_WITH_ICETRAY
#include <clsim/I3CLSimStepToPhotonConverter.h>
#include <phys-services/I3RandomService.h>
#include "I3CLSimStepToPhotonConverterHIPGlue.h"
#else
// ---- stand-alone counterparts of the reference types ----
typedef clsimhip_step I3CLSimStep;                       // public/clsim/I3CLSimStep.h (48 B blob)
typedef clsimhip_photon I3CLSimPhoton;                   // public/clsim/I3CLSimPhoton.h (80 B blob)
typedef std::vector<I3CLSimStep> I3CLSimStepSeries;
typedef std::vector<I3CLSimPhoton> I3CLSimPhotonSeries;
typedef std::shared_ptr<const I3CLSimStepSeries> I3CLSimStepSeriesConstPtr;
typedef std::shared_ptr<I3CLSimPhotonSeries> I3CLSimPhotonSeriesPtr;
struct I3CLSimPhotonHistory {                            // public/clsim/I3CLSimPhotonHistory.h:41-70 (accessors used here)
    std::size_t size() const { return posX_.size(); }
    float GetX(std::size_t i) const { return posX_[i]; }
    float GetY(std::size_t i) const { return posY_[i]; }
    float GetZ(std::size_t i) const { return posZ_[i]; }
    float GetDistanceInAbsorptionLengths(std::size_t i) const { return distanceInAbsorptionLengths_[i]; }
    void push_back(float x, float y, float z, float abslens)
    {
        posX_.push_back(x); posY_.push_back(y); posZ_.push_back(z); distanceInAbsorptionLengths_.push_back(abslens);
    }
private:
    std::vector<float> posX_, posY_, posZ_, distanceInAbsorptionLengths_;
};
typedef std::vector<I3CLSimPhotonHistory> I3CLSimPhotonHistorySeries;
typedef std::shared_ptr<I3CLSimPhotonHistorySeries> I3CLSimPhotonHistorySeriesPtr;

class I3CLSimStepToPhotonConverter_exception : public std::runtime_error {
public:
    explicit I3CLSimStepToPhotonConverter_exception(const std::string &msg) : std::runtime_error(msg) {}
};

struct I3CLSimStepToPhotonConverter {
    struct ConversionResult_t {
        ConversionResult_t() : identifier(0) {}
        uint32_t identifier;
        I3CLSimPhotonSeriesPtr photons;
        I3CLSimPhotonHistorySeriesPtr photonHistories;  // null unless PhotonHistoryEntries > 0
    };
    virtual ~I3CLSimStepToPhotonConverter() {}
    virtual void SetWlenGenerators(const std::vector<clsimhip_random_value> &wlenGenerators) = 0;
    virtual void SetWlenBias(const clsimhip_function &wlenBias) = 0;
    virtual void SetMediumProperties(const clsimhip_medium *mediumProperties) = 0;
    virtual void SetGeometry(const std::vector<int32_t> &stringIDs, const std::vector<uint32_t> &domIDs,
                             const std::vector<double> &x, const std::vector<double> &y, const std::vector<double> &z,
                             const std::vector<std::string> &subdetectors, double omRadius) = 0;
    virtual void Initialize() = 0;
    virtual bool IsInitialized() const = 0;
    virtual void EnqueueSteps(I3CLSimStepSeriesConstPtr steps, uint32_t identifier) = 0;
    virtual std::size_t GetWorkgroupSize() const = 0;
    virtual std::size_t GetMaxNumWorkitems() const = 0;
    virtual std::size_t QueueSize() const = 0;
    virtual bool MorePhotonsAvailable() const = 0;
    virtual ConversionResult_t GetConversionResult() = 0;
    virtual std::map<std::string, double> GetStatistics() const { return std::map<std::string, double>(); }
};
#endif

static_assert(sizeof(I3CLSimStep) == sizeof(clsimhip_step), "I3CLSimStep must be the 48-byte record of the C ABI");
static_assert(sizeof(I3CLSimPhoton) == sizeof(clsimhip_photon), "I3CLSimPhoton must be the 80-byte record of the C ABI");

class I3CLSimStepToPhotonConverterHIP : public I3CLSimStepToPhotonConverter {
public:
#ifdef CLSIMHIP_WITH_ICETRAY
    // I3CLSimStepToPhotonConverterOpenCL(I3RandomServicePtr, bool useNativeMath) (OpenCL.cxx:68-69); there is one math
    // library here, so the second argument has no counterpart
    explicit I3CLSimStepToPhotonConverterHIP(I3RandomServicePtr randomService, int device = 0) : handle_(nullptr), seed_(12345), randomService_(randomService)
    {
        if (clsimhip_create(device, &handle_) != CLSIMHIP_OK) throw I3CLSimStepToPhotonConverter_exception(clsimhip_last_error(nullptr));
        owner_.reset(handle_, [](clsimhip_converter *h) { clsimhip_destroy(h); });
    }
#else
    explicit I3CLSimStepToPhotonConverterHIP(int device = 0, uint64_t seed = 12345) : handle_(nullptr), seed_(seed)
    {
        if (clsimhip_create(device, &handle_) != CLSIMHIP_OK) throw I3CLSimStepToPhotonConverter_exception(clsimhip_last_error(nullptr));
        owner_.reset(handle_, [](clsimhip_converter *h) { clsimhip_destroy(h); });
    }
#endif
    // the reference interface declares no virtual destructor (I3CLSimStepToPhotonConverter.h:88 has it commented out):
    // converters live in shared_ptrs made from the concrete type, as I3CLSimStepToPhotonConverterOpenCLPtr does
    // (the library's converter goes when this object AND every ConversionResultView handed out by GetConversionResultInPlace() are
    // gone: a view keeps the converter it must return its buffer to alive -- ADVICE r5)
    virtual ~I3CLSimStepToPhotonConverterHIP() {}
    I3CLSimStepToPhotonConverterHIP(const I3CLSimStepToPhotonConverterHIP &) = delete;
    I3CLSimStepToPhotonConverterHIP &operator=(const I3CLSimStepToPhotonConverterHIP &) = delete;

    // ---- interface: configuration ----
#ifdef CLSIMHIP_WITH_ICETRAY
    void SetWlenGenerators(const std::vector<I3CLSimRandomValueConstPtr> &wlenGenerators) override
    {
        std::vector<clsimhip_glue::RandomValueHolder> held(wlenGenerators.size());
        std::vector<clsimhip_random_value> g(wlenGenerators.size());
        for (std::size_t i = 0; i < wlenGenerators.size(); ++i) {
            if (!wlenGenerators[i]) throw I3CLSimStepToPhotonConverter_exception("wavelength generator is (null)!");
            held[i] = clsimhip_glue::MakeHIPWlenGenerator(*wlenGenerators[i], i);
            g[i] = held[i].r;
        }
        check(clsimhip_set_wlen_generators(handle_, g.data(), g.size()));
    }
    void SetWlenBias(I3CLSimFunctionConstPtr wlenBias) override
    {
        if (!wlenBias) throw I3CLSimStepToPhotonConverter_exception("wavelength bias is (null)!");
        const clsimhip_glue::FunctionHolder h = clsimhip_glue::MakeHIPFunction(*wlenBias, "the wavelength bias");
        check(clsimhip_set_wlen_bias(handle_, &h.f));
    }
    void SetMediumProperties(I3CLSimMediumPropertiesConstPtr mediumProperties) override
    {
        if (!mediumProperties) throw I3CLSimStepToPhotonConverter_exception("medium properties are (null)!");
        clsimhip_glue::MediumHolder h;
        clsimhip_glue::MakeHIPMedium(*mediumProperties, h);
        check(clsimhip_set_medium_properties(handle_, h.m));
    }
    // the seven vectors the reference hands to its geometry code generator (GeometrySource.cxx:88-99)
    void SetGeometry(I3CLSimSimpleGeometryConstPtr geometry) override
    {
        if (!geometry) throw I3CLSimStepToPhotonConverter_exception("geometry is (null)!");
        const std::vector<std::string> &sub = geometry->GetSubdetectorVector();
        std::vector<const char *> names;
        for (const std::string &s : sub) names.push_back(s.c_str());
        check(clsimhip_set_geometry(handle_, geometry->size(), geometry->GetStringIDVector().data(), geometry->GetDomIDVector().data(),
                                    geometry->GetPosXVector().data(), geometry->GetPosYVector().data(), geometry->GetPosZVector().data(),
                                    names.data(), geometry->GetOMRadius()));
    }
    // streams seeded from the random service like init_MWC_RNG does (private/opencl/mwcrng_init.h:104-112); the
    // multipliers are the library's (the same safeprimes the reference reads from its file)
    void Initialize() override
    {
        if (!randomService_) { check(clsimhip_initialize(handle_, seed_)); return; }
        if (IsInitialized()) throw I3CLSimStepToPhotonConverter_exception("I3CLSimStepToPhotonConverterHIP already initialized!");
        check(clsimhip_compile(handle_));
        std::size_t n = 0;
        check(clsimhip_get_max_num_workitems(handle_, &n));
        if (n == 0) { n = 1048576; check(clsimhip_set_max_num_workitems(handle_, n)); }
        std::vector<uint32_t> a(n);
        std::vector<uint64_t> x(n, 0);
        check(clsimhip_mwc_multipliers(a.data(), n));
        for (std::size_t i = 0; i < n; ++i) {
            while ((x[i] == 0) | ((static_cast<uint32_t>(x[i] >> 32)) >= (a[i] - 1)) | ((static_cast<uint32_t>(x[i])) >= 0xfffffffful)) {
                x[i] = static_cast<uint32_t>(randomService_->Integer(0xffffffff));
                x[i] = x[i] << 32;
                x[i] += static_cast<uint32_t>(randomService_->Integer(0xffffffff));
            }
        }
        check(clsimhip_initialize_with_streams(handle_, x.data(), a.data(), n));
    }
#else
    void SetWlenGenerators(const std::vector<clsimhip_random_value> &g) override { check(clsimhip_set_wlen_generators(handle_, g.data(), g.size())); }
    void SetWlenBias(const clsimhip_function &b) override { check(clsimhip_set_wlen_bias(handle_, &b)); }
    void SetMediumProperties(const clsimhip_medium *m) override { check(clsimhip_set_medium_properties(handle_, m)); }
    void SetGeometry(const std::vector<int32_t> &stringIDs, const std::vector<uint32_t> &domIDs, const std::vector<double> &x,
                     const std::vector<double> &y, const std::vector<double> &z, const std::vector<std::string> &subdetectors,
                     double omRadius) override
    {
        std::vector<const char *> names;
        for (const std::string &s : subdetectors) names.push_back(s.c_str());
        check(clsimhip_set_geometry(handle_, stringIDs.size(), stringIDs.data(), domIDs.data(), x.data(), y.data(), z.data(),
                                    names.data(), omRadius));
    }
    void Initialize() override { check(clsimhip_initialize(handle_, seed_)); }
#endif
    void InitializeWithStreams(const std::vector<uint64_t> &x, const std::vector<uint32_t> &a) { check(clsimhip_initialize_with_streams(handle_, x.data(), a.data(), x.size())); }

    // ---- interface: steady state ----
    bool IsInitialized() const override { return clsimhip_is_initialized(handle_) != 0; }
    void EnqueueSteps(I3CLSimStepSeriesConstPtr steps, uint32_t identifier) override
    {
        if (!steps) {   // the null check comes after the initialisation check in the reference (OpenCL.cxx:1527-1531)
            if (!IsInitialized()) throw I3CLSimStepToPhotonConverter_exception("I3CLSimStepToPhotonConverterHIP is not initialized!");
            throw I3CLSimStepToPhotonConverter_exception("Steps pointer is (null)!");
        }
        check(clsimhip_enqueue_steps(handle_, reinterpret_cast<const clsimhip_step *>(steps->data()), steps->size(), identifier));
    }
    std::size_t GetWorkgroupSize() const override { size_t v = 0; check(clsimhip_get_workgroup_size(handle_, &v)); return v; }
    std::size_t GetMaxNumWorkitems() const override { size_t v = 0; check(clsimhip_get_max_num_workitems(handle_, &v)); return v; }
    std::size_t QueueSize() const override { size_t v = 0; check(clsimhip_queue_size(handle_, &v)); return v; }
    bool MorePhotonsAvailable() const override { int v = 0; check(clsimhip_more_photons_available(handle_, &v)); return v != 0; }
    ConversionResult_t GetConversionResult() override
    {
        ConversionResult_t r;
        const clsimhip_photon *p = nullptr;
        size_t n = 0;
        check(clsimhip_get_conversion_result(handle_, &r.identifier, &p, &n));
        r.photons = I3CLSimPhotonSeriesPtr(new I3CLSimPhotonSeries(n));
        lastMCPEs_.clear();
        lastSeries_.clear();
        lastMerged_.clear(); lastMergedSeries_.clear(); lastParents_.clear(); lastParentRanges_.clear();
        lastMasked_ = 0;
        lastFramePhotons_.clear();
        lastFramePhotonSeries_.clear();
        lastMaskedFramePhotons_ = 0;
        lastShadowFlags_.clear();
        lastShadowCounts_[0] = 0; lastShadowCounts_[1] = 0;
        lastEventStatistics_.clear();
        lastEventStatisticsCounters_[0] = 0; lastEventStatisticsCounters_[1] = 0; lastEventStatisticsCounters_[2] = 0;
        if (eventStatistics_) {     // (before every other getter: whichever comes last releases a result without photon records)
            const clsimhip_event_statistics *e = nullptr;
            size_t ne = 0;
            check(clsimhip_get_result_event_statistics(handle_, p, &e, &ne, lastEventStatisticsCounters_));
            lastEventStatistics_.assign(e, e + ne);
            if (!n && !cableShadow_ && !framePhotons_ && !mcpeGenerator_ && !pmtHitGenerator_) check(clsimhip_release_result(handle_, p));
        }
        if (cableShadow_) {         // (before every other getter but that one: whichever comes last releases a result without photon records)
            const uint8_t *flags = nullptr;
            size_t nf = 0;
            check(clsimhip_get_result_cable_shadow(handle_, p, &flags, &nf, lastShadowCounts_));
            lastShadowFlags_.assign(flags, flags + nf);
            if (!n && !framePhotons_ && !mcpeGenerator_ && !pmtHitGenerator_) check(clsimhip_release_result(handle_, p));
        }
        if (framePhotons_) {        // (fetched first: a result without photon records is released behind the last getter)
            const clsimhip_frame_photon *f = nullptr;
            const clsimhip_mcpe_series *s = nullptr;
            size_t nf = 0, ns = 0;
            check(clsimhip_get_result_frame_photons(handle_, p, &f, &nf, &s, &ns, &lastMaskedFramePhotons_));
            lastFramePhotons_.assign(f, f + nf);
            lastFramePhotonSeries_.assign(s, s + ns);
            if (!n && !mcpeGenerator_ && !pmtHitGenerator_) check(clsimhip_release_result(handle_, p));
        }
        if (mcpeGenerator_) {       // (ConversionResult_t has no place for them: GetLastMCPEs())
            const clsimhip_mcpe *m = nullptr;
            size_t nm = 0;
            if (mcpeSeries_) {
                const clsimhip_mcpe_series *s = nullptr;
                size_t ns = 0;
                check(clsimhip_get_result_mcpe_series(handle_, p, &m, &nm, &s, &ns, &lastMasked_));
                lastSeries_.assign(s, s + ns);
                if (mcpeMerging_) {
                    const clsimhip_mcpe_merged *g = nullptr;
                    const clsimhip_mcpe_parent *q = nullptr;
                    const clsimhip_mcpe_parent_range *ranges = nullptr;
                    size_t ng = 0, nq = 0;
                    check(clsimhip_get_result_mcpe_merged(handle_, p, &g, &ng, &s, &ns, &q, &nq, &ranges));
                    lastMerged_.assign(g, g + ng);
                    lastMergedSeries_.assign(s, s + ns);
                    lastParents_.assign(q, q + nq);
                    lastParentRanges_.assign(ranges, ranges + ns);
                }
            } else
                check(clsimhip_get_result_mcpes(handle_, p, &m, &nm));
            lastMCPEs_.assign(m, m + nm);
            if (!n) check(clsimhip_release_result(handle_, p));     // the handle of a result without photon records
        }
        lastPMTHits_.clear();
        lastPMTSeries_.clear();
        if (pmtHitGenerator_) {     // (likewise: GetLastPMTHits())
            const clsimhip_pmt_hit *h = nullptr;
            size_t nh = 0;
            if (pmtSeries_) {
                const clsimhip_pmt_series *s = nullptr;
                size_t ns = 0;
                check(clsimhip_get_result_pmt_series(handle_, p, &h, &nh, &s, &ns, &lastMasked_));
                lastPMTSeries_.assign(s, s + ns);
            } else
                check(clsimhip_get_result_pmt_hits(handle_, p, &h, &nh));
            lastPMTHits_.assign(h, h + nh);
            if (!n) check(clsimhip_release_result(handle_, p));
        }
        if (n) {
            std::memcpy(static_cast<void *>(r.photons->data()), p, n * sizeof(clsimhip_photon));
            // I3CLSimPhotonHistory (public/clsim/I3CLSimPhotonHistory.h): per photon the recorded scatter points
            const float *h = nullptr;
            uint32_t entries = 0;
            check(clsimhip_get_result_histories(handle_, p, &h, &entries));
            if (h && entries) {
                r.photonHistories = I3CLSimPhotonHistorySeriesPtr(new I3CLSimPhotonHistorySeries(n));
                for (size_t i = 0; i < n; ++i) {
                    const uint32_t k = p[i].num_scatters < entries ? p[i].num_scatters : entries;
                    for (uint32_t j = 0; j < k; ++j) {
                        const float *e = h + (i * entries + j) * 4;
                        (*r.photonHistories)[i].push_back(e[0], e[1], e[2], e[3]);
                    }
                }
            }
            check(clsimhip_release_result(handle_, p));
        }
        return r;
    }
    // Extension (no reference counterpart): the result where the library left it -- the page-locked buffer the device's records were
    // downloaded into -- for a caller that consumes the records in place (a server that serialises them, a hit maker that walks
    // them once): no I3CLSimPhotonSeries is allocated, nothing is copied.  `photons` stays valid while `hold` (or a copy of it) lives
    // -- also beyond this adapter's own lifetime: `hold` shares ownership of the library's converter, which is destroyed (and its
    // page-locked buffers freed) only after the adapter and the last view are gone.  The buffer goes back to the converter's pool
    // when the last copy is dropped.  Photon histories, if recorded, are not part
    // of the view: use GetConversionResult().  GetConversionResult() copies because its interface type owns a std::vector.
    struct ConversionResultView {
        uint32_t identifier = 0;
        const I3CLSimPhoton *photons = nullptr;
        std::size_t size = 0;
        std::shared_ptr<const void> hold;
        const clsimhip_mcpe *mcpes = nullptr;       // with an MCPE generator: the bunch's MCPEs, valid as long as `photons`
        std::size_t numMCPEs = 0;
        const clsimhip_pmt_hit *pmtHits = nullptr;  // with a PMT hit generator: the bunch's hits, valid as long as `photons`
        std::size_t numPMTHits = 0;
        const uint8_t *shadowFlags = nullptr;       // with the cable shadow stage: one flag per photon record (1 = shadowed), valid as long as `photons`
        std::size_t numShadowFlags = 0;
        uint64_t shadowCounts[2] = {0, 0};          // records tested, records shadowed
        const clsimhip_event_statistics *eventStatistics = nullptr;     // with the event statistics stage: its records, valid as long as `photons`
        std::size_t numEventStatistics = 0;
        uint64_t eventStatisticsCounters[3] = {0, 0, 0};
        const I3CLSimPhoton *begin() const { return photons; }
        const I3CLSimPhoton *end() const { return photons + size; }
    };
    ConversionResultView GetConversionResultInPlace()
    {
        ConversionResultView v;
        const clsimhip_photon *p = nullptr;
        check(clsimhip_get_conversion_result(handle_, &v.identifier, &p, &v.size));
        v.photons = reinterpret_cast<const I3CLSimPhoton *>(p);
        if (mcpeGenerator_) check(clsimhip_get_result_mcpes(handle_, p, &v.mcpes, &v.numMCPEs));
        if (pmtHitGenerator_) check(clsimhip_get_result_pmt_hits(handle_, p, &v.pmtHits, &v.numPMTHits));
        if (cableShadow_) check(clsimhip_get_result_cable_shadow(handle_, p, &v.shadowFlags, &v.numShadowFlags, v.shadowCounts));
        if (eventStatistics_) check(clsimhip_get_result_event_statistics(handle_, p, &v.eventStatistics, &v.numEventStatistics, v.eventStatisticsCounters));
        if (p) {
            std::shared_ptr<clsimhip_converter> keep = owner_;
            v.hold = std::shared_ptr<const void>(static_cast<const void *>(p), [keep](const void *q) { (void)clsimhip_release_result(keep.get(), static_cast<const clsimhip_photon *>(q)); });
        }
        return v;
    }
    std::map<std::string, double> GetStatistics() const override
    {
        double v[8];
        check(clsimhip_get_statistics(handle_, v));
        static const char *keys[8] = {"TotalDeviceTime", "TotalHostTime", "NumKernelCalls", "TotalNumPhotonsGenerated",
                                      "TotalNumPhotonsAtDOMs", "AverageDeviceTimePerPhoton", "AverageHostTimePerPhoton", "DeviceUtilization"};
        std::map<std::string, double> m;
        for (int i = 0; i < 8; ++i) m[keys[i]] = v[i];
        return m;
    }

    // the statistics accessors I3CLSimModule::Finish reads from the concrete class (OpenCL.h:377-381, I3CLSimModule.cxx:1626-1634):
    // times in nanoseconds
    double GetTotalDeviceTime() const { return stat(0); }
    double GetTotalHostTime() const { return stat(1); }
    uint64_t GetNumKernelCalls() const { return static_cast<uint64_t>(stat(2)); }
    uint64_t GetTotalNumPhotonsGenerated() const { return static_cast<uint64_t>(stat(3)); }
    uint64_t GetTotalNumPhotonsAtDOMs() const { return static_cast<uint64_t>(stat(4)); }

    // ---- tuning (no reference counterpart; keys and ranges: include/clsimhip.h, clsimhip_set_tuning).  No result depends on it; the library
    // reads none of it from the environment ----
    void SetTuning(const std::string &key, long long value) { check(clsimhip_set_tuning(handle_, key.c_str(), value)); }
    long long GetTuning(const std::string &key) const
    {
        long long v = 0;
        check(clsimhip_get_tuning(handle_, key.c_str(), &v));
        return v;
    }

    // ---- concrete setters and getters of the OpenCL converter (OpenCL.h:78-258) ----
    bool GetEnableDoubleBuffering() const { return option(CLSIMHIP_OPTION_ENABLE_DOUBLE_BUFFERING) != 0.; }
    bool GetDoublePrecision() const { return option(CLSIMHIP_OPTION_DOUBLE_PRECISION) != 0.; }
    bool GetStopDetectedPhotons() const { return option(CLSIMHIP_OPTION_STOP_DETECTED_PHOTONS) != 0.; }
    bool GetSaveAllPhotons() const { return option(CLSIMHIP_OPTION_SAVE_ALL_PHOTONS) != 0.; }
    double GetSaveAllPhotonsPrescale() const { return option(CLSIMHIP_OPTION_SAVE_ALL_PHOTONS_PRESCALE); }
    double GetFixedNumberOfAbsorptionLengths() const { return option(CLSIMHIP_OPTION_FIXED_NUMBER_OF_ABSORPTION_LENGTHS); }
    double GetDOMPancakeFactor() const { return option(CLSIMHIP_OPTION_DOM_PANCAKE_FACTOR); }
    uint32_t GetPhotonHistoryEntries() const { return static_cast<uint32_t>(option(CLSIMHIP_OPTION_PHOTON_HISTORY_ENTRIES)); }
    void SetDevice(int hipDeviceOrdinal) { check(clsimhip_set_device(handle_, hipDeviceOrdinal)); }
    void SetEnableDoubleBuffering(bool v) { check(clsimhip_set_enable_double_buffering(handle_, v)); }
    void SetDoublePrecision(bool v) { check(clsimhip_set_double_precision(handle_, v)); }
    void SetStopDetectedPhotons(bool v) { check(clsimhip_set_stop_detected_photons(handle_, v)); }
    void SetSaveAllPhotons(bool v) { check(clsimhip_set_save_all_photons(handle_, v)); }
    void SetSaveAllPhotonsPrescale(double v) { check(clsimhip_set_save_all_photons_prescale(handle_, v)); }
    void SetFixedNumberOfAbsorptionLengths(double v) { check(clsimhip_set_fixed_number_of_absorption_lengths(handle_, v)); }
    void SetDOMPancakeFactor(double v) { check(clsimhip_set_dom_pancake_factor(handle_, v)); }
    void SetPhotonHistoryEntries(uint32_t v) { check(clsimhip_set_photon_history_entries(handle_, v)); }
    void SetWorkgroupSize(std::size_t v) { check(clsimhip_set_workgroup_size(handle_, v)); }
    void SetMaxNumWorkitems(std::size_t v) { check(clsimhip_set_max_num_workitems(handle_, v)); }
    void Compile() { check(clsimhip_compile(handle_)); }
    std::size_t GetMaxWorkgroupSize() const { size_t v = 0; check(clsimhip_get_max_workgroup_size(handle_, &v)); return v; }
    clsimhip_converter *Handle() { return handle_; }

    // ---- MCPE generator (no reference counterpart: the reference makes MCPEs from the returned photons on a host thread,
    // I3CLSimClientModule.cxx:359-439; include/clsimhip.h, "MCPE generator").  Before Initialize(); nullptr switches it off.  With
    // keepPhotons = false results carry no photon records.  The generator object stays the caller's (the converter shares it). ----
    void SetMCPEGenerator(clsimhip_mcpe_generator *generator, bool keepPhotons = true)
    {
        check(clsimhip_set_mcpe_generator(handle_, generator, keepPhotons ? 1 : 0));
        mcpeGenerator_ = generator != nullptr;
    }
    // the MCPEs of the bunch the last GetConversionResult() returned (its identifier: that result's), in no particular order --
    // with SetMCPESeries(true) in the order of the series
    const std::vector<clsimhip_mcpe> &GetLastMCPEs() const { return lastMCPEs_; }

    // ---- Multi-PMT hit generator (include/clsimhip.h, "Multi-PMT hit generator": what I3PhotonToMCHitConverterForMultiPMT does with the
    // photons of a frame, on the GPU behind the propagator).  Before Initialize(); nullptr switches it off; not beside an MCPE
    // generator (Compile() refuses).  The generator object stays the caller's (the converter shares it). ----
    void SetPMTHitGenerator(clsimhip_pmt_generator *generator, bool keepPhotons = true)
    {
        check(clsimhip_set_pmt_generator(handle_, generator, keepPhotons ? 1 : 0));
        pmtHitGenerator_ = generator != nullptr;
    }
    // the hits of the bunch the last GetConversionResult() returned, in no particular order -- with SetPMTSeries(true) in the order
    // of the series
    const std::vector<clsimhip_pmt_hit> &GetLastPMTHits() const { return lastPMTHits_; }

    // ---- PMT series (include/clsimhip.h, "PMT series"): what replaces the client module's AddPhotonsToFrames loop and the filing
    // and per-PMT time sort of I3PhotonToMCHitConverterForMultiPMT::DAQ.  Before Initialize(); needs a PMT hit generator.  A bunch is
    // enqueued with its particle table and its frames' ignored modules (EnqueueSteps below); its result's hits come back per frame,
    // per module in OMKey order, per PMT, in time order. ----
    void SetPMTSeries(bool on = true)
    {
        check(clsimhip_set_pmt_series(handle_, on ? 1 : 0));
        pmtSeries_ = on;
    }
    // the flat views of the last result: GetLastPMTHits() and its series table (entries partition the records), the MASKED count
    const std::vector<clsimhip_pmt_series> &GetLastPMTSeries() const { return lastPMTSeries_; }
    uint64_t GetLastMaskedPMTHits() const { return lastMasked_; }
    // ... and as the frames receive them: frame -> (string ID, OM ID) -> PMT -> time-ordered hits (an I3MCHitSeriesMultiOMMap per frame)
    typedef std::map<std::pair<int, unsigned>, std::map<uint32_t, std::vector<clsimhip_pmt_hit> > > PMTHitSeriesMap;
    std::map<uint32_t, PMTHitSeriesMap> GetLastPMTSeriesMaps() const
    {
        std::map<uint32_t, PMTHitSeriesMap> frames;
        for (const clsimhip_pmt_series &s : lastPMTSeries_)
            frames[s.frame][std::make_pair(static_cast<int>(s.string_id), static_cast<unsigned>(s.om_id))][s.pmt]
                .assign(lastPMTHits_.begin() + s.first, lastPMTHits_.begin() + s.first + s.count);
        return frames;
    }

    // ---- Event statistics (include/clsimhip.h, "Event statistics"): the client module's I3CLSimEventStatistics -- per particle of the
    // bunch's table (EnqueueSteps with particles below; without one: one record) the photons generated and the photons at DOMs, as
    // counts and as exact integer weight sums (clsimhip_event_statistics_weight turns one into a double, rounded once;
    // clsimhip_event_statistics_add adds two bunches' records exactly).  Before Initialize().  It sees ALL detected photons, also with a
    // cable shadow bound, and works with keepPhotons = false. ----
    void SetEventStatistics(bool on = true)
    {
        check(clsimhip_set_event_statistics(handle_, on ? 1 : 0));
        eventStatistics_ = on;
    }
    // of the last result: one record per table entry in table order, and the counters (CLSIMHIP_EVENT_STATISTICS_*)
    const std::vector<clsimhip_event_statistics> &GetLastEventStatistics() const { return lastEventStatistics_; }
    uint64_t GetLastEventStatisticsCounter(int which) const { return which >= 0 && which < 3 ? lastEventStatisticsCounters_[which] : 0; }

    // ---- Cable shadow (include/clsimhip.h, "Cable shadow"): the reference's I3ShadowedPhotonRemoverModule as a stage right behind the
    // propagation kernel.  Before Initialize(); shadow = nullptr switches it off.  The photons of a result stay ALL detected photons
    // (PropagatedPhotons); the flags say which of them PropagatedPhotonsWithShadow would not hold, and every hit maker and series
    // stage attached works on the lit ones.  The cylinder set is the caller's (clsimhip_cable_shadow_create); it may be destroyed
    // once this call has returned. ----
    void SetCableShadow(clsimhip_cable_shadow *shadow)
    {
        check(clsimhip_set_cable_shadow(handle_, shadow));
        cableShadow_ = shadow != nullptr;
    }
    // of the last result: one flag per photon record it carried (1 = shadowed), records tested and records shadowed
    const std::vector<uint8_t> &GetLastShadowFlags() const { return lastShadowFlags_; }
    uint64_t GetLastShadowTested() const { return lastShadowCounts_[0]; }
    uint64_t GetLastShadowShadowed() const { return lastShadowCounts_[1]; }

    // ---- Frame photons (include/clsimhip.h, "Frame photons"): the client module's PropagatedPhotons, an I3CompressedPhotonSeriesMap per
    // frame, made on the GPU from the bunch's photon records.  Before Initialize(); beside either hit generator or none.  A bunch is
    // enqueued with its particle table and its frames' ignored modules (EnqueueSteps below); keepPhotons = false leaves the 80-byte
    // records on the device. ----
    void SetFramePhotons(bool on = true, bool keepPhotons = true)
    {
        check(clsimhip_set_frame_photons(handle_, on ? 1 : 0, keepPhotons ? 1 : 0));
        framePhotons_ = on;
    }
    // the flat views of the last result: the records in the order of the series, the series table (entries partition the records),
    // the MASKED count
    const std::vector<clsimhip_frame_photon> &GetLastFramePhotons() const { return lastFramePhotons_; }
    const std::vector<clsimhip_mcpe_series> &GetLastFramePhotonSeries() const { return lastFramePhotonSeries_; }
    uint64_t GetLastMaskedFramePhotons() const { return lastMaskedFramePhotons_; }
    // ... and as the frames receive them: frame -> (string ID, OM ID) -> the module's photons
    typedef std::map<std::pair<int, unsigned>, std::vector<clsimhip_frame_photon> > FramePhotonSeriesMap;
    std::map<uint32_t, FramePhotonSeriesMap> GetLastFramePhotonMaps() const
    {
        std::map<uint32_t, FramePhotonSeriesMap> frames;
        for (const clsimhip_mcpe_series &s : lastFramePhotonSeries_)
            frames[s.frame][std::make_pair(static_cast<int>(s.string_id), static_cast<unsigned>(s.om_id))]
                .assign(lastFramePhotons_.begin() + s.first, lastFramePhotons_.begin() + s.first + s.count);
        return frames;
    }

    // ---- MCPE series (include/clsimhip.h, "MCPE series"): what replaces the client module's AddPhotonsToFrames loop and the per-DOM
    // time sort.  Before Initialize(); needs a generator.  A bunch is enqueued with its particle table (strictly increasing in
    // identifier) and its frames' ignored modules; its result's MCPEs come back per frame, per DOM in OMKey order, in time order. ----
    void SetMCPESeries(bool on = true)
    {
        check(clsimhip_set_mcpe_series(handle_, on ? 1 : 0));
        mcpeSeries_ = on;
    }
    void EnqueueSteps(I3CLSimStepSeriesConstPtr steps, uint32_t identifier, const std::vector<clsimhip_mcpe_particle> &particles,
                      const std::vector<clsimhip_mcpe_mask> &ignored = std::vector<clsimhip_mcpe_mask>())
    {
        if (!steps) throw I3CLSimStepToPhotonConverter_exception("Steps pointer is (null)!");
        static const clsimhip_mcpe_particle none = {0u, 0u, 0.};       // (an empty table is still a table)
        check(clsimhip_enqueue_steps_with_particles(handle_, reinterpret_cast<const clsimhip_step *>(steps->data()), steps->size(), identifier,
                                                    particles.empty() ? &none : particles.data(), particles.size(),
                                                    ignored.empty() ? nullptr : ignored.data(), ignored.size()));
    }
    // the flat views of the last result: GetLastMCPEs() and its series table (entries partition the records), the MASKED count
    const std::vector<clsimhip_mcpe_series> &GetLastMCPESeries() const { return lastSeries_; }
    uint64_t GetLastMaskedMCPEs() const { return lastMasked_; }
    // ... and as the frames receive them: frame -> (string ID, OM ID) -> time-ordered MCPEs (an I3MCPESeriesMap per frame)
    typedef std::map<std::pair<int, unsigned>, std::vector<clsimhip_mcpe> > MCPESeriesMap;
    std::map<uint32_t, MCPESeriesMap> GetLastMCPESeriesMaps() const
    {
        std::map<uint32_t, MCPESeriesMap> frames;
        for (const clsimhip_mcpe_series &s : lastSeries_)
            frames[s.frame][std::make_pair(static_cast<int>(s.string_id), static_cast<unsigned>(s.om_id))]
                .assign(lastMCPEs_.begin() + s.first, lastMCPEs_.begin() + s.first + s.count);
        return frames;
    }

    // ---- MCPE merging (include/clsimhip.h, "MCPE merging"): what stands where the client module's MCHitMerging::MCPEStream and
    // extractMCPEsWithPIDInfo() do -- this project's own rule, unpinned against the reference.  Before Initialize(); needs
    // SetMCPESeries.  GetLastMCPEs() / GetLastMCPESeries() stay the unmerged series. ----
    void SetMCPEMerging(double window, bool on = true)
    {
        check(clsimhip_set_mcpe_merging(handle_, on ? 1 : 0, window));
        mcpeMerging_ = on;
    }
    // the flat views of the last result: merged records, their series table (the entries of GetLastMCPESeries(), over the merged
    // records), the parent table and one range of it per series
    const std::vector<clsimhip_mcpe_merged> &GetLastMergedMCPEs() const { return lastMerged_; }
    const std::vector<clsimhip_mcpe_series> &GetLastMergedMCPESeries() const { return lastMergedSeries_; }
    const std::vector<clsimhip_mcpe_parent> &GetLastMCPEParents() const { return lastParents_; }
    const std::vector<clsimhip_mcpe_parent_range> &GetLastMCPEParentRanges() const { return lastParentRanges_; }
    // ... and as the frames receive them: frame -> (string ID, OM ID) -> merged MCPEs (an I3MCPESeriesMap per frame), and
    // frame -> (string ID, OM ID) -> identifier -> indices into that DOM's merged MCPEs, ascending (an I3ParticleIDMap per frame)
    typedef std::map<std::pair<int, unsigned>, std::vector<clsimhip_mcpe_merged> > MergedMCPESeriesMap;
    typedef std::map<std::pair<int, unsigned>, std::map<uint32_t, std::vector<uint32_t> > > ParticleIDMap;
    std::map<uint32_t, MergedMCPESeriesMap> GetLastMergedMCPESeriesMaps() const
    {
        std::map<uint32_t, MergedMCPESeriesMap> frames;
        for (const clsimhip_mcpe_series &s : lastMergedSeries_)
            frames[s.frame][std::make_pair(static_cast<int>(s.string_id), static_cast<unsigned>(s.om_id))]
                .assign(lastMerged_.begin() + s.first, lastMerged_.begin() + s.first + s.count);
        return frames;
    }
    std::map<uint32_t, ParticleIDMap> GetLastParticleIDMaps() const
    {
        std::map<uint32_t, ParticleIDMap> frames;
        for (size_t k = 0; k < lastMergedSeries_.size(); ++k) {
            const clsimhip_mcpe_series &s = lastMergedSeries_[k];
            std::map<uint32_t, std::vector<uint32_t> > &dom = frames[s.frame][std::make_pair(static_cast<int>(s.string_id), static_cast<unsigned>(s.om_id))];
            for (uint32_t i = lastParentRanges_[k].first; i < lastParentRanges_[k].first + lastParentRanges_[k].count; ++i)
                dom[lastParents_[i].identifier].push_back(lastParents_[i].index);
        }
        return frames;
    }

private:
    void check(int rc) const
    {
        if (rc == CLSIMHIP_OK) return;
#ifdef CLSIMHIP_WITH_ICETRAY
        // a device error is where the reference's worker log_fatal()s (OpenCL.cxx:768-774)
        if (rc == CLSIMHIP_ERR_DEVICE) log_fatal("%s", clsimhip_last_error(handle_));
#endif
        throw I3CLSimStepToPhotonConverter_exception(clsimhip_last_error(handle_));
    }
    double stat(int i) const { double v[8]; check(clsimhip_get_statistics(handle_, v)); return v[i]; }
    double option(int which) const { double v = 0.; check(clsimhip_get_option(handle_, which, &v)); return v; }
    clsimhip_converter *handle_;
    std::shared_ptr<clsimhip_converter> owner_;      // owns handle_ (deleter: clsimhip_destroy); shared with the in-place result views
    uint64_t seed_;
    bool mcpeGenerator_ = false;
    std::vector<clsimhip_mcpe> lastMCPEs_;
    bool mcpeSeries_ = false;
    std::vector<clsimhip_mcpe_series> lastSeries_;
    uint64_t lastMasked_ = 0;
    bool mcpeMerging_ = false;
    std::vector<clsimhip_mcpe_merged> lastMerged_;
    std::vector<clsimhip_mcpe_series> lastMergedSeries_;
    std::vector<clsimhip_mcpe_parent> lastParents_;
    std::vector<clsimhip_mcpe_parent_range> lastParentRanges_;
    bool pmtHitGenerator_ = false;
    std::vector<clsimhip_pmt_hit> lastPMTHits_;
    bool pmtSeries_ = false;
    bool framePhotons_ = false;
    bool cableShadow_ = false;
    bool eventStatistics_ = false;
    std::vector<clsimhip_event_statistics> lastEventStatistics_;
    uint64_t lastEventStatisticsCounters_[3] = {0, 0, 0};
    std::vector<uint8_t> lastShadowFlags_;
    uint64_t lastShadowCounts_[2] = {0, 0};
    std::vector<clsimhip_frame_photon> lastFramePhotons_;
    std::vector<clsimhip_mcpe_series> lastFramePhotonSeries_;
    uint64_t lastMaskedFramePhotons_ = 0;
    std::vector<clsimhip_pmt_series> lastPMTSeries_;
#ifdef CLSIMHIP_WITH_ICETRAY
    I3RandomServicePtr randomService_;
#endif
};

#ifdef CLSIMHIP_WITH_ICETRAY
typedef boost::shared_ptr<I3CLSimStepToPhotonConverterHIP> I3CLSimStepToPhotonConverterHIPPtr;

namespace I3CLSimModuleHelper {
// initializeOpenCL (private/clsim/I3CLSimModuleHelper.cxx:303-372) with a HIP device ordinal in the place of the
// I3CLSimOpenCLDevice (its GetApproximateNumberOfWorkItems() becomes an argument): the same calls in the same order
inline I3CLSimStepToPhotonConverterHIPPtr initializeHIP(int device, uint32_t approximateNumberOfWorkItems, I3RandomServicePtr rng,
                                                        I3CLSimSimpleGeometryConstPtr geometry, I3CLSimMediumPropertiesConstPtr medium,
                                                        I3CLSimFunctionConstPtr wavelengthGenerationBias,
                                                        const std::vector<I3CLSimRandomValueConstPtr> &wavelengthGenerators,
                                                        bool enableDoubleBuffering, bool doublePrecision, bool stopDetectedPhotons,
                                                        bool saveAllPhotons, double saveAllPhotonsPrescale, double fixedNumberOfAbsorptionLengths,
                                                        double pancakeFactor, uint32_t photonHistoryEntries, uint32_t limitWorkgroupSize)
{
    I3CLSimStepToPhotonConverterHIPPtr conv(new I3CLSimStepToPhotonConverterHIP(rng));
    conv->SetDevice(device);
    conv->SetWlenGenerators(wavelengthGenerators);
    conv->SetWlenBias(wavelengthGenerationBias);
    conv->SetMediumProperties(medium);
    conv->SetGeometry(geometry);
    conv->SetEnableDoubleBuffering(enableDoubleBuffering);
    conv->SetDoublePrecision(doublePrecision);
    conv->SetStopDetectedPhotons(stopDetectedPhotons);
    conv->SetSaveAllPhotons(saveAllPhotons);
    conv->SetSaveAllPhotonsPrescale(saveAllPhotonsPrescale);
    conv->SetFixedNumberOfAbsorptionLengths(fixedNumberOfAbsorptionLengths);
    conv->SetDOMPancakeFactor(pancakeFactor);
    conv->SetPhotonHistoryEntries(photonHistoryEntries);
    conv->Compile();
    std::size_t maxWorkgroupSize = conv->GetMaxWorkgroupSize();
    if (limitWorkgroupSize != 0 && limitWorkgroupSize < maxWorkgroupSize) maxWorkgroupSize = limitWorkgroupSize;
    conv->SetWorkgroupSize(maxWorkgroupSize);
    const std::size_t workgroupSize = conv->GetWorkgroupSize();
    std::size_t maxNumWorkitems = (static_cast<std::size_t>(approximateNumberOfWorkItems) / workgroupSize) * workgroupSize;
    if (maxNumWorkitems == 0) maxNumWorkitems = workgroupSize;
    conv->SetMaxNumWorkitems(maxNumWorkitems);
    conv->Initialize();
    return conv;
}
}
#endif
