// C++ adapter: the reference's hit maker for segmented modules, I3PhotonToMCHitConverterForMultiPMT
// (private/clsim/dom/I3PhotonToMCHitConverterForMultiPMT.cxx), on the C ABI's PMT photon hits stage (include/clsimhip.h: "PMT photon
// hits").
//
// The setters carry the module's parameter names (I3PhotonToMCHitConverterForMultiPMT.cxx:64-82): InputPhotonSeriesMapName,
// OutputMultiOMMCHitMapName and MCTreeName are kept for the caller, who reads and writes the frame; in place of RandomService there
// is Seed: the draw is a hash of the record and this seed.  What the module reads from the geometry -- I3OMTypeInfo per module type,
// position and orientation per module -- the caller hands over as the generator's description (functions, types, PMTs, modules).
// Convert() takes the stored photons of one or more frames as the frame photons stage delivers them and returns the hits, time-sorted
// per (frame, module, PMT), with their series table.  The MCTree lookup (:356-360) stays with the caller: a hit carries the photon's
// identifier.  A condition the reference ends the run on throws here with its text.  Header-only; needs nothing but include/clsimhip.h
// and libclsimhip.so.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/clsimhip.h"

class I3PhotonToMCHitConverterForMultiPMT_exception : public std::runtime_error {
public:
    explicit I3PhotonToMCHitConverterForMultiPMT_exception(const std::string &msg) : std::runtime_error(msg) {}
};

class I3PhotonToMCHitConverterForMultiPMTHIP {
public:
    struct Result {
        std::vector<clsimhip_pmt_hit> hits;                 // ascending in (input series, PMT, time key, identifier)
        std::vector<clsimhip_pmt_series> series;            // one entry per non-empty (input series, PMT)
        uint64_t offSurface = 0;                            // positions more than 3 cm off the module's sphere (the reference warns)
    };

    I3PhotonToMCHitConverterForMultiPMTHIP() {}
    ~I3PhotonToMCHitConverterForMultiPMTHIP() { clsimhip_pmt_generator_destroy(generator_); }
    I3PhotonToMCHitConverterForMultiPMTHIP(const I3PhotonToMCHitConverterForMultiPMTHIP &) = delete;
    I3PhotonToMCHitConverterForMultiPMTHIP &operator=(const I3PhotonToMCHitConverterForMultiPMTHIP &) = delete;

    // the module's parameters (defaults: :68, :73, :78)
    void SetInputPhotonSeriesMapName(const std::string &v) { inputPhotonSeriesMapName_ = v; }
    void SetOutputMultiOMMCHitMapName(const std::string &v) { outputMCHitSeriesMapName_ = v; }
    void SetMCTreeName(const std::string &v) { MCTreeName_ = v; }
    const std::string &GetInputPhotonSeriesMapName() const { return inputPhotonSeriesMapName_; }
    const std::string &GetOutputMultiOMMCHitMapName() const { return outputMCHitSeriesMapName_; }
    const std::string &GetMCTreeName() const { return MCTreeName_; }
    // in place of "RandomService"
    void SetSeed(uint64_t seed) { seed_ = seed; }

    // the geometry's I3OMTypeInfo and module map: functions (tables are copied), module types, their PMTs, the modules
    void SetGeometry(const std::vector<clsimhip_function> &functions, const std::vector<clsimhip_pmt_type> &types, const std::vector<clsimhip_pmt> &pmts,
                     const std::vector<clsimhip_pmt_module> &modules)
    {
        functions_ = functions;
        tables_.assign(functions.size(), std::vector<double>());
        for (size_t k = 0; k < functions.size(); ++k)
            if (functions[k].values && functions[k].n > 0) {
                tables_[k].assign(functions[k].values, functions[k].values + functions[k].n);
                functions_[k].values = tables_[k].data();
            }
        types_ = types; pmts_ = pmts; modules_ = modules;
    }

    void Configure()
    {
        clsimhip_pmt_generator *made = nullptr;
        if (clsimhip_pmt_generator_create(functions_.data(), functions_.size(), types_.data(), types_.size(), pmts_.data(), pmts_.size(), modules_.data(),
                                          modules_.size(), seed_, &made) != CLSIMHIP_OK)
            throw I3PhotonToMCHitConverterForMultiPMT_exception(clsimhip_pmt_generator_last_error(nullptr));
        clsimhip_pmt_generator_destroy(generator_);
        generator_ = made;
    }
    bool IsConfigured() const { return generator_ != nullptr; }
    clsimhip_pmt_generator *GetGenerator() const { return generator_; }    // for clsimhip_pmt_photon_hits_device on records in device memory

    // the module's DAQ() on the stored photons (the host twin)
    Result Convert(const std::vector<clsimhip_frame_photon> &photons, const std::vector<clsimhip_mcpe_series> &series) const
    {
        Result r;
        r.hits.resize(photons.size());
        r.series.resize(photons.size());
        size_t kept = 0, made = 0;
        uint64_t c[5] = {0, 0, 0, 0, 0};
        if (clsimhip_pmt_photon_hits_host(need(), photons.data(), photons.size(), series.data(), series.size(), r.hits.data(), r.series.data(), &kept, &made, c) !=
            CLSIMHIP_OK)
            throw I3PhotonToMCHitConverterForMultiPMT_exception(clsimhip_pmt_generator_last_error(nullptr));
        r.hits.resize(kept);
        r.series.resize(made);
        Check(c);
        r.offSurface = c[CLSIMHIP_PMT_PHOTON_HITS_OFF_SURFACE];
        return r;
    }

    // what the reference log_fatals on, from the stage's five counters (of the host twin, or downloaded behind the device stage)
    static void Check(const uint64_t counters[5])
    {
        const auto count = [&](int which) { return std::to_string(static_cast<unsigned long long>(counters[which])); };
        if (counters[CLSIMHIP_PMT_PHOTON_HITS_UNCOVERED] || counters[CLSIMHIP_PMT_PHOTON_HITS_SERIES_MISMATCH])
            throw I3PhotonToMCHitConverterForMultiPMT_exception("the series table does not describe the photons: " + count(CLSIMHIP_PMT_PHOTON_HITS_UNCOVERED) +
                                                                " records outside every entry, " + count(CLSIMHIP_PMT_PHOTON_HITS_SERIES_MISMATCH) +
                                                                " with other IDs than their entry");
        if (counters[CLSIMHIP_PMT_PHOTON_HITS_UNKNOWN_MODULE])
            throw I3PhotonToMCHitConverterForMultiPMT_exception("OM not found in the current geometry map! (" + count(CLSIMHIP_PMT_PHOTON_HITS_UNKNOWN_MODULE) +
                                                                " photons)");                                                                        // :283
        if (counters[CLSIMHIP_PMT_PHOTON_HITS_PROBABILITY_ABOVE_ONE])
            throw I3PhotonToMCHitConverterForMultiPMT_exception("measurement_prob > 1: cannot continue. your hit weights are too high. (" +
                                                                count(CLSIMHIP_PMT_PHOTON_HITS_PROBABILITY_ABOVE_ONE) + " photons)");                // :349
    }

private:
    clsimhip_pmt_generator *need() const
    {
        if (!generator_) throw I3PhotonToMCHitConverterForMultiPMT_exception("I3PhotonToMCHitConverterForMultiPMTHIP is not configured!");
        return generator_;
    }
    std::string inputPhotonSeriesMapName_ = "PropagatedPhotons", outputMCHitSeriesMapName_ = "MCHitSeriesMultiOMMap", MCTreeName_ = "I3MCTree";
    uint64_t seed_ = 0;
    std::vector<clsimhip_function> functions_;
    std::vector<std::vector<double> > tables_;
    std::vector<clsimhip_pmt_type> types_;
    std::vector<clsimhip_pmt> pmts_;
    std::vector<clsimhip_pmt_module> modules_;
    clsimhip_pmt_generator *generator_ = nullptr;
};
