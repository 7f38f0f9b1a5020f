// C++ adapter: the reference's older hit maker module, I3PhotonToMCPEConverter (private/clsim/dom/I3PhotonToMCPEConverter.cxx), on
// the C ABI's photon hits stage (include/clsimhip.h: "Photon hits") -- the second step of I3CLSimMakeHitsFromPhotons.
//
// The setters carry the module's parameter names (I3PhotonToMCPEConverter.cxx:61-135) with their defaults; Configure() builds the
// maker, as the module's Configure() checks its parameters (:137-193).  What the module reads from the frame -- geometry, calibration,
// detector status -- the caller hands over as the DOM table: one clsimhip_photon_hit_dom per DOM.  Convert() takes the stored
// photons of one or more frames as the frame photons stage delivers them and returns the time-sorted MCPEs with their series table;
// with MergeHits, also what the MCPE merging stage makes of them.  A condition the reference ends the run on throws here with its
// text.  Header-only; needs nothing but include/clsimhip.h and libclsimhip.so.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/clsimhip.h"

class I3PhotonToMCPEConverter_exception : public std::runtime_error {
public:
    explicit I3PhotonToMCPEConverter_exception(const std::string &msg) : std::runtime_error(msg) {}
};

class I3PhotonToMCPEConverterHIP {
public:
    struct Result {
        std::vector<clsimhip_mcpe> mcpes;                   // ascending in (input series, time key, identifier)
        std::vector<clsimhip_mcpe_series> series;           // one entry per input entry that kept a record
        uint64_t inactive = 0, offSurface = 0;              // records of ignored DOMs; positions that were only warned about
        // with MergeHits: the merged series, its table (as many entries as `series`), and the particle-ID map
        std::vector<clsimhip_mcpe_merged> merged;
        std::vector<clsimhip_mcpe_series> mergedSeries;
        std::vector<clsimhip_mcpe_parent> parents;
        std::vector<clsimhip_mcpe_parent_range> parentRanges;
    };

    I3PhotonToMCPEConverterHIP()
    {
        angular_.n = 0; angular_.coefficients = nullptr;
        angular_.range_min = -std::numeric_limits<double>::infinity(); angular_.range_max = std::numeric_limits<double>::infinity();
        angular_.underflow = 0.; angular_.overflow = 0.;
    }
    ~I3PhotonToMCPEConverterHIP() { clsimhip_photon_hit_maker_destroy(maker_); }
    I3PhotonToMCPEConverterHIP(const I3PhotonToMCPEConverterHIP &) = delete;
    I3PhotonToMCPEConverterHIP &operator=(const I3PhotonToMCPEConverterHIP &) = delete;

    // "WavelengthAcceptance": the module has one; here one per class of DOMs (clsimhip_photon_hit_dom::class_index), tables are copied
    void SetWavelengthAcceptance(const std::vector<clsimhip_function> &classes)
    {
        classes_ = classes;
        tables_.assign(classes.size(), std::vector<double>());
        for (size_t k = 0; k < classes.size(); ++k)
            if (classes[k].values && classes[k].n > 0) {
                tables_[k].assign(classes[k].values, classes[k].values + classes[k].n);
                classes_[k].values = tables_[k].data();
            }
    }
    // "AngularAcceptance"
    void SetAngularAcceptance(const clsimhip_polynomial &polynomial)
    {
        angular_ = polynomial;
        coefficients_.assign(polynomial.coefficients, polynomial.coefficients + (polynomial.n > 0 ? polynomial.n : 0));
        angular_.coefficients = coefficients_.data();
    }
    void SetDOMOversizeFactor(double v) { oversize_ = v; }
    void SetDOMPancakeFactor(double v) { pancake_ = v; }
    void SetDOMRadiusWithoutOversize(double v) { radius_ = v; }
    void SetDefaultRelativeDOMEfficiency(double v) { defaultEfficiency_ = v; }
    void SetReplaceRelativeDOMEfficiencyWithDefault(bool v) { replace_ = v; }
    void SetIgnoreDOMsWithoutDetectorStatusEntry(bool v) { ignoreInactive_ = v; }
    void SetOnlyWarnAboutInvalidPhotonPositions(bool v) { onlyWarn_ = v; }
    // "MergeHits"; the window is this library's parameter (the reference's lies in MCHitMerging, outside it)
    void SetMergeHits(bool v, double window = 0.) { mergeHits_ = v; mergeWindow_ = window; }
    // "RandomService": the draw is a hash of the record and this seed
    void SetRandomSeed(uint64_t seed) { seed_ = seed; }
    // geometry, calibration and detector status of the frame, per DOM
    void SetDOMs(const std::vector<clsimhip_photon_hit_dom> &doms) { doms_ = doms; }

    void Configure()
    {
        clsimhip_photon_hit_config config;
        config.dom_radius = radius_; config.oversize = oversize_; config.pancake = pancake_;
        config.default_relative_efficiency = defaultEfficiency_;
        config.replace_efficiency_with_default = replace_ ? 1 : 0;
        config.ignore_inactive = ignoreInactive_ ? 1 : 0;
        config.only_warn_off_surface = onlyWarn_ ? 1 : 0;
        config.reserved = 0;
        config.seed = seed_;
        if (classes_.empty()) throw I3PhotonToMCPEConverter_exception("The \"WavelengthAcceptance\" parameter must not be empty.");       // :175
        if (angular_.n <= 0) throw I3PhotonToMCPEConverter_exception("The \"AngularAcceptance\" parameter must not be empty.");           // :177
        if (mergeHits_ && !(mergeWindow_ >= 0. && std::isfinite(mergeWindow_))) throw I3PhotonToMCPEConverter_exception("the merging window must be finite and >= 0");
        clsimhip_photon_hit_maker *made = nullptr;
        if (clsimhip_photon_hit_maker_create(classes_.data(), classes_.size(), &angular_, doms_.data(), doms_.size(), &config, &made) != CLSIMHIP_OK)
            throw I3PhotonToMCPEConverter_exception(clsimhip_photon_hit_maker_last_error(nullptr));
        clsimhip_photon_hit_maker_destroy(maker_);
        maker_ = made;
    }
    bool IsConfigured() const { return maker_ != nullptr; }
    clsimhip_photon_hit_maker *GetMaker() const { return maker_; }         // for clsimhip_photon_hits_device on records in device memory

    double GetEfficiency(int32_t stringID, uint32_t omID) const
    {
        double out = 0.;
        if (clsimhip_photon_hit_maker_efficiency(need(), stringID, omID, &out) != CLSIMHIP_OK)
            throw I3PhotonToMCPEConverter_exception(clsimhip_photon_hit_maker_last_error(nullptr));
        return out;
    }

    // the module's DAQ() on the stored photons (the host twin)
    Result Convert(const std::vector<clsimhip_frame_photon> &photons, const std::vector<clsimhip_mcpe_series> &series) const
    {
        Result r;
        r.mcpes.resize(photons.size());
        r.series.resize(series.size());
        size_t kept = 0, made = 0;
        uint64_t c[7] = {0, 0, 0, 0, 0, 0, 0};
        if (clsimhip_photon_hits_host(need(), photons.data(), photons.size(), series.data(), series.size(), r.mcpes.data(), r.series.data(), &kept, &made, c) !=
            CLSIMHIP_OK)
            throw I3PhotonToMCPEConverter_exception(clsimhip_photon_hit_maker_last_error(nullptr));
        r.mcpes.resize(kept);
        r.series.resize(made);
        Check(c, onlyWarn_);
        r.inactive = c[CLSIMHIP_PHOTON_HITS_INACTIVE];
        r.offSurface = c[CLSIMHIP_PHOTON_HITS_OFF_SURFACE];
        if (mergeHits_) {                                   // :531-532
            r.merged.resize(kept); r.parents.resize(kept);
            r.mergedSeries.resize(made); r.parentRanges.resize(made);
            size_t n_merged = 0, n_parents = 0;
            if (clsimhip_mcpe_merge_host(r.mcpes.data(), kept, r.series.data(), made, mergeWindow_, r.merged.data(), r.mergedSeries.data(), r.parents.data(),
                                         r.parentRanges.data(), &n_merged, &n_parents) != CLSIMHIP_OK)
                throw I3PhotonToMCPEConverter_exception(clsimhip_last_error(nullptr));
            r.merged.resize(n_merged);
            r.parents.resize(n_parents);
        }
        return r;
    }

    // what the reference log_fatals on, from the stage's seven counters (of the host twin, or downloaded behind the device stage)
    static void Check(const uint64_t counters[7], bool onlyWarnAboutInvalidPhotonPositions)
    {
        const auto count = [&](int which) { return std::to_string(static_cast<unsigned long long>(counters[which])); };
        if (counters[CLSIMHIP_PHOTON_HITS_UNCOVERED] || counters[CLSIMHIP_PHOTON_HITS_SERIES_MISMATCH])
            throw I3PhotonToMCPEConverter_exception("the series table does not describe the photons: " + count(CLSIMHIP_PHOTON_HITS_UNCOVERED) + " records outside every entry, " +
                                                    count(CLSIMHIP_PHOTON_HITS_SERIES_MISMATCH) + " with other IDs than their entry");
        if (counters[CLSIMHIP_PHOTON_HITS_UNKNOWN_DOM])
            throw I3PhotonToMCPEConverter_exception("OM not found in the current geometry map! (" + count(CLSIMHIP_PHOTON_HITS_UNKNOWN_DOM) + " photons)");       // :297
        if (counters[CLSIMHIP_PHOTON_HITS_NEGATIVE_WEIGHT])
            throw I3PhotonToMCPEConverter_exception("Photon with negative weight found. (" + count(CLSIMHIP_PHOTON_HITS_NEGATIVE_WEIGHT) + " photons)");          // :398
        if (counters[CLSIMHIP_PHOTON_HITS_OFF_SURFACE] && !onlyWarnAboutInvalidPhotonPositions)
            throw I3PhotonToMCPEConverter_exception("distance not DOMOversizeFactor*DOMRadiusWithoutOversize (" + count(CLSIMHIP_PHOTON_HITS_OFF_SURFACE) + " photons)");  // :437
        if (counters[CLSIMHIP_PHOTON_HITS_PROBABILITY_ABOVE_ONE])
            throw I3PhotonToMCPEConverter_exception("hitProbability > 1: your hit weights are too high. cannot continue. (" + count(CLSIMHIP_PHOTON_HITS_PROBABILITY_ABOVE_ONE) +
                                                    " photons)");                                                                                            // :479-503
    }

private:
    clsimhip_photon_hit_maker *need() const
    {
        if (!maker_) throw I3PhotonToMCPEConverter_exception("I3PhotonToMCPEConverterHIP is not configured!");
        return maker_;
    }
    std::vector<clsimhip_function> classes_;
    std::vector<std::vector<double> > tables_;
    clsimhip_polynomial angular_;
    std::vector<double> coefficients_;
    std::vector<clsimhip_photon_hit_dom> doms_;
    // the module's defaults (:81-121)
    double oversize_ = 1., pancake_ = 1., radius_ = 0.16510;
    double defaultEfficiency_ = 1.;
    bool replace_ = false, ignoreInactive_ = false, onlyWarn_ = false, mergeHits_ = false;
    double mergeWindow_ = 0.;
    uint64_t seed_ = 0;
    clsimhip_photon_hit_maker *maker_ = nullptr;
};
