// Photon hits through the C++ adapter (I3PhotonToMCPEConverterHIP.h), host only.
//     photon_hits_adapter_test IN OUT WINDOW
// IN (written by tests/test_photon_hits_adapter.py, the format of tests/photon_hits_host_main.cpp): 5 + n_classes uint64 {n_classes,
// n_coefficients, n_doms, n_records, n_series, then the number of values of every class; 0: the constant 1}; per table class {start,
// step} and its values; the coefficients; the configuration (clsimhip_photon_hit_config); the DOM table; the records
// (clsimhip_frame_photon) and their series table.  WINDOW >= 0: MergeHits with that window; negative: no merging.
// The configuration goes through the module's parameter names.  OUT: mcpes, series, merged, merged series, parents, parent ranges.
// A condition the reference ends on is printed as "refused: <text>", exit code 3.
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "I3PhotonToMCPEConverterHIP.h"

template <class T>
static std::vector<T> read_array(std::ifstream &in, size_t n)
{
    std::vector<T> v(n);
    if (n) in.read(reinterpret_cast<char *>(v.data()), static_cast<std::streamsize>(n * sizeof(T)));
    if (!in) throw std::runtime_error("the input file is too short");
    return v;
}

template <class T>
static void write_array(std::ofstream &out, const std::vector<T> &v)
{
    if (!v.empty()) out.write(reinterpret_cast<const char *>(v.data()), static_cast<std::streamsize>(v.size() * sizeof(T)));
}

int main(int argc, char **argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: photon_hits_adapter_test IN OUT WINDOW\n"); return 2; }
    try {
        std::ifstream in(argv[1], std::ios::binary);
        const std::vector<uint64_t> head = read_array<uint64_t>(in, 5);
        const std::vector<uint64_t> sizes = read_array<uint64_t>(in, head[0]);
        std::vector<std::vector<double> > values(head[0]);
        std::vector<clsimhip_function> classes(head[0]);
        for (size_t k = 0; k < classes.size(); ++k) {
            clsimhip_function &f = classes[k];
            f = clsimhip_function();
            if (sizes[k] == 0u) { f.kind = CLSIMHIP_FUNCTION_CONSTANT; f.value = 1.0; continue; }
            const std::vector<double> range = read_array<double>(in, 2);
            values[k] = read_array<double>(in, sizes[k]);
            f.kind = CLSIMHIP_FUNCTION_TABLE; f.n = static_cast<int32_t>(sizes[k]);
            f.start = range[0]; f.step = range[1]; f.values = values[k].data();
        }
        const std::vector<double> coefficients = read_array<double>(in, head[1]);
        const clsimhip_photon_hit_config config = read_array<clsimhip_photon_hit_config>(in, 1)[0];
        const std::vector<clsimhip_photon_hit_dom> doms = read_array<clsimhip_photon_hit_dom>(in, head[2]);
        const std::vector<clsimhip_frame_photon> records = read_array<clsimhip_frame_photon>(in, head[3]);
        const std::vector<clsimhip_mcpe_series> series = read_array<clsimhip_mcpe_series>(in, head[4]);
        const double window = std::atof(argv[3]);

        I3PhotonToMCPEConverterHIP conv;
        bool refused = false;
        try { conv.Convert(records, series); } catch (const I3PhotonToMCPEConverter_exception &) { refused = true; }
        if (!refused) { std::printf("FAILED: Convert() before Configure() was not refused\n"); return 1; }
        try { conv.Configure(); refused = false; } catch (const I3PhotonToMCPEConverter_exception &) { refused = true; }
        if (!refused) { std::printf("FAILED: Configure() without a wavelength acceptance was not refused\n"); return 1; }
        clsimhip_polynomial angular = clsimhip_polynomial();
        angular.n = static_cast<int32_t>(coefficients.size());
        angular.coefficients = coefficients.data();
        angular.range_min = -std::numeric_limits<double>::infinity();
        angular.range_max = std::numeric_limits<double>::infinity();
        conv.SetWavelengthAcceptance(classes);
        conv.SetAngularAcceptance(angular);
        conv.SetDOMOversizeFactor(config.oversize);
        conv.SetDOMPancakeFactor(config.pancake);
        conv.SetDOMRadiusWithoutOversize(config.dom_radius);
        conv.SetDefaultRelativeDOMEfficiency(config.default_relative_efficiency);
        conv.SetReplaceRelativeDOMEfficiencyWithDefault(config.replace_efficiency_with_default != 0);
        conv.SetIgnoreDOMsWithoutDetectorStatusEntry(config.ignore_inactive != 0);
        conv.SetOnlyWarnAboutInvalidPhotonPositions(config.only_warn_off_surface != 0);
        conv.SetMergeHits(window >= 0., window >= 0. ? window : 0.);
        conv.SetRandomSeed(config.seed);
        conv.SetDOMs(doms);
        try {
            conv.Configure();
            std::printf("configured with %zu DOMs\n", doms.size());
            if (!doms.empty()) std::printf("efficiency of the first DOM %.17g\n", conv.GetEfficiency(doms[0].string_id, doms[0].om_id));
            const I3PhotonToMCPEConverterHIP::Result r = conv.Convert(records, series);
            std::ofstream out(argv[2], std::ios::binary);
            write_array(out, r.mcpes); write_array(out, r.series); write_array(out, r.merged); write_array(out, r.mergedSeries);
            write_array(out, r.parents); write_array(out, r.parentRanges);
            if (!out) throw std::runtime_error("cannot write the output file");
            std::printf("mcpes %zu series %zu merged %zu merged_series %zu parents %zu ranges %zu inactive %llu off_surface %llu\n", r.mcpes.size(), r.series.size(),
                        r.merged.size(), r.mergedSeries.size(), r.parents.size(), r.parentRanges.size(), (unsigned long long)r.inactive,
                        (unsigned long long)r.offSurface);
        } catch (const I3PhotonToMCPEConverter_exception &e) {
            std::printf("refused: %s\n", e.what());
            return 3;
        }
        std::printf("photon hits adapter ok\n");
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "photon_hits_adapter_test: %s\n", e.what());
        return 1;
    }
}
