// PMT photon hits through the C++ adapter (I3PhotonToMCHitConverterForMultiPMTHIP.h), host only.
//     pmt_photon_hits_adapter_test IN OUT
// IN (written by tests/test_pmt_photon_hits_adapter.py, the format of tests/pmt_photon_hits_host_main.cpp): eight uint64 {n_functions,
// n_types, n_pmts, n_modules, n_records, n_series, seed, 0}; per function {kind, n} as int64, {start, step, value} as doubles and n
// values; the types, PMTs, modules, frame photons and their series table as they lie in memory.
// The configuration goes through the module's parameter names.  OUT: hits, then series.  A condition the reference ends on is printed
// as "refused: <text>", exit code 3.
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "I3PhotonToMCHitConverterForMultiPMTHIP.h"

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
    if (argc != 3) { std::fprintf(stderr, "usage: pmt_photon_hits_adapter_test IN OUT\n"); return 2; }
    try {
        std::ifstream in(argv[1], std::ios::binary);
        const std::vector<uint64_t> head = read_array<uint64_t>(in, 8);
        std::vector<std::vector<double> > values(head[0]);
        std::vector<clsimhip_function> functions(head[0]);
        for (size_t k = 0; k < functions.size(); ++k) {
            const std::vector<int64_t> kn = read_array<int64_t>(in, 2);
            const std::vector<double> ssv = read_array<double>(in, 3);
            values[k] = read_array<double>(in, static_cast<size_t>(kn[1]));
            clsimhip_function &f = functions[k];
            f = clsimhip_function();
            f.kind = static_cast<int32_t>(kn[0]); f.n = static_cast<int32_t>(kn[1]);
            f.start = ssv[0]; f.step = ssv[1]; f.value = ssv[2];
            f.values = values[k].empty() ? nullptr : values[k].data();
        }
        const std::vector<clsimhip_pmt_type> types = read_array<clsimhip_pmt_type>(in, head[1]);
        const std::vector<clsimhip_pmt> pmts = read_array<clsimhip_pmt>(in, head[2]);
        const std::vector<clsimhip_pmt_module> modules = read_array<clsimhip_pmt_module>(in, head[3]);
        const std::vector<clsimhip_frame_photon> records = read_array<clsimhip_frame_photon>(in, head[4]);
        const std::vector<clsimhip_mcpe_series> series = read_array<clsimhip_mcpe_series>(in, head[5]);

        I3PhotonToMCHitConverterForMultiPMTHIP conv;
        if (conv.GetInputPhotonSeriesMapName() != "PropagatedPhotons" || conv.GetOutputMultiOMMCHitMapName() != "MCHitSeriesMultiOMMap" ||
            conv.GetMCTreeName() != "I3MCTree") {
            std::printf("FAILED: the parameters' defaults are not the module's\n");
            return 1;
        }
        bool refused = false;
        try { conv.Convert(records, series); } catch (const I3PhotonToMCHitConverterForMultiPMT_exception &) { refused = true; }
        if (!refused) { std::printf("FAILED: Convert() before Configure() was not refused\n"); return 1; }
        try { conv.Configure(); refused = false; } catch (const I3PhotonToMCHitConverterForMultiPMT_exception &) { refused = true; }
        if (!refused) { std::printf("FAILED: Configure() without a geometry was not refused\n"); return 1; }
        conv.SetInputPhotonSeriesMapName("PropagatedPhotonsWithShadow");
        conv.SetOutputMultiOMMCHitMapName("MCHitSeriesMultiOMMap");
        conv.SetMCTreeName("I3MCTree");
        conv.SetSeed(head[6]);
        conv.SetGeometry(functions, types, pmts, modules);
        try {
            conv.Configure();
            std::printf("configured with %zu modules, reading %s\n", modules.size(), conv.GetInputPhotonSeriesMapName().c_str());
            const I3PhotonToMCHitConverterForMultiPMTHIP::Result r = conv.Convert(records, series);
            std::ofstream out(argv[2], std::ios::binary);
            write_array(out, r.hits); write_array(out, r.series);
            if (!out) throw std::runtime_error("cannot write the output file");
            std::printf("hits %zu series %zu off_surface %llu\n", r.hits.size(), r.series.size(), (unsigned long long)r.offSurface);
        } catch (const I3PhotonToMCHitConverterForMultiPMT_exception &e) {
            std::printf("refused: %s\n", e.what());
            return 3;
        }
        std::printf("pmt photon hits adapter ok\n");
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "pmt_photon_hits_adapter_test: %s\n", e.what());
        return 1;
    }
}
