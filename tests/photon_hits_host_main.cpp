// Stand-alone host program for the photon hits' host twin (clsim_amd/csrc/photon_hits.cpp), built by tests/test_photon_hits.py with
// -fsanitize=address,undefined: no Python, no GPU, no HIP runtime -- the few HIP entry points the file names are defined here and
// answer "no device".
//     photon_hits_host_main IN OUT
// IN:  5 + n_classes uint64 {n_classes, n_coefficients, n_doms, n_records, n_series, then the number of values of every class}; a
//      class with 0 values is the constant 1; then per table class {start, step} and its values (double); the coefficients
//      (double); the configuration (clsimhip_photon_hit_config), the DOM table (clsimhip_photon_hit_dom), the records
//      (clsimhip_frame_photon) and their series table (clsimhip_mcpe_series) as they lie in memory.
// OUT: the kept records (clsimhip_mcpe), then the series table (clsimhip_mcpe_series).  Prints "kept N series S counters" and the seven.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>
#include <vector>

#include "photon_hits.h"

extern "C" {
hipError_t hipMalloc(void **, size_t) { return hipErrorNoDevice; }
hipError_t hipFree(void *) { return hipErrorNoDevice; }
hipError_t hipMemcpy(void *, const void *, size_t, hipMemcpyKind) { return hipErrorNoDevice; }
hipError_t hipGetDevice(int *) { return hipErrorNoDevice; }
hipError_t hipSetDevice(int) { return hipErrorNoDevice; }
hipError_t hipGetDeviceCount(int *count) { *count = 0; return hipErrorNoDevice; }
const char *hipGetErrorString(hipError_t) { return "no device"; }
}
namespace clsimhip {
hipError_t launch_photon_hits(const PhotonHitsDeviceArgs &, hipStream_t) { return hipErrorNoDevice; }
}

template <class T>
static std::vector<T> read_array(std::ifstream &in, size_t n)
{
    std::vector<T> v(n);
    if (n) in.read(reinterpret_cast<char *>(v.data()), static_cast<std::streamsize>(n * sizeof(T)));
    if (!in) throw clsimhip::Error(CLSIMHIP_ERR_IO, "the input file is too short");
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: photon_hits_host_main IN OUT\n"); return 2; }
    try {
        std::ifstream in(argv[1], std::ios::binary);
        const std::vector<uint64_t> head = read_array<uint64_t>(in, 5);
        if (head[0] > 8u) throw clsimhip::Error(CLSIMHIP_ERR_ARGUMENT, "more than 8 classes");
        const std::vector<uint64_t> sizes = read_array<uint64_t>(in, head[0]);
        std::vector<clsimhip::FunctionData> classes(head[0]);
        for (size_t k = 0; k < classes.size(); ++k) {
            if (sizes[k] == 0u) { classes[k].kind = CLSIMHIP_FUNCTION_CONSTANT; classes[k].value = 1.0; continue; }
            const std::vector<double> range = read_array<double>(in, 2);
            classes[k].kind = CLSIMHIP_FUNCTION_TABLE;
            classes[k].start = range[0]; classes[k].step = range[1];
            classes[k].values = read_array<double>(in, sizes[k]);
        }
        const std::vector<double> coefficients = read_array<double>(in, head[1]);
        const std::vector<clsimhip_photon_hit_config> config = read_array<clsimhip_photon_hit_config>(in, 1);
        const std::vector<clsimhip_photon_hit_dom> doms = read_array<clsimhip_photon_hit_dom>(in, head[2]);
        const std::vector<clsimhip_frame_photon> records = read_array<clsimhip_frame_photon>(in, head[3]);
        const std::vector<clsimhip_mcpe_series> series = read_array<clsimhip_mcpe_series>(in, head[4]);
        clsimhip_polynomial angular{};
        angular.n = static_cast<int32_t>(coefficients.size());
        angular.coefficients = coefficients.data();
        angular.range_min = -std::numeric_limits<double>::infinity();
        angular.range_max = std::numeric_limits<double>::infinity();
        clsimhip::PhotonHitMaker maker(classes, angular, doms.data(), doms.size(), config[0]);
        // exactly n entries each: a write past the kept records or the table is the sanitizer's to find
        std::vector<clsimhip_mcpe> out(records.size());
        std::vector<clsimhip_mcpe_series> out_series(series.size());
        size_t kept = 0, made = 0;
        uint64_t counters[7] = {0, 0, 0, 0, 0, 0, 0};
        maker.host(records.data(), records.size(), series.data(), series.size(), out.data(), out_series.data(), &kept, &made, counters);
        // no counters, no counts: the optional outputs are optional
        maker.host(records.data(), records.size(), series.data(), series.size(), std::vector<clsimhip_mcpe>(records.size()).data(),
                   std::vector<clsimhip_mcpe_series>(series.size()).data(), nullptr, nullptr, nullptr);
        for (const clsimhip_photon_hit_dom &d : doms) (void)maker.efficiency(d.string_id, d.om_id);
        // the device path without a device: an error, not a crash
        try {
            alignas(16) static uint8_t block[1 << 16];
            maker.device(0, block, block, block, 1, block, block, block, block, sizeof block, nullptr);
            std::fprintf(stderr, "device() succeeded without a device\n");
            return 1;
        } catch (const clsimhip::Error &e) {
            if (e.code != CLSIMHIP_ERR_DEVICE) throw;
        }
        std::ofstream file(argv[2], std::ios::binary);
        file.write(reinterpret_cast<const char *>(out.data()), static_cast<std::streamsize>(kept * sizeof(clsimhip_mcpe)));
        file.write(reinterpret_cast<const char *>(out_series.data()), static_cast<std::streamsize>(made * sizeof(clsimhip_mcpe_series)));
        if (!file) throw clsimhip::Error(CLSIMHIP_ERR_IO, "cannot write the output file");
        std::printf("kept %zu series %zu counters", kept, made);
        for (uint64_t c : counters) std::printf(" %llu", (unsigned long long)c);
        std::printf("\n");
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "photon_hits_host_main: %s\n", e.what());
        return 1;
    }
}
