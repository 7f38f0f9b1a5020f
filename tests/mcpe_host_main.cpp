// Stand-alone host program for the MCPE generator's host twin (clsim_amd/csrc/mcpe.cpp), built by tests/test_hit_records.py with
// -fsanitize=address,undefined: no Python, no GPU, no HIP runtime -- the few HIP entry points the generator object names are
// defined here and answer "no device".
//     mcpe_host_main IN OUT
// IN:  eight uint64 {n_classes, n_coefficients, n_doms, n_records, seed, 0, 0, 0}; three doubles {dom_radius, oversize, pancake};
//      per class {kind, n} as int64, {start, step, value} as doubles and n values; the polynomial's coefficients and {range_min,
//      range_max, underflow, overflow} as doubles; string IDs (int32), OM IDs (uint32) and class indices (int32) of the DOMs; the
//      photon records (clsimhip_photon) as they lie in memory.
// OUT: the MCPEs (clsimhip_mcpe) in input order.  Prints "mcpes N counters A B C D".
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "mcpe.h"

extern "C" {
hipError_t hipMalloc(void **, size_t) { return hipErrorNoDevice; }
hipError_t hipFree(void *) { return hipErrorNoDevice; }
hipError_t hipHostFree(void *) { return hipErrorNoDevice; }
hipError_t hipEventDestroy(hipEvent_t) { return hipErrorNoDevice; }
hipError_t hipMemcpy(void *, const void *, size_t, hipMemcpyKind) { return hipErrorNoDevice; }
hipError_t hipMemsetAsync(void *, int, size_t, hipStream_t) { return hipErrorNoDevice; }
hipError_t hipGetDevice(int *) { return hipErrorNoDevice; }
hipError_t hipSetDevice(int) { return hipErrorNoDevice; }
hipError_t hipGetDeviceCount(int *count) { *count = 0; return hipErrorNoDevice; }
const char *hipGetErrorString(hipError_t) { return "no device"; }
}
namespace clsimhip {
hipError_t launch_mcpe_kernel(const McpeParams &, hipStream_t) { return hipErrorNoDevice; }
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
    if (argc != 3) { std::fprintf(stderr, "usage: mcpe_host_main IN OUT\n"); return 2; }
    try {
        std::ifstream in(argv[1], std::ios::binary);
        const std::vector<uint64_t> head = read_array<uint64_t>(in, 8);
        const std::vector<double> sphere = read_array<double>(in, 3);
        std::vector<clsimhip::FunctionData> classes(head[0]);
        for (clsimhip::FunctionData &f : classes) {
            const std::vector<int64_t> kn = read_array<int64_t>(in, 2);
            const std::vector<double> ssv = read_array<double>(in, 3);
            f.kind = static_cast<int>(kn[0]);
            f.start = ssv[0]; f.step = ssv[1]; f.value = ssv[2];
            f.values = read_array<double>(in, static_cast<size_t>(kn[1]));
        }
        const std::vector<double> coefficients = read_array<double>(in, head[1]);
        const std::vector<double> range = read_array<double>(in, 4);
        const std::vector<int32_t> string_ids = read_array<int32_t>(in, head[2]);
        const std::vector<uint32_t> om_ids = read_array<uint32_t>(in, head[2]);
        const std::vector<int32_t> class_index = read_array<int32_t>(in, head[2]);
        const std::vector<clsimhip_photon> photons = read_array<clsimhip_photon>(in, head[3]);
        clsimhip_polynomial angular;
        angular.n = static_cast<int32_t>(coefficients.size());
        angular.coefficients = coefficients.data();
        angular.range_min = range[0]; angular.range_max = range[1]; angular.underflow = range[2]; angular.overflow = range[3];
        clsimhip::McpeGenerator generator(classes, string_ids.size(), string_ids.data(), om_ids.data(), class_index.data(), angular, sphere[0], sphere[1],
                                          sphere[2], head[4]);
        // a capacity short of the result: the twin counts on and stores what fits; then the whole of it
        std::vector<clsimhip_mcpe> few(3);
        size_t made = 0;
        generator.convert_host(photons.data(), photons.size(), few.data(), few.size(), &made, nullptr);
        std::vector<clsimhip_mcpe> mcpes(made);
        uint64_t counters[4] = {0, 0, 0, 0};
        size_t again = 0;
        generator.convert_host(photons.data(), photons.size(), mcpes.data(), mcpes.size(), &again, counters);
        if (again != made || (made >= 3 && std::memcmp(few.data(), mcpes.data(), 3 * sizeof(clsimhip_mcpe)) != 0)) {
            std::fprintf(stderr, "the second pass made %zu MCPEs, the first %zu\n", again, made);
            return 1;
        }
        // the device path without a device: an error, not a crash
        try {
            generator.convert_device(0, photons.data(), photons.data(), 1, mcpes.data(), 1, counters, nullptr);
            std::fprintf(stderr, "convert_device succeeded without a device\n");
            return 1;
        } catch (const clsimhip::Error &e) {
            if (e.code != CLSIMHIP_ERR_DEVICE && e.code != CLSIMHIP_ERR_ARGUMENT) throw;
        }
        std::ofstream out(argv[2], std::ios::binary);
        out.write(reinterpret_cast<const char *>(mcpes.data()), static_cast<std::streamsize>(mcpes.size() * sizeof(clsimhip_mcpe)));
        if (!out) throw clsimhip::Error(CLSIMHIP_ERR_IO, "cannot write the output file");
        std::printf("mcpes %zu counters %llu %llu %llu %llu\n", made, (unsigned long long)counters[0], (unsigned long long)counters[1],
                    (unsigned long long)counters[2], (unsigned long long)counters[3]);
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "mcpe_host_main: %s\n", e.what());
        return 1;
    }
}
