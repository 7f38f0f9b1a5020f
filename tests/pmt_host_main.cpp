// Stand-alone host program for the multi-PMT hit generator's host twin (clsim_amd/csrc/pmt_hits.cpp), built by
// tests/test_pmt_hits.py with -fsanitize=address,undefined: no Python, no GPU, no HIP runtime -- the few HIP entry points the
// generator object names are defined here and answer "no device".
//     pmt_host_main IN OUT
// IN:  eight uint64 {n_functions, n_types, n_pmts, n_modules, n_records, seed, 0, 0}; per function {kind, n} as int64, {start, step,
//      value} as doubles and n values; the types (clsimhip_pmt_type), PMTs (clsimhip_pmt), modules (clsimhip_pmt_module) and photon
//      records (clsimhip_photon) as they lie in memory.
// OUT: the hits (clsimhip_pmt_hit) in input order.  Prints "hits N counters A B C".
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "pmt_hits.h"

extern "C" {
hipError_t hipMalloc(void **, size_t) { return hipErrorNoDevice; }
hipError_t hipFree(void *) { return hipErrorNoDevice; }
hipError_t hipMemcpy(void *, const void *, size_t, hipMemcpyKind) { return hipErrorNoDevice; }
hipError_t hipMemsetAsync(void *, int, size_t, hipStream_t) { return hipErrorNoDevice; }
hipError_t hipGetDevice(int *) { return hipErrorNoDevice; }
hipError_t hipSetDevice(int) { return hipErrorNoDevice; }
hipError_t hipGetDeviceCount(int *count) { *count = 0; return hipErrorNoDevice; }
const char *hipGetErrorString(hipError_t) { return "no device"; }
}
namespace clsimhip {
hipError_t launch_pmt_hits_kernel(const PmtHitParams &, hipStream_t) { return hipErrorNoDevice; }
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
    if (argc != 3) { std::fprintf(stderr, "usage: pmt_host_main IN OUT\n"); return 2; }
    try {
        std::ifstream in(argv[1], std::ios::binary);
        const std::vector<uint64_t> head = read_array<uint64_t>(in, 8);
        std::vector<clsimhip::FunctionData> functions(head[0]);
        for (clsimhip::FunctionData &f : functions) {
            const std::vector<int64_t> kn = read_array<int64_t>(in, 2);
            const std::vector<double> ssv = read_array<double>(in, 3);
            f.kind = static_cast<int>(kn[0]);
            f.start = ssv[0]; f.step = ssv[1]; f.value = ssv[2];
            f.values = read_array<double>(in, static_cast<size_t>(kn[1]));
        }
        const std::vector<clsimhip_pmt_type> types = read_array<clsimhip_pmt_type>(in, head[1]);
        const std::vector<clsimhip_pmt> pmts = read_array<clsimhip_pmt>(in, head[2]);
        const std::vector<clsimhip_pmt_module> modules = read_array<clsimhip_pmt_module>(in, head[3]);
        const std::vector<clsimhip_photon> photons = read_array<clsimhip_photon>(in, head[4]);
        clsimhip::PmtHitGenerator generator(functions, types.data(), types.size(), pmts.data(), pmts.size(), modules.data(), modules.size(), head[5]);
        // a capacity short of the result: the twin counts on and stores what fits; then the whole of it
        std::vector<clsimhip_pmt_hit> few(3);
        size_t made = 0;
        generator.convert_host(photons.data(), photons.size(), few.data(), few.size(), &made, nullptr);
        std::vector<clsimhip_pmt_hit> hits(made);
        uint64_t counters[3] = {0, 0, 0};
        size_t again = 0;
        generator.convert_host(photons.data(), photons.size(), hits.data(), hits.size(), &again, counters);
        if (again != made || (made >= 3 && std::memcmp(few.data(), hits.data(), 3 * sizeof(clsimhip_pmt_hit)) != 0)) {
            std::fprintf(stderr, "the second pass made %zu hits, the first %zu\n", again, made);
            return 1;
        }
        // the device path without a device: an error, not a crash
        try {
            generator.convert_device(0, photons.data(), photons.data(), 1, hits.data(), 1, counters, nullptr);
            std::fprintf(stderr, "convert_device succeeded without a device\n");
            return 1;
        } catch (const clsimhip::Error &e) {
            if (e.code != CLSIMHIP_ERR_DEVICE && e.code != CLSIMHIP_ERR_ARGUMENT) throw;
        }
        std::ofstream out(argv[2], std::ios::binary);
        out.write(reinterpret_cast<const char *>(hits.data()), static_cast<std::streamsize>(hits.size() * sizeof(clsimhip_pmt_hit)));
        if (!out) throw clsimhip::Error(CLSIMHIP_ERR_IO, "cannot write the output file");
        std::printf("hits %zu counters %llu %llu %llu\n", made, (unsigned long long)counters[0], (unsigned long long)counters[1], (unsigned long long)counters[2]);
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "pmt_host_main: %s\n", e.what());
        return 1;
    }
}
