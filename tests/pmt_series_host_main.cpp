// Stand-alone host program for the PMT series' host twin (clsim_amd/csrc/pmt_series.cpp on the generator of pmt_hits.cpp), built by
// tests/test_pmt_series.py with -fsanitize=address,undefined: no Python, no GPU, no HIP runtime -- the few HIP entry points the
// two files name are defined here and answer "no device".
//     pmt_series_host_main IN OUT
// IN:  eight uint64 {n_functions, n_types, n_pmts, n_modules, n_hits, n_particles, n_masked, have_table}; per function {kind, n} as
//      int64, {start, step, value} as doubles and n values; the types (clsimhip_pmt_type), PMTs (clsimhip_pmt), modules
//      (clsimhip_pmt_module), hits (clsimhip_pmt_hit), particle table (clsimhip_mcpe_particle) and mask (clsimhip_mcpe_mask) as they
//      lie in memory.
// OUT: the kept records (clsimhip_pmt_hit), then the series table (clsimhip_pmt_series).  Prints "kept N series S counters A B C".
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "pmt_series.h"

extern "C" {
hipError_t hipMalloc(void **, size_t) { return hipErrorNoDevice; }
hipError_t hipFree(void *) { return hipErrorNoDevice; }
hipError_t hipHostMalloc(void **, size_t, unsigned int) { return hipErrorNoDevice; }
hipError_t hipHostFree(void *) { return hipErrorNoDevice; }
hipError_t hipMemcpy(void *, const void *, size_t, hipMemcpyKind) { return hipErrorNoDevice; }
hipError_t hipMemcpyAsync(void *, const void *, size_t, hipMemcpyKind, hipStream_t) { return hipErrorNoDevice; }
hipError_t hipMemsetAsync(void *, int, size_t, hipStream_t) { return hipErrorNoDevice; }
hipError_t hipEventCreateWithFlags(hipEvent_t *, unsigned int) { return hipErrorNoDevice; }
hipError_t hipEventDestroy(hipEvent_t) { return hipErrorNoDevice; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipErrorNoDevice; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipErrorNoDevice; }
hipError_t hipGetDevice(int *) { return hipErrorNoDevice; }
hipError_t hipSetDevice(int) { return hipErrorNoDevice; }
hipError_t hipGetDeviceCount(int *count) { *count = 0; return hipErrorNoDevice; }
const char *hipGetErrorString(hipError_t) { return "no device"; }
}
namespace clsimhip {
hipError_t launch_pmt_hits_kernel(const PmtHitParams &, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_pmt_series(const PmtSeriesDeviceArgs &, hipStream_t) { return hipErrorNoDevice; }
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
    if (argc != 3) { std::fprintf(stderr, "usage: pmt_series_host_main IN OUT\n"); return 2; }
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
        const std::vector<clsimhip_pmt_hit> hits = read_array<clsimhip_pmt_hit>(in, head[4]);
        std::vector<clsimhip_mcpe_particle> particles = read_array<clsimhip_mcpe_particle>(in, head[5]);
        const std::vector<clsimhip_mcpe_mask> masked = read_array<clsimhip_mcpe_mask>(in, head[6]);
        const bool have_table = head[7] != 0;
        if (have_table && particles.empty()) particles.reserve(1);      // (an empty table is still a table: it gets an address)
        clsimhip::PmtHitGenerator generator(functions, types.data(), types.size(), pmts.data(), pmts.size(), modules.data(), modules.size(), 1);
        // exactly n entries each: a write past the kept records or the table is the sanitizer's to find
        std::vector<clsimhip_pmt_hit> out(hits.size());
        std::vector<clsimhip_pmt_series> series(hits.size());
        size_t kept = 0, made = 0;
        uint64_t counters[3] = {0, 0, 0};
        generator.series_host(hits.data(), hits.size(), have_table ? particles.data() : nullptr, particles.size(), masked.data(), masked.size(), out.data(),
                              series.data(), &kept, &made, counters);
        // no table and no mask, no counters, no counts: the optional outputs are optional
        generator.series_host(hits.data(), hits.size(), nullptr, 0, nullptr, 0, std::vector<clsimhip_pmt_hit>(hits.size()).data(),
                              std::vector<clsimhip_pmt_series>(hits.size()).data(), nullptr, nullptr, nullptr);
        // the device path without a device: an error, not a crash
        try {
            generator.series_device(0, hits.data(), hits.data(), 1, nullptr, 0, nullptr, 0, out.data(), series.data(), counters, out.data(), 1 << 20, nullptr);
            std::fprintf(stderr, "series_device succeeded without a device\n");
            return 1;
        } catch (const clsimhip::Error &e) {
            if (e.code != CLSIMHIP_ERR_DEVICE && e.code != CLSIMHIP_ERR_ARGUMENT) throw;
        }
        std::ofstream file(argv[2], std::ios::binary);
        file.write(reinterpret_cast<const char *>(out.data()), static_cast<std::streamsize>(kept * sizeof(clsimhip_pmt_hit)));
        file.write(reinterpret_cast<const char *>(series.data()), static_cast<std::streamsize>(made * sizeof(clsimhip_pmt_series)));
        if (!file) throw clsimhip::Error(CLSIMHIP_ERR_IO, "cannot write the output file");
        std::printf("kept %zu series %zu counters %llu %llu %llu\n", kept, made, (unsigned long long)counters[0], (unsigned long long)counters[1],
                    (unsigned long long)counters[2]);
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "pmt_series_host_main: %s\n", e.what());
        return 1;
    }
}
