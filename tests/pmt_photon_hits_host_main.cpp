// Stand-alone host program for the PMT photon hits' host twin (clsim_amd/csrc/pmt_photon_hits.cpp on the generator of pmt_hits.cpp),
// built by tests/test_pmt_photon_hits.py with -fsanitize=address,undefined: no Python, no GPU, no HIP runtime -- the few HIP entry
// points the two files name are defined here and answer "no device".
//     pmt_photon_hits_host_main IN OUT
// IN:  eight uint64 {n_functions, n_types, n_pmts, n_modules, n_records, n_series, seed, 0}; per function {kind, n} as int64, {start,
//      step, value} as doubles and n values; the types (clsimhip_pmt_type), PMTs (clsimhip_pmt), modules (clsimhip_pmt_module), frame
//      photons (clsimhip_frame_photon) and their series table (clsimhip_mcpe_series) as they lie in memory.
// OUT: the hits (clsimhip_pmt_hit), then the series table (clsimhip_pmt_series).  Prints "kept N series S counters A B C D E".
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "pmt_photon_hits.h"

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
hipError_t launch_pmt_photon_hits(const PmtPhotonHitsDeviceArgs &, hipStream_t) { return hipErrorNoDevice; }
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
    if (argc != 3) { std::fprintf(stderr, "usage: pmt_photon_hits_host_main IN OUT\n"); return 2; }
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
        const std::vector<clsimhip_frame_photon> records = read_array<clsimhip_frame_photon>(in, head[4]);
        const std::vector<clsimhip_mcpe_series> table = read_array<clsimhip_mcpe_series>(in, head[5]);
        clsimhip::PmtHitGenerator generator(functions, types.data(), types.size(), pmts.data(), pmts.size(), modules.data(), modules.size(), head[6]);
        // exactly n entries each: a write past the hits or the table is the sanitizer's to find
        std::vector<clsimhip_pmt_hit> out(records.size());
        std::vector<clsimhip_pmt_series> series(records.size());
        size_t kept = 0, made = 0;
        uint64_t counters[5] = {0, 0, 0, 0, 0};
        generator.photon_hits_host(records.data(), records.size(), table.data(), table.size(), out.data(), series.data(), &kept, &made, counters);
        // no counters, no counts: the optional outputs are optional
        generator.photon_hits_host(records.data(), records.size(), table.data(), table.size(), std::vector<clsimhip_pmt_hit>(records.size()).data(),
                                   std::vector<clsimhip_pmt_series>(records.size()).data(), nullptr, nullptr, nullptr);
        // no table at all: every record is UNCOVERED
        {
            uint64_t none[5] = {0, 0, 0, 0, 0};
            size_t k = 1, m = 1;
            generator.photon_hits_host(records.data(), records.size(), nullptr, 0, out.size() ? std::vector<clsimhip_pmt_hit>(records.size()).data() : nullptr,
                                       out.size() ? std::vector<clsimhip_pmt_series>(records.size()).data() : nullptr, &k, &m, none);
            if (k != 0 || m != 0 || none[0] != records.size()) throw clsimhip::Error(CLSIMHIP_ERR_STATE, "records without a table were not all UNCOVERED");
        }
        // more series than a key's group holds: refused by the argument alone
        try {
            generator.photon_hits_host(records.data(), 0, table.data(), (size_t{1} << 26) + 1u, nullptr, nullptr, nullptr, nullptr, nullptr);
            std::fprintf(stderr, "2^26 + 1 series were not refused\n");
            return 1;
        } catch (const clsimhip::Error &e) {
            if (e.code != CLSIMHIP_ERR_ARGUMENT) throw;
        }
        // the device path without a device: an error, not a crash
        try {
            alignas(16) static unsigned char scratch[1 << 20];
            generator.photon_hits_device(0, scratch, scratch, scratch, 1, scratch, scratch, scratch, scratch, sizeof scratch, nullptr);
            std::fprintf(stderr, "photon_hits_device succeeded without a device\n");
            return 1;
        } catch (const clsimhip::Error &e) {
            if (e.code != CLSIMHIP_ERR_DEVICE) throw;
        }
        std::ofstream file(argv[2], std::ios::binary);
        file.write(reinterpret_cast<const char *>(out.data()), static_cast<std::streamsize>(kept * sizeof(clsimhip_pmt_hit)));
        file.write(reinterpret_cast<const char *>(series.data()), static_cast<std::streamsize>(made * sizeof(clsimhip_pmt_series)));
        if (!file) throw clsimhip::Error(CLSIMHIP_ERR_IO, "cannot write the output file");
        std::printf("kept %zu series %zu counters %llu %llu %llu %llu %llu\n", kept, made, (unsigned long long)counters[0], (unsigned long long)counters[1],
                    (unsigned long long)counters[2], (unsigned long long)counters[3], (unsigned long long)counters[4]);
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "pmt_photon_hits_host_main: %s\n", e.what());
        return 1;
    }
}
