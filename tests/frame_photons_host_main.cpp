// Stand-alone host program for the frame photons' host twin (clsim_amd/csrc/frame_photons.cpp), built by tests/test_frame_photons.py
// with -fsanitize=address,undefined: no Python, no GPU, no HIP runtime -- the few HIP entry points the file names are defined here
// and answer "no device".
//     frame_photons_host_main IN OUT
// IN:  five uint64 {n_doms, n_photons, n_particles, n_masked, have_table}; the DOMs' string IDs (int32) and OM IDs (uint32); the photons
//      (clsimhip_photon), particle table (clsimhip_mcpe_particle) and mask (clsimhip_mcpe_mask) as they lie in memory.
// OUT: the kept records (clsimhip_frame_photon), then the series table (clsimhip_mcpe_series).  Prints "kept N series S counters A B C D".
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "frame_photons.h"

extern "C" {
hipError_t hipMalloc(void **, size_t) { return hipErrorNoDevice; }
hipError_t hipFree(void *) { return hipErrorNoDevice; }
hipError_t hipHostMalloc(void **, size_t, unsigned int) { return hipErrorNoDevice; }
hipError_t hipHostFree(void *) { return hipErrorNoDevice; }
hipError_t hipMemcpy(void *, const void *, size_t, hipMemcpyKind) { return hipErrorNoDevice; }
hipError_t hipMemcpyAsync(void *, const void *, size_t, hipMemcpyKind, hipStream_t) { return hipErrorNoDevice; }
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
hipError_t launch_frame_photons(const FramePhotonsDeviceArgs &, hipStream_t) { return hipErrorNoDevice; }
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
    if (argc != 3) { std::fprintf(stderr, "usage: frame_photons_host_main IN OUT\n"); return 2; }
    try {
        std::ifstream in(argv[1], std::ios::binary);
        const std::vector<uint64_t> head = read_array<uint64_t>(in, 5);
        const std::vector<int32_t> strings = read_array<int32_t>(in, head[0]);
        const std::vector<uint32_t> oms = read_array<uint32_t>(in, head[0]);
        const std::vector<clsimhip_photon> photons = read_array<clsimhip_photon>(in, head[1]);
        std::vector<clsimhip_mcpe_particle> particles = read_array<clsimhip_mcpe_particle>(in, head[2]);
        const std::vector<clsimhip_mcpe_mask> masked = read_array<clsimhip_mcpe_mask>(in, head[3]);
        const bool have_table = head[4] != 0;
        if (have_table && particles.empty()) particles.reserve(1);      // (an empty table is still a table: it gets an address)
        clsimhip::FramePhotonDoms doms(strings.data(), oms.data(), strings.size());
        // exactly n entries each: a write past the kept records or the table is the sanitizer's to find
        std::vector<clsimhip_frame_photon> out(photons.size());
        std::vector<clsimhip_mcpe_series> series(photons.size());
        size_t kept = 0, made = 0;
        uint64_t counters[4] = {0, 0, 0, 0};
        doms.host(photons.data(), photons.size(), have_table ? particles.data() : nullptr, particles.size(), masked.data(), masked.size(), out.data(), series.data(),
                  &kept, &made, counters);
        // no table and no mask, no counters, no counts: the optional outputs are optional
        doms.host(photons.data(), photons.size(), nullptr, 0, nullptr, 0, std::vector<clsimhip_frame_photon>(photons.size()).data(),
                  std::vector<clsimhip_mcpe_series>(photons.size()).data(), nullptr, nullptr, nullptr);
        // the device path without a device: an error, not a crash
        try {
            doms.device(0, out.data(), out.data(), 1, nullptr, 0, nullptr, 0, out.data(), series.data(), counters, out.data(), 1 << 20, nullptr);
            std::fprintf(stderr, "device() succeeded without a device\n");
            return 1;
        } catch (const clsimhip::Error &e) {
            if (e.code != CLSIMHIP_ERR_DEVICE && e.code != CLSIMHIP_ERR_ARGUMENT) throw;
        }
        std::ofstream file(argv[2], std::ios::binary);
        file.write(reinterpret_cast<const char *>(out.data()), static_cast<std::streamsize>(kept * sizeof(clsimhip_frame_photon)));
        file.write(reinterpret_cast<const char *>(series.data()), static_cast<std::streamsize>(made * sizeof(clsimhip_mcpe_series)));
        if (!file) throw clsimhip::Error(CLSIMHIP_ERR_IO, "cannot write the output file");
        std::printf("kept %zu series %zu counters %llu %llu %llu %llu\n", kept, made, (unsigned long long)counters[0], (unsigned long long)counters[1],
                    (unsigned long long)counters[2], (unsigned long long)counters[3]);
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "frame_photons_host_main: %s\n", e.what());
        return 1;
    }
}
