// Stand-alone host program for the cable shadow's host twin (clsim_amd/csrc/cable_shadow.cpp), built by tests/test_cable_shadow.py
// with -fsanitize=address,undefined: no Python, no GPU, no HIP runtime -- the few HIP entry points the file names are defined here
// and answer "no device".
//     cable_shadow_host_main IN OUT
// IN:  two uint64 {n_cylinders, n_photons} and the distance (double); the cylinders' tops (3 doubles each), bottoms (3 doubles each)
//      and radii; the photons (clsimhip_photon) as they lie in memory.
// OUT: the flags (one byte per photon), then the lit records (clsimhip_photon).  Prints "lit N tested T shadowed S".
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "cable_shadow.h"

extern "C" {
hipError_t hipMalloc(void **, size_t) { return hipErrorNoDevice; }
hipError_t hipFree(void *) { return hipErrorNoDevice; }
hipError_t hipHostMalloc(void **, size_t, unsigned int) { return hipErrorNoDevice; }
hipError_t hipHostFree(void *) { return hipErrorNoDevice; }
hipError_t hipMemcpy(void *, const void *, size_t, hipMemcpyKind) { return hipErrorNoDevice; }
hipError_t hipEventCreateWithFlags(hipEvent_t *, unsigned int) { return hipErrorNoDevice; }
hipError_t hipEventDestroy(hipEvent_t) { return hipErrorNoDevice; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipErrorNoDevice; }
hipError_t hipGetDevice(int *) { return hipErrorNoDevice; }
hipError_t hipSetDevice(int) { return hipErrorNoDevice; }
hipError_t hipGetDeviceCount(int *count) { *count = 0; return hipErrorNoDevice; }
const char *hipGetErrorString(hipError_t) { return "no device"; }
}
namespace clsimhip {
hipError_t launch_cable_shadow(const CableShadowDeviceArgs &, hipStream_t) { return hipErrorNoDevice; }
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
    if (argc != 3) { std::fprintf(stderr, "usage: cable_shadow_host_main IN OUT\n"); return 2; }
    try {
        std::ifstream in(argv[1], std::ios::binary);
        const std::vector<uint64_t> head = read_array<uint64_t>(in, 2);
        const double distance = read_array<double>(in, 1)[0];
        const std::vector<double> top = read_array<double>(in, 3 * head[0]), bottom = read_array<double>(in, 3 * head[0]);
        const std::vector<double> radius = read_array<double>(in, head[0]);
        const std::vector<clsimhip_photon> photons = read_array<clsimhip_photon>(in, head[1]);
        clsimhip::CableShadow shadow(head[0], top.data(), bottom.data(), radius.data(), distance);
        // exactly n entries each: a write past the flags or the lit records is the sanitizer's to find
        std::vector<uint8_t> flags(photons.size());
        std::vector<clsimhip_photon> lit(photons.size());
        size_t kept = 0;
        uint64_t counts[2] = {0, 0};
        shadow.host(photons.data(), photons.size(), flags.data(), lit.data(), &kept, counts);
        // no count and no counts: the optional outputs are optional
        shadow.host(photons.data(), photons.size(), std::vector<uint8_t>(photons.size()).data(), std::vector<clsimhip_photon>(photons.size()).data(), nullptr, nullptr);
        // a set the constructor refuses, and the device path without a device: errors, not crashes
        try {
            clsimhip::CableShadow none(0, top.data(), bottom.data(), radius.data(), distance);
            std::fprintf(stderr, "an empty cylinder set was accepted\n");
            return 1;
        } catch (const clsimhip::Error &e) {
            if (e.code != CLSIMHIP_ERR_ARGUMENT) throw;
        }
        try {
            shadow.device(0, lit.data(), lit.data(), 1, flags.data(), lit.data(), counts, lit.data(), 1 << 20, nullptr);
            std::fprintf(stderr, "device() succeeded without a device\n");
            return 1;
        } catch (const clsimhip::Error &e) {
            if (e.code != CLSIMHIP_ERR_DEVICE && e.code != CLSIMHIP_ERR_ARGUMENT) throw;
        }
        std::ofstream file(argv[2], std::ios::binary);
        file.write(reinterpret_cast<const char *>(flags.data()), static_cast<std::streamsize>(flags.size()));
        file.write(reinterpret_cast<const char *>(lit.data()), static_cast<std::streamsize>(kept * sizeof(clsimhip_photon)));
        if (!file) throw clsimhip::Error(CLSIMHIP_ERR_IO, "cannot write the output file");
        std::printf("lit %zu tested %llu shadowed %llu\n", kept, (unsigned long long)counts[0], (unsigned long long)counts[1]);
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "cable_shadow_host_main: %s\n", e.what());
        return 1;
    }
}
