// Stand-alone host program for the event statistics' host twin (clsim_amd/csrc/event_stats.cpp), built by tests/test_event_statistics.py
// with -fsanitize=address,undefined: no Python, no GPU, no HIP runtime -- the few HIP entry points the file names are defined here
// and answer "no device".
//     event_statistics_host_main IN OUT
// IN:  five uint64 {n_steps, n_photons, n_particles, n_masked, have_table}; the steps (clsimhip_step), the photons (clsimhip_photon),
//      the particle table (clsimhip_mcpe_particle) and the mask (clsimhip_mcpe_mask) as they lie in memory.
// OUT: the records (clsimhip_event_statistics), three uint64 counters, then one record: all records added up with
//      clsimhip_event_statistics_add's implementation, and two doubles: its sums through clsimhip_event_statistics_weight's.
//      Prints "records N".
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "event_stats.h"

extern "C" {
hipError_t hipMalloc(void **, size_t) { return hipErrorNoDevice; }
hipError_t hipFree(void *) { return hipErrorNoDevice; }
hipError_t hipHostMalloc(void **, size_t, unsigned int) { return hipErrorNoDevice; }
hipError_t hipHostFree(void *) { return hipErrorNoDevice; }
hipError_t hipMemcpy(void *, const void *, size_t, hipMemcpyKind) { return hipErrorNoDevice; }
hipError_t hipMemcpyAsync(void *, const void *, size_t, hipMemcpyKind, hipStream_t) { return hipErrorNoDevice; }
hipError_t hipEventCreateWithFlags(hipEvent_t *, unsigned int) { return hipErrorNoDevice; }
hipError_t hipEventDestroy(hipEvent_t) { return hipErrorNoDevice; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipErrorNoDevice; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipErrorNoDevice; }
hipError_t hipGetDevice(int *) { return hipErrorNoDevice; }
hipError_t hipSetDevice(int) { return hipErrorNoDevice; }
hipError_t hipGetDeviceCount(int *count) { *count = 0; return hipErrorNoDevice; }
const char *hipGetErrorString(hipError_t) { return "no device"; }
}
namespace clsimhip {
hipError_t launch_event_stats(const EventStatsDeviceArgs &, hipStream_t) { return hipErrorNoDevice; }
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
    if (argc != 3) { std::fprintf(stderr, "usage: event_statistics_host_main IN OUT\n"); return 2; }
    try {
        std::ifstream in(argv[1], std::ios::binary);
        const std::vector<uint64_t> head = read_array<uint64_t>(in, 5);
        const std::vector<clsimhip_step> steps = read_array<clsimhip_step>(in, head[0]);
        const std::vector<clsimhip_photon> photons = read_array<clsimhip_photon>(in, head[1]);
        std::vector<clsimhip_mcpe_particle> particles = read_array<clsimhip_mcpe_particle>(in, head[2]);
        const std::vector<clsimhip_mcpe_mask> masked = read_array<clsimhip_mcpe_mask>(in, head[3]);
        const bool have_table = head[4] != 0;
        if (have_table && particles.empty()) particles.reserve(1);         // (an empty table is still a table: it has an address)
        const clsimhip_mcpe_particle *table = have_table ? particles.data() : nullptr;
        // exactly the records the call writes: a write past them is the sanitizer's to find
        std::vector<clsimhip_event_statistics> out(have_table ? particles.size() : 1u);
        uint64_t counters[3] = {0, 0, 0};
        clsimhip::event_stats_host(steps.data(), steps.size(), photons.data(), photons.size(), table, particles.size(), masked.data(), masked.size(), out.data(), counters);
        // no counters: the optional output is optional
        std::vector<clsimhip_event_statistics> again(out.size());
        clsimhip::event_stats_host(steps.data(), steps.size(), photons.data(), photons.size(), table, particles.size(), masked.data(), masked.size(), again.data(), nullptr);
        if (out.size() && std::memcmp(out.data(), again.data(), out.size() * sizeof out[0]) != 0) { std::fprintf(stderr, "a second run gave other bytes\n"); return 1; }
        // a table the twin refuses, and the device path without a device: errors, not crashes
        if (particles.size() >= 2) {
            std::vector<clsimhip_mcpe_particle> bad(particles);
            bad[1].identifier = bad[0].identifier;
            try {
                clsimhip::event_stats_host(steps.data(), steps.size(), photons.data(), photons.size(), bad.data(), bad.size(), masked.data(), masked.size(), again.data(), nullptr);
                std::fprintf(stderr, "a table that is not strictly increasing was accepted\n");
                return 1;
            } catch (const clsimhip::Error &e) {
                if (e.code != CLSIMHIP_ERR_ARGUMENT) throw;
            }
        }
        try {
            alignas(16) static uint8_t room[1 << 16];
            clsimhip::event_stats_device(0, room, 1, room, room, 1, nullptr, 0, nullptr, 0, room, room, room, sizeof room, nullptr);
            std::fprintf(stderr, "device() succeeded without a device\n");
            return 1;
        } catch (const clsimhip::Error &e) {
            if (e.code != CLSIMHIP_ERR_DEVICE) throw;
        }
        clsimhip_event_statistics total;
        std::memset(&total, 0, sizeof total);
        for (const clsimhip_event_statistics &r : out) clsimhip::event_stats_add(total, r);
        const double weights[2] = {clsimhip::event_stats_weight(total.generated_sum, total.generated_special),
                                   clsimhip::event_stats_weight(total.at_doms_sum, total.at_doms_special)};
        std::ofstream file(argv[2], std::ios::binary);
        file.write(reinterpret_cast<const char *>(out.data()), static_cast<std::streamsize>(out.size() * sizeof out[0]));
        file.write(reinterpret_cast<const char *>(counters), sizeof counters);
        file.write(reinterpret_cast<const char *>(&total), sizeof total);
        file.write(reinterpret_cast<const char *>(weights), sizeof weights);
        if (!file) throw clsimhip::Error(CLSIMHIP_ERR_IO, "cannot write the output file");
        std::printf("records %zu\n", out.size());
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "event_statistics_host_main: %s\n", e.what());
        return 1;
    }
}
