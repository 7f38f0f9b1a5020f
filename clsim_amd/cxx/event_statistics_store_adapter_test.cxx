// The event statistics frame store through the C++ adapter (I3EventStatisticsStoreHIP.h).  `event_statistics_store_adapter_test` alone
// builds a host store, adds three small bunches under a relabel map and drains them in two steps (host only);
// `event_statistics_store_adapter_test run` needs a GPU: a converter with the event statistics stage on (homogeneous ice, single string),
// three bunches of 1024 steps dealt to 16 particles in three frames, half of them slices of the other half, every result added to a device
// store and to a host store, and both compared with the twin's canonical form of all results.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "I3EventStatisticsStoreHIP.h"

namespace {
typedef std::vector<clsimhip_event_statistics> Records;
typedef I3EventStatisticsStoreHIP::RelabelMap RelabelMap;
typedef std::map<uint32_t, I3EventStatisticsStoreHIP::ParticleMap> Frames;

// a record whose sums are whole multiples of 2^-149 x 2^149 = 1: `generated` and `atDOMs` as weights 1.0 each
clsimhip_event_statistics record(uint32_t frame, uint32_t identifier, uint64_t generated, uint64_t atDOMs)
{
    clsimhip_event_statistics r;
    std::memset(&r, 0, sizeof r);
    r.frame = frame; r.identifier = identifier;
    r.generated_count = generated; r.at_doms_count = atDOMs;
    r.generated_sum[2] = generated << 21;                               // 2^149 = bit 21 of word 2
    r.at_doms_sum[2] = atDOMs << 21;
    return r;
}

size_t count(const Frames &frames)
{
    size_t n = 0;
    for (const auto &frame : frames) n += frame.second.size();
    return n;
}
} // namespace

static int host_store()
{
    I3EventStatisticsStoreHIP store(64);
    const RelabelMap slices = {{1000u, 7u}, {1001u, 7u}};               // two slices of muon 7
    store.Add({record(3u, 7u, 0u, 0u), record(3u, 1000u, 10u, 1u), record(3u, 1001u, 20u, 2u), record(9u, 5u, 100u, 3u)}, slices);
    store.Add({record(3u, 1001u, 5u, 1u), record(4u, 6u, 50u, 0u)}, slices);
    store.Add({record(9u, 5u, 1u, 1u), record(9u, 1000u, 2u, 2u), record(3u, 8u, 0u, 0u)}, slices);
    if (store.Size() != 4 || store.Size(4u) != 2) { std::printf("FAILED: sizes\n"); return 1; }
    // a map that sends a muon on is refused and changes nothing
    bool refused = false;
    try { store.Add({record(3u, 7u, 1u, 1u)}, RelabelMap{{5u, 8u}, {8u, 2u}}); } catch (const I3CLSimStepToPhotonConverter_exception &e) { refused = std::strstr(e.what(), "sends 5 to 8") != nullptr; }
    if (!refused || store.Size() != 4) { std::printf("FAILED: a bad map was taken\n"); return 1; }
    const Frames early = store.Drain(4u);
    const I3EventStatisticsStoreHIP::ParticleStatistics &muon = early.at(3u).at(7u);
    if (early.size() != 2 || count(early) != 2 || muon.numPhotonsGenerated != 35u || muon.numPhotonsAtDOMs != 4u || muon.sumOfWeightsPhotonsGenerated != 35. ||
        muon.sumOfWeightsPhotonsAtDOMs != 4. || early.at(4u).at(6u).numPhotonsGenerated != 50u) { std::printf("FAILED: the early frames\n"); return 1; }
    const Frames late = store.Drain();
    if (late.size() != 1 || late.at(9u).size() != 2 || late.at(9u).at(5u).numPhotonsGenerated != 101u || late.at(9u).at(5u).sumOfWeightsPhotonsAtDOMs != 4. ||
        late.at(9u).at(7u).numPhotonsAtDOMs != 2u || store.Size() != 0) { std::printf("FAILED: the late frames\n"); return 1; }
    std::printf("host store: 3 bunches 9 records, 2 empty, frames <= 4 gave 2 particles in 2 frames, the rest 2 particles in one frame\n");
    return 0;
}

int main(int argc, char **argv)
{
    const bool run = argc > 1 && std::strcmp(argv[1], "run") == 0;
    if (host_store() != 0) return 1;
    if (!run) { std::printf("event statistics store adapter ok (no GPU run requested)\n"); return 0; }

    I3CLSimStepToPhotonConverterHIP conv(0);
    clsimhip_medium_desc d;
    std::memset(&d, 0, sizeof d);
    const double absLen = 100., scaLen = 25.;
    d.num_layers = 1; d.layers_z_start = -1000.; d.layers_height = 2000.;
    d.min_wavelength = 265e-9; d.max_wavelength = 675e-9;
    d.lengths_kind = CLSIMHIP_LENGTHS_CONSTANT; d.abs_length = &absLen; d.sca_length = &scaLen;
    const double n[5] = {1.55749, -1.57988, 3.99993, -4.68271, 2.09354}, g[5] = {1.227106, -0.954648, 1.42568, -0.711832, 0.0};
    for (int i = 0; i < 5; ++i) { d.n[i] = n[i]; d.g[i] = g[i]; }
    d.scatter_kind = CLSIMHIP_SCATTER_MIXED; d.liu_fraction = 0.45; d.mean_cosine = 0.9;
    clsimhip_medium *medium = nullptr;
    if (clsimhip_medium_create(&d, &medium) != CLSIMHIP_OK) { std::printf("medium: %s\n", clsimhip_last_error(nullptr)); return 1; }

    std::vector<double> acc(43), y(43);
    double start = 0, step = 0, first = 0, spacing = 0;
    clsimhip_icecube_dom_acceptance(0.16510, 1.0, acc.data(), &start, &step);
    clsimhip_function bias = {CLSIMHIP_FUNCTION_TABLE, 43, start, step, acc.data(), 0., nullptr};
    clsimhip_make_cherenkov_wlen_generator(&bias, medium, y.data(), &first, &spacing);
    clsimhip_random_value gen = {CLSIMHIP_RANDOM_INTERPOLATED, 43, first, spacing, y.data(), 0., nullptr};

    std::vector<int32_t> sid; std::vector<uint32_t> did; std::vector<double> x, yy, z; std::vector<std::string> sub;
    for (int k = 0; k < 60; ++k) { sid.push_back(1); did.push_back(k + 1); x.push_back(20.); yy.push_back(20.); z.push_back(500. - 17. * k); sub.push_back("IceCube"); }

    conv.SetWlenGenerators(std::vector<clsimhip_random_value>(1, gen));
    conv.SetWlenBias(bias);
    conv.SetMediumProperties(medium);
    conv.SetGeometry(sid, did, x, yy, z, sub, 0.16510 * 5.);
    conv.SetStopDetectedPhotons(true);
    conv.SetDOMPancakeFactor(5.);
    conv.SetEventStatistics(true);
    conv.Compile();
    conv.SetWorkgroupSize(conv.GetMaxWorkgroupSize());
    conv.SetMaxNumWorkitems(1024);
    clsimhip_medium_destroy(medium);
    conv.Initialize();

    // sixteen particles in three frames; 508 ... 515 are slices of 500 ... 507 (a slice lies in its muon's frame)
    const uint32_t frame_ids[3] = {90u, 3u, 41u};
    std::vector<clsimhip_mcpe_particle> particles;
    for (uint32_t k = 0; k < 16; ++k) { clsimhip_mcpe_particle p = {500u + k, frame_ids[(k % 8) % 3], 0.}; particles.push_back(p); }
    RelabelMap slices;
    for (uint32_t k = 8; k < 16; ++k) { clsimhip_relabel m = {500u + k, 500u + k - 8u}; slices.push_back(m); }
    I3EventStatisticsStoreHIP on_device(64, 0), on_host(64), late(64, 0);
    Records all;
    uint64_t generated = 0, atDOMs = 0;
    for (uint32_t bunch = 0; bunch < 3; ++bunch) {
        std::shared_ptr<I3CLSimStepSeries> steps(new I3CLSimStepSeries(1024));
        for (size_t i = 0; i < steps->size(); ++i) {
            I3CLSimStep &s = (*steps)[i];
            std::memset(&s, 0, sizeof s);
            s.theta = static_cast<float>(std::acos(1. - 2. * ((i * 37 + bunch) % 1024) / 1024.));
            s.phi = static_cast<float>(6.283185307 * ((i * 101) % 1024) / 1024.);
            s.length = 0.001f; s.beta = 1.f; s.num_photons = (i < 1000) ? 200 : 0; s.weight = 1.f; s.identifier = 500u + static_cast<uint32_t>(i % 16);
            generated += s.num_photons;
        }
        conv.EnqueueSteps(steps, 42 + bunch, particles);
        conv.GetConversionResult();
        const Records &records = conv.GetLastEventStatistics();
        if (records.size() != particles.size()) { std::printf("FAILED: %zu records for %zu particles\n", records.size(), particles.size()); return 1; }
        on_device.Add(records, slices);
        on_host.Add(records, slices);
        late.Add(records);
        all.insert(all.end(), records.begin(), records.end());
        for (const clsimhip_event_statistics &r : records) atDOMs += r.at_doms_count;
    }
    Records twin(all.size());
    size_t made = 0;
    uint64_t counters[2] = {0, 0};
    if (clsimhip_event_statistics_canonical_host(all.data(), all.size(), slices.data(), slices.size(), twin.data(), twin.size(), &made, counters) != CLSIMHIP_OK) {
        std::printf("host twin: %s\n", clsimhip_last_error(nullptr));
        return 1;
    }
    twin.resize(made);
    if (made != 8 || counters[0] != 24 || on_device.Size() != made || on_host.Size() != made || late.Size() != 16) {
        std::printf("FAILED: %zu records in the twin, %zu in the device store, %zu in the host store\n", made, on_device.Size(), on_host.Size());
        return 1;
    }
    // frames 3 and 41 leave, frame 90 stays: flat from the device stores (one folds when the frames leave), as maps from the host store
    Records head, folded;
    on_device.DrainFlat(41u, head);
    late.DrainFlat(41u, folded, slices);
    const size_t n_head = head.size();
    if (n_head == 0 || n_head >= made || std::memcmp(head.data(), twin.data(), n_head * sizeof(clsimhip_event_statistics)) != 0 || head.back().frame != 41u ||
        twin[n_head].frame != 90u || folded.size() != n_head || std::memcmp(folded.data(), head.data(), n_head * sizeof(clsimhip_event_statistics)) != 0) {
        std::printf("FAILED: the head of the device stores\n");
        return 1;
    }
    const Frames frames = on_host.Drain(41u);
    if (frames.size() != 2 || count(frames) != n_head) { std::printf("FAILED: the head of the host store\n"); return 1; }
    Records tail;
    on_device.DrainFlat(I3EventStatisticsStoreHIP::AllFrames, tail);
    if (tail.size() != made - n_head || std::memcmp(tail.data(), twin.data() + n_head, tail.size() * sizeof(clsimhip_event_statistics)) != 0 || on_device.Size() != 0) {
        std::printf("FAILED: the tail of the device store\n");
        return 1;
    }
    const Frames rest = on_host.Drain();
    uint64_t seen_generated = 0, seen_atDOMs = 0;
    double weight = 0.;
    for (const Frames *f : {&frames, &rest})
        for (const auto &frame : *f)
            for (const auto &particle : frame.second) {
                seen_generated += particle.second.numPhotonsGenerated;
                seen_atDOMs += particle.second.numPhotonsAtDOMs;
                weight += particle.second.sumOfWeightsPhotonsGenerated;
            }
    if (rest.size() != 1 || !rest.count(90u) || count(rest) != tail.size() || seen_generated != generated || seen_atDOMs != atDOMs || weight != static_cast<double>(generated)) {
        std::printf("FAILED: the tail of the host store\n");
        return 1;
    }
    std::printf("bunches 3 records %zu particles %zu head %zu tail %zu generated %llu at DOMs %llu equal to the host twin\n", all.size(), made, n_head, tail.size(),
                static_cast<unsigned long long>(generated), static_cast<unsigned long long>(atDOMs));
    std::printf("event statistics store adapter ok\n");
    return 0;
}
