// Event statistics through the C++ adapter.  `event_statistics_adapter_test` alone checks the configuration and the two helpers (host
// only); `event_statistics_adapter_test run` needs a GPU: one bunch of 1024 steps (homogeneous ice, single string) of ten particles in
// two frames with the stage attached -- the adapter's GetLastEventStatistics() is the host twin's records of the enqueued steps and
// the returned photons byte for byte, and the in-place view carries them too.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "I3CLSimStepToPhotonConverterHIP.h"

int main(int argc, char **argv)
{
    const bool run = argc > 1 && std::strcmp(argv[1], "run") == 0;
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

    // the helpers: 3 x 2^-149 and -1 x 2^-149 add to 2 x 2^-149; a sum with both infinities is NaN
    clsimhip_event_statistics a, b;
    std::memset(&a, 0, sizeof a);
    std::memset(&b, 0, sizeof b);
    a.at_doms_sum[0] = 3u;
    for (int k = 0; k < 6; ++k) b.at_doms_sum[k] = ~uint64_t{0};
    b.at_doms_special[0] = 1u;
    if (clsimhip_event_statistics_add(&a, &b) != CLSIMHIP_OK || a.at_doms_sum[0] != 2u || a.at_doms_sum[5] != 0u || a.at_doms_special[0] != 1u) {
        std::printf("FAILED: clsimhip_event_statistics_add\n");
        return 1;
    }
    const uint32_t none[3] = {0, 0, 0}, both[3] = {1, 1, 0};
    if (clsimhip_event_statistics_weight(a.at_doms_sum, none) != std::ldexp(2., -149) || !std::isinf(clsimhip_event_statistics_weight(a.at_doms_sum, a.at_doms_special)) ||
        !std::isnan(clsimhip_event_statistics_weight(a.at_doms_sum, both))) {
        std::printf("FAILED: clsimhip_event_statistics_weight\n");
        return 1;
    }

    conv.SetWlenGenerators(std::vector<clsimhip_random_value>(1, gen));
    conv.SetWlenBias(bias);
    conv.SetMediumProperties(medium);
    conv.SetGeometry(sid, did, x, yy, z, sub, 0.16510 * 5.);
    conv.SetStopDetectedPhotons(true);
    conv.SetDOMPancakeFactor(5.);
    conv.SetEventStatistics(true);
    conv.SetEventStatistics(false);         // off again ...
    conv.SetEventStatistics(true);          // ... and on
    conv.Compile();
    conv.SetWorkgroupSize(conv.GetMaxWorkgroupSize());
    conv.SetMaxNumWorkitems(1024);
    clsimhip_medium_destroy(medium);
    std::printf("configured with the event statistics stage\n");
    if (!run) {
        std::printf("event statistics adapter ok (no GPU run requested)\n");
        return 0;
    }

    conv.Initialize();
    bool refused = false;
    try { conv.SetEventStatistics(false); } catch (const I3CLSimStepToPhotonConverter_exception &) { refused = true; }
    if (!refused) { std::printf("FAILED: the switch was taken after Initialize()\n"); return 1; }
    std::shared_ptr<I3CLSimStepSeries> steps(new I3CLSimStepSeries(1024));
    for (size_t i = 0; i < steps->size(); ++i) {
        I3CLSimStep &s = (*steps)[i];
        std::memset(&s, 0, sizeof s);
        s.theta = static_cast<float>(std::acos(1. - 2. * ((i * 37) % 1024) / 1024.));
        s.phi = static_cast<float>(6.283185307 * ((i * 101) % 1024) / 1024.);
        s.length = 0.001f; s.beta = 1.f; s.num_photons = (i < 1000) ? 200 : 0; s.weight = 0.25f + 0.001f * static_cast<float>(i % 7);
        s.identifier = 500u + static_cast<uint32_t>(i % 11);          // (510 is not in the table: UNKNOWN_STEP_PARTICLE, and it makes no photons)
        if (s.identifier == 510u) s.num_photons = 0;
    }
    std::vector<clsimhip_mcpe_particle> particles;
    for (uint32_t k = 0; k < 10; ++k) particles.push_back(clsimhip_mcpe_particle{500u + k, k % 2 ? 8u : 3u, 0.});
    std::vector<clsimhip_mcpe_mask> ignored;
    for (uint16_t om = 1; om <= 60; om += 2) ignored.push_back(clsimhip_mcpe_mask{3u, 1, om});
    conv.EnqueueSteps(steps, 42, particles, ignored);
    I3CLSimStepToPhotonConverter::ConversionResult_t r = conv.GetConversionResult();
    const size_t made = r.photons->size();
    std::vector<clsimhip_event_statistics> want(particles.size());
    uint64_t counters[3] = {0, 0, 0};
    if (clsimhip_event_statistics_host(reinterpret_cast<const clsimhip_step *>(steps->data()), steps->size(), reinterpret_cast<const clsimhip_photon *>(r.photons->data()), made,
                                       particles.data(), particles.size(), ignored.data(), ignored.size(), want.data(), counters) != CLSIMHIP_OK) {
        std::printf("host twin: %s\n", clsimhip_last_error(nullptr));
        return 1;
    }
    const std::vector<clsimhip_event_statistics> &got = conv.GetLastEventStatistics();
    uint64_t at_doms = 0;
    for (const clsimhip_event_statistics &e : want) at_doms += e.at_doms_count;
    bool same = got.size() == want.size() && std::memcmp(got.data(), want.data(), want.size() * sizeof want[0]) == 0;
    for (int k = 0; k < 3; ++k) same = same && conv.GetLastEventStatisticsCounter(k) == counters[k];
    if (!same || made == 0 || at_doms == 0 || counters[CLSIMHIP_EVENT_STATISTICS_MASKED] == 0 || at_doms + counters[CLSIMHIP_EVENT_STATISTICS_MASKED] != made ||
        counters[CLSIMHIP_EVENT_STATISTICS_UNKNOWN_STEP_PARTICLE] == 0) {
        std::printf("FAILED: %zu records from the adapter, %zu from the host twin of its %zu photons (%llu at DOMs, %llu masked)\n", got.size(), want.size(), made,
                    (unsigned long long)at_doms, (unsigned long long)counters[CLSIMHIP_EVENT_STATISTICS_MASKED]);
        return 1;
    }
    std::printf("identifier %u photons %zu at DOMs %llu masked %llu equal to the host twin\n", r.identifier, made, (unsigned long long)at_doms,
                (unsigned long long)counters[CLSIMHIP_EVENT_STATISTICS_MASKED]);
    // the in-place view carries the records too; a bunch without a table yields one
    conv.EnqueueSteps(steps, 43);
    I3CLSimStepToPhotonConverterHIP::ConversionResultView v = conv.GetConversionResultInPlace();
    clsimhip_event_statistics one;
    if (clsimhip_event_statistics_host(reinterpret_cast<const clsimhip_step *>(steps->data()), steps->size(), reinterpret_cast<const clsimhip_photon *>(v.photons), v.size, nullptr, 0,
                                       nullptr, 0, &one, counters) != CLSIMHIP_OK ||
        v.identifier != 43u || v.numEventStatistics != 1 || v.size == 0 || one.at_doms_count != v.size || std::memcmp(v.eventStatistics, &one, sizeof one) != 0) {
        std::printf("FAILED: the in-place view's records\n");
        return 1;
    }
    v.hold.reset();
    std::printf("event statistics adapter ok\n");
    return 0;
}
