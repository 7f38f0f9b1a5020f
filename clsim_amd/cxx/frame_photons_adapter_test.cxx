// Frame photons through the C++ adapter.  `frame_photons_adapter_test` alone checks the configuration (host only);
// `frame_photons_adapter_test run` needs a GPU: one bunch of 1024 steps of ten particles in two frames (homogeneous ice, single
// string) with the stage attached, the adapter's GetLastFramePhotons() and GetLastFramePhotonSeries() against the host twin of the
// photons the same result carries, byte for byte.
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

    // the stage's DOM list for the host twin: the geometry's; IDs that do not fit the record are refused
    clsimhip_frame_photon_doms *doms = nullptr, *none = nullptr;
    if (clsimhip_frame_photon_doms_create(sid.size(), sid.data(), did.data(), &doms) != CLSIMHIP_OK) {
        std::printf("DOM list: %s\n", clsimhip_frame_photon_doms_last_error(nullptr));
        return 1;
    }
    const int32_t far_string = 40000;
    if (clsimhip_frame_photon_doms_create(1, &far_string, did.data(), &none) != CLSIMHIP_ERR_ARGUMENT ||
        !std::strstr(clsimhip_frame_photon_doms_last_error(nullptr), "does not fit the photon record")) {
        std::printf("FAILED: a string ID outside the record was not refused\n");
        return 1;
    }

    conv.SetWlenGenerators(std::vector<clsimhip_random_value>(1, gen));
    conv.SetWlenBias(bias);
    conv.SetMediumProperties(medium);
    conv.SetGeometry(sid, did, x, yy, z, sub, 0.16510 * 5.);
    conv.SetStopDetectedPhotons(true);
    conv.SetDOMPancakeFactor(5.);
    conv.SetFramePhotons(true, true);       // no generator is needed
    conv.Compile();
    conv.SetWorkgroupSize(conv.GetMaxWorkgroupSize());
    conv.SetMaxNumWorkitems(1024);
    clsimhip_medium_destroy(medium);
    std::printf("configured with the frame photons stage\n");
    if (!run) { clsimhip_frame_photon_doms_destroy(doms); std::printf("frame photons adapter ok (no GPU run requested)\n"); return 0; }

    conv.Initialize();
    std::shared_ptr<I3CLSimStepSeries> steps(new I3CLSimStepSeries(1024));
    for (size_t i = 0; i < steps->size(); ++i) {
        I3CLSimStep &s = (*steps)[i];
        std::memset(&s, 0, sizeof s);
        s.theta = static_cast<float>(std::acos(1. - 2. * ((i * 37) % 1024) / 1024.));
        s.phi = static_cast<float>(6.283185307 * ((i * 101) % 1024) / 1024.);
        s.length = 0.001f; s.beta = 1.f; s.num_photons = (i < 1000) ? 200 : 0; s.weight = 1.f; s.identifier = 500u + static_cast<uint32_t>(i % 10);
    }
    // ten particles, dealt to frames 9 and 4, with shifts; frame 9 ignores the module nearest to the source
    std::vector<clsimhip_mcpe_particle> particles(10);
    for (uint32_t k = 0; k < 10; ++k) { particles[k].identifier = 500u + k; particles[k].frame = (k % 2) ? 4u : 9u; particles[k].time_shift = 100. * k - 0.5; }
    std::vector<clsimhip_mcpe_mask> ignored(1);
    ignored[0].frame = 9u; ignored[0].string_id = 1; ignored[0].om_id = 30;
    conv.EnqueueSteps(steps, 42, particles, ignored);
    I3CLSimStepToPhotonConverter::ConversionResult_t r = conv.GetConversionResult();
    const std::vector<clsimhip_frame_photon> got = conv.GetLastFramePhotons();
    const std::vector<clsimhip_mcpe_series> table = conv.GetLastFramePhotonSeries();
    const size_t made = r.photons->size();
    std::vector<clsimhip_frame_photon> want(made);
    std::vector<clsimhip_mcpe_series> want_table(made);
    size_t kept = 0, n_series = 0;
    uint64_t counters[4];
    if (clsimhip_frame_photons_host(doms, reinterpret_cast<const clsimhip_photon *>(r.photons->data()), made, particles.data(), particles.size(), ignored.data(),
                                    ignored.size(), want.data(), want_table.data(), &kept, &n_series, counters) != CLSIMHIP_OK) {
        std::printf("host twin: %s\n", clsimhip_frame_photon_doms_last_error(nullptr));
        return 1;
    }
    if (counters[CLSIMHIP_FRAME_PHOTONS_UNKNOWN_PARTICLE] | counters[CLSIMHIP_FRAME_PHOTONS_UNKNOWN_DOM] | counters[CLSIMHIP_FRAME_PHOTONS_TIE_OVERFLOW]) {
        std::printf("FAILED: the host twin met a condition\n");
        return 1;
    }
    if (got.size() != kept || table.size() != n_series || kept == 0 || n_series < 2 || counters[CLSIMHIP_FRAME_PHOTONS_MASKED] == 0 ||
        conv.GetLastMaskedFramePhotons() != counters[CLSIMHIP_FRAME_PHOTONS_MASKED] || kept + counters[CLSIMHIP_FRAME_PHOTONS_MASKED] != made ||
        std::memcmp(got.data(), want.data(), kept * sizeof(clsimhip_frame_photon)) != 0 ||
        std::memcmp(table.data(), want_table.data(), n_series * sizeof(clsimhip_mcpe_series)) != 0) {
        std::printf("FAILED: %zu records in %zu series (%llu masked) from the adapter, %zu in %zu (%llu masked) from the host twin of its %zu photons\n", got.size(),
                    table.size(), (unsigned long long)conv.GetLastMaskedFramePhotons(), kept, n_series,
                    (unsigned long long)counters[CLSIMHIP_FRAME_PHOTONS_MASKED], made);
        return 1;
    }
    // as the frames receive them: two frames, every series under its module, nothing of the ignored module in frame 9
    const std::map<uint32_t, I3CLSimStepToPhotonConverterHIP::FramePhotonSeriesMap> frames = conv.GetLastFramePhotonMaps();
    size_t filed = 0;
    for (const auto &frame : frames)
        for (const auto &module : frame.second) filed += module.second.size();
    if (frames.size() != 2 || !frames.count(4) || !frames.count(9) || filed != kept || frames.at(9).count(std::make_pair(1, 30u)) || !frames.at(4).count(std::make_pair(1, 30u))) {
        std::printf("FAILED: the per-frame maps\n");
        return 1;
    }
    std::printf("identifier %u photons %zu records %zu series %zu masked %llu equal to the host twin\n", r.identifier, made, kept, n_series,
                (unsigned long long)counters[CLSIMHIP_FRAME_PHOTONS_MASKED]);
    // a bunch without a table: one frame, 0
    conv.EnqueueSteps(steps, 43);
    r = conv.GetConversionResult();
    if (r.identifier != 43u || conv.GetLastFramePhotonSeries().empty() || conv.GetLastMaskedFramePhotons() != 0) { std::printf("FAILED: the bunch without a table\n"); return 1; }
    for (const clsimhip_mcpe_series &s : conv.GetLastFramePhotonSeries())
        if (s.frame != 0u) { std::printf("FAILED: the bunch without a table has frame %u\n", s.frame); return 1; }
    clsimhip_frame_photon_doms_destroy(doms);
    std::printf("frame photons adapter ok\n");
    return 0;
}
