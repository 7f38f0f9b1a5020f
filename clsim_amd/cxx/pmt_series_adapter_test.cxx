// The PMT series through the C++ adapter.  `pmt_series_adapter_test` alone checks the configuration errors (host only);
// `pmt_series_adapter_test run` needs a GPU: one bunch of 1024 steps of ten particles in two frames (homogeneous ice, single string, a
// 12-PMT module at every DOM) with the generator and the series stage attached, the adapter's GetLastPMTHits() and
// GetLastPMTSeries() against the host twins (hit maker, then series) of the photons the same result carries, byte for byte.
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

    // the hit maker: glass / gel survival 0.9, the quantum efficiency the photons were biased with (weight x Q = 1), an angular
    // acceptance factor of 0.8 c; twelve PMTs on a Fibonacci sphere, discs of 0.3 R at 0.85 R; every module turned about z
    const double R = 0.16510, factor[2] = {0., 0.8};
    const clsimhip_function functions[3] = {{CLSIMHIP_FUNCTION_CONSTANT, 0, 0., 0., nullptr, 0.9, nullptr}, bias,
                                            {CLSIMHIP_FUNCTION_TABLE, 2, 0., 1., factor, 0., nullptr}};
    std::vector<clsimhip_pmt> pmts(12);
    for (int i = 0; i < 12; ++i) {
        const double az = 1. - (2. * i + 1.) / 12., rho = std::sqrt(1. - az * az), phi = i * 2.399963229728653;
        const double axis[3] = {rho * std::cos(phi), rho * std::sin(phi), az};
        for (int k = 0; k < 3; ++k) { pmts[i].axis[k] = axis[k]; pmts[i].position[k] = 0.85 * R * axis[k]; }
        pmts[i].radius = 0.3 * R; pmts[i].collection_efficiency = 0.9; pmts[i].quantum_efficiency = 1; pmts[i].angular_acceptance = 2;
    }
    const clsimhip_pmt_type type = {R, 0, 12, 0, 0};
    std::vector<clsimhip_pmt_module> modules(60);
    for (int k = 0; k < 60; ++k) {
        const double c = std::cos(0.1 * k), s = std::sin(0.1 * k);
        const double m[9] = {c, -s, 0., s, c, 0., 0., 0., 1.};
        modules[k].string_id = 1; modules[k].om_id = k + 1; modules[k].type = 0; modules[k].reserved = 0;
        std::memcpy(modules[k].rotation, m, sizeof m);
    }
    clsimhip_pmt_generator *all = nullptr, *but_one = nullptr, *none = nullptr;
    if (clsimhip_pmt_generator_create(functions, 3, &type, 1, pmts.data(), 12, modules.data(), 60, 2024, &all) != CLSIMHIP_OK ||
        clsimhip_pmt_generator_create(functions, 3, &type, 1, pmts.data(), 12, modules.data(), 59, 2024, &but_one) != CLSIMHIP_OK) {
        std::printf("generator: %s\n", clsimhip_pmt_generator_last_error(nullptr));
        return 1;
    }
    modules[7].rotation[0] *= 1.01;
    if (clsimhip_pmt_generator_create(functions, 3, &type, 1, pmts.data(), 12, modules.data(), 60, 2024, &none) != CLSIMHIP_ERR_CONFIG ||
        !std::strstr(clsimhip_pmt_generator_last_error(nullptr), "rotation does change vector length")) {
        std::printf("FAILED: a rotation that changes lengths was not refused\n");
        return 1;
    }

    conv.SetWlenGenerators(std::vector<clsimhip_random_value>(1, gen));
    conv.SetWlenBias(bias);
    conv.SetMediumProperties(medium);
    conv.SetGeometry(sid, did, x, yy, z, sub, 0.16510 * 5.);
    conv.SetStopDetectedPhotons(true);
    conv.SetDOMPancakeFactor(5.);
    // the switch without a generator
    conv.SetPMTSeries(true);
    bool refused = false;
    try { conv.Compile(); } catch (const I3CLSimStepToPhotonConverter_exception &e) { refused = std::strstr(e.what(), "need a PMT hit generator") != nullptr; }
    if (!refused) { std::printf("FAILED: the PMT series switch without a generator was not refused\n"); return 1; }
    conv.SetPMTHitGenerator(all, true);
    conv.Compile();
    conv.SetWorkgroupSize(conv.GetMaxWorkgroupSize());
    conv.SetMaxNumWorkitems(1024);
    clsimhip_medium_destroy(medium);
    clsimhip_pmt_generator_destroy(but_one);
    std::printf("configured with the PMT series stage\n");
    if (!run) { clsimhip_pmt_generator_destroy(all); std::printf("pmt series adapter ok (no GPU run requested)\n"); return 0; }

    conv.Initialize();
    std::shared_ptr<I3CLSimStepSeries> steps(new I3CLSimStepSeries(1024));
    for (size_t i = 0; i < steps->size(); ++i) {
        I3CLSimStep &s = (*steps)[i];
        std::memset(&s, 0, sizeof s);
        s.theta = static_cast<float>(std::acos(1. - 2. * ((i * 37) % 1024) / 1024.));
        s.phi = static_cast<float>(6.283185307 * ((i * 101) % 1024) / 1024.);
        s.length = 0.001f; s.beta = 1.f; s.num_photons = (i < 1000) ? 200 : 0; s.weight = 1.f; s.identifier = 500u + static_cast<uint32_t>(i % 10);
    }
    // ten particles, dealt to frames 9 and 4, with shifts; both frames ignore the module nearest to the source in one of them
    std::vector<clsimhip_mcpe_particle> particles(10);
    for (uint32_t k = 0; k < 10; ++k) { particles[k].identifier = 500u + k; particles[k].frame = (k % 2) ? 4u : 9u; particles[k].time_shift = 100. * k - 0.5; }
    std::vector<clsimhip_mcpe_mask> ignored(1);
    ignored[0].frame = 9u; ignored[0].string_id = 1; ignored[0].om_id = 30;
    conv.EnqueueSteps(steps, 42, particles, ignored);
    I3CLSimStepToPhotonConverter::ConversionResult_t r = conv.GetConversionResult();
    const std::vector<clsimhip_pmt_hit> got = conv.GetLastPMTHits();
    const std::vector<clsimhip_pmt_series> table = conv.GetLastPMTSeries();
    std::vector<clsimhip_pmt_hit> hits(r.photons->size());
    size_t made = 0;
    uint64_t conditions[3];
    if (clsimhip_pmt_convert_host(all, reinterpret_cast<const clsimhip_photon *>(r.photons->data()), r.photons->size(), hits.data(), hits.size(), &made,
                                  conditions) != CLSIMHIP_OK) { std::printf("host twin: %s\n", clsimhip_pmt_generator_last_error(nullptr)); return 1; }
    hits.resize(made);
    std::vector<clsimhip_pmt_hit> want(made);
    std::vector<clsimhip_pmt_series> want_table(made);
    size_t kept = 0, n_series = 0;
    uint64_t counters[3];
    if (clsimhip_pmt_series_host(all, hits.data(), hits.size(), particles.data(), particles.size(), ignored.data(), ignored.size(), want.data(), want_table.data(),
                                 &kept, &n_series, counters) != CLSIMHIP_OK) { std::printf("host twin: %s\n", clsimhip_pmt_generator_last_error(nullptr)); return 1; }
    if (counters[CLSIMHIP_PMT_SERIES_UNKNOWN_PARTICLE] | counters[CLSIMHIP_PMT_SERIES_UNKNOWN_CHANNEL]) { std::printf("FAILED: the host twin met a condition\n"); return 1; }
    if (got.size() != kept || table.size() != n_series || kept == 0 || n_series < 2 || counters[CLSIMHIP_PMT_SERIES_MASKED] == 0 ||
        conv.GetLastMaskedPMTHits() != counters[CLSIMHIP_PMT_SERIES_MASKED] || kept + counters[CLSIMHIP_PMT_SERIES_MASKED] != made ||
        std::memcmp(got.data(), want.data(), kept * sizeof(clsimhip_pmt_hit)) != 0 ||
        std::memcmp(table.data(), want_table.data(), n_series * sizeof(clsimhip_pmt_series)) != 0) {
        std::printf("FAILED: %zu hits in %zu series (%llu masked) from the adapter, %zu in %zu (%llu masked) from the host twins of its %zu photons\n", got.size(),
                    table.size(), (unsigned long long)conv.GetLastMaskedPMTHits(), kept, n_series, (unsigned long long)counters[CLSIMHIP_PMT_SERIES_MASKED],
                    r.photons->size());
        return 1;
    }
    // as the frames receive them: two frames, every series under its module and PMT, nothing of the ignored module in frame 9
    const std::map<uint32_t, I3CLSimStepToPhotonConverterHIP::PMTHitSeriesMap> frames = conv.GetLastPMTSeriesMaps();
    size_t filed = 0;
    for (const auto &frame : frames)
        for (const auto &module : frame.second)
            for (const auto &pmt : module.second) filed += pmt.second.size();
    if (frames.size() != 2 || !frames.count(4) || !frames.count(9) || filed != kept || frames.at(9).count(std::make_pair(1, 30u)) || !frames.at(4).count(std::make_pair(1, 30u))) {
        std::printf("FAILED: the per-frame maps\n");
        return 1;
    }
    std::printf("identifier %u photons %zu hits %zu series %zu masked %llu equal to the host twins\n", r.identifier, r.photons->size(), kept, n_series,
                (unsigned long long)counters[CLSIMHIP_PMT_SERIES_MASKED]);
    // a bunch without a table: one frame, 0
    conv.EnqueueSteps(steps, 43);
    r = conv.GetConversionResult();
    if (r.identifier != 43u || conv.GetLastPMTSeries().empty() || conv.GetLastMaskedPMTHits() != 0) { std::printf("FAILED: the bunch without a table\n"); return 1; }
    for (const clsimhip_pmt_series &s : conv.GetLastPMTSeries())
        if (s.frame != 0u) { std::printf("FAILED: the bunch without a table has frame %u\n", s.frame); return 1; }
    clsimhip_pmt_generator_destroy(all);        // the converter keeps it alive
    std::printf("pmt series adapter ok\n");
    return 0;
}
