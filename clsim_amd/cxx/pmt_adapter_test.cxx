// The multi-PMT hit generator through the C++ adapter.  `pmt_adapter_test` alone checks the configuration errors (host only);
// `pmt_adapter_test run` needs a GPU: one bunch of 1024 steps (homogeneous ice, single string, a 12-PMT module at every DOM) with the
// generator attached, the adapter's GetLastPMTHits() against the host twin of the photons the same result carries.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "I3CLSimStepToPhotonConverterHIP.h"

static bool less_hit(const clsimhip_pmt_hit &a, const clsimhip_pmt_hit &b)
{
    if (a.identifier != b.identifier) return a.identifier < b.identifier;
    if (a.om_id != b.om_id) return a.om_id < b.om_id;
    if (a.pmt != b.pmt) return a.pmt < b.pmt;
    return a.time < b.time;
}

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
    conv.SetPMTHitGenerator(but_one);
    bool refused = false;
    try { conv.Compile(); } catch (const I3CLSimStepToPhotonConverter_exception &e) { refused = std::strstr(e.what(), "No module configured for OMKey(1,60)") != nullptr; }
    if (!refused) { std::printf("FAILED: a DOM without module was not refused\n"); return 1; }
    conv.SetPMTHitGenerator(all, true);
    conv.Compile();
    conv.SetWorkgroupSize(conv.GetMaxWorkgroupSize());
    conv.SetMaxNumWorkitems(1024);
    clsimhip_medium_destroy(medium);
    clsimhip_pmt_generator_destroy(but_one);
    std::printf("configured with a PMT hit generator\n");
    if (!run) { clsimhip_pmt_generator_destroy(all); std::printf("pmt adapter ok (no GPU run requested)\n"); return 0; }

    conv.Initialize();
    std::shared_ptr<I3CLSimStepSeries> steps(new I3CLSimStepSeries(1024));
    for (size_t i = 0; i < steps->size(); ++i) {
        I3CLSimStep &s = (*steps)[i];
        std::memset(&s, 0, sizeof s);
        s.theta = static_cast<float>(std::acos(1. - 2. * ((i * 37) % 1024) / 1024.));
        s.phi = static_cast<float>(6.283185307 * ((i * 101) % 1024) / 1024.);
        s.length = 0.001f; s.beta = 1.f; s.num_photons = (i < 1000) ? 200 : 0; s.weight = 1.f; s.identifier = static_cast<uint32_t>(i);
    }
    conv.EnqueueSteps(steps, 42);
    I3CLSimStepToPhotonConverter::ConversionResult_t r = conv.GetConversionResult();
    std::vector<clsimhip_pmt_hit> got = conv.GetLastPMTHits();
    std::vector<clsimhip_pmt_hit> want(r.photons->size());
    size_t made = 0;
    uint64_t conditions[3];
    if (clsimhip_pmt_convert_host(all, reinterpret_cast<const clsimhip_photon *>(r.photons->data()), r.photons->size(), want.data(), want.size(), &made,
                                  conditions) != CLSIMHIP_OK) { std::printf("host twin: %s\n", clsimhip_pmt_generator_last_error(nullptr)); return 1; }
    want.resize(made);
    if (conditions[0] | conditions[1] | conditions[2]) { std::printf("FAILED: the host twin met a condition\n"); return 1; }
    std::sort(got.begin(), got.end(), less_hit);
    std::sort(want.begin(), want.end(), less_hit);
    if (got.size() != want.size() || got.empty() || got.size() >= r.photons->size() ||
        std::memcmp(got.data(), want.data(), got.size() * sizeof(clsimhip_pmt_hit)) != 0) {
        std::printf("FAILED: %zu hits from the adapter, %zu from the host twin of its %zu photons\n", got.size(), want.size(), r.photons->size());
        return 1;
    }
    std::printf("identifier %u photons %zu hits %zu equal to the host twin\n", r.identifier, r.photons->size(), got.size());
    // the in-place view carries them too
    conv.EnqueueSteps(steps, 43);
    {
        I3CLSimStepToPhotonConverterHIP::ConversionResultView v = conv.GetConversionResultInPlace();
        if (v.identifier != 43u || v.size == 0 || v.numPMTHits == 0 || !v.pmtHits || v.numPMTHits >= v.size) { std::printf("FAILED: in-place view\n"); return 1; }
        std::printf("view: identifier %u photons %zu hits %zu\n", v.identifier, v.size, v.numPMTHits);
    }
    clsimhip_pmt_generator_destroy(all);        // the converter keeps it alive
    conv.EnqueueSteps(steps, 44);
    r = conv.GetConversionResult();
    if (conv.GetLastPMTHits().empty()) { std::printf("FAILED: no hits after the caller dropped the generator\n"); return 1; }
    std::printf("pmt adapter ok\n");
    return 0;
}
