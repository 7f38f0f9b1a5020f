// The MCPE generator through the C++ adapter.  `mcpe_adapter_test` alone checks the configuration errors (host only);
// `mcpe_adapter_test run` needs a GPU: one bunch of 1024 steps (homogeneous ice, single string) with the generator attached,
// the adapter's GetLastMCPEs() against the host twin of the photons the same result carries.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "I3CLSimStepToPhotonConverterHIP.h"

static bool less_mcpe(const clsimhip_mcpe &a, const clsimhip_mcpe &b)
{
    if (a.identifier != b.identifier) return a.identifier < b.identifier;
    if (a.om_id != b.om_id) return a.om_id < b.om_id;
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

    // the hit maker: the wavelength acceptance the photons were biased with (weight x acceptance = 1), a linear angular acceptance
    const double coefficients[2] = {0.4, 0.3};
    clsimhip_polynomial angular = {2, coefficients, -INFINITY, INFINITY, NAN, NAN};
    std::vector<int32_t> classes(60, 0);
    clsimhip_mcpe_generator *all = nullptr, *but_one = nullptr;
    if (clsimhip_mcpe_generator_create(&bias, 1, 60, sid.data(), did.data(), classes.data(), &angular, 0.16510, 5., 5., 2024, &all) != CLSIMHIP_OK ||
        clsimhip_mcpe_generator_create(&bias, 1, 59, sid.data(), did.data(), classes.data(), &angular, 0.16510, 5., 5., 2024, &but_one) != CLSIMHIP_OK) {
        std::printf("generator: %s\n", clsimhip_mcpe_generator_last_error(nullptr));
        return 1;
    }

    conv.SetWlenGenerators(std::vector<clsimhip_random_value>(1, gen));
    conv.SetWlenBias(bias);
    conv.SetMediumProperties(medium);
    conv.SetGeometry(sid, did, x, yy, z, sub, 0.16510 * 5.);
    conv.SetStopDetectedPhotons(true);
    conv.SetDOMPancakeFactor(5.);
    conv.SetMCPEGenerator(but_one);
    bool refused = false;
    try { conv.Compile(); } catch (const I3CLSimStepToPhotonConverter_exception &e) { refused = std::strstr(e.what(), "No wavelength acceptance configured for OMKey(1,60)") != nullptr; }
    if (!refused) { std::printf("FAILED: a DOM without class was not refused\n"); return 1; }
    conv.SetMCPEGenerator(all, true);
    conv.Compile();
    conv.SetWorkgroupSize(conv.GetMaxWorkgroupSize());
    conv.SetMaxNumWorkitems(1024);
    clsimhip_medium_destroy(medium);
    clsimhip_mcpe_generator_destroy(but_one);
    std::printf("configured with an MCPE generator\n");
    if (!run) { clsimhip_mcpe_generator_destroy(all); std::printf("mcpe adapter ok (no GPU run requested)\n"); return 0; }

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
    std::vector<clsimhip_mcpe> got = conv.GetLastMCPEs();
    std::vector<clsimhip_mcpe> want(r.photons->size());
    size_t made = 0;
    uint64_t conditions[4];
    if (clsimhip_mcpe_convert_host(all, reinterpret_cast<const clsimhip_photon *>(r.photons->data()), r.photons->size(), want.data(), want.size(), &made,
                                   conditions) != CLSIMHIP_OK) { std::printf("host twin: %s\n", clsimhip_mcpe_generator_last_error(nullptr)); return 1; }
    want.resize(made);
    if (conditions[0] | conditions[1] | conditions[2] | conditions[3]) { std::printf("FAILED: the host twin met a condition\n"); return 1; }
    std::sort(got.begin(), got.end(), less_mcpe);
    std::sort(want.begin(), want.end(), less_mcpe);
    if (got.size() != want.size() || got.empty() || got.size() >= r.photons->size() ||
        std::memcmp(got.data(), want.data(), got.size() * sizeof(clsimhip_mcpe)) != 0) {
        std::printf("FAILED: %zu MCPEs from the adapter, %zu from the host twin of its %zu photons\n", got.size(), want.size(), r.photons->size());
        return 1;
    }
    std::printf("identifier %u photons %zu mcpes %zu equal to the host twin\n", r.identifier, r.photons->size(), got.size());
    // the in-place view carries them too
    conv.EnqueueSteps(steps, 43);
    {
        I3CLSimStepToPhotonConverterHIP::ConversionResultView v = conv.GetConversionResultInPlace();
        if (v.identifier != 43u || v.size == 0 || v.numMCPEs == 0 || !v.mcpes || v.numMCPEs >= v.size) { std::printf("FAILED: in-place view\n"); return 1; }
        std::printf("view: identifier %u photons %zu mcpes %zu\n", v.identifier, v.size, v.numMCPEs);
    }
    clsimhip_mcpe_generator_destroy(all);       // the converter keeps it alive
    conv.EnqueueSteps(steps, 44);
    r = conv.GetConversionResult();
    if (conv.GetLastMCPEs().empty()) { std::printf("FAILED: no MCPEs after the caller dropped the generator\n"); return 1; }
    std::printf("mcpe adapter ok\n");
    return 0;
}
