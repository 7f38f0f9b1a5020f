// Cable shadow through the C++ adapter.  `cable_shadow_adapter_test` alone checks the configuration (host only);
// `cable_shadow_adapter_test run` needs a GPU: one bunch of 1024 steps (homogeneous ice, single string) with the stage attached and
// the frame photons stage above it -- the result's photons are all detected photons, the adapter's GetLastShadowFlags() is the host
// twin's flags of those photons byte for byte, and GetLastFramePhotons() is the frame photons' host twin of the LIT ones.
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

    // one cable per DOM, in the DOM's own frame (a record's position is relative to its module): 20 cm from the centre, the azimuths
    // over half the circle, 1 m long, 2.3 cm thick; the last metre of a photon's path is tested
    std::vector<double> top, bottom, radius;
    for (int k = 0; k < 60; ++k) {
        const double azimuth = 3.141592653589793 * (k + 0.5) / 60.;
        top.push_back(0.2 * std::cos(azimuth)); top.push_back(0.2 * std::sin(azimuth)); top.push_back(0.5);
        bottom.push_back(0.2 * std::cos(azimuth)); bottom.push_back(0.2 * std::sin(azimuth)); bottom.push_back(-0.5);
        radius.push_back(0.023);
    }
    clsimhip_cable_shadow *shadow = nullptr, *none = nullptr;
    if (clsimhip_cable_shadow_create(radius.size(), top.data(), bottom.data(), radius.data(), 1.0, &shadow) != CLSIMHIP_OK) {
        std::printf("cable shadow: %s\n", clsimhip_cable_shadow_last_error(nullptr));
        return 1;
    }
    if (clsimhip_cable_shadow_create(radius.size(), top.data(), top.data(), radius.data(), 1.0, &none) != CLSIMHIP_ERR_ARGUMENT ||
        !std::strstr(clsimhip_cable_shadow_last_error(nullptr), "has no length")) {
        std::printf("FAILED: a cylinder without length was not refused\n");
        return 1;
    }
    clsimhip_frame_photon_doms *doms = nullptr;
    if (clsimhip_frame_photon_doms_create(sid.size(), sid.data(), did.data(), &doms) != CLSIMHIP_OK) { std::printf("DOM list: %s\n", clsimhip_last_error(nullptr)); return 1; }

    conv.SetWlenGenerators(std::vector<clsimhip_random_value>(1, gen));
    conv.SetWlenBias(bias);
    conv.SetMediumProperties(medium);
    conv.SetGeometry(sid, did, x, yy, z, sub, 0.16510 * 5.);
    conv.SetStopDetectedPhotons(true);
    conv.SetDOMPancakeFactor(5.);
    conv.SetCableShadow(shadow);
    conv.SetCableShadow(nullptr);           // off again ...
    conv.SetCableShadow(shadow);            // ... and on
    conv.SetFramePhotons(true, true);
    conv.Compile();
    conv.SetWorkgroupSize(conv.GetMaxWorkgroupSize());
    conv.SetMaxNumWorkitems(1024);
    clsimhip_medium_destroy(medium);
    std::printf("configured with the cable shadow stage\n");
    if (!run) {
        clsimhip_cable_shadow_destroy(shadow);
        clsimhip_frame_photon_doms_destroy(doms);
        std::printf("cable shadow adapter ok (no GPU run requested)\n");
        return 0;
    }

    conv.Initialize();
    bool refused = false;
    try { conv.SetCableShadow(nullptr); } catch (const I3CLSimStepToPhotonConverter_exception &) { refused = true; }
    if (!refused) { std::printf("FAILED: the switch was taken after Initialize()\n"); return 1; }
    std::shared_ptr<I3CLSimStepSeries> steps(new I3CLSimStepSeries(1024));
    for (size_t i = 0; i < steps->size(); ++i) {
        I3CLSimStep &s = (*steps)[i];
        std::memset(&s, 0, sizeof s);
        s.theta = static_cast<float>(std::acos(1. - 2. * ((i * 37) % 1024) / 1024.));
        s.phi = static_cast<float>(6.283185307 * ((i * 101) % 1024) / 1024.);
        s.length = 0.001f; s.beta = 1.f; s.num_photons = (i < 1000) ? 200 : 0; s.weight = 1.f; s.identifier = 500u + static_cast<uint32_t>(i % 10);
    }
    conv.EnqueueSteps(steps, 42);
    I3CLSimStepToPhotonConverter::ConversionResult_t r = conv.GetConversionResult();
    const size_t made = r.photons->size();
    const clsimhip_photon *photons = reinterpret_cast<const clsimhip_photon *>(r.photons->data());
    std::vector<uint8_t> flags(made);
    std::vector<clsimhip_photon> lit(made);
    size_t n_lit = 0;
    uint64_t counts[2] = {0, 0};
    if (clsimhip_cable_shadow_host(shadow, photons, made, flags.data(), lit.data(), &n_lit, counts) != CLSIMHIP_OK) {
        std::printf("host twin: %s\n", clsimhip_cable_shadow_last_error(nullptr));
        return 1;
    }
    const std::vector<uint8_t> &got = conv.GetLastShadowFlags();
    if (got.size() != made || counts[0] != made || counts[1] == 0 || counts[1] >= made || conv.GetLastShadowTested() != counts[0] ||
        conv.GetLastShadowShadowed() != counts[1] || std::memcmp(got.data(), flags.data(), made) != 0) {
        std::printf("FAILED: %zu flags, %llu tested, %llu shadowed from the adapter; %llu tested, %llu shadowed from the host twin of its %zu photons\n", got.size(),
                    (unsigned long long)conv.GetLastShadowTested(), (unsigned long long)conv.GetLastShadowShadowed(), (unsigned long long)counts[0],
                    (unsigned long long)counts[1], made);
        return 1;
    }
    // the stage above saw the lit records only
    std::vector<clsimhip_frame_photon> want(made);
    std::vector<clsimhip_mcpe_series> want_table(made);
    size_t kept = 0, n_series = 0;
    if (clsimhip_frame_photons_host(doms, lit.data(), n_lit, nullptr, 0, nullptr, 0, want.data(), want_table.data(), &kept, &n_series, nullptr) != CLSIMHIP_OK) {
        std::printf("frame photons host twin: %s\n", clsimhip_last_error(nullptr));
        return 1;
    }
    if (kept != n_lit || conv.GetLastFramePhotons().size() != kept || conv.GetLastFramePhotonSeries().size() != n_series ||
        std::memcmp(conv.GetLastFramePhotons().data(), want.data(), kept * sizeof(clsimhip_frame_photon)) != 0 ||
        std::memcmp(conv.GetLastFramePhotonSeries().data(), want_table.data(), n_series * sizeof(clsimhip_mcpe_series)) != 0) {
        std::printf("FAILED: %zu frame photons from the adapter, %zu from the host twin of the %zu lit records\n", conv.GetLastFramePhotons().size(), kept, n_lit);
        return 1;
    }
    std::printf("identifier %u photons %zu shadowed %llu lit %zu equal to the host twin\n", r.identifier, made, (unsigned long long)counts[1], n_lit);
    // the in-place view carries flags and counts too
    conv.EnqueueSteps(steps, 43);
    I3CLSimStepToPhotonConverterHIP::ConversionResultView v = conv.GetConversionResultInPlace();
    std::vector<uint8_t> again(v.size);
    if (clsimhip_cable_shadow_host(shadow, reinterpret_cast<const clsimhip_photon *>(v.photons), v.size, again.data(), std::vector<clsimhip_photon>(v.size).data(), nullptr,
                                   counts) != CLSIMHIP_OK ||
        v.identifier != 43u || v.numShadowFlags != v.size || v.size == 0 || v.shadowCounts[0] != counts[0] || v.shadowCounts[1] != counts[1] ||
        std::memcmp(v.shadowFlags, again.data(), v.size) != 0) {
        std::printf("FAILED: the in-place view's flags\n");
        return 1;
    }
    v.hold.reset();
    clsimhip_cable_shadow_destroy(shadow);
    clsimhip_frame_photon_doms_destroy(doms);
    std::printf("cable shadow adapter ok\n");
    return 0;
}
