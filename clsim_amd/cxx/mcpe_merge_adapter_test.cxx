// MCPE merging through the C++ adapter.  `mcpe_merge_adapter_test` alone checks the configuration errors (host only);
// `mcpe_merge_adapter_test run` needs a GPU: one bunch of 1024 steps (homogeneous ice, single string) dealt to 16 particles in
// three frames; the adapter's flat views and per-frame maps against the host twins applied to the photons the result carries.
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

    // the hit maker: the wavelength acceptance the photons were biased with (weight x acceptance = 1), a linear angular acceptance
    const double coefficients[2] = {0.4, 0.3};
    clsimhip_polynomial angular = {2, coefficients, -INFINITY, INFINITY, NAN, NAN};
    std::vector<int32_t> classes(60, 0);
    clsimhip_mcpe_generator *all = nullptr;
    if (clsimhip_mcpe_generator_create(&bias, 1, 60, sid.data(), did.data(), classes.data(), &angular, 0.16510, 5., 5., 2024, &all) != CLSIMHIP_OK) {
        std::printf("generator: %s\n", clsimhip_mcpe_generator_last_error(nullptr));
        return 1;
    }

    conv.SetWlenGenerators(std::vector<clsimhip_random_value>(1, gen));
    conv.SetWlenBias(bias);
    conv.SetMediumProperties(medium);
    conv.SetGeometry(sid, did, x, yy, z, sub, 0.16510 * 5.);
    conv.SetStopDetectedPhotons(true);
    conv.SetDOMPancakeFactor(5.);
    // merging without the series stage is refused when compiling; a window that is no window at once
    const double window = 40.;
    conv.SetMCPEGenerator(all, true);
    conv.SetMCPEMerging(window);
    bool refused = false;
    try { conv.Compile(); } catch (const I3CLSimStepToPhotonConverter_exception &e) { refused = std::strstr(e.what(), "needs the MCPE series stage") != nullptr; }
    if (!refused) { std::printf("FAILED: MCPE merging without the series stage was not refused\n"); return 1; }
    refused = false;
    try { conv.SetMCPEMerging(-1.); } catch (const I3CLSimStepToPhotonConverter_exception &) { refused = true; }
    if (!refused) { std::printf("FAILED: a negative window was taken\n"); return 1; }
    conv.SetMCPESeries(true);
    conv.Compile();
    conv.SetWorkgroupSize(conv.GetMaxWorkgroupSize());
    conv.SetMaxNumWorkitems(1024);
    clsimhip_medium_destroy(medium);
    std::printf("configured with MCPE merging\n");
    if (!run) { clsimhip_mcpe_generator_destroy(all); std::printf("mcpe merge adapter ok (no GPU run requested)\n"); return 0; }

    conv.Initialize();
    refused = false;
    try { conv.SetMCPEMerging(window); } catch (const I3CLSimStepToPhotonConverter_exception &) { refused = true; }
    if (!refused) { std::printf("FAILED: the switch was taken after Initialize()\n"); return 1; }
    std::shared_ptr<I3CLSimStepSeries> steps(new I3CLSimStepSeries(1024));
    for (size_t i = 0; i < steps->size(); ++i) {
        I3CLSimStep &s = (*steps)[i];
        std::memset(&s, 0, sizeof s);
        s.theta = static_cast<float>(std::acos(1. - 2. * ((i * 37) % 1024) / 1024.));
        s.phi = static_cast<float>(6.283185307 * ((i * 101) % 1024) / 1024.);
        s.length = 0.001f; s.beta = 1.f; s.num_photons = (i < 1000) ? 200 : 0; s.weight = 1.f; s.identifier = 500u + static_cast<uint32_t>(i % 16);
    }
    const uint32_t frame_ids[3] = {90u, 3u, 41u};
    std::vector<clsimhip_mcpe_particle> particles;
    for (uint32_t k = 0; k < 16; ++k) { clsimhip_mcpe_particle p = {500u + k, frame_ids[k % 3], 1000. * (k % 4) - 0.5}; particles.push_back(p); }
    conv.EnqueueSteps(steps, 42, particles);
    I3CLSimStepToPhotonConverter::ConversionResult_t r = conv.GetConversionResult();
    const size_t count = r.photons->size();
    std::vector<clsimhip_mcpe> made(count), sorted(count);
    std::vector<clsimhip_mcpe_series> series(count), merged_series(count);
    std::vector<clsimhip_mcpe_merged> merged(count);
    std::vector<clsimhip_mcpe_parent> parents(count);
    std::vector<clsimhip_mcpe_parent_range> ranges(count);
    size_t n_made = 0, n_kept = 0, n_series = 0, n_merged = 0, n_parents = 0;
    uint64_t conditions[4], counters[3];
    if (clsimhip_mcpe_convert_host(all, reinterpret_cast<const clsimhip_photon *>(r.photons->data()), count, made.data(), made.size(), &n_made, conditions) != CLSIMHIP_OK ||
        clsimhip_mcpe_series_host(all, made.data(), n_made, particles.data(), particles.size(), nullptr, 0, sorted.data(), series.data(), &n_kept, &n_series,
                                  counters) != CLSIMHIP_OK ||
        clsimhip_mcpe_merge_host(sorted.data(), n_kept, series.data(), n_series, window, merged.data(), merged_series.data(), parents.data(), ranges.data(),
                                 &n_merged, &n_parents) != CLSIMHIP_OK) {
        std::printf("host twin: %s\n", clsimhip_last_error(nullptr));
        return 1;
    }
    if (conv.GetLastMCPEs().size() != n_kept || conv.GetLastMCPESeries().size() != n_series || conv.GetLastMergedMCPEs().size() != n_merged ||
        conv.GetLastMergedMCPESeries().size() != n_series || conv.GetLastMCPEParents().size() != n_parents || conv.GetLastMCPEParentRanges().size() != n_series ||
        n_merged == 0 || n_merged >= n_kept || n_parents < n_merged ||
        std::memcmp(conv.GetLastMCPEs().data(), sorted.data(), n_kept * sizeof(clsimhip_mcpe)) != 0 ||
        std::memcmp(conv.GetLastMergedMCPEs().data(), merged.data(), n_merged * sizeof(clsimhip_mcpe_merged)) != 0 ||
        std::memcmp(conv.GetLastMergedMCPESeries().data(), merged_series.data(), n_series * sizeof(clsimhip_mcpe_series)) != 0 ||
        std::memcmp(conv.GetLastMCPEParents().data(), parents.data(), n_parents * sizeof(clsimhip_mcpe_parent)) != 0 ||
        std::memcmp(conv.GetLastMCPEParentRanges().data(), ranges.data(), n_series * sizeof(clsimhip_mcpe_parent_range)) != 0) {
        std::printf("FAILED: %zu merged MCPEs and %zu parents from the adapter, %zu and %zu from the host twin (%zu records)\n", conv.GetLastMergedMCPEs().size(),
                    conv.GetLastMCPEParents().size(), n_merged, n_parents, n_kept);
        return 1;
    }
    // the frames' objects: every merged MCPE once, npe adding up to the records; every parent entry once, indices inside its DOM
    const std::map<uint32_t, I3CLSimStepToPhotonConverterHIP::MergedMCPESeriesMap> frames = conv.GetLastMergedMCPESeriesMaps();
    const std::map<uint32_t, I3CLSimStepToPhotonConverterHIP::ParticleIDMap> ids = conv.GetLastParticleIDMaps();
    size_t in_maps = 0, npe = 0, entries = 0;
    for (const auto &frame : frames)
        for (const auto &dom : frame.second) {
            in_maps += dom.second.size();
            for (const clsimhip_mcpe_merged &m : dom.second) npe += m.npe;
            const auto &particles_of = ids.at(frame.first).at(dom.first);
            for (const auto &particle : particles_of)
                for (size_t i = 0; i < particle.second.size(); ++i) {
                    ++entries;
                    if (particle.second[i] >= dom.second.size() || (i > 0 && particle.second[i] <= particle.second[i - 1])) { std::printf("FAILED: particle-ID map\n"); return 1; }
                }
        }
    if (frames.size() != 3 || ids.size() != 3 || in_maps != n_merged || npe != n_kept || entries != n_parents) { std::printf("FAILED: per-frame maps\n"); return 1; }
    std::printf("identifier %u photons %zu mcpes %zu series %zu merged %zu parents %zu frames %zu equal to the host twin\n", r.identifier, count, n_kept, n_series,
                n_merged, n_parents, frames.size());
    clsimhip_mcpe_generator_destroy(all);
    std::printf("mcpe merge adapter ok\n");
    return 0;
}
