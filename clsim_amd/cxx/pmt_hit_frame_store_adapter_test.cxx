// The PMT hit frame store through the C++ adapter (I3PMTHitFrameStoreHIP.h).  `pmt_hit_frame_store_adapter_test` alone builds a host
// store, adds three small bunches and drains them in two steps (host only); `pmt_hit_frame_store_adapter_test run` needs a GPU: a
// converter with the PMT hit generator and the PMT series stage on and keep_photons = 0 (homogeneous ice, single string, a 12-PMT
// module at every DOM), three bunches of 1024 steps dealt to 16 particles in three frames, every result added to a device store and
// to a host store, and both compared with the twin's union of the results.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "I3PMTHitFrameStoreHIP.h"

namespace {
typedef std::vector<clsimhip_pmt_hit> Records;
typedef std::vector<clsimhip_pmt_series> Table;
struct Where { uint32_t frame; unsigned om; uint32_t pmt; };

// one record per (frame, om, pmt) given, at string 1, as a series form
void small_bunch(const std::vector<Where> &where, uint32_t identifier, double time, Records &records, Table &table)
{
    records.clear(); table.clear();
    for (size_t k = 0; k < where.size(); ++k) {                        // (given ascending in (frame, om, pmt))
        clsimhip_pmt_hit h = {identifier, 1, static_cast<uint16_t>(where[k].om), where[k].pmt, 0u, time + k};
        clsimhip_pmt_series s = {where[k].frame, 1, static_cast<uint16_t>(where[k].om), where[k].pmt, static_cast<uint32_t>(k), 1u, 0u};
        records.push_back(h);
        table.push_back(s);
    }
}

size_t count(const std::map<uint32_t, I3PMTHitFrameStoreHIP::PMTHitSeriesMap> &frames)
{
    size_t n = 0;
    for (const auto &frame : frames)
        for (const auto &module : frame.second)
            for (const auto &pmt : module.second) n += pmt.second.size();
    return n;
}
} // namespace

static int host_store()
{
    I3PMTHitFrameStoreHIP store(64);
    Records records; Table table;
    small_bunch({{3u, 5u, 2u}, {3u, 5u, 11u}, {9u, 5u, 2u}}, 70u, 100., records, table);
    store.Add(records, table);
    small_bunch({{3u, 5u, 2u}, {4u, 2u, 0u}}, 71u, 50., records, table);
    store.Add(records, table);
    small_bunch({{3u, 5u, 11u}, {9u, 5u, 2u}, {9u, 5u, 3u}}, 72u, 100., records, table);
    store.Add(records, table);
    if (store.Size() != std::make_pair(size_t(8), size_t(5)) || store.Size(4u) != std::make_pair(size_t(5), size_t(3))) { std::printf("FAILED: sizes\n"); return 1; }
    // a bunch that is no series form is refused and changes nothing: two PMTs of one module in descending order
    bool refused = false;
    small_bunch({{3u, 5u, 11u}, {3u, 5u, 2u}}, 73u, 1., records, table);
    try { store.Add(records, table); } catch (const I3CLSimStepToPhotonConverter_exception &e) { refused = std::strstr(e.what(), "no series form: entry 1 of 2") != nullptr; }
    if (!refused || store.Size().first != 8) { std::printf("FAILED: a malformed bunch was taken\n"); return 1; }
    // ... and a record with a reserved word set
    small_bunch({{3u, 5u, 2u}}, 73u, 1., records, table);
    records[0].reserved = 1u;
    refused = false;
    try { store.Add(records, table); } catch (const I3CLSimStepToPhotonConverter_exception &e) { refused = std::strstr(e.what(), "no series form: record 0 of 1") != nullptr; }
    if (!refused || store.Size().first != 8) { std::printf("FAILED: a record with reserved != 0 was taken\n"); return 1; }
    const std::map<uint32_t, I3PMTHitFrameStoreHIP::PMTHitSeriesMap> early = store.Drain(4u);
    const std::vector<clsimhip_pmt_hit> &first = early.at(3u).at(std::make_pair(1, 5u)).at(2u);
    if (early.size() != 2 || count(early) != 5 || first.size() != 2 || first[0].identifier != 71u || first[0].time != 50. || first[1].identifier != 70u ||
        early.at(3u).at(std::make_pair(1, 5u)).size() != 2 || early.at(3u).at(std::make_pair(1, 5u)).at(11u).size() != 2 || early.at(4u).size() != 1) {
        std::printf("FAILED: the early frames\n");
        return 1;
    }
    const std::map<uint32_t, I3PMTHitFrameStoreHIP::PMTHitSeriesMap> late = store.Drain();
    const std::vector<clsimhip_pmt_hit> &both = late.at(9u).at(std::make_pair(1, 5u)).at(2u);      // times 101 (72) and 102 (70)
    if (late.size() != 1 || late.at(9u).size() != 1 || late.at(9u).at(std::make_pair(1, 5u)).size() != 2 || both.size() != 2 || both[0].identifier != 72u ||
        both[0].time != 101. || both[1].time != 102. || count(late) != 3 || store.Size().first != 0) { std::printf("FAILED: the late frames\n"); return 1; }
    std::printf("host store: 3 bunches 8 hits 5 series, frames <= 4 gave 5 hits in 2 frames, the rest 3 hits on 2 PMTs of one module\n");
    return 0;
}

int main(int argc, char **argv)
{
    const bool run = argc > 1 && std::strcmp(argv[1], "run") == 0;
    if (host_store() != 0) return 1;
    if (!run) { std::printf("pmt hit frame store adapter ok (no GPU run requested)\n"); return 0; }

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

    // the hit maker of pmt_series_adapter_test.cxx: twelve PMTs on a Fibonacci sphere, discs of 0.3 R at 0.85 R; every module turned about z
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
    clsimhip_pmt_generator *all = nullptr;
    if (clsimhip_pmt_generator_create(functions, 3, &type, 1, pmts.data(), 12, modules.data(), 60, 2024, &all) != CLSIMHIP_OK) {
        std::printf("generator: %s\n", clsimhip_pmt_generator_last_error(nullptr));
        return 1;
    }
    conv.SetWlenGenerators(std::vector<clsimhip_random_value>(1, gen));
    conv.SetWlenBias(bias);
    conv.SetMediumProperties(medium);
    conv.SetGeometry(sid, did, x, yy, z, sub, 0.16510 * 5.);
    conv.SetStopDetectedPhotons(true);
    conv.SetDOMPancakeFactor(5.);
    conv.SetPMTHitGenerator(all, false);                                // keep_photons = 0: the store is what joins the bunches
    conv.SetPMTSeries(true);
    conv.Compile();
    conv.SetWorkgroupSize(conv.GetMaxWorkgroupSize());
    conv.SetMaxNumWorkitems(1024);
    clsimhip_medium_destroy(medium);
    conv.Initialize();

    const uint32_t frame_ids[3] = {90u, 3u, 41u};
    std::vector<clsimhip_mcpe_particle> particles;
    for (uint32_t k = 0; k < 16; ++k) { clsimhip_mcpe_particle p = {500u + k, frame_ids[k % 3], 1000. * (k % 4) - 0.5}; particles.push_back(p); }
    I3PMTHitFrameStoreHIP on_device(1u << 16, 0), on_host(1u << 16);
    Records twin; Table twin_table;
    size_t added = 0;
    for (uint32_t bunch = 0; bunch < 3; ++bunch) {
        std::shared_ptr<I3CLSimStepSeries> steps(new I3CLSimStepSeries(1024));
        for (size_t i = 0; i < steps->size(); ++i) {
            I3CLSimStep &s = (*steps)[i];
            std::memset(&s, 0, sizeof s);
            s.theta = static_cast<float>(std::acos(1. - 2. * ((i * 37 + bunch) % 1024) / 1024.));
            s.phi = static_cast<float>(6.283185307 * ((i * 101) % 1024) / 1024.);
            s.length = 0.001f; s.beta = 1.f; s.num_photons = (i < 1000) ? 200 : 0; s.weight = 1.f; s.identifier = 500u + static_cast<uint32_t>(i % 16);
        }
        conv.EnqueueSteps(steps, 42 + bunch, particles);
        conv.GetConversionResult();
        const Records &records = conv.GetLastPMTHits();
        const Table &table = conv.GetLastPMTSeries();
        on_device.Add(records, table);
        on_host.Add(records, table);
        Records out(twin.size() + records.size());
        Table out_table(out.size());
        size_t made = 0, entries = 0;
        if (clsimhip_pmt_hits_union_host(twin.data(), twin.size(), twin_table.data(), twin_table.size(), records.data(), records.size(), table.data(), table.size(),
                                         out.data(), out_table.data(), out.size(), &made, &entries) != CLSIMHIP_OK) {
            std::printf("host twin: %s\n", clsimhip_last_error(nullptr));
            return 1;
        }
        out_table.resize(entries);
        twin.swap(out);
        twin_table.swap(out_table);
        added += records.size();
    }
    if (twin.size() != added || added == 0 || on_device.Size() != std::make_pair(twin.size(), twin_table.size()) || on_host.Size() != on_device.Size()) {
        std::printf("FAILED: %zu records added, %zu in the twin, %zu in the device store\n", added, twin.size(), on_device.Size().first);
        return 1;
    }
    // frames 3 and 41 leave, frame 90 stays: flat from the device store, as maps from the host store
    Records head; Table head_table;
    on_device.DrainFlat(41u, head, head_table);
    const size_t n_head = head.size();
    if (n_head == 0 || n_head >= added || std::memcmp(head.data(), twin.data(), n_head * sizeof(clsimhip_pmt_hit)) != 0 ||
        std::memcmp(head_table.data(), twin_table.data(), head_table.size() * sizeof(clsimhip_pmt_series)) != 0 || head_table.back().frame != 41u ||
        twin_table[head_table.size()].frame != 90u) { std::printf("FAILED: the head of the device store\n"); return 1; }
    const std::map<uint32_t, I3PMTHitFrameStoreHIP::PMTHitSeriesMap> frames = on_host.Drain(41u);
    if (frames.size() != 2 || count(frames) != n_head) { std::printf("FAILED: the head of the host store\n"); return 1; }
    Records tail; Table tail_table;
    on_device.DrainFlat(I3PMTHitFrameStoreHIP::AllFrames, tail, tail_table);
    if (tail.size() != added - n_head || std::memcmp(tail.data(), twin.data() + n_head, tail.size() * sizeof(clsimhip_pmt_hit)) != 0 || tail_table.front().first != 0u ||
        on_device.Size().first != 0) { std::printf("FAILED: the tail of the device store\n"); return 1; }
    const std::map<uint32_t, I3PMTHitFrameStoreHIP::PMTHitSeriesMap> rest = on_host.Drain();
    if (rest.size() != 1 || !rest.count(90u) || count(rest) != tail.size()) { std::printf("FAILED: the tail of the host store\n"); return 1; }
    std::printf("bunches 3 hits %zu series %zu head %zu tail %zu equal to the host twin\n", added, twin_table.size(), n_head, tail.size());
    clsimhip_pmt_generator_destroy(all);
    std::printf("pmt hit frame store adapter ok\n");
    return 0;
}
