// I3MuonSlicerHIP.h through the C ABI, compiled with g++ (tests/test_muon_slicer_adapter.py).  Without arguments (host only): one muon
// of 30 m with three cascades is sliced, the MCPEs and frame photons its slices and cascades "produced" are relabelled, and so is a
// parent table.  `muon_slicer_adapter_test run` needs a GPU: the same series forms are relabelled in HBM and compared with the host's.
#include <dlfcn.h>

#include <cmath>
#include <cstdio>
#include <cstring>

#include "I3MuonSlicerHIP.h"

namespace {
const double kC = 0.299792458;

clsimhip_tree_particle node(uint32_t identifier, int32_t parent, int32_t type, double z, double energy, double length)
{
    clsimhip_tree_particle p;
    std::memset(&p, 0, sizeof p);
    p.particle.type = type;
    p.particle.z = z; p.particle.time = 10. + z / kC;
    p.particle.dz = 1.;
    p.particle.energy = energy; p.particle.length = length;
    p.particle.identifier = identifier;
    p.speed = kC; p.parent = parent;
    return p;
}

template <class Record>
Record record(uint32_t identifier, double time, float x = 0.f)
{
    Record r;
    std::memset(&r, 0, sizeof r);
    r.identifier = identifier; r.string_id = 21; r.om_id = 30; r.time = time;
    if (sizeof(Record) > sizeof(clsimhip_mcpe)) reinterpret_cast<float *>(&r)[7] = x;      // (a frame photon's x: distinct contents)
    return r;
}

// the HIP runtime the library already brought into the process
template <class F> F hip(const char *name) { return reinterpret_cast<F>(dlsym(RTLD_DEFAULT, name)); }

template <class Record>
bool on_device(const std::vector<clsimhip_relabel> &map, const std::vector<Record> &records, const std::vector<clsimhip_mcpe_series> &series,
               const std::vector<Record> &want)
{
    typedef int (*malloc_t)(void **, size_t);
    typedef int (*copy_t)(void *, const void *, size_t, int);
    typedef int (*free_t)(void *);
    typedef int (*sync_t)();
    malloc_t dmalloc = hip<malloc_t>("hipMalloc");
    copy_t dcopy = hip<copy_t>("hipMemcpy");
    free_t dfree = hip<free_t>("hipFree");
    sync_t dsync = hip<sync_t>("hipDeviceSynchronize");
    if (!dmalloc || !dcopy || !dfree || !dsync) { std::printf("FAILED: no HIP runtime in the process\n"); return false; }
    const size_t capacity = records.size() + 5, ws = I3MuonSlicerHIP::RelabelWorkspaceBytes(capacity, map.size(), sizeof(Record));
    void *d[7] = {nullptr};                                             // records, series, counts, out records, out series, out counts, workspace
    const size_t bytes[7] = {capacity * sizeof(Record), capacity * 16, 20, capacity * sizeof(Record), capacity * 16, 20, ws};
    for (int k = 0; k < 7; ++k)
        if (dmalloc(&d[k], bytes[k]) != 0) { std::printf("FAILED: hipMalloc\n"); return false; }
    const uint32_t counts[5] = {static_cast<uint32_t>(records.size()), static_cast<uint32_t>(series.size()), 0, 0, 0};
    bool ok = dcopy(d[0], records.data(), records.size() * sizeof(Record), 1) == 0 && dcopy(d[1], series.data(), series.size() * 16, 1) == 0 &&
              dcopy(d[2], counts, 20, 1) == 0;
    I3MuonSlicerHIP::RelabelSlicesDevice(map, sizeof(Record), 0, d[0], d[1], d[2], capacity, d[3], d[4], d[5], d[6], ws);
    ok = ok && dsync() == 0;
    std::vector<Record> got(records.size());
    std::vector<clsimhip_mcpe_series> table(series.size());
    uint32_t out_counts[5] = {9, 9, 9, 9, 9};
    ok = ok && dcopy(got.data(), d[3], got.size() * sizeof(Record), 2) == 0 && dcopy(table.data(), d[4], table.size() * 16, 2) == 0 && dcopy(out_counts, d[5], 20, 2) == 0;
    for (int k = 0; k < 7; ++k) dfree(d[k]);
    return ok && out_counts[0] == records.size() && out_counts[1] == series.size() && out_counts[3] == 0 && out_counts[4] == 0 &&
           std::memcmp(got.data(), want.data(), got.size() * sizeof(Record)) == 0 && std::memcmp(table.data(), series.data(), table.size() * 16) == 0;
}
} // namespace

int main(int argc, char **argv)
{
    const bool run = argc > 1 && std::strcmp(argv[1], "run") == 0;
    // a muon of 30 m with losses at 5, 12 and 20 m below a neutrino
    std::vector<clsimhip_tree_particle> tree;
    tree.push_back(node(1, -1, 14, 0., 500., NAN));
    tree.push_back(node(2, 0, CLSIMHIP_PARTICLE_MUMINUS, 0., 200., 30.));
    tree.push_back(node(3, 1, CLSIMHIP_PARTICLE_BREMS, 5., 2., NAN));
    tree.push_back(node(4, 1, CLSIMHIP_PARTICLE_PAIRPROD, 12., 5., NAN));
    tree.push_back(node(5, 1, CLSIMHIP_PARTICLE_DELTAE, 20., 1., NAN));
    const clsimhip_mmc_track track = {2u, 0u, 200., 150., 10., 10. + 30. / kC};
    std::vector<clsimhip_tree_particle> sliced;
    std::vector<clsimhip_relabel> relabel;
    uint64_t counters[5];
    I3MuonSlicerHIP::SliceMuons(tree, std::vector<clsimhip_mmc_track>(1, track), 100u, sliced, relabel, counters);
    const std::vector<clsimhip_particle> sources = I3MuonSlicerHIP::LightSources(sliced);
    bool ok = sliced.size() == 9 && relabel.size() == 4 && sources.size() == 8 && (sliced[1].flags & CLSIMHIP_TREE_DARK) && sliced[2].particle.identifier == 100u &&
              sliced[8].particle.identifier == 103u && sliced[8].particle.energy < 200. && sliced[8].particle.energy > 150.;
    for (const clsimhip_relabel &r : relabel) ok = ok && r.to == 2u;
    for (int k = 0; k < 5; ++k) ok = ok && counters[k] == 0;
    bool refused = false;
    try {
        I3MuonSlicerHIP::SliceMuons(tree, std::vector<clsimhip_mmc_track>(2, track), 100u, sliced, relabel);
    } catch (const I3CLSimStepToPhotonConverter_exception &e) {
        refused = std::strstr(e.what(), "more than once") != nullptr;
    }
    ok = ok && refused && sliced.size() == 9;
    // what slices and cascades produced at one DOM: equal times under 3 (a cascade), 100 and 102 (slices), so the map disturbs the run
    std::vector<clsimhip_mcpe> mcpes;
    std::vector<clsimhip_frame_photon> photons;
    const uint32_t ids[6] = {100u, 3u, 100u, 102u, 4u, 103u};
    const double times[6] = {50., 60., 60., 60., 70., 70.};
    for (int k = 0; k < 6; ++k) {
        mcpes.push_back(record<clsimhip_mcpe>(ids[k], times[k]));
        photons.push_back(record<clsimhip_frame_photon>(ids[k], times[k], 1.f));
    }
    const std::vector<clsimhip_mcpe_series> series(1, clsimhip_mcpe_series{7u, 21, 30, 0u, 6u});
    const std::vector<clsimhip_mcpe> mcpes_in = mcpes;
    const std::vector<clsimhip_frame_photon> photons_in = photons;
    const uint64_t moved = I3MuonSlicerHIP::RelabelSlices(relabel, mcpes, series);
    const uint64_t moved_photons = I3MuonSlicerHIP::RelabelSlices(relabel, photons, series);
    const uint32_t want[6] = {2u, 2u, 2u, 3u, 2u, 4u};
    for (int k = 0; k < 6; ++k) ok = ok && mcpes[k].identifier == want[k] && photons[k].identifier == want[k];
    ok = ok && moved == 4 && moved_photons == 4;
    std::vector<clsimhip_mcpe_parent> parents = {{3u, 0u}, {100u, 0u}, {100u, 1u}, {102u, 1u}, {4u, 0u}};
    std::vector<clsimhip_mcpe_parent_range> ranges = {{0u, 4u}, {4u, 1u}};
    I3MuonSlicerHIP::RelabelSlices(relabel, parents, ranges);
    ok = ok && parents.size() == 4 && parents[0].identifier == 2u && parents[1].identifier == 2u && parents[1].index == 1u && parents[2].identifier == 3u &&
         ranges[0].count == 3 && ranges[1].first == 3 && ranges[1].count == 1;
    if (!ok) { std::printf("FAILED: host path\n"); return 1; }
    std::printf("sliced: 5 nodes -> %zu nodes, %zu slices, %zu light sources; relabelled %llu of 6 mcpes and %llu of 6 photons, %zu parents\n", sliced.size(),
                relabel.size(), sources.size(), static_cast<unsigned long long>(moved), static_cast<unsigned long long>(moved_photons), parents.size());
    if (!run) { std::printf("muon slicer adapter ok (no GPU run requested)\n"); return 0; }
    if (!on_device(relabel, mcpes_in, series, mcpes) || !on_device(relabel, photons_in, series, photons)) { std::printf("FAILED: device path\n"); return 1; }
    std::printf("device: 6 mcpes and 6 photons relabelled in HBM equal to the host twin\n");
    std::printf("muon slicer adapter ok\n");
    return 0;
}
