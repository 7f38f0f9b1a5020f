// The muon slicer and the relabelling of what its slices produced (include/clsimhip.h, "Muon slicer" and "Series relabel") for a C++
// client: what stands where the reference's standard chain runs I3MuonSlicer in front of the light source converter and
// I3MuonSliceRemoverAndPulseRelabeler behind the hit makers (python/traysegments/I3CLSimMakePhotons.py).  Header-only over the C ABI.
//
//   I3MuonSlicerHIP::SliceMuons(tree, tracks, firstSliceIdentifier, sliced, relabel);      // per frame, in front of clsimhip_ppc_enqueue
//   ... propagate the nodes of `sliced` without CLSIMHIP_TREE_DARK; particle table: slices with their muon's frame and shift ...
//   I3MuonSlicerHIP::RelabelSlices(relabel, records, series);                              // per drain, in front of the merging stage
#ifndef I3MUONSLICERHIP_H_INCLUDED
#define I3MUONSLICERHIP_H_INCLUDED

#include <cstdint>
#include <string>
#include <vector>

#include "I3CLSimStepToPhotonConverterHIP.h"

class I3MuonSlicerHIP {
public:
    // I3MuonSlicer on a flattened tree in depth-first pre-order; counters (may be null): the five CLSIMHIP_SLICER_* counts
    static void SliceMuons(const std::vector<clsimhip_tree_particle> &tree, const std::vector<clsimhip_mmc_track> &tracks, uint32_t firstSliceIdentifier,
                           std::vector<clsimhip_tree_particle> &sliced, std::vector<clsimhip_relabel> &relabel, uint64_t *counters = nullptr)
    {
        size_t n = 0, nRelabel = 0;
        check(clsimhip_slice_muons(tree.data(), tree.size(), tracks.data(), tracks.size(), firstSliceIdentifier, nullptr, 0, &n, nullptr, 0, &nRelabel, nullptr));
        sliced.resize(n);
        relabel.resize(nRelabel);
        check(clsimhip_slice_muons(tree.data(), tree.size(), tracks.data(), tracks.size(), firstSliceIdentifier, sliced.data(), sliced.size(), &n, relabel.data(),
                                   relabel.size(), &nRelabel, counters));
    }
    // what clsimhip_ppc_enqueue takes: the nodes that are not dark
    static std::vector<clsimhip_particle> LightSources(const std::vector<clsimhip_tree_particle> &sliced)
    {
        std::vector<clsimhip_particle> out;
        for (const clsimhip_tree_particle &p : sliced)
            if (!(p.flags & CLSIMHIP_TREE_DARK)) out.push_back(p.particle);
        return out;
    }

    // RELABEL of a series form, in place (the table is unchanged); returns the number of records that took a new identifier.  A
    // TIE_OVERFLOW throws: nothing would have been delivered.
    static uint64_t RelabelSlices(const std::vector<clsimhip_relabel> &map, std::vector<clsimhip_mcpe> &records, const std::vector<clsimhip_mcpe_series> &series)
    {
        std::vector<clsimhip_mcpe> out(records.size());
        uint64_t counters[2] = {0, 0};
        size_t kept = 0;
        check(clsimhip_mcpe_series_relabel_host(records.data(), records.size(), series.data(), series.size(), map.data(), map.size(), out.data(), counters, &kept));
        overflow(counters);
        records.swap(out);
        return counters[CLSIMHIP_RELABEL_RELABELLED];
    }
    static uint64_t RelabelSlices(const std::vector<clsimhip_relabel> &map, std::vector<clsimhip_frame_photon> &records, const std::vector<clsimhip_mcpe_series> &series)
    {
        std::vector<clsimhip_frame_photon> out(records.size());
        uint64_t counters[2] = {0, 0};
        size_t kept = 0;
        check(clsimhip_frame_photons_relabel_host(records.data(), records.size(), series.data(), series.size(), map.data(), map.size(), out.data(), counters, &kept));
        overflow(counters);
        records.swap(out);
        return counters[CLSIMHIP_RELABEL_RELABELLED];
    }
    // ... of the merging stage's parent table, in place
    static void RelabelSlices(const std::vector<clsimhip_relabel> &map, std::vector<clsimhip_mcpe_parent> &parents, std::vector<clsimhip_mcpe_parent_range> &ranges)
    {
        std::vector<clsimhip_mcpe_parent> out(parents.size());
        std::vector<clsimhip_mcpe_parent_range> outRanges(ranges.size());
        size_t n = 0;
        check(clsimhip_mcpe_parents_relabel_host(parents.data(), ranges.data(), ranges.size(), map.data(), map.size(), out.data(), outRanges.data(), &n));
        out.resize(n);
        parents.swap(out);
        ranges.swap(outRanges);
    }
    // ... of series forms that live in HBM (asynchronous on hipStream; dOutCounts: five uint32 -- records, series, RELABELLED, 0,
    // TIE_OVERFLOW); recordBytes: sizeof(clsimhip_mcpe) or sizeof(clsimhip_frame_photon)
    static size_t RelabelWorkspaceBytes(size_t capacity, size_t mapSize, size_t recordBytes) { return clsimhip_series_relabel_workspace_bytes(capacity, mapSize, recordBytes); }
    static void RelabelSlicesDevice(const std::vector<clsimhip_relabel> &map, size_t recordBytes, int device, const void *dRecords, const void *dSeries,
                                    const void *dCounts, size_t capacity, void *dOutRecords, void *dOutSeries, void *dOutCounts, void *dWorkspace, size_t workspaceBytes,
                                    void *hipStream = nullptr)
    {
        if (recordBytes == sizeof(clsimhip_mcpe))
            check(clsimhip_mcpe_series_relabel_device(device, dRecords, dSeries, dCounts, capacity, map.data(), map.size(), dOutRecords, dOutSeries, dOutCounts,
                                                      dWorkspace, workspaceBytes, hipStream));
        else if (recordBytes == sizeof(clsimhip_frame_photon))
            check(clsimhip_frame_photons_relabel_device(device, dRecords, dSeries, dCounts, capacity, map.data(), map.size(), dOutRecords, dOutSeries, dOutCounts,
                                                        dWorkspace, workspaceBytes, hipStream));
        else
            throw I3CLSimStepToPhotonConverter_exception("RelabelSlicesDevice: recordBytes is neither an MCPE's nor a frame photon's");
    }

private:
    static void check(int rc)
    {
        if (rc != CLSIMHIP_OK) throw I3CLSimStepToPhotonConverter_exception(clsimhip_last_error(nullptr));
    }
    static void overflow(const uint64_t counters[2])
    {
        if (counters[CLSIMHIP_RELABEL_TIE_OVERFLOW])
            throw I3CLSimStepToPhotonConverter_exception("series relabel: TIE_OVERFLOW = " + std::to_string(counters[CLSIMHIP_RELABEL_TIE_OVERFLOW]) + ", nothing is delivered");
    }
};

#endif
