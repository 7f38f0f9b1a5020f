// Series relabel: the records of a series form take new identifiers from a map, and the form's order is restored
// (include/clsimhip.h: "Series relabel").  The definition lives here ONCE, as functions both the host twins (series_relabel.cpp) and
// the HIP kernels (series_relabel_kernel.hip) compile.  It stands where the reference replaces, behind its hit makers, every slice's
// identifier by that of the muon it was cut from
//   I3MuonSliceRemoverAndPulseRelabeler::DAQ   private/clsim/util/I3MuonSliceRemoverAndPulseRelabeler.cxx:230-400
//                                              (the sanity check on the map :320-332, the MCPEs :336-352, the photons :388-400)
// and pays what the reference does not: the series forms end their key in the identifier, so the order has to be made again.
// Only runs of records equal in (series entry, tkey) can be out of order; a run is DISTURBED when its new identifiers descend somewhere.
// Undisturbed runs are copied whatever their length; a disturbed run of at most kRelabelRunBound records is sorted on the rest of the
// key; a longer one is counted member by member as TIE_OVERFLOW and the call delivers nothing.
//
// The parent table of the merging stage needs no device stage of its own: merging ignores particles, so on the device it comes
// from running the existing merge stage BEHIND the relabel stage.  parents_relabel_host is for tables that were made before.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "frame_photon_union.h"
#include "mcpe_union.h"

namespace clsimhip {

constexpr uint32_t kRelabelRunBound = 2048u;                            // the frame photons stage's bound on tie work
constexpr uint32_t kRelabelPivots = 256u;                               // the map's upper levels, held in LDS by the kernel

// ---- a record type: its words, and what of the key lies behind (entry, tkey) ----
// MCPE: 4 words -- identifier, string ID | OM ID << 16, the time's bit pattern; the rest of the key is the identifier
struct RelabelMcpe {
    using Record = clsimhip_mcpe;
    static constexpr uint32_t kWords = 4u;
    // a before b in the rest of the key (identifiers given, the other words from the records)
    static UNION_HD bool rest_less(uint32_t id_a, const uint32_t *, uint32_t id_b, const uint32_t *) { return id_a < id_b; }
};
// frame photon: 12 words -- identifier, string ID | OM ID << 16, time, w0 ... w7; the rest of the key is identifier, h, w0 ... w7
struct RelabelFramePhoton {
    using Record = clsimhip_frame_photon;
    static constexpr uint32_t kWords = kFramePhotonRecordWords;
    static UNION_HD bool rest_less(uint32_t id_a, const uint32_t *a, uint32_t id_b, const uint32_t *b)
    {
        if (id_a != id_b) return id_a < id_b;
        FramePhotonContent ca, cb;
        frame_photon_union_content(a, ca);
        frame_photon_union_content(b, cb);
        const uint32_t ha = frame_photons_mix(ca), hb = frame_photons_mix(cb);
        if (ha != hb) return ha < hb;
        return frame_photons_compare(ca, cb) < 0;
    }
};

// the time's bit pattern as the forms' total order (mcpe_series.h: series_tkey, on the bits)
UNION_HD uint64_t relabel_tkey(const uint32_t *rec) { return frame_photon_union_tkey((uint64_t)rec[2] | ((uint64_t)rec[3] << 32)); }

// index of `identifier` among map[lo, hi), ascending in `from`; -1: not there
UNION_HD int64_t relabel_find(const clsimhip_relabel *map, uint32_t lo, uint32_t hi, uint32_t identifier)
{
    const uint32_t end = hi;
    while (lo < hi) {                                                   // first entry with from >= identifier
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (map[mid].from < identifier) lo = mid + 1u; else hi = mid;
    }
    return (lo < end && map[lo].from == identifier) ? (int64_t)lo : -1;
}

// record i opens a run: it is the first of all, or of its entry, or differs from its predecessor in the time key.  (Records of one
// entry carry one DOM word, so a DOM word that differs is an entry that differs; only for equal words is the table looked into.)
UNION_HD bool relabel_is_head(const uint32_t *rec, const uint32_t *before, const clsimhip_mcpe_series *series, uint32_t n_series, uint32_t i)
{
    if (i == 0u) return true;
    if (rec[2] != before[2] || rec[3] != before[3] || rec[1] != before[1]) return true;
    const int64_t s = union_entry_of(series, n_series, i);
    return s >= 0 && series[s].first == i;
}

// ---- the host twins (series_relabel.cpp: host only, no HIP call); they throw Error (CLSIMHIP_ERR_ARGUMENT) ----
void relabel_map_check(const clsimhip_relabel *map, size_t n_map);
void mcpe_series_relabel_host(const clsimhip_mcpe *records, size_t n, const clsimhip_mcpe_series *series, size_t n_series, const clsimhip_relabel *map, size_t n_map,
                              clsimhip_mcpe *out_records, uint64_t counters[2], size_t *n_kept);
void frame_photons_relabel_host(const clsimhip_frame_photon *records, size_t n, const clsimhip_mcpe_series *series, size_t n_series, const clsimhip_relabel *map,
                                size_t n_map, clsimhip_frame_photon *out_records, uint64_t counters[2], size_t *n_kept);
void mcpe_parents_relabel_host(const clsimhip_mcpe_parent *parents, const clsimhip_mcpe_parent_range *ranges, size_t n_series, const clsimhip_relabel *map, size_t n_map,
                               clsimhip_mcpe_parent *out, clsimhip_mcpe_parent_range *out_ranges, size_t *n_out);

// ---- the device stage (series_relabel_kernel.hip) ----
// header words beside mcpe_series.h's SH_KEPT (the records) and SH_SERIES (the tile scan's total: the runs)
enum RelabelHeader : uint32_t { RH_RELABELLED = 2, RH_TIE_OVERFLOW = 4, RH_DESCENTS = 40, RH_N_SERIES = 41 };

template <class T>
struct RelabelDeviceArgs {
    const typename T::Record *records;
    const clsimhip_mcpe_series *series;
    const uint32_t *counts;                 // records = min([0], capacity), series = min([1], capacity)
    uint32_t capacity;
    const clsimhip_relabel *map;            // in the workspace
    uint32_t n_map, pivot_stride;           // pivot k = map[k x pivot_stride].from
    uint32_t *header;                       // kSeriesHeaderWords
    uint32_t *tile_counts;                  // run heads per tile, scanned in place
    uint32_t *run_first;                    // by run: its first record
    uint32_t *run_disturbed;                // by run: nonzero when its new identifiers descend somewhere
    typename T::Record *out_records;
    clsimhip_mcpe_series *out_series;
    uint32_t *out_counts;                   // five: records, series, RELABELLED, 0, TIE_OVERFLOW
};

size_t series_relabel_workspace_bytes(size_t capacity, size_t n_map, size_t record_bytes);
void mcpe_series_relabel_device(int device, const void *d_records, const void *d_series, const void *d_counts, size_t capacity, const clsimhip_relabel *map, size_t n_map,
                                void *d_out_records, void *d_out_series, void *d_out_counts, void *d_workspace, size_t workspace_bytes, hipStream_t stream);
void frame_photons_relabel_device(int device, const void *d_records, const void *d_series, const void *d_counts, size_t capacity, const clsimhip_relabel *map, size_t n_map,
                                  void *d_out_records, void *d_out_series, void *d_out_counts, void *d_workspace, size_t workspace_bytes, hipStream_t stream);

} // namespace clsimhip
