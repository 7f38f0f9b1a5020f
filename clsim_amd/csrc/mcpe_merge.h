// MCPE merging: the series of one bunch -> per series, groups of records within a time window, one merged record per group, and
// the flattened particle-ID map (include/clsimhip.h: "MCPE merging").  The definition lives here ONCE, as predicates both the host
// twin (mcpe_merge.cpp) and the HIP kernels (mcpe_merge_kernel.hip) compile.  It stands where the reference's client module pushes
// every MCPE through MCHitMerging::MCPEStream and extracts the merged series with their I3ParticleIDMap
//   I3CLSimClientModule.h:193-194, I3CLSimClientModule.cxx:430, :710-719;  dom/I3PhotonToMCPEConverter.cxx:524-533
// but the stream class lies outside the reference and depends on insertion order: the rule below is this project's own, unpinned
// against the reference.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "mcpe_series.h"

namespace clsimhip {

#define MERGE_HD __host__ __device__ __forceinline__

// 0 <= window < +inf (NaN fails the first comparison)
MERGE_HD bool merge_window_ok(double window) { return window >= 0. && window < __builtin_inf(); }

MERGE_HD bool merge_is_finite(double t)
{
    return ((__builtin_bit_cast(uint64_t, t) >> 52) & 0x7ffu) != 0x7ffu;
}

// does a record at time t, behind a group whose opener has time T, open a group of its own?  One binary64 subtraction and one >:
// the rounded difference decides (a difference that overflows to +inf opens: window < +inf).
MERGE_HD bool merge_opens(double t, double T, double window)
{
    if (!merge_is_finite(t) || !merge_is_finite(T)) return true;
    return t - T > window;
}

// ---- the device stage (mcpe_merge_kernel.hip) ----
// words of the series stage's header (mcpe_series.h: SeriesHeader) the merge stage keeps its own sizes in; the sort passes and the
// tile scan it shares with the series stage read SH_KEPT and write SH_SERIES
enum MergeHeader : uint32_t { MH_SERIES = 48 /* entries of the series table */, MH_MERGED = 49, MH_PARENTS = 50 };

struct MergeDeviceArgs {
    const clsimhip_mcpe *in;                // the series stage's records, table and five counts
    const clsimhip_mcpe_series *series;
    const uint32_t *series_counts;          // records = min([0], capacity), series = min([1], capacity)
    uint32_t capacity;
    double window;
    uint32_t *header;                       // kSeriesHeaderWords, then the histogram (zeroed together)
    uint32_t *histogram;                    // 16 x 256
    uint32_t *tile_counts;                  // 256 x tiles(capacity)
    SeriesKey *keys[2];
    uint32_t *opens;                        // per record: 1 where it opens a group   (opens and owner are zeroed together)
    uint32_t *owner;                        // per record: its series
    uint32_t *group;                        // per record: its group, counted over the bunch
    uint32_t *position;                     // per group: its opener's record
    clsimhip_mcpe_merged *merged;
    clsimhip_mcpe_series *merged_series;
    clsimhip_mcpe_parent *parents;
    clsimhip_mcpe_parent_range *ranges;
    uint32_t *counts;                       // two: merged records, parent entries
};

// the host twin (mcpe_merge.cpp: host only, no HIP call); throws Error (CLSIMHIP_ERR_ARGUMENT) for a bad window or a table that does not partition the records
void mcpe_merge_host(const clsimhip_mcpe *records, size_t n, const clsimhip_mcpe_series *series, size_t n_series, double window,
                     clsimhip_mcpe_merged *out_merged, clsimhip_mcpe_series *out_series, clsimhip_mcpe_parent *out_parents,
                     clsimhip_mcpe_parent_range *out_ranges, size_t *n_merged, size_t *n_parents);

// mcpe_merge_kernel.hip: the workspace, and the stage on device memory -- checks the arguments, lays the workspace out and launches
// all kernels, asynchronous on `stream`
size_t mcpe_merge_workspace_bytes(size_t capacity);
void mcpe_merge_device(int device, const void *d_records, const void *d_series, const void *d_series_counts, size_t capacity, double window,
                       void *d_merged, void *d_merged_series, void *d_parents, void *d_ranges, void *d_counts, void *d_workspace,
                       size_t workspace_bytes, hipStream_t stream);

} // namespace clsimhip
