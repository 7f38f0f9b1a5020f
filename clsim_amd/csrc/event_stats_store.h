// Event statistics frame store: per frame and per particle, the exact sums of the event statistics records of bunch after bunch, with a
// relabel map folding slices into their muon (include/clsimhip.h: "Event statistics frame store").  It stands where the reference's
// client module keeps one I3CLSimEventStatistics per frame across bunches and files it when the frame is flushed
//   I3CLSimClientModule::DigestOtherFrame / AddPhotonsToFrames   private/clsim/I3CLSimClientModule.cxx:513-520, 386-405
//   I3CLSimClientModule::FlushFrameCache                         :686-758  (the statistics into the frame :728-740)
// and where I3MuonSliceRemoverAndPulseRelabeler (private/clsim/util/I3MuonSliceRemoverAndPulseRelabeler.cxx:230-400) gives a slice's
// light to its muon.  The definition lives here ONCE, as functions both the host twins (event_stats_store.cpp) and the HIP kernels
// (event_stats_store_kernel.hip) compile.  A record is a key (frame, identifier) and 136 bytes of integers that ADD (event_stats.h)
// adds exactly; ADD is associative and commutative, so CANON of a list is a function of the list as a multiset, and the store's
// content does not depend on the order the bunches arrive in.  There is no table and no tie: series_union.h's traits contract is not
// used here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <memory>

#include "event_stats.h"
#include "series_relabel.h"
#include "series_union.h"

namespace clsimhip {

// a record as words: 36 uint32 -- 0 identifier, 1 frame, 2-3 generated_count, 4-5 at_doms_count, 6-17 the limbs of generated_sum,
// 18-29 those of at_doms_sum, 30-35 the six special counters -- or nine 16-byte quarters
constexpr uint32_t kEventStatsRecordWords = 36u, kEventStatsRecordQuads = 9u;
static_assert(sizeof(clsimhip_event_statistics) == 4u * kEventStatsRecordWords, "a record is its words");
// records per workgroup in the tiled kernels (256 lanes x 8): the one tile size of the stage
constexpr uint32_t kEventStatsStoreTile = 2048u;
// a run of this many records or more is summed by a whole wave, a shorter one by one lane
constexpr uint32_t kEventStatsLongRun = 16u;

// THE key: (frame, identifier) as one integer, frame first
SERIES_HD uint64_t event_stats_store_key(uint32_t identifier, uint32_t frame) { return ((uint64_t)frame << 32) | identifier; }
SERIES_HD uint64_t event_stats_store_key(const clsimhip_event_statistics &r) { return event_stats_store_key(r.identifier, r.frame); }
SERIES_HD uint32_t event_stats_store_key_frame(uint64_t key) { return (uint32_t)(key >> 32); }

// EMPTY: the 136 bytes behind identifier and frame are all zero
SERIES_HD bool event_stats_store_words_empty(const uint32_t w[kEventStatsRecordWords])
{
    uint32_t any = 0u;
#pragma unroll
    for (uint32_t k = 2; k < kEventStatsRecordWords; ++k) any |= w[k];
    return any == 0u;
}

// the identifier behind the map (ascending in `from`; series_relabel.h: relabel_find)
SERIES_HD uint32_t event_stats_store_relabel(const clsimhip_relabel *map, uint32_t n_map, uint32_t identifier, bool *hit)
{
    const int64_t k = relabel_find(map, 0u, n_map, identifier);
    *hit = k >= 0;
    return k >= 0 ? map[k].to : identifier;
}

// SPLIT: the records with frame <= last_frame, a prefix of a form ascending in the key; at most 32 trips whatever the keys hold.
// `key_at(i)`: the key of record i.
template <class KeyAt>
SERIES_HD uint32_t event_stats_store_split_point(KeyAt key_at, uint32_t n, uint32_t last_frame)
{
    uint32_t lo = 0u, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (event_stats_store_key_frame(key_at(mid)) <= last_frame) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// ---- the host twins (event_stats_store.cpp: host only, no HIP call); they throw Error (CLSIMHIP_ERR_ARGUMENT) and write nothing then ----
// what is wrong with a statistics form: throws, with text that names the first offending element (`what`: "A", "B" ...)
void event_stats_form_check(const char *what, const clsimhip_event_statistics *records, size_t n);
void event_stats_canonical_host(const clsimhip_event_statistics *records, size_t n, const clsimhip_relabel *map, size_t n_map, clsimhip_event_statistics *out,
                                size_t capacity, size_t *n_out, uint64_t counters[2]);
void event_stats_combine_host(const clsimhip_event_statistics *a, size_t n_a, const clsimhip_event_statistics *b, size_t n_b, clsimhip_event_statistics *out,
                              size_t capacity, size_t *n_out);
void event_stats_split_host(const clsimhip_event_statistics *records, size_t n, uint32_t last_frame, clsimhip_event_statistics *head, size_t head_capacity,
                            size_t *n_head, clsimhip_event_statistics *tail, size_t tail_capacity, size_t *n_tail);

// ---- the device stages (event_stats_store_kernel.hip) ----
// output counts (five uint32, the frame stores' layout): records, 0, RELABELLED / MALFORMED in A, EMPTY_DROPPED / MALFORMED in B, overflow
enum EventStatsStoreCounts : uint32_t { ESC_RECORDS = 0, ESC_RELABELLED = 2, ESC_EMPTY_DROPPED = 3, ESC_MALFORMED_A = 2, ESC_MALFORMED_B = 3, ESC_OVERFLOW = 4 };
// one size for the three stages: CANON of `capacity` records with a map of n_map entries needs (capacity, n_map), COMBINE (capacity_a, capacity_b)
size_t event_stats_store_workspace_bytes(size_t capacity_a, size_t capacity_b);
void event_stats_canonical_device(int device, const void *d_records, const void *d_count, size_t capacity, const clsimhip_relabel *map, size_t n_map, void *d_out,
                                  void *d_out_counts, size_t out_capacity, void *d_workspace, size_t workspace_bytes, hipStream_t stream);
void event_stats_combine_device(int device, const void *d_a, const void *d_a_count, size_t capacity_a, const void *d_b, const void *d_b_count, size_t capacity_b,
                                void *d_out, void *d_out_counts, size_t out_capacity, void *d_workspace, size_t workspace_bytes, hipStream_t stream);
void event_stats_split_device(int device, const void *d_records, const void *d_count, size_t capacity, uint32_t last_frame, void *d_head, void *d_head_counts,
                              size_t head_capacity, void *d_tail, void *d_tail_counts, size_t tail_capacity, hipStream_t stream);

// ---- the store: add = COMBINE(store, CANON(bunch, map)); drain = CANON(head of SPLIT, map), the tail stays.  The sticky counters are
// FrameStoreSticky (series_union.h).  Sizes are those of the head BEFORE the drain's map folds it: what the output must hold. ----
class EventStatsStore {
public:
    virtual ~EventStatsStore() = default;
    virtual bool on_device() const = 0;
    virtual void add_host(const clsimhip_event_statistics *records, size_t n, const clsimhip_relabel *map, size_t n_map) = 0;
    virtual void add_device(const void *d_records, const void *d_count, size_t capacity, const clsimhip_relabel *map, size_t n_map, hipStream_t stream) = 0;
    virtual void drain_device(uint32_t last_frame, const clsimhip_relabel *map, size_t n_map, void *d_out, void *d_counts, size_t capacity, hipStream_t stream) = 0;
    virtual void drain_host(uint32_t last_frame, const clsimhip_relabel *map, size_t n_map, clsimhip_event_statistics *out, size_t capacity, size_t *n) = 0;
    virtual void size(uint32_t last_frame, size_t *n) = 0;
};
std::unique_ptr<EventStatsStore> make_host_event_stats_store(size_t capacity);                  // event_stats_store.cpp
std::unique_ptr<EventStatsStore> make_device_event_stats_store(int device, size_t capacity);    // event_stats_store_kernel.hip

} // namespace clsimhip
