// MCPE frame store: the union of two series-form inputs, the split of one at a frame bound, and the store that folds bunches into
// accumulated state and gives up finished frames (include/clsimhip.h: "MCPE frame store").  The definition lives here ONCE, as
// functions both the host twins (mcpe_union.cpp) and the HIP kernels (mcpe_union_kernel.hip) compile.  It stands where the
// reference's client module files every result's hits into a frame cache that lives across bunches and commits the oldest frames no
// bunch in flight can still touch
//   I3CLSimClientModule::AddPhotonsToFrames   private/clsim/I3CLSimClientModule.cxx:359-439  (frame->hits)
//   I3CLSimClientModule::FlushFrameCache      :686-758  (framesForBunches_, lastPendingFrame: a prefix of the cache)
// A series form is sorted by one integer key and equal keys are equal bytes, so the union is a function of the multiset of records:
// the same bytes whatever order the bunches arrive in.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <memory>

#include "mcpe_series.h"

namespace clsimhip {

#define UNION_HD __host__ __device__ __forceinline__

// The key of a record: (frame of its entry, DOM code, tkey high, tkey low, identifier), most significant word first, compared word
// by word as unsigned integers.  The comparison takes the number of words: a 24- or 48-byte record's key is a longer array.
constexpr uint32_t kUnionKeyWords = 5u;
struct UnionKey { uint32_t w[kUnionKeyWords]; };

// ascending in (string ID signed, OM ID); `word` = string ID | OM ID << 16, as in the records and the table entries
UNION_HD uint32_t union_dom_code(uint32_t word) { return (((word & 0xffffu) ^ 0x8000u) << 16) | (word >> 16); }
UNION_HD uint32_t union_dom_word(uint32_t code) { return ((code >> 16) ^ 0x8000u) | (code << 16); }

UNION_HD bool union_words_less(const uint32_t *a, const uint32_t *b, uint32_t words)
{
    for (uint32_t k = 0; k < words; ++k)
        if (a[k] != b[k]) return a[k] < b[k];
    return false;
}
UNION_HD bool union_key_less(const UnionKey &a, const UnionKey &b) { return union_words_less(a.w, b.w, kUnionKeyWords); }

// a record's first 8 bytes: identifier | string ID << 32 | OM ID << 48; a table entry's: frame | string ID << 32 | OM ID << 48
UNION_HD UnionKey union_make_key(uint32_t frame, uint64_t ids, uint64_t time_bits)
{
    const uint64_t t = series_tkey(__builtin_bit_cast(double, time_bits));
    UnionKey k;
    k.w[0] = frame;
    k.w[1] = union_dom_code((uint32_t)(ids >> 32));
    k.w[2] = (uint32_t)(t >> 32);
    k.w[3] = (uint32_t)t;
    k.w[4] = (uint32_t)ids;
    return k;
}

// (frame, DOM code) of a table entry as one integer
UNION_HD uint64_t union_entry_code(const clsimhip_mcpe_series &e)
{
    return ((uint64_t)e.frame << 32) | union_dom_code((uint32_t)(uint16_t)e.string_id | ((uint32_t)e.om_id << 16));
}

// ---- the local checks of a series form: every element that breaks one is one MALFORMED element; together they imply that the
// table partitions the records and that the records ascend in the key ----
// entry s of a table of n_series entries over n records
UNION_HD bool union_entry_ok(const clsimhip_mcpe_series *series, uint32_t n_series, uint32_t n, uint32_t s)
{
    const clsimhip_mcpe_series e = series[s];
    if (e.count == 0u) return false;
    if (s == 0u) {
        if (e.first != 0u) return false;
    } else {
        const clsimhip_mcpe_series p = series[s - 1u];
        if ((uint64_t)e.first != (uint64_t)p.first + p.count) return false;
        if (!(union_entry_code(p) < union_entry_code(e))) return false;
    }
    if (s + 1u == n_series && (uint64_t)e.first + e.count != (uint64_t)n) return false;
    return true;
}

// the entry record i belongs to: the last one with first <= i, by bisection over `first` (as the photon hits stage finds it); -1
// when there is none.  At most 32 trips whatever the table holds.
UNION_HD int64_t union_entry_of(const clsimhip_mcpe_series *series, uint32_t n_series, uint32_t i)
{
    uint32_t lo = 0u, hi = n_series;                                    // first entry with first > i
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (series[mid].first <= i) lo = mid + 1u; else hi = mid;
    }
    return (int64_t)lo - 1;
}

// record i of n; *frame receives its entry's frame (0 without an entry)
UNION_HD bool union_record_ok(const clsimhip_mcpe *records, const clsimhip_mcpe_series *series, uint32_t n_series, uint32_t i, uint32_t *frame)
{
    *frame = 0u;
    const int64_t s = union_entry_of(series, n_series, i);
    if (s < 0) return false;                                            // (an empty table needs zero records)
    const clsimhip_mcpe_series e = series[s];
    *frame = e.frame;
    if ((uint64_t)i >= (uint64_t)e.first + e.count) return false;
    const uint64_t *rec = reinterpret_cast<const uint64_t *>(records + i);
    if ((uint32_t)(rec[0] >> 32) != ((uint32_t)(uint16_t)e.string_id | ((uint32_t)e.om_id << 16))) return false;
    if (i > e.first) {                                                  // inside a series (tkey, identifier) does not descend
        const uint64_t *before = reinterpret_cast<const uint64_t *>(records + (i - 1u));
        const uint64_t ta = series_tkey(__builtin_bit_cast(double, before[1])), tb = series_tkey(__builtin_bit_cast(double, rec[1]));
        if (ta > tb || (ta == tb && (uint32_t)before[0] > (uint32_t)rec[0])) return false;
    }
    return true;
}

// Split: the number of entries with frame <= last_frame, a prefix of a table ascending in the frame
UNION_HD uint32_t union_split_entries(const clsimhip_mcpe_series *series, uint32_t n_series, uint32_t last_frame)
{
    uint32_t lo = 0u, hi = n_series;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (series[mid].frame <= last_frame) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// ---- the host twins (mcpe_union.cpp: host only, no HIP call); they throw Error (CLSIMHIP_ERR_ARGUMENT) ----
void mcpe_series_union_host(const clsimhip_mcpe *a_records, size_t n_a, const clsimhip_mcpe_series *a_series, size_t n_series_a, const clsimhip_mcpe *b_records,
                            size_t n_b, const clsimhip_mcpe_series *b_series, size_t n_series_b, clsimhip_mcpe *out_records, clsimhip_mcpe_series *out_series,
                            size_t out_capacity, size_t *n, size_t *n_series);
void mcpe_series_split_host(const clsimhip_mcpe *records, size_t n, const clsimhip_mcpe_series *series, size_t n_series, uint32_t last_frame,
                            clsimhip_mcpe *head_records, clsimhip_mcpe_series *head_series, size_t head_capacity, size_t *n_head, size_t *n_series_head,
                            clsimhip_mcpe *tail_records, clsimhip_mcpe_series *tail_series, size_t tail_capacity, size_t *n_tail, size_t *n_series_tail);
// what is wrong with a series form: throws, with text that names the first offending element (`what`: "A", "B", "the bunch" ...)
void mcpe_series_form_check(const char *what, const clsimhip_mcpe *records, size_t n, const clsimhip_mcpe_series *series, size_t n_series);

// ---- the device stage (mcpe_union_kernel.hip) ----
// words of the series stage's header (mcpe_series.h: SeriesHeader) the union keeps its own sizes in; the tile scan it shares with
// the series stage reads SH_KEPT (the records of the output) and writes SH_SERIES
enum UnionHeader : uint32_t { UH_MALFORMED_A = 2, UH_MALFORMED_B = 3, UH_OVERFLOW = 4 /* with SH_KEPT, SH_SERIES: the five output counts */,
                              UH_N_A = 40 /* the effective sizes */, UH_N_B = 41, UH_IN_A = 42 /* what the inputs hold */, UH_IN_B = 43,
                              UH_SERIES_A = 44, UH_SERIES_B = 45 };

struct UnionDeviceArgs {
    const clsimhip_mcpe *a_records;
    const clsimhip_mcpe_series *a_series;
    const uint32_t *a_counts;               // records = min([0], capacity_a), series = min([1], capacity_a)
    const clsimhip_mcpe *b_records;
    const clsimhip_mcpe_series *b_series;
    const uint32_t *b_counts;
    uint32_t capacity_a, capacity_b, out_capacity;
    uint32_t *header;                       // kSeriesHeaderWords
    uint32_t *tile_counts;                  // heads per output tile, scanned in place
    uint32_t *partition;                    // per output tile boundary: records of A in front of it
    uint32_t *a_frames, *b_frames;          // per input record: its entry's frame
    uint32_t *out_frames;                   // per output record
    clsimhip_mcpe *out_records;
    clsimhip_mcpe_series *out_series;
    uint32_t *out_counts;                   // five
};

struct SplitDeviceArgs {
    const clsimhip_mcpe *records;
    const clsimhip_mcpe_series *series;
    const uint32_t *counts;
    uint32_t capacity, last_frame;
    const uint32_t *blocked;                // (may be null) five words: any nonzero -> nothing is drained
    clsimhip_mcpe *head_records;            // (null with head_series: the head is dropped, the store's own use behind a download)
    clsimhip_mcpe_series *head_series;
    uint32_t *head_counts;                  // five: records, series, 0, 0, overflow
    uint32_t head_capacity;
    clsimhip_mcpe *tail_records;
    clsimhip_mcpe_series *tail_series;
    uint32_t *tail_counts;                  // five: records, series, 0, 0, 0
};

size_t mcpe_union_workspace_bytes(size_t capacity_a, size_t capacity_b);
void mcpe_union_device(int device, const void *d_a_records, const void *d_a_series, const void *d_a_counts, size_t capacity_a, const void *d_b_records,
                       const void *d_b_series, const void *d_b_counts, size_t capacity_b, void *d_out_records, void *d_out_series, void *d_out_counts,
                       size_t out_capacity, void *d_workspace, size_t workspace_bytes, hipStream_t stream);
void mcpe_split_device(int device, const void *d_records, const void *d_series, const void *d_counts, size_t capacity, uint32_t last_frame,
                       void *d_head_records, void *d_head_series, void *d_head_counts, size_t head_capacity, void *d_tail_records, void *d_tail_series,
                       void *d_tail_counts, size_t tail_capacity, hipStream_t stream);

// ---- the store ----
constexpr size_t kFrameStoreMaxCapacity = size_t{1} << 31;
// sticky counters of a device store: data that was dropped on the device, where no call could refuse it
enum FrameStoreSticky : uint32_t { FS_MALFORMED_BUNCHES = 0, FS_MALFORMED_ELEMENTS = 1, FS_OVERFLOWED_BUNCHES = 2, FS_OVERFLOWED_RECORDS = 3, FS_MALFORMED_STORE = 4 };

class FrameStore {
public:
    virtual ~FrameStore() = default;
    virtual bool on_device() const = 0;
    virtual void add_host(const clsimhip_mcpe *records, size_t n, const clsimhip_mcpe_series *series, size_t n_series) = 0;
    virtual void add_device(const void *d_records, const void *d_series, const void *d_series_counts, size_t capacity, hipStream_t stream) = 0;
    virtual void drain_device(uint32_t last_frame, void *d_records, void *d_series, void *d_counts, size_t capacity, hipStream_t stream) = 0;
    virtual void drain_host(uint32_t last_frame, clsimhip_mcpe *records, clsimhip_mcpe_series *series, size_t capacity, size_t *n, size_t *n_series) = 0;
    virtual void size(uint32_t last_frame, size_t *n, size_t *n_series) = 0;
};
std::unique_ptr<FrameStore> make_host_frame_store(size_t capacity);                     // mcpe_union.cpp
std::unique_ptr<FrameStore> make_device_frame_store(int device, size_t capacity);       // mcpe_union_kernel.hip

} // namespace clsimhip
