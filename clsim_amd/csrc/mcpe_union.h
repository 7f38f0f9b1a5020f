// MCPE frame store: the union of two series-form inputs, the split of one at a frame bound, and the store that folds bunches into
// accumulated state and gives up finished frames (include/clsimhip.h: "MCPE frame store").  The stage itself is stated once for
// every record type (series_union.h, series_union_host.h, series_union_device.hip.h); what is the MCPE's own lives here ONCE, as
// functions both the host twins (mcpe_union.cpp) and the HIP kernels (mcpe_union_kernel.hip) compile: the key, the local checks of
// its series form and the traits type McpeUnion that hands them to the shared statement.  The stage stands where the reference's
// client module files every result's hits into a frame cache that lives across bunches and commits the oldest frames no bunch in
// flight can still touch
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
#include "series_union.h"

namespace clsimhip {

// The key of a record: (frame of its entry, DOM code, tkey high, tkey low, identifier), most significant word first, compared word
// by word as unsigned integers (union_words_less).
constexpr uint32_t kUnionKeyWords = 5u;
struct UnionKey { uint32_t w[kUnionKeyWords]; };

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

// what the shared statement of the stage (series_union.h) takes from this header
struct McpeUnion {
    using Record = clsimhip_mcpe;
    using Entry = clsimhip_mcpe_series;
    using Key = UnionKey;
    static constexpr uint32_t kRecordWords = 4u, kEntryWords = 4u, kKeyWords = kUnionKeyWords, kChannelWords = 2u /* frame, DOM code */, kAlign = 16u;
    static constexpr const char *kStore = "MCPE frame store", *kName = "MCPE";
    static constexpr const char *kEntryRule = "the table must ascend strictly in (frame, string_id, om_id), every count > 0, first[0] = 0, first[s] = first[s-1] + count[s-1]";
    static constexpr const char *kRecordRule = "every record must lie in an entry, carry its string_id and om_id, and not descend in (time key, identifier) behind its predecessor";
    static UNION_HD Key key_of(uint32_t frame, const Record *records, size_t i)
    {
        const uint64_t *rec = reinterpret_cast<const uint64_t *>(records + i);
        return union_make_key(frame, rec[0], rec[1]);
    }
    static UNION_HD bool entry_ok(const Entry *series, uint32_t n_series, uint32_t n, uint32_t s) { return union_entry_ok(series, n_series, n, s); }
    static UNION_HD bool record_ok(const Record *records, const Entry *series, uint32_t n_series, uint32_t i, uint32_t *frame)
    {
        return union_record_ok(records, series, n_series, i, frame);
    }
    // the table entry a record opens (first: the caller's)
    static void open_entry(Entry &s, uint32_t frame, const Record &r)
    {
        s.frame = frame;
        s.string_id = r.string_id; s.om_id = r.om_id;
        s.count = 0u;
    }
};
static_assert(union_traits_ok<McpeUnion>(), "");

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
size_t mcpe_union_workspace_bytes(size_t capacity_a, size_t capacity_b);
void mcpe_union_device(int device, const void *d_a_records, const void *d_a_series, const void *d_a_counts, size_t capacity_a, const void *d_b_records,
                       const void *d_b_series, const void *d_b_counts, size_t capacity_b, void *d_out_records, void *d_out_series, void *d_out_counts,
                       size_t out_capacity, void *d_workspace, size_t workspace_bytes, hipStream_t stream);
void mcpe_split_device(int device, const void *d_records, const void *d_series, const void *d_counts, size_t capacity, uint32_t last_frame,
                       void *d_head_records, void *d_head_series, void *d_head_counts, size_t head_capacity, void *d_tail_records, void *d_tail_series,
                       void *d_tail_counts, size_t tail_capacity, hipStream_t stream);

// ---- the store ----
using FrameStore = FrameStoreOf<McpeUnion>;
std::unique_ptr<FrameStore> make_host_frame_store(size_t capacity);                     // mcpe_union.cpp
std::unique_ptr<FrameStore> make_device_frame_store(int device, size_t capacity);       // mcpe_union_kernel.hip

} // namespace clsimhip
