// PMT hit frame store: the union of two series forms of PMT hits, the split of one at a frame bound, and the store that folds bunches
// into accumulated state and gives up finished frames (include/clsimhip.h: "PMT hit frame store").  The stage itself is stated once
// for every record type (series_union.h, series_union_host.h, series_union_device.hip.h); what is the PMT hit's own lives here ONCE,
// as functions both the host twins (pmt_hit_union.cpp) and the HIP kernels (pmt_hit_union_kernel.hip) compile, with the traits type
// PmtHitUnion that hands them to the shared statement.  The stage stands where the reference's client module files every result into
// a frame cache that lives across bunches and commits the oldest frames no bunch in flight can still touch
//   I3CLSimClientModule::AddPhotonsToFrames   private/clsim/I3CLSimClientModule.cxx:359-439
//   I3CLSimClientModule::FlushFrameCache      :686-758  (framesForBunches_, lastPendingFrame: a prefix of the cache)
// The integer time key is the frame photon store's, taken as it stands.  What needs the PMT table type (24-byte entries with a pmt
// word and a reserved word) is stated here: the entry check and the record check.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <memory>

#include "frame_photon_union.h"
#include "mcpe_union.h"

namespace clsimhip {

// The key of a record: (frame of its entry, DOM code, pmt, tkey high, tkey low, identifier), most significant word first, compared
// word by word as unsigned integers (union_words_less).  pmt is the whole word.  The record is a function of its key.
constexpr uint32_t kPmtHitKeyWords = 6u;
constexpr uint32_t kPmtHitChannelWords = 3u;                            // frame, DOM code, pmt: what a table entry stands for
constexpr uint32_t kPmtHitRecordWords = 6u;                             // a clsimhip_pmt_hit as uint32 words
constexpr uint32_t kPmtHitEntryWords = 6u;                              // a clsimhip_pmt_series as uint32 words
struct PmtHitKey { uint32_t w[kPmtHitKeyWords]; };

// a record as words: 0 identifier, 1 string ID | OM ID << 16, 2 pmt, 3 reserved, 4-5 the time's bit pattern
// an entry as words: 0 frame, 1 string ID | OM ID << 16, 2 pmt, 3 first, 4 count, 5 reserved
UNION_HD const uint32_t *pmt_hit_union_words(const clsimhip_pmt_hit *records, size_t i) { return reinterpret_cast<const uint32_t *>(records + i); }
UNION_HD const uint32_t *pmt_hit_union_entry_words(const clsimhip_pmt_series *series, size_t s) { return reinterpret_cast<const uint32_t *>(series + s); }

// The time travels as its bit pattern (frame_photon_union_tkey is an inversion on the bits): no floating-point value is made of it,
// so a signalling NaN keeps its payload on both targets.
UNION_HD PmtHitKey pmt_hit_union_make_key(uint32_t frame, const uint32_t rec[kPmtHitRecordWords])
{
    const uint64_t t = frame_photon_union_tkey((uint64_t)rec[4] | ((uint64_t)rec[5] << 32));
    PmtHitKey k;
    k.w[0] = frame;
    k.w[1] = union_dom_code(rec[1]);
    k.w[2] = rec[2];
    k.w[3] = (uint32_t)(t >> 32);
    k.w[4] = (uint32_t)t;
    k.w[5] = rec[0];
    return k;
}

// the record of a key: identifier, DOM word, pmt, 0, the time whose key it is (the inversion's inverse)
UNION_HD void pmt_hit_union_record_of(const uint32_t key[kPmtHitKeyWords], uint32_t rec[kPmtHitRecordWords])
{
    const uint64_t t = ((uint64_t)key[3] << 32) | key[4];
    const uint64_t bits = t ^ ((t >> 63) ? (1ull << 63) : ~0ull);
    rec[0] = key[5];
    rec[1] = union_dom_word(key[1]);
    rec[2] = key[2];
    rec[3] = 0u;
    rec[4] = (uint32_t)bits;
    rec[5] = (uint32_t)(bits >> 32);
}

// (frame, DOM code, pmt) of a table entry
UNION_HD void pmt_hit_union_entry_channel(const uint32_t e[kPmtHitEntryWords], uint32_t channel[kPmtHitChannelWords])
{
    channel[0] = e[0];
    channel[1] = union_dom_code(e[1]);
    channel[2] = e[2];
}

// ---- the local checks of a series form of PMT hits: every element that breaks one is one MALFORMED element ----
// entry s of a table of n_series entries over n records
UNION_HD bool pmt_hit_union_entry_ok(const clsimhip_pmt_series *series, uint32_t n_series, uint32_t n, uint32_t s)
{
    const uint32_t *e = pmt_hit_union_entry_words(series, s);
    const uint32_t first = e[3], count = e[4];
    if (count == 0u) return false;
    if (e[5] != 0u) return false;
    if (s == 0u) {
        if (first != 0u) return false;
    } else {
        const uint32_t *p = pmt_hit_union_entry_words(series, s - 1u);
        if ((uint64_t)first != (uint64_t)p[3] + p[4]) return false;
        uint32_t before[kPmtHitChannelWords], here[kPmtHitChannelWords];
        pmt_hit_union_entry_channel(p, before);
        pmt_hit_union_entry_channel(e, here);
        if (!union_words_less(before, here, kPmtHitChannelWords)) return false;
    }
    if (s + 1u == n_series && (uint64_t)first + count != (uint64_t)n) return false;
    return true;
}

// record i of n; *frame receives its entry's frame (0 without an entry)
UNION_HD bool pmt_hit_union_record_ok(const clsimhip_pmt_hit *records, const clsimhip_pmt_series *series, uint32_t n_series, uint32_t i, uint32_t *frame)
{
    *frame = 0u;
    const int64_t s = union_entry_of(series, n_series, i);
    if (s < 0) return false;                                            // (an empty table needs zero records)
    const uint32_t *e = pmt_hit_union_entry_words(series, (size_t)s);
    const uint32_t first = e[3], count = e[4];
    *frame = e[0];
    if ((uint64_t)i >= (uint64_t)first + count) return false;
    const uint32_t *rec = pmt_hit_union_words(records, i);
    if (rec[1] != e[1] || rec[2] != e[2] || rec[3] != 0u) return false;
    if (i > first) {                                                    // inside a series (tkey, identifier) does not descend
        const PmtHitKey before = pmt_hit_union_make_key(e[0], pmt_hit_union_words(records, i - 1u));
        const PmtHitKey here = pmt_hit_union_make_key(e[0], rec);
        if (union_words_less(here.w + 3, before.w + 3, 3u)) return false;
    }
    return true;
}

// what the shared statement of the stage (series_union.h) takes from this header
struct PmtHitUnion {
    using Record = clsimhip_pmt_hit;
    using Entry = clsimhip_pmt_series;
    using Key = PmtHitKey;
    static constexpr uint32_t kRecordWords = kPmtHitRecordWords, kEntryWords = kPmtHitEntryWords, kKeyWords = kPmtHitKeyWords, kChannelWords = kPmtHitChannelWords,
                              kAlign = 8u;
    static constexpr const char *kStore = "PMT hit frame store", *kName = "PMT hit";
    static constexpr const char *kEntryRule =
        "the table must ascend strictly in (frame, string_id, om_id, pmt), every count > 0, every reserved = 0, first[0] = 0, first[s] = first[s-1] + count[s-1]";
    static constexpr const char *kRecordRule =
        "every record must lie in an entry, carry its string_id, om_id and pmt, have reserved = 0, and not descend in (time key, identifier) behind its predecessor";
    static UNION_HD Key key_of(uint32_t frame, const Record *records, size_t i) { return pmt_hit_union_make_key(frame, pmt_hit_union_words(records, i)); }
    static UNION_HD bool entry_ok(const Entry *series, uint32_t n_series, uint32_t n, uint32_t s) { return pmt_hit_union_entry_ok(series, n_series, n, s); }
    static UNION_HD bool record_ok(const Record *records, const Entry *series, uint32_t n_series, uint32_t i, uint32_t *frame)
    {
        return pmt_hit_union_record_ok(records, series, n_series, i, frame);
    }
    static void open_entry(Entry &s, uint32_t frame, const Record &r)
    {
        s.frame = frame;
        s.string_id = r.string_id; s.om_id = r.om_id;
        s.pmt = r.pmt;
        s.count = 0u;
        s.reserved = 0u;
    }
};
static_assert(union_traits_ok<PmtHitUnion>(), "");

// ---- the host twins (pmt_hit_union.cpp: host only, no HIP call); they throw Error (CLSIMHIP_ERR_ARGUMENT) ----
void pmt_hits_union_host(const clsimhip_pmt_hit *a_records, size_t n_a, const clsimhip_pmt_series *a_series, size_t n_series_a, const clsimhip_pmt_hit *b_records,
                         size_t n_b, const clsimhip_pmt_series *b_series, size_t n_series_b, clsimhip_pmt_hit *out_records, clsimhip_pmt_series *out_series,
                         size_t out_capacity, size_t *n, size_t *n_series);
void pmt_hits_split_host(const clsimhip_pmt_hit *records, size_t n, const clsimhip_pmt_series *series, size_t n_series, uint32_t last_frame,
                         clsimhip_pmt_hit *head_records, clsimhip_pmt_series *head_series, size_t head_capacity, size_t *n_head, size_t *n_series_head,
                         clsimhip_pmt_hit *tail_records, clsimhip_pmt_series *tail_series, size_t tail_capacity, size_t *n_tail, size_t *n_series_tail);
// what is wrong with a series form: throws, with text that names the first offending element (`what`: "A", "B", "the bunch" ...)
void pmt_hits_form_check(const char *what, const clsimhip_pmt_hit *records, size_t n, const clsimhip_pmt_series *series, size_t n_series);

// ---- the device stage (pmt_hit_union_kernel.hip) ----
// The header is the MCPE union's (series_union.h: UnionHeader beside mcpe_series.h's SH_KEPT and SH_SERIES), so that
// launch_series_tile_scan runs unchanged on it.
size_t pmt_hits_union_workspace_bytes(size_t capacity_a, size_t capacity_b);
void pmt_hits_union_device(int device, const void *d_a_records, const void *d_a_series, const void *d_a_counts, size_t capacity_a, const void *d_b_records,
                           const void *d_b_series, const void *d_b_counts, size_t capacity_b, void *d_out_records, void *d_out_series, void *d_out_counts,
                           size_t out_capacity, void *d_workspace, size_t workspace_bytes, hipStream_t stream);
void pmt_hits_split_device(int device, const void *d_records, const void *d_series, const void *d_counts, size_t capacity, uint32_t last_frame,
                           void *d_head_records, void *d_head_series, void *d_head_counts, size_t head_capacity, void *d_tail_records, void *d_tail_series,
                           void *d_tail_counts, size_t tail_capacity, hipStream_t stream);

// ---- the store: the sticky counters are FrameStoreSticky ----
using PmtHitStore = FrameStoreOf<PmtHitUnion>;
std::unique_ptr<PmtHitStore> make_host_pmt_hit_store(size_t capacity);                  // pmt_hit_union.cpp
std::unique_ptr<PmtHitStore> make_device_pmt_hit_store(int device, size_t capacity);    // pmt_hit_union_kernel.hip

} // namespace clsimhip
