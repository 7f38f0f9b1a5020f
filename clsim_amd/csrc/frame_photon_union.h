// Frame photon store: the union of two series forms of frame photons, the split of one at a frame bound, and the store that folds
// bunches into accumulated state and gives up finished frames (include/clsimhip.h: "Frame photon store").  The stage itself is stated
// once for every record type (series_union.h, series_union_host.h, series_union_device.hip.h); what is the frame photon's own lives
// here ONCE, as functions both the host twins (frame_photon_union.cpp) and the HIP kernels (frame_photon_union_kernel.hip) compile,
// with the traits type FramePhotonUnion that hands them to the shared statement.  The stage stands where the reference's client
// module files every result's photons into a frame cache that lives across bunches and commits the oldest frames no bunch in flight
// can still touch
//   I3CLSimClientModule::AddPhotonsToFrames   private/clsim/I3CLSimClientModule.cxx:359-439  ((*frame->photons)[ModuleKey] :407-415)
//   I3CLSimClientModule::FlushFrameCache      :686-758  (framesForBunches_, lastPendingFrame: a prefix of the cache)
// The table is the MCPE frame store's and its rules are taken from mcpe_union.h as they stand.  What is this stage's own is the key:
// 14 words, the last nine of them the record's content, so that records equal in the key are equal bytes and the union is a function
// of the multiset of records.  The comparison is the full key everywhere: the frame photons stage's bound on runs of content ties
// (frame_photons.h: kFramePhotonsTieBound) has no counterpart here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <memory>

#include "frame_photons.h"
#include "mcpe_union.h"

namespace clsimhip {

// The key of a record: (frame of its entry, DOM code, tkey high, tkey low, identifier, h, w0 ... w7), most significant word first,
// compared word by word as unsigned integers (union_words_less).  h = frame_photons_mix(w), w the eight float fields' bit patterns
// in declared order, as frame_photons.h defines them.
constexpr uint32_t kFramePhotonKeyWords = 14u;
constexpr uint32_t kFramePhotonSuffixWords = 12u;                       // tkey high ... w7: what must not descend inside a series
constexpr uint32_t kFramePhotonRecordWords = 12u;                       // a clsimhip_frame_photon as uint32 words
struct FramePhotonKey { uint32_t w[kFramePhotonKeyWords]; };

// a record as words: 0 identifier, 1 string ID | OM ID << 16, 2-3 the time's bit pattern, 4-11 w0 ... w7
UNION_HD void frame_photon_union_content(const uint32_t rec[kFramePhotonRecordWords], FramePhotonContent &c)
{
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k) c.w[k] = rec[4u + k];
}

// The time travels as its bit pattern: tkey is inverted on the bits (as pmt_photon_hits.h does), no floating-point value is made of
// it, so a signalling NaN keeps its payload on both targets.
UNION_HD uint64_t frame_photon_union_tkey(uint64_t time_bits) { return time_bits ^ ((time_bits >> 63) ? ~0ull : (1ull << 63)); }

UNION_HD FramePhotonKey frame_photon_union_make_key(uint32_t frame, const uint32_t rec[kFramePhotonRecordWords])
{
    const uint64_t t = frame_photon_union_tkey((uint64_t)rec[2] | ((uint64_t)rec[3] << 32));
    FramePhotonContent c;
    frame_photon_union_content(rec, c);
    FramePhotonKey k;
    k.w[0] = frame;
    k.w[1] = union_dom_code(rec[1]);
    k.w[2] = (uint32_t)(t >> 32);
    k.w[3] = (uint32_t)t;
    k.w[4] = rec[0];
    k.w[5] = frame_photons_mix(c);
#pragma unroll
    for (uint32_t j = 0; j < 8u; ++j) k.w[6u + j] = c.w[j];
    return k;
}

UNION_HD const uint32_t *frame_photon_union_words(const clsimhip_frame_photon *records, size_t i)
{
    return reinterpret_cast<const uint32_t *>(records + i);
}

// record i of n; *frame receives its entry's frame (0 without an entry).  The table's own rules are union_entry_ok's.
UNION_HD bool frame_photon_union_record_ok(const clsimhip_frame_photon *records, const clsimhip_mcpe_series *series, uint32_t n_series, uint32_t i, uint32_t *frame)
{
    *frame = 0u;
    const int64_t s = union_entry_of(series, n_series, i);
    if (s < 0) return false;                                            // (an empty table needs zero records)
    const clsimhip_mcpe_series e = series[s];
    *frame = e.frame;
    if ((uint64_t)i >= (uint64_t)e.first + e.count) return false;
    const uint32_t *rec = frame_photon_union_words(records, i);
    if (rec[1] != ((uint32_t)(uint16_t)e.string_id | ((uint32_t)e.om_id << 16))) return false;
    if (i > e.first) {                                                  // inside a series the 12-word suffix does not descend
        const FramePhotonKey before = frame_photon_union_make_key(e.frame, frame_photon_union_words(records, i - 1u));
        const FramePhotonKey here = frame_photon_union_make_key(e.frame, rec);
        if (union_words_less(here.w + 2, before.w + 2, kFramePhotonSuffixWords)) return false;
    }
    return true;
}

// what the shared statement of the stage (series_union.h) takes from this header
struct FramePhotonUnion {
    using Record = clsimhip_frame_photon;
    using Entry = clsimhip_mcpe_series;
    using Key = FramePhotonKey;
    static constexpr uint32_t kRecordWords = kFramePhotonRecordWords, kEntryWords = 4u, kKeyWords = kFramePhotonKeyWords, kChannelWords = 2u /* frame, DOM code */,
                              kAlign = 16u;
    static constexpr const char *kStore = "frame photon store", *kName = "frame photon";
    static constexpr const char *kEntryRule = McpeUnion::kEntryRule;
    static constexpr const char *kRecordRule =
        "every record must lie in an entry, carry its string_id and om_id, and not descend in (time key, identifier, h, w0 ... w7) behind its predecessor";
    static UNION_HD Key key_of(uint32_t frame, const Record *records, size_t i) { return frame_photon_union_make_key(frame, frame_photon_union_words(records, i)); }
    static UNION_HD bool entry_ok(const Entry *series, uint32_t n_series, uint32_t n, uint32_t s) { return union_entry_ok(series, n_series, n, s); }
    static UNION_HD bool record_ok(const Record *records, const Entry *series, uint32_t n_series, uint32_t i, uint32_t *frame)
    {
        return frame_photon_union_record_ok(records, series, n_series, i, frame);
    }
    static void open_entry(Entry &s, uint32_t frame, const Record &r)
    {
        s.frame = frame;
        s.string_id = r.string_id; s.om_id = r.om_id;
        s.count = 0u;
    }
};
static_assert(union_traits_ok<FramePhotonUnion>(), "");

// ---- the host twins (frame_photon_union.cpp: host only, no HIP call); they throw Error (CLSIMHIP_ERR_ARGUMENT) ----
void frame_photons_union_host(const clsimhip_frame_photon *a_records, size_t n_a, const clsimhip_mcpe_series *a_series, size_t n_series_a,
                              const clsimhip_frame_photon *b_records, size_t n_b, const clsimhip_mcpe_series *b_series, size_t n_series_b,
                              clsimhip_frame_photon *out_records, clsimhip_mcpe_series *out_series, size_t out_capacity, size_t *n, size_t *n_series);
void frame_photons_split_host(const clsimhip_frame_photon *records, size_t n, const clsimhip_mcpe_series *series, size_t n_series, uint32_t last_frame,
                              clsimhip_frame_photon *head_records, clsimhip_mcpe_series *head_series, size_t head_capacity, size_t *n_head, size_t *n_series_head,
                              clsimhip_frame_photon *tail_records, clsimhip_mcpe_series *tail_series, size_t tail_capacity, size_t *n_tail, size_t *n_series_tail);
// what is wrong with a series form: throws, with text that names the first offending element (`what`: "A", "B", "the bunch" ...)
void frame_photons_form_check(const char *what, const clsimhip_frame_photon *records, size_t n, const clsimhip_mcpe_series *series, size_t n_series);

// ---- the device stage (frame_photon_union_kernel.hip) ----
// The header is the MCPE union's (series_union.h: UnionHeader beside mcpe_series.h's SH_KEPT and SH_SERIES), so that
// launch_series_tile_scan runs unchanged on it.
size_t frame_photons_union_workspace_bytes(size_t capacity_a, size_t capacity_b);
void frame_photons_union_device(int device, const void *d_a_records, const void *d_a_series, const void *d_a_counts, size_t capacity_a, const void *d_b_records,
                                const void *d_b_series, const void *d_b_counts, size_t capacity_b, void *d_out_records, void *d_out_series, void *d_out_counts,
                                size_t out_capacity, void *d_workspace, size_t workspace_bytes, hipStream_t stream);
void frame_photons_split_device(int device, const void *d_records, const void *d_series, const void *d_counts, size_t capacity, uint32_t last_frame,
                                void *d_head_records, void *d_head_series, void *d_head_counts, size_t head_capacity, void *d_tail_records, void *d_tail_series,
                                void *d_tail_counts, size_t tail_capacity, hipStream_t stream);

// ---- the store: the sticky counters are FrameStoreSticky ----
using FramePhotonStore = FrameStoreOf<FramePhotonUnion>;
std::unique_ptr<FramePhotonStore> make_host_frame_photon_store(size_t capacity);                    // frame_photon_union.cpp
std::unique_ptr<FramePhotonStore> make_device_frame_photon_store(int device, size_t capacity);      // frame_photon_union_kernel.hip

} // namespace clsimhip
