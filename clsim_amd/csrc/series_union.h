// Frame stores: what the union of two series forms, the split of one at a frame bound and the store built on them share, whatever the
// record is.  A stage is this statement instantiated over a traits type T (McpeUnion in mcpe_union.h, FramePhotonUnion in
// frame_photon_union.h, PmtHitUnion in pmt_hit_union.h), which carries
//   Record, Entry, Key; kRecordWords, kEntryWords, kKeyWords, kChannelWords (the leading key words a table entry stands for);
//   kAlign: what the device side asks of record and table addresses;
//   key_of(frame, records, i), entry_ok, record_ok, open_entry (a new table entry for a record, count 0);
//   kStore, kName, kEntryRule, kRecordRule: the words of its messages.
// The definition lives here ONCE, as functions both the host twins (series_union_host.h) and the HIP kernels
// (series_union_device.hip.h) compile.  A series form is sorted by one integer key and equal keys are equal bytes, so the union is a
// function of the multiset of records: the same bytes whatever order the bunches arrive in.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <memory>

namespace clsimhip {

#define UNION_HD __host__ __device__ __forceinline__

// ascending in (string ID signed, OM ID); `word` = string ID | OM ID << 16, as in the records and the table entries
UNION_HD uint32_t union_dom_code(uint32_t word) { return (((word & 0xffffu) ^ 0x8000u) << 16) | (word >> 16); }
UNION_HD uint32_t union_dom_word(uint32_t code) { return ((code >> 16) ^ 0x8000u) | (code << 16); }

// keys compare word by word as unsigned integers, most significant word first
UNION_HD bool union_words_less(const uint32_t *a, const uint32_t *b, uint32_t words)
{
    for (uint32_t k = 0; k < words; ++k)
        if (a[k] != b[k]) return a[k] < b[k];
    return false;
}
template <class T>
UNION_HD bool union_key_less(const typename T::Key &a, const typename T::Key &b) { return union_words_less(a.w, b.w, T::kKeyWords); }

// the entry record i belongs to: the last one with first <= i, by bisection over `first` (as the photon hits stage finds it); -1
// when there is none.  At most 32 trips whatever the table holds.
template <class Entry>
UNION_HD int64_t union_entry_of(const Entry *series, uint32_t n_series, uint32_t i)
{
    uint32_t lo = 0u, hi = n_series;                                    // first entry with first > i
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (series[mid].first <= i) lo = mid + 1u; else hi = mid;
    }
    return (int64_t)lo - 1;
}

// Split: the number of entries with frame <= last_frame, a prefix of a table ascending in the frame
template <class Entry>
UNION_HD uint32_t union_split_entries(const Entry *series, uint32_t n_series, uint32_t last_frame)
{
    uint32_t lo = 0u, hi = n_series;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (series[mid].frame <= last_frame) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// ---- the device stage ----
// words of the series stage's header (mcpe_series.h: SeriesHeader) the union keeps its own sizes in; the tile scan it shares with
// the series stage reads SH_KEPT (the records of the output) and writes SH_SERIES
enum UnionHeader : uint32_t { UH_MALFORMED_A = 2, UH_MALFORMED_B = 3, UH_OVERFLOW = 4 /* with SH_KEPT, SH_SERIES: the five output counts */,
                              UH_N_A = 40 /* the effective sizes */, UH_N_B = 41, UH_IN_A = 42 /* what the inputs hold */, UH_IN_B = 43,
                              UH_SERIES_A = 44, UH_SERIES_B = 45 };

template <class T>
struct UnionDeviceArgs {
    const typename T::Record *a_records;
    const typename T::Entry *a_series;
    const uint32_t *a_counts;               // records = min([0], capacity_a), series = min([1], capacity_a)
    const typename T::Record *b_records;
    const typename T::Entry *b_series;
    const uint32_t *b_counts;
    uint32_t capacity_a, capacity_b, out_capacity;
    uint32_t *header;                       // kSeriesHeaderWords
    uint32_t *tile_counts;                  // heads per output tile, scanned in place
    uint32_t *partition;                    // per output tile boundary: records of A in front of it
    uint32_t *a_frames, *b_frames;          // per input record: its entry's frame
    uint32_t *out_frames;                   // per output record
    typename T::Record *out_records;
    typename T::Entry *out_series;
    uint32_t *out_counts;                   // five
};

template <class T>
struct SplitDeviceArgs {
    const typename T::Record *records;
    const typename T::Entry *series;
    const uint32_t *counts;
    uint32_t capacity, last_frame;
    const uint32_t *blocked;                // (may be null) five words: any nonzero -> nothing is drained
    typename T::Record *head_records;       // (null with head_series: the head is dropped, the store's own use behind a download)
    typename T::Entry *head_series;
    uint32_t *head_counts;                  // five: records, series, 0, 0, overflow
    uint32_t head_capacity;
    typename T::Record *tail_records;
    typename T::Entry *tail_series;
    uint32_t *tail_counts;                  // five: records, series, 0, 0, 0
};

// what every traits type must keep: the word counts are the types' sizes, and the kernels' arguments have the layout they always had
template <class T>
constexpr bool union_traits_ok()
{
    static_assert(sizeof(typename T::Record) == 4u * T::kRecordWords, "kRecordWords is not the record's size");
    static_assert(sizeof(typename T::Entry) == 4u * T::kEntryWords, "kEntryWords is not the table entry's size");
    static_assert(sizeof(typename T::Key) == 4u * T::kKeyWords, "kKeyWords is not the key's size");
    static_assert(sizeof(UnionDeviceArgs<T>) == 136u && sizeof(SplitDeviceArgs<T>) == 96u, "the kernels' arguments changed their layout");
    return true;
}

// ---- the store ----
constexpr size_t kFrameStoreMaxCapacity = size_t{1} << 31;
// sticky counters of a device store: data that was dropped on the device, where no call could refuse it
enum FrameStoreSticky : uint32_t { FS_MALFORMED_BUNCHES = 0, FS_MALFORMED_ELEMENTS = 1, FS_OVERFLOWED_BUNCHES = 2, FS_OVERFLOWED_RECORDS = 3, FS_MALFORMED_STORE = 4 };

template <class T>
class FrameStoreOf {
public:
    using Record = typename T::Record;
    using Entry = typename T::Entry;
    virtual ~FrameStoreOf() = default;
    virtual bool on_device() const = 0;
    virtual void add_host(const Record *records, size_t n, const Entry *series, size_t n_series) = 0;
    virtual void add_device(const void *d_records, const void *d_series, const void *d_series_counts, size_t capacity, hipStream_t stream) = 0;
    virtual void drain_device(uint32_t last_frame, void *d_records, void *d_series, void *d_counts, size_t capacity, hipStream_t stream) = 0;
    virtual void drain_host(uint32_t last_frame, Record *records, Entry *series, size_t capacity, size_t *n, size_t *n_series) = 0;
    virtual void size(uint32_t last_frame, size_t *n, size_t *n_series) = 0;
};

} // namespace clsimhip
