// Frame stores (series_union.h): the host twins over a traits type T -- the local checks in element order, std::merge on the key, a
// bisection and copies for the split -- and the host store built on them.  Host only: no HIP call.  mcpe_union.cpp,
// frame_photon_union.cpp and pmt_hit_union.cpp instantiate them under their exported names; the kernels, the device calls and the
// device store are in series_union_device.hip.h.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "host_model.h"
#include "series_union.h"

namespace clsimhip {

// what is wrong with a series form: throws, with text that names the first offending element (`what`: "A", "B", "the bunch" ...)
template <class T>
void series_form_check(const char *what, const typename T::Record *records, size_t n, const typename T::Entry *series, size_t n_series)
{
    const std::string name = std::string(T::kStore) + ": " + what;
    if (n > 0xffffffffull || n_series > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, name + " holds more than 2^32 - 1 records or series");
    if (n && !records) throw Error(CLSIMHIP_ERR_ARGUMENT, name + ": records is (null)");
    if (n_series && !series) throw Error(CLSIMHIP_ERR_ARGUMENT, name + ": series is (null)");
    const uint32_t ns = static_cast<uint32_t>(n_series), nr = static_cast<uint32_t>(n);
    for (uint32_t s = 0; s < ns; ++s)
        if (!T::entry_ok(series, ns, nr, s))
            throw Error(CLSIMHIP_ERR_ARGUMENT, name + " is no series form: entry " + std::to_string(s) + " of " + std::to_string(ns) + " (" + T::kEntryRule +
                                                   ", and the last entry must end at " + std::to_string(nr) + " records)");
    for (uint32_t i = 0; i < nr; ++i) {
        uint32_t frame;
        if (!T::record_ok(records, series, ns, i, &frame))
            throw Error(CLSIMHIP_ERR_ARGUMENT, name + " is no series form: record " + std::to_string(i) + " of " + std::to_string(nr) + " (" + T::kRecordRule + ")");
    }
}

template <class T>
struct UnionKeyed { typename T::Key key; uint32_t at; };

template <class T>
void series_union_keys(const typename T::Record *records, const typename T::Entry *series, size_t n_series, std::vector<UnionKeyed<T>> &out)
{
    for (size_t s = 0; s < n_series; ++s)
        for (uint32_t i = series[s].first; i < series[s].first + series[s].count; ++i) out.push_back(UnionKeyed<T>{T::key_of(series[s].frame, records, i), i});
}

template <class T>
void series_union_host(const typename T::Record *a_records, size_t n_a, const typename T::Entry *a_series, size_t n_series_a, const typename T::Record *b_records,
                       size_t n_b, const typename T::Entry *b_series, size_t n_series_b, typename T::Record *out_records, typename T::Entry *out_series,
                       size_t out_capacity, size_t *n, size_t *n_series)
{
    using Keyed = UnionKeyed<T>;
    const std::string store = T::kStore;
    series_form_check<T>("A", a_records, n_a, a_series, n_series_a);
    series_form_check<T>("B", b_records, n_b, b_series, n_series_b);
    if (n_a + n_b > out_capacity)
        throw Error(CLSIMHIP_ERR_ARGUMENT, store + ": the union holds " + std::to_string(n_a + n_b) + " records, the output " + std::to_string(out_capacity));
    if (n_a + n_b > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, store + ": the union holds more than 2^32 - 1 records");
    if (n_a + n_b && (!out_records || !out_series)) throw Error(CLSIMHIP_ERR_ARGUMENT, "out_records / out_series is (null)");
    std::vector<Keyed> a, b, merged(n_a + n_b);
    a.reserve(n_a); b.reserve(n_b);
    series_union_keys<T>(a_records, a_series, n_series_a, a);
    series_union_keys<T>(b_records, b_series, n_series_b, b);
    for (Keyed &k : b) k.at += static_cast<uint32_t>(n_a);              // (marks B; n_a + n_b < 2^32)
    // std::merge takes the first range's element where neither is less: ties take A's record first
    std::merge(a.begin(), a.end(), b.begin(), b.end(), merged.begin(), [](const Keyed &x, const Keyed &y) { return union_key_less<T>(x.key, y.key); });
    size_t made = 0;
    for (size_t i = 0; i < merged.size(); ++i) {
        const Keyed &k = merged[i];
        out_records[i] = k.at < n_a ? a_records[k.at] : b_records[k.at - n_a];
        if (i == 0 || !std::equal(k.key.w, k.key.w + T::kChannelWords, merged[i - 1].key.w)) {      // a new channel: a new entry
            T::open_entry(out_series[made++], k.key.w[0], out_records[i]);
            out_series[made - 1].first = static_cast<uint32_t>(i);
        }
        ++out_series[made - 1].count;
    }
    if (n) *n = merged.size();
    if (n_series) *n_series = made;
}

template <class T>
void series_split_host(const typename T::Record *records, size_t n, const typename T::Entry *series, size_t n_series, uint32_t last_frame,
                       typename T::Record *head_records, typename T::Entry *head_series, size_t head_capacity, size_t *n_head, size_t *n_series_head,
                       typename T::Record *tail_records, typename T::Entry *tail_series, size_t tail_capacity, size_t *n_tail, size_t *n_series_tail)
{
    const std::string store = T::kStore;
    series_form_check<T>("the input of the split", records, n, series, n_series);
    const size_t h = union_split_entries(series, static_cast<uint32_t>(n_series), last_frame);
    const size_t head = h < n_series ? series[h].first : n;
    if (head > head_capacity)
        throw Error(CLSIMHIP_ERR_ARGUMENT, store + ": the head holds " + std::to_string(head) + " records, its output " + std::to_string(head_capacity));
    if (n - head > tail_capacity)
        throw Error(CLSIMHIP_ERR_ARGUMENT, store + ": the tail holds " + std::to_string(n - head) + " records, its output " + std::to_string(tail_capacity));
    if (head && (!head_records || !head_series)) throw Error(CLSIMHIP_ERR_ARGUMENT, "head_records / head_series is (null)");
    if (n - head && (!tail_records || !tail_series)) throw Error(CLSIMHIP_ERR_ARGUMENT, "tail_records / tail_series is (null)");
    if (head) std::copy(records, records + head, head_records);
    if (h) std::copy(series, series + h, head_series);
    if (n - head) std::copy(records + head, records + n, tail_records);
    for (size_t s = h; s < n_series; ++s) {
        tail_series[s - h] = series[s];
        tail_series[s - h].first -= static_cast<uint32_t>(head);
    }
    if (n_head) *n_head = head;
    if (n_series_head) *n_series_head = h;
    if (n_tail) *n_tail = n - head;
    if (n_series_tail) *n_series_tail = n_series - h;
}

template <class T>
class HostFrameStoreOf final : public FrameStoreOf<T> {
public:
    using Record = typename T::Record;
    using Entry = typename T::Entry;
    explicit HostFrameStoreOf(size_t capacity) : capacity_(capacity) {}
    bool on_device() const override { return false; }
    void add_host(const Record *records, size_t n, const Entry *series, size_t n_series) override
    {
        series_form_check<T>("the bunch", records, n, series, n_series);
        if (records_.size() + n > capacity_)
            throw Error(CLSIMHIP_ERR_ARGUMENT, std::string(T::kStore) + ": a bunch of " + std::to_string(n) + " records does not fit behind " +
                                                   std::to_string(records_.size()) + " in a store of " + std::to_string(capacity_));
        std::vector<Record> out(records_.size() + n);
        std::vector<Entry> table(records_.size() + n);
        size_t made = 0, entries = 0;
        series_union_host<T>(records_.data(), records_.size(), series_.data(), series_.size(), records, n, series, n_series, out.data(), table.data(), out.size(), &made,
                             &entries);
        table.resize(entries);
        records_.swap(out);
        series_.swap(table);
    }
    void add_device(const void *, const void *, const void *, size_t, hipStream_t) override
    {
        throw Error(CLSIMHIP_ERR_STATE, std::string(T::kStore) + ": a host store takes no device bunch");
    }
    void drain_device(uint32_t, void *, void *, void *, size_t, hipStream_t) override
    {
        throw Error(CLSIMHIP_ERR_STATE, std::string(T::kStore) + ": a host store drains to the host");
    }
    void drain_host(uint32_t last_frame, Record *records, Entry *series, size_t capacity, size_t *n, size_t *n_series) override
    {
        size_t head = 0, h = 0;
        size(last_frame, &head, &h);
        if (head > capacity)
            throw Error(CLSIMHIP_ERR_ARGUMENT, std::string(T::kStore) + ": the frames up to " + std::to_string(last_frame) + " hold " + std::to_string(head) +
                                                   " records, the output " + std::to_string(capacity));
        std::vector<Record> tail(records_.size() - head);
        std::vector<Entry> table(series_.size() - h);
        series_split_host<T>(records_.data(), records_.size(), series_.data(), series_.size(), last_frame, records, series, capacity, n, n_series, tail.data(),
                             table.data(), tail.size(), nullptr, nullptr);
        records_.swap(tail);
        series_.swap(table);
    }
    void size(uint32_t last_frame, size_t *n, size_t *n_series) override
    {
        const size_t h = union_split_entries(series_.data(), static_cast<uint32_t>(series_.size()), last_frame);
        if (n) *n = h < series_.size() ? series_[h].first : records_.size();
        if (n_series) *n_series = h;
    }
private:
    size_t capacity_;
    std::vector<Record> records_;
    std::vector<Entry> series_;
};

// (the device store's maker checks the same bound with the same words: series_union_device.hip.h)
template <class T>
void frame_store_capacity_check(size_t capacity)
{
    if (capacity > kFrameStoreMaxCapacity) throw Error(CLSIMHIP_ERR_ARGUMENT, std::string(T::kStore) + ": capacity beyond 2^31 records");
}

template <class T>
std::unique_ptr<FrameStoreOf<T>> make_host_frame_store_of(size_t capacity)
{
    frame_store_capacity_check<T>(capacity);
    return std::unique_ptr<FrameStoreOf<T>>(new HostFrameStoreOf<T>(capacity));
}

} // namespace clsimhip
