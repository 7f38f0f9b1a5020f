// PMT hit frame store (pmt_hit_union.h): the host twins -- the local checks in element order, std::merge on the 6-word key, a
// bisection and copies for the split -- and the host store built on them.  Host only: no HIP call.  The kernels, the device calls
// and the device store are in pmt_hit_union_kernel.hip.
#include "pmt_hit_union.h"

#include <algorithm>
#include <string>
#include <vector>

#include "host_model.h"

namespace clsimhip {

void pmt_hits_form_check(const char *what, const clsimhip_pmt_hit *records, size_t n, const clsimhip_pmt_series *series, size_t n_series)
{
    const std::string name = std::string("PMT hit frame store: ") + what;
    if (n > 0xffffffffull || n_series > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, name + " holds more than 2^32 - 1 records or series");
    if (n && !records) throw Error(CLSIMHIP_ERR_ARGUMENT, name + ": records is (null)");
    if (n_series && !series) throw Error(CLSIMHIP_ERR_ARGUMENT, name + ": series is (null)");
    const uint32_t ns = static_cast<uint32_t>(n_series), nr = static_cast<uint32_t>(n);
    for (uint32_t s = 0; s < ns; ++s)
        if (!pmt_hit_union_entry_ok(series, ns, nr, s))
            throw Error(CLSIMHIP_ERR_ARGUMENT, name + " is no series form: entry " + std::to_string(s) + " of " + std::to_string(ns) +
                                                   " (the table must ascend strictly in (frame, string_id, om_id, pmt), every count > 0, every reserved = 0, first[0] = 0, first[s] = first[s-1] + count[s-1], and the last entry must end at " +
                                                   std::to_string(nr) + " records)");
    for (uint32_t i = 0; i < nr; ++i) {
        uint32_t frame;
        if (!pmt_hit_union_record_ok(records, series, ns, i, &frame))
            throw Error(CLSIMHIP_ERR_ARGUMENT, name + " is no series form: record " + std::to_string(i) + " of " + std::to_string(nr) +
                                                   " (every record must lie in an entry, carry its string_id, om_id and pmt, have reserved = 0, and not descend in (time key, identifier) behind its predecessor)");
    }
}

namespace {
struct Keyed { PmtHitKey key; uint32_t at; };

void keys_of(const clsimhip_pmt_hit *records, const clsimhip_pmt_series *series, size_t n_series, std::vector<Keyed> &out)
{
    for (size_t s = 0; s < n_series; ++s)
        for (uint32_t i = series[s].first; i < series[s].first + series[s].count; ++i)
            out.push_back(Keyed{pmt_hit_union_make_key(series[s].frame, pmt_hit_union_words(records, i)), i});
}
} // namespace

void pmt_hits_union_host(const clsimhip_pmt_hit *a_records, size_t n_a, const clsimhip_pmt_series *a_series, size_t n_series_a, const clsimhip_pmt_hit *b_records,
                         size_t n_b, const clsimhip_pmt_series *b_series, size_t n_series_b, clsimhip_pmt_hit *out_records, clsimhip_pmt_series *out_series,
                         size_t out_capacity, size_t *n, size_t *n_series)
{
    pmt_hits_form_check("A", a_records, n_a, a_series, n_series_a);
    pmt_hits_form_check("B", b_records, n_b, b_series, n_series_b);
    if (n_a + n_b > out_capacity)
        throw Error(CLSIMHIP_ERR_ARGUMENT, "PMT hit frame store: the union holds " + std::to_string(n_a + n_b) + " records, the output " + std::to_string(out_capacity));
    if (n_a + n_b > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "PMT hit frame store: the union holds more than 2^32 - 1 records");
    if (n_a + n_b && (!out_records || !out_series)) throw Error(CLSIMHIP_ERR_ARGUMENT, "out_records / out_series is (null)");
    std::vector<Keyed> a, b, merged(n_a + n_b);
    a.reserve(n_a); b.reserve(n_b);
    keys_of(a_records, a_series, n_series_a, a);
    keys_of(b_records, b_series, n_series_b, b);
    for (Keyed &k : b) k.at += static_cast<uint32_t>(n_a);              // (marks B; n_a + n_b < 2^32)
    // std::merge takes the first range's element where neither is less: ties take A's record first
    std::merge(a.begin(), a.end(), b.begin(), b.end(), merged.begin(), [](const Keyed &x, const Keyed &y) { return pmt_hit_union_key_less(x.key, y.key); });
    size_t made = 0;
    for (size_t i = 0; i < merged.size(); ++i) {
        const Keyed &k = merged[i];
        out_records[i] = k.at < n_a ? a_records[k.at] : b_records[k.at - n_a];
        if (i == 0 || union_words_less(merged[i - 1].key.w, k.key.w, kPmtHitChannelWords)) {    // (ascending: less = differs)
            clsimhip_pmt_series &s = out_series[made++];
            s.frame = k.key.w[0];
            s.string_id = out_records[i].string_id; s.om_id = out_records[i].om_id;
            s.pmt = out_records[i].pmt;
            s.first = static_cast<uint32_t>(i);
            s.count = 0u;
            s.reserved = 0u;
        }
        ++out_series[made - 1].count;
    }
    if (n) *n = merged.size();
    if (n_series) *n_series = made;
}

void pmt_hits_split_host(const clsimhip_pmt_hit *records, size_t n, const clsimhip_pmt_series *series, size_t n_series, uint32_t last_frame,
                         clsimhip_pmt_hit *head_records, clsimhip_pmt_series *head_series, size_t head_capacity, size_t *n_head, size_t *n_series_head,
                         clsimhip_pmt_hit *tail_records, clsimhip_pmt_series *tail_series, size_t tail_capacity, size_t *n_tail, size_t *n_series_tail)
{
    pmt_hits_form_check("the input of the split", records, n, series, n_series);
    const size_t h = pmt_hit_union_split_entries(series, static_cast<uint32_t>(n_series), last_frame);
    const size_t head = h < n_series ? series[h].first : n;
    if (head > head_capacity)
        throw Error(CLSIMHIP_ERR_ARGUMENT, "PMT hit frame store: the head holds " + std::to_string(head) + " records, its output " + std::to_string(head_capacity));
    if (n - head > tail_capacity)
        throw Error(CLSIMHIP_ERR_ARGUMENT, "PMT hit frame store: the tail holds " + std::to_string(n - head) + " records, its output " + std::to_string(tail_capacity));
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

namespace {
class HostPmtHitStore final : public PmtHitStore {
public:
    explicit HostPmtHitStore(size_t capacity) : capacity_(capacity) {}
    bool on_device() const override { return false; }
    void add_host(const clsimhip_pmt_hit *records, size_t n, const clsimhip_pmt_series *series, size_t n_series) override
    {
        pmt_hits_form_check("the bunch", records, n, series, n_series);
        if (records_.size() + n > capacity_)
            throw Error(CLSIMHIP_ERR_ARGUMENT, "PMT hit frame store: a bunch of " + std::to_string(n) + " records does not fit behind " + std::to_string(records_.size()) +
                                                   " in a store of " + std::to_string(capacity_));
        std::vector<clsimhip_pmt_hit> out(records_.size() + n);
        std::vector<clsimhip_pmt_series> table(records_.size() + n);
        size_t made = 0, entries = 0;
        pmt_hits_union_host(records_.data(), records_.size(), series_.data(), series_.size(), records, n, series, n_series, out.data(), table.data(), out.size(), &made,
                            &entries);
        table.resize(entries);
        records_.swap(out);
        series_.swap(table);
    }
    void add_device(const void *, const void *, const void *, size_t, hipStream_t) override
    {
        throw Error(CLSIMHIP_ERR_STATE, "PMT hit frame store: a host store takes no device bunch");
    }
    void drain_device(uint32_t, void *, void *, void *, size_t, hipStream_t) override
    {
        throw Error(CLSIMHIP_ERR_STATE, "PMT hit frame store: a host store drains to the host");
    }
    void drain_host(uint32_t last_frame, clsimhip_pmt_hit *records, clsimhip_pmt_series *series, size_t capacity, size_t *n, size_t *n_series) override
    {
        size_t head = 0, h = 0;
        size(last_frame, &head, &h);
        if (head > capacity)
            throw Error(CLSIMHIP_ERR_ARGUMENT, "PMT hit frame store: the frames up to " + std::to_string(last_frame) + " hold " + std::to_string(head) + " records, the output " +
                                                   std::to_string(capacity));
        std::vector<clsimhip_pmt_hit> tail(records_.size() - head);
        std::vector<clsimhip_pmt_series> table(series_.size() - h);
        pmt_hits_split_host(records_.data(), records_.size(), series_.data(), series_.size(), last_frame, records, series, capacity, n, n_series, tail.data(), table.data(),
                            tail.size(), nullptr, nullptr);
        records_.swap(tail);
        series_.swap(table);
    }
    void size(uint32_t last_frame, size_t *n, size_t *n_series) override
    {
        const size_t h = pmt_hit_union_split_entries(series_.data(), static_cast<uint32_t>(series_.size()), last_frame);
        if (n) *n = h < series_.size() ? series_[h].first : records_.size();
        if (n_series) *n_series = h;
    }
private:
    size_t capacity_;
    std::vector<clsimhip_pmt_hit> records_;
    std::vector<clsimhip_pmt_series> series_;
};
} // namespace

std::unique_ptr<PmtHitStore> make_host_pmt_hit_store(size_t capacity)
{
    if (capacity > kFrameStoreMaxCapacity) throw Error(CLSIMHIP_ERR_ARGUMENT, "PMT hit frame store: capacity beyond 2^31 records");
    return std::unique_ptr<PmtHitStore>(new HostPmtHitStore(capacity));
}

} // namespace clsimhip
