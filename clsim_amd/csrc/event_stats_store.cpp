// Event statistics frame store (event_stats_store.h): the host twins -- CANON as a stable sort on the key and ADD over every run,
// COMBINE as a merge in which equal keys become one record, SPLIT as a bisection and two copies -- and the host store built on them.
// Host only: no HIP call.  The kernels, the device calls and the device store are in event_stats_store_kernel.hip.
#include "event_stats_store.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "host_model.h"

namespace clsimhip {

namespace {

using Record = clsimhip_event_statistics;
const std::string kStore = "event statistics store";

bool is_empty(const Record &r)
{
    uint32_t w[kEventStatsRecordWords];
    std::memcpy(w, &r, sizeof r);
    return event_stats_store_words_empty(w);
}

// CANON into a vector; the counters are RELABELLED and EMPTY_DROPPED
void canonical(const Record *records, size_t n, const clsimhip_relabel *map, size_t n_map, std::vector<Record> &out, uint64_t counters[2])
{
    if (n > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, kStore + ": more than 2^32 - 1 records");
    if (n && !records) throw Error(CLSIMHIP_ERR_ARGUMENT, "records is (null)");
    relabel_map_check(map, n_map);
    struct Keyed { uint64_t key; uint32_t at; };
    std::vector<Keyed> keyed;
    keyed.reserve(n);
    uint64_t relabelled = 0, empty = 0;
    for (size_t i = 0; i < n; ++i) {
        if (is_empty(records[i])) { ++empty; continue; }
        bool hit;
        const uint32_t identifier = event_stats_store_relabel(map, static_cast<uint32_t>(n_map), records[i].identifier, &hit);
        relabelled += hit ? 1u : 0u;
        keyed.push_back(Keyed{event_stats_store_key(identifier, records[i].frame), static_cast<uint32_t>(i)});
    }
    std::stable_sort(keyed.begin(), keyed.end(), [](const Keyed &x, const Keyed &y) { return x.key < y.key; });
    out.clear();
    for (size_t p = 0; p < keyed.size(); ++p) {
        const Record &r = records[keyed[p].at];
        if (p == 0 || keyed[p].key != keyed[p - 1].key) {
            out.push_back(r);
            out.back().identifier = static_cast<uint32_t>(keyed[p].key);
        } else
            event_stats_add(out.back(), r);
    }
    counters[0] = relabelled;
    counters[1] = empty;
}

void combine(const Record *a, size_t n_a, const Record *b, size_t n_b, std::vector<Record> &out)
{
    event_stats_form_check("A", a, n_a);
    event_stats_form_check("B", b, n_b);
    out.clear();
    out.reserve(n_a + n_b);
    size_t i = 0, j = 0;
    while (i < n_a || j < n_b) {
        if (j == n_b || (i < n_a && event_stats_store_key(a[i]) < event_stats_store_key(b[j]))) out.push_back(a[i++]);
        else if (i == n_a || event_stats_store_key(b[j]) < event_stats_store_key(a[i])) out.push_back(b[j++]);
        else {
            out.push_back(a[i++]);
            event_stats_add(out.back(), b[j++]);
        }
    }
}

size_t split_point(const Record *records, size_t n, uint32_t last_frame)
{
    return event_stats_store_split_point([&](uint32_t i) { return event_stats_store_key(records[i]); }, static_cast<uint32_t>(n), last_frame);
}

void deliver(const std::vector<Record> &made, Record *out, size_t capacity, const std::string &what)
{
    if (made.size() > capacity)
        throw Error(CLSIMHIP_ERR_ARGUMENT, kStore + ": " + what + " holds " + std::to_string(made.size()) + " records, the output " + std::to_string(capacity));
    if (!made.empty() && !out) throw Error(CLSIMHIP_ERR_ARGUMENT, "out is (null)");
    if (!made.empty()) std::copy(made.begin(), made.end(), out);
}

class HostEventStatsStore final : public EventStatsStore {
public:
    explicit HostEventStatsStore(size_t capacity) : capacity_(capacity) {}
    bool on_device() const override { return false; }
    void add_host(const Record *records, size_t n, const clsimhip_relabel *map, size_t n_map) override
    {
        std::vector<Record> bunch, both;
        uint64_t counters[2];
        canonical(records, n, map, n_map, bunch, counters);
        combine(records_.data(), records_.size(), bunch.data(), bunch.size(), both);
        if (both.size() > capacity_)
            throw Error(CLSIMHIP_ERR_ARGUMENT, kStore + ": a bunch of " + std::to_string(n) + " records makes " + std::to_string(both.size()) + " behind " +
                                                   std::to_string(records_.size()) + " in a store of " + std::to_string(capacity_));
        records_.swap(both);
    }
    void add_device(const void *, const void *, size_t, const clsimhip_relabel *, size_t, hipStream_t) override
    {
        throw Error(CLSIMHIP_ERR_STATE, kStore + ": a host store takes no device bunch");
    }
    void drain_device(uint32_t, const clsimhip_relabel *, size_t, void *, void *, size_t, hipStream_t) override
    {
        throw Error(CLSIMHIP_ERR_STATE, kStore + ": a host store drains to the host");
    }
    void drain_host(uint32_t last_frame, const clsimhip_relabel *map, size_t n_map, Record *out, size_t capacity, size_t *n) override
    {
        const size_t head = split_point(records_.data(), records_.size(), last_frame);
        if (head > capacity)
            throw Error(CLSIMHIP_ERR_ARGUMENT, kStore + ": the frames up to " + std::to_string(last_frame) + " hold " + std::to_string(head) + " records, the output " +
                                                   std::to_string(capacity));
        std::vector<Record> folded;
        uint64_t counters[2];
        canonical(records_.data(), head, map, n_map, folded, counters);
        deliver(folded, out, capacity, "the drained head");
        records_.erase(records_.begin(), records_.begin() + static_cast<std::ptrdiff_t>(head));
        if (n) *n = folded.size();
    }
    void size(uint32_t last_frame, size_t *n) override
    {
        if (n) *n = split_point(records_.data(), records_.size(), last_frame);
    }
private:
    size_t capacity_;
    std::vector<Record> records_;
};

} // namespace

void event_stats_form_check(const char *what, const clsimhip_event_statistics *records, size_t n)
{
    const std::string name = kStore + ": " + what;
    if (n > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, name + " holds more than 2^32 - 1 records");
    if (n && !records) throw Error(CLSIMHIP_ERR_ARGUMENT, name + ": records is (null)");
    for (size_t i = 0; i < n; ++i) {
        if (is_empty(records[i]))
            throw Error(CLSIMHIP_ERR_ARGUMENT, name + " is no statistics form: record " + std::to_string(i) + " of " + std::to_string(n) + " is empty (no record of a form is)");
        if (i > 0 && !(event_stats_store_key(records[i - 1]) < event_stats_store_key(records[i])))
            throw Error(CLSIMHIP_ERR_ARGUMENT, name + " is no statistics form: record " + std::to_string(i) + " of " + std::to_string(n) +
                                                   " (the records must ascend strictly in (frame, identifier))");
    }
}

void event_stats_canonical_host(const clsimhip_event_statistics *records, size_t n, const clsimhip_relabel *map, size_t n_map, clsimhip_event_statistics *out,
                                size_t capacity, size_t *n_out, uint64_t counters[2])
{
    std::vector<Record> made;
    uint64_t counted[2];
    canonical(records, n, map, n_map, made, counted);
    deliver(made, out, capacity, "the canonical form");
    if (n_out) *n_out = made.size();
    if (counters) { counters[0] = counted[0]; counters[1] = counted[1]; }
}

void event_stats_combine_host(const clsimhip_event_statistics *a, size_t n_a, const clsimhip_event_statistics *b, size_t n_b, clsimhip_event_statistics *out,
                              size_t capacity, size_t *n_out)
{
    std::vector<Record> made;
    combine(a, n_a, b, n_b, made);
    deliver(made, out, capacity, "the combination");
    if (n_out) *n_out = made.size();
}

void event_stats_split_host(const clsimhip_event_statistics *records, size_t n, uint32_t last_frame, clsimhip_event_statistics *head, size_t head_capacity,
                            size_t *n_head, clsimhip_event_statistics *tail, size_t tail_capacity, size_t *n_tail)
{
    event_stats_form_check("the input of the split", records, n);
    const size_t h = split_point(records, n, last_frame);
    if (h > head_capacity) throw Error(CLSIMHIP_ERR_ARGUMENT, kStore + ": the head holds " + std::to_string(h) + " records, its output " + std::to_string(head_capacity));
    if (n - h > tail_capacity)
        throw Error(CLSIMHIP_ERR_ARGUMENT, kStore + ": the tail holds " + std::to_string(n - h) + " records, its output " + std::to_string(tail_capacity));
    if ((h && !head) || (n - h && !tail)) throw Error(CLSIMHIP_ERR_ARGUMENT, "head / tail is (null)");
    if (h) std::copy(records, records + h, head);
    if (n - h) std::copy(records + h, records + n, tail);
    if (n_head) *n_head = h;
    if (n_tail) *n_tail = n - h;
}

std::unique_ptr<EventStatsStore> make_host_event_stats_store(size_t capacity)
{
    if (capacity > kFrameStoreMaxCapacity) throw Error(CLSIMHIP_ERR_ARGUMENT, kStore + ": capacity beyond 2^31 records");
    return std::unique_ptr<EventStatsStore>(new HostEventStatsStore(capacity));
}

} // namespace clsimhip
