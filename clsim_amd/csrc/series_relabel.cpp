// Series relabel (series_relabel.h): the host twins -- the map's check, a sequential walk over the runs of every series with
// std::stable_sort for the disturbed ones -- and the parent table's relabelling.  Host only: no HIP call.  The kernels and the
// device calls are in series_relabel_kernel.hip.
#include "series_relabel.h"

#include <algorithm>
#include <string>
#include <vector>

#include "host_model.h"

namespace clsimhip {

void relabel_map_check(const clsimhip_relabel *map, size_t n_map)
{
    if (n_map && !map) throw Error(CLSIMHIP_ERR_ARGUMENT, "map is (null)");
    if (n_map > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "series relabel: the map holds more than 2^32 - 1 entries");
    for (size_t k = 1; k < n_map; ++k)
        if (!(map[k].from > map[k - 1].from))
            throw Error(CLSIMHIP_ERR_ARGUMENT, "series relabel: the map is not strictly ascending in `from` (entry " + std::to_string(k) + ")");
    for (size_t k = 0; k < n_map; ++k)                                  // I3MuonSliceRemoverAndPulseRelabeler.cxx:320-332
        if (relabel_find(map, 0u, static_cast<uint32_t>(n_map), map[k].to) >= 0)
            throw Error(CLSIMHIP_ERR_ARGUMENT, "series relabel: entry " + std::to_string(k) + " of the map sends " + std::to_string(map[k].from) + " to " +
                                                   std::to_string(map[k].to) + ", which the map sends on (a muon must not be a slice)");
}

namespace {

bool record_ok(const clsimhip_mcpe *records, const clsimhip_mcpe_series *series, uint32_t n_series, uint32_t i)
{
    uint32_t frame;
    return union_record_ok(records, series, n_series, i, &frame);
}
bool record_ok(const clsimhip_frame_photon *records, const clsimhip_mcpe_series *series, uint32_t n_series, uint32_t i)
{
    uint32_t frame;
    return frame_photon_union_record_ok(records, series, n_series, i, &frame);
}

template <class T>
void relabel_host(const typename T::Record *records, size_t n, const clsimhip_mcpe_series *series, size_t n_series, const clsimhip_relabel *map, size_t n_map,
                  typename T::Record *out, uint64_t counters[2], size_t *n_kept)
{
    using Record = typename T::Record;
    static_assert(sizeof(Record) == T::kWords * sizeof(uint32_t), "a record is its words");
    if (n > 0xffffffffull || n_series > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "series relabel: more than 2^32 - 1 records or series");
    if (n && (!records || !out)) throw Error(CLSIMHIP_ERR_ARGUMENT, "records / out_records is (null)");
    if (n_series && !series) throw Error(CLSIMHIP_ERR_ARGUMENT, "series is (null)");
    relabel_map_check(map, n_map);
    const uint32_t nr = static_cast<uint32_t>(n), ns = static_cast<uint32_t>(n_series), nm = static_cast<uint32_t>(n_map);
    for (uint32_t s = 0; s < ns; ++s)
        if (!union_entry_ok(series, ns, nr, s))
            throw Error(CLSIMHIP_ERR_ARGUMENT, "series relabel: the input is no series form: entry " + std::to_string(s) + " of " + std::to_string(ns));
    if (ns == 0u && nr != 0u) throw Error(CLSIMHIP_ERR_ARGUMENT, "series relabel: the input is no series form: records without a table");
    for (uint32_t i = 0; i < nr; ++i)
        if (!record_ok(records, series, ns, i))
            throw Error(CLSIMHIP_ERR_ARGUMENT, "series relabel: the input is no series form: record " + std::to_string(i) + " of " + std::to_string(nr));
    const auto words = [&](uint32_t i) { return reinterpret_cast<const uint32_t *>(records + i); };
    std::vector<uint32_t> ids(nr);
    uint64_t relabelled = 0, overflow = 0;
    for (uint32_t i = 0; i < nr; ++i) {
        const int64_t k = relabel_find(map, 0u, nm, words(i)[0]);
        ids[i] = k < 0 ? words(i)[0] : map[k].to;
        relabelled += k < 0 ? 0u : 1u;
    }
    const auto put = [&](uint32_t to, uint32_t from) {
        out[to] = records[from];
        out[to].identifier = ids[from];
    };
    std::vector<uint32_t> order;
    for (uint32_t s = 0; s < ns; ++s) {
        const uint32_t end = series[s].first + series[s].count;
        for (uint32_t a = series[s].first, b; a < end; a = b) {
            bool disturbed = false;
            for (b = a + 1u; b < end && relabel_tkey(words(b)) == relabel_tkey(words(a)); ++b)
                disturbed = disturbed || T::rest_less(ids[b], words(b), ids[b - 1u], words(b - 1u));
            if (!disturbed || b - a > kRelabelRunBound) {
                if (disturbed) overflow += b - a;
                for (uint32_t i = a; i < b; ++i) put(i, i);
                continue;
            }
            order.resize(b - a);
            for (uint32_t i = a; i < b; ++i) order[i - a] = i;
            std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return T::rest_less(ids[x], words(x), ids[y], words(y)); });
            for (uint32_t i = a; i < b; ++i) put(i, order[i - a]);
        }
    }
    if (counters) { counters[0] = relabelled; counters[1] = overflow; }
    if (n_kept) *n_kept = overflow ? 0u : n;
}

} // namespace

void mcpe_series_relabel_host(const clsimhip_mcpe *records, size_t n, const clsimhip_mcpe_series *series, size_t n_series, const clsimhip_relabel *map, size_t n_map,
                              clsimhip_mcpe *out_records, uint64_t counters[2], size_t *n_kept)
{
    relabel_host<RelabelMcpe>(records, n, series, n_series, map, n_map, out_records, counters, n_kept);
}

void frame_photons_relabel_host(const clsimhip_frame_photon *records, size_t n, const clsimhip_mcpe_series *series, size_t n_series, const clsimhip_relabel *map,
                                size_t n_map, clsimhip_frame_photon *out_records, uint64_t counters[2], size_t *n_kept)
{
    relabel_host<RelabelFramePhoton>(records, n, series, n_series, map, n_map, out_records, counters, n_kept);
}

void mcpe_parents_relabel_host(const clsimhip_mcpe_parent *parents, const clsimhip_mcpe_parent_range *ranges, size_t n_series, const clsimhip_relabel *map, size_t n_map,
                               clsimhip_mcpe_parent *out, clsimhip_mcpe_parent_range *out_ranges, size_t *n_out)
{
    if (n_series && (!ranges || !out_ranges)) throw Error(CLSIMHIP_ERR_ARGUMENT, "ranges / out_ranges is (null)");
    relabel_map_check(map, n_map);
    uint64_t total = 0;
    for (size_t s = 0; s < n_series; ++s) {
        if (ranges[s].first != total)
            throw Error(CLSIMHIP_ERR_ARGUMENT, "series relabel: parent range " + std::to_string(s) + " does not start where its predecessor ends");
        total += ranges[s].count;
    }
    if (total > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "series relabel: more than 2^32 - 1 parent entries");
    if (total && (!parents || !out)) throw Error(CLSIMHIP_ERR_ARGUMENT, "parents / out is (null)");
    std::vector<clsimhip_mcpe_parent> one;
    uint32_t made = 0;
    for (size_t s = 0; s < n_series; ++s) {
        one.assign(parents + ranges[s].first, parents + ranges[s].first + ranges[s].count);
        for (clsimhip_mcpe_parent &p : one) {
            const int64_t k = relabel_find(map, 0u, static_cast<uint32_t>(n_map), p.identifier);
            if (k >= 0) p.identifier = map[k].to;
        }
        std::sort(one.begin(), one.end(), [](const clsimhip_mcpe_parent &a, const clsimhip_mcpe_parent &b) {
            return a.identifier != b.identifier ? a.identifier < b.identifier : a.index < b.index;
        });
        one.erase(std::unique(one.begin(), one.end(), [](const clsimhip_mcpe_parent &a, const clsimhip_mcpe_parent &b) { return a.identifier == b.identifier && a.index == b.index; }),
                  one.end());
        out_ranges[s].first = made;
        out_ranges[s].count = static_cast<uint32_t>(one.size());
        std::copy(one.begin(), one.end(), out + made);
        made += static_cast<uint32_t>(one.size());
    }
    if (n_out) *n_out = made;
}

} // namespace clsimhip
