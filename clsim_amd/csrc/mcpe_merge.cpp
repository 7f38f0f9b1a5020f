// MCPE merging (mcpe_merge.h): the host twin -- a sequential walk over every series, std::sort and std::unique for the parents.
// Host only: no HIP call.  The kernels and the host side of the device stage are in mcpe_merge_kernel.hip.
#include "mcpe_merge.h"

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "host_model.h"

namespace clsimhip {

void mcpe_merge_host(const clsimhip_mcpe *records, size_t n, const clsimhip_mcpe_series *series, size_t n_series, double window,
                     clsimhip_mcpe_merged *out_merged, clsimhip_mcpe_series *out_series, clsimhip_mcpe_parent *out_parents,
                     clsimhip_mcpe_parent_range *out_ranges, size_t *n_merged, size_t *n_parents)
{
    if (!merge_window_ok(window)) throw Error(CLSIMHIP_ERR_ARGUMENT, "MCPE merging: the window must be a number with 0 <= window < +inf");
    if (n > 0xffffffffull || n_series > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "more than 2^32 - 1 records or series");
    if (n && (!records || !out_merged || !out_parents)) throw Error(CLSIMHIP_ERR_ARGUMENT, "records / out_merged / out_parents is (null)");
    if (n_series && (!series || !out_series || !out_ranges)) throw Error(CLSIMHIP_ERR_ARGUMENT, "series / out_series / out_ranges is (null)");
    size_t covered = 0;
    for (size_t s = 0; s < n_series; ++s) {
        if (series[s].first != covered || series[s].count == 0u || series[s].count > n - covered)
            throw Error(CLSIMHIP_ERR_ARGUMENT, "MCPE merging: the series table does not partition the records into non-empty series (entry " + std::to_string(s) + ")");
        covered += series[s].count;
    }
    if (covered != n) throw Error(CLSIMHIP_ERR_ARGUMENT, "MCPE merging: the series table covers " + std::to_string(covered) + " of " + std::to_string(n) + " records");
    size_t merged = 0, parents = 0;
    std::vector<std::pair<uint32_t, uint32_t>> pairs;       // (identifier, index of the group within the series)
    for (size_t s = 0; s < n_series; ++s) {
        const size_t first_group = merged;
        double T = 0.;
        pairs.clear();
        for (size_t i = series[s].first; i < static_cast<size_t>(series[s].first) + series[s].count; ++i) {
            const clsimhip_mcpe &r = records[i];
            if (i == series[s].first || merge_opens(r.time, T, window)) {
                T = r.time;
                clsimhip_mcpe_merged &m = out_merged[merged++];
                m.npe = 0u;
                m.string_id = r.string_id; m.om_id = r.om_id;
                m.time = T;
            }
            ++out_merged[merged - 1].npe;
            pairs.emplace_back(r.identifier, static_cast<uint32_t>(merged - 1 - first_group));
        }
        std::sort(pairs.begin(), pairs.end());
        pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
        out_series[s] = series[s];
        out_series[s].first = static_cast<uint32_t>(first_group);
        out_series[s].count = static_cast<uint32_t>(merged - first_group);
        out_ranges[s].first = static_cast<uint32_t>(parents);
        out_ranges[s].count = static_cast<uint32_t>(pairs.size());
        for (const auto &p : pairs) {
            out_parents[parents].identifier = p.first;
            out_parents[parents].index = p.second;
            ++parents;
        }
    }
    if (n_merged) *n_merged = merged;
    if (n_parents) *n_parents = parents;
}

} // namespace clsimhip
