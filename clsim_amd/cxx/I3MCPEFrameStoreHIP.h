// The MCPE frame store (include/clsimhip.h, "MCPE frame store") for a C++ client: what stands where the reference's client module
// keeps its frame cache across bunches (private/clsim/I3CLSimClientModule.cxx:359-439) and commits the oldest frames no bunch in
// flight can still touch (FlushFrameCache, :686-758).  Header-only over the C ABI.
//
//   I3MCPEFrameStoreHIP store(capacity);                // host store; I3MCPEFrameStoreHIP(capacity, 0): the state lives on GPU 0
//   ... per result:   store.Add(conv.GetLastMCPEs(), conv.GetLastMCPESeries());
//   ... per flush:    frames = store.Drain(lastFrame);  // lastFrame: the last frame no bunch in flight can still touch
#ifndef I3MCPEFRAMESTOREHIP_H_INCLUDED
#define I3MCPEFRAMESTOREHIP_H_INCLUDED

#include <cstdint>
#include <map>
#include <utility>
#include <vector>

#include "I3CLSimStepToPhotonConverterHIP.h"

class I3MCPEFrameStoreHIP {
public:
    typedef I3CLSimStepToPhotonConverterHIP::MCPESeriesMap MCPESeriesMap;
    typedef I3CLSimStepToPhotonConverterHIP::MergedMCPESeriesMap MergedMCPESeriesMap;
    typedef I3CLSimStepToPhotonConverterHIP::ParticleIDMap ParticleIDMap;
    static const uint32_t AllFrames = 0xFFFFFFFFu;

    // device < 0: a host store, which needs no GPU
    explicit I3MCPEFrameStoreHIP(size_t capacity, int device = -1) : handle_(nullptr) { check(clsimhip_mcpe_frame_store_create(device, capacity, &handle_)); }
    ~I3MCPEFrameStoreHIP() { clsimhip_mcpe_frame_store_destroy(handle_); }
    I3MCPEFrameStoreHIP(const I3MCPEFrameStoreHIP &) = delete;
    I3MCPEFrameStoreHIP &operator=(const I3MCPEFrameStoreHIP &) = delete;

    // one result: the flat views the converter adapter hands out for its last result (GetLastMCPEs(), GetLastMCPESeries())
    void Add(const std::vector<clsimhip_mcpe> &records, const std::vector<clsimhip_mcpe_series> &series)
    {
        check(clsimhip_mcpe_frame_store_add_host(handle_, records.data(), records.size(), series.data(), series.size()));
    }
    // one result that stayed in HBM (device store only; asynchronous on hipStream)
    void AddDevice(const void *dRecords, const void *dSeries, const void *dSeriesCounts, size_t capacity, void *hipStream = nullptr)
    {
        check(clsimhip_mcpe_frame_store_add_device(handle_, dRecords, dSeries, dSeriesCounts, capacity, hipStream));
    }
    // records and series the frames up to lastFrame hold
    std::pair<size_t, size_t> Size(uint32_t lastFrame = AllFrames) const
    {
        size_t n = 0, nSeries = 0;
        check(clsimhip_mcpe_frame_store_size(handle_, lastFrame, &n, &nSeries));
        return std::make_pair(n, nSeries);
    }
    // the flat form of the frames up to lastFrame, which leave the store
    void DrainFlat(uint32_t lastFrame, std::vector<clsimhip_mcpe> &records, std::vector<clsimhip_mcpe_series> &series)
    {
        const std::pair<size_t, size_t> sizes = Size(lastFrame);
        records.resize(sizes.first);
        series.resize(sizes.second);
        size_t n = 0, nSeries = 0;
        check(clsimhip_mcpe_frame_store_drain_host(handle_, lastFrame, records.data(), series.data(), sizes.first, &n, &nSeries));
        records.resize(n);
        series.resize(nSeries);
    }
    // ... as the frames receive them: frame -> (string ID, OM ID) -> time-ordered MCPEs, the structure of GetLastMCPESeriesMaps()
    std::map<uint32_t, MCPESeriesMap> Drain(uint32_t lastFrame = AllFrames)
    {
        std::vector<clsimhip_mcpe> records;
        std::vector<clsimhip_mcpe_series> series;
        DrainFlat(lastFrame, records, series);
        std::map<uint32_t, MCPESeriesMap> frames;
        for (const clsimhip_mcpe_series &s : series)
            frames[s.frame][std::make_pair(static_cast<int>(s.string_id), static_cast<unsigned>(s.om_id))].assign(records.begin() + s.first, records.begin() + s.first + s.count);
        return frames;
    }
    // ... merged within `window` (include/clsimhip.h, "MCPE merging"), with the particle-ID maps: the structures of
    // GetLastMergedMCPESeriesMaps() and GetLastParticleIDMaps()
    std::pair<std::map<uint32_t, MergedMCPESeriesMap>, std::map<uint32_t, ParticleIDMap> > DrainMerged(uint32_t lastFrame, double window)
    {
        std::vector<clsimhip_mcpe> records;
        std::vector<clsimhip_mcpe_series> series;
        DrainFlat(lastFrame, records, series);
        std::vector<clsimhip_mcpe_merged> merged(records.size());
        std::vector<clsimhip_mcpe_parent> parents(records.size());
        std::vector<clsimhip_mcpe_series> mergedSeries(series.size());
        std::vector<clsimhip_mcpe_parent_range> ranges(series.size());
        size_t nMerged = 0, nParents = 0;
        check(clsimhip_mcpe_merge_host(records.data(), records.size(), series.data(), series.size(), window, merged.data(), mergedSeries.data(), parents.data(),
                                       ranges.data(), &nMerged, &nParents));
        std::pair<std::map<uint32_t, MergedMCPESeriesMap>, std::map<uint32_t, ParticleIDMap> > out;
        for (size_t k = 0; k < mergedSeries.size(); ++k) {
            const clsimhip_mcpe_series &s = mergedSeries[k];
            const std::pair<int, unsigned> key = std::make_pair(static_cast<int>(s.string_id), static_cast<unsigned>(s.om_id));
            out.first[s.frame][key].assign(merged.begin() + s.first, merged.begin() + s.first + s.count);
            std::map<uint32_t, std::vector<uint32_t> > &dom = out.second[s.frame][key];
            for (uint32_t i = ranges[k].first; i < ranges[k].first + ranges[k].count; ++i) dom[parents[i].identifier].push_back(parents[i].index);
        }
        return out;
    }

private:
    void check(int rc) const
    {
        if (rc != CLSIMHIP_OK) throw I3CLSimStepToPhotonConverter_exception(clsimhip_mcpe_frame_store_last_error(handle_));
    }
    clsimhip_mcpe_frame_store *handle_;
};

#endif
