// The PMT hit frame store (include/clsimhip.h, "PMT hit frame store") for a C++ client of segmented modules: what stands where the
// reference's client module keeps its frame cache across bunches (private/clsim/I3CLSimClientModule.cxx:359-439) and commits the
// oldest frames no bunch in flight can still touch (FlushFrameCache, :686-758).  Header-only over the C ABI.
//
//   I3PMTHitFrameStoreHIP store(capacity);              // host store; I3PMTHitFrameStoreHIP(capacity, 0): the state lives on GPU 0
//   ... per result:   store.Add(conv.GetLastPMTHits(), conv.GetLastPMTSeries());
//   ... per flush:    frames = store.Drain(lastFrame);  // lastFrame: the last frame no bunch in flight can still touch
#ifndef I3PMTHITFRAMESTOREHIP_H_INCLUDED
#define I3PMTHITFRAMESTOREHIP_H_INCLUDED

#include <cstdint>
#include <map>
#include <utility>
#include <vector>

#include "I3CLSimStepToPhotonConverterHIP.h"

class I3PMTHitFrameStoreHIP {
public:
    typedef I3CLSimStepToPhotonConverterHIP::PMTHitSeriesMap PMTHitSeriesMap;
    static const uint32_t AllFrames = 0xFFFFFFFFu;

    // device < 0: a host store, which needs no GPU
    explicit I3PMTHitFrameStoreHIP(size_t capacity, int device = -1) : handle_(nullptr) { check(clsimhip_pmt_hit_store_create(device, capacity, &handle_)); }
    ~I3PMTHitFrameStoreHIP() { clsimhip_pmt_hit_store_destroy(handle_); }
    I3PMTHitFrameStoreHIP(const I3PMTHitFrameStoreHIP &) = delete;
    I3PMTHitFrameStoreHIP &operator=(const I3PMTHitFrameStoreHIP &) = delete;

    // one result: the flat views the converter adapter hands out for its last result (GetLastPMTHits(), GetLastPMTSeries())
    void Add(const std::vector<clsimhip_pmt_hit> &records, const std::vector<clsimhip_pmt_series> &series)
    {
        check(clsimhip_pmt_hit_store_add_host(handle_, records.data(), records.size(), series.data(), series.size()));
    }
    // one result that stayed in HBM (device store only; asynchronous on hipStream)
    void AddDevice(const void *dRecords, const void *dSeries, const void *dSeriesCounts, size_t capacity, void *hipStream = nullptr)
    {
        check(clsimhip_pmt_hit_store_add_device(handle_, dRecords, dSeries, dSeriesCounts, capacity, hipStream));
    }
    // records and series the frames up to lastFrame hold
    std::pair<size_t, size_t> Size(uint32_t lastFrame = AllFrames) const
    {
        size_t n = 0, nSeries = 0;
        check(clsimhip_pmt_hit_store_size(handle_, lastFrame, &n, &nSeries));
        return std::make_pair(n, nSeries);
    }
    // the flat form of the frames up to lastFrame, which leave the store
    void DrainFlat(uint32_t lastFrame, std::vector<clsimhip_pmt_hit> &records, std::vector<clsimhip_pmt_series> &series)
    {
        const std::pair<size_t, size_t> sizes = Size(lastFrame);
        records.resize(sizes.first);
        series.resize(sizes.second);
        size_t n = 0, nSeries = 0;
        check(clsimhip_pmt_hit_store_drain_host(handle_, lastFrame, records.data(), series.data(), sizes.first, &n, &nSeries));
        records.resize(n);
        series.resize(nSeries);
    }
    // ... as the frames receive them: frame -> (string ID, OM ID) -> PMT -> time-ordered hits (an I3MCHitSeriesMultiOMMap per frame),
    // the structure of GetLastPMTSeriesMaps()
    std::map<uint32_t, PMTHitSeriesMap> Drain(uint32_t lastFrame = AllFrames)
    {
        std::vector<clsimhip_pmt_hit> records;
        std::vector<clsimhip_pmt_series> series;
        DrainFlat(lastFrame, records, series);
        std::map<uint32_t, PMTHitSeriesMap> frames;
        for (const clsimhip_pmt_series &s : series)
            frames[s.frame][std::make_pair(static_cast<int>(s.string_id), static_cast<unsigned>(s.om_id))][s.pmt].assign(records.begin() + s.first,
                                                                                                                        records.begin() + s.first + s.count);
        return frames;
    }

private:
    void check(int rc) const
    {
        if (rc != CLSIMHIP_OK) throw I3CLSimStepToPhotonConverter_exception(clsimhip_pmt_hit_store_last_error(handle_));
    }
    clsimhip_pmt_hit_store *handle_;
};

#endif
