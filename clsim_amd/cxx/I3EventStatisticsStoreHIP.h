// The event statistics frame store (include/clsimhip.h, "Event statistics frame store") for a C++ client of segmented modules: what
// stands where the reference's client module keeps one I3CLSimEventStatistics per frame across bunches and files it when the frame
// is flushed (private/clsim/I3CLSimClientModule.cxx:513-520, 386-405, 728-740), with the slices of a muon folded into the muon
// (I3MuonSliceRemoverAndPulseRelabeler).  Header-only over the C ABI.
//
//   I3EventStatisticsStoreHIP store(capacity);              // host store; I3EventStatisticsStoreHIP(capacity, 0): the state lives on GPU 0
//   ... per result:   store.Add(conv.GetLastEventStatistics(), relabel);     // relabel: clsimhip_slice_muons' table of the frames in flight
//   ... per flush:    frames = store.Drain(lastFrame);      // lastFrame: the last frame no bunch in flight can still touch
#ifndef I3EVENTSTATISTICSSTOREHIP_H_INCLUDED
#define I3EVENTSTATISTICSSTOREHIP_H_INCLUDED

#include <cstdint>
#include <map>
#include <vector>

#include "I3CLSimStepToPhotonConverterHIP.h"

class I3EventStatisticsStoreHIP {
public:
    // what I3CLSimEventStatistics holds per particle: counts, and the weight sums as binary64 (clsimhip_event_statistics_weight: the exact
    // integer rounded once)
    struct ParticleStatistics {
        uint64_t numPhotonsGenerated, numPhotonsAtDOMs;
        double sumOfWeightsPhotonsGenerated, sumOfWeightsPhotonsAtDOMs;
    };
    typedef std::map<uint32_t, ParticleStatistics> ParticleMap;         // particle identifier -> its statistics
    typedef std::vector<clsimhip_relabel> RelabelMap;
    static const uint32_t AllFrames = 0xFFFFFFFFu;

    // device < 0: a host store, which needs no GPU
    explicit I3EventStatisticsStoreHIP(size_t capacity, int device = -1) : handle_(nullptr) { check(clsimhip_event_statistics_store_create(device, capacity, &handle_)); }
    ~I3EventStatisticsStoreHIP() { clsimhip_event_statistics_store_destroy(handle_); }
    I3EventStatisticsStoreHIP(const I3EventStatisticsStoreHIP &) = delete;
    I3EventStatisticsStoreHIP &operator=(const I3EventStatisticsStoreHIP &) = delete;

    // one result: the view the converter adapter hands out for its last result (GetLastEventStatistics()), zeros included, and the
    // relabel map that folds slices into their muons (may be empty)
    void Add(const std::vector<clsimhip_event_statistics> &records, const RelabelMap &relabel = RelabelMap())
    {
        check(clsimhip_event_statistics_store_add_host(handle_, records.data(), records.size(), relabel.data(), relabel.size()));
    }
    // one result that stayed in HBM (device store only; asynchronous on hipStream): dCount is one uint32, word 3 of
    // clsimhip_event_statistics_device's d_counters
    void AddDevice(const void *dRecords, const void *dCount, size_t capacity, const RelabelMap &relabel = RelabelMap(), void *hipStream = nullptr)
    {
        check(clsimhip_event_statistics_store_add_device(handle_, dRecords, dCount, capacity, relabel.data(), relabel.size(), hipStream));
    }
    // records the frames up to lastFrame hold, before a drain's map folds them
    size_t Size(uint32_t lastFrame = AllFrames) const
    {
        size_t n = 0;
        check(clsimhip_event_statistics_store_size(handle_, lastFrame, &n));
        return n;
    }
    // the records of the frames up to lastFrame under the map, which leave the store
    void DrainFlat(uint32_t lastFrame, std::vector<clsimhip_event_statistics> &records, const RelabelMap &relabel = RelabelMap())
    {
        const size_t size = Size(lastFrame);
        records.resize(size);
        size_t n = 0;
        check(clsimhip_event_statistics_store_drain_host(handle_, lastFrame, relabel.data(), relabel.size(), records.data(), size, &n));
        records.resize(n);
    }
    // ... as the frames receive them: frame -> particle -> (counts, weights), an I3CLSimEventStatistics per frame
    std::map<uint32_t, ParticleMap> Drain(uint32_t lastFrame = AllFrames, const RelabelMap &relabel = RelabelMap())
    {
        std::vector<clsimhip_event_statistics> records;
        DrainFlat(lastFrame, records, relabel);
        std::map<uint32_t, ParticleMap> frames;
        for (const clsimhip_event_statistics &r : records) {
            const ParticleStatistics s = {r.generated_count, r.at_doms_count, clsimhip_event_statistics_weight(r.generated_sum, r.generated_special),
                                          clsimhip_event_statistics_weight(r.at_doms_sum, r.at_doms_special)};
            frames[r.frame][r.identifier] = s;
        }
        return frames;
    }

private:
    void check(int rc) const
    {
        if (rc != CLSIMHIP_OK) throw I3CLSimStepToPhotonConverter_exception(clsimhip_event_statistics_store_last_error(handle_));
    }
    clsimhip_event_statistics_store *handle_;
};

#endif
