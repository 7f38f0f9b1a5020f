// PMT photon hits on the host: see pmt_photon_hits.h.  The host twin and the device call of the multi-PMT hit generator
// (pmt_hits.h: PmtHitGenerator, whose tables and device image the stage reads), the kernels in pmt_photon_hits_kernel.hip.
#include "pmt_photon_hits.h"

#include <algorithm>
#include <cstring>

#include "series_bunch.h"

namespace clsimhip {

size_t pmt_photon_hits_workspace_bytes(size_t capacity) { return SeriesWorkspaceLayout(capacity, 0u).bytes; }

void PmtHitGenerator::photon_hits_host(const clsimhip_frame_photon *records, size_t n, const clsimhip_mcpe_series *series, size_t n_series, clsimhip_pmt_hit *out,
                                       clsimhip_pmt_series *out_series, size_t *n_kept, size_t *n_series_out, uint64_t counters[5]) const
{
    if (n_series > kPmtPhotonHitMaxSeries) throw Error(CLSIMHIP_ERR_ARGUMENT, "more than 2^26 series: series x 64 + PMT number does not fit 32 bits");
    if (n && (!records || !out || !out_series)) throw Error(CLSIMHIP_ERR_ARGUMENT, "records / out / out_series is (null)");
    if (n_series && !series) throw Error(CLSIMHIP_ERR_ARGUMENT, "series is (null)");
    if (n > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "more than 2^32 - 1 records");
    PmtPhotonHitLookup L{};
    L.series = series;
    L.n_series = static_cast<uint32_t>(n_series);
    std::vector<SeriesKey> keys;
    keys.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        uint32_t w[12];
        std::memcpy(w, records + i, sizeof w);
        SeriesKey k;
        uint32_t pmt = 0u;
        bool off_surface = false;
        const int code = pmt_photon_hit_make(L, params_, values_.data(), pmts_.data(), static_cast<uint32_t>(i), w, k, pmt, off_surface);
        if (code == PMT_PHOTON_HIT_KEPT) keys.push_back(k);
        else if (code != PMT_PHOTON_HIT_DROPPED && counters) ++counters[code];
        if (off_surface && counters) ++counters[PMT_PHOTON_HIT_OFF_SURFACE];
    }
    std::sort(keys.begin(), keys.end(), series_key_less);
    size_t made = 0;
    for (size_t i = 0; i < keys.size(); ++i) {
        const SeriesKey &k = keys[i];
        const clsimhip_mcpe_series &entry = series[k.group / static_cast<uint32_t>(kPmtMaxPerType)];
        const uint32_t pmt = k.group % static_cast<uint32_t>(kPmtMaxPerType);
        clsimhip_pmt_hit &hit = out[i];
        hit.identifier = k.identifier;
        hit.string_id = entry.string_id; hit.om_id = entry.om_id;
        hit.pmt = pmt;
        hit.reserved = 0u;
        const uint64_t bits = pmt_photon_hit_time_bits(k);
        std::memcpy(&hit.time, &bits, sizeof bits);
        if (i == 0 || keys[i - 1].group != k.group) {
            clsimhip_pmt_series &s = out_series[made++];        // (made <= the records kept <= n)
            s.frame = entry.frame;
            s.string_id = entry.string_id; s.om_id = entry.om_id;
            s.pmt = pmt;
            s.first = static_cast<uint32_t>(i);
            s.count = 0u;
            s.reserved = 0u;
        }
        ++out_series[made - 1].count;
    }
    if (n_kept) *n_kept = keys.size();
    if (n_series_out) *n_series_out = made;
}

void PmtHitGenerator::photon_hits_device(int device, const void *d_records, const void *d_series, const void *d_in_counts, size_t capacity, void *d_out,
                                         void *d_out_series, void *d_counts, void *d_workspace, size_t workspace_bytes, hipStream_t stream)
{
    if (capacity > kPmtPhotonHitMaxSeries) throw Error(CLSIMHIP_ERR_ARGUMENT, "capacity beyond 2^26 records: series x 64 + PMT number does not fit 32 bits");
    const SeriesWorkspaceLayout W(capacity, 0u);
    check_series_device_args("PMT photon hits", "d_records", 16u, d_records, d_in_counts, capacity, d_out, d_out_series, d_counts, d_workspace, workspace_bytes, W.bytes);
    if (capacity && !d_series) throw Error(CLSIMHIP_ERR_ARGUMENT, "d_series is (null)");
    if (reinterpret_cast<uintptr_t>(d_series) & 15u) throw Error(CLSIMHIP_ERR_ARGUMENT, "d_series must be aligned to 16 bytes");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) throw Error(CLSIMHIP_ERR_DEVICE, "no HIP device available (the PMT photon hits' device path has no CPU fallback)");
    if (device < 0 || device >= count) throw Error(CLSIMHIP_ERR_ARGUMENT, "device ordinal out of range");
    DeviceGuard on_device(device);
    const DeviceImage im = image_on(device);            // (the image convert_device uses: the first call on a device copies the tables there)
    uint8_t *ws = static_cast<uint8_t *>(d_workspace);
    PmtPhotonHitsDeviceArgs A{};
    A.P = params_;
    A.P.values = im.values;
    A.P.pmts = im.pmts;
    A.P.module_table = im.module_table;
    A.P.modules = im.modules;
    A.in_series = static_cast<const clsimhip_mcpe_series *>(d_series);
    A.in = static_cast<const clsimhip_frame_photon *>(d_records);
    A.in_counts = static_cast<const uint32_t *>(d_in_counts);
    A.capacity = static_cast<uint32_t>(capacity);
    // a group is (the index of a series in use) x 64 + a PMT number, below capacity x 64: the bytes of it that can differ between two keys
    A.group_passes = 0u;
    for (uint64_t top = capacity ? capacity * static_cast<uint64_t>(kPmtMaxPerType) - 1u : 0u; top != 0u; top >>= 8) ++A.group_passes;
    set_series_workspace(A, ws, W);
    A.out = static_cast<clsimhip_pmt_hit *>(d_out);
    A.series = static_cast<clsimhip_pmt_series *>(d_out_series);
    A.counts = static_cast<uint32_t *>(d_counts);
    const hipError_t e = launch_pmt_photon_hits(A, stream);
    if (e != hipSuccess) throw Error(CLSIMHIP_ERR_DEVICE, std::string("PMT photon hits kernel launch: ") + hipGetErrorString(e));
}

} // namespace clsimhip
