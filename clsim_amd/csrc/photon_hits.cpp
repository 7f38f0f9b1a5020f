// The photon hit maker object: see photon_hits.h.  Configuration, the efficiency rule and the host twin here, the kernels in
// photon_hits_kernel.hip.
#include "photon_hits.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "series_bunch.h"

namespace clsimhip {

namespace {
std::string dom_name(const PhotonHitDom &d) { return "OM (" + std::to_string(d.string_id) + "/" + std::to_string(d.om_id) + ")"; }

// I3PhotonToMCPEConverter.cxx:327-388: efficiency_from_calibration of one DOM.  Its log_fatals depend on the configuration alone.
double resolve_efficiency(const PhotonHitDom &d, const PhotonHitConfig &K)
{
    const double fallback = K.default_relative_efficiency;
    const char *advice = " (Consider setting \"DefaultRelativeDOMEfficiency\" != NaN)";
    if (K.replace_efficiency_with_default) {                                            // :332-335 (the NaN default: :166-170)
        if (std::isnan(fallback))
            throw Error(CLSIMHIP_ERR_CONFIG, dom_name(d) + ": You need to set \"DefaultRelativeDOMEfficiency\" to a value other than NaN if you enabled "
                                                           "\"ReplaceRelativeDOMEfficiencyWithDefault\"");
        return fallback;
    }
    if ((d.flags & kPhotonHitInCalibration) == 0u) {                                    // :349-357
        if (std::isnan(fallback)) throw Error(CLSIMHIP_ERR_CONFIG, dom_name(d) + " not found in the current calibration map!" + advice);
        return fallback;
    }
    if (std::isnan(d.relative_dom_eff)) {                                               // :370-378: the default, without the SPE factor
        if (std::isnan(fallback)) throw Error(CLSIMHIP_ERR_CONFIG, dom_name(d) + " found in the current calibration map, but it is NaN!" + advice);
        return fallback;
    }
    const double spe = std::isnan(d.spe_compensation_factor) ? 1.0 : d.spe_compensation_factor;      // :360-366
    return d.relative_dom_eff * spe;                                                    // :380
}
} // namespace

size_t photon_hits_workspace_bytes(size_t capacity) { return SeriesWorkspaceLayout(capacity, 0u).bytes; }

PhotonHitMaker::PhotonHitMaker(const std::vector<FunctionData> &classes, const clsimhip_polynomial &angular, const PhotonHitDom *doms, size_t n_doms,
                               const PhotonHitConfig &K)
{
    // (classes, polynomial and their limits: McpeGenerator's, mcpe.cpp)
    if (classes.empty() || classes.size() > static_cast<size_t>(kMcpeMaxClasses))
        throw Error(CLSIMHIP_ERR_ARGUMENT, "a photon hit maker takes 1 ... " + std::to_string(kMcpeMaxClasses) + " wavelength acceptance classes");
    McpeParams &P = params_;
    P.num_classes = static_cast<int32_t>(classes.size());
    for (size_t k = 0; k < classes.size(); ++k) {
        const FunctionData &f = classes[k];
        if (!f.on_device()) throw Error(CLSIMHIP_ERR_CONFIG, "a wavelength acceptance must be a table with equal spacing or a constant");
        McpeClass &c = P.classes[k];
        c.kind = f.kind;
        c.value = f.value;
        if (f.kind == CLSIMHIP_FUNCTION_TABLE) {
            if (!(f.step > 0.) || !std::isfinite(f.step) || !std::isfinite(f.start))
                throw Error(CLSIMHIP_ERR_ARGUMENT, "a wavelength acceptance table needs a finite first wavelength and a positive spacing");
            c.n = static_cast<int32_t>(f.values.size());
            c.offset = static_cast<uint32_t>(values_.size());
            c.start = f.start; c.step = f.step;
            values_.insert(values_.end(), f.values.begin(), f.values.end());
        }
    }
    if (values_.size() > kMcpeMaxTableValues)
        throw Error(CLSIMHIP_ERR_CONFIG, "the wavelength acceptance tables hold more than " + std::to_string(kMcpeMaxTableValues) + " values together");
    P.num_values = static_cast<uint32_t>(values_.size());
    if (angular.n < 0 || angular.n > kMcpeMaxCoefficients || (angular.n > 0 && !angular.coefficients))
        throw Error(CLSIMHIP_ERR_ARGUMENT, "the angular acceptance polynomial has 0 ... " + std::to_string(kMcpeMaxCoefficients) + " coefficients");
    P.num_coefficients = angular.n;
    for (int i = 0; i < angular.n; ++i) P.coefficients[i] = angular.coefficients[i];
    P.range_min = angular.range_min; P.range_max = angular.range_max;
    P.underflow = angular.underflow; P.overflow = angular.overflow;

    if (!(K.dom_radius > 0.) || !(K.oversize > 0.) || !(K.pancake > 0.) || !std::isfinite(K.dom_radius) || !std::isfinite(K.oversize) || !std::isfinite(K.pancake))
        throw Error(CLSIMHIP_ERR_ARGUMENT, "dom_radius, oversize and pancake must be positive and finite");
    if (K.default_relative_efficiency < 0.) throw Error(CLSIMHIP_ERR_CONFIG, "The \"DefaultRelativeDOMEfficiency\" parameter must not be < 0!");      // :172
    // the surface check is made for spherical DOMs only, against the oversized radius (:417-420)
    const double R = K.oversize * K.dom_radius;
    const double lo = (R - 0.03 > 0.) ? R - 0.03 : 0., hi = R + 0.03;
    P.lo2 = lo * lo; P.hi2 = hi * hi;
    P.time_factor = 1. - K.pancake / K.oversize;                                        // :516
    P.seed = K.seed;
    switches_ = (K.ignore_inactive ? kPhotonHitIgnoreInactive : 0u) | (K.only_warn_off_surface ? kPhotonHitOnlyWarn : 0u) |
                (K.pancake == 1. ? kPhotonHitCheckSurface : 0u);

    if (n_doms && !doms) throw Error(CLSIMHIP_ERR_ARGUMENT, "doms is (null)");
    if (n_doms > (size_t{1} << 24)) throw Error(CLSIMHIP_ERR_ARGUMENT, "a photon hit maker takes at most 2^24 DOMs");
    size_t slots = 16;
    while (slots < 2 * n_doms) slots *= 2;
    dom_table_.assign(slots, 0u);
    dom_values_.assign(4u * slots, 0.);
    P.dom_mask = static_cast<uint32_t>(slots - 1);
    for (size_t i = 0; i < n_doms; ++i) {
        const PhotonHitDom &d = doms[i];
        if (d.string_id < -32768 || d.string_id > 32767 || d.om_id > 65535u)
            throw Error(CLSIMHIP_ERR_ARGUMENT, "string ID " + std::to_string(d.string_id) + " / OM ID " + std::to_string(d.om_id) + " does not fit the photon record");
        if (d.class_index < 0 || d.class_index >= P.num_classes) throw Error(CLSIMHIP_ERR_ARGUMENT, dom_name(d) + ": class_index out of range");
        if ((d.flags & ~(kPhotonHitHasStatus | kPhotonHitInCalibration)) != 0u) throw Error(CLSIMHIP_ERR_ARGUMENT, dom_name(d) + ": unknown flags");
        const uint32_t word = record_word(d.string_id, d.om_id);
        uint32_t slot = mcpe_dom_slot(word, P.dom_mask);
        while (dom_table_[slot] != 0u && static_cast<uint32_t>(dom_table_[slot]) != word) slot = (slot + 1u) & P.dom_mask;
        if (dom_table_[slot] != 0u) throw Error(CLSIMHIP_ERR_ARGUMENT, dom_name(d) + " is named twice");
        dom_table_[slot] = word | (static_cast<uint64_t>(d.class_index + 1) << 32) | (static_cast<uint64_t>(d.flags) << 40);
        double *v = dom_values_.data() + 4u * slot;
        v[0] = resolve_efficiency(d, K);
        v[1] = d.dir_x; v[2] = d.dir_y; v[3] = d.dir_z;
    }
    if (values_.empty()) values_.push_back(0.);         // (never read: only constant classes)
    P.values = values_.data();
    P.dom_table = dom_table_.data();
}

PhotonHitMaker::~PhotonHitMaker()
{
    for (auto &kv : images_) {
        DeviceGuard on_device(kv.first, std::nothrow);
        DeviceBuffer<McpeParams> params(kv.second.params);
        DeviceBuffer<double> values(kv.second.values), dom_values(kv.second.dom_values);
        DeviceBuffer<uint64_t> dom_table(kv.second.dom_table);
    }
}

double PhotonHitMaker::efficiency(int32_t string_id, uint32_t om_id) const
{
    int64_t slot = -1;
    if (string_id >= -32768 && string_id <= 32767 && om_id <= 65535u) slot = photon_hit_dom_slot(dom_table_.data(), params_.dom_mask, record_word(string_id, om_id));
    if (slot < 0) throw Error(CLSIMHIP_ERR_ARGUMENT, "OM (" + std::to_string(string_id) + "/" + std::to_string(om_id) + ") is not in the DOM table");
    return dom_values_[4u * static_cast<size_t>(slot)];
}

void PhotonHitMaker::host(const clsimhip_frame_photon *records, size_t n, const clsimhip_mcpe_series *series, size_t n_series, clsimhip_mcpe *out,
                          clsimhip_mcpe_series *out_series, size_t *n_kept, size_t *n_series_out, uint64_t counters[7]) const
{
    if (n && (!records || !out)) throw Error(CLSIMHIP_ERR_ARGUMENT, "records / out is (null)");
    if (n_series && (!series || !out_series)) throw Error(CLSIMHIP_ERR_ARGUMENT, "series / out_series is (null)");
    if (n > 0xffffffffull || n_series > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "more than 2^32 - 1 records or series");
    PhotonHitLookup L{};
    L.series = series;
    L.n_series = static_cast<uint32_t>(n_series);
    L.dom_table = dom_table_.data();
    L.dom_values = dom_values_.data();
    L.dom_mask = params_.dom_mask;
    L.switches = switches_;
    std::vector<SeriesKey> keys;
    keys.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        uint32_t w[12];
        std::memcpy(w, records + i, sizeof w);
        SeriesKey k;
        bool off_surface = false;
        const int code = photon_hit_make(L, params_, values_.data(), static_cast<uint32_t>(i), w, k, off_surface);
        if (code == PHOTON_HIT_KEPT) keys.push_back(k);
        else if (code != PHOTON_HIT_DROPPED && code != PHOTON_HIT_OFF_SURFACE && counters) ++counters[code];
        if (off_surface && counters) ++counters[PHOTON_HIT_OFF_SURFACE];
    }
    std::sort(keys.begin(), keys.end(), series_key_less);
    size_t made = 0;
    for (size_t i = 0; i < keys.size(); ++i) {
        const SeriesKey &k = keys[i];
        const clsimhip_mcpe_series &entry = series[k.group];
        clsimhip_mcpe &m = out[i];
        m.identifier = k.identifier;
        m.string_id = entry.string_id; m.om_id = entry.om_id;
        m.time = series_time_of((static_cast<uint64_t>(k.t_hi) << 32) | k.t_lo);
        if (i == 0 || keys[i - 1].group != k.group) {
            clsimhip_mcpe_series &s = out_series[made++];       // (made <= the entries in use <= n_series)
            s.frame = entry.frame;
            s.string_id = entry.string_id; s.om_id = entry.om_id;
            s.first = static_cast<uint32_t>(i);
            s.count = 0u;
        }
        ++out_series[made - 1].count;
    }
    if (n_kept) *n_kept = keys.size();
    if (n_series_out) *n_series_out = made;
}

PhotonHitMaker::Image PhotonHitMaker::image_on(int device)
{
    std::lock_guard<std::mutex> lk(device_mutex_);
    auto it = images_.find(device);
    if (it != images_.end()) return it->second;
    DeviceBuffer<McpeParams> params(1, "photon hits: parameters");
    DeviceBuffer<double> values(values_.size(), "photon hits: acceptance tables"), dom_values(dom_values_.size(), "photon hits: DOM efficiencies and directions");
    DeviceBuffer<uint64_t> dom_table(dom_table_.size(), "photon hits: DOM table");
    McpeParams P = params_;                             // (the pointers in it are not read on the device: the kernel has the lookup's)
    P.values = values.get();
    P.dom_table = dom_table.get();
    hip_check(hipMemcpy(params.get(), &P, sizeof P, hipMemcpyHostToDevice), "photon hits: parameters");
    hip_check(hipMemcpy(values.get(), values_.data(), values_.size() * sizeof(double), hipMemcpyHostToDevice), "photon hits: acceptance tables");
    hip_check(hipMemcpy(dom_values.get(), dom_values_.data(), dom_values_.size() * sizeof(double), hipMemcpyHostToDevice), "photon hits: DOM efficiencies and directions");
    hip_check(hipMemcpy(dom_table.get(), dom_table_.data(), dom_table_.size() * sizeof(uint64_t), hipMemcpyHostToDevice), "photon hits: DOM table");
    const Image im{params.release(), values.release(), dom_table.release(), dom_values.release()};
    images_[device] = im;
    return im;
}

void PhotonHitMaker::device(int device, const void *d_records, const void *d_series, const void *d_in_counts, size_t capacity, void *d_out, void *d_out_series,
                            void *d_counts, void *d_workspace, size_t workspace_bytes, hipStream_t stream)
{
    const SeriesWorkspaceLayout W(capacity, 0u);
    check_series_device_args("photon hits", "d_records", 16u, d_records, d_in_counts, capacity, d_out, d_out_series, d_counts, d_workspace, workspace_bytes, W.bytes);
    if (capacity && !d_series) throw Error(CLSIMHIP_ERR_ARGUMENT, "d_series is (null)");
    if (reinterpret_cast<uintptr_t>(d_series) & 15u) throw Error(CLSIMHIP_ERR_ARGUMENT, "d_series must be aligned to 16 bytes");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) throw Error(CLSIMHIP_ERR_DEVICE, "no HIP device available (the photon hits' device path has no CPU fallback)");
    if (device < 0 || device >= count) throw Error(CLSIMHIP_ERR_ARGUMENT, "device ordinal out of range");
    DeviceGuard on_device(device);
    const Image im = image_on(device);                  // (the first call on a device copies the maker's tables there)
    uint8_t *ws = static_cast<uint8_t *>(d_workspace);
    PhotonHitsDeviceArgs A{};
    A.lookup.series = static_cast<const clsimhip_mcpe_series *>(d_series);
    A.lookup.dom_table = im.dom_table;
    A.lookup.dom_values = im.dom_values;
    A.lookup.dom_mask = params_.dom_mask;
    A.lookup.switches = switches_;
    A.params = im.params;
    A.values = im.values;
    A.num_values = params_.num_values;
    // a group is the index of a series in use, below `capacity`: the bytes of it that can differ between two keys
    A.group_passes = 0u;
    for (uint64_t top = capacity ? capacity - 1u : 0u; top != 0u; top >>= 8) ++A.group_passes;
    A.in = static_cast<const clsimhip_frame_photon *>(d_records);
    A.in_counts = static_cast<const uint32_t *>(d_in_counts);
    A.capacity = static_cast<uint32_t>(capacity);
    set_series_workspace(A, ws, W);
    A.out = static_cast<clsimhip_mcpe *>(d_out);
    A.series = static_cast<clsimhip_mcpe_series *>(d_out_series);
    A.counts = static_cast<uint32_t *>(d_counts);
    const hipError_t e = launch_photon_hits(A, stream);
    if (e != hipSuccess) throw Error(CLSIMHIP_ERR_DEVICE, std::string("photon hits kernel launch: ") + hipGetErrorString(e));
}

} // namespace clsimhip
