// The MCPE generator object: see mcpe.h.  Configuration and the host twin here, the kernel in mcpe_kernel.hip.
#include "mcpe.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "converter.h"

namespace clsimhip {

McpeGenerator::McpeGenerator(const std::vector<FunctionData> &classes, size_t n_doms, const int32_t *string_ids, const uint32_t *om_ids,
                             const int32_t *class_index, const clsimhip_polynomial &angular, double dom_radius, double oversize, double pancake,
                             uint64_t seed)
{
    if (classes.empty() || classes.size() > static_cast<size_t>(kMcpeMaxClasses))
        throw Error(CLSIMHIP_ERR_ARGUMENT, "an MCPE generator takes 1 ... " + std::to_string(kMcpeMaxClasses) + " wavelength acceptance classes");
    McpeParams &P = params_;
    P.num_classes = static_cast<int32_t>(classes.size());
    for (size_t k = 0; k < classes.size(); ++k) {
        const FunctionData &f = classes[k];
        // like the wavelength bias of a converter: FromTable has no device code for unequal spacing (FromTable.cxx:169-170)
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

    if (!(dom_radius > 0.) || !(oversize > 0.) || !(pancake > 0.) || !std::isfinite(dom_radius) || !std::isfinite(oversize) || !std::isfinite(pancake))
        throw Error(CLSIMHIP_ERR_ARGUMENT, "dom_radius, oversize and pancake must be positive and finite");
    // the radius photons are recorded at: the oversized sphere, flattened along the photon's direction by the pancake factor
    const double R = dom_radius * oversize / pancake;
    const double lo = (R - 0.03 > 0.) ? R - 0.03 : 0., hi = R + 0.03;                  // 3 cm (:612)
    P.lo2 = lo * lo; P.hi2 = hi * hi;
    P.time_factor = 1. - pancake / oversize;                                            // :516
    P.seed = seed;
    pancake_ = pancake;

    if (n_doms && (!string_ids || !om_ids || !class_index)) throw Error(CLSIMHIP_ERR_ARGUMENT, "string_ids / om_ids / class_index are (null)");
    // (only 2^32 pairs exist; the table's hash spreads over 25 bits)
    if (n_doms > (size_t{1} << 24)) throw Error(CLSIMHIP_ERR_ARGUMENT, "an MCPE generator takes at most 2^24 DOMs");
    size_t slots = 16;
    while (slots < 2 * n_doms) slots *= 2;
    dom_table_.assign(slots, 0u);
    P.dom_mask = static_cast<uint32_t>(slots - 1);
    for (size_t i = 0; i < n_doms; ++i) {
        if (string_ids[i] < -32768 || string_ids[i] > 32767 || om_ids[i] > 65535u)
            throw Error(CLSIMHIP_ERR_CONFIG, "string ID " + std::to_string(string_ids[i]) + " / OM ID " + std::to_string(om_ids[i]) + " does not fit the photon record");
        if (class_index[i] < 0 || class_index[i] >= P.num_classes) throw Error(CLSIMHIP_ERR_ARGUMENT, "class_index out of range");
        const uint32_t key = static_cast<uint32_t>(static_cast<uint16_t>(static_cast<int16_t>(string_ids[i]))) | (om_ids[i] << 16);
        const uint64_t entry = key | (static_cast<uint64_t>(class_index[i] + 1) << 32);
        uint32_t slot = mcpe_dom_slot(key, P.dom_mask);
        while (dom_table_[slot] != 0u && static_cast<uint32_t>(dom_table_[slot]) != key) slot = (slot + 1u) & P.dom_mask;
        if (dom_table_[slot] != 0u && dom_table_[slot] != entry)
            throw Error(CLSIMHIP_ERR_ARGUMENT, "DOM (" + std::to_string(string_ids[i]) + ", " + std::to_string(om_ids[i]) + ") is given two different classes");
        dom_table_[slot] = entry;
    }
    // MCPE series: every DOM's rank in ascending (string ID signed, OM ID) order -- OMKey::operator< with PMT 0 -- in an array of
    // its own beside the table (the table's entries, and what mcpe_class_of reads in them, stay what they are)
    for (uint64_t e : dom_table_)
        if (e != 0u) dom_of_rank_.push_back(static_cast<uint32_t>(e));
    std::sort(dom_of_rank_.begin(), dom_of_rank_.end(), [](uint32_t a, uint32_t b) {
        const int16_t sa = static_cast<int16_t>(a & 0xffffu), sb = static_cast<int16_t>(b & 0xffffu);
        return sa != sb ? sa < sb : (a >> 16) < (b >> 16);
    });
    dom_ranks_.assign(slots, 0u);
    for (size_t r = 0; r < dom_of_rank_.size(); ++r) {
        uint32_t slot = mcpe_dom_slot(dom_of_rank_[r], P.dom_mask);
        while (static_cast<uint32_t>(dom_table_[slot]) != dom_of_rank_[r] || dom_table_[slot] == 0u) slot = (slot + 1u) & P.dom_mask;
        dom_ranks_[slot] = static_cast<uint32_t>(r);
    }
    if (values_.empty()) values_.push_back(0.);         // (never read: only constant classes)
    P.values = values_.data();
    P.dom_table = dom_table_.data();
}

McpeGenerator::~McpeGenerator()
{
    // (mcpe.h is shared with the kernel and keeps plain pointers in its images: they are handed to owners here to be freed)
    for (auto &kv : images_) {
        DeviceGuard on_device(kv.first, std::nothrow);
        DeviceBuffer<double> values(kv.second.values);
        DeviceBuffer<uint64_t> dom_table(kv.second.dom_table);
        DeviceBuffer<uint32_t> dom_ranks(kv.second.dom_ranks), dom_of_rank(kv.second.dom_of_rank);
    }
}

bool McpeGenerator::has_class(int32_t string_id, uint32_t om_id) const
{
    if (string_id < -32768 || string_id > 32767 || om_id > 65535u) return false;
    const uint32_t key = static_cast<uint32_t>(static_cast<uint16_t>(static_cast<int16_t>(string_id))) | (om_id << 16);
    return mcpe_class_of(dom_table_.data(), params_.dom_mask, key) >= 0;
}

void McpeGenerator::convert_host(const clsimhip_photon *photons, size_t n, clsimhip_mcpe *out, size_t capacity, size_t *n_out, uint64_t counters[4]) const
{
    if (n && !photons) throw Error(CLSIMHIP_ERR_ARGUMENT, "photons is (null)");
    if (capacity && !out) throw Error(CLSIMHIP_ERR_ARGUMENT, "out is (null)");
    size_t made = 0;
    for (size_t i = 0; i < n; ++i) {
        uint32_t w[20];
        std::memcpy(w, photons + i, sizeof w);
        clsimhip_mcpe m;
        const int code = mcpe_make(params_, values_.data(), w, m);
        if (code == MCPE_ACCEPTED) {
            if (made < capacity) out[made] = m;
            ++made;                                     // (keeps counting past `capacity`, like the device counter)
        } else if (code != MCPE_DROPPED && counters)
            ++counters[code - 1];
    }
    if (n_out) *n_out = made;
}

McpeGenerator::DeviceImage McpeGenerator::image_on(int device)
{
    std::lock_guard<std::mutex> lk(device_mutex_);
    auto it = images_.find(device);
    if (it != images_.end()) return it->second;
    DeviceBuffer<double> values(values_.size(), "MCPE acceptance tables");
    DeviceBuffer<uint64_t> dom_table(dom_table_.size(), "MCPE DOM classes");
    hip_check(hipMemcpy(values.get(), values_.data(), values_.size() * sizeof(double), hipMemcpyHostToDevice), "MCPE acceptance tables");
    hip_check(hipMemcpy(dom_table.get(), dom_table_.data(), dom_table_.size() * sizeof(uint64_t), hipMemcpyHostToDevice), "MCPE DOM classes");
    DeviceBuffer<uint32_t> dom_ranks(dom_ranks_.size(), "MCPE DOM ranks"), dom_of_rank(dom_of_rank_.size(), "MCPE DOMs by rank");
    hip_check(hipMemcpy(dom_ranks.get(), dom_ranks_.data(), dom_ranks_.size() * sizeof(uint32_t), hipMemcpyHostToDevice), "MCPE DOM ranks");
    if (!dom_of_rank_.empty())
        hip_check(hipMemcpy(dom_of_rank.get(), dom_of_rank_.data(), dom_of_rank_.size() * sizeof(uint32_t), hipMemcpyHostToDevice), "MCPE DOMs by rank");
    const DeviceImage im{values.release(), dom_table.release(), dom_ranks.release(), dom_of_rank.release()};
    images_[device] = im;
    return im;
}

void McpeGenerator::convert_device(int device, const void *d_photons, const void *d_hit_count, size_t capacity, void *d_mcpes, size_t mcpe_capacity,
                                   void *d_counters, hipStream_t stream)
{
    if (!d_photons || !d_hit_count || !d_counters) throw Error(CLSIMHIP_ERR_ARGUMENT, "device pointers are (null)");
    if (mcpe_capacity && !d_mcpes) throw Error(CLSIMHIP_ERR_ARGUMENT, "d_mcpes is (null)");
    // the kernel reads a record as five 16-byte words and writes an MCPE as two 8-byte words
    if ((reinterpret_cast<uintptr_t>(d_photons) & 15u) || (reinterpret_cast<uintptr_t>(d_mcpes) & 7u) || (reinterpret_cast<uintptr_t>(d_counters) & 3u))
        throw Error(CLSIMHIP_ERR_ARGUMENT, "d_photons must be aligned to 16 bytes, d_mcpes to 8, d_counters to 4");
    if (capacity > 0xffffffffull || mcpe_capacity > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "capacity beyond 2^32 - 1 records");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) throw Error(CLSIMHIP_ERR_DEVICE, "no HIP device available (the hit maker's device path has no CPU fallback)");
    if (device < 0 || device >= count) throw Error(CLSIMHIP_ERR_ARGUMENT, "device ordinal out of range");
    DeviceGuard on_device(device);
    const DeviceImage im = image_on(device);
    McpeParams P = params_;
    P.values = im.values;
    P.dom_table = im.dom_table;
    P.photons = static_cast<const uint32_t *>(d_photons);
    P.hit_count = static_cast<const uint32_t *>(d_hit_count);
    P.out = static_cast<clsimhip_mcpe *>(d_mcpes);
    P.counters = static_cast<uint32_t *>(d_counters);
    P.capacity = static_cast<uint32_t>(capacity);
    P.out_capacity = static_cast<uint32_t>(mcpe_capacity);
    hipError_t e = hipMemsetAsync(d_counters, 0, 5 * sizeof(uint32_t), stream);
    if (e == hipSuccess) e = launch_mcpe_kernel(P, stream);
    if (e != hipSuccess) throw Error(CLSIMHIP_ERR_DEVICE, std::string("MCPE kernel launch: ") + hipGetErrorString(e));
}

} // namespace clsimhip
