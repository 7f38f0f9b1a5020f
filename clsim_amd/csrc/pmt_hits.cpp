// The multi-PMT hit generator object: see pmt_hits.h.  Configuration and the host twin here, the kernel in pmt_hits_kernel.hip.
#include "pmt_hits.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace clsimhip {

namespace {

// v rotated as pmt_make rotates it
void rotate(const double m[9], const double v[3], double out[3])
{
    out[0] = (m[0] * v[0] + m[1] * v[1]) + m[2] * v[2];
    out[1] = (m[3] * v[0] + m[4] * v[1]) + m[5] * v[2];
    out[2] = (m[6] * v[0] + m[7] * v[1]) + m[8] * v[2];
}
double length2(const double v[3]) { return v[0] * v[0] + v[1] * v[1] + v[2] * v[2]; }
bool within(double x, double tolerance) { return std::fabs(x) <= tolerance; }          // (false for a NaN)

std::string module_name(const clsimhip_pmt_module &m) { return "module (" + std::to_string(m.string_id) + ", " + std::to_string(m.om_id) + ")"; }

} // namespace

PmtHitGenerator::PmtHitGenerator(const std::vector<FunctionData> &functions, const clsimhip_pmt_type *types, size_t n_types, const clsimhip_pmt *pmts,
                                 size_t n_pmts, const clsimhip_pmt_module *modules, size_t n_modules, uint64_t seed)
{
    PmtHitParams &P = params_;
    if (functions.empty() || !types || !n_types || !pmts || !n_pmts) throw Error(CLSIMHIP_ERR_ARGUMENT, "a PMT hit generator needs functions, types and PMTs");
    if (functions.size() > static_cast<size_t>(kPmtMaxFunctions))
        throw Error(CLSIMHIP_ERR_CONFIG, "a PMT hit generator takes at most " + std::to_string(kPmtMaxFunctions) + " functions");
    if (n_types > static_cast<size_t>(kPmtMaxTypes))
        throw Error(CLSIMHIP_ERR_CONFIG, "a PMT hit generator takes at most " + std::to_string(kPmtMaxTypes) + " module types");
    P.num_functions = static_cast<int32_t>(functions.size());
    for (size_t k = 0; k < functions.size(); ++k) {
        const FunctionData &f = functions[k];
        if (!f.on_device()) throw Error(CLSIMHIP_ERR_CONFIG, "a PMT hit generator's functions must be tables with equal spacing or constants");
        McpeClass &c = P.functions[k];
        c.kind = f.kind;
        c.value = f.value;
        if (f.kind == CLSIMHIP_FUNCTION_TABLE) {
            if (!(f.step > 0.) || !std::isfinite(f.step) || !std::isfinite(f.start) || f.values.size() < 2)
                throw Error(CLSIMHIP_ERR_ARGUMENT, "a function table needs a finite first argument, a positive spacing and two values or more");
            c.n = static_cast<int32_t>(f.values.size());
            c.offset = static_cast<uint32_t>(values_.size());
            c.start = f.start; c.step = f.step;
            values_.insert(values_.end(), f.values.begin(), f.values.end());
        }
    }
    if (values_.size() > kPmtMaxTableValues)
        throw Error(CLSIMHIP_ERR_CONFIG, "the function tables hold more than " + std::to_string(kPmtMaxTableValues) + " values together");
    P.num_values = static_cast<uint32_t>(values_.size());
    const auto function_index = [&](int32_t i, const char *what) {
        if (i < 0 || i >= P.num_functions) throw Error(CLSIMHIP_ERR_ARGUMENT, std::string(what) + ": function index out of range");
        return i;
    };

    P.num_types = static_cast<int32_t>(n_types);
    std::vector<double> radius(n_types);
    for (size_t t = 0; t < n_types; ++t) {
        const clsimhip_pmt_type &in = types[t];
        const std::string name = "module type " + std::to_string(t);
        if (in.n_pmts > kPmtMaxPerType) throw Error(CLSIMHIP_ERR_CONFIG, name + ": more than " + std::to_string(kPmtMaxPerType) + " PMTs");
        if (in.n_pmts < 1 || in.first_pmt < 0 || static_cast<size_t>(in.first_pmt) + static_cast<size_t>(in.n_pmts) > n_pmts)
            throw Error(CLSIMHIP_ERR_ARGUMENT, name + ": its PMTs are not in the array");
        if (!(in.sphere_radius > 0.) || !std::isfinite(in.sphere_radius)) throw Error(CLSIMHIP_ERR_ARGUMENT, name + ": the sphere radius must be positive and finite");
        const double R = in.sphere_radius;
        radius[t] = R;
        PmtType &T = P.types[t];
        const double lo = (R - 0.03 > 0.) ? R - 0.03 : 0., hi = R + 0.03;                  // 3 cm (:140)
        T.lo2 = lo * lo; T.hi2 = hi * hi;
        T.first = static_cast<int32_t>(pmts_.size());
        T.count = in.n_pmts;
        T.g = function_index(in.glass_gel_survival, "glass_gel_survival");
        for (int i = 0; i < in.n_pmts; ++i) {
            const clsimhip_pmt &p = pmts[in.first_pmt + i];
            const std::string pmt = name + ", PMT " + std::to_string(i);
            if (!within(length2(p.axis) - 1., 1e-6)) throw Error(CLSIMHIP_ERR_CONFIG, pmt + ": the axis is not a unit vector");
            if (!(length2(p.position) <= R * R)) throw Error(CLSIMHIP_ERR_CONFIG, pmt + ": OM sphere radius too small for this PMT");       // :191
            if (!(p.radius > 0.) || !std::isfinite(p.radius) || !std::isfinite(p.collection_efficiency))
                throw Error(CLSIMHIP_ERR_ARGUMENT, pmt + ": the radius must be positive and finite, the collection efficiency finite");
            PmtEntry e;
            for (int k = 0; k < 3; ++k) { e.n[k] = p.axis[k]; e.a[k] = p.position[k]; }
            e.radius2 = p.radius * p.radius;                                               // :157-158
            e.ce = p.collection_efficiency;
            e.q = function_index(p.quantum_efficiency, "quantum_efficiency");
            e.acceptance = function_index(p.angular_acceptance, "angular_acceptance");
            pmts_.push_back(e);
        }
    }
    P.num_pmts = static_cast<uint32_t>(pmts_.size());
    P.seed = seed;

    if (n_modules && !modules) throw Error(CLSIMHIP_ERR_ARGUMENT, "modules is (null)");
    if (n_modules > (size_t{1} << 24)) throw Error(CLSIMHIP_ERR_CONFIG, "a PMT hit generator takes at most 2^24 modules");
    size_t slots = 16;
    while (slots < 2 * n_modules) slots *= 2;
    module_table_.assign(slots, 0u);
    P.module_mask = static_cast<uint32_t>(slots - 1);
    modules_.resize(n_modules);
    std::vector<bool> used(n_types, false);
    for (size_t i = 0; i < n_modules; ++i) {
        const clsimhip_pmt_module &in = modules[i];
        if (in.string_id < -32768 || in.string_id > 32767 || in.om_id > 65535u) throw Error(CLSIMHIP_ERR_CONFIG, module_name(in) + " does not fit the photon record");
        if (in.type < 0 || static_cast<size_t>(in.type) >= n_types) throw Error(CLSIMHIP_ERR_CONFIG, "No type information found for " + module_name(in));     // :286-287
        // the rotation keeps lengths: the unit vectors, and what the reference checks per photon (:172, :189, :191)
        for (int k = 0; k < 3; ++k) {
            const double unit[3] = {k == 0 ? 1. : 0., k == 1 ? 1. : 0., k == 2 ? 1. : 0.};
            double r[3];
            rotate(in.rotation, unit, r);
            if (!within(length2(r) - 1., 1e-6)) throw Error(CLSIMHIP_ERR_CONFIG, module_name(in) + ": rotation does change vector length");
        }
        const PmtType &T = P.types[in.type];
        for (int k = 0; k < T.count; ++k) {
            const PmtEntry &e = pmts_[T.first + k];
            double n[3], a[3];
            rotate(in.rotation, e.n, n);
            rotate(in.rotation, e.a, a);
            if (!within(length2(n) - 1., 1e-6) || !within(length2(e.a) - length2(a), 1e-6))
                throw Error(CLSIMHIP_ERR_CONFIG, module_name(in) + ": rotation does change vector length");
            if (!(length2(a) <= radius[in.type] * radius[in.type]))
                throw Error(CLSIMHIP_ERR_CONFIG, module_name(in) + ", PMT " + std::to_string(k) + ": OM sphere radius too small for this PMT");
        }
        const uint32_t key = static_cast<uint32_t>(static_cast<uint16_t>(static_cast<int16_t>(in.string_id))) | (in.om_id << 16);
        uint32_t slot = mcpe_dom_slot(key, P.module_mask);
        while (module_table_[slot] != 0u && static_cast<uint32_t>(module_table_[slot]) != key) slot = (slot + 1u) & P.module_mask;
        if (module_table_[slot] != 0u) throw Error(CLSIMHIP_ERR_CONFIG, module_name(in) + " is given twice");
        module_table_[slot] = key | (static_cast<uint64_t>(i + 1) << 32);
        std::memcpy(modules_[i].m, in.rotation, sizeof modules_[i].m);
        modules_[i].type = in.type;
        modules_[i].reserved = 0;
        used[in.type] = true;
    }
    for (size_t t = 0; t < n_types; ++t)
        if (used[t]) used_radii_.push_back(radius[t]);
    if (values_.empty()) values_.push_back(0.);         // (never read: only constants)
    if (modules_.empty()) modules_.resize(1);           // (never read: every lookup fails)
    P.values = values_.data();
    P.pmts = pmts_.data();
    P.module_table = module_table_.data();
    P.modules = modules_.data();
    build_series_tables();
}

PmtHitGenerator::~PmtHitGenerator()
{
    // (pmt_hits.h is shared with the kernel and keeps plain pointers in its images: they are handed to owners here to be freed)
    for (auto &kv : images_) {
        DeviceGuard on_device(kv.first, std::nothrow);
        DeviceBuffer<double> values(kv.second.values);
        DeviceBuffer<PmtEntry> pmts(kv.second.pmts);
        DeviceBuffer<uint64_t> module_table(kv.second.module_table);
        DeviceBuffer<PmtModule> modules(kv.second.modules);
    }
}

void PmtHitGenerator::build_series_tables()
{
    // PMT series (pmt_series.h): every module's rank in ascending (string ID signed, OM ID) order -- OMKey::operator< -- and its
    // channels, in arrays of their own beside the table (the table's entries, and what pmt_make reads in them, stay what they are)
    for (uint64_t e : module_table_)
        if (e != 0u) module_of_rank_.push_back(static_cast<uint32_t>(e));
    std::sort(module_of_rank_.begin(), module_of_rank_.end(), [](uint32_t a, uint32_t b) {
        const int16_t sa = static_cast<int16_t>(a & 0xffffu), sb = static_cast<int16_t>(b & 0xffffu);
        return sa != sb ? sa < sb : (a >> 16) < (b >> 16);
    });
    module_ranks_.assign(module_table_.size(), 0u);
    channel_bases_.assign(module_table_.size(), 0u);
    base_.assign(module_of_rank_.size() + 1u, 0u);
    for (size_t r = 0; r < module_of_rank_.size(); ++r) {                // (at most 2^24 modules of at most 64 PMTs: 32 bits hold the sum)
        uint32_t slot = mcpe_dom_slot(module_of_rank_[r], params_.module_mask);
        while (static_cast<uint32_t>(module_table_[slot]) != module_of_rank_[r] || module_table_[slot] == 0u) slot = (slot + 1u) & params_.module_mask;
        const size_t index = static_cast<size_t>(module_table_[slot] >> 32) - 1u;
        module_ranks_[slot] = static_cast<uint32_t>(r);
        channel_bases_[slot] = base_[r];
        base_[r + 1u] = base_[r] + static_cast<uint32_t>(params_.types[modules_[index].type].count);
    }
}

bool PmtHitGenerator::has_module(int32_t string_id, uint32_t om_id) const
{
    if (string_id < -32768 || string_id > 32767 || om_id > 65535u) return false;
    const uint32_t key = static_cast<uint32_t>(static_cast<uint16_t>(static_cast<int16_t>(string_id))) | (om_id << 16);
    return mcpe_class_of(module_table_.data(), params_.module_mask, key) >= 0;
}

void PmtHitGenerator::convert_host(const clsimhip_photon *photons, size_t n, clsimhip_pmt_hit *out, size_t capacity, size_t *n_out, uint64_t counters[3]) const
{
    if (n && !photons) throw Error(CLSIMHIP_ERR_ARGUMENT, "photons is (null)");
    if (capacity && !out) throw Error(CLSIMHIP_ERR_ARGUMENT, "out is (null)");
    size_t made = 0;
    for (size_t i = 0; i < n; ++i) {
        uint32_t w[20];
        std::memcpy(w, photons + i, sizeof w);
        clsimhip_pmt_hit hit;
        bool off_surface;
        const int code = pmt_make(params_, values_.data(), pmts_.data(), w, hit, off_surface);
        if (code == PMT_ACCEPTED) {
            if (made < capacity) out[made] = hit;
            ++made;                                     // (keeps counting past `capacity`, like the device counter)
        } else if (code != PMT_DROPPED && counters)
            ++counters[code - 1];
        if (off_surface && counters) ++counters[2];
    }
    if (n_out) *n_out = made;
}

PmtHitGenerator::DeviceImage PmtHitGenerator::image_on(int device)
{
    std::lock_guard<std::mutex> lk(device_mutex_);
    auto it = images_.find(device);
    if (it != images_.end()) return it->second;
    DeviceBuffer<double> values(values_.size(), "PMT function tables");
    DeviceBuffer<PmtEntry> pmts(pmts_.size(), "PMT tables");
    DeviceBuffer<uint64_t> module_table(module_table_.size(), "PMT module table");
    DeviceBuffer<PmtModule> modules(modules_.size(), "PMT modules");
    hip_check(hipMemcpy(values.get(), values_.data(), values_.size() * sizeof(double), hipMemcpyHostToDevice), "PMT function tables");
    hip_check(hipMemcpy(pmts.get(), pmts_.data(), pmts_.size() * sizeof(PmtEntry), hipMemcpyHostToDevice), "PMT tables");
    hip_check(hipMemcpy(module_table.get(), module_table_.data(), module_table_.size() * sizeof(uint64_t), hipMemcpyHostToDevice), "PMT module table");
    hip_check(hipMemcpy(modules.get(), modules_.data(), modules_.size() * sizeof(PmtModule), hipMemcpyHostToDevice), "PMT modules");
    const DeviceImage im{values.release(), pmts.release(), module_table.release(), modules.release()};
    images_[device] = im;
    return im;
}

void PmtHitGenerator::convert_device(int device, const void *d_photons, const void *d_hit_count, size_t capacity, void *d_hits, size_t hit_capacity,
                                     void *d_counters, hipStream_t stream)
{
    if (!d_photons || !d_hit_count || !d_counters) throw Error(CLSIMHIP_ERR_ARGUMENT, "device pointers are (null)");
    if (hit_capacity && !d_hits) throw Error(CLSIMHIP_ERR_ARGUMENT, "d_hits is (null)");
    // the kernel reads a record as five 16-byte words and writes a hit as three 8-byte words
    if ((reinterpret_cast<uintptr_t>(d_photons) & 15u) || (reinterpret_cast<uintptr_t>(d_hits) & 7u) || (reinterpret_cast<uintptr_t>(d_counters) & 3u))
        throw Error(CLSIMHIP_ERR_ARGUMENT, "d_photons must be aligned to 16 bytes, d_hits to 8, d_counters to 4");
    if (capacity > 0xffffffffull || hit_capacity > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "capacity beyond 2^32 - 1 records");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) throw Error(CLSIMHIP_ERR_DEVICE, "no HIP device available (the hit maker's device path has no CPU fallback)");
    if (device < 0 || device >= count) throw Error(CLSIMHIP_ERR_ARGUMENT, "device ordinal out of range");
    DeviceGuard on_device(device);
    const DeviceImage im = image_on(device);
    PmtHitParams P = params_;
    P.values = im.values;
    P.pmts = im.pmts;
    P.module_table = im.module_table;
    P.modules = im.modules;
    P.photons = static_cast<const uint32_t *>(d_photons);
    P.hit_count = static_cast<const uint32_t *>(d_hit_count);
    P.out = static_cast<clsimhip_pmt_hit *>(d_hits);
    P.counters = static_cast<uint32_t *>(d_counters);
    P.capacity = static_cast<uint32_t>(capacity);
    P.out_capacity = static_cast<uint32_t>(hit_capacity);
    hipError_t e = hipMemsetAsync(d_counters, 0, 4 * sizeof(uint32_t), stream);
    if (e == hipSuccess) e = launch_pmt_hits_kernel(P, stream);
    if (e != hipSuccess) throw Error(CLSIMHIP_ERR_DEVICE, std::string("PMT hit kernel launch: ") + hipGetErrorString(e));
}

} // namespace clsimhip
