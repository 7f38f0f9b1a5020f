// Host runtime: see converter.h.  One worker thread owns the HIP streams
// (upload -> kernel on the compute stream, photon download on the copy stream,
// OpenCL.cxx:1142-1315); callers talk to it through two bounded queues, like the
// reference's queueToOpenCL_/queueFromOpenCL_.  With double buffering one bunch
// is on the GPU while the previous one is downloaded and converted.
#include "converter.h"
#include "mcpe.h"
#include "mcpe_merge.h"
#include "pmt_hits.h"
#include "cable_shadow.h"
#include "event_stats.h"
#include "frame_photons.h"
#include "pmt_series.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>

namespace clsimhip {
[[maybe_unused]] constexpr size_t kCensusBytes = 4u << 20;      // analysis build: counters + per-wave records + per-wave region counters


static_assert(sizeof(clsimhip_step) == sizeof(DevStep), "step layouts");
static_assert(sizeof(clsimhip_photon) == sizeof(DevPhoton), "photon layouts");
constexpr uint32_t kQueueSlots = 256;
// The pooled kernel keeps 64 + R units per wave in flight (about 0.6M on the chip): it wins on bunches that hold more
// steps than that by a margin (1M steps: +9 %, 4M: +8 %) and loses on smaller ones (0.5M: -17 %), where the classic
// kernel's smaller grids apply.  Chosen per launch; results do not depend on the choice.
// (round 4, with bunches just below the chip's unit slots sliced like larger ones -- prop_pool_kernel.hip.h -- and a ring of 45: cascade steps, classic /
// pooled 1e9 photons/s: 0.39M 2.57 / 2.56, 0.49M 2.89 / 2.90, 0.56M 2.98 / 3.18, 0.59M 3.00 / 3.30, 0.62M 3.02 / 3.42, 0.66M 3.03 / 3.50; flasher steps 0.31M 1.62 / 1.55,
// 0.63M 2.00 / 2.23.  Round 2's threshold was 614 400.)
constexpr size_t kPooledKernelMinSteps = 524288;

hipError_t Converter::launch(const KParams &P, const LaunchTuning &tuning, hipStream_t stream) const
{
    KVariant v = tables_.variant;
    const bool pooled = tuning.pooled_for(P.n_steps, concurrent_launches_);
    v.grid = tuning.grid;
    v.generic_only = tuning.generic_only;
    KLaunched launched;
    v.launched = &launched;
    // the kernel compiled for this configuration: on the bunches the launcher itself sends to the pooled kernel -- their launches last
    // long enough for the one-off compilation to vanish in a run; the small bunches of tests take it only where asked to ("baked_kernel" 2)
    BakedReport baked;
    if (pooled && tuning.baked_kernel == 2) baked.wanted = 2;
    else if (pooled && tuning.baked_kernel == 1 && P.n_steps * static_cast<size_t>(concurrent_launches_) >= kPooledKernelMinSteps) baked.wanted = 1;
    v.baked = &baked;
    const hipError_t err = v.keep_detected ? (pooled ? launch_pool_keep_kernel(P, v, stream) : launch_keep_kernel(P, v, stream))
                                           : (pooled ? launch_pool_kernel(P, v, stream) : launch_prop_kernel(P, v, stream));
    if (launched.family >= 0) {              // (an empty bunch launches nothing: the report of the last real launch stays)
        std::lock_guard<std::mutex> lk(launched_mutex_);
        launched_ = launched;
        if (baked.state != kBakedUnused) baked_ = baked;
    }
    return err;
}

// ---- tuning (include/clsimhip.h: clsimhip_set_tuning) -----------------------------------------------------------------
void Converter::apply_kernel_choice()
{
    LaunchTuning &t = tuning_;
    t.derived = true;
    t.use_pool = pool_possible_ && t.kernel != 2;
    t.pool_min_steps = (t.kernel != 0) ? 0 : kPooledKernelMinSteps;
    if (t.tuned_pool_min_steps >= 0) t.pool_min_steps = static_cast<size_t>(t.tuned_pool_min_steps);
    t.pool_max_steps = pool_kernel_max_steps();
    if (t.tuned_pool_max_steps >= 0) t.pool_max_steps = std::min(t.pool_max_steps, static_cast<size_t>(t.tuned_pool_max_steps));
}

namespace {
struct TuningKey {
    const char *name;
    long long lo, hi;
    bool shapes_tables;             // one of the three keys of Compile()
    long long (*get)(const LaunchTuning &, const TableTuning &);
    void (*set)(LaunchTuning &, TableTuning &, long long);
};
#define LAUNCH_FIELD(f) false, [](const LaunchTuning &l, const TableTuning &) { return static_cast<long long>(l.f); }, \
                        [](LaunchTuning &l, TableTuning &, long long v) { l.f = static_cast<decltype(l.f)>(v); }
#define TABLE_FIELD(f) true, [](const LaunchTuning &, const TableTuning &t) { return static_cast<long long>(t.f); }, \
                       [](LaunchTuning &, TableTuning &t, long long v) { t.f = static_cast<decltype(t.f)>(v); }
// (the table of include/clsimhip.h, in its order)
const TuningKey kTuningKeys[] = {
    {"kernel", 0, 2, LAUNCH_FIELD(kernel)},
    // (once initialized the two report what the launches use)
    {"pool_min_steps", -1, 1ll << 40, false,
     [](const LaunchTuning &l, const TableTuning &) { return l.derived ? static_cast<long long>(l.pool_min_steps) : l.tuned_pool_min_steps; },
     [](LaunchTuning &l, TableTuning &, long long v) { l.tuned_pool_min_steps = v; }},
    {"pool_max_steps", -1, 1ll << 40, false,
     [](const LaunchTuning &l, const TableTuning &) { return l.derived ? static_cast<long long>(l.pool_max_steps) : l.tuned_pool_max_steps; },
     [](LaunchTuning &l, TableTuning &, long long v) { l.tuned_pool_max_steps = v; }},
    {"pool_ring", 0, 4096, LAUNCH_FIELD(pool_ring)},
    {"k_new", 0, 4096, LAUNCH_FIELD(k_new)},
    {"k_search", 0, 64, LAUNCH_FIELD(k_search)},
    {"slices", 0, 65535, LAUNCH_FIELD(slices)},
    {"k_pop", 0, 64, LAUNCH_FIELD(k_pop)},
    {"k_wait", -1, 255, LAUNCH_FIELD(k_wait)},
    {"k_aim", -1, 64, LAUNCH_FIELD(k_aim)},
    {"grid", 0, 1 << 20, LAUNCH_FIELD(grid)},
    {"generic_kernels", 0, 1, LAUNCH_FIELD(generic_only)},
    {"baked_kernel", 0, 2, LAUNCH_FIELD(baked_kernel)},
    {"result_min_records", 1, 1ll << 32, LAUNCH_FIELD(result_min_records)},
    {"string_map_cells", 8, 4096, TABLE_FIELD(string_map_cells)},
    {"dom_map_cells", 4, 512, TABLE_FIELD(dom_map_cells)},
    {"named_search", 0, 1, TABLE_FIELD(named_search)},
};
#undef LAUNCH_FIELD
#undef TABLE_FIELD

const TuningKey &tuning_key(const std::string &key)
{
    for (const TuningKey &t : kTuningKeys) if (key == t.name) return t;
    throw Error(CLSIMHIP_ERR_ARGUMENT, "no tuning key named " + key);
}
} // namespace

void Converter::set_tuning(const std::string &key, long long value)
{
    const TuningKey &k = tuning_key(key);
    if (value < k.lo || value > k.hi)
        throw Error(CLSIMHIP_ERR_ARGUMENT, "tuning " + key + ": " + std::to_string(value) + " is outside " + std::to_string(k.lo) + " ... " + std::to_string(k.hi));
    if (k.shapes_tables && compiled_) throw Error(CLSIMHIP_ERR_STATE, "tuning " + key + " shapes a table of Compile(): set it before Compile()");
    std::lock_guard<std::mutex> lk(tuning_mutex_);          // (a launch copies its tuning under the same lock)
    k.set(tuning_, table_tuning_, value);
    if (initialized_) apply_kernel_choice();
}

long long Converter::get_tuning(const std::string &key) const
{
    if (key == "baked_state") return baked_report().state;       // (read only: kBakedUnused, kBakedActive, kBakedFallback)
    const TuningKey &k = tuning_key(key);
    std::lock_guard<std::mutex> lk(tuning_mutex_);
    return k.get(tuning_, table_tuning_);
}

BakedResult Converter::baked_compile_probe(const char *arch, const char *flags) const
{
    BakedResult r;
    if (!compiled_) { r.why = "Compile() first"; return r; }
    const KVariant &v = tables_.variant;
    LaunchTuning t;
    {
        std::lock_guard<std::mutex> lk(tuning_mutex_);
        t = tuning_;
    }
    return baked_compile(tables_.params, BakedVariant{v.lengths, v.tilt, v.aniso, v.flasher, v.fast && !t.generic_only, v.keep_detected}, arch, flags);
}

void Converter::set_concurrent_device_launches(int k)
{
    if (k < 1 || k > 16) throw Error(CLSIMHIP_ERR_ARGUMENT, "concurrent device launches: 1 ... 16");
    concurrent_launches_ = k;
}

Converter::Converter(int device) : device_(device)
{
    // configuration and Compile() are host-only; the GPU is required from Initialize() on
    if (device < 0) throw Error(CLSIMHIP_ERR_ARGUMENT, "device ordinal out of range");
}

Converter::~Converter()
{
    if (in_queue_) in_queue_->close();
    if (out_queue_) out_queue_->close();
    if (worker_.joinable()) worker_.join();
    in_queue_.reset();              // jobs nobody took give their page-locked step buffers back to the pool, which release_device() frees
    release_device();
}

void Converter::release_device()
{
    if (!dev_.stream) return;       // nothing was created
    DeviceGuard on_device(device_, std::nothrow);
    // results nobody released, and results nobody fetched: their page-locked buffers go back to the pools first
    handed_out_.clear();
    if (out_queue_) {
        Result r;
        while (out_queue_->get_for(r, 0)) {}
    }
    dev_ = DeviceState();           // (the slots' step buffers go back to their pool)
    step_pool_.reset();
    result_pool_.reset();
    mcpe_pool_.reset();
    series_pool_.reset();
    merge_pool_.reset();
    pmt_pool_.reset();
    pmt_series_pool_.reset();
    fp_pool_.reset();
    fp_series_pool_.reset();
    bunch_pool_.reset();
}

void Converter::set_device(int device)
{
    guard();
    if (device < 0) throw Error(CLSIMHIP_ERR_ARGUMENT, "device ordinal out of range");
    device_ = device;
}

void Converter::check_worker() const
{
    std::lock_guard<std::mutex> lk(fatal_mutex_);
    if (worker_failed_) throw Error(CLSIMHIP_ERR_DEVICE, "the converter's worker thread stopped after a device error: " + fatal_error_);
}

void Converter::set_wlen_generators(std::vector<RandomValueData> g)
{
    guard();
    // a wavelength that is zero, negative or not finite gives a photon lengths of 0/0 = NaN, and a NaN absorption
    // budget never runs out (propagation_kernel.c.cl:536): refused here rather than spun on by the GPU
    for (const RandomValueData &r : g) {
        if (r.kind == CLSIMHIP_RANDOM_CONSTANT) {
            if (!std::isfinite(r.value) || !(r.value > 0.)) throw Error(CLSIMHIP_ERR_ARGUMENT, "a constant wavelength must be finite and positive");
        } else if (r.kind == CLSIMHIP_RANDOM_CHERENKOV_NO_DISPERSION) {
            // WlenCherenkovNoDispersion.cxx:47-51
            if (std::isnan(r.first)) throw Error(CLSIMHIP_ERR_ARGUMENT, "The \"fromWlen\" argument must not be NaN!");
            if (std::isnan(r.spacing)) throw Error(CLSIMHIP_ERR_ARGUMENT, "The \"toWlen\" argument must not be NaN!");
            if (r.first > r.spacing) throw Error(CLSIMHIP_ERR_ARGUMENT, "The \"fromWlen\" argument must not be greater than \"toWlen\".");
            if (!(r.first > 0.) || !std::isfinite(r.spacing)) throw Error(CLSIMHIP_ERR_ARGUMENT, "the wavelength range must be positive and finite");
        } else {
            if (r.kind == CLSIMHIP_RANDOM_INTERPOLATED_X) {
                if (r.x.size() != r.y.size()) throw Error(CLSIMHIP_ERR_ARGUMENT, "The \"x\" and \"y\" vectors must have the same size!");
                for (size_t i = 0; i < r.x.size(); ++i)
                    if (!std::isfinite(r.x[i]) || !(r.x[i] > 0.) || (i > 0 && !(r.x[i] > r.x[i - 1])))
                        throw Error(CLSIMHIP_ERR_ARGUMENT, "the wavelengths of a distribution must be positive, finite and ascending");
            } else if (!std::isfinite(r.first) || !(r.first > 0.) || !std::isfinite(r.spacing) || !(r.spacing > 0.))
                throw Error(CLSIMHIP_ERR_ARGUMENT, "a wavelength distribution needs a positive first wavelength and spacing");
            double sum = 0.;
            for (double y : r.y) {
                if (!std::isfinite(y) || y < 0.) throw Error(CLSIMHIP_ERR_ARGUMENT, "wavelength distribution values must be finite and non-negative");
                sum += y;
            }
            if (!(sum > 0.)) throw Error(CLSIMHIP_ERR_ARGUMENT, "a wavelength distribution must not be zero everywhere");
        }
    }
    compiled_ = false;
    generators_ = std::move(g);
}
void Converter::set_wlen_bias(FunctionData b)
{
    guard();
    if (!b.on_device()) throw Error(CLSIMHIP_ERR_ARGUMENT, "the wavelength bias must be a table with equal spacing or a constant (FromTable.cxx:169-170)");
    compiled_ = false; bias_ = std::move(b); have_bias_ = true;
}
void Converter::set_medium(MediumData m) { guard(); m.validate(); compiled_ = false; medium_ = std::move(m); have_medium_ = true; }
void Converter::set_geometry(GeometryInput g) { guard(); compiled_ = false; geometry_ = std::move(g); have_geometry_ = true; }

void Converter::set_mcpe_generator(std::shared_ptr<McpeGenerator> g, bool keep_photons)
{
    guard();
    compiled_ = false;
    mcpe_ = std::move(g);
    keep_photons_ = keep_photons;
}

void Converter::set_pmt_generator(std::shared_ptr<PmtHitGenerator> g, bool keep_photons)
{
    guard();
    compiled_ = false;
    pmt_ = std::move(g);
    pmt_keep_photons_ = keep_photons;
}

void Converter::set_workgroup_size(size_t v)
{
    guard();
    if (v == 0) throw Error(CLSIMHIP_ERR_ARGUMENT, "workgroup size must not be 0");
    if (v > max_workgroup_size()) throw Error(CLSIMHIP_ERR_ARGUMENT, "Workgroup size too large!");
    workgroup_size_ = v;
}
void Converter::set_max_num_workitems(size_t v)
{
    guard();
    if (v == 0) throw Error(CLSIMHIP_ERR_ARGUMENT, "maximum number of work items must not be 0");
    max_workitems_ = v;
}

// OpenCL.cxx:485-533
void Converter::compile()
{
    guard();
    if (compiled_) return;
    if (generators_.empty()) throw Error(CLSIMHIP_ERR_CONFIG, "WlenGenerators not set!");
    if (!have_bias_) throw Error(CLSIMHIP_ERR_CONFIG, "WlenBias not set!");
    if (!have_medium_) throw Error(CLSIMHIP_ERR_CONFIG, "MediumProperties not set!");
    if (!have_geometry_) throw Error(CLSIMHIP_ERR_CONFIG, "Geometry not set!");
    if (double_precision_) throw Error(CLSIMHIP_ERR_CONFIG, "DoublePrecision is not available in the HIP propagator");
    // SAVE_ALL_PHOTONS is unusable in the reference at this revision: it leaves out the geometry source (OpenCL.cxx:461-466)
    // that saveHit() needs for geometryGetDomPosition (propagation_kernel.c.cl:339).
    // StopDetectedPhotons=false (no STOP_PHOTONS_ON_DETECTION) runs the classic kernel's instantiations of their own
    // (prop_keep_kernel.hip).  The reference's collision code indexes dom_bitmask[stringNum/64] in an array of
    // (GEO_MAX_DOM_INDEX+63)/64 words there -- out of bounds from the 65th string on when no string has more than 64 DOMs
    // (sparse_collision_kernel.c.cl:85-104), undefined; here (and in the oracle) that word exists, which is also what the
    // kernel text compiled for x86-64 does (tools/verbatim_cl_check.py clear_keep).
    if (save_all_) throw Error(CLSIMHIP_ERR_CONFIG, "SaveAllPhotons is not available in the HIP propagator");
    if (history_entries_ > 1024) throw Error(CLSIMHIP_ERR_CONFIG, "PhotonHistoryEntries > 1024 is not supported");
#ifdef CLSIMHIP_DEVELOPER
    // (developer build only: the round 1-5 environment names of the three table keys; written directly, because set_tuning() is the
    // callers' door and refuses these keys once a Compile() has happened)
    {
        std::lock_guard<std::mutex> lk(tuning_mutex_);
        if (const char *e = std::getenv("CLSIMHIP_PROX_N")) table_tuning_.string_map_cells = std::max(8, std::min(4096, std::atoi(e)));
        if (const char *e = std::getenv("CLSIMHIP_DOM_PROX_N")) table_tuning_.dom_map_cells = std::max(4, std::min(512, std::atoi(e)));
        if (const char *e = std::getenv("CLSIMHIP_NO_NAMED_SEARCH")) table_tuning_.named_search = (e[0] != '1');
    }
#endif
    if (series_ && !mcpe_) throw Error(CLSIMHIP_ERR_CONFIG, "MCPE series need an MCPE generator (clsimhip_set_mcpe_generator)");
    if (merging_ && !series_) throw Error(CLSIMHIP_ERR_CONFIG, "MCPE merging needs the MCPE series stage (clsimhip_set_mcpe_series)");
    if (pmt_series_ && !pmt_) throw Error(CLSIMHIP_ERR_CONFIG, "PMT series need a PMT hit generator (clsimhip_set_pmt_generator)");
    // The stages read IDs from the records: DOM by DOM, the pair must fit them (the host conversion reports such IDs only when a
    // photon carries them, OpenCL.cxx:1577-1586) and pass the stage's own check
    const auto require_ids_fit_record = [&](const char *stage, auto also) {
        for (size_t i = 0; i < geometry_.string_ids.size(); ++i) {
            const int32_t sid = geometry_.string_ids[i];
            const uint32_t did = geometry_.dom_ids[i];
            if (sid < -32768 || sid > 32767 || did > 65535u)
                throw Error(CLSIMHIP_ERR_CONFIG, std::string(stage) + ": string ID " + std::to_string(sid) + " / OM ID " + std::to_string(did) + " does not fit the photon record");
            also(sid, did);
        }
    };
    if (mcpe_) {
        // every DOM must have a class (log_fatal per photon in the reference, :628-630)
        require_ids_fit_record("MCPE generator", [&](int32_t sid, uint32_t did) {
            if (!mcpe_->has_class(sid, did))
                throw Error(CLSIMHIP_ERR_CONFIG, "No wavelength acceptance configured for OMKey(" + std::to_string(sid) + "," + std::to_string(did) + ")");
        });
        if (history_entries_ && !keep_photons_) throw Error(CLSIMHIP_ERR_CONFIG, "photon histories need keep_photons");
        // records of a converter with another pancake factor sit at another radius: every one of them would be OFF_SURFACE
        if (mcpe_->pancake() != pancake_)
            throw Error(CLSIMHIP_ERR_CONFIG, "MCPE generator: made for DOM pancake factor " + std::to_string(mcpe_->pancake()) + ", the converter's is " + std::to_string(pancake_));
    }
    if (pmt_) {
        if (mcpe_) throw Error(CLSIMHIP_ERR_CONFIG, "a converter takes an MCPE generator or a PMT hit generator, not both");
        if (series_) throw Error(CLSIMHIP_ERR_CONFIG, "MCPE series are not made from PMT hits (clsimhip_set_mcpe_series with a PMT hit generator)");
        // every DOM must have a module (log_fatal per module in the reference, I3PhotonToMCHitConverterForMultiPMT.cxx:281-287)
        require_ids_fit_record("PMT hit generator", [&](int32_t sid, uint32_t did) {
            if (!pmt_->has_module(sid, did))
                throw Error(CLSIMHIP_ERR_CONFIG, "No module configured for OMKey(" + std::to_string(sid) + "," + std::to_string(did) + ")");
        });
        // records sit at the geometry's (oversized) OM radius, flattened by the pancake factor: a type made for another radius would
        // find every record OFF_SURFACE and its discs in the wrong places
        const double recorded_at = geometry_.om_radius / pancake_;
        for (double radius : pmt_->used_sphere_radii())
            if (!(std::fabs(radius - recorded_at) <= 0.03))
                throw Error(CLSIMHIP_ERR_CONFIG, "PMT hit generator: a module type's sphere radius is " + std::to_string(radius) + " m, photons are recorded at " +
                                                     std::to_string(recorded_at) + " m");
        if (history_entries_ && !pmt_keep_photons_) throw Error(CLSIMHIP_ERR_CONFIG, "photon histories need keep_photons");
    }
    fp_doms_.reset();
    if (frame_photons_) {
        // (the stage files the records under the geometry's DOMs)
        require_ids_fit_record("frame photons", [](int32_t, uint32_t) {});
        if (history_entries_ && !fp_keep_photons_) throw Error(CLSIMHIP_ERR_CONFIG, "photon histories need keep_photons");
        fp_doms_ = std::make_shared<FramePhotonDoms>(geometry_.string_ids.data(), geometry_.dom_ids.data(), geometry_.string_ids.size());
    }
    tables_ = compile_tables(medium_, geometry_, generators_, bias_, pancake_, table_tuning_);
    if (!std::isnan(fixed_abs_lengths_)) {                      // OpenCL.cxx:425-431
        tables_.params.has_fixed_abs = 1;
        tables_.params.fixed_abs = to_float_literal(fixed_abs_lengths_);
    }
    tables_.params.history_n = static_cast<int32_t>(history_entries_);   // OpenCL.cxx:416-419
    tables_.variant.keep_detected = !stop_detected_;                     // OpenCL.cxx:395-397
    compiled_ = true;
}

bool load_multipliers_from_file(const char *path, uint32_t *a, size_t count)
{
    // mwcrng_init.h:62-103: binary format = 17-byte tag "safeprimes_base32" + int64 LE each; else text, first column
    std::ifstream f(path, std::ios::binary);
    if (!f.good()) return false;
    char tag[18] = {0};
    f.read(tag, 17);
    if (std::strcmp(tag, "safeprimes_base32") == 0) {
        for (size_t i = 0; i < count; ++i) {
            int64_t m = 0;
            f.read(reinterpret_cast<char *>(&m), sizeof m);
            if (f.fail() || m < 0 || m > 0xffffffffll) return false;
            a[i] = static_cast<uint32_t>(m);
        }
        return true;
    }
    f.close();
    std::ifstream t(path);
    std::string line;
    for (size_t i = 0; i < count; ++i) {
        if (!std::getline(t, line)) return false;
        char *end = nullptr;
        const long long m = std::strtoll(line.c_str(), &end, 10);
        if (end == line.c_str() || m < 0 || m > 0xffffffffll) return false;
        a[i] = static_cast<uint32_t>(m);
    }
    return true;
}

void Converter::initialize(uint64_t seed)
{
    guard();
    compile();
    if (max_workitems_ == 0) max_workitems_ = 1048576;
    std::vector<uint32_t> a(max_workitems_);
    std::vector<uint64_t> x(max_workitems_);
    const char *file = std::getenv("CLSIMHIP_SAFEPRIMES_FILE");
    if (!(file && load_multipliers_from_file(file, a.data(), a.size()))) mwc_multipliers(a.data(), a.size());
    seed_streams(a.data(), a.size(), seed, x.data());
    initialize_with_streams(x.data(), a.data(), a.size());
}

// OpenCL.cxx:217-388
void Converter::initialize_with_streams(const uint64_t *x, const uint32_t *a, size_t count)
{
    guard();
    if (!x || !a || count == 0) throw Error(CLSIMHIP_ERR_ARGUMENT, "RNG streams are (null) or empty");
    compile();
    if (workgroup_size_ == 0) workgroup_size_ = max_workgroup_size();
    if (max_workitems_ == 0) max_workitems_ = count;
    if (count != max_workitems_) throw Error(CLSIMHIP_ERR_ARGUMENT, "number of RNG streams must equal the maximum number of work items");
    if (max_workitems_ % workgroup_size_ != 0)
        throw Error(CLSIMHIP_ERR_ARGUMENT, "The maximum number of work items (" + std::to_string(max_workitems_) +
                                               ") must be a multiple of the workgroup size (" + std::to_string(workgroup_size_) + ").");
    if (max_workitems_ > 0x7fffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "too many work items");
    for (size_t i = 0; i < count; ++i) {
        // mwcrng_init.h:107: a state outside this range breaks the generator
        if ((x[i] == 0) | ((static_cast<uint32_t>(x[i] >> 32)) >= (a[i] - 1)) | ((static_cast<uint32_t>(x[i])) >= 0xfffffffful))
            throw Error(CLSIMHIP_ERR_ARGUMENT, "invalid MWC state word for stream " + std::to_string(i));
    }
    // OpenCL.cxx:266-277
    max_output_photons_ = static_cast<uint32_t>(std::min<size_t>(max_workitems_ * 10, 0xffffffffull));
    if (max_output_photons_ < 1000) max_output_photons_ = 1000;

    {
        int count = 0;
        const hipError_t e = hipGetDeviceCount(&count);
        if (e != hipSuccess || count <= 0)
            throw Error(CLSIMHIP_ERR_DEVICE, "no HIP device available (the propagator has no CPU fallback)");
        if (device_ >= count) throw Error(CLSIMHIP_ERR_ARGUMENT, "device ordinal out of range");
    }
    // everything below runs with this converter's device current; the caller's current device is restored on return.  A failure
    // half-way frees what `created` holds and leaves dev_ empty: a retry starts from nothing.
    DeviceGuard on_device(device_);
    DeviceState created;
    created.stream.create("hipStreamCreate");
    created.copy_stream.create("hipStreamCreate");
    created.upload_stream.create("hipStreamCreate");
    setup_device_buffers(created);
    hip_check(hipMemcpy(created.rng_x.get(), x, count * sizeof(uint64_t), hipMemcpyHostToDevice), "upload rng x");
    hip_check(hipMemcpy(created.rng_a.get(), a, count * sizeof(uint32_t), hipMemcpyHostToDevice), "upload rng a");
    dev_ = std::move(created);

    in_queue_.reset(new BoundedQueue<Job>(5));          // queueToOpenCL_(5), OpenCL.cxx:77
    out_queue_.reset(new BoundedQueue<Result>(0));      // queueFromOpenCL_(0): rendezvous, OpenCL.cxx:78
    initialized_ = true;
    worker_ = std::thread([this] { worker(); });
}

void Converter::setup_device_buffers(DeviceState &D)
{
    const GeoTables &G = tables_.geo;
    auto upload = [&](auto &dst, const auto &src, const char *what) {
        dst.alloc(src.size(), what);
        if (!src.empty()) hip_check(hipMemcpy(dst.get(), src.data(), src.size() * sizeof(src[0]), hipMemcpyHostToDevice), what);
    };
    upload(D.tables, tables_.lds_image, "tables");
    upload(D.len_table, tables_.len_table, "length tables");
    upload(D.prox_map, tables_.prox_map, "string proximity map");
    {   // the DOM proximity map as the kernels read it: every cell with the centre of the DOM it names (kparams.h: dom_cells).  Built and
        // uploaded in pieces of a million cells: the whole image is up to 256 MB, which the host need not hold beside the words
        const size_t cells = tables_.dom_prox.size();
        D.dom_prox.alloc(cells * 4, "DOM proximity map");
        constexpr size_t kPiece = size_t{1} << 20;
        std::vector<uint32_t> fused(4 * std::min(cells, kPiece));
        for (size_t first = 0; first < cells; first += kPiece) {
            const size_t count = std::min(kPiece, cells - first);
            std::fill(fused.begin(), fused.begin() + static_cast<std::ptrdiff_t>(4 * count), 0u);
            for (size_t k = 0; k < count; ++k) {
                const uint32_t w = tables_.dom_prox[first + k], id = w & 0xffffu;
                fused[4 * k] = w;
                if (id != 0xffffu && 4 * static_cast<size_t>(id) + 2 < tables_.dom_centres.size())
                    std::memcpy(&fused[4 * k + 1], &tables_.dom_centres[4 * static_cast<size_t>(id)], 12);
            }
            hip_check(hipMemcpy(D.dom_prox.get() + 4 * first, fused.data(), count * 16, hipMemcpyHostToDevice), "DOM proximity map");
        }
    }
    upload(D.dom_centres, tables_.dom_centres, "DOM centres");
    upload(D.dom_named, tables_.dom_named, "named-DOM records");
    upload(D.dom_tx, G.dom_tx, "dom_tx");
    upload(D.dom_ty, G.dom_ty, "dom_ty");
    upload(D.dom_tz, G.dom_tz, "dom_tz");
    {   // index -> ID tables for assemble_hits_kernel; an ID that does not fit the record's short / ushort keeps the
        // conversion on the host, which reports it when a photon carries it (OpenCL.cxx:1577-1586)
        std::vector<int16_t> sid(G.string_index_to_id.size());
        std::vector<uint32_t> start(G.string_index_to_id.size() + 1);         // (+ the end of the last string's run)
        std::vector<uint16_t> did;
        bool fits = true;
        for (size_t k = 0; k < G.string_index_to_id.size(); ++k) {
            fits = fits && G.string_index_to_id[k] >= -32768 && G.string_index_to_id[k] <= 32767;
            sid[k] = static_cast<int16_t>(G.string_index_to_id[k]);
            start[k] = static_cast<uint32_t>(did.size());
            for (uint32_t v : G.dom_index_to_id[k]) { fits = fits && v <= 65535u; did.push_back(static_cast<uint16_t>(v)); }
        }
        start.back() = static_cast<uint32_t>(did.size());
        if (fits && !sid.empty()) {
            upload(D.id_strings, sid, "string IDs");
            upload(D.id_doms, did, "OM IDs");
            upload(D.id_dom_start, start, "OM ID offsets");
        }
    }
    if (history_entries_) {
        const size_t floats = prop_kernel_max_lanes() * history_entries_ * 4;
        D.hist_ring.alloc(floats, "history ring");
        hip_check(hipMemset(D.hist_ring.get(), 0, floats * 4), "history ring");
    }
    D.rng_x.alloc(max_workitems_, "rng x");
    D.rng_a.alloc(max_workitems_, "rng a");
    num_slots_ = double_buffering_ ? 2 : 1;
    for (int i = 0; i < num_slots_; ++i) {
        Slot &sl = D.slots[i];
        sl.d_steps.alloc(max_workitems_, "steps");
        sl.d_photons.alloc(max_output_photons_, "photons");
        sl.d_hit_count.alloc(4, "hit counter");
        sl.h_steps.alloc(max_workitems_, "pinned steps");
        sl.h_hit_count.alloc(4, "pinned counter");
        if (history_entries_) {
            const size_t floats = static_cast<size_t>(max_output_photons_) * history_entries_ * 4;
            sl.d_hist_out.alloc(floats, "photon histories");
            sl.h_hist.alloc(floats, "pinned photon histories");
        }
        if (mcpe_) {
            if (!D.id_strings) throw Error(CLSIMHIP_ERR_CONFIG, "MCPE generator: the geometry has no DOM");
            sl.d_mcpes.alloc(max_output_photons_, "MCPEs");
            sl.d_mcpe_counters.alloc(8, "MCPE counters");
            sl.h_mcpe_counters.alloc(8, "pinned MCPE counters");
        }
        if (pmt_) {
            if (!D.id_strings) throw Error(CLSIMHIP_ERR_CONFIG, "PMT hit generator: the geometry has no DOM");
            sl.d_pmt_hits.alloc(max_output_photons_, "PMT hits");
            sl.d_pmt_counters.alloc(4, "PMT hit counters");
            sl.h_pmt_counters.alloc(4, "pinned PMT hit counters");
        }
        if (pmt_series_)
            sl.pmt_series.alloc(max_output_photons_, pmt_series_workspace_bytes(max_output_photons_, 0, 0),
                                {"PMT series workspace", "sorted PMT hits", "PMT series table", "PMT series counts", "pinned PMT series counts"});
        if (frame_photons_) {
            if (!D.id_strings) throw Error(CLSIMHIP_ERR_CONFIG, "frame photons: the geometry has no DOM");
            sl.fp.alloc(max_output_photons_, frame_photons_workspace_bytes(max_output_photons_, 0, 0),
                        {"frame photons workspace", "frame photons", "frame photons series table", "frame photons counts", "pinned frame photons counts"});
        }
        if (shadow_) {
            sl.d_lit.alloc(max_output_photons_, "lit photons");
            sl.d_shadow_flags.alloc(max_output_photons_, "cable shadow flags");
            sl.shadow_workspace_bytes = cable_shadow_workspace_bytes(max_output_photons_);
            sl.d_shadow_workspace.alloc(sl.shadow_workspace_bytes, "cable shadow workspace");
            sl.d_shadow_counts.alloc(4, "cable shadow counts");
            sl.h_shadow_counts.alloc(4, "pinned cable shadow counts");
        }
        if (event_stats_) {
            if (!D.id_strings) throw Error(CLSIMHIP_ERR_CONFIG, "event statistics: the geometry has no DOM");
            sl.d_es_counters.alloc(4, "event statistics counts");
            sl.h_es_counters.alloc(4, "pinned event statistics counts");
        }
        if (series_)
            sl.series.alloc(max_output_photons_, mcpe_series_workspace_bytes(max_output_photons_, 0, 0),
                            {"MCPE series workspace", "sorted MCPEs", "MCPE series table", "MCPE series counts", "pinned MCPE series counts"});
        if (merging_) {
            sl.merge_workspace_bytes = mcpe_merge_workspace_bytes(max_output_photons_);
            sl.d_merge_workspace.alloc(sl.merge_workspace_bytes, "MCPE merging workspace");
            sl.d_merged.alloc(max_output_photons_, "merged MCPEs");
            sl.d_merged_series.alloc(max_output_photons_, "merged MCPE series table");
            sl.d_parents.alloc(max_output_photons_, "MCPE parents");
            sl.d_ranges.alloc(max_output_photons_, "MCPE parent ranges");
            sl.d_merge_counts.alloc(4, "MCPE merging counts");
            sl.h_merge_counts.alloc(4, "pinned MCPE merging counts");
        }
        sl.start.create("hipEventCreate");
        sl.stop.create("hipEventCreate");
        sl.counted.create_untimed("hipEventCreate");
        sl.uploaded.create_untimed("hipEventCreate");
    }
    D.queue.alloc(static_cast<size_t>(kQueueWords) * kQueueSlots, "step queue");
    D.work.alloc(max_workitems_, "work records");
#ifdef CLSIMHIP_DEVELOPER
    // DEVELOPER BUILD ONLY (make DEVELOPER=1; tools/build_variant.sh, tools/scan_env.sh): the round 1-5 environment names, through the
    // same door as clsimhip_set_tuning.  The default build reads none of them.
    {
        static const char *const names[][2] = {
            {"CLSIMHIP_K_NEW", "k_new"}, {"CLSIMHIP_K_SEARCH", "k_search"}, {"CLSIMHIP_SLICES", "slices"}, {"CLSIMHIP_K_POP", "k_pop"},
            {"CLSIMHIP_K_WAIT", "k_wait"}, {"CLSIMHIP_K_AIM", "k_aim"}, {"CLSIMHIP_RESULT_MIN_RECORDS", "result_min_records"},
            {"CLSIMHIP_POOL_R", "pool_ring"}, {"CLSIMHIP_POOL_MIN_STEPS", "pool_min_steps"}, {"CLSIMHIP_GRID", "grid"},
            {"CLSIMHIP_NO_FAST", "generic_kernels"}};
        for (const auto &n : names)
            if (const char *e = std::getenv(n[0])) set_tuning(n[1], std::atoll(e));
        if (const char *e = std::getenv("CLSIMHIP_KERNEL")) set_tuning("kernel", std::strcmp(e, "pool") == 0 ? 1 : 2);
        if (const char *e = std::getenv("CLSIMHIP_POOL_INDEX_BITS")) set_tuning("pool_max_steps", (1ll << std::atoi(e)) - 1);
    }
#endif
    // photon histories are kept per lane and the pooled kernel moves photons between lanes; a very large table image
    // leaves its pools no LDS
    std::lock_guard<std::mutex> lk(tuning_mutex_);
    pool_possible_ = history_entries_ == 0 &&
        pool_kernel_fits(static_cast<uint32_t>(tables_.lds_image.size()), stop_detected_ ? 0u : static_cast<uint32_t>(tables_.params.num_strings), tables_.params.num_layers);
    apply_kernel_choice();
}

KParams Converter::launch_params(const LaunchTuning &tuning, const void *d_steps, size_t n, size_t rng_offset, void *d_photons, size_t capacity, void *d_hits,
                                 hipStream_t stream)
{
    DeviceState &D = dev_;
    KParams P = tables_.params;
    P.tables = D.tables.get();
    P.steps = static_cast<const DevStep *>(d_steps);
    P.n_steps = static_cast<uint32_t>(n);
    P.rng_x = D.rng_x.get() + rng_offset;
    P.rng_a = D.rng_a.get() + rng_offset;
    P.out = static_cast<DevPhoton *>(d_photons);
    P.hit_count = static_cast<uint32_t *>(d_hits);
    P.max_hits = static_cast<uint32_t>(std::min<size_t>(capacity, 0xffffffffull));
    {   // step queue head for this launch (zeroed in stream order)
        std::lock_guard<std::mutex> lk(ev_mutex_);
        P.queue = D.queue.get() + static_cast<size_t>(kQueueWords) * (queue_slot_++ % kQueueSlots);
        D.last_queue = P.queue;
    }
    hip_check(hipMemsetAsync(P.queue, 0, kQueueWords * sizeof(uint32_t), stream), "reset step queue");
    P.k_new = tuning.k_new;
    P.k_search = tuning.k_search;
    P.slices = tuning.slices;
    P.k_pop = tuning.k_pop;
    P.k_wait = tuning.k_wait;
    P.k_aim = tuning.k_aim;
    P.pool_ready = tuning.pool_ring;
    P.chip_share = concurrent_launches_;
#ifdef CLSIMHIP_CENSUS
    if (!D.census) D.census.alloc(kCensusBytes / sizeof(unsigned long long), "census");
    P.census = D.census.get();
    hip_check(hipMemsetAsync(P.census, 0, kCensusBytes, stream), "reset census");
    hip_check(hipMemsetAsync(P.census + 8, 0xff, 8, stream), "reset census");
#endif
    P.work = D.work.get() + rng_offset;       // work records live with the stream slots: launches on disjoint slots may overlap
    P.len_table = D.len_table.get();
    P.prox_map = D.prox_map.get();
    P.dom_cells = reinterpret_cast<const uint4 *>(D.dom_prox.get());
    P.dom_centres = reinterpret_cast<const float4 *>(D.dom_centres.get());
    P.dom_named = reinterpret_cast<const uint4 *>(D.dom_named.get());
    P.hist_ring = D.hist_ring.get();
    P.hist_out = nullptr;               // set per slot by submit(); the device path has no history output
    P.dom_tx = D.dom_tx.get();
    P.dom_ty = D.dom_ty.get();
    P.dom_tz = D.dom_tz.get();
    return P;
}

// OpenCL.cxx:1525-1544
void Converter::enqueue_steps(const clsimhip_step *steps, size_t n, uint32_t identifier)
{
    enqueue_steps(steps, n, identifier, nullptr, 0, nullptr, 0);
}

void Converter::enqueue_steps(const clsimhip_step *steps, size_t n, uint32_t identifier, const clsimhip_mcpe_particle *particles, size_t n_particles,
                              const clsimhip_mcpe_mask *masked, size_t n_masked)
{
    need_init();
    if ((particles || n_particles || masked || n_masked) && !series_ && !pmt_series_ && !frame_photons_ && !event_stats_)
        throw Error(CLSIMHIP_ERR_STATE, "a particle table or mask needs the MCPE series stage (clsimhip_set_mcpe_series), the PMT series stage (clsimhip_set_pmt_series), "
                                        "the frame photons stage (clsimhip_set_frame_photons) or the event statistics stage (clsimhip_set_event_statistics)");
    check_worker();
    if (!steps) throw Error(CLSIMHIP_ERR_ARGUMENT, "Steps pointer is (null)!");
    if (n == 0) throw Error(CLSIMHIP_ERR_ARGUMENT, "Steps are empty!");
    if (n > max_workitems_) throw Error(CLSIMHIP_ERR_ARGUMENT, "Number of steps is greater than maximum number of work items!");
    if (n % workgroup_size_ != 0) throw Error(CLSIMHIP_ERR_ARGUMENT, "The number of steps is not a multiple of the workgroup size!");
    Job job;
    job.id = identifier;
    job.n = n;
    for (size_t i = 0; i < n; ++i) job.generated += steps[i].num_photons;
    job.pinned = step_pool_.take(n, std::max(n, std::min(max_workitems_, n + n / 4)), device_);
    if (job.pinned) std::memcpy(job.pinned.get(), steps, n * sizeof(clsimhip_step));
    else job.steps.assign(steps, steps + n);
    // the table and the mask are checked and brought into the stage's form here, in the caller's thread: a bad table is the caller's
    // error, not the worker's
    const auto fill = [&](BunchTable &table, size_t bytes, auto prepare) {
        table.pinned = bunch_pool_.take(bytes, bytes + bytes / 4, device_);
        uint8_t *blob = table.pinned.get();
        if (!blob) {
            table.pageable.resize((bytes + 15u) / 16u);
            blob = table.pageable.data()->bytes;
        }
        table.bunch = prepare(blob);
    };
    if (series_ || pmt_series_)
        fill(job.bunch, series_ ? mcpe_series_blob_bytes(n_particles, n_masked) : pmt_series_blob_bytes(n_particles, n_masked), [&](uint8_t *blob) {
            return series_ ? mcpe_->prepare_series(particles, n_particles, masked, n_masked, blob) : pmt_->prepare_series(particles, n_particles, masked, n_masked, blob);
        });
    if (frame_photons_)
        fill(job.fp_bunch, frame_photons_blob_bytes(n_particles, n_masked), [&](uint8_t *blob) { return fp_doms_->prepare(particles, n_particles, masked, n_masked, blob); });
    if (event_stats_)
        fill(job.es_bunch, event_stats_blob_bytes(n_particles, n_masked), [&](uint8_t *blob) { return event_stats_prepare(particles, n_particles, masked, n_masked, blob); });
    in_queue_->put(std::move(job));
}

// OpenCL.cxx:824-934: upload, launch; everything is queued on the compute stream, nothing waits
void Converter::submit(Slot &s, Job &job)
{
    const LaunchTuning tuning = tuning_snapshot();      // one setting for the whole launch, whatever set_tuning() does meanwhile
    const hipStream_t stream = dev_.stream.get(), upload_stream = dev_.upload_stream.get();
    const size_t n = job.n;
    s.id = job.id;
    s.generated = job.generated;
    s.result_min_records = tuning.result_min_records;
    // (the slot's previous upload finished long ago: its kernel has, or the slot would not be free)
    s.step_lease = std::move(job.pinned);
    const clsimhip_step *source = s.step_lease.get();
    if (!source) {
        std::memcpy(s.h_steps.get(), job.steps.data(), n * sizeof(clsimhip_step));
        source = s.h_steps.get();
    }
    // the upload has a stream of its own: with double buffering it runs while the previous bunch's kernel does
    hip_check(hipMemcpyAsync(s.d_steps.get(), source, n * sizeof(DevStep), hipMemcpyHostToDevice, upload_stream), "upload steps");
    hip_check(hipEventRecord(s.uploaded.get(), upload_stream), "event");
    hip_check(hipStreamWaitEvent(stream, s.uploaded.get(), 0), "wait for the upload");
    hip_check(hipMemsetAsync(s.d_hit_count.get(), 0, 4, stream), "reset hit counter");
    KParams P = launch_params(tuning, s.d_steps.get(), n, 0, s.d_photons.get(), max_output_photons_, s.d_hit_count.get(), stream);
    P.hist_out = s.d_hist_out.get();
    P.id_strings = dev_.id_strings.get(); P.id_doms = dev_.id_doms.get(); P.id_dom_start = dev_.id_dom_start.get();
    hip_check(hipEventRecord(s.start.get(), stream), "event");
    hip_check(launch(P, tuning, stream), "propagation kernel launch");
    hip_check(hipEventRecord(s.stop.get(), stream), "event");
    hip_check(hipMemcpyAsync(s.h_hit_count.get(), s.d_hit_count.get(), 4, hipMemcpyDeviceToHost, stream), "download hit counter");
    hip_check(hipMemcpyAsync(s.h_hit_count.get() + 1, P.queue + 2, 12, hipMemcpyDeviceToHost, stream), "download skipped-step and bad-record counters");
    // A series stage, on the bunch's stream like everything here: the bunch's table from where the job brought it, a workspace that
    // holds it, the stage's kernels (`launch`), and its counts, which stay on the device until finish() fetches them
    const auto run_series_stage = [&](auto &buffers, BunchUpload &upload, BunchTable &table, size_t (*workspace_bytes)(size_t, size_t, size_t), const char *staging_name,
                                      size_t counts_bytes, const char *counts_download, auto launch) {
        const uint8_t *blob = upload.source(table, staging_name);
        buffers.grow_workspace(workspace_bytes(max_output_photons_, table.bunch.n_particles, table.bunch.n_masked));
        launch(blob);
        hip_check(hipMemcpyAsync(buffers.h_counts.get(), buffers.d_counts.get(), counts_bytes, hipMemcpyDeviceToHost, stream), counts_download);
    };
    // what every stage below reads: the records the bunch stored, or -- behind the cable shadow stage, which runs right behind
    // assemble_hits_kernel -- the lit ones among them and their count
    const void *records = s.d_photons.get(), *record_count = s.d_hit_count.get();
    if (shadow_) {
        shadow_->device(device_, s.d_photons.get(), s.d_hit_count.get(), max_output_photons_, s.d_shadow_flags.get(), s.d_lit.get(), s.d_shadow_counts.get(),
                        s.d_shadow_workspace.get(), s.shadow_workspace_bytes, stream);
        hip_check(hipMemcpyAsync(s.h_shadow_counts.get(), s.d_shadow_counts.get(), 12, hipMemcpyDeviceToHost, stream), "download cable shadow counts");
        records = s.d_lit.get();
        record_count = s.d_shadow_counts.get();
    }
    if (mcpe_) {
        // behind assemble_hits_kernel on the bunch's stream, over the records the bunch stored (min(hit counter, capacity)); outside
        // the start / stop pair: the propagation kernel's time stays what it was
        mcpe_->convert_device(device_, records, record_count, max_output_photons_, s.d_mcpes.get(), max_output_photons_, s.d_mcpe_counters.get(), stream);
        hip_check(hipMemcpyAsync(s.h_mcpe_counters.get(), s.d_mcpe_counters.get(), 20, hipMemcpyDeviceToHost, stream), "download MCPE counters");
    }
    if (series_)        // behind the hit maker, over the MCPEs it stored
        run_series_stage(s.series, s.bunch, job.bunch, mcpe_series_workspace_bytes, "pinned MCPE series bunch", 20, "download MCPE series counts", [&](const uint8_t *blob) {
            mcpe_->series_device_prepared(device_, s.d_mcpes.get(), s.d_mcpe_counters.get(), max_output_photons_, job.bunch.bunch, blob, s.series.out.get(),
                                          s.series.series.get(), s.series.d_counts.get(), s.series.workspace.get(), s.series.workspace_bytes, stream);
        });
    if (merging_) {
        // behind the series stage on the same stream, over the records and the table it left; reads its sizes from the stage's counts
        mcpe_merge_device(device_, s.series.out.get(), s.series.series.get(), s.series.d_counts.get(), max_output_photons_, merge_window_, s.d_merged.get(),
                          s.d_merged_series.get(), s.d_parents.get(), s.d_ranges.get(), s.d_merge_counts.get(), s.d_merge_workspace.get(),
                          s.merge_workspace_bytes, stream);
        hip_check(hipMemcpyAsync(s.h_merge_counts.get(), s.d_merge_counts.get(), 8, hipMemcpyDeviceToHost, stream), "download MCPE merging counts");
    }
    if (pmt_) {
        // where the MCPE stage would run: behind assemble_hits_kernel on the bunch's stream, outside the start / stop pair
        pmt_->convert_device(device_, records, record_count, max_output_photons_, s.d_pmt_hits.get(), max_output_photons_, s.d_pmt_counters.get(), stream);
        hip_check(hipMemcpyAsync(s.h_pmt_counters.get(), s.d_pmt_counters.get(), 16, hipMemcpyDeviceToHost, stream), "download PMT hit counters");
    }
    if (pmt_series_)    // behind the PMT hit maker, over the hits it stored
        run_series_stage(s.pmt_series, s.bunch, job.bunch, pmt_series_workspace_bytes, "pinned PMT series bunch", 20, "download PMT series counts", [&](const uint8_t *blob) {
            pmt_->series_device_prepared(device_, s.d_pmt_hits.get(), s.d_pmt_counters.get(), max_output_photons_, job.bunch.bunch, blob, s.pmt_series.out.get(),
                                         s.pmt_series.series.get(), s.pmt_series.d_counts.get(), s.pmt_series.workspace.get(), s.pmt_series.workspace_bytes, stream);
        });
    if (frame_photons_) // behind assemble_hits_kernel, over the records the bunch stored; beside whatever hit maker ran above
        run_series_stage(s.fp, s.fp_bunch, job.fp_bunch, frame_photons_workspace_bytes, "pinned frame photons bunch", 24, "download frame photons counts", [&](const uint8_t *blob) {
            fp_doms_->device_prepared(device_, records, record_count, max_output_photons_, job.fp_bunch.bunch, blob, s.fp.out.get(), s.fp.series.get(),
                                      s.fp.d_counts.get(), s.fp.workspace.get(), s.fp.workspace_bytes, stream);
        });
    if (event_stats_) {
        // behind the upload and behind assemble_hits_kernel: the steps as they were uploaded, and ALL detected photons -- not the lit
        // ones: the reference takes its statistics before the shadow module runs.  (The slot is free: nothing on the device uses its
        // workspace or its records.)
        const SeriesBunch &B = job.es_bunch.bunch;
        const uint8_t *blob = s.es_bunch.source(job.es_bunch, "pinned event statistics bunch");
        const size_t need = event_stats_workspace_bytes(B.n_particles, B.n_masked) + 64;
        if (s.es_workspace_bytes < need) {
            s.d_es_workspace.reset();
            s.d_es_workspace.alloc(need + need / 4, "event statistics workspace");
            s.es_workspace_bytes = need + need / 4;
        }
        s.es_records = B.have_table ? B.n_particles : 1u;
        if (s.es_capacity < s.es_records) {
            s.d_es_out.reset();
            s.es_capacity = s.es_records + s.es_records / 4 + 16;
            s.d_es_out.alloc(s.es_capacity, "event statistics");
        }
        event_stats_device_prepared(device_, s.d_steps.get(), n, s.d_photons.get(), s.d_hit_count.get(), max_output_photons_, B, blob, s.d_es_out.get(),
                                    s.d_es_counters.get(), s.d_es_workspace.get(), s.es_workspace_bytes, stream);
        hip_check(hipMemcpyAsync(s.h_es_counters.get(), s.d_es_counters.get(), 16, hipMemcpyDeviceToHost, stream), "download event statistics counts");
    }
    hip_check(hipEventRecord(s.counted.get(), stream), "event");
}

template <class T>
T *Converter::download(HostRecords<T> &to, PinnedPool<T> &pool, const void *d_from, size_t n, size_t min_records, const char *what)
{
    if (!n) return nullptr;
    T *where = to.take(pool, n, result_capacity(n, min_records), device_);
    hip_check(hipMemcpyAsync(where, d_from, n * sizeof(T), hipMemcpyDeviceToHost, dev_.copy_stream.get()), what);
    return where;
}

// OpenCL.cxx:994-1086: wait for the bunch, download and convert its photons (on the copy stream, so that the
// next bunch's kernel -- already queued on the compute stream -- runs meanwhile), hand the result out
void Converter::finish(Slot &s, std::chrono::steady_clock::time_point &last_done, bool &first)
{
    const hipStream_t copy_stream = dev_.copy_stream.get();
    hip_check(hipEventSynchronize(s.counted.get()), "propagation kernel");
    const uint32_t *counters = s.h_hit_count.get();
    uint32_t hits = counters[0];
    if (counters[1] != 0)
        std::fprintf(stderr, "clsimhip: %u steps of bunch %u have non-finite position/direction/length/beta or a source type without spectrum and were not propagated\n",
                     counters[1], s.id);
    if (counters[3] != 0)           // (queue[4]: assemble_hits_kernel met records whose string / DOM indices name no DOM)
        throw Error(CLSIMHIP_ERR_DEVICE, "photon record with out-of-range string/DOM index");
    if (hits > max_output_photons_) {
        // OpenCL.cxx:1027-1032: logged, truncated
        std::fprintf(stderr, "clsimhip: maximum number of photons exceeded, only receiving %u of %u photons\n", max_output_photons_, hits);
        hits = max_output_photons_;
    }
    // The download lands in a page-locked buffer of the result pool, which then IS the result (no copy, no conversion on this
    // thread: round 2 zero-filled a vector per result, copied the download into it and converted indices one by one -- 0.4 s
    // per bunch of 8.4 M photons in the reference's benchmark, the device idle 80 % of the time).  With every pool buffer in
    // the caller's hands the records go into a plain vector.
    // A series stage's counts: kept, series, UNKNOWN_PARTICLE, MASKED, a module the stage does not have, and with `ties` TIE_OVERFLOW.
    // The fatal ones end the bunch with the stage's words for them (log_fatal in the reference, I3CLSimClientModule.cxx:388-390); else
    // the records and the series to download
    struct FatalWords { const char *stage, *records, *whose; bool ties; };
    struct Kept { uint32_t records, series; };
    const auto series_counts = [&](const uint32_t *c, const FatalWords &w) {
        if ((c[2] | c[4] | (w.ties ? c[5] : 0u)) != 0u)
            throw Error(CLSIMHIP_ERR_DEVICE, std::string(w.stage) + ", bunch " + std::to_string(s.id) + ": " + std::to_string(c[2]) + " " + w.records +
                                                 " of particles the bunch's particle table does not have, " + std::to_string(c[4]) + " at " + w.whose + " does not have" +
                                                 (w.ties ? ", " + std::to_string(c[5]) + " in runs of colliding records beyond the bound" : std::string()));
        const uint32_t kept = std::min(c[0], max_output_photons_);
        return Kept{kept, std::min(c[1], kept)};
    };
    uint32_t n_mcpes = 0;
    if (mcpe_) {
        const uint32_t *mc = s.h_mcpe_counters.get();
        if ((mc[1] | mc[2] | mc[3] | mc[4]) != 0u)      // log_fatal in the reference, all four (I3PhotonToMCPEConverter.cxx:606, 612, 630, 660)
            throw Error(CLSIMHIP_ERR_DEVICE, "MCPE generator, bunch " + std::to_string(s.id) + ": " + std::to_string(mc[1]) + " photons with negative weight, " +
                                                 std::to_string(mc[2]) + " not on the DOM surface, " + std::to_string(mc[3]) + " at a DOM without wavelength acceptance, " +
                                                 std::to_string(mc[4]) + " with hit probability above 1");
        n_mcpes = std::min(mc[0], max_output_photons_);
    }
    uint32_t n_series = 0;
    if (series_) {
        const Kept k = series_counts(s.series.h_counts.get(), {"MCPE series", "MCPEs", "DOMs the generator", false});
        n_mcpes = k.records; n_series = k.series;
    }
    uint32_t n_pmt_hits = 0;
    if (pmt_) {
        const uint32_t *pc = s.h_pmt_counters.get();       // hits, UNKNOWN_MODULE, PROBABILITY_ABOVE_ONE, OFF_SURFACE
        if ((pc[1] | pc[2]) != 0u)                          // log_fatal in the reference (I3PhotonToMCHitConverterForMultiPMT.cxx:283, 349)
            throw Error(CLSIMHIP_ERR_DEVICE, "PMT hit generator, bunch " + std::to_string(s.id) + ": " + std::to_string(pc[1]) + " photons at a module it does not have, " +
                                                 std::to_string(pc[2]) + " with hit probability above 1");
        if (pc[3] != 0u)                                    // log_warn in the reference (:140-145)
            std::fprintf(stderr, "clsimhip: PMT hit generator, bunch %u: %u photons are not within 3 cm of their module's sphere\n", s.id, pc[3]);
        n_pmt_hits = std::min(pc[0], max_output_photons_);
    }
    uint32_t n_pmt_series = 0;
    if (pmt_series_) {
        const Kept k = series_counts(s.pmt_series.h_counts.get(), {"PMT series", "hits", "modules or PMTs the generator", false});
        n_pmt_hits = k.records; n_pmt_series = k.series;
    }
    const Kept fp = frame_photons_ ? series_counts(s.fp.h_counts.get(), {"frame photons", "photons", "DOMs the geometry", true}) : Kept{0u, 0u};
    const uint32_t n_fp = fp.records, n_fp_series = fp.series;
    if (event_stats_ && s.h_es_counters.get()[CLSIMHIP_EVENT_STATISTICS_UNKNOWN_PARTICLE] != 0u)
        throw Error(CLSIMHIP_ERR_DEVICE, "event statistics, bunch " + std::to_string(s.id) + ": " +
                                             std::to_string(s.h_es_counters.get()[CLSIMHIP_EVENT_STATISTICS_UNKNOWN_PARTICLE]) +
                                             " photons of particles the bunch's particle table does not have");
    const uint32_t detected = hits;
    if (!carries_photons()) hits = 0;                   // the records stay on the device
    // (a failure from here on drops r, whose pool buffers go back to their pools)
    Result r;
    const size_t min_records = s.result_min_records;
    clsimhip_photon *where = download(r.photons, result_pool_, s.d_photons.get(), hits, min_records, "download photons");
    if (shadow_) {      // the flags of the records that cross; the counts always (lit, tested, shadowed on the device)
        download(r.shadow_flags, shadow_pool_, s.d_shadow_flags.get(), hits, min_records, "download cable shadow flags");
        r.shadow_counts[0] = s.h_shadow_counts.get()[1];
        r.shadow_counts[1] = s.h_shadow_counts.get()[2];
    }
    if (hits) {
        if (!r.photons.pinned) {
            // every pool buffer is with the caller (or the host refuses to page-lock more): the download goes into pageable memory,
            // which is correct and slower -- said once, because nothing else shows it
            static std::once_flag noted;
            std::call_once(noted, [] {
                std::fprintf(stderr, "clsimhip: every page-locked result buffer is in the caller's hands (release them with "
                                     "clsimhip_release_result); photons are downloaded into pageable memory until one is free\n");
            });
        }
        hip_check(hipStreamSynchronize(copy_stream), "download photons");
        if (!dev_.id_strings) replace_indices(where, hits);      // OpenCL.cxx:1604-1619 does this on the caller thread
    }
    // every stage: its records, behind them its series table, one wait for both
    if (mcpe_) {
        download(r.mcpes, mcpe_pool_, series_ ? s.series.out.get() : s.d_mcpes.get(), n_mcpes, min_records, "download MCPEs");
        download(r.series, series_pool_, s.series.series.get(), n_series, min_records, "download MCPE series table");
        if (merging_ && n_series) {
            const uint32_t n_merged = std::min(s.h_merge_counts.get()[0], n_mcpes), n_parents = std::min(s.h_merge_counts.get()[1], n_mcpes);
            const size_t at_series = static_cast<size_t>(n_merged) * sizeof(clsimhip_mcpe_merged);
            const size_t at_parents = at_series + static_cast<size_t>(n_series) * sizeof(clsimhip_mcpe_series);
            const size_t at_ranges = at_parents + static_cast<size_t>(n_parents) * sizeof(clsimhip_mcpe_parent);
            const size_t bytes = at_ranges + static_cast<size_t>(n_series) * sizeof(clsimhip_mcpe_parent_range);
            r.merge_pinned = merge_pool_.take(bytes, (bytes + bytes / 4 + 4095) / 4096 * 4096, device_);
            uint8_t *blob = r.merge_pinned.get();
            if (!blob) { r.merge_blob.reset(new std::vector<uint64_t>(bytes / 8)); blob = reinterpret_cast<uint8_t *>(r.merge_blob->data()); }
            hip_check(hipMemcpyAsync(blob, s.d_merged.get(), at_series, hipMemcpyDeviceToHost, copy_stream), "download merged MCPEs");
            hip_check(hipMemcpyAsync(blob + at_series, s.d_merged_series.get(), at_parents - at_series, hipMemcpyDeviceToHost, copy_stream), "download merged MCPE series table");
            hip_check(hipMemcpyAsync(blob + at_parents, s.d_parents.get(), at_ranges - at_parents, hipMemcpyDeviceToHost, copy_stream), "download MCPE parents");
            hip_check(hipMemcpyAsync(blob + at_ranges, s.d_ranges.get(), bytes - at_ranges, hipMemcpyDeviceToHost, copy_stream), "download MCPE parent ranges");
            r.merged_count = n_merged;
            r.parent_count = n_parents;
        }
        if (n_mcpes) hip_check(hipStreamSynchronize(copy_stream), "download MCPEs");
        if (series_) r.masked = s.series.h_counts.get()[3];
    }
    if (pmt_) {
        download(r.pmt_hits, pmt_pool_, pmt_series_ ? s.pmt_series.out.get() : s.d_pmt_hits.get(), n_pmt_hits, min_records, "download PMT hits");
        download(r.pmt_series, pmt_series_pool_, s.pmt_series.series.get(), n_pmt_series, min_records, "download PMT series table");
        if (n_pmt_hits) hip_check(hipStreamSynchronize(copy_stream), "download PMT hits");
        if (pmt_series_) r.pmt_masked = s.pmt_series.h_counts.get()[3];
    }
    if (frame_photons_) {
        download(r.fp_records, fp_pool_, s.fp.out.get(), n_fp, min_records, "download frame photons");
        download(r.fp_series, fp_series_pool_, s.fp.series.get(), n_fp_series, min_records, "download frame photons series table");
        if (n_fp) hip_check(hipStreamSynchronize(copy_stream), "download frame photons");
        r.fp_masked = s.fp.h_counts.get()[3];
    }
    if (event_stats_) {
        for (int k = 0; k < 3; ++k) r.es_counters[k] = s.h_es_counters.get()[k];
        if (const size_t n = s.es_records) {
            clsimhip_event_statistics *to = r.es_records.take(es_pool_, n, n + n / 4 + 16, device_);
            hip_check(hipMemcpyAsync(to, s.d_es_out.get(), n * sizeof(clsimhip_event_statistics), hipMemcpyDeviceToHost, copy_stream), "download event statistics");
            hip_check(hipStreamSynchronize(copy_stream), "download event statistics");
        }
    }
    // a result with no photon records but a stage attached is known by a record of its own
    if (!hits && (mcpe_ || pmt_ || frame_photons_ || shadow_ || event_stats_)) r.handle.reset(new clsimhip_photon());
    std::unique_ptr<std::vector<float>> histories;
    if (hits && history_entries_) {
        // ConvertPhotonHistories (OpenCL.cxx:940-989): unroll each ring into forward order
        const size_t N = history_entries_;
        hip_check(hipMemcpyAsync(s.h_hist.get(), s.d_hist_out.get(), static_cast<size_t>(hits) * N * 16, hipMemcpyDeviceToHost, copy_stream), "download photon histories");
        hip_check(hipStreamSynchronize(copy_stream), "download photon histories");
        histories.reset(new std::vector<float>(static_cast<size_t>(hits) * N * 4, 0.f));
        for (size_t i = 0; i < hits; ++i) {
            const uint32_t num_scatters = where[i].num_scatters;
            if (num_scatters == 0) continue;
            const size_t recorded = std::min<size_t>(num_scatters, N);
            size_t cur = (num_scatters <= N) ? 0 : (num_scatters % N);
            for (size_t j = 0; j < recorded; ++j) {
                std::memcpy(&(*histories)[(i * N + j) * 4], &s.h_hist.get()[(i * N + cur) * 4], 16);
                if (++cur >= N) cur = 0;
            }
        }
    }
    float ms = 0.f;
    hip_check(hipEventElapsedTime(&ms, s.start.get(), s.stop.get()), "event time");
    const auto now = std::chrono::steady_clock::now();
    {
        std::lock_guard<std::mutex> lk(stats_mutex_);
        total_device_ns_ += static_cast<uint64_t>(static_cast<double>(ms) * 1e6);
        if (!first) total_host_ns_ += static_cast<uint64_t>(std::chrono::duration_cast<std::chrono::nanoseconds>(now - last_done).count());
        else total_host_ns_ += static_cast<uint64_t>(static_cast<double>(ms) * 1e6);
        ++num_kernel_calls_;
        photons_generated_ += s.generated;
        photons_at_doms_ += detected;
    }
    first = false;
    last_done = now;
    r.id = s.id;
    r.histories = std::move(histories);
    out_queue_->put(std::move(r));
}

// OpenCL.cxx:1142-1315 (thread body).  With double buffering the worker keeps one bunch on the GPU and one in
// post-processing; it never holds a finished bunch back waiting for more input.
void Converter::worker()
{
    (void)hipSetDevice(device_);
    auto last_done = std::chrono::steady_clock::now();
    bool first = true;
    int cur = 0, pending = -1;
    Slot *const slots = dev_.slots;
    Job job;
    try {
        for (;;) {
            bool have;
            if (pending < 0) {
                have = in_queue_->get(job);
                if (!have) break;
            } else {
                // a bunch is running: take the next one as soon as it arrives, but stop waiting when the kernel is done
                have = false;
                while (!(have = in_queue_->get_for(job, 200))) {
                    if (hipEventQuery(slots[pending].counted.get()) == hipSuccess || in_queue_->closed()) break;
                }
                if (!have) {
                    finish(slots[pending], last_done, first);
                    pending = -1;
                    continue;
                }
            }
            submit(slots[cur], job);
            if (pending >= 0) finish(slots[pending], last_done, first);
            if (num_slots_ == 2) {
                pending = cur;
                cur ^= 1;
            } else {
                finish(slots[cur], last_done, first);
            }
        }
        if (pending >= 0) finish(slots[pending], last_done, first);
    } catch (const Error &e) {
        // The reference's worker log_fatal()s on device errors, which ends the process (OpenCL.cxx:768-774).  A C
        // library must not take its host down: the error is logged and kept, both queues are closed so that blocked
        // callers wake up, and every later EnqueueSteps / GetConversionResult returns CLSIMHIP_ERR_DEVICE with this
        // text (the C++ adapter turns that into the exception / log_fatal of the host framework).
        std::fprintf(stderr, "clsimhip: fatal device error in worker thread: %s\n", e.what());
        {
            std::lock_guard<std::mutex> lk(fatal_mutex_);
            fatal_error_ = e.what();
            worker_failed_ = true;
        }
        in_queue_->close();
        out_queue_->close();
    }
}

// OpenCL.cxx:1604-1619
void Converter::get_result(uint32_t *identifier, const clsimhip_photon **photons, size_t *n)
{
    need_init();
    if (!identifier || !photons || !n) throw Error(CLSIMHIP_ERR_ARGUMENT, "output pointers are (null)");
    Result r;
    if (!out_queue_->get(r)) {
        check_worker();
        throw Error(CLSIMHIP_ERR_STATE, "converter is shutting down");
    }
    *identifier = r.id;
    *n = r.photons.count;
    static const clsimhip_photon empty_sentinel{};
    const clsimhip_photon *key = r.photons.count ? r.photons.data() : r.handle.get();
    *photons = key ? key : &empty_sentinel;
    if (key) {
        std::lock_guard<std::mutex> lk(results_mutex_);
        handed_out_[key] = std::move(r);
    }
}

void Converter::result_histories(const clsimhip_photon *photons, const float **histories, uint32_t *entries)
{
    need_init();
    if (!histories || !entries) throw Error(CLSIMHIP_ERR_ARGUMENT, "output pointers are (null)");
    *histories = nullptr;
    *entries = history_entries_;
    std::lock_guard<std::mutex> lk(results_mutex_);
    auto it = handed_out_.find(photons);
    if (it == handed_out_.end()) {
        if (photons) throw Error(CLSIMHIP_ERR_ARGUMENT, "not a result handed out by GetConversionResult (or already released)");
        return;
    }
    if (it->second.histories) *histories = it->second.histories->data();
}

template <class T>
void Converter::result_records(const clsimhip_photon *photons, bool on, HostRecords<T> Result::*payload, const T **records, size_t *n)
{
    need_init();
    if (!records || !n) throw Error(CLSIMHIP_ERR_ARGUMENT, "output pointers are (null)");
    *records = nullptr;
    *n = 0;
    if (!on) return;
    std::lock_guard<std::mutex> lk(results_mutex_);
    auto it = handed_out_.find(photons);
    if (it == handed_out_.end()) throw Error(CLSIMHIP_ERR_ARGUMENT, "not a result handed out by GetConversionResult (or already released)");
    (it->second.*payload).get(records, n);
}

template <class Rec, class Ser>
void Converter::result_series(const clsimhip_photon *photons, bool on, const char *off_text, HostRecords<Rec> Result::*payload, HostRecords<Ser> Result::*table,
                              uint64_t Result::*masked, const Rec **records, size_t *n, const Ser **series, size_t *n_series, uint64_t *n_masked)
{
    need_init();
    if (!records || !n || !series || !n_series) throw Error(CLSIMHIP_ERR_ARGUMENT, "output pointers are (null)");
    if (!on) throw Error(CLSIMHIP_ERR_STATE, off_text);
    *records = nullptr; *series = nullptr;
    *n = 0; *n_series = 0;
    std::lock_guard<std::mutex> lk(results_mutex_);
    auto it = handed_out_.find(photons);
    if (it == handed_out_.end()) throw Error(CLSIMHIP_ERR_ARGUMENT, "not a result handed out by GetConversionResult (or already released)");
    (it->second.*payload).get(records, n);
    (it->second.*table).get(series, n_series);
    if (n_masked) *n_masked = it->second.*masked;
}

void Converter::result_mcpes(const clsimhip_photon *photons, const clsimhip_mcpe **mcpes, size_t *n)
{
    result_records(photons, mcpe_ != nullptr, &Result::mcpes, mcpes, n);
}

void Converter::result_pmt_hits(const clsimhip_photon *photons, const clsimhip_pmt_hit **hits, size_t *n)
{
    result_records(photons, pmt_ != nullptr, &Result::pmt_hits, hits, n);
}

void Converter::result_mcpe_series(const clsimhip_photon *photons, const clsimhip_mcpe **mcpes, size_t *n, const clsimhip_mcpe_series **series, size_t *n_series,
                                   uint64_t *n_masked)
{
    result_series(photons, series_, "the MCPE series stage is off (clsimhip_set_mcpe_series)", &Result::mcpes, &Result::series, &Result::masked, mcpes, n, series,
                  n_series, n_masked);
}

void Converter::result_pmt_series(const clsimhip_photon *photons, const clsimhip_pmt_hit **hits, size_t *n, const clsimhip_pmt_series **series, size_t *n_series,
                                  uint64_t *n_masked)
{
    result_series(photons, pmt_series_, "the PMT series stage is off (clsimhip_set_pmt_series)", &Result::pmt_hits, &Result::pmt_series, &Result::pmt_masked, hits, n,
                  series, n_series, n_masked);
}

void Converter::result_frame_photons(const clsimhip_photon *photons, const clsimhip_frame_photon **records, size_t *n, const clsimhip_mcpe_series **series,
                                     size_t *n_series, uint64_t *n_masked)
{
    result_series(photons, frame_photons_, "the frame photons stage is off (clsimhip_set_frame_photons)", &Result::fp_records, &Result::fp_series, &Result::fp_masked,
                  records, n, series, n_series, n_masked);
}

void Converter::set_cable_shadow(std::shared_ptr<CableShadow> s)
{
    guard();
    compiled_ = false;
    shadow_ = std::move(s);
}

void Converter::result_cable_shadow(const clsimhip_photon *photons, const uint8_t **flags, size_t *n, uint64_t counts[2])
{
    need_init();
    if (!flags || !n || !counts) throw Error(CLSIMHIP_ERR_ARGUMENT, "output pointers are (null)");
    if (!shadow_) throw Error(CLSIMHIP_ERR_STATE, "the cable shadow stage is off (clsimhip_set_cable_shadow)");
    *flags = nullptr;
    *n = 0;
    counts[0] = 0; counts[1] = 0;
    std::lock_guard<std::mutex> lk(results_mutex_);
    auto it = handed_out_.find(photons);
    if (it == handed_out_.end()) throw Error(CLSIMHIP_ERR_ARGUMENT, "not a result handed out by GetConversionResult (or already released)");
    it->second.shadow_flags.get(flags, n);
    counts[0] = it->second.shadow_counts[0];
    counts[1] = it->second.shadow_counts[1];
}

void Converter::result_event_statistics(const clsimhip_photon *photons, const clsimhip_event_statistics **records, size_t *n, uint64_t counters[3])
{
    need_init();
    if (!records || !n) throw Error(CLSIMHIP_ERR_ARGUMENT, "output pointers are (null)");
    if (!event_stats_) throw Error(CLSIMHIP_ERR_STATE, "the event statistics stage is off (clsimhip_set_event_statistics)");
    *records = nullptr;
    *n = 0;
    std::lock_guard<std::mutex> lk(results_mutex_);
    auto it = handed_out_.find(photons);
    if (it == handed_out_.end()) throw Error(CLSIMHIP_ERR_ARGUMENT, "not a result handed out by GetConversionResult (or already released)");
    it->second.es_records.get(records, n);
    if (counters) std::memcpy(counters, it->second.es_counters, sizeof it->second.es_counters);
}

void Converter::set_mcpe_merging(bool on, double window)
{
    guard();
    if (on && !merge_window_ok(window)) throw Error(CLSIMHIP_ERR_ARGUMENT, "MCPE merging: the window must be a number with 0 <= window < +inf");
    compiled_ = false;
    merging_ = on;
    merge_window_ = on ? window : 0.;
}

void Converter::result_mcpe_merged(const clsimhip_photon *photons, const clsimhip_mcpe_merged **merged, size_t *n_merged, const clsimhip_mcpe_series **series,
                                   size_t *n_series, const clsimhip_mcpe_parent **parents, size_t *n_parents, const clsimhip_mcpe_parent_range **ranges)
{
    need_init();
    if (!merged || !n_merged || !series || !n_series || !parents || !n_parents || !ranges) throw Error(CLSIMHIP_ERR_ARGUMENT, "output pointers are (null)");
    if (!merging_) throw Error(CLSIMHIP_ERR_STATE, "the MCPE merging stage is off (clsimhip_set_mcpe_merging)");
    *merged = nullptr; *series = nullptr; *parents = nullptr; *ranges = nullptr;
    *n_merged = 0; *n_series = 0; *n_parents = 0;
    std::lock_guard<std::mutex> lk(results_mutex_);
    auto it = handed_out_.find(photons);
    if (it == handed_out_.end()) throw Error(CLSIMHIP_ERR_ARGUMENT, "not a result handed out by GetConversionResult (or already released)");
    const Result &r = it->second;
    const uint8_t *blob = r.merge_data();
    if (!blob) return;
    const size_t at_series = r.merged_count * sizeof(clsimhip_mcpe_merged);
    const size_t at_parents = at_series + r.series.count * sizeof(clsimhip_mcpe_series);
    const size_t at_ranges = at_parents + r.parent_count * sizeof(clsimhip_mcpe_parent);
    *n_merged = r.merged_count; *n_series = r.series.count; *n_parents = r.parent_count;
    *merged = reinterpret_cast<const clsimhip_mcpe_merged *>(blob);
    *series = reinterpret_cast<const clsimhip_mcpe_series *>(blob + at_series);
    *parents = reinterpret_cast<const clsimhip_mcpe_parent *>(blob + at_parents);
    *ranges = reinterpret_cast<const clsimhip_mcpe_parent_range *>(blob + at_ranges);
}

void Converter::release_result(const clsimhip_photon *photons)
{
    Result gone;                    // (its pool buffers go back to their pools outside the lock)
    std::lock_guard<std::mutex> lk(results_mutex_);
    auto it = handed_out_.find(photons);
    if (it == handed_out_.end()) return;
    gone = std::move(it->second);
    handed_out_.erase(it);
}

// what a new buffer of a result pool holds: a quarter more than the records that arrive, rounded to 4096, at least "result_min_records",
// never more than max_output_photons_
size_t Converter::result_capacity(size_t records, size_t min_records) const
{
    const size_t c = std::max(min_records, (records + records / 4 + 4095) / 4096 * 4096);
    return std::max(records, std::min(c, static_cast<size_t>(max_output_photons_)));
}

size_t Converter::queue_size() const { need_init(); return in_queue_->size(); }
bool Converter::more_photons_available() const { need_init(); return !out_queue_->empty(); }

void Converter::statistics(double out[8]) const
{
    std::lock_guard<std::mutex> lk(stats_mutex_);
    const double dev = static_cast<double>(total_device_ns_), host = static_cast<double>(total_host_ns_);
    const double gen = static_cast<double>(photons_generated_);
    out[0] = dev; out[1] = host; out[2] = static_cast<double>(num_kernel_calls_); out[3] = gen;
    out[4] = static_cast<double>(photons_at_doms_);
    out[5] = dev / gen; out[6] = host / gen; out[7] = dev / host;
}

double Converter::option(int which) const
{
    switch (which) {
    case CLSIMHIP_OPTION_ENABLE_DOUBLE_BUFFERING: return double_buffering_ ? 1. : 0.;
    case CLSIMHIP_OPTION_DOUBLE_PRECISION: return double_precision_ ? 1. : 0.;
    case CLSIMHIP_OPTION_STOP_DETECTED_PHOTONS: return stop_detected_ ? 1. : 0.;
    case CLSIMHIP_OPTION_SAVE_ALL_PHOTONS: return save_all_ ? 1. : 0.;
    case CLSIMHIP_OPTION_SAVE_ALL_PHOTONS_PRESCALE: return save_all_prescale_;
    case CLSIMHIP_OPTION_FIXED_NUMBER_OF_ABSORPTION_LENGTHS: return fixed_abs_lengths_;
    case CLSIMHIP_OPTION_DOM_PANCAKE_FACTOR: return pancake_;
    case CLSIMHIP_OPTION_PHOTON_HISTORY_ENTRIES: return static_cast<double>(history_entries_);
    }
    throw Error(CLSIMHIP_ERR_ARGUMENT, "unknown option");
}

// OpenCL.cxx:1565-1600
void Converter::replace_indices(clsimhip_photon *photons, size_t n) const
{
    const GeoTables &G = tables_.geo;
    for (size_t i = 0; i < n; ++i) {
        const int16_t s = photons[i].string_id;
        const uint16_t d = photons[i].om_id;
        if (s < 0 || static_cast<size_t>(s) >= G.string_index_to_id.size() || d >= G.dom_index_to_id[s].size())
            throw Error(CLSIMHIP_ERR_DEVICE, "photon record with out-of-range string/DOM index");
        const int string_id = G.string_index_to_id[s];
        const unsigned dom_id = G.dom_index_to_id[s][d];
        if (string_id < -32768 || string_id > 32767)
            throw Error(CLSIMHIP_ERR_CONFIG, "Your detector I3Geometry uses a string ID \"" + std::to_string(string_id) + "\". Large IDs like that are currently not supported by clsim.");
        if (dom_id > 65535u)
            throw Error(CLSIMHIP_ERR_CONFIG, "Your detector I3Geometry uses a OM ID \"" + std::to_string(dom_id) + "\". Large IDs like that are currently not supported by clsim.");
        photons[i].string_id = static_cast<int16_t>(string_id);
        photons[i].om_id = static_cast<uint16_t>(dom_id);
    }
}

void Converter::propagate_device(const void *d_steps, size_t n, size_t rng_offset, void *d_photons, size_t capacity,
                                 void *d_hit_count, hipStream_t stream)
{
    need_init();
    if (!d_steps || !d_photons || !d_hit_count) throw Error(CLSIMHIP_ERR_ARGUMENT, "device pointers are (null)");
    if (n == 0) throw Error(CLSIMHIP_ERR_ARGUMENT, "Steps are empty!");
    if (rng_offset + n > max_workitems_) throw Error(CLSIMHIP_ERR_ARGUMENT, "Number of steps is greater than maximum number of work items!");
    if (history_entries_) throw Error(CLSIMHIP_ERR_STATE, "photon histories are only delivered through EnqueueSteps/GetConversionResult");
    DeviceGuard on_device(device_);
    const LaunchTuning tuning = tuning_snapshot();
    std::pair<Event, Event> ev;
    {
        std::lock_guard<std::mutex> lk(ev_mutex_);
        if (!dev_.free_events.empty()) { ev = std::move(dev_.free_events.back()); dev_.free_events.pop_back(); }
    }
    if (!ev.first.get()) { ev.first.create("hipEventCreate"); ev.second.create("hipEventCreate"); }
    hip_check(hipMemsetAsync(d_hit_count, 0, 4, stream), "reset hit counter");
    const KParams P = launch_params(tuning, d_steps, n, rng_offset, d_photons, capacity, d_hit_count, stream);
    hip_check(hipEventRecord(ev.first.get(), stream), "event");
    hip_check(launch(P, tuning, stream), "propagation kernel launch");
    hip_check(hipEventRecord(ev.second.get(), stream), "event");
    std::lock_guard<std::mutex> lk(ev_mutex_);
    dev_.pending_events.push_back(std::move(ev));
}

void Converter::eval_device_function(int what, int layer, bool fast, const float *in4, size_t n, float *out4)
{
    need_init();
    if (!in4 || !out4) throw Error(CLSIMHIP_ERR_ARGUMENT, "in4 / out4 are (null)");
    if (what < CLSIMHIP_EVAL_LENGTHS || what > CLSIMHIP_EVAL_POST_SCATTER_TRANSFORM) throw Error(CLSIMHIP_ERR_ARGUMENT, "unknown function");
    if (what == CLSIMHIP_EVAL_LENGTHS && (layer < 0 || layer >= tables_.params.num_layers)) throw Error(CLSIMHIP_ERR_ARGUMENT, "no such layer");
    if (fast && !tables_.variant.fast) throw Error(CLSIMHIP_ERR_STATE, "this configuration has no FAST instantiation (Compile() could not prove its ranges)");
    if (n > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "too many points");
    DeviceGuard on_device(device_);
    DeviceBuffer<float4> in(n, "hipMalloc"), out(n, "hipMalloc");
    hip_check(hipMemcpy(in.get(), in4, n * 16, hipMemcpyHostToDevice), "hipMemcpy");
    KParams P = tables_.params;
    P.tables = dev_.tables.get();
    P.len_table = dev_.len_table.get();
    hip_check(launch_eval_function(P, tables_.variant.lengths, tables_.variant.tilt, fast, what, layer, in.get(), static_cast<uint32_t>(n), out.get(), nullptr),
              "function tester launch");
    hip_check(hipDeviceSynchronize(), "function tester");
    hip_check(hipMemcpy(out4, out.get(), n * 16, hipMemcpyDeviceToHost), "hipMemcpy");
}

void Converter::eval_device_random(int what, int generator, bool fast, uint64_t *x, const uint32_t *a, size_t n_streams, size_t draws, float *out)
{
    need_init();
    if (!x || !a || !out) throw Error(CLSIMHIP_ERR_ARGUMENT, "x / a / out are (null)");
    if (what < CLSIMHIP_EVAL_RANDOM_UNIFORM || what > CLSIMHIP_EVAL_RANDOM_SCATTERING_COSINE) throw Error(CLSIMHIP_ERR_ARGUMENT, "unknown distribution");
    if (what == CLSIMHIP_EVAL_RANDOM_WAVELENGTH && (generator < 0 || generator >= tables_.params.num_gen)) throw Error(CLSIMHIP_ERR_ARGUMENT, "no such wavelength generator");
    if (fast && !tables_.variant.fast) throw Error(CLSIMHIP_ERR_STATE, "this configuration has no FAST instantiation (Compile() could not prove its ranges)");
    if (n_streams > 0xffffffffull || draws > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "too many draws");
    DeviceGuard on_device(device_);
    DeviceBuffer<uint64_t> dx(n_streams, "hipMalloc");
    DeviceBuffer<uint32_t> da(n_streams, "hipMalloc");
    DeviceBuffer<float> dout(n_streams * draws, "hipMalloc");
    hip_check(hipMemcpy(dx.get(), x, n_streams * 8, hipMemcpyHostToDevice), "hipMemcpy");
    hip_check(hipMemcpy(da.get(), a, n_streams * 4, hipMemcpyHostToDevice), "hipMemcpy");
    KParams P = tables_.params;
    P.tables = dev_.tables.get();
    P.len_table = dev_.len_table.get();
    hip_check(launch_eval_random(P, fast, what, generator, dx.get(), da.get(), static_cast<uint32_t>(n_streams), static_cast<uint32_t>(draws), dout.get(), nullptr),
              "distribution tester launch");
    hip_check(hipDeviceSynchronize(), "distribution tester");
    hip_check(hipMemcpy(out, dout.get(), n_streams * draws * 4, hipMemcpyDeviceToHost), "hipMemcpy");
    hip_check(hipMemcpy(x, dx.get(), n_streams * 8, hipMemcpyDeviceToHost), "hipMemcpy");
}

void Converter::kernel_time(bool reset, double *total_ms, uint64_t *launches)
{
    std::lock_guard<std::mutex> lk(ev_mutex_);
    for (auto &ev : dev_.pending_events) {
        hip_check(hipEventSynchronize(ev.second.get()), "hipEventSynchronize");
        float ms = 0.f;
        hip_check(hipEventElapsedTime(&ms, ev.first.get(), ev.second.get()), "hipEventElapsedTime");
        dev_total_ms_ += ms;
        ++dev_launches_;
    }
    for (auto &ev : dev_.pending_events) dev_.free_events.push_back(std::move(ev));
    dev_.pending_events.clear();
    if (total_ms) *total_ms = dev_total_ms_;
    if (launches) *launches = dev_launches_;
    if (reset) { dev_total_ms_ = 0; dev_launches_ = 0; }
}

long Converter::get_table(const std::string &name, double *out, size_t cap) const
{
    if (!compiled_) throw Error(CLSIMHIP_ERR_STATE, "not compiled");
    if (name == "dom_proximity_map") {                  // 16 MB of bytes: converted on request, not kept as doubles
        const size_t n = tables_.dom_prox.size();
        if (out) for (size_t i = 0; i < std::min(n, cap); ++i) out[i] = tables_.dom_prox[i];
        return static_cast<long>(n);
    }
    if (name == "kernel_variant") {                     // the struct the launchers dispatch on, as Compile() derived it
        const KVariant &v = tables_.variant;
        const double values[6] = {double(v.lengths), v.tilt ? 1. : 0., v.aniso ? 1. : 0., v.flasher ? 1. : 0., v.keep_detected ? 1. : 0., v.fast ? 1. : 0.};
        if (out) std::memcpy(out, values, std::min<size_t>(6, cap) * sizeof(double));
        return 6;
    }
    if (name == "lds_image") {                          // the words every workgroup copies into LDS, as they are uploaded
        const size_t n = tables_.lds_image.size();
        if (out) for (size_t i = 0; i < std::min(n, cap); ++i) out[i] = tables_.lds_image[i];
        return static_cast<long>(n);
    }
    if (name == "dom_named") {
        const size_t n = tables_.dom_named.size();
        if (out) for (size_t i = 0; i < std::min(n, cap); ++i) out[i] = tables_.dom_named[i];
        return static_cast<long>(n);
    }
    if (name == "dom_centres") {
        const size_t n = tables_.dom_centres.size();
        if (out) for (size_t i = 0; i < std::min(n, cap); ++i) out[i] = tables_.dom_centres[i];
        return static_cast<long>(n);
    }
    const auto it = tables_.named.find(name);
    if (it == tables_.named.end()) throw Error(CLSIMHIP_ERR_ARGUMENT, "no table named " + name);
    const size_t n = it->second.size();
    if (out) std::memcpy(out, it->second.data(), std::min(n, cap) * sizeof(double));
    return static_cast<long>(n);
}

void Converter::debug_counters(uint32_t out[4])
{
    need_init();
    DeviceGuard on_device(device_);
    hip_check(hipDeviceSynchronize(), "sync");
#ifdef CLSIMHIP_CENSUS
    hip_check(hipMemcpy(out, dev_.census.get(), kCensusBytes, hipMemcpyDeviceToHost), "download census");     // the caller passes kCensusBytes (4 MiB)
#else
    if (dev_.last_queue) hip_check(hipMemcpy(out, dev_.last_queue, 16, hipMemcpyDeviceToHost), "download counters");
#endif
}

void Converter::get_rng_state(uint64_t *x, size_t count)
{
    need_init();
    if (!x || count > max_workitems_) throw Error(CLSIMHIP_ERR_ARGUMENT, "bad rng state request");
    DeviceGuard on_device(device_);
    hip_check(hipDeviceSynchronize(), "sync");
    hip_check(hipMemcpy(x, dev_.rng_x.get(), count * sizeof(uint64_t), hipMemcpyDeviceToHost), "download rng state");
}

} // namespace clsimhip
