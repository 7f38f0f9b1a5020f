// Host runtime of the MI355X step->photon converter: configuration, table
// compilation, RNG set-up, the worker thread that owns the device, statistics.
// MI355X-native counterpart of I3CLSimStepToPhotonConverterOpenCL
// (private/opencl/I3CLSimStepToPhotonConverterOpenCL.cxx).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>

#include "hip_resources.h"
#include "host_model.h"
#include "baked_kernel.h"
#include "kparams.h"
#include "prop_launch.h"

namespace clsimhip {

class McpeGenerator;            // mcpe.h
class PmtHitGenerator;          // pmt_hits.h
class FramePhotonDoms;          // frame_photons.h
class CableShadow;              // cable_shadow.h
struct alignas(16) SeriesParticle16 { uint8_t bytes[16]; };     // 16-byte aligned storage for a bunch's table and mask (mcpe_series.h)

// RCCL gather of detected photons (comm.cpp)
struct Comm;
void comm_unique_id(uint8_t id[CLSIMHIP_UNIQUE_ID_BYTES]);
Comm *comm_create(int device, int rank, int world, const uint8_t id[CLSIMHIP_UNIQUE_ID_BYTES]);
void comm_destroy(Comm *c);
void comm_info(Comm *c, int *ranks, int *rank, int *device, char *pci_bus_id, size_t pci_bytes);
void comm_statistics(Comm *c, uint64_t *gathers, double *gather_ms, uint64_t *records_sent, uint64_t *records_received, bool reset);
void comm_gather_hits(Comm *c, const void *d_photons, const void *d_hit_count, size_t capacity, int root, void *d_gathered,
                      size_t gathered_capacity, uint64_t *counts_out, hipStream_t stream);

// Result of Compile(): kernel parameters without buffer pointers, the LDS image,
// the DOM templates and the named tables the parity tests read back.
struct CompiledTables {
    KParams params{};
    KVariant variant{};
    std::vector<uint32_t> lds_image;
    std::vector<float> len_table;       // KParams::len_table (TABLE lengths)
    std::vector<uint32_t> prox_map;     // KParams::prox_map
    std::vector<uint32_t> dom_prox;     // KParams::dom_prox
    std::vector<float> dom_centres;     // KParams::dom_centres (4 floats per DOM)
    std::vector<uint32_t> dom_named;    // KParams::dom_named (4 words per DOM)
    GeoTables geo;
    std::map<std::string, std::vector<double>> named;
};
// what Compile() may be told about the search filter's tables ("string_map_cells", "dom_map_cells", "named_search" of
// clsimhip_set_tuning; measurement and the filter-off parity points of tests/): no result depends on it
struct TableTuning {
    int string_map_cells = 512;     // string proximity map: cells per axis (8 ... 4096)
    int dom_map_cells = 256;        // DOM proximity map: at most this many cubic cells per axis (4 ... 512)
    bool named_search = true;       // false: every DOM is marked "not nameable" and takes the full search
};
CompiledTables compile_tables(const MediumData &medium, const GeometryInput &geometry,
                              const std::vector<RandomValueData> &generators, const FunctionData &bias,
                              double pancake_factor, const TableTuning &tuning = TableTuning());

// bounded blocking queue (I3CLSimQueue.h:48-195).  Like the reference's, a consumer that waits in get() counts as
// one free place: with capacity 0 the queue is a rendezvous -- put() returns only once a get() is there to take the
// item (queueFromOpenCL_, OpenCL.cxx:77-78), so size() / empty() show an item only while it is being handed over.
template <class T>
class BoundedQueue {
public:
    explicit BoundedQueue(size_t cap) : cap_(cap) {}
    void put(T v)
    {
        std::unique_lock<std::mutex> lk(m_);
        cond_.wait(lk, [&] { return q_.size() < cap_ + waiting_ || closed_; });
        if (closed_) return;
        q_.push_back(std::move(v));
        cond_.notify_all();
    }
    bool get(T &out)
    {
        std::unique_lock<std::mutex> lk(m_);
        ++waiting_;                     // I3CLSimQueue.h:85-87: tell the producer that somebody is waiting
        cond_.notify_all();
        cond_.wait(lk, [&] { return !q_.empty() || closed_; });
        --waiting_;
        if (q_.empty()) return false;
        out = std::move(q_.front());
        q_.pop_front();
        cond_.notify_all();
        return true;
    }
    // waits at most `us` microseconds; false if nothing arrived (or the queue was closed and is empty)
    bool get_for(T &out, long us)
    {
        std::unique_lock<std::mutex> lk(m_);
        ++waiting_;
        cond_.notify_all();
        const bool got = cond_.wait_for(lk, std::chrono::microseconds(us), [&] { return !q_.empty() || closed_; });
        --waiting_;
        if (!got || q_.empty()) { cond_.notify_all(); return false; }
        out = std::move(q_.front());
        q_.pop_front();
        cond_.notify_all();
        return true;
    }
    bool closed() const { std::lock_guard<std::mutex> lk(m_); return closed_; }
    size_t size() const { std::lock_guard<std::mutex> lk(m_); return q_.size(); }
    bool empty() const { return size() == 0; }
    void close() { std::lock_guard<std::mutex> lk(m_); closed_ = true; cond_.notify_all(); }
private:
    size_t cap_;
    mutable std::mutex m_;
    std::condition_variable cond_;
    std::deque<T> q_;
    size_t waiting_ = 0;
    bool closed_ = false;
};

// Page-locked host buffers of T records that go out on loan and come back: the result photons, the MCPEs and the steps of a
// converter each have one.  take() hands out the smallest free buffer that holds the records; else a new one of `new_capacity`
// records (the caller's sizing rule), for which -- with the pool full -- the smallest free buffer is given back to the host; else
// an empty lease (every buffer is out, or the host refuses to page-lock more: the caller then uses pageable memory).
struct PinnedPoolPolicy {
    int max_buffers;                // buffers that exist at a time
    size_t max_bytes;               // ... and their bytes together, which counts once three exist
    const char *all_out_notice;     // said once (buffers made, records asked for) when every buffer is out; null: nothing is said
};

template <class T>
class PinnedPool {
public:
    // A buffer on loan.  Whoever drops it -- a result released or never fetched, a job the closed queue refused, a slot that takes the
    // next bunch -- returns it to the pool.  The pool outlives its leases (Converter declares its pools before everything that holds
    // one); a lease without a pool frees its buffer, so that no path frees twice or not at all.
    class Lease {
    public:
        Lease() = default;
        Lease(Lease &&o) noexcept = default;
        Lease &operator=(Lease &&o) noexcept
        {
            if (this != &o) { drop(); pool_ = o.pool_; buf_ = std::move(o.buf_); capacity_ = o.capacity_; }
            return *this;
        }
        ~Lease() { drop(); }
        T *get() const { return buf_.get(); }
        size_t capacity() const { return capacity_; }
        explicit operator bool() const { return static_cast<bool>(buf_); }
        void drop() { if (pool_ && buf_) pool_->give(std::move(buf_), capacity_); }
    private:
        friend class PinnedPool;
        Lease(PinnedPool *pool, PinnedBuffer<T> buf, size_t capacity) : pool_(pool), buf_(std::move(buf)), capacity_(capacity) {}
        PinnedPool *pool_ = nullptr;
        PinnedBuffer<T> buf_;
        size_t capacity_ = 0;
    };

    explicit PinnedPool(const PinnedPoolPolicy &policy) : policy_(policy) {}
    Lease take(size_t records, size_t new_capacity, int device)
    {
        const size_t bytes = new_capacity * sizeof(T);
        PinnedBuffer<T> retired;
        {
            // one lock scope for "is there a buffer, may another be made, is one to be replaced" and the count (check and
            // increment were in two scopes, so callers side by side could exceed the limit)
            std::lock_guard<std::mutex> lk(mutex_);
            size_t best = free_.size(), smallest = free_.size();
            for (size_t i = 0; i < free_.size(); ++i) {
                const size_t c = free_[i].capacity;
                if (c >= records && (best == free_.size() || c < free_[best].capacity)) best = i;
                if (smallest == free_.size() || c < free_[smallest].capacity) smallest = i;
            }
            if (best != free_.size()) {
                Lease found(this, std::move(free_[best].buf), free_[best].capacity);
                free_.erase(free_.begin() + static_cast<std::ptrdiff_t>(best));
                return found;
            }
            if (refused_) return Lease();
            if (made_ >= policy_.max_buffers || (bytes_ + bytes > policy_.max_bytes && made_ >= 3)) {
                // A pool whose buffers were sized by small first bunches (warm-up, tests) must not stay too small for production bunches:
                // the smallest FREE buffer goes and one of the needed size takes its place.  With none free every buffer is out.
                if (free_.empty()) {
                    if (policy_.all_out_notice && !noticed_) {
                        noticed_ = true;
                        std::fprintf(stderr, policy_.all_out_notice, made_, records);
                    }
                    return Lease();
                }
                const size_t gone = free_[smallest].capacity * sizeof(T);
                if (bytes_ - gone + bytes > policy_.max_bytes && made_ - 1 >= 3) return Lease();     // (over the byte budget even so)
                retired = std::move(free_[smallest].buf);
                free_.erase(free_.begin() + static_cast<std::ptrdiff_t>(smallest));
                bytes_ -= gone;
                --made_;
            }
            ++made_;
            bytes_ += bytes;
        }
        // (outside the lock: giving memory back to the host and page-locking more take milliseconds)
        DeviceGuard on_device(device);
        retired.reset();
        PinnedBuffer<T> fresh;
        if (!fresh.try_alloc(new_capacity)) {
            std::lock_guard<std::mutex> lk(mutex_);
            --made_;
            bytes_ -= bytes;
            refused_ = true;
            return Lease();
        }
        return Lease(this, std::move(fresh), new_capacity);
    }
    // frees the free buffers and starts over (the converter's teardown, with every lease back and the device current)
    void reset()
    {
        std::lock_guard<std::mutex> lk(mutex_);
        free_.clear();
        made_ = 0; bytes_ = 0; refused_ = false; noticed_ = false;
    }

private:
    void give(PinnedBuffer<T> buf, size_t capacity)
    {
        std::lock_guard<std::mutex> lk(mutex_);
        free_.push_back(Entry{std::move(buf), capacity});
    }
    struct Entry { PinnedBuffer<T> buf; size_t capacity; };
    const PinnedPoolPolicy policy_;
    std::mutex mutex_;
    std::vector<Entry> free_;
    int made_ = 0;
    size_t bytes_ = 0;
    bool refused_ = false;          // the host would not page-lock more
    bool noticed_ = false;
};

// Records of a result on the host: in a buffer of their pool, which the download lands in and the caller reads until the result is
// released, or -- every pool buffer being out -- in a vector of their own
template <class T>
struct HostRecords {
    typename PinnedPool<T>::Lease pinned;
    std::unique_ptr<std::vector<T>> pageable;
    size_t count = 0;
    const T *data() const { return pinned ? pinned.get() : (pageable ? pageable->data() : nullptr); }
    // room for n > 0 records: where to download them to
    T *take(PinnedPool<T> &pool, size_t n, size_t new_capacity, int device)
    {
        count = n;
        pinned = pool.take(n, new_capacity, device);
        if (pinned) return pinned.get();
        pageable.reset(new std::vector<T>(n));
        return pageable->data();
    }
    // what a result_* call hands out
    void get(const T **records, size_t *n) const { *n = count; *records = count ? data() : nullptr; }
};

// What a launch is tuned by ("kernel" ... "result_min_records" of clsimhip_set_tuning) and what Initialize() derives from it.
// A launch works on ONE copy of this, taken under the converter's tuning mutex.
struct LaunchTuning {
    int kernel = 0;                              // "kernel": 0 automatic (by bunch size), 1 pooled, 2 classic for every bunch size
    long long tuned_pool_min_steps = -1;         // "pool_min_steps": -1 = the default threshold
    long long tuned_pool_max_steps = -1;         // "pool_max_steps": -1 = what the pending entries' step index can address; only ever lowers it
    int pool_ring = 0, k_pop = 0;                // pooled kernel: ring entries per wave, lanes serviced at once, 0 = automatic
    int k_new = 0, slices = 0;                   // creation threshold; slices per step, 0 = automatic
    int k_search = 0;                            // lanes parked before a wave searches for DOMs, 0 = automatic
    int k_wait = -1, k_aim = -1;                 // -1 = automatic (pooled kernel only: the classic and keep kernels have them as
                                                 // constants); 0 is honoured: never wait / never ask
    int grid = 0;
    bool generic_only = false;                   // "generic_kernels"
    int baked_kernel = 1;                        // "baked_kernel": the pooled kernel compiled for this configuration (baked_kernel.h): 0 never, 1 for
                                                 // the bunches the launcher itself sends to the pooled kernel, in the instantiation it was measured to pay
                                                 // for (prop_pool_kernel.hip.h: kBakedPays); 2 every instantiation, also where it was forced on smaller bunches
    size_t result_min_records = 65536;           // (tests make the result buffers grow with small bunches)
    // derived by Converter::apply_kernel_choice() once initialized
    bool derived = false;
    bool use_pool = false;                       // pooled kernel allowed
    size_t pool_min_steps = 0;                   // ... for bunches of at least this many steps
    size_t pool_max_steps = 0;                   // ... and at most this many (pool_kernel_max_steps(): the pending entries' 23-bit step index)
    // the pooled kernel pays from ~3 steps per unit slot on: a launch that owns 1/k of the chip reaches that with 1/k of the steps
    bool pooled_for(size_t n_steps, int concurrent_launches) const
    {
        return use_pool && n_steps <= pool_max_steps && n_steps * static_cast<size_t>(concurrent_launches) >= pool_min_steps;
    }
};

class Converter {
public:
    explicit Converter(int device);
    ~Converter();

    // configuration; each throws Error(STATE) once initialized (OpenCL.cxx:1322-1523)
    void set_wlen_generators(std::vector<RandomValueData> g);
    void set_wlen_bias(FunctionData b);
    void set_medium(MediumData m);
    void set_geometry(GeometryInput g);
    void set_double_buffering(bool v) { guard(); double_buffering_ = v; }
    void set_double_precision(bool v) { guard(); double_precision_ = v; }
    void set_stop_detected(bool v) { guard(); stop_detected_ = v; }
    void set_save_all(bool v) { guard(); save_all_ = v; }
    void set_save_all_prescale(double v) { guard(); save_all_prescale_ = v; }
    void set_fixed_abs_lengths(double v) { guard(); fixed_abs_lengths_ = v; }
    void set_pancake(double v) { guard(); pancake_ = v; }
    void set_history_entries(uint32_t v) { guard(); history_entries_ = v; }
    void set_workgroup_size(size_t v);
    void set_max_num_workitems(size_t v);
    // clsimhip_set_mcpe_generator: the hit maker runs behind every bunch's propagation (null: off)
    void set_mcpe_generator(std::shared_ptr<McpeGenerator> g, bool keep_photons);
    // clsimhip_set_mcpe_series: the sorting stage behind the hit maker (mcpe_series.h); needs a generator (Compile() checks)
    void set_mcpe_series(bool on) { guard(); compiled_ = false; series_ = on; }
    // clsimhip_set_mcpe_merging: the merging stage behind the series stage (mcpe_merge.h); needs the series stage (Compile() checks)
    void set_mcpe_merging(bool on, double window);
    // clsimhip_set_pmt_generator: the multi-PMT hit maker runs behind every bunch's propagation (null: off)
    void set_pmt_generator(std::shared_ptr<PmtHitGenerator> g, bool keep_photons);
    // clsimhip_set_pmt_series: the sorting stage behind the PMT hit maker (pmt_series.h); needs a PMT hit generator (Compile() checks)
    void set_pmt_series(bool on) { guard(); compiled_ = false; pmt_series_ = on; }
    // clsimhip_set_frame_photons: the sorting stage behind the propagation kernel's photon records (frame_photons.h), with the
    // geometry's DOMs as its list (Compile() makes it); beside either hit generator or none
    void set_frame_photons(bool on, bool keep_photons) { guard(); compiled_ = false; frame_photons_ = on; fp_keep_photons_ = keep_photons; }
    // clsimhip_set_cable_shadow: the filtering stage right behind assemble_hits_kernel (cable_shadow.h; null: off); every stage above
    // then reads the lit records where it reads the detected ones
    void set_cable_shadow(std::shared_ptr<CableShadow> s);
    // clsimhip_set_event_statistics: the counting stage over the bunch's steps and ALL its detected photons (event_stats.h); beside
    // every other stage or none
    void set_event_statistics(bool on) { guard(); compiled_ = false; event_stats_ = on; }

    void compile();
    void initialize(uint64_t seed);
    void initialize_with_streams(const uint64_t *x, const uint32_t *a, size_t count);
    bool initialized() const { return initialized_; }
    size_t max_workgroup_size() const { return static_cast<size_t>(prop_kernel_block_size()); }
    size_t workgroup_size() const { return workgroup_size_; }
    size_t max_num_workitems() const { return max_workitems_; }

    void enqueue_steps(const clsimhip_step *steps, size_t n, uint32_t identifier);
    // clsimhip_enqueue_steps_with_particles: particles = nullptr is "no table"
    void enqueue_steps(const clsimhip_step *steps, size_t n, uint32_t identifier, const clsimhip_mcpe_particle *particles, size_t n_particles,
                       const clsimhip_mcpe_mask *masked, size_t n_masked);
    void get_result(uint32_t *identifier, const clsimhip_photon **photons, size_t *n);
    void result_histories(const clsimhip_photon *photons, const float **histories, uint32_t *entries);
    void result_mcpes(const clsimhip_photon *photons, const clsimhip_mcpe **mcpes, size_t *n);
    void result_mcpe_series(const clsimhip_photon *photons, const clsimhip_mcpe **mcpes, size_t *n, const clsimhip_mcpe_series **series, size_t *n_series,
                            uint64_t *n_masked);
    void result_mcpe_merged(const clsimhip_photon *photons, const clsimhip_mcpe_merged **merged, size_t *n_merged, const clsimhip_mcpe_series **series,
                            size_t *n_series, const clsimhip_mcpe_parent **parents, size_t *n_parents, const clsimhip_mcpe_parent_range **ranges);
    void result_pmt_hits(const clsimhip_photon *photons, const clsimhip_pmt_hit **hits, size_t *n);
    void result_pmt_series(const clsimhip_photon *photons, const clsimhip_pmt_hit **hits, size_t *n, const clsimhip_pmt_series **series, size_t *n_series,
                           uint64_t *n_masked);
    void result_frame_photons(const clsimhip_photon *photons, const clsimhip_frame_photon **records, size_t *n, const clsimhip_mcpe_series **series,
                              size_t *n_series, uint64_t *n_masked);
    void result_cable_shadow(const clsimhip_photon *photons, const uint8_t **flags, size_t *n, uint64_t counts[2]);
    void result_event_statistics(const clsimhip_photon *photons, const clsimhip_event_statistics **records, size_t *n, uint64_t counters[3]);
    void release_result(const clsimhip_photon *photons);
    size_t queue_size() const;
    bool more_photons_available() const;
    void statistics(double out[8]) const;
    double option(int which) const;

    void propagate_device(const void *d_steps, size_t n, size_t rng_offset, void *d_photons, size_t capacity,
                          void *d_hit_count, hipStream_t stream);
    void replace_indices(clsimhip_photon *photons, size_t n) const;
    void kernel_time(bool reset, double *total_ms, uint64_t *launches);
    long get_table(const std::string &name, double *out, size_t cap) const;
    void get_rng_state(uint64_t *x, size_t count);
    // the reference's tester classes (prop_eval_kernel.hip)
    void eval_device_function(int what, int layer, bool fast, const float *in4, size_t n, float *out4);
    void eval_device_random(int what, int generator, bool fast, uint64_t *x, const uint32_t *a, size_t n_streams, size_t draws, float *out);
    void debug_counters(uint32_t out[4]);
    // SetDevice (OpenCL.cxx:1322-1331): the HIP device ordinal, before Initialize()
    void set_device(int device);
    int device() const { return device_; }
    bool pooled_for(size_t n_steps) const { need_init(); return tuning_snapshot().pooled_for(n_steps, concurrent_launches_); }
    // clsimhip_set_tuning / clsimhip_get_tuning (include/clsimhip.h has the table of keys): launcher parameters, any time between
    // launches; the three table keys before Compile().  The DEFAULT build reads no tuning from the environment.
    void set_tuning(const std::string &key, long long value);
    long long get_tuning(const std::string &key) const;
    void set_concurrent_device_launches(int k);
    int concurrent_device_launches() const { return concurrent_launches_; }
    bool uses_pooled_kernel() const { need_init(); const LaunchTuning t = tuning_snapshot(); return t.use_pool && t.pool_min_steps == 0; }     // for every bunch size
    // clsimhip_get_last_launch: the instantiation the last launch (worker or device path) dispatched to, every field -1 before the first
    KLaunched last_launch() const { std::lock_guard<std::mutex> lk(launched_mutex_); return launched_; }
    // clsimhip_baked_info: what the last pooled launch that wanted the run-time compiled kernel got ("baked_state" of clsimhip_get_tuning)
    BakedReport baked_report() const { std::lock_guard<std::mutex> lk(launched_mutex_); return baked_; }
    // clsimhip_baked_compile: compiles this configuration's pooled kernel without a device (after Compile()); never throws
    BakedResult baked_compile_probe(const char *arch, const char *flags) const;

private:
    using StepPool = PinnedPool<clsimhip_step>;
    using PhotonPool = PinnedPool<clsimhip_photon>;
    using McpePool = PinnedPool<clsimhip_mcpe>;
    using SeriesPool = PinnedPool<clsimhip_mcpe_series>;
    using PmtHitPool = PinnedPool<clsimhip_pmt_hit>;
    using PmtSeriesPool = PinnedPool<clsimhip_pmt_series>;
    using FramePhotonPool = PinnedPool<clsimhip_frame_photon>;
    using EventStatsPool = PinnedPool<clsimhip_event_statistics>;
    using BlobPool = PinnedPool<uint8_t>;
    // A bunch on its way to the worker: the caller's steps are copied ONCE, in the caller's thread, into a page-locked buffer of the
    // step pool, which the worker uploads from (round 5; before, a vector here and a second copy into the slot's staging buffer on
    // the worker thread -- 8 ms per million steps in front of the first kernel of a run).  With every pool buffer in flight the
    // steps travel in a vector as before.
    // With the MCPE series stage the bunch's particle table and mask travel the same way, in the form the stage reads (mcpe_series.h);
    // with the PMT series stage likewise (pmt_series.h: the two stages never run in one converter).  The frame photons stage ranks the
    // geometry's DOMs, not a generator's, so its table and mask travel in a blob of their own; the event statistics stage keys its mask
    // by module, not by rank, and has its own too.
    struct BunchTable { SeriesBunch bunch; BlobPool::Lease pinned; std::vector<SeriesParticle16> pageable; };
    struct Job {
        uint32_t id = 0; size_t n = 0; uint64_t generated = 0; StepPool::Lease pinned; std::vector<clsimhip_step> steps;
        BunchTable bunch, fp_bunch, es_bunch;
    };
    // The records of a result live in page-locked buffers of the converter's pools (back to their pool with release_result, or with
    // a result nobody fetched), or -- when a pool is exhausted because the caller holds more results than it has buffers -- in
    // vectors of their own.
    struct Result {
        uint32_t id = 0;
        HostRecords<clsimhip_photon> photons;
        std::unique_ptr<std::vector<float>> histories;     // [photons][history_entries_][4], forward order
        // with a stage attached, a result that carries no photon record has a record of its own whose address is the result's handle
        std::unique_ptr<clsimhip_photon> handle;
        // with an MCPE generator: the bunch's MCPEs; with the MCPE series stage sorted, with their series table and the MASKED count
        HostRecords<clsimhip_mcpe> mcpes;
        HostRecords<clsimhip_mcpe_series> series;
        uint64_t masked = 0;
        // with the MCPE merging stage: merged records, merged series table, parent table and its ranges, one behind the other (every
        // one starts at a multiple of 8 bytes) in a page-locked buffer of the merge pool or (pool exhausted) a vector
        BlobPool::Lease merge_pinned;
        std::unique_ptr<std::vector<uint64_t>> merge_blob;
        size_t merged_count = 0, parent_count = 0;
        const uint8_t *merge_data() const { return merge_pinned ? merge_pinned.get() : (merge_blob ? reinterpret_cast<const uint8_t *>(merge_blob->data()) : nullptr); }
        // with a PMT hit generator: the bunch's hits; with the PMT series stage sorted, with their series table and the MASKED count
        HostRecords<clsimhip_pmt_hit> pmt_hits;
        HostRecords<clsimhip_pmt_series> pmt_series;
        uint64_t pmt_masked = 0;
        // with the frame photons stage: its records, its series table and its MASKED count
        HostRecords<clsimhip_frame_photon> fp_records;
        HostRecords<clsimhip_mcpe_series> fp_series;
        uint64_t fp_masked = 0;
        // with the cable shadow stage: one flag per photon record the result carries (1 = shadowed), records tested and shadowed
        HostRecords<uint8_t> shadow_flags;
        uint64_t shadow_counts[2] = {0, 0};
        // with the event statistics stage: one record per entry of the bunch's particle table (one without a table), the three counters
        HostRecords<clsimhip_event_statistics> es_records;
        uint64_t es_counters[3] = {0, 0, 0};
    };

    void guard() const { if (initialized_) throw Error(CLSIMHIP_ERR_STATE, "I3CLSimStepToPhotonConverterHIP already initialized!"); }
    void need_init() const { if (!initialized_) throw Error(CLSIMHIP_ERR_STATE, "I3CLSimStepToPhotonConverterHIP is not initialized!"); }
    struct DeviceState;
    void setup_device_buffers(DeviceState &D);
    void release_device();      // frees every device / pinned allocation, stream and event (idempotent)
    void worker();
    void check_worker() const;  // throws the worker thread's device error, if it has died of one
    KParams launch_params(const LaunchTuning &tuning, const void *d_steps, size_t n, size_t rng_offset, void *d_photons, size_t capacity, void *d_hits,
                          hipStream_t stream);

    int device_;
    std::vector<RandomValueData> generators_;
    FunctionData bias_;
    MediumData medium_;
    GeometryInput geometry_;
    bool have_bias_ = false, have_medium_ = false, have_geometry_ = false;
    bool double_buffering_ = false, double_precision_ = false, stop_detected_ = false, save_all_ = false;     // (OpenCL.cxx:83-87: the class's own defaults;
                                                                                                          // initializeOpenCL's callers pass stopDetectedPhotons = true)
    double save_all_prescale_ = 0.001, fixed_abs_lengths_ = NAN, pancake_ = 1.0;
    uint32_t history_entries_ = 0;
    size_t workgroup_size_ = 0, max_workitems_ = 0;
    uint32_t max_output_photons_ = 0;

    std::shared_ptr<McpeGenerator> mcpe_;       // null: no MCPEs are made (the default)
    bool keep_photons_ = true;
    bool series_ = false;                       // the MCPE series stage runs behind the hit maker
    bool merging_ = false;                      // the MCPE merging stage runs behind the series stage
    double merge_window_ = 0.;
    std::shared_ptr<PmtHitGenerator> pmt_;      // null: no PMT hits are made (the default)
    bool pmt_keep_photons_ = true;
    bool pmt_series_ = false;                   // the PMT series stage runs behind the PMT hit maker
    bool frame_photons_ = false;                // the frame photons stage runs behind the propagation kernel
    bool fp_keep_photons_ = true;
    std::shared_ptr<FramePhotonDoms> fp_doms_;  // the geometry's DOMs (Compile())
    std::shared_ptr<CableShadow> shadow_;       // null: every detected photon goes on (the default)
    bool event_stats_ = false;                  // the event statistics stage runs over every bunch's steps and detected photons
    bool carries_photons() const { return !(mcpe_ && !keep_photons_) && !(pmt_ && !pmt_keep_photons_) && !(frame_photons_ && !fp_keep_photons_); }

    std::atomic<bool> compiled_{false}, initialized_{false};    // (atomic: set_tuning() reads them from any thread)
    CompiledTables tables_;

    // The pools come before everything that holds a lease (the device state's slots, the queues, handed_out_): members go in reverse
    // order, so every lease is back before its pool frees the buffers.
    // Result buffers are sized by the photons that arrive: a bunch's download lands in a buffer of at least its own record count (a
    // quarter more, at least "result_min_records", never more than max_output_photons_), which then IS the result until the caller
    // releases it.  At most six exist at a time.  (Rounds 3-4 kept buffers of max_output_photons_ records each -- 840 MB at a
    // million work items, six of them.)  The same for MCPEs (16-byte records).
    PhotonPool result_pool_{PinnedPoolPolicy{6, SIZE_MAX, nullptr}};
    McpePool mcpe_pool_{PinnedPoolPolicy{6, SIZE_MAX, nullptr}};
    SeriesPool series_pool_{PinnedPoolPolicy{6, SIZE_MAX, nullptr}};
    BlobPool merge_pool_{PinnedPoolPolicy{6, SIZE_MAX, nullptr}};
    PmtHitPool pmt_pool_{PinnedPoolPolicy{6, SIZE_MAX, nullptr}};
    PmtSeriesPool pmt_series_pool_{PinnedPoolPolicy{6, SIZE_MAX, nullptr}};
    FramePhotonPool fp_pool_{PinnedPoolPolicy{6, SIZE_MAX, nullptr}};
    SeriesPool fp_series_pool_{PinnedPoolPolicy{6, SIZE_MAX, nullptr}};
    BlobPool shadow_pool_{PinnedPoolPolicy{6, SIZE_MAX, nullptr}};
    EventStatsPool es_pool_{PinnedPoolPolicy{6, SIZE_MAX, nullptr}};
    // particle tables and masks of the bunches on their way (input queue depth + one per slot + the one being filled)
    BlobPool bunch_pool_{PinnedPoolPolicy{8, size_t{1} << 28, nullptr}};
    size_t result_capacity(size_t records, size_t min_records) const;
    // `n` records from the device into a payload of the result being made, queued on the copy stream; where they land (n = 0: null)
    template <class T>
    T *download(HostRecords<T> &to, PinnedPool<T> &pool, const void *d_from, size_t n, size_t min_records, const char *what);
    // the result_* calls: one payload of the result `photons` is the handle of, or a stage's records, series table and MASKED count
    template <class T>
    void result_records(const clsimhip_photon *photons, bool on, HostRecords<T> Result::*payload, const T **records, size_t *n);
    template <class Rec, class Ser>
    void result_series(const clsimhip_photon *photons, bool on, const char *off_text, HostRecords<Rec> Result::*payload, HostRecords<Ser> Result::*table,
                       uint64_t Result::*masked, const Rec **records, size_t *n, const Ser **series, size_t *n_series, uint64_t *n_masked);
    // Step buffers (see Job): input queue depth + one per slot + the one being filled, each sized by the bunch it first carried (a
    // quarter more) and replaced by a larger one when a later bunch needs it, at most 1 GiB in all
    StepPool step_pool_{PinnedPoolPolicy{8, size_t{1} << 30,
        "clsimhip: all %d page-locked step buffers are in flight; this bunch of %zu steps is staged through pageable memory\n"}};

    // What a series stage has in a slot: its workspace (grown when a bunch's table needs it), its records in order, their series
    // table, its counts on the device and where finish() reads them
    struct StageNames { const char *workspace, *out, *series, *counts, *pinned_counts; };
    template <class Rec, class Ser>
    struct SeriesStageBuffers {
        DeviceBuffer<uint8_t> workspace;
        size_t workspace_bytes = 0;
        const char *workspace_name = nullptr;
        DeviceBuffer<Rec> out;
        DeviceBuffer<Ser> series;
        DeviceBuffer<uint32_t> d_counts;
        PinnedBuffer<uint32_t> h_counts;
        void alloc(size_t capacity, size_t initial_workspace_bytes, const StageNames &names)
        {
            workspace_name = names.workspace;
            workspace_bytes = initial_workspace_bytes;
            workspace.alloc(workspace_bytes, names.workspace);
            out.alloc(capacity, names.out);
            series.alloc(capacity, names.series);
            d_counts.alloc(8, names.counts);
            h_counts.alloc(8, names.pinned_counts);
        }
        // for a bunch whose stage needs stage_bytes (the slot is free: nothing on the device uses its workspace)
        void grow_workspace(size_t stage_bytes)
        {
            const size_t need = stage_bytes + 64;
            if (workspace_bytes >= need) return;
            workspace.reset();
            workspace.alloc(need + need / 4, workspace_name);
            workspace_bytes = need + need / 4;
        }
    };
    // Where a slot's table upload reads: the job's pool buffer, which goes back to the pool when the slot is used again, or -- for a
    // job that came without one -- pinned staging of the slot's own
    struct BunchUpload {
        BlobPool::Lease lease;
        PinnedBuffer<uint8_t> staging;
        size_t staging_bytes = 0;
        const uint8_t *source(BunchTable &table, const char *what)
        {
            lease = std::move(table.pinned);
            if (lease) return lease.get();
            if (staging_bytes < table.bunch.bytes) {
                staging.reset();
                staging.alloc(table.bunch.bytes, what);
                staging_bytes = table.bunch.bytes;
            }
            std::memcpy(staging.get(), table.pageable.data(), table.bunch.bytes);
            return staging.get();
        }
    };
    // One buffer set per bunch in flight (OpenCL.cxx:296-340 allocates numBuffers = 1 or 2 of each): while
    // the kernel of bunch k+1 runs, the photons of bunch k are downloaded on the copy stream and converted.
    // (In every struct here events come first: they go before the buffers their work touches.)
    struct Slot {
        Event start, stop, counted, uploaded;
        DeviceBuffer<DevStep> d_steps;
        DeviceBuffer<DevPhoton> d_photons;
        DeviceBuffer<uint32_t> d_hit_count;
        DeviceBuffer<float> d_hist_out;         // photon histories of the slot's hits (history_entries_ float4 each)
        PinnedBuffer<float> h_hist;
        PinnedBuffer<clsimhip_step> h_steps;    // pinned staging (for a job that came without a pool buffer)
        StepPool::Lease step_lease;             // the pool buffer the slot's upload reads; goes back to the pool when the slot is used again
        PinnedBuffer<uint32_t> h_hit_count;
        DeviceBuffer<clsimhip_mcpe> d_mcpes;    // with an MCPE generator: max_output_photons_ records, five counters (mcpe.h)
        DeviceBuffer<uint32_t> d_mcpe_counters;
        PinnedBuffer<uint32_t> h_mcpe_counters;
        DeviceBuffer<clsimhip_pmt_hit> d_pmt_hits;  // with a PMT hit generator: max_output_photons_ records, four counters (pmt_hits.h)
        DeviceBuffer<uint32_t> d_pmt_counters;
        PinnedBuffer<uint32_t> h_pmt_counters;
        // with the MCPE series, the PMT series, the frame photons stage: its buffers; the bunch's table and mask for the hit maker's
        // series stage (the two never run in one converter) and for the frame photons stage
        SeriesStageBuffers<clsimhip_mcpe, clsimhip_mcpe_series> series;
        SeriesStageBuffers<clsimhip_pmt_hit, clsimhip_pmt_series> pmt_series;
        SeriesStageBuffers<clsimhip_frame_photon, clsimhip_mcpe_series> fp;
        BunchUpload bunch, fp_bunch, es_bunch;
        // with the MCPE merging stage: its workspace, merged records, merged series table, parents, ranges, two counts
        DeviceBuffer<uint8_t> d_merge_workspace;
        size_t merge_workspace_bytes = 0;
        DeviceBuffer<clsimhip_mcpe_merged> d_merged;
        DeviceBuffer<clsimhip_mcpe_series> d_merged_series;
        DeviceBuffer<clsimhip_mcpe_parent> d_parents;
        DeviceBuffer<clsimhip_mcpe_parent_range> d_ranges;
        DeviceBuffer<uint32_t> d_merge_counts;
        PinnedBuffer<uint32_t> h_merge_counts;
        // with the cable shadow stage: the lit records (what every stage above reads), one flag per detected record, its workspace,
        // three counts (lit, tested, shadowed)
        DeviceBuffer<DevPhoton> d_lit;
        DeviceBuffer<uint8_t> d_shadow_flags, d_shadow_workspace;
        size_t shadow_workspace_bytes = 0;
        DeviceBuffer<uint32_t> d_shadow_counts;
        PinnedBuffer<uint32_t> h_shadow_counts;
        // with the event statistics stage: its workspace and records (both grown when a bunch's table needs it), four counts (the
        // three counters, the records written)
        DeviceBuffer<uint8_t> d_es_workspace;
        size_t es_workspace_bytes = 0;
        DeviceBuffer<clsimhip_event_statistics> d_es_out;
        size_t es_capacity = 0, es_records = 0;
        DeviceBuffer<uint32_t> d_es_counters;
        PinnedBuffer<uint32_t> h_es_counters;
        uint32_t id = 0;
        uint64_t generated = 0;
        size_t result_min_records = 0;          // of the tuning the bunch was launched with
    };
    // Everything Initialize() creates on the device.  Assigning an empty one releases it all, in declaration order: events and
    // streams before the buffers.
    struct DeviceState {
        std::vector<std::pair<Event, Event>> pending_events, free_events;      // device-resident path: event pairs on the caller's stream (ev_mutex_)
        Stream stream;                          // upload + kernels (bunches serialise here: they share the RNG streams)
        Stream copy_stream;                     // photon download
        Stream upload_stream;                   // step upload of the next bunch while the previous kernel runs
        Slot slots[2];
        DeviceBuffer<uint32_t> tables;
        DeviceBuffer<int16_t> dom_tx, dom_ty;
        DeviceBuffer<float> dom_tz;
        DeviceBuffer<float> len_table;
        DeviceBuffer<uint32_t> prox_map, dom_prox, dom_named;
        DeviceBuffer<float> dom_centres;
        DeviceBuffer<float> hist_ring;          // per resident lane: the last history_entries_ scatter points
        DeviceBuffer<uint64_t> rng_x;
        DeviceBuffer<uint32_t> rng_a;
        // index -> ID tables on the device (host path: converted by assemble_hits_kernel); null when an ID does not fit the record
        DeviceBuffer<int16_t> id_strings;
        DeviceBuffer<uint16_t> id_doms;
        DeviceBuffer<uint32_t> id_dom_start;
        DeviceBuffer<WorkRecord> work;          // per step: work record (kparams.h), rebuilt by every launch
        DeviceBuffer<uint32_t> queue;           // ring of step-queue heads, one per launch in flight
        uint32_t *last_queue = nullptr;
#ifdef CLSIMHIP_CENSUS
        DeviceBuffer<unsigned long long> census;
#endif
    };
    DeviceState dev_;
    int num_slots_ = 1;
    void submit(Slot &s, Job &job);
    void finish(Slot &s, std::chrono::steady_clock::time_point &last_done, bool &first);
    uint32_t queue_slot_ = 0;
    int concurrent_launches_ = 1;            // device path: launches the caller keeps in flight side by side (chip share of each)
    LaunchTuning tuning_;
    TableTuning table_tuning_;
    bool pool_possible_ = false;                 // set by Initialize(): no photon histories, the table image leaves the pools their LDS
    void apply_kernel_choice();                  // (the caller holds tuning_mutex_)
    mutable std::mutex tuning_mutex_;            // tuning_, table_tuning_, pool_possible_: set_tuning() against the launches that read them
    LaunchTuning tuning_snapshot() const { std::lock_guard<std::mutex> lk(tuning_mutex_); return tuning_; }
    hipError_t launch(const KParams &P, const LaunchTuning &tuning, hipStream_t stream) const;
    mutable std::mutex launched_mutex_;          // launched_: the worker (or a device-path caller) writes, any thread reads
    mutable KLaunched launched_;
    mutable BakedReport baked_;                  // (under launched_mutex_ too)

    // worker + queues (in: capacity 5 like queueToOpenCL_, OpenCL.cxx:77)
    std::unique_ptr<BoundedQueue<Job>> in_queue_;
    std::unique_ptr<BoundedQueue<Result>> out_queue_;
    std::thread worker_;
    // a device error in the worker thread: kept for the callers (every later call returns CLSIMHIP_ERR_DEVICE with this text)
    mutable std::mutex fatal_mutex_;
    std::string fatal_error_;
    bool worker_failed_ = false;
    mutable std::mutex results_mutex_;
    std::map<const clsimhip_photon *, Result> handed_out_;

    // statistics (OpenCL.cxx:1088-1140, 1621-1640)
    mutable std::mutex stats_mutex_;
    uint64_t total_device_ns_ = 0, total_host_ns_ = 0, num_kernel_calls_ = 0, photons_generated_ = 0, photons_at_doms_ = 0;

    // device-resident path: the event pairs of DeviceState
    std::mutex ev_mutex_;
    double dev_total_ms_ = 0;
    uint64_t dev_launches_ = 0;
};

} // namespace clsimhip
