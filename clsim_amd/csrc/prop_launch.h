// What the kernel launchers share, host code only: their prototypes, the checks they all make, the one mapping from a KVariant's
// run-time switches to a kernel template's arguments, and the per-kernel launch plan (CUs, resident workgroups, the dynamic-LDS
// attribute).  The kernels and their launch arithmetic live with the kernel templates (prop_kernel.hip.h, prop_pool_kernel.hip.h).
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>

#include <map>
#include <mutex>
#include <tuple>
#include <type_traits>

#include "../../include/clsimhip.h"
#include "kparams.h"

namespace clsimhip {

// ---- prop_kernel.hip: one photon per lane ----
hipError_t launch_prop_kernel(const KParams &P, const KVariant &v, hipStream_t stream);
size_t prop_kernel_lds_bytes(uint32_t table_words);
int prop_kernel_block_size();
size_t prop_kernel_max_lanes();
size_t prop_kernel_lds_budget();
hipError_t launch_keep_kernel(const KParams &P, const KVariant &v, hipStream_t stream);     // prop_keep_kernel.hip: without STOP_PHOTONS_ON_DETECTION
hipError_t launch_tab_kernel(const KParams &P, const KVariant &v, hipStream_t stream);      // prop_tab_kernel.hip: the table maker
// ---- prop_pool_kernel.hip: pooled scheduling, same results, propagation without photon histories only ----
hipError_t launch_pool_kernel(const KParams &P, const KVariant &v, hipStream_t stream);
bool pool_kernel_fits(uint32_t table_words, uint32_t keep_strings, int num_layers);
size_t pool_kernel_max_steps();     // bunches beyond this many steps do not fit the pooled kernel's pending entries (23-bit step index)
hipError_t launch_pool_keep_kernel(const KParams &P, const KVariant &v, hipStream_t stream);     // prop_pool_keep_kernel.hip: without STOP_PHOTONS_ON_DETECTION
// ---- prop_aux_kernels.hip: the passes before and after every propagation launch, the math probes ----
hipError_t launch_scan_steps(const KParams &P, hipStream_t stream);
hipError_t launch_assemble_hits(const KParams &P, bool flasher, hipStream_t stream);
hipError_t launch_eval_math(int what, const float *xs, const float *ys, uint32_t n, float *out, hipStream_t stream);
hipError_t launch_check_math(int what, int exp_lo, int exp_hi, uint32_t *result, uint32_t result_cap, hipStream_t stream);
// ---- index_clamp_check_kernel.hip: launch_check_math's what = 20 ----
hipError_t launch_check_index_clamp(uint32_t *result, uint32_t result_cap, hipStream_t stream);
// ---- prop_eval_kernel.hip: single functions of the propagator ----
hipError_t launch_eval_function(const KParams &P, int lengths_kind, bool has_tilt, bool fast, int what, int layer, const float4 *in, uint32_t n, float4 *out,
                                hipStream_t stream);
hipError_t launch_eval_random(const KParams &P, bool fast, int what, int generator, uint64_t *x, const uint32_t *a, uint32_t n_streams, uint32_t draws,
                              float *out, hipStream_t stream);
// ---- steps_kernel.hip: step generators ----
hipError_t launch_generate_flasher_steps(const clsimhip_flasher_config &cfg, const clsimhip_flasher_request *d_requests, const void *d_plan,
                                         uint32_t n_requests, uint64_t total, uint64_t seed, const float *d_profiles, void *d_out,
                                         hipStream_t stream);
hipError_t launch_generate_steps(const clsimhip_step_request *d_requests, const uint64_t *d_first_step, uint32_t n_requests,
                                 uint64_t total_real, uint64_t total_padded, uint64_t seed, void *d_out, hipStream_t stream);

// A lengths kind the kernels are instantiated for, and for TABLE its table
inline hipError_t check_lengths(const KParams &P, const KVariant &v)
{
    if (v.lengths < CLSIMHIP_LENGTHS_CONSTANT || v.lengths > CLSIMHIP_LENGTHS_TABLE) return hipErrorInvalidValue;
    if (v.lengths == CLSIMHIP_LENGTHS_TABLE && (!P.len_table || P.len_tab_n < 2)) return hipErrorInvalidValue;
    return hipSuccess;
}

// Run-time values as compile-time tags: f receives std::integral_constant objects and reads its template arguments from their types.
// The order in which the tags are named here is the order in which a translation unit's kernels are instantiated, hence their order
// in its code object: lengths kinds and switches ascending, FAST before generic -- the order the kernels have always had (the last
// kernel of a code object has no padding behind it, which tools/code_hash.py sees).
template <typename F>
hipError_t dispatch_lengths(int lengths, F &&f)
{
    switch (lengths) {
    case CLSIMHIP_LENGTHS_CONSTANT: return f(std::integral_constant<int, CLSIMHIP_LENGTHS_CONSTANT>{});
    case CLSIMHIP_LENGTHS_ICECUBE: return f(std::integral_constant<int, CLSIMHIP_LENGTHS_ICECUBE>{});
    case CLSIMHIP_LENGTHS_TABLE: return f(std::integral_constant<int, CLSIMHIP_LENGTHS_TABLE>{});
    }
    return hipErrorInvalidValue;
}
template <typename F> hipError_t dispatch_switch(bool on, F &&f) { return !on ? f(std::false_type{}) : f(std::true_type{}); }
template <typename F> hipError_t dispatch_fast(bool fast, F &&f) { return fast ? f(std::true_type{}) : f(std::false_type{}); }
// The instantiation of a propagation family for (v.lengths, v.tilt, v.aniso, v.flasher, fast): f(lengths, tilt, aniso, flasher, fast) is
// called with the five tags; a lengths kind out of range is an error and f is not called.  ALWAYS_FLASHER (the table maker, which looks
// at the source type per step): v.flasher is not consulted and f is only ever instantiated with flasher = true.
template <bool ALWAYS_FLASHER = false, typename F>
hipError_t dispatch_variant(const KVariant &v, bool fast, F &&f)
{
    return dispatch_lengths(v.lengths, [&](auto lengths) {
        return dispatch_switch(v.tilt, [&](auto tilt) {
            return dispatch_switch(v.aniso, [&](auto aniso) {
                const auto rest = [&](auto flasher) {
                    return dispatch_fast(fast, [&](auto fast_tag) { return f(lengths, tilt, aniso, flasher, fast_tag); });
                };
                if constexpr (ALWAYS_FLASHER) return rest(std::true_type{});
                else return dispatch_switch(v.flasher, rest);
            });
        });
    });
}

// Persistent grids are sized by what the chip holds at once.  CU count, occupancy and the function attribute are per (current device,
// kernel, block size, LDS bytes of the workgroup: the image differs per configuration): one process may drive converters on several
// GPUs (the reference's usual model, I3CLSimServer.cxx:77-137) and from several threads.  Asked of the runtime once per key; a key
// whose calls failed is asked again.  block = 0: only the attribute (a kernel whose grid does not depend on occupancy).
struct LaunchPlan { int cus = 0, resident = 0; };
inline hipError_t plan_launch(const void *kernel, int block, size_t lds_bytes, LaunchPlan &plan)
{
    static std::mutex mutex;
    static std::map<std::tuple<int, const void *, int, size_t>, LaunchPlan> plans;
    int device = 0;
    if (const hipError_t e = hipGetDevice(&device)) return e;
    std::lock_guard<std::mutex> lk(mutex);
    LaunchPlan &pl = plans[std::make_tuple(device, kernel, block, lds_bytes)];
    if (pl.resident == 0) {
        int cus = 0, per_cu = 0;
        hipError_t e = !block ? hipSuccess : hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
        if (e == hipSuccess && lds_bytes > 64 * 1024)
            e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e == hipSuccess && block) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, lds_bytes);
        if (e != hipSuccess) return e;
        if (per_cu < 1) per_cu = 1;
        if (cus < 1) cus = 1;
        pl = LaunchPlan{cus, cus * per_cu};
    }
    plan = pl;
    return hipSuccess;
}
// A workgroup's dynamic LDS beyond 64 KB needs the function attribute: set once per (device, kernel, size)
inline hipError_t allow_dynamic_lds(const void *kernel, size_t lds_bytes)
{
    LaunchPlan unused;
    return (lds_bytes > 64 * 1024) ? plan_launch(kernel, 0, lds_bytes, unused) : hipSuccess;
}

} // namespace clsimhip
