// The kernels around and beside propagation, compiled once with the propagation kernels' code generation (Makefile: KERNEL_CODEGEN):
// the pass that turns a bunch's steps into work records before every propagation launch, the pass that expands hit stubs into
// photon records after it, and the math probes of the tests.  Device functions: prop_device.hip.h, detmath.hip.h.
#include <hip/hip_runtime.h>

#include "prop_device.hip.h"
#include "prop_launch.h"

namespace clsimhip {

// meta[1] = largest numPhotons of the bunch (sizes the slices of the unit queue)
__global__ void __launch_bounds__(256) scan_steps_kernel(const DevStep *steps, uint32_t n, uint32_t *meta, WorkRecord *work,
                                                         const uint64_t *rng_x, const uint32_t *rng_a, uint32_t num_generators)
{
    // one pass over the bunch: largest numPhotons (-> slice size) and the work records
    uint32_t m = 0;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        WorkRecord r;
        r.step = steps[i];
        r.x = rng_x[i];
        r.a = rng_a[i];
        r.done = 0u;
        {   // A step with a non-finite field makes the reference's photon loop spin forever (a NaN absorption budget
            // never drops below EPSILON); here that would hang the GPU.  Such a step propagates no photons and is
            // counted in meta[2]; its RNG stream is left alone.
            const float f[8] = {r.step.x, r.step.y, r.step.z, r.step.t, r.step.theta, r.step.phi, r.step.length, r.step.beta};
            bool finite = true;
#pragma unroll
            for (int k = 0; k < 8; ++k) finite = finite && (__builtin_fabsf(f[k]) <= 3.0e38f);
            // likewise a source type without a wavelength generator: generateWavelength() returns 0 for it
            // (MediumPropertiesSource.cxx:392-432) and every length of that photon becomes 0/0
            const bool no_spectrum = (num_generators > 1u) && ((r.step.source_type_and_pad & 0xffu) >= num_generators);
            if ((!finite || no_spectrum) && r.step.num_photons != 0u) { r.step.num_photons = 0u; atomicAdd(meta + 2, 1u); }
        }
        {   // The work record's step is the view photon creation needs: the direction of the step (c.cl:482-489), two
            // sincos per step here instead of per photon, takes the place of theta, phi and of the weight, which only a hit
            // record needs -- and that reads the caller's step array (make_hit_record, save_path_wave)
            const Vec3 d = step_direction(&r.step);
            r.step.theta = d.x; r.step.phi = d.y; r.step.weight = d.z;
        }
        work[i] = r;
        const uint32_t v = r.step.num_photons;
        m = v > m ? v : m;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)m, off);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63u) == 0u && m != 0u) atomicMax(meta + 1, m);
}

// Expands the hit stubs of one launch into I3CLSimPhoton records, in place (slot i -> record i).
template <bool FLASHER>
__global__ void __launch_bounds__(256) assemble_hits_kernel(const KParams Pvalue)
{
    const KP P = (KP)__builtin_amdgcn_kernarg_segment_ptr();
    (void)Pvalue;
    {
        const uint32_t words = P->table_words;
        const uint32_t *src = P->tables;
        for (uint32_t i = threadIdx.x; i < words; i += 256) lds_words[i] = src[i];
    }
    __syncthreads();
    const uint32_t counted = *P->hit_count;
    const uint32_t n = counted < P->max_hits ? counted : P->max_hits;
    uint32_t *out_words = reinterpret_cast<uint32_t *>(P->out);
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        uint32_t *slot = out_words + (size_t)i * 20u;
        HitStub h;
        uint32_t *hw = reinterpret_cast<uint32_t *>(&h);
#pragma unroll
        for (int w = 0; w < kStubWords; ++w) hw[w] = slot[w];
        // A stub whose indices name no step / string / DOM (a corrupted record) is not expanded -- expanding it would read the step, the
        // stream multiplier and the DOM tables out of range -- it stays as it is and is counted in queue[4]: the host path then fails
        // the bunch like its own conversion would (converter.cpp: finish / replace_indices).  id_dom_start has one entry more than
        // there are strings.
        const uint32_t s_index = h.string_and_dom & 0xffffu, d_index = h.string_and_dom >> 16;
        bool named = (h.step_index < P->n_steps) && (s_index < (uint32_t)P->num_strings);
        if (named && P->id_strings) named = d_index < P->id_dom_start[s_index + 1u] - P->id_dom_start[s_index];
        if (!named) {
            atomicAdd(P->queue + 4, 1u);
            continue;
        }
        uint32_t rec[20];
        const float abs_lens_initial = make_hit_record<FLASHER>(P, h, rec);
        if (P->id_strings)                   // index -> ID (OpenCL.cxx:1565-1600), same for every record: wave-uniform branch
            rec[11] = (uint32_t)(uint16_t)P->id_strings[s_index] | ((uint32_t)P->id_doms[P->id_dom_start[s_index] + d_index] << 16);
#pragma unroll
        for (int w = 0; w < 20; ++w) slot[w] = rec[w];
        // c.cl:836: the ring holds the absorption lengths LEFT at each scatter; the reference stores initial - left
        const uint32_t hn = (uint32_t)P->history_n;
        for (uint32_t k = 0; k < hn; ++k) {
            float *w = P->hist_out + ((size_t)i * hn + k) * 4u + 3u;
            *w = abs_lens_initial - *w;
        }
    }
}

// ---- math probe used by tests/test_detmath_gpu.py ----
__global__ void eval_math_kernel(int what, const float *xs, const float *ys, uint32_t n, float *out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = xs[i], y = ys ? ys[i] : 0.0f;
    float r = 0.0f, s, c;
    switch (what) {
    case 0: r = dm::log_(x); break;
    case 1: r = dm::exp_(x); break;
    case 2: dm::sincos_(x, s, c); r = s; break;
    case 3: dm::sincos_(x, s, c); r = c; break;
    case 4: r = dm::powr_(x, y); break;
    case 5: r = dm::acos_(x); break;
    case 6: r = dm::atan2_(x, y); break;
    case 7: r = dm::rsqrt_(x); break;
    case 8: r = dm::sqrt_(x); break;
    case 9: r = x / y; break;
    case 10: r = dm::acos_f(x); break;
    case 11: r = dm::rcp_(x); break;
    case 12: r = dm::sqrt_near_(x); break;
    case 13: r = dm::rsqrt_near_(x); break;
    case 14: r = dm::powr_unit_(x, y); break;
    case 15: r = dm::cbrt_(x); break;
    case 16: r = dm::div_near_(x, y); break;
    default: break;
    }
    out[i] = r;
}

// Exhaustive proof runs for the range-restricted operations of detmath.hip.h: every significand (2^23) x every binary
// exponent in [exp_lo, exp_hi], both signs for the reciprocal, against the IEEE operation.  what: 11 rcp_, 12 sqrt_near_,
// 13 rsqrt_near_; 16 div_near_ (two-argument: see the kernel); 17 rcp_of_rcp_(rcp_(x), x) against 1/(1/x); 18 rsqrt_unit_ on its window;
// 19 the table maker's axis_bin_ on every bit pattern (exponents do not apply).
// result[0] = mismatches, result[1..] = bit patterns of the first few mismatching arguments.
__global__ void check_math_kernel(int what, int exp_lo, int exp_hi, uint32_t *result, uint32_t result_cap)
{
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;        // significand bits
    if (m >= (1u << 23)) return;
    if (what == 19) {
        // axis_bin_ against axis_bin_generic_: every one of the 2^32 bit patterns (512 per thread) x five bin counts
        for (uint32_t k = 0; k < 512u; ++k) {
            const float t = dm::u2f((m << 9) | k);
            const int counts[5] = {1, 36, 105, 200, 65534};
            for (int c = 0; c < 5; ++c) {
                const int nb = __builtin_amdgcn_readfirstlane(counts[c]);
                if (axis_bin_(t, nb) != axis_bin_generic_(t, nb)) {
                    const uint32_t k2 = atomicAdd(result, 1u);
                    if (k2 + 1u < result_cap) result[k2 + 1u] = dm::f2u(t);
                }
            }
        }
        return;
    }
    if (what == 16) {
        // div_near_: every divisor significand x the divisor exponents [exp_lo, exp_hi] x both divisor signs x 40 numerators:
        // 32 pseudo-random ones over the whole admissible range and both signs, and 8 built from the divisor (exact and
        // nearly exact quotients, all-ones and power-of-two significands), where a wrong last bit would show first
        for (int e = exp_lo; e <= exp_hi; ++e) {
            const uint32_t bbits = ((uint32_t)(e + 127) << 23) | m;
            for (int j = 0; j < 40; ++j) {
                uint32_t h = (m * 2654435761u) ^ ((uint32_t)(e + 1000) * 40503u) ^ ((uint32_t)j * 2246822519u);
                h ^= h >> 15; h *= 2246822519u; h ^= h >> 13; h *= 3266489917u; h ^= h >> 16;
                uint32_t abits;
                if (j < 32) {
                    const uint32_t ae = 127u - 40u + (h >> 23) % 101u;                     // exponents -40 ... 60
                    abits = (h & 0x807fffffu) | (ae << 23);
                } else {
                    const uint32_t ae = 127u - 40u + (h >> 9) % 101u;
                    const uint32_t k = (h & 7u) + 1u;
                    const float bb = dm::u2f((127u << 23) | m);                            // the divisor's significand in [1, 2)
                    float t;
                    switch (j - 32) {
                        case 0: t = bb * (float)k; break;                                   // exact small quotients (when the product is exact)
                        case 1: t = dm::u2f(dm::f2u(bb * (float)k) + 1u); break;            // ... and their neighbours
                        case 2: t = dm::u2f(dm::f2u(bb * (float)k) - 1u); break;
                        case 3: t = dm::u2f((127u << 23) | 0x7fffffu); break;               // all ones
                        case 4: t = 1.0f; break;                                           // a power of two: the quotient is RN(1/b) scaled
                        case 5: t = dm::u2f((127u << 23) | (0x7fffffu & ~m)); break;        // complement of the divisor's bits
                        case 6: t = bb * bb; break;                                        // quotient close to the divisor itself
                        default: t = dm::u2f((127u << 23) | ((m + k) & 0x7fffffu)); break;  // quotient within a few ulp of one
                    }
                    abits = (dm::f2u(t) & 0x007fffffu) | (ae << 23) | (h & 0x80000000u);
                }
                for (int sign = 0; sign < 2; ++sign) {
                    const float b = dm::u2f(bbits | ((uint32_t)sign << 31)), a = dm::u2f(abits);
                    const float want = a / b, got = dm::div_near_(a, b);
                    if (dm::f2u(want) != dm::f2u(got)) {
                        const uint32_t k2 = atomicAdd(result, 1u);
                        if (k2 + 2u < result_cap && (k2 & 1u) == 0u) { result[k2 + 1u] = dm::f2u(a); result[k2 + 2u] = dm::f2u(b); }
                    }
                }
            }
        }
        return;
    }
    for (int e = exp_lo; e <= exp_hi; ++e) {
        const uint32_t bits = ((uint32_t)(e + 127) << 23) | m;
        for (int sign = 0; sign < ((what == 11 || what == 17) ? 2 : 1); ++sign) {
            const float x = dm::u2f(bits | ((uint32_t)sign << 31));
            float want, got;
            if (what == 18) {       // rsqrt_unit_: the 2047 patterns of its window (exponents and the rest of the significands do not apply)
                if (e != exp_lo || sign != 0 || m > 2046u) continue;
                const float xx = dm::u2f(0x3f800000u - 1023u + m);
                want = 1.0f / __builtin_sqrtf(xx); got = dm::rsqrt_unit_(xx);
                if (!dm::rsqrt_unit_ok_(xx) || dm::rsqrt_unit_ok_(dm::u2f(0x3f800000u + 1024u)) || dm::rsqrt_unit_ok_(dm::u2f(0x3f800000u - 1024u))) got = 0.0f;
                if (dm::f2u(want) != dm::f2u(got)) { const uint32_t k = atomicAdd(result, 1u); if (k + 1u < result_cap) result[k + 1u] = dm::f2u(xx); }
                continue;
            }
            if (what == 17) { const float b = 1.0f / x; want = 1.0f / b; got = dm::rcp_of_rcp_(dm::rcp_(x), x); }       // (rcp_(x) == b: what = 11)
            else if (what == 11) { want = 1.0f / x; got = dm::rcp_(x); }
            else if (what == 12) { want = __builtin_sqrtf(x); got = dm::sqrt_near_(x); }
            else { want = 1.0f / __builtin_sqrtf(x); got = dm::rsqrt_near_(x); }
            if (dm::f2u(want) != dm::f2u(got)) {
                const uint32_t k = atomicAdd(result, 1u);
                if (k + 1u < result_cap) result[k + 1u] = dm::f2u(x);
            }
        }
    }
}

// ---- host-side launchers (scan_steps, assemble_hits: called by launch_variant and launch_pool_variant around every propagation launch) ----
hipError_t launch_scan_steps(const KParams &P, hipStream_t stream)
{
    const uint32_t sgrid = (P.n_steps + 255u) / 256u;
    hipLaunchKernelGGL(scan_steps_kernel, dim3(sgrid < 1024u ? sgrid : 1024u), dim3(256), 0, stream, P.steps, P.n_steps, P.queue,
                       P.work, P.rng_x, P.rng_a, (uint32_t)P.num_gen);
    return hipGetLastError();
}

// second pass (same stream): stubs -> I3CLSimPhoton records.  Hits are ~1e-3 of the photons.
hipError_t launch_assemble_hits(const KParams &P, bool flasher, hipStream_t stream)
{
    const size_t image_bytes = (size_t)P.table_words * 4;
    const void *kernel = flasher ? reinterpret_cast<const void *>(&assemble_hits_kernel<true>) : reinterpret_cast<const void *>(&assemble_hits_kernel<false>);
    if (const hipError_t e = allow_dynamic_lds(kernel, image_bytes)) return e;
    if (flasher) hipLaunchKernelGGL((assemble_hits_kernel<true>), dim3(512), dim3(256), image_bytes, stream, P);
    else hipLaunchKernelGGL((assemble_hits_kernel<false>), dim3(512), dim3(256), image_bytes, stream, P);
    return hipGetLastError();
}

hipError_t launch_check_math(int what, int exp_lo, int exp_hi, uint32_t *result, uint32_t result_cap, hipStream_t stream)
{
    if (what == 20) return launch_check_index_clamp(result, result_cap, stream);        // (index_clamp_check_kernel.hip)
    hipLaunchKernelGGL(check_math_kernel, dim3((1u << 23) / 256), dim3(256), 0, stream, what, exp_lo, exp_hi, result, result_cap);
    return hipGetLastError();
}

hipError_t launch_eval_math(int what, const float *xs, const float *ys, uint32_t n, float *out, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(eval_math_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, what, xs, ys, n, out);
    return hipGetLastError();
}

} // namespace clsimhip
