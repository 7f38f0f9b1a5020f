// Event statistics: per particle, the photons generated and the photons at DOMs as counts and exact weight sums (include/clsimhip.h:
// "Event statistics").  The definition lives here ONCE, as functions both the host twin (event_stats.cpp) and the HIP kernels
// (event_stats_kernel.hip) compile: integer arithmetic only, no floating-point operation, so x86-64 and gfx950 cannot disagree.  It
// stands where the reference has
//   I3CLSimClientModule::DigestOtherFrame / the step loop   private/clsim/I3CLSimClientModule.cxx:513-520  (generated: count and weight)
//   I3CLSimClientModule::AddPhotonsToFrames                 :386-405  (particle lookup :388-390, ignoreModules :399, at DOMs: count and weight)
//   I3CLSimEventStatistics into the frame                   :728-740
// A term is sign, a magnitude M < 2^56 and a shift s <= 253: M * 2^s in units of 2^-149.  It touches at most three of the 32-bit limb
// positions 0 ... 9: with p = s / 32 and b = s % 32, the limbs of M << b at p, p + 1, p + 2.
//
// Accumulators are DEFERRED-CARRY LIMBS: per record, side (generated, at DOMs) and sign twelve uint64 slots, one per limb position,
// each the plain sum of the 32-bit limbs that fell on it.  A bunch has at most 2^32 - 1 records, so a slot stays below
// (2^32 - 1)^2 < 2^64: adding never carries, and integer addition commutes -- the order of the additions cannot matter.  Closing a
// record propagates the carries once, subtracts the negative accumulator from the positive one and packs six words.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/clsimhip.h"
#include "host_model.h"
#include "mcpe_series.h"

namespace clsimhip {

enum EventStatsKind : uint32_t { ES_FINITE = 0, ES_PLUS_INF = 1, ES_MINUS_INF = 2, ES_NAN = 3 };
enum EventStatsSide : uint32_t { ES_GENERATED = 0, ES_AT_DOMS = 1 };

struct EventStatsTerm {
    uint32_t kind;          // EventStatsKind; the rest holds for ES_FINITE
    uint32_t negative;      // 0 / 1
    uint32_t position;      // of limb[0]: 0 ... 7
    uint32_t limb[3];
};

// THE decomposition: the exact product count x w of a float weight's bit pattern (the at-DOM term has count = 1, generated = false;
// the generated term count = num_photons, generated = true, where a non-finite weight times 0 is a NaN term)
SERIES_HD void event_stats_term(uint32_t weight_bits, uint32_t count, bool generated, EventStatsTerm &t)
{
    const uint32_t e = (weight_bits >> 23) & 255u, f = weight_bits & 0x7fffffu;
    t.negative = weight_bits >> 31;
    t.position = 0u;
    t.limb[0] = 0u; t.limb[1] = 0u; t.limb[2] = 0u;
    if (e == 255u) {
        t.kind = (f != 0u || (generated && count == 0u)) ? ES_NAN : (t.negative ? ES_MINUS_INF : ES_PLUS_INF);
        return;
    }
    t.kind = ES_FINITE;
    const uint32_t m = e ? (f | 0x800000u) : f;                 // < 2^24
    const uint32_t s = (e ? e : 1u) - 1u;                       // 0 ... 253
    const uint64_t M = (uint64_t)count * m;                     // < 2^56
    const uint32_t b = s & 31u;
    t.position = s >> 5;
    t.limb[0] = (uint32_t)(M << b);
    t.limb[1] = (uint32_t)(b ? M >> (32u - b) : M >> 32);       // bits 32 ... 63 of M << b
    t.limb[2] = b ? (uint32_t)(M >> (64u - b)) : 0u;            // bits 64 ... 95
}

// ---- the accumulators of one record: kEventStatsSlots uint64 ----
constexpr uint32_t kEventStatsLimbs = 12u;
// [side][sign][limb position], then the two counts, then [side][+inf, -inf, NaN]
constexpr uint32_t kEventStatsCounts = 4u * kEventStatsLimbs, kEventStatsSpecial = kEventStatsCounts + 2u, kEventStatsSlots = kEventStatsSpecial + 6u;
SERIES_HD uint32_t event_stats_limb_slot(uint32_t side, uint32_t negative, uint32_t position) { return (side * 2u + negative) * kEventStatsLimbs + position; }

// positive - negative accumulator of one side, carries propagated: six words, two's complement
SERIES_HD void event_stats_close_side(const uint64_t *positive, const uint64_t *negative, uint64_t words[6])
{
    uint64_t carry_p = 0u, carry_n = 0u, borrow = 0u;
#pragma unroll
    for (uint32_t w = 0; w < 6u; ++w) {
        uint64_t word = 0u;
#pragma unroll
        for (uint32_t h = 0; h < 2u; ++h) {
            const uint32_t i = 2u * w + h;
            const uint64_t p = positive[i] + carry_p, n = negative[i] + carry_n;    // slot <= (2^32 - 1)^2, carry < 2^32: no overflow
            carry_p = p >> 32; carry_n = n >> 32;
            const uint64_t d = (p & 0xffffffffu) - (n & 0xffffffffu) - borrow;      // modulo 2^64; bit 32 up is set iff it went below zero
            borrow = (d >> 32) & 1u;
            word |= (d & 0xffffffffu) << (32u * h);
        }
        words[w] = word;
    }
}

// one record from its accumulators
SERIES_HD void event_stats_close(const uint64_t *slots, uint32_t identifier, uint32_t frame, clsimhip_event_statistics &r)
{
    r.identifier = identifier;
    r.frame = frame;
    r.generated_count = slots[kEventStatsCounts + ES_GENERATED];
    r.at_doms_count = slots[kEventStatsCounts + ES_AT_DOMS];
    event_stats_close_side(slots + event_stats_limb_slot(ES_GENERATED, 0u, 0u), slots + event_stats_limb_slot(ES_GENERATED, 1u, 0u), r.generated_sum);
    event_stats_close_side(slots + event_stats_limb_slot(ES_AT_DOMS, 0u, 0u), slots + event_stats_limb_slot(ES_AT_DOMS, 1u, 0u), r.at_doms_sum);
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k) {
        r.generated_special[k] = (uint32_t)slots[kEventStatsSpecial + k];          // (at most 2^32 - 1 records)
        r.at_doms_special[k] = (uint32_t)slots[kEventStatsSpecial + 3u + k];
    }
}

// ADD, acc += rec (include/clsimhip.h: clsimhip_event_statistics_add): the words of both sums with carry, modulo 2^384, both counts modulo
// 2^64, the six special counters modulo 2^32; acc's identifier and frame stay.  Associative and commutative: what the event statistics
// store (event_stats_store.h) rests on.
SERIES_HD void event_stats_add_words(uint64_t *a, const uint64_t *b)
{
    uint64_t carry = 0u;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const uint64_t s = a[k] + b[k];
        const uint64_t c = s < a[k] ? 1u : 0u;
        a[k] = s + carry;
        carry = c | (a[k] < s ? 1u : 0u);
    }
}
SERIES_HD void event_stats_add(clsimhip_event_statistics &acc, const clsimhip_event_statistics &rec)
{
    event_stats_add_words(acc.generated_sum, rec.generated_sum);
    event_stats_add_words(acc.at_doms_sum, rec.at_doms_sum);
    acc.generated_count += rec.generated_count;
    acc.at_doms_count += rec.at_doms_count;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        acc.generated_special[k] += rec.generated_special[k];
        acc.at_doms_special[k] += rec.at_doms_special[k];
    }
}

// the mask: keys frame rank << 32 | record word (string ID | OM ID << 16), ascending and distinct
SERIES_HD bool event_stats_is_masked(const uint64_t *keys, uint32_t n, uint64_t key)
{
    uint32_t lo = 0u, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (keys[mid] < key) lo = mid + 1u; else hi = mid;
    }
    return lo < n && keys[lo] == key;
}

// ---- the device stage (event_stats_kernel.hip) ----
// header words (uint32) at the start of the workspace, beside CLSIMHIP_EVENT_STATISTICS_* at 0 ... 2
constexpr uint32_t kEventStatsHeaderWords = 16u;

struct EventStatsDeviceArgs {
    const SeriesParticle *particles;        // device memory; null: no table -- every identifier is record 0
    const uint32_t *frames;                 // frame ID by frame rank
    const uint64_t *masked;                 // ascending, distinct
    uint32_t n_particles, n_masked, consecutive, records;      // records: n_particles, or 1 without a table
    const clsimhip_step *steps;             // 4-byte aligned
    uint32_t n_steps;
    const clsimhip_photon *photons;         // 4-byte aligned
    const uint32_t *photon_count;           // records = min(*photon_count, capacity)
    uint32_t capacity;
    uint32_t *header;                       // kEventStatsHeaderWords, zeroed with the accumulators by every call
    uint64_t *slots;                        // records x kEventStatsSlots
    clsimhip_event_statistics *out;         // records
    uint32_t *counters;                     // four: the three counters, the records written
};

// all kernels of the stage, asynchronous on `stream`
hipError_t launch_event_stats(const EventStatsDeviceArgs &A, hipStream_t stream);

// ---- the host side (event_stats.cpp) ----
size_t event_stats_blob_bytes(size_t n_particles, size_t n_masked);
size_t event_stats_workspace_bytes(size_t n_particles, size_t n_masked);

// One bunch's particle table and mask, checked and brought into the form the stage reads (event_stats_blob_bytes(n_particles,
// n_masked) bytes at `blob`, 16-byte aligned): the series stages' table and frame IDs by rank (series_bunch.h), then the masked
// keys as uint64 at masked_offset, n_masked of them
SeriesBunch event_stats_prepare(const clsimhip_mcpe_particle *particles, size_t n_particles, const clsimhip_mcpe_mask *masked, size_t n_masked, uint8_t *blob);

// the host twin
void event_stats_host(const clsimhip_step *steps, size_t n_steps, const clsimhip_photon *photons, size_t n_photons, const clsimhip_mcpe_particle *particles,
                      size_t n_particles, const clsimhip_mcpe_mask *masked, size_t n_masked, clsimhip_event_statistics *out, uint64_t counters[3]);
// the kernels; the table and the mask are prepared in a page-locked buffer of the process' (one call at a time)
void event_stats_device(int device, const void *d_steps, size_t n_steps, const void *d_photons, const void *d_count, size_t capacity,
                        const clsimhip_mcpe_particle *particles, size_t n_particles, const clsimhip_mcpe_mask *masked, size_t n_masked, void *d_out, void *d_counters,
                        void *d_workspace, size_t workspace_bytes, hipStream_t stream);
// the same with a bunch prepared earlier; h_blob must stay as it is until the copy queued on `stream` is over (`uploaded`, if given,
// is recorded right behind it)
void event_stats_device_prepared(int device, const void *d_steps, size_t n_steps, const void *d_photons, const void *d_count, size_t capacity, const SeriesBunch &bunch,
                                 const uint8_t *h_blob, void *d_out, void *d_counters, void *d_workspace, size_t workspace_bytes, hipStream_t stream,
                                 hipEvent_t uploaded = nullptr);
// the helper of the C ABI that is host only (event_stats_add is above)
double event_stats_weight(const uint64_t words[6], const uint32_t special[3]);

} // namespace clsimhip
