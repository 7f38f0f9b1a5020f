// Cable shadow: a detected photon whose last path crosses a cable is dropped (include/clsimhip.h: "Cable shadow").  The definition
// lives here ONCE, as functions both the host twin (cable_shadow.cpp) and the HIP kernels (cable_shadow_kernel.hip) compile:
// binary64 + - * / in the order written, no contraction (-ffp-contract=off, Makefile), no sqrt, no fma; the two angles go through
// mcpe_sincos (mcpe.h), the deterministic single-precision library, and the results are widened.  It decides booleans only, so NaN
// payloads cannot matter, and x86-64 and gfx950 agree.  It stands where the reference has
//   I3ShadowedPhotonRemoverModule                  private/clsim/shadow/I3ShadowedPhotonRemoverModule.cxx  (PropagatedPhotons ->
//                                                   PropagatedPhotonsWithShadow, which the photon-to-MCPE converter then reads)
//   I3ShadowedPhotonRemover::IsPhotonShadowed      private/clsim/shadow/I3ShadowedPhotonRemover.cxx:63-81  (every photon against
//                                                   the whole I3CylinderMap, on one host thread)
//   the cable map                                  python/shadow/AddCylinder.py:38-65  (one cylinder per DOM)
// Two things there cannot be restated and are this project's own.  The cylinder test it calls, I3ExtraGeometryItemCylinder::
// DoesLineIntersect, lies outside the reference: the rule below is "the segment meets the solid finite cylinder".  And its start
// point has a slip: dy is computed with cos(azimuth) (:68, beside the class comment "This code is NOT functional at the moment");
// here the y component is the corrected one, sin(theta) sin(phi).
//
// Per record, with `distance` D (finite, >= 0):
//     P1 = ((double)x, (double)y, (double)z)
//     (st, ct) = mcpe_sincos(theta);  (sp, cp) = mcpe_sincos(phi)
//     dir = ((double)st*(double)cp, (double)st*(double)sp, (double)ct);  d = D*dir;  P0 = P1 - d
// P0 is the point D back along the arrival direction (the reference's zenith and azimuth are those of -dir).  Per cylinder, once on
// the host: A = bottom, a = top - bottom, L2 = a.a, r2 = r*r.  Then with m = P0 - A and every dot product x*x' + y*y' + z*z' from
// left to right: cable_hit below.  The radial condition is a convex quadratic in t; its minimum over the slab interval clipped to
// [0, 1] sits at the clamped vertex.  A record is shadowed iff some cylinder hits: the set's order cannot matter.
//   * a NaN in position or angles is never shadowed, because every comparison is false;
//   * D = 0 is a point-in-cylinder test;
//   * the position is used as stored: with oversized DOMs it lies on the oversized sphere, and what that means is the caller's
//     business.
#pragma once
#include <map>
#include <mutex>
#include <vector>

#include "mcpe.h"
#include "mcpe_series.h"

namespace clsimhip {

constexpr size_t kCableShadowMaxCylinders = 16384;     // bounds the work of a launch at capacity x 16 384 tests
constexpr uint32_t kCableShadowTile = kSeriesTile;     // records per kept-count and per workgroup of the compact kernel

// one cylinder as twin and kernel read it: 64 bytes
struct alignas(16) CableCylinder { double A[3], a[3], L2, r2; };
static_assert(sizeof(CableCylinder) == 64, "the cylinder record is 64 bytes");

// a record's segment: P0, d and d.d (which no cylinder changes)
struct CableSegment { double P0[3], d[3], dd; };

MCPE_HD void cable_segment(float x, float y, float z, float theta, float phi, double D, CableSegment &s)
{
    float st, ct, sp, cp;
    mcpe_sincos(theta, st, ct);
    mcpe_sincos(phi, sp, cp);
    const double dirx = (double)st * (double)cp, diry = (double)st * (double)sp, dirz = (double)ct;
    s.d[0] = D * dirx; s.d[1] = D * diry; s.d[2] = D * dirz;
    s.P0[0] = (double)x - s.d[0]; s.P0[1] = (double)y - s.d[1]; s.P0[2] = (double)z - s.d[2];
    s.dd = s.d[0] * s.d[0] + s.d[1] * s.d[1] + s.d[2] * s.d[2];
}

// the segment P0 + t d, 0 <= t <= 1, meets the solid finite cylinder
MCPE_HD bool cable_hit(const CableSegment &s, const CableCylinder &c)
{
    const double mx = s.P0[0] - c.A[0], my = s.P0[1] - c.A[1], mz = s.P0[2] - c.A[2];
    const double ma = mx * c.a[0] + my * c.a[1] + mz * c.a[2];
    const double da = s.d[0] * c.a[0] + s.d[1] * c.a[1] + s.d[2] * c.a[2];
    const double u1 = ma + da;
    const double L2 = c.L2;
    if ((ma < 0. && u1 < 0.) || (ma > L2 && u1 > L2)) return false;     // both ends beyond the same cap
    double lo = 0., hi = 1.;
    if (da != 0.) {
        double ta = (0. - ma) / da, tb = (L2 - ma) / da;
        if (ta > tb) { const double swap = ta; ta = tb; tb = swap; }
        if (ta > lo) lo = ta;
        if (tb < hi) hi = tb;
        if (lo > hi) return false;
    } else if (!(ma >= 0. && ma <= L2)) {
        return false;
    }
    const double mm = mx * mx + my * my + mz * mz;
    const double md = mx * s.d[0] + my * s.d[1] + mz * s.d[2];
    const double al = s.dd * L2 - da * da, be = md * L2 - ma * da, ga = (mm - c.r2) * L2 - ma * ma;
    double t = lo;
    if (al > 0.) {
        t = (0. - be) / al;
        if (t < lo) t = lo;
        if (t > hi) t = hi;
    }
    return (al * t + (be + be)) * t + ga <= 0.;
}

// ---- the device stage (cable_shadow_kernel.hip) ----
struct CableShadowDeviceArgs {
    const CableCylinder *cylinders;         // device memory, 64-byte records
    uint32_t n_cylinders;
    double distance;
    const clsimhip_photon *in;              // 16-byte aligned
    const uint32_t *in_count;               // records = min(*in_count, capacity)
    uint32_t capacity;
    uint32_t *header;                       // kSeriesHeaderWords: [SH_KEPT] the records tested, [SH_SERIES] the lit ones
    uint32_t *tile_counts;                  // tiles(capacity): lit records per tile, then their exclusive scan
    uint8_t *flags;                         // capacity bytes: 1 = shadowed
    clsimhip_photon *lit;                   // capacity records, 16-byte aligned
    uint32_t *counts;                       // three: lit, tested, shadowed
};

// all kernels of the stage, asynchronous on `stream`
hipError_t launch_cable_shadow(const CableShadowDeviceArgs &A, hipStream_t stream);

// ---- the host side (cable_shadow.cpp) ----
size_t cable_shadow_workspace_bytes(size_t capacity);

// The cylinder set: the precomputed records, the host twin, and the table on every device it has been used on
class CableShadow {
public:
    // top, bottom: 3 doubles per cylinder; radius: one
    CableShadow(size_t n, const double *top, const double *bottom, const double *radius, double distance);
    ~CableShadow();
    CableShadow(const CableShadow &) = delete;
    CableShadow &operator=(const CableShadow &) = delete;
    size_t num_cylinders() const { return cylinders_.size(); }
    double distance() const { return distance_; }
    // the host twin: flags[n] (1 = shadowed), the lit records in input order (lit holds n), counts = {tested, shadowed}
    void host(const clsimhip_photon *in, size_t n, uint8_t *flags, clsimhip_photon *lit, size_t *n_lit, uint64_t counts[2]) const;
    // the kernels on `stream` of `device`, over min(*d_count, capacity) records: d_flags capacity bytes, d_lit capacity records,
    // d_counts three uint32 (lit, tested, shadowed)
    void device(int device, const void *d_photons, const void *d_count, size_t capacity, void *d_flags, void *d_lit, void *d_counts, void *d_workspace,
                size_t workspace_bytes, hipStream_t stream);

private:
    const CableCylinder *image_on(int device);
    std::vector<CableCylinder> cylinders_;
    double distance_ = 0.;
    std::mutex device_mutex_;
    std::map<int, CableCylinder *> images_;
};

} // namespace clsimhip
