// Cable shadow (cable_shadow.h): the cylinder set, the host twin, and the host side of the device stage.  The kernels are in
// cable_shadow_kernel.hip.
#include "cable_shadow.h"

#include <cmath>
#include <cstring>

namespace clsimhip {

namespace {
// the workspace: header and tile counts, zeroed together by every call
struct CableShadowWorkspace {
    size_t tile_counts, bytes;
    explicit CableShadowWorkspace(size_t capacity)
    {
        const size_t tiles = std::max<size_t>((capacity + kCableShadowTile - 1u) / kCableShadowTile, 1u);
        tile_counts = kSeriesHeaderWords * sizeof(uint32_t);
        bytes = round16(tile_counts + tiles * sizeof(uint32_t));
    }
};
} // namespace

size_t cable_shadow_workspace_bytes(size_t capacity) { return CableShadowWorkspace(capacity).bytes; }

CableShadow::CableShadow(size_t n, const double *top, const double *bottom, const double *radius, double distance)
{
    if (n == 0) throw Error(CLSIMHIP_ERR_ARGUMENT, "cable shadow: no cylinder");
    if (n > kCableShadowMaxCylinders) throw Error(CLSIMHIP_ERR_ARGUMENT, "cable shadow: more than 16384 cylinders");
    if (!top || !bottom || !radius) throw Error(CLSIMHIP_ERR_ARGUMENT, "top / bottom / radius is (null)");
    if (!std::isfinite(distance) || distance < 0.) throw Error(CLSIMHIP_ERR_ARGUMENT, "cable shadow: the distance must be finite and not negative");
    distance_ = distance;
    cylinders_.resize(n);
    for (size_t i = 0; i < n; ++i) {
        const std::string which = "cable shadow: cylinder " + std::to_string(i);
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(top[3 * i + k]) || !std::isfinite(bottom[3 * i + k])) throw Error(CLSIMHIP_ERR_ARGUMENT, which + " has a non-finite end point");
        if (!std::isfinite(radius[i]) || !(radius[i] > 0.)) throw Error(CLSIMHIP_ERR_ARGUMENT, which + ": the radius must be finite and positive");
        CableCylinder &c = cylinders_[i];
        for (int k = 0; k < 3; ++k) {
            c.A[k] = bottom[3 * i + k];
            c.a[k] = top[3 * i + k] - bottom[3 * i + k];
        }
        c.L2 = c.a[0] * c.a[0] + c.a[1] * c.a[1] + c.a[2] * c.a[2];
        c.r2 = radius[i] * radius[i];
        if (!std::isfinite(c.L2) || !(c.L2 > 0.)) throw Error(CLSIMHIP_ERR_ARGUMENT, which + " has no length (or one whose square is not finite)");
        if (!std::isfinite(c.r2) || !(c.r2 > 0.)) throw Error(CLSIMHIP_ERR_ARGUMENT, which + ": the radius' square is zero or not finite");
    }
}

CableShadow::~CableShadow()
{
    for (auto &kv : images_) {
        DeviceGuard on_device(kv.first, std::nothrow);
        DeviceBuffer<CableCylinder> table(kv.second);
    }
}

void CableShadow::host(const clsimhip_photon *in, size_t n, uint8_t *flags, clsimhip_photon *lit, size_t *n_lit, uint64_t counts[2]) const
{
    if (n && (!in || !flags || !lit)) throw Error(CLSIMHIP_ERR_ARGUMENT, "photons / flags / lit is (null)");
    if (n > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "more than 2^32 - 1 records");
    size_t kept = 0;
    for (size_t i = 0; i < n; ++i) {
        float g[8];                                                         // (the record is packed: no word of it is read in place)
        std::memcpy(g, in + i, sizeof g);                                   // x y z time, theta phi wavelength cherenkov_dist
        CableSegment s;
        cable_segment(g[0], g[1], g[2], g[4], g[5], distance_, s);
        bool hit = false;
        for (size_t c = 0; c < cylinders_.size() && !hit; ++c) hit = cable_hit(s, cylinders_[c]);
        flags[i] = hit ? 1u : 0u;
        if (!hit) std::memcpy(lit + kept++, in + i, sizeof(clsimhip_photon));
    }
    if (n_lit) *n_lit = kept;
    if (counts) { counts[0] = n; counts[1] = n - kept; }
}

const CableCylinder *CableShadow::image_on(int device)
{
    std::lock_guard<std::mutex> lk(device_mutex_);
    auto it = images_.find(device);
    if (it != images_.end()) return it->second;
    DeviceBuffer<CableCylinder> table(cylinders_.size(), "cable shadow: cylinders");
    hip_check(hipMemcpy(table.get(), cylinders_.data(), cylinders_.size() * sizeof(CableCylinder), hipMemcpyHostToDevice), "cable shadow: cylinders");
    CableCylinder *p = table.release();
    images_[device] = p;
    return p;
}

void CableShadow::device(int device, const void *d_photons, const void *d_count, size_t capacity, void *d_flags, void *d_lit, void *d_counts, void *d_workspace,
                         size_t workspace_bytes, hipStream_t stream)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) throw Error(CLSIMHIP_ERR_DEVICE, "no HIP device available (the cable shadow's device path has no CPU fallback)");
    if (device < 0 || device >= count) throw Error(CLSIMHIP_ERR_ARGUMENT, "device ordinal out of range");
    const CableShadowWorkspace W(capacity);
    const auto off = [](const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) != 0u; };
    if (!d_count || !d_counts || !d_workspace) throw Error(CLSIMHIP_ERR_ARGUMENT, "device pointers are (null)");
    if (capacity && (!d_photons || !d_flags || !d_lit)) throw Error(CLSIMHIP_ERR_ARGUMENT, "d_photons / d_flags / d_lit is (null)");
    if (capacity > 0xffffffffull) throw Error(CLSIMHIP_ERR_ARGUMENT, "capacity beyond 2^32 - 1 records");
    if (off(d_photons, 16u) || off(d_lit, 16u) || off(d_workspace, 16u) || off(d_counts, 4u) || off(d_count, 4u))
        throw Error(CLSIMHIP_ERR_ARGUMENT, "d_photons, d_lit and d_workspace must be aligned to 16 bytes, d_count and d_counts to 4");
    if (workspace_bytes < W.bytes)
        throw Error(CLSIMHIP_ERR_ARGUMENT, "the cable shadow workspace holds " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(W.bytes) + " are needed");
    DeviceGuard on_device(device);
    uint8_t *ws = static_cast<uint8_t *>(d_workspace);
    CableShadowDeviceArgs A{};
    A.cylinders = image_on(device);
    A.n_cylinders = static_cast<uint32_t>(cylinders_.size());
    A.distance = distance_;
    A.in = static_cast<const clsimhip_photon *>(d_photons);
    A.in_count = static_cast<const uint32_t *>(d_count);
    A.capacity = static_cast<uint32_t>(capacity);
    A.header = reinterpret_cast<uint32_t *>(ws);
    A.tile_counts = reinterpret_cast<uint32_t *>(ws + W.tile_counts);
    A.flags = static_cast<uint8_t *>(d_flags);
    A.lit = static_cast<clsimhip_photon *>(d_lit);
    A.counts = static_cast<uint32_t *>(d_counts);
    const hipError_t e = launch_cable_shadow(A, stream);
    if (e != hipSuccess) throw Error(CLSIMHIP_ERR_DEVICE, std::string("cable shadow kernel launch: ") + hipGetErrorString(e));
}

} // namespace clsimhip
