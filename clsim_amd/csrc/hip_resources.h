// The one place host code checks a HIP call and owns a HIP object: hip_check, DeviceGuard, and move-only owners of a device
// allocation, a page-locked host allocation, a stream and an event.  Every owner's destructor ignores what HIP returns
// (teardown has nobody to tell); whoever destroys one from a thread that is not the device's own holds a DeviceGuard.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>

#include "host_model.h"

namespace clsimhip {

inline void hip_check(hipError_t e, const char *what)
{
    if (e != hipSuccess) throw Error(CLSIMHIP_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

// hipSetDevice for the duration of a call made on the CALLER's thread; the caller's current device is restored
struct DeviceGuard {
    explicit DeviceGuard(int device)
    {
        if (hipGetDevice(&previous_) != hipSuccess) previous_ = -1;
        hip_check(hipSetDevice(device), "hipSetDevice");
    }
    // for destructors: a device that cannot be selected is not reported
    DeviceGuard(int device, std::nothrow_t) noexcept
    {
        if (hipGetDevice(&previous_) != hipSuccess) previous_ = -1;
        (void)hipSetDevice(device);
    }
    ~DeviceGuard() { if (previous_ >= 0) (void)hipSetDevice(previous_); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
private:
    int previous_ = -1;
};

// `count` records of device memory, at least 16 bytes (an empty table still has an address the kernels may be given)
template <class T>
class DeviceBuffer {
public:
    DeviceBuffer() = default;
    DeviceBuffer(size_t count, const char *what) { alloc(count, what); }
    explicit DeviceBuffer(T *adopted) : p_(adopted) {}
    DeviceBuffer(DeviceBuffer &&o) noexcept : p_(o.release()) {}
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept { if (this != &o) reset(o.release()); return *this; }
    ~DeviceBuffer() { reset(); }
    void alloc(size_t count, const char *what)
    {
        reset();
        void *p = nullptr;
        hip_check(hipMalloc(&p, std::max<size_t>(count * sizeof(T), 16)), what);
        p_ = static_cast<T *>(p);
    }
    T *get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
    T *release() { T *p = p_; p_ = nullptr; return p; }
    void reset(T *p = nullptr) { if (p_) (void)hipFree(p_); p_ = p; }
private:
    T *p_ = nullptr;
};

// `count` records of page-locked host memory
template <class T>
class PinnedBuffer {
public:
    PinnedBuffer() = default;
    PinnedBuffer(size_t count, const char *what) { alloc(count, what); }
    PinnedBuffer(PinnedBuffer &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    PinnedBuffer &operator=(PinnedBuffer &&o) noexcept { if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; } return *this; }
    ~PinnedBuffer() { reset(); }
    void alloc(size_t count, const char *what) { hip_check(allocate(count), what); }
    // false when the host will not page-lock that much (a buffer pool then does without)
    bool try_alloc(size_t count) noexcept
    {
        if (allocate(count) == hipSuccess) return true;
        (void)hipGetLastError();
        return false;
    }
    T *get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
    void reset() { if (p_) (void)hipHostFree(p_); p_ = nullptr; }
private:
    hipError_t allocate(size_t count)
    {
        reset();
        void *p = nullptr;
        const hipError_t e = hipHostMalloc(&p, count * sizeof(T), hipHostMallocDefault);
        if (e == hipSuccess) p_ = static_cast<T *>(p);
        return e;
    }
    T *p_ = nullptr;
};

// a non-blocking stream
class Stream {
public:
    Stream() = default;
    Stream(Stream &&o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    Stream &operator=(Stream &&o) noexcept { if (this != &o) { reset(); s_ = o.s_; o.s_ = nullptr; } return *this; }
    ~Stream() { reset(); }
    void create(const char *what) { reset(); hip_check(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking), what); }
    void create_with_priority(int priority, const char *what) { reset(); hip_check(hipStreamCreateWithPriority(&s_, hipStreamNonBlocking, priority), what); }
    hipStream_t get() const { return s_; }
    explicit operator bool() const { return s_ != nullptr; }
    void reset() { if (s_) (void)hipStreamDestroy(s_); s_ = nullptr; }
private:
    hipStream_t s_ = nullptr;
};

// an event: one that takes times (create) or one that only orders (create_untimed: hipEventDisableTiming)
class Event {
public:
    Event() = default;
    Event(Event &&o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    Event &operator=(Event &&o) noexcept { if (this != &o) { reset(); e_ = o.e_; o.e_ = nullptr; } return *this; }
    ~Event() { reset(); }
    void create(const char *what) { reset(); hip_check(hipEventCreate(&e_), what); }
    void create_untimed(const char *what) { reset(); hip_check(hipEventCreateWithFlags(&e_, hipEventDisableTiming), what); }
    hipEvent_t get() const { return e_; }
    void reset() { if (e_) (void)hipEventDestroy(e_); e_ = nullptr; }
private:
    hipEvent_t e_ = nullptr;
};

} // namespace clsimhip
