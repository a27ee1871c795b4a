// same_hipmem.h -- move-only owners of the HIP resources the batch host holds (same_batch.cpp): a device buffer, a pinned
// host buffer (plain, mapped with its device view, mapped and coherent) and an event.  They wrap the runtime's handles so
// that "freed exactly once" is a property of the type; there is no pool, no cache and no allocator behind them.
//
// A buffer only grows: ensure(n) keeps an allocation of at least n elements and otherwise frees it and allocates exactly n
// (nothing is copied over; a site with a growth rule of its own passes the padded size).  After a failed allocation the
// owner is empty: null pointer, size zero.  The owner of a void buffer counts bytes.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace same {

namespace detail {
template <typename T> struct ElemBytes { static constexpr size_t value = sizeof(T); };
template <> struct ElemBytes<void> { static constexpr size_t value = 1; };

struct DeviceMemory {
    static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t release(void *p) { return hipFree(p); }
};
template <unsigned Flags>
struct PinnedMemory {
    static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, Flags); }
    static hipError_t release(void *p) { return hipHostFree(p); }
};

template <typename T, typename Memory>
class Buffer {
public:
    Buffer() = default;
    Buffer(const Buffer &) = delete;
    Buffer &operator=(const Buffer &) = delete;
    Buffer(Buffer &&o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    Buffer &operator=(Buffer &&o) noexcept
    {
        if (this != &o) { (void)reset(); p_ = std::exchange(o.p_, nullptr); n_ = std::exchange(o.n_, 0); }
        return *this;
    }
    ~Buffer() { (void)reset(); }

    T *get() const { return p_; }
    operator T *() const { return p_; }
    T *operator->() const { return p_; }
    size_t size() const { return n_; }      // elements allocated (bytes of a void buffer)

    hipError_t reset()
    {
        T *p = std::exchange(p_, nullptr);
        n_ = 0;
        return p ? Memory::release(p) : hipSuccess;
    }
    hipError_t ensure(size_t n)
    {
        if (n <= n_) return hipSuccess;
        hipError_t e = reset();
        if (e != hipSuccess) return e;
        void *p = nullptr;
        e = Memory::alloc(&p, n * ElemBytes<T>::value);
        if (e != hipSuccess) return e;
        p_ = static_cast<T *>(p);
        n_ = n;
        return hipSuccess;
    }

private:
    T *p_ = nullptr;
    size_t n_ = 0;
};
}  // namespace detail

template <typename T> using DevBuf = detail::Buffer<T, detail::DeviceMemory>;
template <typename T> using PinnedBuf = detail::Buffer<T, detail::PinnedMemory<hipHostMallocDefault>>;

// pinned host memory the device reads or writes in place: dev() is its address on the device
template <typename T, unsigned Flags = hipHostMallocMapped>
class MappedBuf {
public:
    T *get() const { return host_.get(); }
    operator T *() const { return host_.get(); }
    T *operator->() const { return host_.get(); }
    T *dev() const { return dev_; }
    size_t size() const { return host_.size(); }
    hipError_t reset() { dev_ = nullptr; return host_.reset(); }
    hipError_t ensure(size_t n)
    {
        if (n <= host_.size()) return hipSuccess;
        dev_ = nullptr;
        hipError_t e = host_.ensure(n);
        if (e == hipSuccess) e = hipHostGetDevicePointer((void **)&dev_, host_.get(), 0);
        return e;
    }

private:
    detail::Buffer<T, detail::PinnedMemory<Flags>> host_;
    T *dev_ = nullptr;
};
template <typename T> using CoherentBuf = MappedBuf<T, hipHostMallocMapped | hipHostMallocCoherent>;

class Event {
public:
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    Event(Event &&o) noexcept : ev_(std::exchange(o.ev_, nullptr)) {}
    Event &operator=(Event &&o) noexcept
    {
        if (this != &o) { (void)reset(); ev_ = std::exchange(o.ev_, nullptr); }
        return *this;
    }
    ~Event() { (void)reset(); }

    operator hipEvent_t() const { return ev_; }
    // makes the event unless there is one already (the flags of the first call hold)
    hipError_t ensure(unsigned flags = hipEventDisableTiming) { return ev_ ? hipSuccess : hipEventCreateWithFlags(&ev_, flags); }
    hipError_t reset()
    {
        hipEvent_t ev = std::exchange(ev_, nullptr);
        return ev ? hipEventDestroy(ev) : hipSuccess;
    }

private:
    hipEvent_t ev_ = nullptr;
};

}  // namespace same
