// dev_buffer.hpp -- DevBuf<T>: the one owner of a device allocation in the host layer.
//
// A DevBuf is empty, OWNS one hipMalloc block (freed by reset(), by the next alloc() and by the destructor) or BORROWS a pointer somebody else
// owns (never freed).  It converts to T *, so launches and pointer arithmetic read as they do on a raw pointer.  Freeing is hipFree: it waits
// for the device, which is what makes growing a buffer between launches safe.  Nothing here is thread-safe but the byte count.
// Only <hip/hip_runtime_api.h>: a plain host compiler builds this (tests/host/dev_buffer_check.cpp does, against a fake runtime).
#pragma once

#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace bitnet_host {

// bytes every live DevBuf of the process owns (bitnet_host_device_bytes)
inline std::atomic<uint64_t> dev_bytes_live{0};

// The untyped part: what a table of differently typed buffers can hold a pointer to.
class DevMem {
  public:
    DevMem() = default;
    DevMem(DevMem &&o) noexcept : p_(o.p_), owned_(o.owned_) { o.p_ = nullptr, o.owned_ = 0; }
    DevMem &operator=(DevMem &&o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_, owned_ = o.owned_;
            o.p_ = nullptr, o.owned_ = 0;
        }
        return *this;
    }
    DevMem(const DevMem &) = delete;
    DevMem &operator=(const DevMem &) = delete;
    ~DevMem() { reset(); }

    // Releases what it holds, then allocates `bytes` (at least 1).  On failure it holds nothing.
    hipError_t alloc_bytes(size_t bytes) {
        reset();
        void *p = nullptr;
        const size_t n = bytes ? bytes : 1;
        if (hipError_t e = hipMalloc(&p, n)) return e;
        p_ = p, owned_ = n;
        dev_bytes_live += n;
        return hipSuccess;
    }
    // ... and fills the `bytes` with zeros (synchronous, as hipMemset is)
    hipError_t alloc_zeroed_bytes(size_t bytes) {
        if (hipError_t e = alloc_bytes(bytes)) return e;
        return hipMemset(p_, 0, bytes);
    }
    void reset() {
        if (owned_) {
            (void)hipFree(p_);
            dev_bytes_live -= owned_;
        }
        p_ = nullptr, owned_ = 0;
    }

  protected:
    void *p_ = nullptr;
    size_t owned_ = 0;  // bytes of the block it owns; 0: empty, or a borrowed pointer
};

template <class T>
class DevBuf : public DevMem {
    static constexpr size_t elem() {
        if constexpr (std::is_void_v<T>) return 1;
        else return sizeof(T);
    }

  public:
    T *get() const { return static_cast<T *>(p_); }
    operator T *() const { return get(); }
    hipError_t alloc(size_t count) { return alloc_bytes(count * elem()); }                // `count` elements (bytes for DevBuf<void>)
    hipError_t alloc_zeroed(size_t count) { return alloc_zeroed_bytes(count * elem()); }
    // A view of memory somebody else owns and outlives this: never freed here.  May be pointed elsewhere at any time.
    void borrow(T *p) {
        reset();
        p_ = p;
    }
};

// Frees a group as a whole BEFORE any member is allocated again: a growing group then peaks at max(old, new) bytes, not old + new.
template <class... B>
void release_all(B &...b) {
    (b.reset(), ...);
}

}  // namespace bitnet_host
