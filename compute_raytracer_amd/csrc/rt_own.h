// rt_own.h -- owners of what a context takes from the HIP runtime: device memory, pinned host memory, events, streams.
// Host-only, nothing of the project.  Whoever declares one of these owns it: the destructor releases, so no list of members
// has to be kept anywhere else (rt_destroy names no resource).  All four are move-only; none is exported from the library.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>

#pragma GCC visibility push(hidden)

struct RtDeviceMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t release(void* p) { return hipFree(p); }
};
struct RtPinnedMem {     // device-visible host memory
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static hipError_t release(void* p) { return hipHostFree(p); }
};

// An allocation: `cap` bytes at `p`, of which the first `used` hold what was written (the user's bookkeeping).
// Rounding, minimum sizes and zero-filling are the caller's: replace() allocates exactly what it is asked for.
template <class MEM> struct RtBuf {
    void* p = nullptr;
    size_t cap = 0;
    size_t used = 0;

    RtBuf() = default;
    RtBuf(const RtBuf&) = delete;
    RtBuf& operator=(const RtBuf&) = delete;
    RtBuf(RtBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)), used(std::exchange(o.used, 0)) {}
    RtBuf& operator=(RtBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p = std::exchange(o.p, nullptr); cap = std::exchange(o.cap, 0); used = std::exchange(o.used, 0);
        }
        return *this;
    }
    ~RtBuf() { reset(); }

    void reset() {
        if (p) (void)MEM::release(p);
        p = nullptr; cap = used = 0;
    }
    // frees, then allocates exactly `bytes`; on failure the buffer stays empty
    hipError_t replace(size_t bytes) {
        reset();
        const hipError_t e = MEM::alloc(&p, bytes);
        if (e != hipSuccess) p = nullptr;
        else cap = bytes;
        return e;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
};
using DevBuf = RtBuf<RtDeviceMem>;
using PinnedBuf = RtBuf<RtPinnedMem>;

// One event or stream.  ensure() creates it at its first call and does nothing afterwards; converts to the raw handle
// (nullptr: not made), so HIP calls take it as they took the handle.
template <class H, hipError_t (*CREATE)(H*, unsigned), hipError_t (*DESTROY)(H)> struct RtHandle {
    H h = nullptr;

    RtHandle() = default;
    RtHandle(const RtHandle&) = delete;
    RtHandle& operator=(const RtHandle&) = delete;
    RtHandle(RtHandle&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
    RtHandle& operator=(RtHandle&& o) noexcept {
        if (this != &o) { reset(); h = std::exchange(o.h, nullptr); }
        return *this;
    }
    ~RtHandle() { reset(); }

    void reset() {
        if (h) (void)DESTROY(h);
        h = nullptr;
    }
    hipError_t ensure(unsigned flags = 0) {      // 0: hipEventDefault, hipStreamDefault
        if (h) return hipSuccess;
        const hipError_t e = CREATE(&h, flags);
        if (e != hipSuccess) h = nullptr;
        return e;
    }
    operator H() const { return h; }
};
using Event = RtHandle<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;
using Stream = RtHandle<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;

#pragma GCC visibility pop
