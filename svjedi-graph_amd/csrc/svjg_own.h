// Owners of what a context allocates: a device buffer, a pinned host buffer, an event, a stream.  Host code only.  Each is non-copyable and
// movable, empty until asked, and gives back what it holds in its destructor; none knows svjg_ctx: a call returns a hipError_t and the caller
// reports it (HIPCHK).  tests/own_sim compiles this header against malloc-backed stand-ins of the HIP calls below, under ASan and UBSan.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace svjg {

// device memory: pointer and capacity in elements
template <class T>
struct DevBuf {
    T *p = nullptr;  uint64_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;  DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    ~DevBuf() { release(); }
    operator T *() const { return p; }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }

    // Room for `want` elements; with room already, a compare and a return.  keep: the contents move to the new block, copied on `copy_on`.
    // quiesce() -> hipError_t: the caller's wait for everything enqueued that still uses the old block (the copy included); only then is the old
    // block freed.  On any failure the old block and its capacity stand as they were and nothing new stays allocated.
    template <class Quiesce>
    hipError_t reserve(uint64_t want, bool keep, hipStream_t copy_on, Quiesce quiesce) {
        if (want <= cap) return hipSuccess;
        // a buffer that keeps its contents grows by at least half: the hit records of a file classified in pieces used to be moved into a
        // buffer a piece larger 2 x 169 times at configs[3] (hipMalloc / copy / hipFree of up to 5.7 GB each: 7 of the 8.9 s of its ingest)
        const uint64_t asked = want;
        if (keep && cap && want < cap + cap / 2) want = cap + cap / 2;
        void *q = nullptr;
        if (want != asked && hipMalloc(&q, want * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); q = nullptr; want = asked; }   // (no room for the margin: what was asked for)
        hipError_t e = q ? hipSuccess : hipMalloc(&q, want * sizeof(T));
        if (e != hipSuccess) return e;
        if (keep && p && cap) e = hipMemcpyAsync(q, p, cap * sizeof(T), hipMemcpyDeviceToDevice, copy_on);
        if (e == hipSuccess) e = quiesce();
        if (e != hipSuccess) { (void)hipFree(q); return e; }      // (hipFree waits for the device: a copy under way does not outlive its target)
        if (p) (void)hipFree(p);
        p = (T *)q; cap = want;
        return hipSuccess;
    }
    // the same for a buffer nothing enqueued uses (empty, or the caller has waited): contents not kept
    hipError_t reserve(uint64_t want) { return reserve(want, false, nullptr, [] { return hipSuccess; }); }
};

// pinned host memory: pointer and capacity in bytes; growing drops the contents
struct PinBuf {
    uint8_t *p = nullptr;  uint64_t cap = 0;
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;  PinBuf &operator=(const PinBuf &) = delete;
    PinBuf(PinBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    PinBuf &operator=(PinBuf &&o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    ~PinBuf() { release(); }
    operator uint8_t *() const { return p; }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
    hipError_t reserve(uint64_t want, unsigned int flags) {
        if (want <= cap) return hipSuccess;
        release();
        void *q = nullptr;
        const hipError_t e = hipHostMalloc(&q, want, flags);
        if (e != hipSuccess) return e;
        p = (uint8_t *)q; cap = want;
        return hipSuccess;
    }
};

// create(): nothing when the handle is there already
struct Event {
    hipEvent_t h = nullptr;
    Event() = default;
    Event(const Event &) = delete;  Event &operator=(const Event &) = delete;
    Event(Event &&o) noexcept : h(o.h) { o.h = nullptr; }
    Event &operator=(Event &&o) noexcept { if (this != &o) { release(); h = o.h; o.h = nullptr; } return *this; }
    ~Event() { release(); }
    operator hipEvent_t() const { return h; }
    void release() { if (h) (void)hipEventDestroy(h); h = nullptr; }
    hipError_t create(unsigned int flags = hipEventDefault) { return h ? hipSuccess : hipEventCreateWithFlags(&h, flags); }
};

// priority 0 is the default one: create() makes what hipStreamCreate does, create(flags) what hipStreamCreateWithFlags does
struct Stream {
    hipStream_t h = nullptr;
    Stream() = default;
    Stream(const Stream &) = delete;  Stream &operator=(const Stream &) = delete;
    Stream(Stream &&o) noexcept : h(o.h) { o.h = nullptr; }
    Stream &operator=(Stream &&o) noexcept { if (this != &o) { release(); h = o.h; o.h = nullptr; } return *this; }
    ~Stream() { release(); }
    operator hipStream_t() const { return h; }
    void release() { if (h) (void)hipStreamDestroy(h); h = nullptr; }
    hipError_t create(unsigned int flags = hipStreamDefault, int priority = 0) { return h ? hipSuccess : hipStreamCreateWithPriority(&h, flags, priority); }
};

}  // namespace svjg
