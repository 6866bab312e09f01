// The context's owners (svjedi-graph_amd/csrc/svjg_own.h) against malloc-backed stand-ins of the HIP calls the header makes: a stand-alone program
// for a build under AddressSanitizer / UBSan (no HIP runtime is linked, nothing is preloaded into anything).  The stand-ins count what is alive,
// log what is given back, and fail on request: the n-th allocation from now, the next copy.
#include "../../svjedi-graph_amd/csrc/svjg_own.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <utility>

using namespace svjg;

static long live_dev = 0, live_pin = 0, live_ev = 0, live_st = 0;
static long n_malloc = 0, n_dev_free = 0, n_copy = 0, n_last_error = 0;
static long fail_alloc_in = 0, fail_alloc_n = 1;                   // k > 0: the k-th allocation from now fails, and fail_alloc_n - 1 behind it (device and pinned count alike)
static bool fail_copy = false;
static std::string freed;                                          // one letter per object given back, in order: d, p, e, s
static unsigned last_pin_flags = 0, last_ev_flags = 0, last_st_flags = 0;
static int last_st_priority = 0;

static bool alloc_fails() {
    if (fail_alloc_in > 1) { --fail_alloc_in; return false; }
    if (fail_alloc_in == 1 && fail_alloc_n > 0) { if (--fail_alloc_n == 0) { fail_alloc_in = 0; fail_alloc_n = 1; } return true; }
    return false;
}
static void fail_allocs(long from, long n) { fail_alloc_in = from; fail_alloc_n = n; }
static long live() { return live_dev + live_pin + live_ev + live_st; }

extern "C" {
hipError_t hipMalloc(void **p, size_t n) {
    ++n_malloc;
    if (alloc_fails()) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = malloc(n ? n : 1); ++live_dev;
    return hipSuccess;
}
hipError_t hipFree(void *p) { if (p) { free(p); --live_dev; ++n_dev_free; freed += 'd'; } return hipSuccess; }
hipError_t hipHostMalloc(void **p, size_t n, unsigned int flags) {
    last_pin_flags = flags;
    if (alloc_fails()) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = malloc(n ? n : 1); ++live_pin;
    return hipSuccess;
}
hipError_t hipHostFree(void *p) { if (p) { free(p); --live_pin; freed += 'p'; } return hipSuccess; }
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind, hipStream_t) {
    if (fail_copy) { fail_copy = false; return hipErrorInvalidValue; }
    memcpy(dst, src, n); ++n_copy;
    return hipSuccess;
}
hipError_t hipGetLastError(void) { ++n_last_error; return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags) { *e = (hipEvent_t)malloc(1); last_ev_flags = flags; ++live_ev; return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { free(e); --live_ev; freed += 'e'; return hipSuccess; }
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned int flags, int priority) {
    *s = (hipStream_t)malloc(1); last_st_flags = flags; last_st_priority = priority; ++live_st;
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) { free(s); --live_st; freed += 's'; return hipSuccess; }
}

static int bad = 0, checks = 0;
#define CHECK(x) do { ++checks; if (!(x)) { ++bad; fprintf(stderr, "own_sim.cpp:%d: %s\n", __LINE__, #x); } } while (0)

static long n_quiesce = 0;
static hipError_t idle() { ++n_quiesce; return hipSuccess; }
static hipError_t idle_fails() { ++n_quiesce; return hipErrorUnknown; }

static void fill(DevBuf<uint32_t> &b, uint32_t seed) { for (uint64_t i = 0; i < b.cap; ++i) b.p[i] = seed + (uint32_t)i; }
static bool holds(const DevBuf<uint32_t> &b, uint32_t seed, uint64_t n) { for (uint64_t i = 0; i < n; ++i) if (b.p[i] != seed + (uint32_t)i) return false; return true; }

static void growth_without_keep() {
    DevBuf<uint32_t> b;
    CHECK(!b && b.cap == 0);
    CHECK(b.reserve(100) == hipSuccess && b.p && b.cap == 100 && live_dev == 1);
    uint32_t *old = b.p;
    const long copies = n_copy, frees = n_dev_free, mallocs = n_malloc, waits = n_quiesce;
    CHECK(b.reserve(100, false, nullptr, idle) == hipSuccess && b.p == old && n_malloc == mallocs && n_quiesce == waits);   // room: a compare and a return
    CHECK(b.reserve(40, true, nullptr, idle) == hipSuccess && b.p == old && b.cap == 100 && n_malloc == mallocs);
    CHECK(b.reserve(120, false, nullptr, idle) == hipSuccess);
    CHECK(b.cap == 120 && n_copy == copies && n_dev_free == frees + 1 && n_malloc == mallocs + 1 && n_quiesce == waits + 1 && live_dev == 1);   // (no margin without keep)
    fill(b, 7);                                                    // (all 120 elements are the buffer's: ASan looks on)
}

static void growth_with_keep() {
    DevBuf<uint32_t> b;
    CHECK(b.reserve(1000, true, nullptr, idle) == hipSuccess && b.cap == 1000 && n_copy == 0);   // (an empty buffer: nothing to keep, no margin)
    fill(b, 11);
    long frees = n_dev_free;
    CHECK(b.reserve(1001, true, nullptr, idle) == hipSuccess);     // below the margin: half again
    CHECK(b.cap == 1500 && n_copy == 1 && n_dev_free == frees + 1 && holds(b, 11, 1000) && live_dev == 1);
    fill(b, 13);
    CHECK(b.reserve(2249, true, nullptr, idle) == hipSuccess && b.cap == 2250 && holds(b, 13, 1500));   // (one below it still)
    fill(b, 17);
    CHECK(b.reserve(3375, true, nullptr, idle) == hipSuccess && b.cap == 3375 && holds(b, 17, 2250));   // at the margin: what was asked
    fill(b, 19);
    CHECK(b.reserve(9000, true, nullptr, idle) == hipSuccess && b.cap == 9000 && holds(b, 19, 3375));   // above it: exactly what was asked
    CHECK(live_dev == 1);
}

static void failures() {
    DevBuf<uint32_t> b;
    CHECK(b.reserve(1000) == hipSuccess);
    fill(b, 23);
    // the margin's allocation fails: what was asked for, contents kept
    long errs = n_last_error, mallocs = n_malloc;
    fail_allocs(1, 1);
    CHECK(b.reserve(1100, true, nullptr, idle) == hipSuccess && b.cap == 1100 && holds(b, 23, 1000) && n_last_error == errs + 1 && n_malloc == mallocs + 2 && live_dev == 1);
    fill(b, 29);
    // both fail: an error, everything as before, nothing waited for, and a later reserve works
    uint32_t *old = b.p;
    long frees = n_dev_free, waits = n_quiesce, copies = n_copy;
    mallocs = n_malloc;
    fail_allocs(1, 2);
    CHECK(b.reserve(1200, true, nullptr, idle) == hipErrorOutOfMemory && n_malloc == mallocs + 2);
    CHECK(b.p == old && b.cap == 1100 && holds(b, 29, 1100) && n_dev_free == frees && n_quiesce == waits && n_copy == copies && live_dev == 1);
    fail_allocs(1, 1);
    CHECK(b.reserve(5000, false, nullptr, idle) == hipErrorOutOfMemory && b.p == old && b.cap == 1100 && live_dev == 1);   // (the one allocation of a request without margin)
    CHECK(b.reserve(1200, true, nullptr, idle) == hipSuccess && b.cap == 1650 && holds(b, 29, 1100) && live_dev == 1);
    // the copy fails, the wait fails: an error, the old block stands, the new one is given back
    old = b.p; fill(b, 31); frees = n_dev_free; waits = n_quiesce;
    fail_copy = true;
    CHECK(b.reserve(4000, true, nullptr, idle) == hipErrorInvalidValue && n_quiesce == waits);
    CHECK(b.p == old && b.cap == 1650 && holds(b, 31, 1650) && n_dev_free == frees + 1 && live_dev == 1);
    CHECK(b.reserve(4000, true, nullptr, idle_fails) == hipErrorUnknown && n_quiesce == waits + 1);
    CHECK(b.p == old && b.cap == 1650 && holds(b, 31, 1650) && n_dev_free == frees + 2 && live_dev == 1);
    CHECK(b.reserve(4000, false, nullptr, idle_fails) == hipErrorUnknown && b.p == old && b.cap == 1650 && live_dev == 1);
    CHECK(b.reserve(4000, true, nullptr, idle) == hipSuccess && b.cap == 4000 && holds(b, 31, 1650) && live_dev == 1);
}

static void release_and_move() {
    DevBuf<uint32_t> a, b;
    CHECK(a.reserve(10) == hipSuccess && b.reserve(20) == hipSuccess && live_dev == 2);
    fill(b, 37);
    uint32_t *pb = b.p;
    long frees = n_dev_free;
    a = std::move(b);                                              // the target's old block goes, the source is empty
    CHECK(n_dev_free == frees + 1 && live_dev == 1 && a.p == pb && a.cap == 20 && holds(a, 37, 20) && !b.p && b.cap == 0);
    DevBuf<uint32_t> c(std::move(a));
    CHECK(c.p == pb && c.cap == 20 && !a.p && a.cap == 0 && live_dev == 1);
    DevBuf<uint32_t> &self = c;
    c = std::move(self);
    CHECK(c.p == pb && c.cap == 20 && live_dev == 1);
    c.release();
    CHECK(!c.p && c.cap == 0 && live_dev == 0 && n_dev_free == frees + 2);
    c.release();
    CHECK(live_dev == 0 && n_dev_free == frees + 2);
    CHECK(c.reserve(5) == hipSuccess && c.cap == 5 && live_dev == 1);   // (and is as good as new)

    PinBuf h, g;
    CHECK(h.reserve(64, 3u) == hipSuccess && last_pin_flags == 3u && g.reserve(8, 0) == hipSuccess && live_pin == 2);
    h = std::move(g);
    CHECK(live_pin == 1 && h.cap == 8 && !g.p && g.cap == 0);
    h.release(); h.release();
    CHECK(live_pin == 0 && !h.p && h.cap == 0);

    Event e, f;
    CHECK(e.create(2u) == hipSuccess && last_ev_flags == 2u && live_ev == 1);
    hipEvent_t he = e;
    CHECK(he && e.create() == hipSuccess && (hipEvent_t)e == he && live_ev == 1);   // create(): nothing when it is there
    CHECK(f.create() == hipSuccess && last_ev_flags == hipEventDefault && live_ev == 2);
    f = std::move(e);
    CHECK(live_ev == 1 && (hipEvent_t)f == he && !(hipEvent_t)e);
    f.release(); f.release();
    CHECK(live_ev == 0);

    Stream s, t;
    CHECK(s.create() == hipSuccess && last_st_flags == hipStreamDefault && last_st_priority == 0 && live_st == 1);
    hipStream_t hs = s;
    CHECK(hs && s.create(hipStreamNonBlocking, 1) == hipSuccess && (hipStream_t)s == hs && live_st == 1);
    CHECK(t.create(hipStreamNonBlocking, 1) == hipSuccess && last_st_flags == hipStreamNonBlocking && last_st_priority == 1 && live_st == 2);
    t = std::move(s);
    CHECK(live_st == 1 && (hipStream_t)t == hs && !(hipStream_t)s);
    t.release(); t.release();
    CHECK(live_st == 0);
}

// as svjg_ctx declares them: streams first, so that they are destroyed last
struct Several { Stream st;  Event ev;  DevBuf<uint64_t> d;  PinBuf h;  DevBuf<uint8_t> never; };

static void several() {
    {
        Several x;
        CHECK(x.st.create() == hipSuccess && x.ev.create() == hipSuccess && x.d.reserve(3) == hipSuccess && x.h.reserve(3, 0) == hipSuccess && live() == 4);
        freed.clear();
    }
    CHECK(freed == "pdes" && live() == 0);
    {
        Several a[2];                                              // (an array member, as svjg_ctx::run: the last element first)
        CHECK(a[0].d.reserve(1) == hipSuccess && a[1].h.reserve(1, 0) == hipSuccess && a[1].st.create() == hipSuccess);
        freed.clear();
    }
    CHECK(freed == "psd" && live() == 0);
}

static void pinned() {
    PinBuf h;
    CHECK(!h && h.cap == 0);
    CHECK(h.reserve(100, 0) == hipSuccess && h.p && h.cap == 100 && live_pin == 1);
    memset(h, 0xA5, 100);
    uint8_t *old = h.p;
    freed.clear();
    CHECK(h.reserve(50, 0) == hipSuccess && h.p == old && h.cap == 100 && freed.empty());    // smaller
    CHECK(h.reserve(100, 0) == hipSuccess && h.p == old && h.cap == 100 && freed.empty());   // equal
    CHECK(h.p[99] == 0xA5);
    CHECK(h.reserve(101, 0) == hipSuccess && h.cap == 101 && freed == "p" && live_pin == 1);   // larger: the old block goes first, the contents with it
    memset(h, 0x5A, 101);
    fail_allocs(1, 1);
    CHECK(h.reserve(200, 0) == hipErrorOutOfMemory && !h.p && h.cap == 0 && live_pin == 0);   // (the old block was given up before: empty, not dangling)
    CHECK(h.reserve(200, 0) == hipSuccess && h.cap == 200 && live_pin == 1);
}

int main() {
    growth_without_keep();
    growth_with_keep();
    failures();
    release_and_move();
    several();
    pinned();
    CHECK(live() == 0);
    if (bad) { fprintf(stderr, "own_sim: %d of %d checks failed\n", bad, checks); return 1; }
    printf("own_sim ok: %d checks\n", checks);
    return 0;
}
