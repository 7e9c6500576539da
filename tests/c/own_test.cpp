// The owners of a context's HIP resources (compute_raytracer_amd/csrc/rt_own.h) without a GPU and without the HIP runtime: this
// program defines the eight entry points the header calls itself -- backed by malloc, counting calls and live objects per kind,
// refusing an allocation above a limit -- and prints one line per case.  Built and run by tests/test_own_cpu.py, which holds
// every line against the expectation written out.
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "../../compute_raytracer_amd/csrc/rt_own.h"

namespace {
struct Kind { long made = 0, released = 0, live = 0; };
Kind g_dev, g_pin, g_ev, g_st;
size_t g_limit = ~(size_t)0;        // an allocation above it is refused
unsigned g_flags = 0;               // of the last event / stream made

hipError_t make(Kind& k, void** out, size_t bytes) {
    ++k.made;
    if (bytes > g_limit) { *out = reinterpret_cast<void*>(0x1); return hipErrorOutOfMemory; }   // garbage the owner must not keep
    *out = std::malloc(bytes ? bytes : 1);
    ++k.live;
    return hipSuccess;
}
hipError_t release(Kind& k, void* p) {
    ++k.released;
    --k.live;
    std::free(p);
    return hipSuccess;
}
}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return make(g_dev, p, bytes); }
hipError_t hipFree(void* p) { return release(g_dev, p); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return make(g_pin, p, bytes); }
hipError_t hipHostFree(void* p) { return release(g_pin, p); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) { g_flags = flags; return make(g_ev, reinterpret_cast<void**>(e), 1); }
hipError_t hipEventDestroy(hipEvent_t e) { return release(g_ev, e); }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags) { g_flags = flags; return make(g_st, reinterpret_cast<void**>(s), 1); }
hipError_t hipStreamDestroy(hipStream_t s) { return release(g_st, s); }
}

template <class T> constexpr bool move_only() {
    return !std::is_copy_constructible<T>::value && !std::is_copy_assignable<T>::value &&
           std::is_nothrow_move_constructible<T>::value && std::is_nothrow_move_assignable<T>::value;
}
static_assert(move_only<DevBuf>() && move_only<PinnedBuf>() && move_only<Event>() && move_only<Stream>(), "the owners are move-only");

// made / released since the last call of the kind, what is alive, and the case's own fields
static void line(const char* name, const char* what, Kind& k, const char* own) {
    static Kind before[4];
    Kind& b = before[&k == &g_dev ? 0 : &k == &g_pin ? 1 : &k == &g_ev ? 2 : 3];
    std::printf("%s %s: made=%ld released=%ld live=%ld %s\n", name, what, k.made - b.made, k.released - b.released, k.live, own);
    b = k;
}

template <class BUF> static void buffer_cases(const char* name, Kind& k) {
    char own[64];
    auto say = [&](const char* c, const BUF* b, int err) {
        std::snprintf(own, sizeof own, "p=%d cap=%zu err=%d", b && b->p ? 1 : 0, b ? b->cap : 0, err);
        line(name, c, k, own);
    };
    {
        BUF b;
        int e = (int)b.replace(100);
        say("replace empty", &b, e);
        e = (int)b.replace(1000);
        say("replace larger", &b, e);
        e = (int)b.replace(10);
        say("replace smaller", &b, e);
        g_limit = 500;
        e = (int)b.replace(501);
        g_limit = ~(size_t)0;
        say("replace refused", &b, e != 0);
        e = (int)b.replace(7);
        say("replace after refusal", &b, e);
        b.reset();
        say("reset", &b, 0);
        b.reset();
        say("reset again", &b, 0);
    }
    say("scope exit", nullptr, 0);
    {
        BUF a;
        (void)a.replace(100);
        BUF b(std::move(a));
        say("move construct", &b, 0);
        say("moved from", &a, 0);
        BUF c;
        (void)c.replace(200);
        say("target made", &c, 0);
        c = std::move(b);
        say("move assign", &c, 0);
        say("moved from", &b, 0);
    }
    say("scope exit", nullptr, 0);
    {
        BUF a[4], b[4];
        for (int i = 0; i < 4; ++i) { (void)a[i].replace(16u << i); (void)b[i].replace(8); }
        say("arrays made", &a[3], 0);
        for (int i = 0; i < 4; ++i) b[i] = std::move(a[i]);
        say("array move assign", &b[3], 0);
        say("moved from", &a[3], 0);
    }
    say("scope exit", nullptr, 0);
}

template <class H> static void handle_cases(const char* name, Kind& k, unsigned flags) {
    char own[64];
    g_flags = 0;
    auto say = [&](const char* c, const H* h, int err) {
        std::snprintf(own, sizeof own, "h=%d flags=%u err=%d", h && h->h ? 1 : 0, g_flags, err);      // flags: of the last one made
        line(name, c, k, own);
    };
    {
        H h;
        say("fresh", &h, 0);
        int e = (int)h.ensure(flags);
        say("ensure", &h, e);
        const void* first = h.h;
        e = (int)h.ensure(flags);
        say("ensure again", &h, e || h.h != first);
        const void* raw = static_cast<decltype(h.h)>(h);      // the conversion HIP calls rely on
        say("converts", &h, raw != first);
        H g(std::move(h));
        say("move construct", &g, g.h != first);
        say("moved from", &h, 0);
        H f;
        (void)f.ensure();
        f = std::move(g);
        say("move assign", &f, f.h != first);
        say("moved from", &g, 0);
        g_limit = 0;
        H r;
        e = (int)r.ensure(flags);
        g_limit = ~(size_t)0;
        say("ensure refused", &r, e != 0);
    }
    say("scope exit", nullptr, 0);
    {
        H a[4], b[4];
        for (int i = 0; i < 4; ++i) { (void)a[i].ensure(flags); (void)b[i].ensure(flags); }
        for (int i = 0; i < 4; ++i) b[i] = std::move(a[i]);
        say("array move assign", &b[3], 0);
    }
    say("scope exit", nullptr, 0);
}

int main() {
    buffer_cases<DevBuf>("DevBuf", g_dev);
    buffer_cases<PinnedBuf>("PinnedBuf", g_pin);
    handle_cases<Event>("Event", g_ev, hipEventDisableTiming);
    handle_cases<Stream>("Stream", g_st, hipStreamNonBlocking);
    {   // `used` is the caller's: replace and reset zero it, a move carries it
        DevBuf b;
        (void)b.replace(64);
        b.used = 48;
        DevBuf c(std::move(b));
        std::printf("used: moved=%zu from=%zu", c.used, b.used);
        (void)c.replace(32);
        std::printf(" replaced=%zu", c.used);
        c.used = 5;
        g_limit = 0;
        (void)c.replace(1);
        g_limit = ~(size_t)0;
        std::printf(" refused=%zu as=%d\n", c.used, c.as<float>() == nullptr);
    }
    std::printf("live: dev=%ld pinned=%ld events=%ld streams=%ld\n", g_dev.live, g_pin.live, g_ev.live, g_st.live);
    return (g_dev.live || g_pin.live || g_ev.live || g_st.live) ? 1 : 0;
}
