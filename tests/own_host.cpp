// The owners of f_renderer_amd/csrc/frr_own.h (DevBuf, Event) on the host alone: the four HIP calls they make are defined
// here over malloc, with a set of the live blocks that aborts on a double or foreign free.  Built with the address and
// undefined-behaviour sanitizers by tests/test_own_cpu.py; the HIP runtime is not linked.
#include "frr_own.h"
#include <hip/hip_runtime_api.h>

#include <stdio.h>
#include <stdlib.h>
#include <set>
#include <type_traits>
#include <vector>

static std::set<void *> g_live, g_events;
static int g_mallocs = 0, g_frees = 0, g_created = 0, g_destroyed = 0, g_timing = 0;
static bool g_fail_malloc = false, g_fail_event = false;
static size_t g_last_bytes = 0;

extern "C" hipError_t hipMalloc(void **p, size_t bytes)
{
    if (g_fail_malloc) { *p = (void *)0x10; return hipErrorOutOfMemory; }   // (a failing call may leave anything in *p)
    *p = malloc(bytes);
    g_live.insert(*p);
    g_last_bytes = bytes;
    ++g_mallocs;
    return hipSuccess;
}
extern "C" hipError_t hipFree(void *p)
{
    if (!g_live.erase(p)) { fprintf(stderr, "hipFree of a block that is not live: %p\n", p); abort(); }
    free(p);
    ++g_frees;
    return hipSuccess;
}
extern "C" hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags)
{
    if (g_fail_event) { *e = (hipEvent_t)0x10; return hipErrorOutOfMemory; }   // (... or in *e)
    *e = (hipEvent_t)malloc(1);
    g_events.insert(*e);
    ++g_created;
    if (flags != hipEventDisableTiming) ++g_timing;
    return hipSuccess;
}
extern "C" hipError_t hipEventDestroy(hipEvent_t e)
{
    if (!g_events.erase(e)) { fprintf(stderr, "hipEventDestroy of an event that is not live: %p\n", (void *)e); abort(); }
    free(e);
    ++g_destroyed;
    return hipSuccess;
}

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

using frr::DevBuf;
using frr::Event;

static_assert(!std::is_copy_constructible<DevBuf<float>>::value && !std::is_copy_assignable<DevBuf<float>>::value, "one owner");
static_assert(std::is_nothrow_move_constructible<DevBuf<float>>::value && std::is_nothrow_move_assignable<DevBuf<float>>::value, "vector growth moves");
static_assert(!std::is_copy_constructible<Event>::value && !std::is_copy_assignable<Event>::value, "one owner");
static_assert(std::is_nothrow_move_constructible<Event>::value && std::is_nothrow_move_assignable<Event>::value, "vector growth moves");

// the Mesh / Lines pattern of frr_api.hip: a slot record with owners, views and a flag
struct Rec {
    DevBuf<float> a; DevBuf<uint32_t> b;
    const float *view = nullptr;
    Event ev;
    bool used = false;
};

static void test_devbuf()
{
    {
        DevBuf<float> e;                                         // an empty one frees nothing
        CHECK(e.get() == nullptr && e.cap() == 0 && !e);
        CHECK(e.release() == hipSuccess);
    }
    CHECK(g_mallocs == 0 && g_frees == 0);
    {
        DevBuf<float> b;
        CHECK(b.reset(10) == hipSuccess && b.get() && b.cap() == 10 && g_last_bytes == 40);
        float *first = b.get();
        first[9] = 1.0f;                                         // (the sanitizer watches the bounds)
        CHECK(b.reset(1000) == hipSuccess && b.cap() == 1000 && g_last_bytes == 4000);   // larger: the old block goes exactly once
        CHECK(g_mallocs == 2 && g_frees == 1 && g_live.size() == 1 && !g_live.count(first));
        b.get()[999] = 2.0f;
        float *p = b;                                            // the view
        CHECK(p == b.get());
        DevBuf<float> m(std::move(b));                           // a move leaves the source empty
        CHECK(b.get() == nullptr && b.cap() == 0 && m.get() == p && m.cap() == 1000 && g_frees == 1);
        DevBuf<float> full;
        CHECK(full.reset(5) == hipSuccess);
        float *old = full.get();
        full = std::move(m);                                     // move-assignment onto a full one frees the target's block
        CHECK(g_frees == 2 && !g_live.count(old) && full.get() == p && full.cap() == 1000 && m.get() == nullptr && m.cap() == 0);
        DevBuf<float> &self = full;
        full = std::move(self);                                  // onto itself: nothing happens
        CHECK(full.get() == p && g_frees == 2);
        DevBuf<float> z;
        CHECK(z.reset(0) == hipSuccess && z.get() && z.cap() == 0 && g_last_bytes == 16);   // a zero-size request: 16 bytes
        g_fail_malloc = true;                                    // a failed allocation leaves it empty (the old block is gone)
        CHECK(full.reset(2000) == hipErrorOutOfMemory && full.get() == nullptr && full.cap() == 0 && g_frees == 3);
        DevBuf<float> never;
        CHECK(never.reset(8) == hipErrorOutOfMemory && never.get() == nullptr && never.cap() == 0);
        g_fail_malloc = false;
        CHECK(g_live.size() == 1);                               // z
    }
    CHECK(g_live.empty() && g_mallocs == g_frees && g_mallocs == 4);
}

static void test_event()
{
    {
        Event e;                                                 // an empty one destroys nothing
        CHECK((hipEvent_t)e == nullptr);
    }
    CHECK(g_created == 0 && g_destroyed == 0);
    {
        Event a, t;
        CHECK(a.create() == hipSuccess && (hipEvent_t)a && g_timing == 0);
        CHECK(t.create(true) == hipSuccess && g_timing == 1);    // with timing
        hipEvent_t ha = a;
        CHECK(a.create() == hipSuccess && g_destroyed == 1 && !g_events.count(ha));   // again: the old one goes exactly once
        ha = a;
        Event m(std::move(a));                                   // a move leaves the source empty
        CHECK((hipEvent_t)a == nullptr && (hipEvent_t)m == ha && g_destroyed == 1);
        hipEvent_t ht = t;
        t = std::move(m);                                        // move-assignment onto a full one destroys the target's event
        CHECK(g_destroyed == 2 && !g_events.count(ht) && (hipEvent_t)t == ha && (hipEvent_t)m == nullptr);
        g_fail_event = true;
        Event f;
        CHECK(f.create() != hipSuccess && (hipEvent_t)f == nullptr);
        CHECK(t.create() != hipSuccess && (hipEvent_t)t == nullptr && g_destroyed == 3);   // (the old one is gone)
        g_fail_event = false;
        t.destroy(); t.destroy();                                // on an empty one: nothing
        CHECK(g_destroyed == 3);
    }
    CHECK(g_events.empty() && g_created == g_destroyed && g_created == 3);
}

static void test_slots()
{
    const int frees0 = g_frees;
    {
        std::vector<Rec> v;
        std::vector<const float *> views;
        for (int i = 0; i < 100; ++i) {                          // growth moves every record, many times
            Rec r;
            CHECK(r.a.reset(16 + i) == hipSuccess && r.b.reset(3) == hipSuccess && r.ev.create() == hipSuccess);
            r.view = r.a; r.used = true;
            r.a.get()[15 + i] = (float)i;
            views.push_back(r.view);
            v.push_back(std::move(r));
            CHECK(r.a.get() == nullptr && r.b.get() == nullptr && (hipEvent_t)r.ev == nullptr);
        }
        CHECK(g_frees == frees0 && g_live.size() == 200 && g_events.size() == 100);
        for (int i = 0; i < 100; ++i) CHECK(v[i].a.get() == views[i] && v[i].view == views[i] && v[i].a.cap() == (size_t)16 + i && v[i].a.get()[15 + i] == (float)i);
        v[7] = Rec();                                            // slot reset: the slot's blocks and event go, the others stay
        CHECK(g_frees == frees0 + 2 && g_live.size() == 198 && g_events.size() == 99 && !g_live.count((void *)views[7]) && !v[7].used && !v[7].a);
        Rec n;                                                   // ... and the slot is taken again
        CHECK(n.a.reset(4) == hipSuccess);
        n.used = true;
        v[7] = std::move(n);
        CHECK(v[7].used && v[7].a.cap() == 4 && g_live.size() == 199);
        v.erase(v.begin());                                      // every later record moves down one
        CHECK(g_live.size() == 197 && v[0].a.get() == views[1]);
        std::vector<Event> pool;                                 // the pools of frr_api.hip: hand out the last, take it back
        for (int i = 0; i < 20; ++i) { pool.emplace_back(); CHECK(pool.back().create(i & 1) == hipSuccess); }
        Event e = std::move(pool.back()); pool.pop_back();
        CHECK((hipEvent_t)e && pool.size() == 19);
        pool.push_back(std::move(e));
        CHECK((hipEvent_t)e == nullptr && g_events.size() == 118);
    }
    CHECK(g_live.empty() && g_events.empty());
}

int main()
{
    test_devbuf();
    test_event();
    test_slots();
    if (!g_live.empty() || !g_events.empty() || g_mallocs != g_frees || g_created != g_destroyed) { fprintf(stderr, "leak\n"); return 1; }
    printf("own_host: ok (%d allocations, %d events)\n", g_mallocs, g_created);
    return 0;
}
