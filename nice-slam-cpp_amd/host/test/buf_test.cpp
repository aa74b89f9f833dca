// CPU test of csrc/nsk_buf.h (no torch, no HIP): DevBuf over a counting allocator whose k-th allocation fails.  The allocator aborts on
// a pointer freed twice or never handed out; built with AddressSanitizer + UBSan (make buf_test_asan), driven by tests/test_host_io.py.
#include "../../csrc/nsk_buf.h"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>

#define REQUIRE(x) do { if (!(x)) { std::printf("buf_test: %s:%d: %s\n", __FILE__, __LINE__, #x); std::exit(1); } } while (0)

struct Fake {
    static std::set<void*> live, freed;
    static int allocs, frees, calls, fail_at;       // fail_at: the call (1-based) that fails, 0 = none
    static void restart(int k) { live.clear(); freed.clear(); allocs = frees = calls = 0; fail_at = k; }
    static int alloc(void** p, size_t bytes)
    {
        if (++calls == fail_at) return 2;            // leaves *p alone, as hipMalloc does
        *p = std::malloc(bytes ? bytes : 1);
        REQUIRE(*p);
        live.insert(*p); freed.erase(*p); ++allocs;   // (malloc may hand an address out again)
        return 0;
    }
    static void free(void* p)
    {
        REQUIRE(!freed.count(p));                    // freed twice
        REQUIRE(live.erase(p) == 1);                 // never handed out
        freed.insert(p); ++frees;
        std::free(p);
    }
    static bool balanced() { return live.empty() && allocs == frees; }
};
std::set<void*> Fake::live, Fake::freed;
int Fake::allocs, Fake::frees, Fake::calls, Fake::fail_at;

template <typename T> using Buf = DevBuf<T, Fake>;
struct Group { Buf<float> v, m, s; Buf<unsigned char> mask; };

// a grow-and-retry sequence over a few owners; the k-th allocation of the run fails
static void scenario(int k)
{
    Fake::restart(k);
    {
        Buf<float> a;
        Buf<int> b[3];
        const size_t sizes[4] = {16, 64, 8, 256};
        for (size_t n : sizes) {
            const int e = a.alloc(n);
            if (e != 0) { REQUIRE(e == 2 && a.get() == nullptr && a.cap() == 0); }
            else { REQUIRE(a.get() != nullptr && a.cap() == n); a[n - 1] = 1.f; }
            if (e != 0) REQUIRE(a.alloc(n) == 0 && a.cap() == n);      // the retry finds an empty buffer, not a stale one
            for (auto& x : b) {
                if (x.alloc(n) != 0) { REQUIRE(!x && x.cap() == 0); x.reset(); REQUIRE(!x && x.cap() == 0); }
                else REQUIRE(x.cap() == n);
            }
        }
        Group g;                                      // fails as a group: after a failure no member is allocated
        int r = g.v.alloc(32);
        if (r == 0) r = g.m.alloc(32);
        if (r == 0) r = g.s.alloc(32);
        if (r == 0) r = g.mask.alloc(1);
        if (r != 0) {
            const int before = Fake::frees, held = !!g.v + !!g.m + !!g.s + !!g.mask;
            reset_all(g.v, g.m, g.s, g.mask);
            REQUIRE(Fake::frees == before + held);
            REQUIRE(!g.v && !g.m && !g.s && !g.mask && g.v.cap() + g.m.cap() + g.s.cap() + g.mask.cap() == 0);
        }
    }
    REQUIRE(Fake::balanced());
}

static void ownership()
{
    Fake::restart(0);
    {
        Buf<float> a, b;
        REQUIRE(a.alloc(10) == 0 && b.alloc(20) == 0);
        float* pa = a; float* pb = b;
        a.swap(b);                                    // forward_core exchanges the two sampling sets
        REQUIRE(Fake::frees == 0 && a.get() == pb && a.cap() == 20 && b.get() == pa && b.cap() == 10);
        std::swap(a, b);
        REQUIRE(Fake::frees == 0 && a.get() == pa && a.cap() == 10 && b.get() == pb && b.cap() == 20);
        Buf<float> c(std::move(a));
        REQUIRE(Fake::frees == 0 && !a && a.cap() == 0 && c.get() == pa && c.cap() == 10);
        Buf<float> d;
        d = std::move(c);
        REQUIRE(Fake::frees == 0 && !c && d.get() == pa && d.cap() == 10);
        d = std::move(b);                             // the target's own allocation is freed, once
        REQUIRE(Fake::frees == 1 && !b && d.get() == pb && d.cap() == 20 && Fake::freed.count(pa));
        Group g, h;
        REQUIRE(g.v.alloc(4) == 0 && g.mask.alloc(4) == 0);
        float* pv = g.v;
        h = std::move(g);                             // w = Workspace(): member-wise
        REQUIRE(Fake::frees == 1 && h.v.get() == pv && !g.v && !g.mask);
        h = Group();
        REQUIRE(Fake::frees == 3 && !h.v && !h.mask);
        REQUIRE(d.alloc(0) == 0 && d.cap() == 0);     // replaces, even by nothing
        REQUIRE(Fake::frees == 4);
    }
    REQUIRE(Fake::balanced());
}

int main()
{
    scenario(0);
    const int total = Fake::calls;
    REQUIRE(total > 16);
    for (int k = 1; k <= total + 1; ++k) scenario(k);
    ownership();
    std::printf("buf_test ok: %d failure points\n", total + 1);
    return 0;
}
