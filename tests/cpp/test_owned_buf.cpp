// mx::Owned (memex_amd/csrc/mx_owned.h) with a fake counting policy: plain C++, no HIP, no GPU.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "../../memex_amd/csrc/mx_owned.h"

static std::set<void *> g_live;
static int g_double_free = 0, g_allocs = 0, g_fail_at = 0;  // g_fail_at: fail the n-th next acquire (0: none)

struct Fake {
    using error = int;
    static constexpr error ok = 0;
    static unsigned last_flags;
    static size_t last_bytes;
    static error acquire(void **p, size_t bytes, unsigned flags) {
        ++g_allocs;
        if (g_fail_at > 0 && --g_fail_at == 0) return 7;
        last_flags = flags;
        last_bytes = bytes;
        *p = malloc(bytes ? bytes : 1);
        g_live.insert(*p);
        return ok;
    }
    static void release(void *p) {
        if (!g_live.erase(p)) {
            ++g_double_free;
            return;
        }
        free(p);
    }
};
unsigned Fake::last_flags = 0;
size_t Fake::last_bytes = 0;

#define CHECK(c)                                                 \
    do {                                                         \
        if (!(c)) {                                              \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                            \
        }                                                        \
    } while (0)

template <class T>
using Buf = mx::Owned<T, Fake>;

static const void *as_cvoid(const void *p) { return p; }

int main() {
    {   // alloc / realloc / reset, and the reads the host code makes through the implicit conversion
        Buf<float> a;
        CHECK(!a && a.get() == nullptr);
        CHECK(a.alloc(10, 3u) == 0 && a && Fake::last_bytes == 40 && Fake::last_flags == 3u && g_live.size() == 1);
        float *first = a;
        a[2] = 5.f;
        CHECK(first[2] == 5.f && a + 2 == first + 2 && as_cvoid(a) == first);
        float *other = nullptr;
        CHECK((a ? a : other) == first);
        CHECK(a.alloc(20) == 0 && Fake::last_bytes == 80 && g_live.size() == 1);  // the first block went before the second came
        a.reset();
        CHECK(!a && g_live.empty());
        a.reset();  // twice: nothing to release
        Buf<void> v;
        CHECK(v.alloc_bytes(33) == 0 && Fake::last_bytes == 33 && g_live.size() == 1);
    }
    CHECK(g_live.empty() && g_double_free == 0);
    {   // move construction and move assignment over a held buffer
        Buf<int> a, b;
        CHECK(a.alloc(4) == 0 && b.alloc(4) == 0 && g_live.size() == 2);
        int *pa = a;
        Buf<int> c(std::move(a));
        CHECK(!a && c.get() == pa && g_live.size() == 2);
        b = std::move(c);  // b's own block is released, c gives up pa
        CHECK(!c && b.get() == pa && g_live.size() == 1);
        Buf<int> &same = b;
        b = std::move(same);  // self-assignment keeps the block
        CHECK(b.get() == pa && g_live.size() == 1);
        Buf<int> empty;
        b = std::move(empty);  // assigning an empty buffer releases
        CHECK(!b && g_live.empty());
    }
    CHECK(g_live.empty() && g_double_free == 0);
    {   // a vector of buffers: grown (elements move), cleared
        std::vector<Buf<char>> v(3);
        for (auto &b : v) CHECK(b.alloc(8) == 0);
        v.resize(64);
        CHECK(g_live.size() == 3 && v[0] && v[2] && !v[3]);
        v.clear();
        CHECK(g_live.empty());
    }
    CHECK(g_double_free == 0);
    {   // a failed allocation leaves the buffer null (what it held is gone, once) and is not counted live
        Buf<float> a;
        CHECK(a.alloc(4) == 0);
        g_fail_at = 1;
        CHECK(a.alloc(8) == 7 && !a && g_live.empty());
        g_fail_at = 2;
        Buf<float> b;
        CHECK(b.alloc(1) == 0 && a.alloc(1) == 7 && !a && b && g_live.size() == 1);
        CHECK(a.alloc(1) == 0 && g_live.size() == 2);
    }
    CHECK(g_live.empty() && g_double_free == 0 && g_allocs == 13);
    printf("OK owned buffers\n");
    return 0;
}
