// Stand-alone host check of the owning wrappers in csrc/vs_internal.h (DevBuf, HostBuf, DevEvent,
// PinnedPair): move-construct, move-assign, self-move, a growing vector of them, and the live-byte
// count.  The HIP allocation calls are replaced by counting host stubs, so an address / undefined
// behaviour sanitizer build of this program sees every double free, leak and use after move.
// Built and run by tests/test_devbuf_host.py; never loaded into another process.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

namespace stub {
std::set<void*> live_dev, live_host, live_ev;
int fail_next = 0;  // > 0: the next device allocation fails

inline hipError_t dev_malloc(void** p, size_t n) {
    if (fail_next > 0) {
        --fail_next;
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
    *p = std::malloc(n ? n : 1);
    live_dev.insert(*p);
    return hipSuccess;
}
template <typename T>
hipError_t dev_malloc(T** p, size_t n) { return dev_malloc((void**)p, n); }
inline hipError_t dev_free(void* p) {
    if (!live_dev.erase(p)) std::abort();  // freed twice, or never allocated
    std::free(p);
    return hipSuccess;
}
inline hipError_t host_malloc(void** p, size_t n, unsigned) {
    *p = std::malloc(n ? n : 1);
    live_host.insert(*p);
    return hipSuccess;
}
inline hipError_t host_free(void* p) {
    if (!live_host.erase(p)) std::abort();
    std::free(p);
    return hipSuccess;
}
inline hipError_t event_create(hipEvent_t* e, unsigned) {
    *e = (hipEvent_t)std::malloc(1);
    live_ev.insert(*e);
    return hipSuccess;
}
inline hipError_t event_destroy(hipEvent_t e) {
    if (!live_ev.erase(e)) std::abort();
    std::free(e);
    return hipSuccess;
}
}  // namespace stub

#define hipMalloc stub::dev_malloc
#define hipFree stub::dev_free
#define hipHostMalloc stub::host_malloc
#define hipHostFree stub::host_free
#define hipEventCreateWithFlags stub::event_create
#define hipEventDestroy stub::event_destroy
#include "../../photo_search_engine_amd/csrc/vs_internal.h"

void vs::set_last_error(const std::string&) {}

using namespace vs;

static int g_failed = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);      \
            ++g_failed;                                                \
        }                                                              \
    } while (0)

static int64_t live() { return g_dev_bytes_live.load(); }

template <typename T>
static void self_move(T& x) {
    T* alias = &x;  // (through a pointer: compilers warn about the literal x = std::move(x))
    x = std::move(*alias);
}

int main() {
    const int64_t base = live();
    {
        DevBuf a;
        a.ensure(100);
        CHECK(live() == base + 100 && a.bytes == 100 && a.p);
        void* p100 = a.p;
        a.ensure(50);  // grow-only: nothing happens
        CHECK(a.p == p100 && live() == base + 100);
        a.ensure(300);
        CHECK(a.bytes == 300 && live() == base + 300 && stub::live_dev.size() == 1);

        DevBuf b(std::move(a));  // move-construct: the source is left empty
        CHECK(!a.p && a.bytes == 0 && b.bytes == 300 && live() == base + 300);
        a.ensure(7);  // a moved-from buffer is usable again
        CHECK(live() == base + 307);

        a = std::move(b);  // move-assign: the target's old allocation is freed
        CHECK(!b.p && b.bytes == 0 && a.bytes == 300 && live() == base + 300 && stub::live_dev.size() == 1);

        self_move(a);
        CHECK(a.bytes == 300 && a.p && live() == base + 300);

        a.release();
        a.release();  // idempotent
        CHECK(live() == base && stub::live_dev.empty());

        // a failed growth leaves the buffer empty and the count right
        a.ensure(64);
        stub::fail_next = 1;
        bool threw = false;
        try {
            a.ensure(128);
        } catch (const VsError& e) {
            threw = e.code == VS_ERR_OOM;
        }
        CHECK(threw && !a.p && a.bytes == 0 && live() == base);

        // a vector of them growing: every reallocation moves, nothing is freed twice
        std::vector<DevBuf> v;
        int64_t want = 0;
        for (int i = 1; i <= 100; ++i) {
            v.emplace_back();
            v.back().ensure((size_t)i);
            want += i;
        }
        CHECK(live() == base + want && stub::live_dev.size() == 100);
        v.resize(10);
        CHECK(live() == base + 55 && stub::live_dev.size() == 10);
        std::vector<DevBuf> w(4);  // (vs_multi.hip sizes its per-device arrays this way)
        w[3].ensure(9);
        w = std::move(v);
        CHECK(live() == base + 55);
    }
    CHECK(live() == base && stub::live_dev.empty());

    {
        HostBuf h;
        h.ensure(32);
        HostBuf g(std::move(h));
        CHECK(!h.p && g.bytes == 32);
        h = std::move(g);
        self_move(h);
        CHECK(h.bytes == 32 && stub::live_host.size() == 1);
    }
    CHECK(stub::live_host.empty());

    {
        DevEvent none;  // empty until created
        CHECK((hipEvent_t)none == nullptr);
        DevEvent e(hipEventDisableTiming);
        CHECK((hipEvent_t)e != nullptr && stub::live_ev.size() == 1);
        DevEvent f(std::move(e));
        CHECK((hipEvent_t)e == nullptr && stub::live_ev.size() == 1);
        e = std::move(f);
        self_move(e);
        CHECK((hipEvent_t)e != nullptr && stub::live_ev.size() == 1);
        std::vector<std::pair<DevEvent, DevEvent>> tev;  // the screen-timing pairs
        for (int i = 0; i < 50; ++i) {
            DevEvent e0, e1;
            e0.create();
            e1.create();
            tev.emplace_back(std::move(e0), std::move(e1));
        }
        CHECK(stub::live_ev.size() == 101);
        tev.clear();
        CHECK(stub::live_ev.size() == 1);

        PinnedPair pp;
        pp.ensure(16);
        pp.ensure(64);
        CHECK(pp.host(0) && pp.host(1) && pp.chunk[1].bytes == 64 && stub::live_host.size() == 2 &&
              stub::live_ev.size() == 3);
        PinnedPair moved(std::move(pp));
        CHECK(stub::live_host.size() == 2 && moved.host(0) && !pp.host(0) && !(hipEvent_t)pp.done[1]);
    }
    CHECK(stub::live_ev.empty() && stub::live_host.empty());

    if (g_failed) return 1;
    std::printf("devbuf_moves: ok\n");
    return 0;
}
