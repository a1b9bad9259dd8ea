// device_memory_check.cpp -- csrc/device_memory.h over a HIP made of malloc / free / memcpy, under AddressSanitizer (with leak detection) and UBSan:
// every block the owner hands out is a host block, so a double free, a use after free or a block left behind is a sanitizer report.
// tests/test_cpp_device_memory.py builds and runs it; no GPU, no HIP runtime library.
#include "device_memory.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

// ---- the five HIP entry points the header uses.  fail_malloc_at / fail_memcpy_at = n > 0: the n-th call from now fails.
static long fail_malloc_at = 0, fail_memcpy_at = 0, syncs = 0;
static std::set<void*> live_blocks;

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) {
    if (fail_malloc_at > 0 && --fail_malloc_at == 0) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = std::malloc(bytes);
    live_blocks.insert(*p);
    return hipSuccess;
}
hipError_t hipFree(void* p) {
    if (!p) return hipSuccess;
    if (!live_blocks.erase(p)) { std::fprintf(stderr, "hipFree of a block that is not live\n"); std::abort(); }
    std::free(p);
    return hipSuccess;
}
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
    if (fail_memcpy_at > 0 && --fail_memcpy_at == 0) return hipErrorInvalidValue;
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) { ++syncs; return hipSuccess; }
const char* hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "error"; }
}

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)
template <class F> static bool throws(F f) { try { f(); } catch (const mkhe::Error&) { return true; } return false; }

static void* counting_alloc_calls_hip(size_t bytes) {          // a caller's allocation function: the owner must go through it
    void* d = nullptr;
    if (hipMalloc(&d, bytes) != hipSuccess) throw mkhe::Error("counting_alloc: no memory");
    return d;
}

// mark, two uploads, a third that fails (in its allocation or in its copy): the exception comes out, rollback frees exactly the two, a retry succeeds
static void rollback_case(bool fail_in_copy) {
    mkhe::DeviceMemory m;
    const std::vector<uint64_t> a(100, 7), b(3, 9), c(50, 11);
    uint64_t* keep = m.upload(a);
    const size_t mark = m.mark();
    CHECK(mark == 1 && m.live() == 1);
    for (int attempt = 0; attempt < 2; ++attempt) {
        const bool fail = attempt == 0;
        uint64_t *x = nullptr, *y = nullptr, *z = nullptr;
        bool threw = false;
        try {
            x = m.upload(b); y = m.upload(c);
            if (fail) (fail_in_copy ? fail_memcpy_at : fail_malloc_at) = 1;
            z = m.upload(a);
        } catch (const mkhe::Error&) {
            threw = true;
            CHECK(m.live() == mark + 2);                       // the failed upload left no block of its own
            m.rollback(mark);
        }
        CHECK(threw == fail);
        if (fail) { CHECK(m.live() == mark && live_blocks.size() == 1 && live_blocks.count(keep)); continue; }
        CHECK(m.live() == mark + 3 && live_blocks.size() == 4);
        CHECK(x[2] == 9 && y[49] == 11 && z[99] == 7 && keep[0] == 7);
    }
    m.rollback(m.mark());                                      // nothing since the mark: nothing goes
    CHECK(m.live() == 4);
}

int main() {
    {   // upload of an empty vector, alloc / free / free(nullptr), free of an unknown pointer
        mkhe::DeviceMemory m;
        CHECK(m.live() == 0 && m.mark() == 0);
        int* e = m.upload(std::vector<int>());
        CHECK(e != nullptr && m.live() == 1);
        void* p = m.alloc(64);
        void* z = m.alloc(0);
        CHECK(p && z && m.live() == 3 && live_blocks.size() == 3);
        std::memset(p, 1, 64);
        m.free(p);
        CHECK(m.live() == 2 && !live_blocks.count(p));
        m.free(nullptr);
        CHECK(m.live() == 2);
        int other = 0;
        CHECK(throws([&] { m.free(&other); }));
        CHECK(throws([&] { m.free(p); }));                     // (freed already: no longer one of its blocks)
        CHECK(m.live() == 2);
        fail_malloc_at = 1;
        CHECK(throws([&] { m.alloc(8); }));
        CHECK(m.live() == 2);
        m.free(e); m.free(z);
        CHECK(m.live() == 0 && live_blocks.empty());
    }
    rollback_case(false);
    rollback_case(true);
    CHECK(live_blocks.empty());
    {   // grow
        mkhe::DeviceMemory m;
        mkhe::Scratch s;
        CHECK(m.grow(s, 0, nullptr) == nullptr && m.live() == 0);
        uint64_t* p0 = m.grow(s, 16, nullptr);
        CHECK(p0 && s.p == p0 && s.words == 16 && m.live() == 1 && syncs == 0);         // nothing to drain before the first block
        p0[15] = 1;
        CHECK(m.grow(s, 4, nullptr) == p0 && m.grow(s, 16, nullptr) == p0 && s.words == 16 && syncs == 0);
        uint64_t* p1 = m.grow(s, 17, nullptr);
        CHECK(p1 && s.p == p1 && s.words == 17 && m.live() == 1 && syncs == 1);         // drained, then the old block freed
        CHECK(live_blocks.size() == 1 && live_blocks.count(p1));
        p1[16] = 2;
        fail_malloc_at = 1;
        CHECK(throws([&] { m.grow(s, 1000, nullptr); }));
        // consistent afterwards: the old block intact, or empty
        CHECK((s.p == p1 && s.words == 17 && m.live() == 1) || (s.p == nullptr && s.words == 0 && m.live() == 0));
        CHECK(live_blocks.size() == m.live());
        uint64_t* p2 = m.grow(s, 1000, nullptr);
        CHECK(p2 && s.words == 1000 && m.live() == 1);
        p2[999] = 3;
        m.release();
        CHECK(m.live() == 0 && live_blocks.empty());
        m.release();                                           // twice
        CHECK(m.live() == 0);
        void* again = m.alloc(8);                              // and usable afterwards
        CHECK(again && m.live() == 1);
    }
    CHECK(live_blocks.empty());                                // (the destructor released `again`)
    {   // the caller's allocation function; an owner destroyed with blocks still held
        mkhe::DeviceMemory m(&counting_alloc_calls_hip);
        m.alloc(32); m.upload(std::vector<double>(5, 1.5));
        mkhe::Scratch s;
        m.grow(s, 8, nullptr);
        CHECK(m.live() == 3 && live_blocks.size() == 3);
        fail_malloc_at = 1;
        CHECK(throws([&] { m.alloc(8); }));
    }
    CHECK(live_blocks.empty());
    std::printf("device memory owner ok\n");
    return 0;
}
