// device_memory.h -- the one owner of a Context's device allocations.  Host-side C++ over the HIP runtime API and the standard
// library only, so that a host compiler builds it: tests/cpp/device_memory_check.cpp runs it over a malloc-backed HIP under the sanitizers.
// The pointers the engine keeps (Context::d_*, the pools) are non-owning copies.  Memory a caller can see (handles) is not in here: Context::pool_free.
#pragma once
#include <hip/hip_runtime_api.h>
#include <assert.h>
#include <stdint.h>
#include <stdexcept>
#include <string>
#include <vector>

namespace mkhe {

struct Error : std::runtime_error { using std::runtime_error::runtime_error; };
#define MKHE_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) throw ::mkhe::Error(std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

// a grow-only scratch buffer (DeviceMemory::grow): the block and what it holds, in 8-byte words
struct Scratch { uint64_t* p = nullptr; size_t words = 0; };

class DeviceMemory {
  public:
    typedef void* (*AllocFn)(size_t bytes);     // bytes >= 1; throws Error when there is no memory
    explicit DeviceMemory(AllocFn fn = nullptr) : alloc_fn_(fn ? fn : &plain_alloc) {}
    DeviceMemory(const DeviceMemory&) = delete; DeviceMemory& operator=(const DeviceMemory&) = delete;
    ~DeviceMemory() { release(); }
    void* alloc(size_t bytes) {
        blocks_.reserve(blocks_.size() + 1);    // (the list cannot fail once the block exists)
        blocks_.push_back(alloc_fn_(bytes ? bytes : 1));
        return blocks_.back();
    }
    // a block with the vector's contents (synchronous copy; released again if the copy fails); an empty vector still gives a block
    template <class E> E* upload(const std::vector<E>& v) {
        E* d = static_cast<E*>(alloc(v.size() * sizeof(E)));
        if (v.empty()) return d;
        const hipError_t e = hipMemcpy(d, v.data(), v.size() * sizeof(E), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            rollback(blocks_.size() - 1);
            throw Error(std::string("hipMemcpy of a table to the device: ") + hipGetErrorString(e));
        }
        return d;
    }
    void free(void* p) {                        // nullptr: nothing; a pointer that is not one of the blocks throws
        if (!p) return;
        for (size_t i = blocks_.size(); i-- > 0;)
            if (blocks_[i] == p) { blocks_.erase(blocks_.begin() + i); MKHE_HIP(hipFree(p)); return; }
        throw Error("mkhe: DeviceMemory::free of a pointer that is not one of its blocks");
    }
    // A build step of several blocks that leaves none behind when it fails half way: m = mark() in front, rollback(m) in the handler -- every block
    // allocated since goes (nothing older may have been freed in between).  The step's pointers dangle then: its next run assigns all of them again.
    size_t mark() const { return blocks_.size(); }
    void rollback(size_t mark) noexcept {
        assert(mark <= blocks_.size());         // a mark above the list: something older than it was freed since it was taken
        while (blocks_.size() > mark) { (void)hipFree(blocks_.back()); blocks_.pop_back(); }
    }
    void release() noexcept { rollback(0); }
    size_t live() const { return blocks_.size(); }
    // at least want_words in s: the block it has when that is enough, else a new one -- the old one is freed first, behind everything `drain` has
    // queued (its last readers).  An allocation that fails leaves s empty.
    uint64_t* grow(Scratch& s, size_t want_words, hipStream_t drain) {
        if (s.words >= want_words) return s.p;
        if (s.p) {
            MKHE_HIP(hipStreamSynchronize(drain));
            void* old = s.p;
            s = Scratch{};
            free(old);
        }
        s.p = static_cast<uint64_t*>(alloc(want_words * sizeof(uint64_t)));
        s.words = want_words;
        return s.p;
    }
  private:
    static void* plain_alloc(size_t bytes) { void* d = nullptr; MKHE_HIP(hipMalloc(&d, bytes)); return d; }
    AllocFn alloc_fn_;
    std::vector<void*> blocks_;
};

}  // namespace mkhe
