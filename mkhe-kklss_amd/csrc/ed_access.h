// ed_access.h -- how the protocol kernels (every *_kernels.hip that includes this file) reach memory: the two launch shapes, the 16-byte accesses, the
// 8-coefficient row access built from them and the lookup of a pointer table.  The names are short: include it from kernel files only.
#pragma once
#include "encdec_kernels.h"

namespace mkhe {

// streaming kernels: 256 threads, grid.x strides over PAIRS of coefficients (one 16-byte access per lane)
constexpr int ED_THREADS = 256;
inline int ed_bx(int N) { return (N / 2 + ED_THREADS - 1) / ED_THREADS; }
// sampling kernels: 128 threads, one thread = one ChaCha20 block = 8 consecutive coefficients; grid.x covers the N / 8 blocks of a row
constexpr int BLK_THREADS = 128;
inline int blk_bx(int N) { return (N / 8 + BLK_THREADS - 1) / BLK_THREADS; }

typedef ulonglong2 u64x2;
__device__ __forceinline__ u64x2 ld2(const u64* p, long pair) { return reinterpret_cast<const u64x2*>(p)[pair]; }
__device__ __forceinline__ void st2(u64* p, long pair, u64 a, u64 b) { reinterpret_cast<u64x2*>(p)[pair] = u64x2{a, b}; }
__device__ __forceinline__ const u64* ed_entry(const EdTable& t, int i) { return t.dev ? t.dev[i] : t.p[i]; }

// 8 consecutive coefficients of a u64 row from pair `pair` on: four 16-byte accesses
__device__ __forceinline__ void ld8(const u64* p, long pair, u64 (&v)[8]) {
    const u64x2 v0 = ld2(p, pair), v1 = ld2(p, pair + 1), v2 = ld2(p, pair + 2), v3 = ld2(p, pair + 3);
    v[0] = v0.x; v[1] = v0.y; v[2] = v1.x; v[3] = v1.y; v[4] = v2.x; v[5] = v2.y; v[6] = v3.x; v[7] = v3.y;
}
__device__ __forceinline__ void st8(u64* p, long pair, const u64 (&v)[8]) {
    st2(p, pair, v[0], v[1]); st2(p, pair + 1, v[2], v[3]); st2(p, pair + 2, v[4], v[5]); st2(p, pair + 3, v[6], v[7]);
}
// the same of an int32 row, from quadruple `quad` on: two 16-byte accesses
__device__ __forceinline__ void ld8(const i32* p, long quad, i32 (&v)[8]) {
    const int4 s0 = reinterpret_cast<const int4*>(p)[quad], s1 = reinterpret_cast<const int4*>(p)[quad + 1];
    v[0] = s0.x; v[1] = s0.y; v[2] = s0.z; v[3] = s0.w; v[4] = s1.x; v[5] = s1.y; v[6] = s1.z; v[7] = s1.w;
}
__device__ __forceinline__ void st8(i32* p, long quad, const i32 (&v)[8]) {
    reinterpret_cast<int4*>(p)[quad] = int4{v[0], v[1], v[2], v[3]};
    reinterpret_cast<int4*>(p)[quad + 1] = int4{v[4], v[5], v[6], v[7]};
}

}  // namespace mkhe
