// ed_access.h -- what the streaming kernels of encdec_kernels.hip, decshare_kernels.hip, refresh_kernels.hip, bfv_refresh_kernels.hip, pcks_kernels.hip
// and skenc_kernels.hip share: the launch shape (256 threads, grid.x over PAIRS of coefficients), the 16-byte accesses and the lookup of a pointer
// table.  Included by those six files only (the names are short).
#pragma once
#include "encdec_kernels.h"

namespace mkhe {

constexpr int ED_THREADS = 256;
inline int ed_bx(int N) { return (N / 2 + ED_THREADS - 1) / ED_THREADS; }

typedef ulonglong2 u64x2;
__device__ __forceinline__ u64x2 ld2(const u64* p, long pair) { return reinterpret_cast<const u64x2*>(p)[pair]; }
__device__ __forceinline__ void st2(u64* p, long pair, u64 a, u64 b) { reinterpret_cast<u64x2*>(p)[pair] = u64x2{a, b}; }
__device__ __forceinline__ const u64* ed_entry(const EdTable& t, int i) { return t.dev ? t.dev[i] : t.p[i]; }

}  // namespace mkhe
