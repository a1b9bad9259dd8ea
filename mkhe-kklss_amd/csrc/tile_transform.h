// tile_transform.h -- the in-place radix-2 transform of 2^logn points that both encoders run on tiles in LDS: the float64 FFT of the CKKS encoder
// (ckks_kernels.hip) and the 32-bit NTT mod T of the BFV batch encoder (bfv_kernels.hip).  Device code plus the launch shape; only those two
// files include it.  Decimation in frequency forward, in time inverse, so position p holds X[bitrev(p)].
//
// One workgroup transforms a TILE of 2^logt points in LDS.  2^logn <= the LDS limit: one tile = one message, one launch.  Larger transforms, or a
// lowered limit: two launches over a work buffer in global memory; 2^logn = A * B, A = 2^a_log:
//     column tile       A rows x (2^logt / A) adjacent columns of the A x B matrix: the a_log stages that span B and more
//     contiguous tile   2^logt adjacent points: the stages below
// forward in this order, inverse the other way round (TilePass, Context::tile_two_pass).  Two stages per pass over the tile (four elements per
// thread); the stages of span 8 .. 1 of a contiguous tile run on 16 adjacent elements per thread in registers (tile_tail16).
//
// The load of the first launch and the store of the last one differ between the encoders and stay in their kernels.  What else differs is in a
// traits struct Tr:
//     elem, twid, ctx                   element in LDS, twiddle table entry, what a butterfly needs besides (the modulus; nothing for float64)
//     bfly<INV>(a, b, w, ctx)           forward (a, b) <- (a + b, (a - b) w); inverse: the butterfly that undoes it up to the factor 2
//     swz(l), swzc(c)                   where element l resp. the parts of chunk c (16 elements) sit in LDS; each header derives its own
//     load16(s, c, x), store16(s, c, x) chunk c to registers and back
//     EPT                               elements per thread that size the workgroup
#pragma once
#include <hip/hip_runtime.h>
#include "tile_pass.h"

namespace mkhe {

// where the elements of a tile sit in the transform, and the twiddle of a butterfly
struct TileGeom {
    int logn, a_log, cc_log, tile, logt;
    __device__ __forceinline__ static TileGeom of(const TilePass& p) { return TileGeom{p.logn, p.a_log, p.logt - p.a_log, (int)blockIdx.x, p.logt}; }
    // global index of local element l: contiguous tile: tile * T + l; column tile: l = r * Cc + c -> r * B + tile * Cc + c (B = n >> a_log)
    __device__ __forceinline__ int g(int l) const {
        if (!a_log) return (tile << logt) + l;
        return ((l >> cc_log) << (logn - a_log)) + (tile << cc_log) + (l & ((1 << cc_log) - 1));
    }
    // the stage whose butterflies pair local elements 2^logh apart pairs global elements H = 2^logH apart; its twiddle at global index g is
    // omega^((g mod H) * n / 2H)
    __device__ __forceinline__ int tw(int l, int logh) const {
        const int logH = a_log ? logh - cc_log + logn - a_log : logh;
        return (g(l) & ((1 << logH) - 1)) << (logn - 1 - logH);
    }
};

// one stage on the tile in LDS: every thread takes butterflies of adjacent first elements
template <bool INV, class Tr> __device__ __forceinline__ void tile_stage2(typename Tr::elem* s, const typename Tr::twid* __restrict__ w, const TileGeom& ge, int logh, typename Tr::ctx cx) {
    const int h = 1 << logh, T = 1 << ge.logt;
    for (int u = threadIdx.x; u < T / 2; u += blockDim.x) {
        const int i = ((u >> logh) << (logh + 1)) | (u & (h - 1));
        typename Tr::elem a = s[Tr::swz(i)], b = s[Tr::swz(i + h)];
        Tr::template bfly<INV>(a, b, w[ge.tw(i, logh)], cx);
        s[Tr::swz(i)] = a; s[Tr::swz(i + h)] = b;
    }
}
// the stages 2^(lq+1) and 2^lq in one pass over the tile (forward: in this order; inverse: the other way round): the same operations
// as two tile_stage2 calls on the four elements i + {0, 1, 2, 3} * 2^lq
template <bool INV, class Tr> __device__ __forceinline__ void tile_stage4(typename Tr::elem* s, const typename Tr::twid* __restrict__ w, const TileGeom& ge, int lq, typename Tr::ctx cx) {
    const int hq = 1 << lq, T = 1 << ge.logt;
    for (int u = threadIdx.x; u < T / 4; u += blockDim.x) {
        const int i = ((u >> lq) << (lq + 2)) | (u & (hq - 1));
        typename Tr::elem x0 = s[Tr::swz(i)], x1 = s[Tr::swz(i + hq)], x2 = s[Tr::swz(i + 2 * hq)], x3 = s[Tr::swz(i + 3 * hq)];
        const typename Tr::twid wa = w[ge.tw(i, lq + 1)], wb = w[ge.tw(i + hq, lq + 1)], wc = w[ge.tw(i, lq)];
        if (INV) {
            Tr::template bfly<INV>(x0, x1, wc, cx); Tr::template bfly<INV>(x2, x3, wc, cx);
            Tr::template bfly<INV>(x0, x2, wa, cx); Tr::template bfly<INV>(x1, x3, wb, cx);
        } else {
            Tr::template bfly<INV>(x0, x2, wa, cx); Tr::template bfly<INV>(x1, x3, wb, cx);
            Tr::template bfly<INV>(x0, x1, wc, cx); Tr::template bfly<INV>(x2, x3, wc, cx);
        }
        s[Tr::swz(i)] = x0; s[Tr::swz(i + hq)] = x1; s[Tr::swz(i + 2 * hq)] = x2; s[Tr::swz(i + 3 * hq)] = x3;
    }
}
// the stages 8, 4, 2, 1 of a contiguous tile on 16 adjacent elements per thread, in registers.  Their twiddles are the 16th roots
// omega^(m n / 16), the same for every chunk.
template <bool INV, class Tr> __device__ __forceinline__ void tile_tail16(typename Tr::elem* s, const typename Tr::twid* __restrict__ w, int logn, int logt, typename Tr::ctx cx) {
    typename Tr::twid r16[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) r16[m] = w[m << (logn - 4)];
    for (int c = threadIdx.x; c < (1 << (logt - 4)); c += blockDim.x) {
        typename Tr::elem x[16];
        Tr::load16(s, c, x);
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const int h = INV ? 1 << st : 8 >> st;
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (!(e & h)) Tr::template bfly<INV>(x[e], x[e + h], r16[(e & (h - 1)) * (8 / h)], cx);
        }
        Tr::store16(s, c, x);
    }
}
// every stage of one launch on the loaded tile, a barrier behind each pass.  A contiguous tile has the local spans 2^(logt-1) .. 1, the last four
// of them in tile_tail16; a column tile the spans 2^(logt-1) .. Cc.
template <bool INV, class Tr> __device__ __forceinline__ void tile_stages(typename Tr::elem* s, const typename Tr::twid* __restrict__ w, const TilePass& p, const TileGeom& ge, typename Tr::ctx cx) {
    const int lo_log = p.a_log ? ge.cc_log : 4, hi_log = p.logt - 1;      // head stages lo_log .. hi_log
    const int odd = (hi_log - lo_log + 1) & 1;
    if (!INV) {
        int lh = hi_log;
        if (odd) { tile_stage2<INV, Tr>(s, w, ge, lh, cx); __syncthreads(); --lh; }
        for (; lh > lo_log; lh -= 2) { tile_stage4<INV, Tr>(s, w, ge, lh - 1, cx); __syncthreads(); }
        if (!p.a_log) { tile_tail16<INV, Tr>(s, w, p.logn, p.logt, cx); __syncthreads(); }
    } else {
        if (!p.a_log) { tile_tail16<INV, Tr>(s, w, p.logn, p.logt, cx); __syncthreads(); }
        int lh = lo_log;
        for (; lh + 1 <= hi_log; lh += 2) { tile_stage4<INV, Tr>(s, w, ge, lh, cx); __syncthreads(); }
        if (odd) { tile_stage2<INV, Tr>(s, w, ge, hi_log, cx); __syncthreads(); }
    }
}

// ---- host side
// 2^(logn - logt) tiles per message; 2^logt / elems_per_thread threads, at least one wave and at most 1024; the tile in dynamic LDS
struct TileLaunch { dim3 grid, block; size_t lds; };
inline TileLaunch tile_launch_shape(const TilePass& p, int count, int elems_per_thread, size_t elem_bytes) {
    const int T = 1 << p.logt;
    int threads = T / elems_per_thread;
    threads = threads < 64 ? 64 : threads > 1024 ? 1024 : threads;
    return TileLaunch{dim3(1 << (p.logn - p.logt), count), dim3(threads), elem_bytes * (size_t)T};
}
// asks for `bytes` of dynamic LDS (beyond the default limit) for both directions of a kernel; false: the runtime refused
template <class K> bool tile_request_lds(K kernel_fwd, K kernel_inv, int bytes) {
    const hipError_t e0 = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel_fwd), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    const hipError_t e1 = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel_inv), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e0 == hipSuccess && e1 == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}

}  // namespace mkhe
