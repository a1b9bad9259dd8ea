// bfv_arith.h -- the device functions bfv_kernels.hip (the batch encoder) and bfv_refresh_kernels.hip (the collective refresh of MK-BFV) share:
// arithmetic mod T < 2^32 on canonical residues and scale_up / scale_down of one coefficient (bfv_kernels.h).  Included by those two files only.
#pragma once
#include "bfv_kernels.h"

namespace mkhe {

// ---- arithmetic mod T < 2^32 on canonical residues
__device__ __forceinline__ u32 bf_mul(u32 a, uint2 w, u32 T) {            // a * w.x mod T for any 32-bit a; w.y = floor(w.x 2^32 / T)
    const u32 q = hi32((u64)a * w.y);
    const u64 r = (u64)a * w.x - (u64)q * T;                              // in [0, 2T)
    return (u32)(r >= T ? r - T : r);
}
__device__ __forceinline__ u32 bf_add(u32 a, u32 b, u32 T) { const u64 s = (u64)a + b; return (u32)(s >= T ? s - T : s); }
__device__ __forceinline__ u32 bf_sub(u32 a, u32 b, u32 T) { return a >= b ? a - b : a - b + T; }
// any 64-bit value mod T: hi * (2^32 mod T) + lo
__device__ __forceinline__ u32 bf_reduce64(u64 a, const BfvT& t) {
    return bf_add(bf_mul(hi32(a), uint2{t.c32, t.c32_s}, t.T), bf_mul(lo32(a), uint2{1u, t.one_s}, t.T), t.T);
}

// ---- scale_up / scale_down of one coefficient (bfv_kernels.h); pt, dig: the coefficient's column, limb stride N
// scale_up in two halves.  Once per coefficient: r = (Q m + floor(T/2)) mod T as the sign (r > floor(T/2)) and the magnitude of floor(T/2) - r ..
__device__ __forceinline__ u64 bf_scale_up_mag(const BfvT& t, u32 m, bool& neg) {
    const u32 r = bf_add(bf_mul(m, uint2{t.qmod, t.qmod_s}, t.T), t.half, t.T);
    neg = r > t.half;
    return neg ? r - t.half : t.half - r;                                 // |floor(T/2) - r| <= T
}
// .. and per limb l the product with tinv = MForm(T^-1 mod q_l)
__device__ __forceinline__ u64 bf_scale_up_limb(u64 mag, bool neg, u64 tinv, const Mod& md) {
    const u64 v = mont_mul(mag, tinv, md.q, md.ninv32);
    return (neg && v) ? md.q - v : v;
}
__device__ __forceinline__ void bf_scale_up_one(const BfvScale& sc, u32 m, u64* pt) {
    bool neg;
    const u64 mag = bf_scale_up_mag(sc.t, m, neg);
    for (int l = 0; l < sc.limbs; ++l) pt[(long)l * sc.N] = bf_scale_up_limb(mag, neg, sc.tinv_mont[l], sc.mods[l]);
}
// scale_down of the x in [0, Q) whose canonical residue mod q_j is first(j, mods[j])
template <class First> __device__ __forceinline__ u32 bf_scale_down_of(const BfvScale& sc, First first, u64* d) {
    const BfvT& t = sc.t;
    const int L = sc.limbs;
    const long N = sc.N;
    // the digits of r, r_j = T x_j + (q_j - 1) / 2 mod q_j
    garner_digits([&](int j, const Mod& md) { return csub(mont_mul(first(j, md), sc.t_mont[j], md.q, md.ninv32) + (md.q >> 1), md.q); }, d, sc.garner, L, sc.mods, L, N);
    u32 acc = bf_reduce64(d[(L - 1) * N], t);
    for (int i = L - 2; i >= 0; --i) acc = bf_add(bf_mul(acc, sc.qlt[i], t.T), bf_reduce64(d[i * N], t), t.T);
    return bf_mul(bf_sub(t.hq, acc, t.T), uint2{t.qinv, t.qinv_s}, t.T);
}
__device__ __forceinline__ u32 bf_scale_down_one(const BfvScale& sc, const u64* x, u64* d) {
    const long N = sc.N;
    return bf_scale_down_of(sc, [&](int j, const Mod&) { return x[j * N]; }, d);
}

}  // namespace mkhe
