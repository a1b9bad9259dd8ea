// bfv_refresh_kernels.hip -- see bfv_refresh_kernels.h.  No LDS, no scratch.
#include "bfv_refresh_kernels.h"
#include "bfv_arith.h"
#include "sample_arith.h"

namespace mkhe {

// ---- bfv_refresh_finish_kernel: grid.x = ChaCha20 blocks of a polynomial (8 coefficients, 64 bytes of a limb per thread), grid.y = the limb,
// grid.z = the item, so that every stream and every per-modulus constant is wave-uniform and key and nonce are read from the kernel arguments
// (scalar loads).  Per coefficient: A = ((hi 2^64 + lo) T) >> 128 from two 96-bit products -- no division, no sample-dependent branch -- and
// (T - A) mod T by a select; scale_up of both is the sign and magnitude of floor(T/2) - (Q x + floor(T/2)) mod T, formed once, times
// MForm(T^-1 mod q_j).  The flood is reduced by Horner over its words, high to low: f <- f 2^64 + v_w mod q_j, the first as a Montgomery product
// with r2 = 2^128 mod q_j, one block of one stream at a time (8 accumulators and 8 words live, whatever W is); 2^(flood_bits-1) mod q_j, which
// centres it, is wave-uniform.  The blocks are recomputed for every limb: W <= 16 blocks against the 8 W words a thread would otherwise hold.
// SECRET (bfv_e2s_finish_kernel, mkhe_bfv_e2s_share): pt is the caller's secret [count][N] and takes (T - A) mod T itself, over Z_T, from the limb-0 row
// of the grid only; no plaintext is written.  The blocks drawn, their order and the share are the same.  One body, two kernels.
template <bool SECRET> __device__ __forceinline__ void bfv_refresh_finish(const BfvRefreshArgs& a, u64* __restrict__ share, const u64* __restrict__ acc,
                                                                          u64* __restrict__ pt, const BfvScale& sc) {
    const u32 blk = blockIdx.x * BLK_THREADS + threadIdx.x;                 // block index c: coefficients 8 c .. 8 c + 7
    if (blk >= (u32)(sc.N / 8)) return;
    const int j = blockIdx.y, b = blockIdx.z;
    const int W = (a.flood_bits + 63) >> 6;                                 // words of the flood, 0 .. 16
    const u32 s0 = (u32)b * (u32)(2 + W);                                   // the first stream of item b
    const Mod md = sc.mods[j];
    const u64 q = md.q;
    // kind 4 and the two scalings
    u64 lo[8], hi[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) lo[i] = hi[i] = 0;
    if (a.mask) {                                                           // (wave-uniform)
        chacha_block8(a, blk, s0, lo);
        chacha_block8(a, blk, s0 + 1, hi);
    }
    const u64 tinv = sc.tinv_mont[j];
    const u32 T = sc.t.T;
    u64 up[8], dn[8];                                                       // up(A) and up((T - A) mod T) under q_j (SECRET: (T - A) mod T)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const unsigned __int128 ph = (unsigned __int128)hi[i] * T;          // below 2^96
        const u64 pl = (u64)(((unsigned __int128)lo[i] * T) >> 64);
        const u32 A = (u32)((ph + pl) >> 64);                               // in [0, T)
        const u32 An = A ? T - A : 0;
        bool neg;
        u64 mag = bf_scale_up_mag(sc.t, A, neg);
        up[i] = bf_scale_up_limb(mag, neg, tinv, md);
        if (SECRET) dn[i] = An;
        else {
            mag = bf_scale_up_mag(sc.t, An, neg);
            dn[i] = bf_scale_up_limb(mag, neg, tinv, md);
        }
    }
    // kind 5 mod q_j
    u64 f[8];
    flood_mod_q(a, blk, s0 + 2, a.flood_bits, md, f);
    const long row = (((long)b * sc.limbs + j) * sc.N) / 2 + 4 * (long)blk; // in pairs
    u64 v[8];
    ld8(acc, row, v);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = csub(csub(v[i] + up[i], q) + f[i], q);
    st8(share, row, v);
    if (!SECRET) st8(pt, row, dn);
    else if (j == 0) st8(pt, ((long)b * sc.N) / 2 + 4 * (long)blk, dn);
}
__global__ void __launch_bounds__(BLK_THREADS) bfv_refresh_finish_kernel(BfvRefreshArgs a, u64* __restrict__ share, const u64* __restrict__ acc, u64* __restrict__ pt,
                                                                         BfvScale sc) {
    bfv_refresh_finish<false>(a, share, acc, pt, sc);
}
__global__ void __launch_bounds__(BLK_THREADS) bfv_e2s_finish_kernel(BfvRefreshArgs a, u64* __restrict__ share, const u64* __restrict__ acc, u64* __restrict__ secret,
                                                                     BfvScale sc) {
    bfv_refresh_finish<true>(a, share, acc, secret, sc);
}
void launch_bfv_refresh_finish(const BfvRefreshArgs& a, int count, u64* share, const u64* acc, u64* pt, const BfvScale& sc, hipStream_t st) {
    hipLaunchKernelGGL(bfv_refresh_finish_kernel, dim3(blk_bx(sc.N), sc.limbs, count), dim3(BLK_THREADS), 0, st, a, share, acc, pt, sc);
}
void launch_bfv_e2s_finish(const BfvRefreshArgs& a, int count, u64* share, const u64* acc, u64* secret, const BfvScale& sc, hipStream_t st) {
    hipLaunchKernelGGL(bfv_e2s_finish_kernel, dim3(blk_bx(sc.N), sc.limbs, count), dim3(BLK_THREADS), 0, st, a, share, acc, secret, sc);
}

// ---- bfv_refresh_merge_kernel: grid.x over the coefficients, grid.y = the item.  One thread owns coefficient n of item b through every modulus:
// the sums of the input limbs feed bf_scale_down_of (whose Garner digits go to this thread's column of the digit scratch), the result w in [0, T)
// stays in a register and is scaled up under each modulus on the store, with the re-encryptions added there.
constexpr int BRM_THREADS = 256;

__global__ void __launch_bounds__(BRM_THREADS) bfv_refresh_merge_kernel(int count, int nshares, u64* dig, BfvScale sc, EdTable out, EdTable c0, EdTable sh, EdTable re) {
    const long n = (long)blockIdx.x * BRM_THREADS + threadIdx.x;
    if (n >= sc.N) return;
    const int b = blockIdx.y, L = sc.limbs;
    const long N = sc.N;
    u64* o = const_cast<u64*>(ed_entry(out, b));
    const u64* c = ed_entry(c0, b);
    // the residue of R under q_j
    const u32 w = bf_scale_down_of(sc, [&](int j, const Mod& md) { return sum_shares(c[j * N + n], sh, nshares, ((long)b * L + j) * N + n, md.q); },
                                   dig + (long)b * L * N + n);
    bool neg;
    const u64 mag = bf_scale_up_mag(sc.t, w, neg);
    for (int j = 0; j < L; ++j) {
        const Mod md = sc.mods[j];
        u64 v = bf_scale_up_limb(mag, neg, sc.tinv_mont[j], md);
        for (int i = 0; i < nshares; ++i) v = csub(v + ed_entry(re, i * count + b)[j * N + n], md.q);
        o[j * N + n] = v;
    }
    for (int i = 0; i < nshares; ++i) {
        const u64* r1 = ed_entry(re, i * count + b) + (long)L * N;
        u64* o1 = o + (long)(1 + i) * L * N;
        for (int j = 0; j < L; ++j) o1[j * N + n] = r1[j * N + n];
    }
}
void launch_bfv_refresh_merge(int count, int nshares, u64* dig, const BfvScale& sc, const EdTable& out, const EdTable& c0, const EdTable& sh, const EdTable& re,
                              hipStream_t st) {
    hipLaunchKernelGGL(bfv_refresh_merge_kernel, dim3((sc.N + BRM_THREADS - 1) / BRM_THREADS, count), dim3(BRM_THREADS), 0, st, count, nshares, dig, sc, out, c0, sh, re);
}

}  // namespace mkhe
