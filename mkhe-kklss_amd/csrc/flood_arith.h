// flood_arith.h -- kind 5 of the keystream (include/mkhe.h, "collective refresh for MK-BFV": the wide uniform flood) reduced mod one modulus in
// registers: what bfv_refresh_finish_kernel (bfv_refresh_kernels.hip) and pcks_finish_kernel (pcks_kernels.hip) share.  Included by those two
// files only.
#pragma once
#include "chacha.h"

namespace mkhe {

// v mod q for ANY 64-bit v.  mont_mul(a, r1) reduces only a < 2^62, so the word is split: (v >> 32) 2^32 + (v mod 2^32), the high half times
// c32 = MForm(2^32 mod q) (the same reduction with the constant folded in), the low half times r1.
__device__ __forceinline__ u64 brf_reduce64(u64 v, u64 c32, const Mod& md) {
    return csub(mont_mul(hi32(v), c32, md.q, md.ninv32) + mont_mul(lo32(v), md.r1, md.q, md.ninv32), md.q);
}

// f[i] <- e[8 blk + i] mod q, canonical, e = sum_w v_w 2^(64 w) - 2^(flood_bits-1) with v_w the 64-bit value of stream first + w (the top word masked
// to its low flood_bits - 64 (W - 1) bits), W = ceil(flood_bits / 64); flood_bits = 0: f = 0 and no stream is read.  Horner over the words, high to
// low: f <- f 2^64 + v_w mod q, the first as a Montgomery product with r2 = 2^128 mod q, one block of one stream at a time (8 accumulators and 8
// words live, whatever W is); 2^(flood_bits-1) mod q, which centres it, is wave-uniform.  No sample-dependent branch.
__device__ __forceinline__ void flood_mod_q(const u32 (&key)[8], u32 nonce_lo, u32 nonce_hi, u32 blk, u32 first, int flood_bits, const Mod& md, u64 (&f)[8]) {
    const int W = (flood_bits + 63) >> 6;                                   // words of the flood, 0 .. 16
    const u64 q = md.q;
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = 0;
    if (W > 0) {                                                            // (wave-uniform)
        const u64 c32 = mont_mul(1ull << 32, md.r2, q, md.ninv32);          // MForm(2^32 mod q)
        const int tb = flood_bits - 64 * (W - 1);                           // bits of the top word, 1 .. 64
        const u64 topmask = tb == 64 ? ~0ull : (1ull << tb) - 1;
#pragma unroll 1
        for (int w = W - 1; w >= 0; --w) {
            u64 v[8];
            chacha_block8(key, nonce_lo, nonce_hi, blk, first + (u32)w, v);
            const u64 m = w == W - 1 ? topmask : ~0ull;
#pragma unroll
            for (int i = 0; i < 8; ++i) f[i] = csub(mont_mul(f[i], md.r2, q, md.ninv32) + brf_reduce64(v[i] & m, c32, md), q);
        }
        const int hb = flood_bits - 1;                                      // 2^hb = 2^(hb mod 64) (2^64)^(hb / 64)
        u64 half = brf_reduce64(1ull << (hb & 63), c32, md);
        for (int t = 0; t < (hb >> 6); ++t) half = mont_mul(half, md.r2, q, md.ninv32);
#pragma unroll
        for (int i = 0; i < 8; ++i) f[i] = f[i] >= half ? f[i] - half : f[i] + q - half;
    }
}

}  // namespace mkhe
