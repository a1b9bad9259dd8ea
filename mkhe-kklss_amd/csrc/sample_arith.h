// sample_arith.h -- the arithmetic the protocol kernels share, on the 8 coefficients of one ChaCha20 block or on one coefficient: the constant-time
// table scan, a signed sample as a residue, the sum of shares and the wide flood reduced mod one modulus.  Device-only, no state; a kernel that
// samples or merges is written against these, not against a copy of them.
#pragma once
#include "chacha.h"
#include "ed_access.h"

namespace mkhe {

// kind 1 of the keystream: e[i] = #{t : r[i] >= cdt[t]} - ncdt/2.  Every threshold is visited, whatever r is, with a full 64-bit unsigned compare: no
// sample-dependent branch or address.  The table comes from the kernel arguments, one threshold (a scalar load) at a time.
__device__ __forceinline__ void cdt_sample8(const SmallSampleArgs& a, const u64 (&r)[8], i32 (&e)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) e[i] = -(a.ncdt >> 1);
    for (int t = 0; t < a.ncdt; ++t) {
        const u64 T = a.cdt[t];
#pragma unroll
        for (int i = 0; i < 8; ++i) e[i] += (r[i] >= T) ? 1 : 0;
    }
}

// ExtendBasisSmallNormAndCenter of one sample: e >= 0 ? e : q - |e|, by a select
__device__ __forceinline__ u64 small_q(i32 e, u64 q) { return e < 0 ? q - (u64)(-(i64)e) : (u64)e; }

// a sample given as |e| mod q (canonical) and its sign: e mod q, by a select
__device__ __forceinline__ u64 signed_mod_q(u64 mag_mod_q, bool neg, u64 q) { return neg ? csub(q - mag_mod_q, q) : mag_mod_q; }

// kinds 6 and 7 of the keystream: v[i] = ((hi 2^64 + lo) q) >> 128 = (hi q + ((lo q) >> 64)) >> 64 with lo / hi the 64-bit values of coefficient
// 8 blk + i of the streams s0 and s0 + 1 of k: one full 64 x 64 product, the high word of a second and a carry.  Below q, since r < 2^128.
__device__ __forceinline__ void uniform_mod_q8(const StreamKey& k, u32 blk, u32 s0, u64 q, u64 (&v)[8]) {
    u64 lo[8], hi[8];
    chacha_block8(k, blk, s0, lo);
#pragma unroll
    for (int i = 0; i < 8; ++i) lo[i] = mulhi64(lo[i], q);                  // only (lo q) >> 64 is needed
    chacha_block8(k, blk, s0 + 1, hi);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        u64 ph, pl;
        mul64x64(hi[i], q, ph, pl);
        const u64 s = pl + lo[i];
        v[i] = ph + (s < pl ? 1 : 0);
    }
}

// (c0 + sum_{i < nshares} sh[i][at]) mod q, canonical, for any c0 below 3 q and canonical shares: one conditional subtraction per addend.
// One coefficient at word `at`, or the pair of coefficients at pair `at` (16-byte loads).
__device__ __forceinline__ u64 sum_shares(u64 c0, const EdTable& sh, int nshares, long at, u64 q) {
    u64 v = csub(csub(c0, q), q);
    for (int i = 0; i < nshares; ++i) v = csub(v + ed_entry(sh, i)[at], q);
    return v;
}
__device__ __forceinline__ u64x2 sum_shares(u64x2 c0, const EdTable& sh, int nshares, long at, u64 q) {
    u64x2 v{csub(csub(c0.x, q), q), csub(csub(c0.y, q), q)};
    for (int i = 0; i < nshares; ++i) {
        const u64x2 s = ld2(ed_entry(sh, i), at);
        v.x = csub(v.x + s.x, q);
        v.y = csub(v.y + s.y, q);
    }
    return v;
}

// v mod q for ANY 64-bit v.  mont_mul(a, r1) reduces only a < 2^62, so the word is split: (v >> 32) 2^32 + (v mod 2^32), the high half times
// c32 = MForm(2^32 mod q) (the same reduction with the constant folded in), the low half times r1.
__device__ __forceinline__ u64 brf_reduce64(u64 v, u64 c32, const Mod& md) {
    return csub(mont_mul(hi32(v), c32, md.q, md.ninv32) + mont_mul(lo32(v), md.r1, md.q, md.ninv32), md.q);
}

// kind 5 of the keystream (include/mkhe.h, "collective refresh for MK-BFV": the wide uniform flood) reduced mod one modulus in registers:
// f[i] <- e[8 blk + i] mod q, canonical, e = sum_w v_w 2^(64 w) - 2^(flood_bits-1) with v_w the 64-bit value of stream first + w (the top word masked
// to its low flood_bits - 64 (W - 1) bits), W = ceil(flood_bits / 64); flood_bits = 0: f = 0 and no stream is read.  Horner over the words, high to
// low: f <- f 2^64 + v_w mod q, the first as a Montgomery product with r2 = 2^128 mod q, one block of one stream at a time (8 accumulators and 8
// words live, whatever W is); 2^(flood_bits-1) mod q, which centres it, is wave-uniform.  No sample-dependent branch.
__device__ __forceinline__ void flood_mod_q(const StreamKey& k, u32 blk, u32 first, int flood_bits, const Mod& md, u64 (&f)[8]) {
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
            chacha_block8(k, blk, first + (u32)w, v);
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
