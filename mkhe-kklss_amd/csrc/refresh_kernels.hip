// refresh_kernels.hip -- see refresh_kernels.h.  No LDS, no scratch.
#include "refresh_kernels.h"
#include "sample_arith.h"

namespace mkhe {

// ---- refresh_finish_kernel: grid.x = ChaCha20 blocks of a polynomial (8 coefficients, 64 bytes of a limb per thread), grid.y = the item, so that
// both streams are wave-uniform and key and nonce are read from the kernel arguments (scalar loads).  The mask never exists in memory: per
// coefficient |M| = w1 2^60 + w0 with w0, w1 < 2^60 and a sign bit, in registers.  Per modulus |M| mod q = (w0 mod q) + w1 2^60 mod q: one
// Montgomery product with r1 = 2^64 mod q on the low word (mont_mul(a, r1) = a mod q for a < 2^62) and one with MForm(2^60 mod q) on the high
// word (the same reduction with the constant 2^60 folded in; the constant is wave-uniform, from r2), the sign folded in afterwards by a select --
// no sample-dependent branch or address.  One thread walks every modulus: M is formed once, and the share (j < lin) and the plaintext -M
// (j < lout) come out of the same registers and the same reduction.
__global__ void __launch_bounds__(BLK_THREADS) refresh_finish_kernel(RefreshMaskArgs a, u64* __restrict__ share, const u64* __restrict__ acc, u64* __restrict__ pt,
                                                                     const Mod* __restrict__ mods, int lin, int lout, int N) {
    const u32 blk = blockIdx.x * BLK_THREADS + threadIdx.x;                 // block index c: coefficients 8 c .. 8 c + 7
    if (blk >= (u32)(N / 8)) return;
    const int b = blockIdx.y;
    u64 w0[8], w1[8];
    u32 neg = 0;                                                            // bit i: M[i] is negative
#pragma unroll
    for (int i = 0; i < 8; ++i) w0[i] = w1[i] = 0;
    if (a.bits > 0) {
        u64 lo[8], hi[8];
        chacha_block8(a, blk, 2 * (u32)b, lo);
        chacha_block8(a, blk, 2 * (u32)b + 1, hi);
        const int sh = 128 - a.bits;                                        // 8 .. 127, wave-uniform
        const unsigned __int128 half = (unsigned __int128)1 << (a.bits - 1);
#pragma unroll
        for (int i = 0; i < 8; ++i) {                                       // kind 3: M = ((hi 2^64 + lo) >> (128 - bits)) - 2^(bits-1)
            u64 vl, vh;
            if (sh >= 64) { vl = hi[i] >> (sh - 64); vh = 0; }
            else { vl = (lo[i] >> sh) | (hi[i] << (64 - sh)); vh = hi[i] >> sh; }
            const __int128 e = (__int128)((((unsigned __int128)vh) << 64) | vl) - (__int128)half;
            const __int128 s = e >> 127;
            const unsigned __int128 m = (unsigned __int128)((e ^ s) - s);   // |M| <= 2^119
            w0[i] = (u64)m & ((1ull << 60) - 1);
            w1[i] = (u64)(m >> 60);
            neg |= (u32)((u64)s & 1) << i;
        }
    }
    const int top = lin > lout ? lin : lout;
    for (int j = 0; j < top; ++j) {
        const Mod md = mods[j];
        const u64 q = md.q;
        const u64 c60 = mont_mul(1ull << 60, md.r2, q, md.ninv32);          // MForm(2^60 mod q)
        u64 pos[8], ngt[8];                                                 // M mod q and -M mod q
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const u64 m = csub(mont_mul(w0[i], md.r1, q, md.ninv32) + mont_mul(w1[i], c60, q, md.ninv32), q);      // |M| mod q
            const bool n = (neg >> i) & 1;
            pos[i] = signed_mod_q(m, n, q);
            ngt[i] = signed_mod_q(m, !n, q);
        }
        if (j < lin) {
            const long row = (((long)b * lin + j) * N) / 2 + 4 * (long)blk;      // in pairs
            u64 v[8];
            ld8(acc, row, v);
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = csub(v[i] + pos[i], q);
            st8(share, row, v);
        }
        if (j < lout) st8(pt, (((long)b * lout + j) * N) / 2 + 4 * (long)blk, ngt);
    }
}
void launch_refresh_finish(const RefreshMaskArgs& a, int count, u64* share, const u64* acc, u64* pt, const Mod* mods, int lin, int lout, int N,
                           hipStream_t st) {
    hipLaunchKernelGGL(refresh_finish_kernel, dim3(blk_bx(N), count), dim3(BLK_THREADS), 0, st, a, share, acc, pt, mods, lin, lout, N);
}

// ---- refresh_merge_kernel: grid.x over the coefficients, grid.y = the item.  One thread owns coefficient n of item b through every modulus: the
// sums of the lin input limbs feed garner_digits (which stores the digits in this thread's column of the digit scratch) and, with the
// re-encryptions added, are polynomial 0 of the output there; the lift to the moduli above is Horner over the digits.  nre = 0 (mkhe_e2s_merge):
// no re-encryption is read and out[b] is the one polynomial R~ [lout][N].
constexpr int RFM_THREADS = 256;

__global__ void __launch_bounds__(RFM_THREADS) refresh_merge_kernel(RefreshMergeArgs a, EdTable out, EdTable c0, EdTable sh, EdTable re) {
    const long n = (long)blockIdx.x * RFM_THREADS + threadIdx.x;
    if (n >= a.N) return;
    const int b = blockIdx.y, lin = a.lin, lout = a.lout, nq = a.nq;
    const long N = a.N;
    u64* o = const_cast<u64*>(ed_entry(out, b));
    const u64* c = ed_entry(c0, b);
    u64* d = a.dig + (long)b * lin * N + n;
    // the residue of R under q_j, j < lin; behind it polynomial 0 of the output under that modulus
    auto residue = [&](int j, const Mod& md) {
        const u64 q = md.q;
        const u64 v = sum_shares(c[j * N + n], sh, a.nshares, ((long)b * lin + j) * N + n, q);
        if (j < lout) {
            u64 w = v;
            for (int i = 0; i < a.nre; ++i) w = csub(w + ed_entry(re, i * a.count + b)[j * N + n], q);
            o[j * N + n] = w;
        }
        return v;
    };
    if (lout > lin) {
        garner_digits(residue, d, a.garner, nq, a.mods, lin, N);
        bool neg = false;                                                   // R > (Q - 1) / 2  <=>  R > Q - 1 - R, whose digits are q_i - 1 - d_i
        for (int i = lin - 1; i >= 0; --i) {
            const u64 di = d[i * N], oi = a.mods[i].q - 1 - di;
            if (di != oi) { neg = di > oi; break; }
        }
        for (int j = lin; j < lout; ++j) {
            const Mod md = a.mods[j];
            const u64 q = md.q;
            u64 v = mont_mul(d[(lin - 1) * N], md.r1, q, md.ninv32);
            for (int i = lin - 2; i >= 0; --i)
                v = csub(mont_mul(v, a.qmont[i * nq + j], q, md.ninv32) + mont_mul(d[i * N], md.r1, q, md.ninv32), q);
            const u64 qp = a.qprod[(lin - 1) * nq + j];                     // Q_l mod q_j
            if (neg) v = v >= qp ? v - qp : v + q - qp;
            for (int i = 0; i < a.nre; ++i) v = csub(v + ed_entry(re, i * a.count + b)[j * N + n], q);
            o[j * N + n] = v;
        }
    } else {
        for (int j = 0; j < lout; ++j) residue(j, a.mods[j]);
    }
    for (int i = 0; i < a.nre; ++i) {
        const u64* r1 = ed_entry(re, i * a.count + b) + (long)lout * N;
        u64* o1 = o + (long)(1 + i) * lout * N;
        for (int j = 0; j < lout; ++j) o1[j * N + n] = r1[j * N + n];
    }
}
void launch_refresh_merge(const RefreshMergeArgs& a, const EdTable& out, const EdTable& c0, const EdTable& sh, const EdTable& re, hipStream_t st) {
    hipLaunchKernelGGL(refresh_merge_kernel, dim3((a.N + RFM_THREADS - 1) / RFM_THREADS, a.count), dim3(RFM_THREADS), 0, st, a, out, c0, sh, re);
}

}  // namespace mkhe
