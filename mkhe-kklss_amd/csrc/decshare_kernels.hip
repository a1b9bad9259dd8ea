// decshare_kernels.hip -- see decshare_kernels.h.  No LDS, no scratch.
#include "decshare_kernels.h"
#include "sample_arith.h"

namespace mkhe {

// ---- share_finish_kernel: grid.x = ChaCha20 blocks of a polynomial (8 coefficients, 64 bytes of a limb per thread), grid.y = the limb rows,
// grid.z = the item, so that the stream is wave-uniform and key and nonce are read from the kernel arguments (scalar loads).  The flooding
// sample never exists in memory: 8 magnitudes and their signs in registers, reduced per limb by one Montgomery product with r1 = 2^64 mod q
// (mont_mul(a, r1) = a mod q for a < 2^62) on the magnitude, the sign folded in afterwards by a select -- no sample-dependent branch.
__global__ void __launch_bounds__(BLK_THREADS) share_finish_kernel(ShareFloodArgs a, u64* __restrict__ out, const u64* __restrict__ acc, const Mod* __restrict__ mods,
                                                                   int limbs, int N) {
    const u32 blk = blockIdx.x * BLK_THREADS + threadIdx.x;                 // block index c: coefficients 8 c .. 8 c + 7
    if (blk >= (u32)(N / 8)) return;
    const int b = blockIdx.z;
    u64 mag[8];
    u32 neg = 0;                                                            // bit i: sample i is negative
#pragma unroll
    for (int i = 0; i < 8; ++i) mag[i] = 0;
    if (a.bits > 0) {
        u64 r[8];
        chacha_block8(a, blk, (u32)b, r);
        const int sh = 64 - a.bits;
        const i64 half = (i64)1 << (a.bits - 1);
#pragma unroll
        for (int i = 0; i < 8; ++i) {                                       // kind 2: e = (r >> (64 - bits)) - 2^(bits-1)
            const i64 e = (i64)(r[i] >> sh) - half;
            const i64 s = e >> 63;
            mag[i] = (u64)((e ^ s) - s);
            neg |= (u32)(s & 1) << i;
        }
    }
    for (int j = blockIdx.y; j < limbs; j += gridDim.y) {
        const Mod md = mods[j];
        const u64 q = md.q;
        const long row = (((long)b * limbs + j) * N) / 2 + 4 * (long)blk;  // in pairs
        u64 v[8];
        ld8(acc, row, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const u64 m = mont_mul(mag[i], md.r1, q, md.ninv32);            // |e| mod q
            v[i] = csub(v[i] + signed_mod_q(m, (neg >> i) & 1, q), q);
        }
        st8(out, row, v);
    }
}
void launch_share_finish(const ShareFloodArgs& a, int count, u64* out, const u64* acc, const Mod* mods, int limbs, int rows, int N, hipStream_t st) {
    hipLaunchKernelGGL(share_finish_kernel, dim3(blk_bx(N), rows < 1 ? 1 : (rows > limbs ? limbs : rows), count), dim3(BLK_THREADS), 0, st, a, out, acc, mods, limbs, N);
}

// ---- share_merge_kernel: the shape of decrypt_finish_kernel with nshares addends
__global__ void __launch_bounds__(ED_THREADS) share_merge_kernel(int nshares, u64* pt, EdTable c0, EdTable sh, const Mod* mods, int limbs, int N) {
    const int j = blockIdx.y, b = blockIdx.z;
    const u64 q = mods[j].q;
    const long half = N / 2;
    const long row = ((long)b * limbs + j) * half;                          // in pairs: the limb inside a [count][limbs][N] buffer
    const u64* c = ed_entry(c0, b) + (long)j * N;
    for (long n = (long)blockIdx.x * ED_THREADS + threadIdx.x; n < half; n += (long)gridDim.x * ED_THREADS) {
        const u64x2 v = sum_shares(ld2(c, n), sh, nshares, row + n, q);
        st2(pt, row + n, v.x, v.y);
    }
}
void launch_share_merge(int count, int nshares, u64* pt, const EdTable& c0, const EdTable& sh, const Mod* mods, int limbs, int N, hipStream_t st) {
    hipLaunchKernelGGL(share_merge_kernel, dim3(ed_bx(N), limbs, count), dim3(ED_THREADS), 0, st, nshares, pt, c0, sh, mods, limbs, N);
}

}  // namespace mkhe
