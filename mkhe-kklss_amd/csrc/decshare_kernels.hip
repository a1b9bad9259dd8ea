// decshare_kernels.hip -- see decshare_kernels.h.  No LDS, no scratch.
#include "decshare_kernels.h"
#include "chacha.h"
#include "ed_access.h"

namespace mkhe {

// ---- share_finish_kernel: grid.x = ChaCha20 blocks of a polynomial (8 coefficients, 64 bytes of a limb per thread), grid.y = the limb rows,
// grid.z = the item, so that the stream is wave-uniform and key and nonce are read from the kernel arguments (scalar loads).  The flooding
// sample never exists in memory: 8 magnitudes and their signs in registers, reduced per limb by one Montgomery product with r1 = 2^64 mod q
// (mont_mul(a, r1) = a mod q for a < 2^62) on the magnitude, the sign folded in afterwards by a select -- no sample-dependent branch.
constexpr int SHF_THREADS = 128;

__global__ void __launch_bounds__(SHF_THREADS) share_finish_kernel(ShareFloodArgs a, u64* __restrict__ out, const u64* __restrict__ acc, const Mod* __restrict__ mods,
                                                                   int limbs, int N) {
    const u32 blk = blockIdx.x * SHF_THREADS + threadIdx.x;                 // block index c: coefficients 8 c .. 8 c + 7
    if (blk >= (u32)(N / 8)) return;
    const int b = blockIdx.z;
    u64 mag[8];
    u32 neg = 0;                                                            // bit i: sample i is negative
#pragma unroll
    for (int i = 0; i < 8; ++i) mag[i] = 0;
    if (a.bits > 0) {
        const u32 in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, a.key[0], a.key[1], a.key[2], a.key[3],
                            a.key[4],    a.key[5],    a.key[6],    a.key[7],    blk,      a.nonce_lo, a.nonce_hi, (u32)b};
        u32 x[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) x[i] = in[i];
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            chacha_qr(x[0], x[4], x[8], x[12]); chacha_qr(x[1], x[5], x[9], x[13]); chacha_qr(x[2], x[6], x[10], x[14]); chacha_qr(x[3], x[7], x[11], x[15]);
            chacha_qr(x[0], x[5], x[10], x[15]); chacha_qr(x[1], x[6], x[11], x[12]); chacha_qr(x[2], x[7], x[8], x[13]); chacha_qr(x[3], x[4], x[9], x[14]);
        }
        const int sh = 64 - a.bits;
        const i64 half = (i64)1 << (a.bits - 1);
#pragma unroll
        for (int i = 0; i < 8; ++i) {                                       // kind 2: e = (r >> (64 - bits)) - 2^(bits-1)
            const u64 r = (u64)(x[2 * i] + in[2 * i]) | ((u64)(x[2 * i + 1] + in[2 * i + 1]) << 32);
            const i64 e = (i64)(r >> sh) - half;
            const i64 s = e >> 63;
            mag[i] = (u64)((e ^ s) - s);
            neg |= (u32)(s & 1) << i;
        }
    }
    for (int j = blockIdx.y; j < limbs; j += gridDim.y) {
        const Mod md = mods[j];
        const u64 q = md.q;
        const long row = (((long)b * limbs + j) * N) / 2 + 4 * (long)blk;  // in pairs
        const u64x2 v0 = ld2(acc, row), v1 = ld2(acc, row + 1), v2 = ld2(acc, row + 2), v3 = ld2(acc, row + 3);
        const u64 v[8] = {v0.x, v0.y, v1.x, v1.y, v2.x, v2.y, v3.x, v3.y};
        u64 o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const u64 m = mont_mul(mag[i], md.r1, q, md.ninv32);            // |e| mod q
            const u64 em = ((neg >> i) & 1) ? csub(q - m, q) : m;           // e mod q
            o[i] = csub(v[i] + em, q);
        }
        st2(out, row, o[0], o[1]); st2(out, row + 1, o[2], o[3]); st2(out, row + 2, o[4], o[5]); st2(out, row + 3, o[6], o[7]);
    }
}
void launch_share_finish(const ShareFloodArgs& a, int count, u64* out, const u64* acc, const Mod* mods, int limbs, int rows, int N, hipStream_t st) {
    const int bx = (N / 8 + SHF_THREADS - 1) / SHF_THREADS;
    hipLaunchKernelGGL(share_finish_kernel, dim3(bx, rows < 1 ? 1 : (rows > limbs ? limbs : rows), count), dim3(SHF_THREADS), 0, st, a, out, acc, mods, limbs, N);
}

// ---- share_merge_kernel: the shape of decrypt_finish_kernel with nshares addends
__global__ void __launch_bounds__(ED_THREADS) share_merge_kernel(int nshares, u64* pt, EdTable c0, EdTable sh, const Mod* mods, int limbs, int N) {
    const int j = blockIdx.y, b = blockIdx.z;
    const u64 q = mods[j].q;
    const long half = N / 2;
    const long row = ((long)b * limbs + j) * half;                          // in pairs: the limb inside a [count][limbs][N] buffer
    const u64* c = ed_entry(c0, b) + (long)j * N;
    for (long n = (long)blockIdx.x * ED_THREADS + threadIdx.x; n < half; n += (long)gridDim.x * ED_THREADS) {
        const u64x2 x = ld2(c, n);
        u64 vx = csub(csub(x.x, q), q), vy = csub(csub(x.y, q), q);
        for (int i = 0; i < nshares; ++i) {
            const u64x2 s = ld2(ed_entry(sh, i), row + n);
            vx = csub(vx + s.x, q);
            vy = csub(vy + s.y, q);
        }
        st2(pt, row + n, vx, vy);
    }
}
void launch_share_merge(int count, int nshares, u64* pt, const EdTable& c0, const EdTable& sh, const Mod* mods, int limbs, int N, hipStream_t st) {
    hipLaunchKernelGGL(share_merge_kernel, dim3(ed_bx(N), limbs, count), dim3(ED_THREADS), 0, st, nshares, pt, c0, sh, mods, limbs, N);
}

}  // namespace mkhe
