// threshold_kernels.hip -- see threshold_kernels.h.  No LDS, no scratch.
#include "threshold_kernels.h"
#include "sample_arith.h"

namespace mkhe {

// ---- threshold_share_kernel: grid.x = ChaCha20 blocks of a row (8 coefficients per thread), grid.y = the row, grid.z = the group of G points, so that
// the streams, m_j and the points are wave-uniform and key, nonce, points and output pointers are read from the kernel arguments (scalar loads).
// A group re-expands the keystream: 2 (t - 1) blocks per thread whatever G is, against 8 G live 64-bit accumulators.  The last group may be short:
// its spare lanes of the group repeat point n - 1 (no branch in the arithmetic) and store nothing.
template <int G>
__global__ void __launch_bounds__(BLK_THREADS) threshold_share_kernel(ThresholdShareArgs a, const u64* __restrict__ sk, const Mod* __restrict__ mods, int N) {
    const u32 blk = blockIdx.x * BLK_THREADS + threadIdx.x;                 // block index c: coefficients 8 c .. 8 c + 7
    if (blk >= (u32)(N / 8)) return;
    const int j = blockIdx.y, g0 = blockIdx.z * G;
    const u32 R = gridDim.y;
    const Mod md = mods[j];
    const u64 q = md.q;
    u64 X[G];                                                               // MForm(x_p): x_p < 2^32, below q
#pragma unroll
    for (int p = 0; p < G; ++p) X[p] = mont_mul(a.x[min(g0 + p, a.n - 1)], md.r2, q, md.ninv32);
    u64 acc[G][8];
#pragma unroll
    for (int p = 0; p < G; ++p)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[p][i] = 0;
#pragma unroll 1
    for (int k = a.t - 1; k >= 1; --k) {                                    // (wave-uniform)
        u64 c[8];
        uniform_mod_q8(a, blk, 2u * ((u32)(k - 1) * R + (u32)j), q, c);
#pragma unroll
        for (int p = 0; p < G; ++p)
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[p][i] = csub(mont_mul(acc[p][i], X[p], q, md.ninv32) + c[i], q);
    }
    u64 s[8];
    ld8(sk + (long)j * N, 4 * (long)blk, s);
#pragma unroll
    for (int p = 0; p < G; ++p) {
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[p][i] = csub(mont_mul(acc[p][i], X[p], q, md.ninv32) + s[i], q);
        if (g0 + p < a.n) st8(a.out[g0 + p] + (long)j * N, 4 * (long)blk, acc[p]);       // (wave-uniform)
    }
}
void launch_threshold_share(const ThresholdShareArgs& a, const u64* sk, const Mod* mods, int rows, int N, hipStream_t st) {
    hipLaunchKernelGGL(threshold_share_kernel<THR_G>, dim3(blk_bx(N), rows, (a.n + THR_G - 1) / THR_G), dim3(BLK_THREADS), 0, st, a, sk, mods, N);
}

// ---- threshold_scale_kernel: streaming shape (256 threads, grid.x strides over pairs, grid.y = row); lambda_j from the kernel arguments
__global__ void __launch_bounds__(ED_THREADS) threshold_scale_kernel(ThresholdScaleArgs a, u64* out, const u64* share, const Mod* __restrict__ mods, int N) {
    const int j = blockIdx.y;
    const Mod md = mods[j];
    const u64 q = md.q, lam = a.lam[j];
    const long half = N / 2, row = (long)j * half;                          // in pairs
    for (long n = (long)blockIdx.x * ED_THREADS + threadIdx.x; n < half; n += (long)gridDim.x * ED_THREADS) {
        const u64x2 v = ld2(share, row + n);
        st2(out, row + n, mont_mul(v.x, lam, q, md.ninv32), mont_mul(v.y, lam, q, md.ninv32));
    }
}
void launch_threshold_scale(const ThresholdScaleArgs& a, u64* out, const u64* share, const Mod* mods, int rows, int N, hipStream_t st) {
    hipLaunchKernelGGL(threshold_scale_kernel, dim3(ed_bx(N), rows), dim3(ED_THREADS), 0, st, a, out, share, mods, N);
}

// ---- limbs_sum_kernel: streaming shape (grid.y = limb, grid.z = item); sum_shares on nothing but the sources
__global__ void __launch_bounds__(ED_THREADS) limbs_sum_kernel(int nsrc, EdTable src, u64* dst, const Mod* __restrict__ mods, int limbs, int N) {
    const int j = blockIdx.y, b = blockIdx.z;
    const u64 q = mods[j].q;
    const long half = N / 2, row = ((long)b * limbs + j) * half;            // in pairs
    for (long n = (long)blockIdx.x * ED_THREADS + threadIdx.x; n < half; n += (long)gridDim.x * ED_THREADS) {
        const u64x2 v = sum_shares(u64x2{0, 0}, src, nsrc, row + n, q);
        st2(dst, row + n, v.x, v.y);
    }
}
void launch_limbs_sum(int count, int limbs, int nsrc, const EdTable& src, u64* dst, const Mod* mods, int N, hipStream_t st) {
    hipLaunchKernelGGL(limbs_sum_kernel, dim3(ed_bx(N), limbs, count), dim3(ED_THREADS), 0, st, nsrc, src, dst, mods, limbs, N);
}

}  // namespace mkhe
