// skenc_kernels.hip -- see skenc_kernels.h.  No LDS, no scratch.
#include "skenc_kernels.h"
#include "sample_arith.h"

namespace mkhe {

// ---- uniform_sample_kernel: grid.x = ChaCha20 blocks of a row (8 coefficients, 64 bytes per thread), grid.y = the limb, grid.z = the item, so
// that both streams and q_j are wave-uniform and key and nonce are read from the kernel arguments (scalar loads).  Per coefficient
// ((hi 2^64 + lo) q) >> 128 = (hi q + ((lo q) >> 64)) >> 64: one full 64 x 64 product, the high word of a second and a carry.
__global__ void __launch_bounds__(BLK_THREADS) uniform_sample_kernel(UniformArgs a, EdTable out, long poly_off, const Mod* __restrict__ mods, int nq, int N) {
    const u32 blk = blockIdx.x * BLK_THREADS + threadIdx.x;                 // block index c: coefficients 8 c .. 8 c + 7
    if (blk >= (u32)(N / 8)) return;
    const int j = blockIdx.y, b = blockIdx.z;
    const u64 q = mods[j].q;
    const u32 s0 = 2u * ((u32)b * (u32)nq + (u32)j);
    u64 v[8];
    uniform_mod_q8(a, blk, s0, q, v);                                       // below q: (r q) >> 128 with r < 2^128
    st8(const_cast<u64*>(ed_entry(out, b)) + poly_off + (long)j * N, 4 * (long)blk, v);
}
void launch_uniform_sample(const UniformArgs& a, int count, const EdTable& out, long poly_off, const Mod* mods, int limbs, int nq, int N, hipStream_t st) {
    hipLaunchKernelGGL(uniform_sample_kernel, dim3(blk_bx(N), limbs, count), dim3(BLK_THREADS), 0, st, a, out, poly_off, mods, nq, N);
}

// ---- skenc_mul_kernel: the shape of encrypt_mul_kernel (256 threads, grid.x strides over pairs, grid.y = limb, grid.z = item)
__global__ void __launch_bounds__(ED_THREADS) skenc_mul_kernel(u64* w, const u64* __restrict__ sk, const u64* __restrict__ pt_ntt, const Mod* mods, int limbs, int N) {
    const int j = blockIdx.y, b = blockIdx.z;
    const Mod md = mods[j];
    const u64 q = md.q;
    const long half = N / 2;
    const long row = ((long)b * limbs + j) * half;                          // in pairs
    const u64* s = sk + (long)j * N;
    for (long n = (long)blockIdx.x * ED_THREADS + threadIdx.x; n < half; n += (long)gridDim.x * ED_THREADS) {
        const u64x2 c = ld2(w, row + n), sv = ld2(s, n);
        u64 mx = mont_mul(c.x, sv.x, q, md.ninv32), my = mont_mul(c.y, sv.y, q, md.ninv32);
        if (pt_ntt) {                                                       // (wave-uniform)
            const u64x2 p = ld2(pt_ntt, row + n);
            mx = csub(p.x + q - mx, q);
            my = csub(p.y + q - my, q);
        }
        st2(w, row + n, mx, my);
    }
}
void launch_skenc_mul(int count, u64* w, const u64* sk, const u64* pt_ntt, const Mod* mods, int limbs, int N, hipStream_t st) {
    hipLaunchKernelGGL(skenc_mul_kernel, dim3(ed_bx(N), limbs, count), dim3(ED_THREADS), 0, st, w, sk, pt_ntt, mods, limbs, N);
}

// ---- skenc_finish_kernel: the shape of pcks_finish_kernel with one polynomial.  e from the int32 samples (two 16-byte loads) or kind 1 in
// registers: the table scan (cdt_sample8), then e >= 0 ? e : q - |e| by a select (small_q) -- no sample-dependent branch.
__global__ void __launch_bounds__(BLK_THREADS) skenc_finish_kernel(SmallSampleArgs a, const i32* __restrict__ smp, EdTable out, const u64* __restrict__ w,
                                                                   const u64* __restrict__ pt_coeff, const Mod* __restrict__ mods, int limbs, int N) {
    const u32 blk = blockIdx.x * BLK_THREADS + threadIdx.x;                 // block index c: coefficients 8 c .. 8 c + 7
    if (blk >= (u32)(N / 8)) return;
    const int j = blockIdx.y, b = blockIdx.z;
    const u64 q = mods[j].q;
    i32 e[8];
    if (smp) {                                                              // (wave-uniform)
        ld8(smp + (long)b * N, 2 * (long)blk, e);
    } else {
        u64 r64[8];
        chacha_block8(a, blk, (u32)b, r64);
        cdt_sample8(a, r64, e);
    }
    const long row = (((long)b * limbs + j) * N) / 2 + 4 * (long)blk;       // in pairs: w and pt_coeff [count][limbs][N]
    u64 t[8], o[8];
    ld8(w, row, t);
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = small_q(e[i], q);
    if (pt_coeff) {                                                         // (wave-uniform)
        u64 p[8];
        ld8(pt_coeff, row, p);
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = csub(csub(p[i] + o[i], q) + q - t[i], q);
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = csub(t[i] + o[i], q);
    }
    st8(const_cast<u64*>(ed_entry(out, b)) + (long)j * N, 4 * (long)blk, o);
}
void launch_skenc_finish(const SmallSampleArgs& a, const i32* smp, int count, const EdTable& out, const u64* w, const u64* pt_coeff, const Mod* mods,
                         int limbs, int N, hipStream_t st) {
    hipLaunchKernelGGL(skenc_finish_kernel, dim3(blk_bx(N), limbs, count), dim3(BLK_THREADS), 0, st, a, smp, out, w, pt_coeff, mods, limbs, N);
}

}  // namespace mkhe
