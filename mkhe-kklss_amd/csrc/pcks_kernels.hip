// pcks_kernels.hip -- see pcks_kernels.h.  No LDS, no scratch.
#include "pcks_kernels.h"
#include "sample_arith.h"

namespace mkhe {

// ---- pcks_mac_kernel: the shape of encrypt_mul_kernel (256 threads, grid.x strides over pairs, grid.y = limb, grid.z = item)
__global__ void __launch_bounds__(ED_THREADS) pcks_mac_kernel(int count, u64* w, const u64* __restrict__ sk, const u64* __restrict__ pk, const Mod* mods,
                                                              int limbs, int mtot, int N) {
    const int j = blockIdx.y, b = blockIdx.z;
    const Mod md = mods[j];
    const u64 q = md.q;
    const long half = N / 2, slot = (long)count * limbs * half;          // in pairs
    const long row = ((long)b * limbs + j) * half;
    const u64* s = sk + (long)j * N;
    const u64* pk0 = pk + (long)j * N;
    const u64* pk1 = pk + ((long)mtot + j) * N;
    for (long n = (long)blockIdx.x * ED_THREADS + threadIdx.x; n < half; n += (long)gridDim.x * ED_THREADS) {
        const u64x2 c = ld2(w, row + n), uh = ld2(w, 2 * slot + row + n), sv = ld2(s, n), a0 = ld2(pk0, n), a1 = ld2(pk1, n);
        const u64 Ux = mont_mul(uh.x, md.r2, q, md.ninv32), Uy = mont_mul(uh.y, md.r2, q, md.ninv32);       // MForm
        u64 hx = 0, lx = 0, hy = 0, ly = 0;
        mac128(c.x, sv.x, hx, lx); mac128(Ux, a0.x, hx, lx);
        mac128(c.y, sv.y, hy, ly); mac128(Uy, a0.y, hy, ly);
        st2(w, row + n, redc128(hx, lx, md), redc128(hy, ly, md));
        st2(w, slot + row + n, mont_mul(Ux, a1.x, q, md.ninv32), mont_mul(Uy, a1.y, q, md.ninv32));
        st2(w, 2 * slot + row + n, 0, 0);
    }
}
void launch_pcks_mac(int count, u64* w, const u64* sk, const u64* pk, const Mod* mods, int limbs, int mtot, int N, hipStream_t st) {
    hipLaunchKernelGGL(pcks_mac_kernel, dim3(ed_bx(N), limbs, count), dim3(ED_THREADS), 0, st, count, w, sk, pk, mods, limbs, mtot, N);
}

// ---- pcks_finish_kernel: grid.x = ChaCha20 blocks of a polynomial (8 coefficients, 64 bytes of a limb per thread), grid.y = the 2 limbs rows,
// grid.z = the item, so that the half, every stream and every per-modulus constant are wave-uniform and key, nonce and table are read from the
// kernel arguments (scalar loads).  h0 rows: the flood by flood_mod_q.  h1 rows: the table scan (cdt_sample8), then e >= 0 ? e : q - |e| by a
// select (small_q) -- no sample-dependent branch.
__global__ void __launch_bounds__(BLK_THREADS) pcks_finish_kernel(SmallSampleArgs a, int flood_bits, int count, u64* __restrict__ shares, const u64* __restrict__ w,
                                                                  const Mod* __restrict__ mods, int limbs, int N) {
    const u32 blk = blockIdx.x * BLK_THREADS + threadIdx.x;                 // block index c: coefficients 8 c .. 8 c + 7
    if (blk >= (u32)(N / 8)) return;
    const int r = blockIdx.y, b = blockIdx.z;
    const int h = r >= limbs ? 1 : 0, j = r - h * limbs;                    // (wave-uniform)
    const Mod md = mods[j];
    const u64 q = md.q;
    u64 f[8];                                                               // what the row adds, mod q_j
    if (h == 0) {
        const int W = (flood_bits + 63) >> 6;
        flood_mod_q(a, blk, 2u * (u32)count + (u32)b * (u32)W, flood_bits, md, f);
    } else {
        u64 r64[8];
        chacha_block8(a, blk, (u32)count + (u32)b, r64);
        i32 e[8];
        cdt_sample8(a, r64, e);
#pragma unroll
        for (int i = 0; i < 8; ++i) f[i] = small_q(e[i], q);
    }
    const long src = ((((long)h * count + b) * limbs + j) * N) / 2 + 4 * (long)blk;        // in pairs: w [2][count][limbs][N]
    const long dst = ((((long)b * 2 + h) * limbs + j) * N) / 2 + 4 * (long)blk;            // shares [count][2][limbs][N]
    u64 v[8];
    ld8(w, src, v);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = csub(v[i] + f[i], q);
    st8(shares, dst, v);
}
void launch_pcks_finish(const SmallSampleArgs& a, int flood_bits, int count, u64* shares, const u64* w, const Mod* mods, int limbs, int N, hipStream_t st) {
    hipLaunchKernelGGL(pcks_finish_kernel, dim3(blk_bx(N), 2 * limbs, count), dim3(BLK_THREADS), 0, st, a, flood_bits, count, shares, w, mods, limbs, N);
}

// ---- pcks_merge_kernel: the shape of share_merge_kernel with 2 limbs rows; c_0 enters the rows of polynomial 0 only
__global__ void __launch_bounds__(ED_THREADS) pcks_merge_kernel(int nshares, EdTable out, EdTable c0, EdTable sh, const Mod* mods, int limbs, int N) {
    const int r = blockIdx.y, b = blockIdx.z;
    const int h = r >= limbs ? 1 : 0, j = r - h * limbs;                    // (wave-uniform)
    const u64 q = mods[j].q;
    const long half = N / 2;
    const long row = ((long)b * 2 * limbs + r) * half;                      // in pairs: row r of item b inside a [count][2][limbs][N] buffer
    const u64* c = ed_entry(c0, b) + (long)j * N;
    u64* o = const_cast<u64*>(ed_entry(out, b)) + (long)r * N;
    for (long n = (long)blockIdx.x * ED_THREADS + threadIdx.x; n < half; n += (long)gridDim.x * ED_THREADS) {
        const u64x2 v = sum_shares(h == 0 ? ld2(c, n) : u64x2{0, 0}, sh, nshares, row + n, q);
        st2(o, n, v.x, v.y);
    }
}
void launch_pcks_merge(int count, int nshares, const EdTable& out, const EdTable& c0, const EdTable& sh, const Mod* mods, int limbs, int N, hipStream_t st) {
    hipLaunchKernelGGL(pcks_merge_kernel, dim3(ed_bx(N), 2 * limbs, count), dim3(ED_THREADS), 0, st, nshares, out, c0, sh, mods, limbs, N);
}

}  // namespace mkhe
