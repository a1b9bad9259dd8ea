// modraise_kernels.hip -- see modraise_kernels.h.  No LDS, no scratch, no table.
#include "modraise_kernels.h"
#include "ed_access.h"
#include "sample_arith.h"

namespace mkhe {

// ---- mod_raise_kernel: the shape of the sampling kernels -- grid.x = the N / 8 rows of 8 coefficients (64 bytes of a limb per thread), grid.y = the
// polynomial -- so that a thread reads its row ONCE and stores it under every modulus out of the same registers; the moduli are wave-uniform.
// |v| <= (q_0 - 1) / 2 < 2^59 is formed once; per modulus one Montgomery product with r1 = 2^64 mod q (mont_mul(a, r1) = a mod q, canonical, for
// any a < 2^62: q_l may be ten bits shorter than q_0) and the sign by a select -- no data-dependent branch.
__global__ void __launch_bounds__(BLK_THREADS) mod_raise_kernel(u64* __restrict__ out, const u64* __restrict__ in, const Mod* __restrict__ mods, int lout, int N) {
    const u32 blk = blockIdx.x * BLK_THREADS + threadIdx.x;                 // row index: coefficients 8 blk .. 8 blk + 7
    if (blk >= (u32)(N / 8)) return;
    const int p = blockIdx.y;
    const u64 q0 = mods[0].q, half = (q0 - 1) >> 1;
    u64 x[8], mag[8];
    u32 neg = 0;                                                            // bit i: v[i] is negative
    ld8(in, ((long)p * N) / 2 + 4 * (long)blk, x);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const bool n = x[i] > half;
        mag[i] = n ? q0 - x[i] : x[i];
        neg |= (u32)n << i;
    }
    const long row0 = ((long)p * lout * N) / 2 + 4 * (long)blk;             // in pairs
    st8(out, row0, x);
    for (int j = 1; j < lout; ++j) {
        const Mod md = mods[j];
        u64 v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = signed_mod_q(mont_mul(mag[i], md.r1, md.q, md.ninv32), (neg >> i) & 1, md.q);
        st8(out, row0 + (long)j * (N / 2), v);
    }
}
void launch_mod_raise(int polys, u64* out, const u64* in, const Mod* mods, int lout, int N, hipStream_t st) {
    hipLaunchKernelGGL(mod_raise_kernel, dim3(blk_bx(N), polys), dim3(BLK_THREADS), 0, st, out, in, mods, lout, N);
}

}  // namespace mkhe
