// encdec_kernels.hip -- see encdec_kernels.h.  Streaming kernels: 256 threads, grid.x strides over PAIRS of coefficients (one 16-byte
// access per lane), grid.y = limb, grid.z = item of the batch; per-modulus constants are wave-uniform (SGPRs).  No LDS.
#include "sample_arith.h"

namespace mkhe {

__global__ void __launch_bounds__(ED_THREADS) encrypt_mul_kernel(int count, u64* w, const u64* pk, const u64* pt_ntt, const Mod* mods, int limbs,
                                                                 int mtot, int N) {
    const int j = blockIdx.y, b = blockIdx.z;
    const Mod md = mods[j];
    const u64 q = md.q;
    const long half = N / 2, slot = (long)count * limbs * half;          // in pairs
    const long row = ((long)b * limbs + j) * half;
    const u64* pk0 = pk + (long)j * N;
    const u64* pk1 = pk + ((long)mtot + j) * N;
    for (long n = (long)blockIdx.x * ED_THREADS + threadIdx.x; n < half; n += (long)gridDim.x * ED_THREADS) {
        const u64x2 uh = ld2(w, 2 * slot + row + n), a0 = ld2(pk0, n), a1 = ld2(pk1, n);
        const u64 Ux = mont_mul(uh.x, md.r2, q, md.ninv32), Uy = mont_mul(uh.y, md.r2, q, md.ninv32);       // MForm
        st2(w, row + n, mont_mul(Ux, a0.x, q, md.ninv32), mont_mul(Uy, a0.y, q, md.ninv32));
        st2(w, slot + row + n, mont_mul(Ux, a1.x, q, md.ninv32), mont_mul(Uy, a1.y, q, md.ninv32));
        if (pt_ntt) { const u64x2 p = ld2(pt_ntt, row + n); st2(w, 2 * slot + row + n, p.x, p.y); }
        else st2(w, 2 * slot + row + n, 0, 0);
    }
}
void launch_encrypt_mul(int count, u64* w, const u64* pk, const u64* pt_ntt, const Mod* mods, int limbs, int mtot, int N, hipStream_t st) {
    hipLaunchKernelGGL(encrypt_mul_kernel, dim3(ed_bx(N), limbs, count), dim3(ED_THREADS), 0, st, count, w, pk, pt_ntt, mods, limbs, mtot, N);
}

__global__ void __launch_bounds__(ED_THREADS) encrypt_finish_kernel(int count, EdTable out, const u64* w, const i32* smp, const u64* pt_coeff,
                                                                    const Mod* mods, int limbs, int N) {
    const int j = blockIdx.y, b = blockIdx.z;
    const u64 q = mods[j].q;
    const long half = N / 2, slot = (long)count * limbs * half;
    const long row = ((long)b * limbs + j) * half;
    const u64* pt = pt_coeff ? pt_coeff : w + 4 * slot;                    // w[2] in words
    const int2* e0 = reinterpret_cast<const int2*>(smp + ((long)b * 3 + 1) * N);
    const int2* e1 = reinterpret_cast<const int2*>(smp + ((long)b * 3 + 2) * N);
    u64* ct = const_cast<u64*>(ed_entry(out, b));
    u64* c0 = ct + (long)j * N;
    u64* c1 = ct + ((long)limbs + j) * N;
    for (long n = (long)blockIdx.x * ED_THREADS + threadIdx.x; n < half; n += (long)gridDim.x * ED_THREADS) {
        const u64x2 t0 = ld2(w, row + n), t1 = ld2(w, slot + row + n), p = ld2(pt, row + n);
        const int2 s0 = e0[n], s1 = e1[n];
        st2(c0, n, csub(csub(t0.x + small_q(s0.x, q), q) + p.x, q), csub(csub(t0.y + small_q(s0.y, q), q) + p.y, q));
        st2(c1, n, csub(t1.x + small_q(s1.x, q), q), csub(t1.y + small_q(s1.y, q), q));
    }
}
void launch_encrypt_finish(int count, const EdTable& out, const u64* w, const i32* smp, const u64* pt_coeff, const Mod* mods, int limbs, int N, hipStream_t st) {
    hipLaunchKernelGGL(encrypt_finish_kernel, dim3(ed_bx(N), limbs, count), dim3(ED_THREADS), 0, st, count, out, w, smp, pt_coeff, mods, limbs, N);
}

__global__ void __launch_bounds__(ED_THREADS) decrypt_mac_kernel(int k, u64* acc, EdTable ch, EdTable sk, const Mod* mods, int limbs, int N) {
    const int j = blockIdx.y, b = blockIdx.z;
    const Mod md = mods[j];
    const long half = N / 2;
    u64* dst = acc + ((long)b * limbs + j) * N;
    for (long n = (long)blockIdx.x * ED_THREADS + threadIdx.x; n < half; n += (long)gridDim.x * ED_THREADS) {
        u64 hx = 0, lx = 0, hy = 0, ly = 0;
        for (int i = 0; i < k; ++i) {
            const u64x2 c = ld2(ed_entry(ch, b * k + i) + (long)j * N, n), s = ld2(ed_entry(sk, b * k + i) + (long)j * N, n);
            mac128(c.x, s.x, hx, lx);
            mac128(c.y, s.y, hy, ly);
        }
        st2(dst, n, redc128(hx, lx, md), redc128(hy, ly, md));
    }
}
void launch_decrypt_mac(int count, int k, u64* acc, const EdTable& ch, const EdTable& sk, const Mod* mods, int limbs, int N, hipStream_t st) {
    hipLaunchKernelGGL(decrypt_mac_kernel, dim3(ed_bx(N), limbs, count), dim3(ED_THREADS), 0, st, k, acc, ch, sk, mods, limbs, N);
}

__global__ void __launch_bounds__(ED_THREADS) decrypt_finish_kernel(u64* out, long out_stride, const u64* c0, long c0_stride, const u64* acc,
                                                                    const Mod* mods, int limbs, int N, int reduce) {
    const int j = blockIdx.y, b = blockIdx.z;
    const u64 q = mods[j].q;
    const long half = N / 2;
    const u64* a = acc + ((long)b * limbs + j) * N;
    const u64* c = c0 + b * c0_stride + (long)j * N;
    u64* o = out + b * out_stride + (long)j * N;
    for (long n = (long)blockIdx.x * ED_THREADS + threadIdx.x; n < half; n += (long)gridDim.x * ED_THREADS) {
        const u64x2 x = ld2(c, n), y = ld2(a, n);
        u64 vx = csub(x.x + y.x, q), vy = csub(x.y + y.y, q);
        if (reduce) { vx = csub(csub(vx, q), q); vy = csub(csub(vy, q), q); }
        st2(o, n, vx, vy);
    }
}
void launch_decrypt_finish(int count, u64* out, long out_stride, const u64* c0, long c0_stride, const u64* acc, const Mod* mods, int limbs, int N,
                           bool reduce, hipStream_t st) {
    hipLaunchKernelGGL(decrypt_finish_kernel, dim3(ed_bx(N), limbs, count), dim3(ED_THREADS), 0, st, out, out_stride, c0, c0_stride, acc, mods, limbs, N,
                       reduce ? 1 : 0);
}

// ---- small_sample_kernel: one thread = one ChaCha20 block (RFC 8439 section 2.3) = 8 coefficients = 32 bytes of int32.  Integer ALU work
// (20 rounds of 16 add / xor / rotate, then ncdt 64-bit compares per coefficient for a table); no LDS, no scratch, two 16-byte stores.
// grid.x = blocks of a polynomial, grid.y strides over the polynomials: stream, kind and the table are wave-uniform, the table and the
// key are read from the kernel arguments (scalar loads).
constexpr int SMP_MAX_GRID_Y = 65535;

__global__ void __launch_bounds__(BLK_THREADS) small_sample_kernel(SmallSampleArgs a, int kind, int polys, i32* out, i32* u_rows, int N) {
    const u32 blk = blockIdx.x * BLK_THREADS + threadIdx.x;                 // block index c: coefficients 8 c .. 8 c + 7
    if (blk >= (u32)(N / 8)) return;
    for (int p = blockIdx.y; p < polys; p += gridDim.y) {
        const int k = kind == SMP_KIND_ENCRYPT ? (p % 3 != 0) : kind;
        u64 r64[8];
        chacha_block8(a, blk, a.first_stream + (u32)p, r64);
        i32 v[8];
        if (k == 0) {                                                       // ternary, P(0) = 1/2
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = (r64[i] & 1) ? 0 : ((r64[i] & 2) ? 1 : -1);
        } else {
            cdt_sample8(a, r64, v);
        }
        st8(out + (long)p * N, 2 * (long)blk, v);
        if (u_rows && kind == SMP_KIND_ENCRYPT && k == 0) st8(u_rows + (long)(p / 3) * N, 2 * (long)blk, v);
    }
}
void launch_small_sample(const SmallSampleArgs& a, int kind, int polys, i32* out, i32* u_rows, int N, hipStream_t st) {
    hipLaunchKernelGGL(small_sample_kernel, dim3(blk_bx(N), polys < SMP_MAX_GRID_Y ? polys : SMP_MAX_GRID_Y), dim3(BLK_THREADS), 0, st, a, kind, polys,
                       out, u_rows, N);
}

}  // namespace mkhe
