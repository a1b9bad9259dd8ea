// ckks_kernels.hip -- see ckks_kernels.h.
#include "ckks_kernels.h"

namespace mkhe {

typedef double2 cplx;
__device__ __forceinline__ cplx cmul(cplx a, cplx w) { return cplx{a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x}; }
__device__ __forceinline__ cplx cmulc(cplx a, cplx w) { return cplx{a.x * w.x + a.y * w.y, a.y * w.x - a.x * w.y}; }      // a * conj(w)
// decimation in frequency: (a, b) <- (a + b, (a - b) w); decimation in time with the conjugate twiddle undoes it up to the factor 2
template <bool INV> __device__ __forceinline__ void bfly(cplx& a, cplx& b, cplx w) {
    if (INV) { const cplx t = cmulc(b, w); b = cplx{a.x - t.x, a.y - t.y}; a = cplx{a.x + t.x, a.y + t.y}; }
    else { const cplx t = cplx{a.x - b.x, a.y - b.y}; a = cplx{a.x + b.x, a.y + b.y}; b = cmul(t, w); }
}
// slot permutation of chunk c (ckks_kernels.h, LDS layout)
__device__ __forceinline__ int swzc(int c) { c &= 15; return c ^ ((c & 4) << 1); }
__device__ __forceinline__ int swz(int l) { return l ^ swzc(l >> 4); }

// where the elements of a tile sit in the transform, and the twiddle of a butterfly
struct CkGeom {
    int logn, a_log, cc_log, tile, logt;
    // global index of local element l: contiguous tile: tile * T + l; column tile: l = r * Cc + c -> r * B + tile * Cc + c (B = n >> a_log)
    __device__ __forceinline__ int g(int l) const {
        if (!a_log) return (tile << logt) + l;
        return ((l >> cc_log) << (logn - a_log)) + (tile << cc_log) + (l & ((1 << cc_log) - 1));
    }
    // the stage whose butterflies pair local elements 2^logh apart pairs global elements H = 2^logH apart; its twiddle at global index g is
    // omega^((g mod H) * n / 2H)
    __device__ __forceinline__ int tw(int l, int logh) const {
        const int logH = a_log ? logh - cc_log + logn - a_log : logh;
        return (g(l) & ((1 << logH) - 1)) << (logn - 1 - logH);
    }
};

// one stage on the tile in LDS: every thread takes butterflies of adjacent first elements
template <bool INV> __device__ __forceinline__ void stage2(cplx* s, const cplx* __restrict__ w, const CkGeom& ge, int logh) {
    const int h = 1 << logh, T = 1 << ge.logt;
    for (int u = threadIdx.x; u < T / 2; u += blockDim.x) {
        const int i = ((u >> logh) << (logh + 1)) | (u & (h - 1));
        cplx a = s[swz(i)], b = s[swz(i + h)];
        bfly<INV>(a, b, w[ge.tw(i, logh)]);
        s[swz(i)] = a; s[swz(i + h)] = b;
    }
}
// the stages 2^(lq+1) and 2^lq in one pass over the tile (forward: in this order; inverse: the other way round): the same operations
// as two stage2 calls on the four elements i + {0, 1, 2, 3} * 2^lq
template <bool INV> __device__ __forceinline__ void stage4(cplx* s, const cplx* __restrict__ w, const CkGeom& ge, int lq) {
    const int hq = 1 << lq, T = 1 << ge.logt;
    for (int u = threadIdx.x; u < T / 4; u += blockDim.x) {
        const int i = ((u >> lq) << (lq + 2)) | (u & (hq - 1));
        cplx x0 = s[swz(i)], x1 = s[swz(i + hq)], x2 = s[swz(i + 2 * hq)], x3 = s[swz(i + 3 * hq)];
        const cplx wa = w[ge.tw(i, lq + 1)], wb = w[ge.tw(i + hq, lq + 1)], wc = w[ge.tw(i, lq)];
        if (INV) { bfly<INV>(x0, x1, wc); bfly<INV>(x2, x3, wc); bfly<INV>(x0, x2, wa); bfly<INV>(x1, x3, wb); }
        else { bfly<INV>(x0, x2, wa); bfly<INV>(x1, x3, wb); bfly<INV>(x0, x1, wc); bfly<INV>(x2, x3, wc); }
        s[swz(i)] = x0; s[swz(i + hq)] = x1; s[swz(i + 2 * hq)] = x2; s[swz(i + 3 * hq)] = x3;
    }
}
// the stages 8, 4, 2, 1 of a contiguous tile on 16 adjacent elements per thread, in registers.  Their twiddles are the 16th roots
// omega^(m n / 16), the same for every chunk.
template <bool INV> __device__ __forceinline__ void tail16(cplx* s, const cplx* __restrict__ w, int logn, int logt) {
    cplx r16[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) r16[m] = w[m << (logn - 4)];
    for (int c = threadIdx.x; c < (1 << (logt - 4)); c += blockDim.x) {
        cplx x[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) x[k] = s[16 * c + (k ^ swzc(c))];
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const int h = INV ? 1 << st : 8 >> st;
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (!(e & h)) bfly<INV>(x[e], x[e + h], r16[(e & (h - 1)) * (8 / h)]);
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) s[16 * c + (k ^ swzc(c))] = x[k];
    }
}

template <bool INV> __global__ void __launch_bounds__(1024) ck_fft_kernel(CkFft a) {
    extern __shared__ double2 s[];
    const int n = 1 << a.logn, T = 1 << a.logt, b = blockIdx.y;
    CkGeom ge{a.logn, a.a_log, a.logt - a.a_log, (int)blockIdx.x, a.logt};
    const cplx* work = a.work + (long)b * n;
    // ---- load, two adjacent elements per step (one 16-byte access per array)
    for (int l = 2 * threadIdx.x; l < T; l += 2 * blockDim.x) {
        const int g = ge.g(l);
        cplx v0, v1;
        if (!a.first) { v0 = work[g]; v1 = work[g + 1]; }
        else if (INV) {
            const cplx* z = reinterpret_cast<const cplx*>(a.in) + (long)b * n;
            v0 = z[a.pos[g]]; v1 = z[a.pos[g + 1]];
        } else {
            const double* m = a.in + (long)b * 2 * n + g;
            const double2 lo = *reinterpret_cast<const double2*>(m), hi = *reinterpret_cast<const double2*>(m + n);
            v0 = cmul(cplx{lo.x, hi.x}, a.twist[g]); v1 = cmul(cplx{lo.y, hi.y}, a.twist[g + 1]);
        }
        s[swz(l)] = v0; s[swz(l + 1)] = v1;
    }
    __syncthreads();
    // ---- stages.  A contiguous tile has the local spans T/2 .. 1, the last four of them in tail16; a column tile the spans T/2 .. Cc.
    const int lo_log = a.a_log ? ge.cc_log : 4, hi_log = a.logt - 1;      // head stages lo_log .. hi_log
    const int odd = (hi_log - lo_log + 1) & 1;
    if (!INV) {
        int lh = hi_log;
        if (odd) { stage2<INV>(s, a.w, ge, lh); __syncthreads(); --lh; }
        for (; lh > lo_log; lh -= 2) { stage4<INV>(s, a.w, ge, lh - 1); __syncthreads(); }
        if (!a.a_log) { tail16<INV>(s, a.w, a.logn, a.logt); __syncthreads(); }
    } else {
        if (!a.a_log) { tail16<INV>(s, a.w, a.logn, a.logt); __syncthreads(); }
        int lh = lo_log;
        for (; lh + 1 <= hi_log; lh += 2) { stage4<INV>(s, a.w, ge, lh); __syncthreads(); }
        if (odd) { stage2<INV>(s, a.w, ge, hi_log); __syncthreads(); }
    }
    // ---- store
    cplx* wout = a.work + (long)b * n;
    const double invn = 1.0 / (double)n;
    for (int l = 2 * threadIdx.x; l < T; l += 2 * blockDim.x) {
        const int g = ge.g(l);
        const cplx v0 = s[swz(l)], v1 = s[swz(l + 1)];
        if (!a.last) { wout[g] = v0; wout[g + 1] = v1; }
        else if (INV) {
            const cplx c0 = cmulc(v0, a.twist[g]), c1 = cmulc(v1, a.twist[g + 1]);
            double* m = a.out + (long)b * 2 * n + g;
            *reinterpret_cast<double2*>(m) = double2{c0.x * invn, c1.x * invn};
            *reinterpret_cast<double2*>(m + n) = double2{c0.y * invn, c1.y * invn};
        } else {
            cplx* z = reinterpret_cast<cplx*>(a.out) + (long)b * n;
            z[a.pos[g]] = v0; z[a.pos[g + 1]] = v1;
        }
    }
}

bool ck_fft_big_lds() {
    const int bytes = (int)sizeof(double2) << CK_TILE_LOG_BIG;
    const hipError_t e0 = hipFuncSetAttribute(reinterpret_cast<const void*>(&ck_fft_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    const hipError_t e1 = hipFuncSetAttribute(reinterpret_cast<const void*>(&ck_fft_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e0 == hipSuccess && e1 == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}

void launch_ck_fft(bool inverse, const CkFft& a, int count, hipStream_t st) {
    const int T = 1 << a.logt;
    int threads = T / 8;
    threads = threads < 64 ? 64 : threads > 1024 ? 1024 : threads;
    const dim3 grid(1 << (a.logn - a.logt), count);
    const size_t lds = sizeof(double2) * (size_t)T;
    if (inverse) hipLaunchKernelGGL(ck_fft_kernel<true>, grid, dim3(threads), lds, st, a);
    else hipLaunchKernelGGL(ck_fft_kernel<false>, grid, dim3(threads), lds, st, a);
}

constexpr int CK_THREADS = 256;

__global__ void __launch_bounds__(CK_THREADS) ck_scale_up_kernel(const double* coeffs, double scale, u64* pt, const Mod* mods, int limbs, int N) {
    const int n = blockIdx.x * CK_THREADS + threadIdx.x, b = blockIdx.y;
    if (n >= N) return;
    const double r = rint(coeffs[(long)b * N + n] * scale), mag = fabs(r);
    const bool neg = r < 0.0;
    // |r| = a * 2^e with a < 2^62
    u64 a;
    int e = 0;
    if (mag < 0x1p62) a = (u64)mag;
    else {
        const u64 bits = (u64)__double_as_longlong(mag);
        a = (bits & ((1ull << 52) - 1)) | (1ull << 52);
        e = (int)((bits >> 52) & 0x7ff) - 1075;
    }
    for (int l = 0; l < limbs; ++l) {
        const Mod md = mods[l];
        u64 w = md.r1;                                   // MForm(2^e): MRed(a, w) = a * 2^e mod q
        if (e) {
            u64 base = csub(2 * md.r1, md.q);
            for (int k = e; k; k >>= 1) {
                if (k & 1) w = mont_mul(w, base, md.q, md.ninv32);
                base = mont_mul(base, base, md.q, md.ninv32);
            }
        }
        const u64 v = mont_mul(a, w, md.q, md.ninv32);
        pt[((long)b * limbs + l) * N + n] = (neg && v) ? md.q - v : v;
    }
}
void launch_ck_scale_up(int count, const double* coeffs, double scale, u64* pt, const Mod* mods, int limbs, int N, hipStream_t st) {
    hipLaunchKernelGGL(ck_scale_up_kernel, dim3((N + CK_THREADS - 1) / CK_THREADS, count), dim3(CK_THREADS), 0, st, coeffs, scale, pt, mods, limbs, N);
}

__global__ void __launch_bounds__(CK_THREADS) ck_scale_down_kernel(const u64* pt, double scale, double* coeffs, u64* dig, const u64* garner, int nq,
                                                                   const Mod* mods, int limbs, int N) {
    const int n = blockIdx.x * CK_THREADS + threadIdx.x, b = blockIdx.y;
    if (n >= N) return;
    const u64* x = pt + (long)b * limbs * N + n;
    u64* d = dig + (long)b * limbs * N + n;
    // d_j = (..((x_j - d_0) q_0^-1 - d_1) q_1^-1 .. - d_(j-1)) q_(j-1)^-1 mod q_j
    for (int j = 0; j < limbs; ++j) {
        const Mod md = mods[j];
        u64 t = x[(long)j * N];
        for (int i = 0; i < j; ++i) {
            const u64 di = mont_mul(d[(long)i * N], md.r1, md.q, md.ninv32);              // d_i mod q_j
            t = mont_mul(t >= di ? t - di : t + md.q - di, garner[i * nq + j], md.q, md.ninv32);
        }
        d[(long)j * N] = t;
    }
    bool neg = false;
    for (int i = limbs - 1; i >= 0; --i) {
        const u64 di = d[(long)i * N], oi = mods[i].q - 1 - di;
        if (di != oi) { neg = di > oi; break; }
    }
    double acc = 0.0;
    for (int i = limbs - 1; i >= 0; --i) {
        const u64 q = mods[i].q, di = d[(long)i * N];
        acc = acc * (double)q + (double)(neg ? q - 1 - di : di);
    }
    if (neg) acc += 1.0;
    const double v = acc / scale;
    coeffs[(long)b * N + n] = neg ? -v : v;
}
void launch_ck_scale_down(int count, const u64* pt, double scale, double* coeffs, u64* dig, const u64* garner, int nq, const Mod* mods, int limbs, int N,
                          hipStream_t st) {
    hipLaunchKernelGGL(ck_scale_down_kernel, dim3((N + CK_THREADS - 1) / CK_THREADS, count), dim3(CK_THREADS), 0, st, pt, scale, coeffs, dig, garner, nq,
                       mods, limbs, N);
}

}  // namespace mkhe
