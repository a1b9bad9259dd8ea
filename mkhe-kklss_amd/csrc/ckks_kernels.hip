// ckks_kernels.hip -- see ckks_kernels.h.
#include "ckks_kernels.h"
#include "tile_transform.h"

namespace mkhe {

typedef double2 cplx;
__device__ __forceinline__ cplx cmul(cplx a, cplx w) { return cplx{a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x}; }
__device__ __forceinline__ cplx cmulc(cplx a, cplx w) { return cplx{a.x * w.x + a.y * w.y, a.y * w.x - a.x * w.y}; }      // a * conj(w)
// what tile_transform.h needs to know about the FFT
struct CkTr {
    typedef cplx elem, twid;
    struct ctx {};
    static constexpr int EPT = 8;
    // decimation in frequency: (a, b) <- (a + b, (a - b) w); decimation in time with the conjugate twiddle undoes it up to the factor 2
    template <bool INV> __device__ __forceinline__ static void bfly(cplx& a, cplx& b, cplx w, ctx) {
        if (INV) { const cplx t = cmulc(b, w); b = cplx{a.x - t.x, a.y - t.y}; a = cplx{a.x + t.x, a.y + t.y}; }
        else { const cplx t = cplx{a.x - b.x, a.y - b.y}; a = cplx{a.x + b.x, a.y + b.y}; b = cmul(t, w); }
    }
    // slot permutation of chunk c (ckks_kernels.h, LDS layout)
    __device__ __forceinline__ static int swzc(int c) { c &= 15; return c ^ ((c & 4) << 1); }
    __device__ __forceinline__ static int swz(int l) { return l ^ swzc(l >> 4); }
    __device__ __forceinline__ static void load16(const cplx* s, int c, cplx (&x)[16]) {
#pragma unroll
        for (int k = 0; k < 16; ++k) x[k] = s[16 * c + (k ^ swzc(c))];
    }
    __device__ __forceinline__ static void store16(cplx* s, int c, const cplx (&x)[16]) {
#pragma unroll
        for (int k = 0; k < 16; ++k) s[16 * c + (k ^ swzc(c))] = x[k];
    }
};

template <bool INV> __global__ void __launch_bounds__(1024) ck_fft_kernel(CkFft a) {
    extern __shared__ double2 s[];
    const int n = 1 << a.p.logn, T = 1 << a.p.logt, b = blockIdx.y;
    const TileGeom ge = TileGeom::of(a.p);
    const cplx* work = a.work + (long)b * n;
    // ---- load, two adjacent elements per step (one 16-byte access per array)
    for (int l = 2 * threadIdx.x; l < T; l += 2 * blockDim.x) {
        const int g = ge.g(l);
        cplx v0, v1;
        if (!a.p.first) { v0 = work[g]; v1 = work[g + 1]; }
        else if (INV) {
            const cplx* z = reinterpret_cast<const cplx*>(a.in) + (long)b * n;
            v0 = z[a.pos[g]]; v1 = z[a.pos[g + 1]];
        } else {
            const double* m = a.in + (long)b * 2 * n + g;
            const double2 lo = *reinterpret_cast<const double2*>(m), hi = *reinterpret_cast<const double2*>(m + n);
            v0 = cmul(cplx{lo.x, hi.x}, a.twist[g]); v1 = cmul(cplx{lo.y, hi.y}, a.twist[g + 1]);
        }
        s[CkTr::swz(l)] = v0; s[CkTr::swz(l + 1)] = v1;
    }
    __syncthreads();
    // ---- stages
    tile_stages<INV, CkTr>(s, a.w, a.p, ge, CkTr::ctx{});
    // ---- store
    cplx* wout = a.work + (long)b * n;
    const double invn = 1.0 / (double)n;
    for (int l = 2 * threadIdx.x; l < T; l += 2 * blockDim.x) {
        const int g = ge.g(l);
        const cplx v0 = s[CkTr::swz(l)], v1 = s[CkTr::swz(l + 1)];
        if (!a.p.last) { wout[g] = v0; wout[g + 1] = v1; }
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

bool ck_fft_big_lds() { return tile_request_lds(&ck_fft_kernel<false>, &ck_fft_kernel<true>, (int)sizeof(cplx) << CK_TILE_LOG_BIG); }

void launch_ck_fft(bool inverse, const CkFft& a, int count, hipStream_t st) {
    const TileLaunch l = tile_launch_shape(a.p, count, CkTr::EPT, sizeof(cplx));
    if (inverse) hipLaunchKernelGGL(ck_fft_kernel<true>, l.grid, l.block, l.lds, st, a);
    else hipLaunchKernelGGL(ck_fft_kernel<false>, l.grid, l.block, l.lds, st, a);
}

constexpr int CK_THREADS = 256;

// the residues of r = rint(c * scale) under mods[0 .. limbs) into pt[l * N] (ckks_kernels.h, launch_ck_scale_up)
__device__ __forceinline__ void ck_residues(double c, double scale, u64* pt, const Mod* mods, int limbs, long N) {
    const double r = rint(c * scale), mag = fabs(r);
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
        pt[l * N] = (neg && v) ? md.q - v : v;
    }
}
// (centred lift of the residues x[l * xs]) / scale, through the digits d[l * ds] (ckks_kernels.h, launch_ck_scale_down)
__device__ __forceinline__ double ck_lift(const u64* x, long xs, u64* d, long ds, double scale, const u64* garner, int nq, const Mod* mods, int limbs) {
    garner_digits([&](int j, const Mod&) { return x[j * xs]; }, d, garner, nq, mods, limbs, ds);
    bool neg = false;
    for (int i = limbs - 1; i >= 0; --i) {
        const u64 di = d[i * ds], oi = mods[i].q - 1 - di;
        if (di != oi) { neg = di > oi; break; }
    }
    double acc = 0.0;
    for (int i = limbs - 1; i >= 0; --i) {
        const u64 q = mods[i].q, di = d[i * ds];
        acc = acc * (double)q + (double)(neg ? q - 1 - di : di);
    }
    if (neg) acc += 1.0;
    const double v = acc / scale;
    return neg ? -v : v;
}

__global__ void __launch_bounds__(CK_THREADS) ck_scale_up_kernel(const double* coeffs, double scale, u64* pt, const Mod* mods, int limbs, int N) {
    const int n = blockIdx.x * CK_THREADS + threadIdx.x, b = blockIdx.y;
    if (n >= N) return;
    ck_residues(coeffs[(long)b * N + n], scale, pt + (long)b * limbs * N + n, mods, limbs, N);
}
void launch_ck_scale_up(int count, const double* coeffs, double scale, u64* pt, const Mod* mods, int limbs, int N, hipStream_t st) {
    hipLaunchKernelGGL(ck_scale_up_kernel, dim3((N + CK_THREADS - 1) / CK_THREADS, count), dim3(CK_THREADS), 0, st, coeffs, scale, pt, mods, limbs, N);
}

__global__ void __launch_bounds__(CK_THREADS) ck_scale_down_kernel(const u64* pt, double scale, double* coeffs, u64* dig, const u64* garner, int nq,
                                                                   const Mod* mods, int limbs, int N) {
    const int n = blockIdx.x * CK_THREADS + threadIdx.x, b = blockIdx.y;
    if (n >= N) return;
    coeffs[(long)b * N + n] = ck_lift(pt + (long)b * limbs * N + n, N, dig + (long)b * limbs * N + n, N, scale, garner, nq, mods, limbs);
}
void launch_ck_scale_down(int count, const u64* pt, double scale, double* coeffs, u64* dig, const u64* garner, int nq, const Mod* mods, int limbs, int N,
                          hipStream_t st) {
    hipLaunchKernelGGL(ck_scale_down_kernel, dim3((N + CK_THREADS - 1) / CK_THREADS, count), dim3(CK_THREADS), 0, st, pt, scale, coeffs, dig, garner, nq,
                       mods, limbs, N);
}

// ---- sparse packing: compact [count][M] (M = 2n = N >> gap_log) <-> the grid i = c << gap_log of [count][N]
__global__ void __launch_bounds__(CK_THREADS) ck_sparse_scale_up_kernel(const double* compact, double scale, u64* pt, const Mod* mods, int limbs, int N,
                                                                        int gap_log) {
    const int i = blockIdx.x * CK_THREADS + threadIdx.x, b = blockIdx.y;
    if (i >= N) return;
    u64* col = pt + (long)b * limbs * N + i;
    if (i & ((1 << gap_log) - 1)) {
        for (int l = 0; l < limbs; ++l) col[(long)l * N] = 0;
        return;
    }
    ck_residues(compact[(long)b * (N >> gap_log) + (i >> gap_log)], scale, col, mods, limbs, N);
}
void launch_ck_sparse_scale_up(int count, const double* compact, double scale, u64* pt, const Mod* mods, int limbs, int N, int gap_log, hipStream_t st) {
    hipLaunchKernelGGL(ck_sparse_scale_up_kernel, dim3((N + CK_THREADS - 1) / CK_THREADS, count), dim3(CK_THREADS), 0, st, compact, scale, pt, mods, limbs,
                       N, gap_log);
}
__global__ void __launch_bounds__(CK_THREADS) ck_sparse_scale_down_kernel(const u64* pt, double scale, double* compact, u64* dig, const u64* garner, int nq,
                                                                          const Mod* mods, int limbs, int N, int gap_log) {
    const int M = N >> gap_log, c = blockIdx.x * CK_THREADS + threadIdx.x, b = blockIdx.y;
    if (c >= M) return;
    compact[(long)b * M + c] = ck_lift(pt + (long)b * limbs * N + ((long)c << gap_log), N, dig + (long)b * limbs * M + c, M, scale, garner, nq, mods, limbs);
}
void launch_ck_sparse_scale_down(int count, const u64* pt, double scale, double* compact, u64* dig, const u64* garner, int nq, const Mod* mods, int limbs,
                                 int N, int gap_log, hipStream_t st) {
    const int M = N >> gap_log;
    hipLaunchKernelGGL(ck_sparse_scale_down_kernel, dim3((M + CK_THREADS - 1) / CK_THREADS, count), dim3(CK_THREADS), 0, st, pt, scale, compact, dig, garner,
                       nq, mods, limbs, N, gap_log);
}
__global__ void __launch_bounds__(CK_THREADS) ck_spread_kernel(const double* compact, double* coeffs, int N, int gap_log) {
    const int i = blockIdx.x * CK_THREADS + threadIdx.x, b = blockIdx.y;
    if (i >= N) return;
    coeffs[(long)b * N + i] = (i & ((1 << gap_log) - 1)) ? 0.0 : compact[(long)b * (N >> gap_log) + (i >> gap_log)];
}
void launch_ck_spread(int count, const double* compact, double* coeffs, int N, int gap_log, hipStream_t st) {
    hipLaunchKernelGGL(ck_spread_kernel, dim3((N + CK_THREADS - 1) / CK_THREADS, count), dim3(CK_THREADS), 0, st, compact, coeffs, N, gap_log);
}
__global__ void __launch_bounds__(CK_THREADS) ck_pick_kernel(const double* coeffs, double* compact, int N, int gap_log) {
    const int M = N >> gap_log, c = blockIdx.x * CK_THREADS + threadIdx.x, b = blockIdx.y;
    if (c >= M) return;
    compact[(long)b * M + c] = coeffs[(long)b * N + ((long)c << gap_log)];
}
void launch_ck_pick(int count, const double* coeffs, double* compact, int N, int gap_log, hipStream_t st) {
    const int M = N >> gap_log;
    hipLaunchKernelGGL(ck_pick_kernel, dim3((M + CK_THREADS - 1) / CK_THREADS, count), dim3(CK_THREADS), 0, st, coeffs, compact, N, gap_log);
}

// n < 16 slots: the embedding as a direct sum, one thread per output.  root[j * n + k] = zeta_j^k
template <bool INV> __global__ void __launch_bounds__(CK_THREADS) ck_direct_kernel(const double* in, double* out, const cplx* root, int logn, int count) {
    const int n = 1 << logn, t = blockIdx.x * CK_THREADS + threadIdx.x, b = t >> logn, o = t & (n - 1);
    if (b >= count) return;
    cplx acc{0.0, 0.0};
    if (INV) {              // w_k = (1/n) sum_j z_j conj(zeta_j^k), k = o
        const cplx* z = reinterpret_cast<const cplx*>(in) + (long)b * n;
        for (int j = 0; j < n; ++j) { const cplx v = cmulc(z[j], root[j * n + o]); acc.x += v.x; acc.y += v.y; }
        const double invn = 1.0 / (double)n;
        out[(long)b * 2 * n + o] = acc.x * invn; out[(long)b * 2 * n + n + o] = acc.y * invn;
    } else {                // z_j = sum_k (m_k + i m_(k+n)) zeta_j^k, j = o
        const double* m = in + (long)b * 2 * n;
        for (int k = 0; k < n; ++k) { const cplx v = cmul(cplx{m[k], m[k + n]}, root[o * n + k]); acc.x += v.x; acc.y += v.y; }
        reinterpret_cast<cplx*>(out)[(long)b * n + o] = acc;
    }
}
void launch_ck_direct(bool inverse, int count, const double* in, double* out, const double2* root, int logn, hipStream_t st) {
    const dim3 grid((((long)count << logn) + CK_THREADS - 1) / CK_THREADS), block(CK_THREADS);
    if (inverse) hipLaunchKernelGGL(ck_direct_kernel<true>, grid, block, 0, st, in, out, root, logn, count);
    else hipLaunchKernelGGL(ck_direct_kernel<false>, grid, block, 0, st, in, out, root, logn, count);
}

}  // namespace mkhe
