// bfv_kernels.hip -- see bfv_kernels.h.
#include "bfv_kernels.h"

namespace mkhe {

// ---- arithmetic mod T < 2^32 on canonical residues
__device__ __forceinline__ u32 bf_mul(u32 a, uint2 w, u32 T) {            // a * w.x mod T for any 32-bit a; w.y = floor(w.x 2^32 / T)
    const u32 q = hi32((u64)a * w.y);
    const u64 r = (u64)a * w.x - (u64)q * T;                              // in [0, 2T)
    return (u32)(r >= T ? r - T : r);
}
__device__ __forceinline__ u32 bf_add(u32 a, u32 b, u32 T) { const u64 s = (u64)a + b; return (u32)(s >= T ? s - T : s); }
__device__ __forceinline__ u32 bf_sub(u32 a, u32 b, u32 T) { return a >= b ? a - b : a - b + T; }
// any 64-bit value mod T: hi * (2^32 mod T) + lo
__device__ __forceinline__ u32 bf_reduce64(u64 a, const BfvT& t) {
    return bf_add(bf_mul(hi32(a), uint2{t.c32, t.c32_s}, t.T), bf_mul(lo32(a), uint2{1u, t.one_s}, t.T), t.T);
}
// an int64 message value -> its residue in [0, T)
__device__ __forceinline__ u32 bf_from_i64(i64 v, const BfvT& t) {
    const bool neg = v < 0;
    const u32 r = bf_reduce64(neg ? (u64)0 - (u64)v : (u64)v, t);
    return (neg && r) ? t.T - r : r;
}
__device__ __forceinline__ i64 bf_centre(u32 r, const BfvT& t) { return r > t.half ? (i64)r - (i64)t.T : (i64)r; }

// ---- scale_up / scale_down of one coefficient (bfv_kernels.h); pt, dig: the coefficient's column, limb stride N
__device__ __forceinline__ void bf_scale_up_one(const BfvScale& sc, u32 m, u64* pt) {
    const BfvT& t = sc.t;
    const u32 r = bf_add(bf_mul(m, uint2{t.qmod, t.qmod_s}, t.T), t.half, t.T);
    const bool neg = r > t.half;
    const u64 mag = neg ? r - t.half : t.half - r;                        // |floor(T/2) - r| <= T
    for (int l = 0; l < sc.limbs; ++l) {
        const Mod md = sc.mods[l];
        const u64 v = mont_mul(mag, sc.tinv_mont[l], md.q, md.ninv32);
        pt[(long)l * sc.N] = (neg && v) ? md.q - v : v;
    }
}
__device__ __forceinline__ u32 bf_scale_down_one(const BfvScale& sc, const u64* x, u64* d) {
    const BfvT& t = sc.t;
    const int L = sc.limbs;
    const long N = sc.N;
    // d_j = (..((r_j - d_0) q_0^-1 - d_1) q_1^-1 .. - d_(j-1)) q_(j-1)^-1 mod q_j, r_j = T x_j + (q_j - 1) / 2 mod q_j
    for (int j = 0; j < L; ++j) {
        const Mod md = sc.mods[j];
        u64 v = csub(mont_mul(x[j * N], sc.t_mont[j], md.q, md.ninv32) + (md.q >> 1), md.q);
        for (int i = 0; i < j; ++i) {
            const u64 di = mont_mul(d[i * N], md.r1, md.q, md.ninv32);                       // d_i mod q_j
            v = mont_mul(v >= di ? v - di : v + md.q - di, sc.garner[i * L + j], md.q, md.ninv32);
        }
        d[j * N] = v;
    }
    u32 acc = bf_reduce64(d[(L - 1) * N], t);
    for (int i = L - 2; i >= 0; --i) acc = bf_add(bf_mul(acc, sc.qlt[i], t.T), bf_reduce64(d[i * N], t), t.T);
    return bf_mul(bf_sub(t.hq, acc, t.T), uint2{t.qinv, t.qinv_s}, t.T);
}

// decimation in frequency: (a, b) <- (a + b, (a - b) w); decimation in time with the inverse twiddle undoes it up to the factor 2
template <bool INV> __device__ __forceinline__ void bf_bfly(u32& a, u32& b, uint2 w, u32 T) {
    if (INV) { const u32 x = bf_mul(b, w, T); b = bf_sub(a, x, T); a = bf_add(a, x, T); }
    else { const u32 x = bf_sub(a, b, T); a = bf_add(a, b, T); b = bf_mul(x, w, T); }
}
// unit permutation of chunk c (bfv_kernels.h, LDS layout)
__device__ __forceinline__ int bf_swzc(int c) { return ((c >> 2) & 3) ^ (c & 2); }
__device__ __forceinline__ int bf_swz(int l) { return l ^ (bf_swzc(l >> 4) << 2); }

// where the elements of a tile sit in the transform, and the twiddle of a butterfly
struct BfGeom {
    int logn, a_log, cc_log, tile, logt;
    // global index of local element l: contiguous tile: tile * 2^logt + l; column tile: l = r * Cc + c -> r * B + tile * Cc + c (B = N >> a_log)
    __device__ __forceinline__ int g(int l) const {
        if (!a_log) return (tile << logt) + l;
        return ((l >> cc_log) << (logn - a_log)) + (tile << cc_log) + (l & ((1 << cc_log) - 1));
    }
    // the stage whose butterflies pair local elements 2^logh apart pairs global elements H = 2^logH apart; its twiddle at global index g is
    // omega^((g mod H) * N / 2H)
    __device__ __forceinline__ int tw(int l, int logh) const {
        const int logH = a_log ? logh - cc_log + logn - a_log : logh;
        return (g(l) & ((1 << logH) - 1)) << (logn - 1 - logH);
    }
};

// one stage on the tile in LDS: every thread takes butterflies of adjacent first elements
template <bool INV> __device__ __forceinline__ void bf_stage2(u32* s, const uint2* __restrict__ w, const BfGeom& ge, int logh, u32 T) {
    const int h = 1 << logh, n = 1 << ge.logt;
    for (int u = threadIdx.x; u < n / 2; u += blockDim.x) {
        const int i = ((u >> logh) << (logh + 1)) | (u & (h - 1));
        u32 a = s[bf_swz(i)], b = s[bf_swz(i + h)];
        bf_bfly<INV>(a, b, w[ge.tw(i, logh)], T);
        s[bf_swz(i)] = a; s[bf_swz(i + h)] = b;
    }
}
// the stages 2^(lq+1) and 2^lq in one pass over the tile (forward: in this order; inverse: the other way round): the same operations
// as two bf_stage2 calls on the four elements i + {0, 1, 2, 3} * 2^lq
template <bool INV> __device__ __forceinline__ void bf_stage4(u32* s, const uint2* __restrict__ w, const BfGeom& ge, int lq, u32 T) {
    const int hq = 1 << lq, n = 1 << ge.logt;
    for (int u = threadIdx.x; u < n / 4; u += blockDim.x) {
        const int i = ((u >> lq) << (lq + 2)) | (u & (hq - 1));
        u32 x0 = s[bf_swz(i)], x1 = s[bf_swz(i + hq)], x2 = s[bf_swz(i + 2 * hq)], x3 = s[bf_swz(i + 3 * hq)];
        const uint2 wa = w[ge.tw(i, lq + 1)], wb = w[ge.tw(i + hq, lq + 1)], wc = w[ge.tw(i, lq)];
        if (INV) { bf_bfly<INV>(x0, x1, wc, T); bf_bfly<INV>(x2, x3, wc, T); bf_bfly<INV>(x0, x2, wa, T); bf_bfly<INV>(x1, x3, wb, T); }
        else { bf_bfly<INV>(x0, x2, wa, T); bf_bfly<INV>(x1, x3, wb, T); bf_bfly<INV>(x0, x1, wc, T); bf_bfly<INV>(x2, x3, wc, T); }
        s[bf_swz(i)] = x0; s[bf_swz(i + hq)] = x1; s[bf_swz(i + 2 * hq)] = x2; s[bf_swz(i + 3 * hq)] = x3;
    }
}
// the stages 8, 4, 2, 1 of a contiguous tile on 16 adjacent elements per thread, in registers.  Their twiddles are the 16th roots
// omega^(m N / 16), the same for every chunk.
template <bool INV> __device__ __forceinline__ void bf_tail16(u32* s, const uint2* __restrict__ w, int logn, int logt, u32 T) {
    uint2 r16[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) r16[m] = w[m << (logn - 4)];
    uint4* s4 = reinterpret_cast<uint4*>(s);
    for (int c = threadIdx.x; c < (1 << (logt - 4)); c += blockDim.x) {
        const int f = bf_swzc(c);
        u32 x[16];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint4 v = s4[4 * c + (u ^ f)];
            x[4 * u] = v.x; x[4 * u + 1] = v.y; x[4 * u + 2] = v.z; x[4 * u + 3] = v.w;
        }
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const int h = INV ? 1 << st : 8 >> st;
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (!(e & h)) bf_bfly<INV>(x[e], x[e + h], r16[(e & (h - 1)) * (8 / h)], T);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) s4[4 * c + (u ^ f)] = uint4{x[4 * u], x[4 * u + 1], x[4 * u + 2], x[4 * u + 3]};
    }
}

template <bool INV> __global__ void __launch_bounds__(1024) bf_ntt_kernel(BfvNtt a) {
    extern __shared__ uint4 bf_lds[];
    u32* s = reinterpret_cast<u32*>(bf_lds);
    const int n = 1 << a.logn, nt = 1 << a.logt, b = blockIdx.y;
    const u32 T = a.sc.t.T;
    BfGeom ge{a.logn, a.a_log, a.logt - a.a_log, (int)blockIdx.x, a.logt};
    u32* work = a.work + (long)b * n;
    // ---- load
    for (int l = threadIdx.x; l < nt; l += blockDim.x) {
        const int g = ge.g(l);
        u32 v;
        if (!a.first) v = work[g];
        else if (INV) v = bf_from_i64((i64)a.in[(long)b * n + a.pos[g]], a.sc.t);
        else {
            const long col = (long)b * a.sc.limbs * n + g;
            const u32 m = a.fuse ? bf_scale_down_one(a.sc, a.in + col, a.dig + col) : bf_reduce64(a.in[(long)b * n + g], a.sc.t);
            v = bf_mul(m, a.twist[g], T);
        }
        s[bf_swz(l)] = v;
    }
    __syncthreads();
    // ---- stages.  A contiguous tile has the local spans 2^(logt-1) .. 1, the last four of them in bf_tail16; a column tile the spans down to Cc.
    const int lo_log = a.a_log ? ge.cc_log : 4, hi_log = a.logt - 1;      // head stages lo_log .. hi_log
    const int odd = (hi_log - lo_log + 1) & 1;
    if (!INV) {
        int lh = hi_log;
        if (odd) { bf_stage2<INV>(s, a.w, ge, lh, T); __syncthreads(); --lh; }
        for (; lh > lo_log; lh -= 2) { bf_stage4<INV>(s, a.w, ge, lh - 1, T); __syncthreads(); }
        if (!a.a_log) { bf_tail16<INV>(s, a.w, a.logn, a.logt, T); __syncthreads(); }
    } else {
        if (!a.a_log) { bf_tail16<INV>(s, a.w, a.logn, a.logt, T); __syncthreads(); }
        int lh = lo_log;
        for (; lh + 1 <= hi_log; lh += 2) { bf_stage4<INV>(s, a.w, ge, lh, T); __syncthreads(); }
        if (odd) { bf_stage2<INV>(s, a.w, ge, hi_log, T); __syncthreads(); }
    }
    // ---- store
    for (int l = threadIdx.x; l < nt; l += blockDim.x) {
        const int g = ge.g(l);
        const u32 v = s[bf_swz(l)];
        if (!a.last) work[g] = v;
        else if (INV) {
            const u32 m = bf_mul(v, a.twist[g], T);
            if (a.fuse) bf_scale_up_one(a.sc, m, a.out + (long)b * a.sc.limbs * n + g);
            else a.out[(long)b * n + g] = m;
        } else a.out[(long)b * n + a.pos[g]] = (u64)bf_centre(v, a.sc.t);
    }
}

bool bf_ntt_big_lds() {
    const int bytes = (int)sizeof(u32) << BF_TILE_LOG_BIG;
    const hipError_t e0 = hipFuncSetAttribute(reinterpret_cast<const void*>(&bf_ntt_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    const hipError_t e1 = hipFuncSetAttribute(reinterpret_cast<const void*>(&bf_ntt_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e0 == hipSuccess && e1 == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}

void launch_bf_ntt(bool inverse, const BfvNtt& a, int count, hipStream_t st) {
    const int nt = 1 << a.logt;
    int threads = nt / 16;
    threads = threads < 64 ? 64 : threads > 1024 ? 1024 : threads;
    const dim3 grid(1 << (a.logn - a.logt), count);
    const size_t lds = sizeof(u32) * (size_t)nt;
    if (inverse) hipLaunchKernelGGL(bf_ntt_kernel<true>, grid, dim3(threads), lds, st, a);
    else hipLaunchKernelGGL(bf_ntt_kernel<false>, grid, dim3(threads), lds, st, a);
}

constexpr int BF_THREADS = 256;

__global__ void __launch_bounds__(BF_THREADS) bf_scale_up_kernel(const u64* coeffs, u64* pt, BfvScale sc) {
    const int n = blockIdx.x * BF_THREADS + threadIdx.x, b = blockIdx.y;
    if (n >= sc.N) return;
    bf_scale_up_one(sc, bf_reduce64(coeffs[(long)b * sc.N + n], sc.t), pt + (long)b * sc.limbs * sc.N + n);
}
void launch_bf_scale_up(int count, const u64* coeffs, u64* pt, const BfvScale& sc, hipStream_t st) {
    hipLaunchKernelGGL(bf_scale_up_kernel, dim3((sc.N + BF_THREADS - 1) / BF_THREADS, count), dim3(BF_THREADS), 0, st, coeffs, pt, sc);
}

__global__ void __launch_bounds__(BF_THREADS) bf_scale_down_kernel(const u64* pt, u64* coeffs, u64* dig, BfvScale sc) {
    const int n = blockIdx.x * BF_THREADS + threadIdx.x, b = blockIdx.y;
    if (n >= sc.N) return;
    const long col = (long)b * sc.limbs * sc.N + n;
    coeffs[(long)b * sc.N + n] = bf_scale_down_one(sc, pt + col, dig + col);
}
void launch_bf_scale_down(int count, const u64* pt, u64* coeffs, u64* dig, const BfvScale& sc, hipStream_t st) {
    hipLaunchKernelGGL(bf_scale_down_kernel, dim3((sc.N + BF_THREADS - 1) / BF_THREADS, count), dim3(BF_THREADS), 0, st, pt, coeffs, dig, sc);
}

}  // namespace mkhe
