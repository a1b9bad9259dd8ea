// bfv_kernels.hip -- see bfv_kernels.h.
#include "bfv_kernels.h"
#include "bfv_arith.h"
#include "tile_transform.h"

namespace mkhe {

// ---- arithmetic mod T and the scalings of one coefficient: bfv_arith.h
// an int64 message value -> its residue in [0, T)
__device__ __forceinline__ u32 bf_from_i64(i64 v, const BfvT& t) {
    const bool neg = v < 0;
    const u32 r = bf_reduce64(neg ? (u64)0 - (u64)v : (u64)v, t);
    return (neg && r) ? t.T - r : r;
}
__device__ __forceinline__ i64 bf_centre(u32 r, const BfvT& t) { return r > t.half ? (i64)r - (i64)t.T : (i64)r; }

// the lift of one coefficient (bfv_kernels.h): limb l of MForm(centred m)
__device__ __forceinline__ u64 bf_lift_limb(u32 m, const BfvT& t, const Mod& md) {
    const bool neg = m > t.half;
    const u64 v = mont_mul(neg ? t.T - m : m, md.r2, md.q, md.ninv32);    // |c| 2^64 mod q_l, for any size of q_l against T
    return (neg && v) ? md.q - v : v;
}
__device__ __forceinline__ void bf_lift_one(const BfvScale& sc, u32 m, u64* pt) {
    for (int l = 0; l < sc.limbs; ++l) pt[(long)l * sc.N] = bf_lift_limb(m, sc.t, sc.mods[l]);
}

// what tile_transform.h needs to know about the NTT
struct BfTr {
    typedef u32 elem;
    typedef uint2 twid;
    typedef u32 ctx;                                                       // T
    static constexpr int EPT = 16;
    // decimation in frequency: (a, b) <- (a + b, (a - b) w); decimation in time with the inverse twiddle undoes it up to the factor 2
    template <bool INV> __device__ __forceinline__ static void bfly(u32& a, u32& b, uint2 w, u32 T) {
        if (INV) { const u32 x = bf_mul(b, w, T); b = bf_sub(a, x, T); a = bf_add(a, x, T); }
        else { const u32 x = bf_sub(a, b, T); a = bf_add(a, b, T); b = bf_mul(x, w, T); }
    }
    // unit permutation of chunk c (bfv_kernels.h, LDS layout)
    __device__ __forceinline__ static int swzc(int c) { return ((c >> 2) & 3) ^ (c & 2); }
    __device__ __forceinline__ static int swz(int l) { return l ^ (swzc(l >> 4) << 2); }
    __device__ __forceinline__ static void load16(const u32* s, int c, u32 (&x)[16]) {
        const uint4* s4 = reinterpret_cast<const uint4*>(s);
        const int f = swzc(c);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint4 v = s4[4 * c + (u ^ f)];
            x[4 * u] = v.x; x[4 * u + 1] = v.y; x[4 * u + 2] = v.z; x[4 * u + 3] = v.w;
        }
    }
    __device__ __forceinline__ static void store16(u32* s, int c, const u32 (&x)[16]) {
        uint4* s4 = reinterpret_cast<uint4*>(s);
        const int f = swzc(c);
#pragma unroll
        for (int u = 0; u < 4; ++u) s4[4 * c + (u ^ f)] = uint4{x[4 * u], x[4 * u + 1], x[4 * u + 2], x[4 * u + 3]};
    }
};

template <bool INV> __global__ void __launch_bounds__(1024) bf_ntt_kernel(BfvNtt a) {
    extern __shared__ uint4 bf_lds[];
    u32* s = reinterpret_cast<u32*>(bf_lds);
    const int n = 1 << a.p.logn, nt = 1 << a.p.logt, b = blockIdx.y;
    const u32 T = a.sc.t.T;
    const TileGeom ge = TileGeom::of(a.p);
    u32* work = a.work + (long)b * n;
    // ---- load
    for (int l = threadIdx.x; l < nt; l += blockDim.x) {
        const int g = ge.g(l);
        u32 v;
        if (!a.p.first) v = work[g];
        else if (INV) v = bf_from_i64((i64)a.in[(long)b * n + a.pos[g]], a.sc.t);
        else {
            const long col = (long)b * a.sc.limbs * n + g;
            const u32 m = a.fuse ? bf_scale_down_one(a.sc, a.in + col, a.dig + col) : bf_reduce64(a.in[(long)b * n + g], a.sc.t);
            v = bf_mul(m, a.twist[g], T);
        }
        s[BfTr::swz(l)] = v;
    }
    __syncthreads();
    // ---- stages
    tile_stages<INV, BfTr>(s, a.w, a.p, ge, T);
    // ---- store
    for (int l = threadIdx.x; l < nt; l += blockDim.x) {
        const int g = ge.g(l);
        const u32 v = s[BfTr::swz(l)];
        if (!a.p.last) work[g] = v;
        else if (INV) {
            const u32 m = bf_mul(v, a.twist[g], T);
            if (a.fuse == BF_FUSE_LIFT) bf_lift_one(a.sc, m, a.out + (long)b * a.sc.limbs * n + g);
            else if (a.fuse) bf_scale_up_one(a.sc, m, a.out + (long)b * a.sc.limbs * n + g);
            else a.out[(long)b * n + g] = m;
        } else a.out[(long)b * n + a.pos[g]] = (u64)bf_centre(v, a.sc.t);
    }
}

// ---- slot map (bfv_kernels.h).  The pair of entry e: the companion travels, the multiplier is recovered from it (w = ceil(w' T / 2^32), exact for
// every w < T; any other 32-bit w' gives some w <= T, and the Shoup product of a canonical value then stays below 2T before its one subtraction).
__device__ __forceinline__ uint2 bf_map_pair(u64 e, u32 T) { return uint2{hi32((e >> 32) * T + 0xffffffffull), hi32(e)}; }

// One workgroup = one message: twist-load, forward stages, gather, multiply, inverse stages, twist-store; nothing intermediate leaves LDS.  The tile
// may fill LDS, so the gather has no second buffer: every thread reads its sources into registers, the workgroup takes a barrier, every thread
// writes the products to its own elements.  The gathered position is masked to the tile whatever the map holds.
constexpr int BF_MAP_EPT = 32;          // elements per thread at the largest tile (2^15 points, 1024 threads); smaller tiles have 16 or fewer

__global__ void __launch_bounds__(1024) bf_slot_map_kernel(BfvSlotMap a) {
    extern __shared__ uint4 bf_lds[];
    u32* s = reinterpret_cast<u32*>(bf_lds);
    const int n = 1 << a.logn, b = blockIdx.y;
    const u32 T = a.t.T;
    const TilePass p{a.logn, a.logn, 0, 1, 1};
    const TileGeom ge = TileGeom::of(p);
    for (int l = threadIdx.x; l < n; l += blockDim.x) s[BfTr::swz(l)] = bf_mul(bf_reduce64(a.in[(long)b * n + l], a.t), a.twist[l], T);
    __syncthreads();
    tile_stages<false, BfTr>(s, a.w, p, ge, T);
    u32 v[BF_MAP_EPT];
#pragma unroll
    for (int k = 0; k < BF_MAP_EPT; ++k) {
        const int l = threadIdx.x + k * blockDim.x;
        if (l < n) v[k] = s[BfTr::swz((int)((u32)a.map[l] & (u32)(n - 1)))];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < BF_MAP_EPT; ++k) {
        const int l = threadIdx.x + k * blockDim.x;
        if (l < n) s[BfTr::swz(l)] = bf_mul(v[k], bf_map_pair(a.map[l], T), T);
    }
    __syncthreads();
    tile_stages<true, BfTr>(s, a.winv, p, ge, T);
    for (int l = threadIdx.x; l < n; l += blockDim.x) a.out[(long)b * n + l] = bf_mul(s[BfTr::swz(l)], a.itwist[l], T);
}
void launch_bf_slot_map(const BfvSlotMap& a, int count, hipStream_t st) {
    const TilePass p{a.logn, a.logn, 0, 1, 1};
    const TileLaunch l = tile_launch_shape(p, count, BfTr::EPT, sizeof(u32));
    hipLaunchKernelGGL(bf_slot_map_kernel, l.grid, l.block, l.lds, st, a);
}

// the gather and the product of the two-launch form, over the work buffers in global memory: one thread per position
__global__ void __launch_bounds__(256) bf_slot_gather_kernel(const u32* __restrict__ src, u32* __restrict__ dst, const u64* __restrict__ map, int n, u32 T) {
    const int l = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (l >= n) return;
    const u64 e = map[l];
    dst[(long)b * n + l] = bf_mul(src[(long)b * n + (int)((u32)e & (u32)(n - 1))], bf_map_pair(e, T), T);
}
void launch_bf_slot_gather(const u32* src, u32* dst, const u64* map, int n, u32 T, int count, hipStream_t st) {
    hipLaunchKernelGGL(bf_slot_gather_kernel, dim3((n + 255) / 256, count), dim3(256), 0, st, src, dst, map, n, T);
}

bool bf_ntt_big_lds() {
    const int bytes = (int)sizeof(u32) << BF_TILE_LOG_BIG;
    const bool ntt = tile_request_lds(&bf_ntt_kernel<false>, &bf_ntt_kernel<true>, bytes);
    return tile_request_lds(&bf_slot_map_kernel, &bf_slot_map_kernel, bytes) && ntt;
}

void launch_bf_ntt(bool inverse, const BfvNtt& a, int count, hipStream_t st) {
    const TileLaunch l = tile_launch_shape(a.p, count, BfTr::EPT, sizeof(u32));
    if (inverse) hipLaunchKernelGGL(bf_ntt_kernel<true>, l.grid, l.block, l.lds, st, a);
    else hipLaunchKernelGGL(bf_ntt_kernel<false>, l.grid, l.block, l.lds, st, a);
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


__global__ void __launch_bounds__(BF_THREADS) bf_lift_kernel(const u64* coeffs, u64* ptmul, BfvScale sc) {
    const int n = 2 * (blockIdx.x * BF_THREADS + threadIdx.x), b = blockIdx.y;
    if (n >= sc.N) return;                                                 // (N is even: a pair never straddles the end)
    const ulonglong2 c = *reinterpret_cast<const ulonglong2*>(coeffs + (long)b * sc.N + n);
    const u32 m0 = bf_reduce64(c.x, sc.t), m1 = bf_reduce64(c.y, sc.t);
    u64* out = ptmul + (long)b * sc.limbs * sc.N + n;
    for (int l = 0; l < sc.limbs; ++l) {
        const Mod md = sc.mods[l];
        *reinterpret_cast<ulonglong2*>(out + (long)l * sc.N) = ulonglong2{bf_lift_limb(m0, sc.t, md), bf_lift_limb(m1, sc.t, md)};
    }
}
void launch_bf_lift(int count, const u64* coeffs, u64* ptmul, const BfvScale& sc, hipStream_t st) {
    hipLaunchKernelGGL(bf_lift_kernel, dim3((sc.N / 2 + BF_THREADS - 1) / BF_THREADS, count), dim3(BF_THREADS), 0, st, coeffs, ptmul, sc);
}

__global__ void __launch_bounds__(BF_THREADS) bf_mul_prepared_kernel(u64* w, const u64* pt, long pt_stride, const Mod* mods, int L, int N, int per_item) {
    const int l = blockIdx.y, z = blockIdx.z;
    const Mod md = mods[l];
    ulonglong2* x = reinterpret_cast<ulonglong2*>(w + ((long)z * L + l) * N);
    const ulonglong2* p = reinterpret_cast<const ulonglong2*>(pt + (long)(z / per_item) * pt_stride + (long)l * N);
    for (int i = blockIdx.x * BF_THREADS + threadIdx.x; i < N / 2; i += gridDim.x * BF_THREADS) {
        const ulonglong2 a = x[i], b = p[i];
        x[i] = ulonglong2{mont_mul(a.x, b.x, md.q, md.ninv32), mont_mul(a.y, b.y, md.q, md.ninv32)};
    }
}
void launch_bf_mul_prepared(u64* w, const u64* pt, long pt_stride, const Mod* mods, int L, int N, int per_item, int npolys, hipStream_t st) {
    hipLaunchKernelGGL(bf_mul_prepared_kernel, dim3((N / 2 + BF_THREADS - 1) / BF_THREADS, L, npolys), dim3(BF_THREADS), 0, st, w, pt, pt_stride, mods, L, N, per_item);
}

}  // namespace mkhe
