// noise_kernels.hip -- see noise_kernels.h.  64 bytes of LDS per workgroup, no scratch, no atomics.
#include "noise_kernels.h"

namespace mkhe {

constexpr int NZ_WAVES = NZ_THREADS / 64;

// the maximum of one u64 per thread over the workgroup: wave64 shuffles, then one word per wave in LDS.  Every thread of the workgroup calls it.
// Two buffers, taken in turn (round), make one barrier per call enough: whoever writes the buffer of round r + 2 is past the barrier of round
// r + 1, which every thread reaches only behind its reads of round r.
__device__ __forceinline__ u64 nz_block_max(u64 v, u64 (*lds)[NZ_WAVES], int round) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u64 o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    u64* buf = lds[round & 1];
    if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 m = buf[0];
#pragma unroll
    for (int w = 1; w < NZ_WAVES; ++w) m = buf[w] > m ? buf[w] : m;
    return m;
}

// whether this thread holds the workgroup's lexicographic maximum, top digit first, ties to the smaller n (n < 2^63, distinct among the threads
// that are alive; at least one is): per digit a block maximum of digit + 1 (0 = not in the race: digits are below 2^60), whoever is below it
// drops out; the survivors hold equal digits, and a last round on ~n leaves the one with the smallest n.  digit(i) is called by live threads only.
template <class Digit> __device__ __forceinline__ bool nz_select(bool alive, Digit digit, int limbs, u64 n, u64 (*lds)[NZ_WAVES]) {
    int round = 0;
    for (int i = limbs - 1; i >= 0; --i, ++round) {
        const u64 v = alive ? digit(i) + 1 : 0;
        const u64 m = nz_block_max(v, lds, round);                              // (every thread, alive or not: it holds a barrier)
        alive = alive && v == m;
    }
    const u64 key = alive ? ~n : 0;
    const u64 m = nz_block_max(key, lds, round);
    return alive && key == m;
}

__global__ void __launch_bounds__(NZ_THREADS) noise_centre_kernel(NoiseArgs a) {
    __shared__ u64 lds[2][NZ_WAVES];
    const long N = a.N;
    const int L = a.limbs, b = blockIdx.y;
    const long n = (long)blockIdx.x * NZ_THREADS + threadIdx.x;
    const bool alive = n < N;
    u64* d = a.dig + (long)b * L * N + n;
    if (alive) {
        const u64* x = a.phase + (long)b * L * N + n;
        const u64* r = a.ref ? a.ref + (long)b * a.ref_stride + n : nullptr;
        garner_digits([&](int j, const Mod& md) {
            const u64 v = x[j * N];
            if (a.tmont) return mont_mul(v, a.tmont[j], md.q, md.ninv32);      // T x mod q_j; T mod q_j in Montgomery form, q_j may be below T
            if (!r) return v;
            const u64 w = r[j * N];
            return v >= w ? v - w : v + md.q - w;
        }, d, a.garner, a.nq, a.mods, L, N);
        bool neg = false;                                                       // x > (Q - 1) / 2  <=>  x > Q - 1 - x, whose digits are q_i - 1 - d_i
        for (int i = L - 1; i >= 0; --i) {
            const u64 di = d[i * N], oi = a.mods[i].q - 1 - di;
            if (di != oi) { neg = di > oi; break; }
        }
        if (neg) {                                                              // 0 < x < Q: Q - x = (Q - 1 - x) + 1, a digit that reaches q_i becomes 0 and carries
            u64 carry = 1;
            for (int i = 0; i < L; ++i) {
                const u64 q = a.mods[i].q, t = q - 1 - d[i * N] + carry;
                carry = t == q;
                d[i * N] = carry ? 0 : t;
            }
        }
    }
    if (nz_select(alive, [&](int i) { return d[i * N]; }, L, (u64)n, lds)) {
        u64* p = a.part + ((long)b * a.blocks + blockIdx.x) * (L + 1);
        for (int i = 0; i < L; ++i) p[i] = d[i * N];
        p[L] = (u64)n;
    }
}

__global__ void __launch_bounds__(NZ_THREADS) noise_reduce_kernel(NoiseArgs a) {
    __shared__ u64 lds[2][NZ_WAVES];
    const int L = a.limbs, b = blockIdx.y;
    const u64* part = a.part + (long)b * a.blocks * (L + 1);
    long best = threadIdx.x;
    const bool alive = best < a.blocks;
    // this thread's own candidates arrive in the order of their n: only a strictly larger one replaces the best so far
    for (long p = best + NZ_THREADS; p < a.blocks; p += NZ_THREADS)
        for (int i = L - 1; i >= 0; --i) {
            const u64 c = part[p * (L + 1) + i], m = part[best * (L + 1) + i];
            if (c != m) { if (c > m) best = p; break; }
        }
    const u64* mine = part + best * (L + 1);                                    // (read by live threads only)
    if (nz_select(alive, [&](int i) { return mine[i]; }, L, alive ? mine[L] : 0, lds)) {
        u64* o = a.out + (long)b * (L + 1);
        for (int i = 0; i <= L; ++i) o[i] = mine[i];
    }
}

void launch_noise_norm(const NoiseArgs& a, int count, hipStream_t st) {
    hipLaunchKernelGGL(noise_centre_kernel, dim3(a.blocks, count), dim3(NZ_THREADS), 0, st, a);
    hipLaunchKernelGGL(noise_reduce_kernel, dim3(1, count), dim3(NZ_THREADS), 0, st, a);
}

}  // namespace mkhe
