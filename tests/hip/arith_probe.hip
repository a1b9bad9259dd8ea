// arith_probe.hip -- TEST ONLY: one entry point that runs the project's own device arithmetic (csrc/modarith.h, csrc/h16_arith.h, the
// h mod q estimate of csrc/poly_kernels.h) element by element, so that tests/test_gpu_arith_probe.py can compare every primitive with the
// integer models of tests/arith_model.py at the edges of its contract.  Nothing is restated here: the kernels below only instantiate the
// inline functions of those headers.  Built by csrc/Makefile into lib/libmkhe_arith_probe.so, linked with none of the product objects and
// not part of the product ABI (include/mkhe.h).
#include "h16_arith.h"
#include "poly_kernels.h"

using namespace mkhe;
using namespace mkhe::h16;

namespace {

enum Op {
    OP_MONT_MUL_LAZY = 0,   // out0 = mont_mul_lazy(x0, x1, q, ninv32)
    OP_MONT_MUL = 1,        // out0 = mont_mul(x0, x1, q, ninv32)
    OP_MONT_MUL_SD = 2,     // out0 = mont_mul_sd((i64)x0, ws = x1, sd_split(q), ninv32)
    OP_MONT_MUL_SDU = 3,    // out0 = mont_mul_sdu(x0, ws = x1, sd_split(q), q, ninv32)
    OP_MUL64 = 4,           // (out0, out1) = (hi, lo) of x0 * x1
    OP_MAC128 = 5,          // (out0, out1) = (hi, lo) = (x2, x3) + x0 * x1
    OP_REDC128 = 6,         // out0 = redc128(hi = x0, lo = x1, mod)
    OP_CSUB = 7,            // out0 = csub(x0, x1)
    OP_MM_V = 8,            // out0 = mm<false>((i64)x0, ws = x1)                        per-lane twiddle
    OP_MM_S = 9,            // out0 = mm<true>((i64)x0, ws = x1[blockIdx.x])             one twiddle per workgroup, in SGPRs
    OP_MM31_V = 10,         // out0 = mm31<false>((i64)x0, us = x1, vs = x2)
    OP_MM31_S = 11,         // out0 = mm31<true>((i64)x0, x1[blockIdx.x], x2[blockIdx.x])
    OP_MM30U_V = 12,        // out0 = mm30u<false>((i64)x0, us = x1, vs = x2)
    OP_MM30U_S = 13,        // out0 = mm30u<true>((i64)x0, x1[blockIdx.x], x2[blockIdx.x])
    OP_PRED = 14,           // out0 = pred((i64)x0)
    OP_BFLYF = 15,          // (out0, out1) = bit patterns (U', V') of bflyF(U = x0, V = x1, w = x2 as a double's bit pattern)
    OP_U2D = 16,            // out0 = bit pattern of u2d(x0)
    OP_D2U = 17,            // out0 = d2u(x0 as a double's bit pattern)
    OP_CANONF = 18,         // out0 = canonF(x0 as a double's bit pattern)
    OP_MOD_BY_ESTIMATE = 19,// out0 = mod_by_estimate(h = x0, q = x1)
    OP_COUNT = 20
};

constexpr int PROBE_THREADS = 256;
constexpr long PROBE_MAX = 1l << 18;

// what the caller supplies of a modulus (the fields of Mod that the primitives read); passed by value, so wave-uniform
struct ProbeMod { u64 q; u64 qinv; u32 ninv32; u32 finv; };

// the per-job constants as the NTT kernels derive them from Mod (ntt16_kernels.hip limb(), limb_f()): UC selects the radix-2^30 digits of q
template <bool UC> __device__ __forceinline__ MC make_mc(const ProbeMod& pm) {
    const u64 qs = sd_split(pm.q);
    MC c;
    c.q = pm.q; c.ninv = pm.ninv32;
    c.q0 = (i32)lo32(qs); c.q1 = (i32)hi32(qs);
    c.finv = __builtin_bit_cast(float, pm.finv);
    if constexpr (UC) {
        c.p0 = (i32)((u32)c.q << 2) >> 2;
        c.p1 = (i32)((c.q - (u64)(i64)c.p0) >> 30);
    } else {
        c.p0 = (i32)((u32)c.q << 1) >> 1;
        c.p1 = (i32)((c.q - (u64)(i64)c.p0) >> 31);
    }
    asm("" : "+s"(c.q0), "+s"(c.q1), "+s"(c.ninv), "+s"(c.p0), "+s"(c.p1));
    return c;
}
__device__ __forceinline__ FC make_fc(const ProbeMod& pm) {
    FC c;
    c.q = (double)pm.q; c.qinv = 1.0 / (double)pm.q;
    return c;
}
// a 64-bit word that is the same in every lane, moved into scalar registers
__device__ __forceinline__ u64 uniform64(u64 v) {
    return ((u64)(u32)__builtin_amdgcn_readfirstlane((int)hi32(v)) << 32) | (u32)__builtin_amdgcn_readfirstlane((int)lo32(v));
}

template <int OP>
__global__ void __launch_bounds__(PROBE_THREADS) probe_kernel(long n, const u64* x0, const u64* x1, const u64* x2, const u64* x3, ProbeMod pm,
                                                              u64* out0, u64* out1) {
    const long i = (long)blockIdx.x * PROBE_THREADS + threadIdx.x;
    constexpr bool SW = OP == OP_MM_S || OP == OP_MM31_S || OP == OP_MM30U_S;
    // the SW forms read their twiddle before the bounds check: every lane of the workgroup reads word blockIdx.x (< number of workgroups)
    u64 ts0 = 0, ts1 = 0;
    if constexpr (SW) {
        ts0 = uniform64(x1[blockIdx.x]);
        if constexpr (OP != OP_MM_S) ts1 = uniform64(x2[blockIdx.x]);
    }
    if (i >= n) return;
    if constexpr (OP == OP_MONT_MUL_LAZY) out0[i] = mont_mul_lazy(x0[i], x1[i], pm.q, pm.ninv32);
    else if constexpr (OP == OP_MONT_MUL) out0[i] = mont_mul(x0[i], x1[i], pm.q, pm.ninv32);
    else if constexpr (OP == OP_MONT_MUL_SD) out0[i] = (u64)mont_mul_sd((i64)x0[i], x1[i], sd_split(pm.q), pm.ninv32);
    else if constexpr (OP == OP_MONT_MUL_SDU) out0[i] = mont_mul_sdu(x0[i], x1[i], sd_split(pm.q), pm.q, pm.ninv32);
    else if constexpr (OP == OP_MUL64) { u64 h, l; mul64x64(x0[i], x1[i], h, l); out0[i] = h; out1[i] = l; }
    else if constexpr (OP == OP_MAC128) { u64 h = x2[i], l = x3[i]; mac128(x0[i], x1[i], h, l); out0[i] = h; out1[i] = l; }
    else if constexpr (OP == OP_REDC128) {
        Mod md = {};
        md.q = pm.q; md.qinv = pm.qinv;
        out0[i] = redc128(x0[i], x1[i], md);
    }
    else if constexpr (OP == OP_CSUB) out0[i] = csub(x0[i], x1[i]);
    else if constexpr (OP == OP_MM_V) out0[i] = (u64)mm<false>((i64)x0[i], x1[i], make_mc<false>(pm));
    else if constexpr (OP == OP_MM_S) out0[i] = (u64)mm<true>((i64)x0[i], ts0, make_mc<false>(pm));
    else if constexpr (OP == OP_MM31_V) out0[i] = (u64)mm31<false>((i64)x0[i], x1[i], x2[i], make_mc<false>(pm));
    else if constexpr (OP == OP_MM31_S) out0[i] = (u64)mm31<true>((i64)x0[i], ts0, ts1, make_mc<false>(pm));
    else if constexpr (OP == OP_MM30U_V) out0[i] = (u64)mm30u<false>((i64)x0[i], x1[i], x2[i], make_mc<true>(pm));
    else if constexpr (OP == OP_MM30U_S) out0[i] = (u64)mm30u<true>((i64)x0[i], ts0, ts1, make_mc<true>(pm));
    else if constexpr (OP == OP_PRED) out0[i] = (u64)pred((i64)x0[i], make_mc<false>(pm));
    else if constexpr (OP == OP_BFLYF) {
        u64 U = x0[i], V = x1[i];
        bflyF(U, V, __builtin_bit_cast(double, x2[i]), make_fc(pm));
        out0[i] = U; out1[i] = V;
    }
    else if constexpr (OP == OP_U2D) out0[i] = __builtin_bit_cast(u64, u2d(x0[i]));
    else if constexpr (OP == OP_D2U) out0[i] = d2u(__builtin_bit_cast(double, x0[i]));
    else if constexpr (OP == OP_CANONF) out0[i] = canonF(__builtin_bit_cast(double, x0[i]), make_fc(pm));
    else if constexpr (OP == OP_MOD_BY_ESTIMATE) out0[i] = mod_by_estimate(x0[i], x1[i]);
}

struct OpShape { int nin; int nout; int per_block; /* bit k: operand k has one word per workgroup */ };
OpShape shape_of(int op) {
    switch (op) {
    case OP_MONT_MUL_LAZY: case OP_MONT_MUL: case OP_MONT_MUL_SD: case OP_MONT_MUL_SDU: case OP_REDC128: case OP_CSUB: case OP_MM_V:
    case OP_MOD_BY_ESTIMATE: return {2, 1, 0};
    case OP_MUL64: return {2, 2, 0};
    case OP_MAC128: return {4, 2, 0};
    case OP_MM_S: return {2, 1, 2};
    case OP_MM31_V: case OP_MM30U_V: return {3, 1, 0};
    case OP_MM31_S: case OP_MM30U_S: return {3, 1, 6};
    case OP_PRED: case OP_U2D: case OP_D2U: case OP_CANONF: return {1, 1, 0};
    case OP_BFLYF: return {3, 2, 0};
    default: return {0, 0, 0};
    }
}

template <int OP> void launch_one(int op, int blocks, long n, u64* const* d, ProbeMod pm, u64* o0, u64* o1) {
    if (op == OP) hipLaunchKernelGGL(probe_kernel<OP>, dim3(blocks), dim3(PROBE_THREADS), 0, 0, n, d[0], d[1], d[2], d[3], pm, o0, o1);
}
template <int... OPS> void launch_any(std::integer_sequence<int, OPS...>, int op, int blocks, long n, u64* const* d, ProbeMod pm, u64* o0, u64* o1) {
    (launch_one<OPS>(op, blocks, n, d, pm, o0, o1), ...);
}

}  // namespace

// Runs primitive `op` on n <= 2^18 elements.  in[k]: host pointer to operand k (n words, or one word per workgroup of 256 elements for the
// twiddles of the SW forms: ceil(n / 256) words); mod: {q, q^-1 mod 2^64, -q^-1 mod 2^32, float32 bits of 2^32 / q}; out[k]: host pointer to
// result k (n words).  Allocates, copies, launches one kernel, synchronises, copies back and frees.  Returns the HIP error code (0 = success).
extern "C" int mkhe_arith_probe(int op, long n, const uint64_t* const* in, const uint64_t* mod, uint64_t* const* out) {
    if (op < 0 || op >= OP_COUNT || n < 1 || n > PROBE_MAX || !in || !mod || !out) return (int)hipErrorInvalidValue;
    const OpShape sh = shape_of(op);
    const int blocks = (int)((n + PROBE_THREADS - 1) / PROBE_THREADS);
    for (int k = 0; k < sh.nin; ++k) if (!in[k]) return (int)hipErrorInvalidValue;
    for (int k = 0; k < sh.nout; ++k) if (!out[k]) return (int)hipErrorInvalidValue;
    u64* d[4] = {nullptr, nullptr, nullptr, nullptr};
    u64* o[2] = {nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (int k = 0; k < sh.nin && e == hipSuccess; ++k) {
        const size_t words = ((sh.per_block >> k) & 1) ? (size_t)blocks : (size_t)n;
        e = hipMalloc((void**)&d[k], words * 8);
        if (e == hipSuccess) e = hipMemcpy(d[k], in[k], words * 8, hipMemcpyHostToDevice);
    }
    for (int k = 0; k < sh.nout && e == hipSuccess; ++k) {
        e = hipMalloc((void**)&o[k], (size_t)n * 8);
        if (e == hipSuccess) e = hipMemset(o[k], 0xee, (size_t)n * 8);
    }
    if (e == hipSuccess) {
        const ProbeMod pm = {mod[0], mod[1], (u32)mod[2], (u32)mod[3]};
        launch_any(std::make_integer_sequence<int, OP_COUNT>{}, op, blocks, n, d, pm, o[0], o[1]);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    for (int k = 0; k < sh.nout && e == hipSuccess; ++k) e = hipMemcpy(out[k], o[k], (size_t)n * 8, hipMemcpyDeviceToHost);
    for (int k = 0; k < 4; ++k) if (d[k]) (void)hipFree(d[k]);
    for (int k = 0; k < 2; ++k) if (o[k]) (void)hipFree(o[k]);
    return (int)e;
}
