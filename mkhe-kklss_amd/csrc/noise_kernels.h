// noise_kernels.h -- the two kernels of mkhe_noise_norm (include/mkhe.h, "noise measurement"): the exact centred max norm of count polynomials
// given by their residues, max_n min(x_n, Q - x_n) with the smallest n that attains it, Q = q_0 .. q_(limbs-1).  No big integer: x_n is taken to
// its mixed-radix digits (garner_digits, modarith.h), centred on the digits, and the maximum is the lexicographic one, top digit first.
// No atomics, no inter-workgroup hand-off: every workgroup of the first launch writes one candidate, the second launch (one workgroup per item)
// selects among them by the same rule, so the result is a pure function of the inputs.  Per-modulus constants are wave-uniform.
#pragma once
#include "modarith.h"

namespace mkhe {

constexpr int NZ_THREADS = 256;    // coefficients per workgroup of the first launch = candidates per pass of the second

inline int nz_blocks(int N) { return (N + NZ_THREADS - 1) / NZ_THREADS; }

struct NoiseArgs {
    const u64* phase;              // [count][limbs][N] canonical, coefficient domain
    const u64* ref;                // kind 0: same shape (item stride ref_stride words, 0 = one for all), or null; kind 1: null
    long ref_stride;
    const u64* tmont;              // kind 1: [limbs] MForm(T mod q_l) (Context::bf_init); kind 0: null
    const u64* garner;             // [nq][nq]  Context::garner_table
    const Mod* mods;
    u64* dig;                      // [count][limbs][N] digit scratch: the centred digits behind the first launch
    u64* part;                     // [count][blocks][limbs + 1] candidates of the workgroups: digits, then n
    u64* out;                      // [count][limbs + 1] digits of the maximum, then the smallest n that attains it
    int nq, limbs, N, blocks;
};
// first launch: one thread = one coefficient n of one item b (grid.y; count <= 65535).  x = (phase - ref) mod q_l resp. T phase mod q_l by its residues,
// its digits into column n of dig, x > (Q - 1) / 2 decided on the digits (x > Q - 1 - x, whose digits are q_i - 1 - d_i) and then the digits of
// Q - x in their place (q_i - 1 - d_i plus one, with carry from digit 0); the workgroup's lexicographic maximum, ties to the smaller n, to part.
// second launch: grid.x = count; every thread takes the candidates tid, tid + NZ_THREADS, .. in turn, the workgroup selects as above, to out.
void launch_noise_norm(const NoiseArgs& a, int count, hipStream_t st);

}  // namespace mkhe
