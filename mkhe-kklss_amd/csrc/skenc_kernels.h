// skenc_kernels.h -- the three kernels of secret-key encryption with a seeded c1 (include/mkhe.h, "secret-key encryption").  For item b the party
// that holds s publishes
//     c1 = a_b (kind 6 of the keystream: uniform mod q_j, expanded from a PUBLIC key and nonce),     c0 = pt + e - InvNTT(NTT(c1) * s)
// so that only c0 and the 32-byte seed travel and the phase error is e alone.  The transforms in between are the batched kernels of ntt_kernels.hip.
// All three kernels are HBM-streaming, per-modulus constants wave-uniform, every stored value canonical.  No LDS, no scratch.
#pragma once
#include "encdec_kernels.h"

namespace mkhe {

// the PUBLIC seed of kind 6: nothing here is secret, but it travels like the secret keys do (kernel arguments, scalar loads)
struct UniformArgs : StreamKey {};

// Row (b, j), b < count, j < limbs: out[b][poly_off + j N + n] = ((hi 2^64 + lo) q_j) >> 128, lo / hi = the 64-bit values of coefficient n of the
// streams 2 (b nq + j) and 2 (b nq + j) + 1 of (a.key, a.nonce): nq, the context's number of Q primes, NOT limbs, so that a row does not depend on
// the level it is expanded at.  out: per-item base pointers; poly_off in words (a multiple of 2).  One thread = 8 consecutive coefficients of one
// row: two ChaCha20 blocks, eight 128 x 64-bit products of which the top word is kept, four 16-byte stores.  grid (blocks of a row, limb, item):
// both streams and q_j are wave-uniform.  No division, no rejection, no sample-dependent branch.  N is a multiple of 8, count <= 65535,
// 2 count nq <= 2^32.
void launch_uniform_sample(const UniformArgs& a, int count, const EdTable& out, long poly_off, const Mod* mods, int limbs, int nq, int N, hipStream_t st);

// w [count][limbs][N] (NTT domain, canonical) <- MRed(w, sk) or, with pt_ntt != null (plaintexts [count][limbs][N] in the NTT domain),
// (pt_ntt - MRed(w, sk)) mod q_j: the plaintext rides in the one inverse NTT that follows.  sk: the Q limbs of the party's secret [..][N], the
// same for every item, so no pointer table is staged whatever count is (what decrypt_mac_kernel with k = 1 would need above ED_INLINE items).
void launch_skenc_mul(int count, u64* w, const u64* sk, const u64* pt_ntt, const Mod* mods, int limbs, int N, hipStream_t st);

// With t = w [count][limbs][N] after its inverse NTT (canonical), polynomial 0 of out[b] (row j at out[b] + j N):
//   pt_coeff != null:  c0[b][j][n] = (pt_coeff[b][j][n] + (e_b[n] mod q_j) - t[b][j][n]) mod q_j          pt_coeff [count][limbs][N]
//   pt_coeff == null:  c0[b][j][n] = (t[b][j][n] + (e_b[n] mod q_j)) mod q_j                              (skenc_mul has formed pt - product)
// e_b: smp != null: the int32 samples smp [count][N], e mod q = e >= 0 ? e : q - |e|; smp == null: stream b of (a.key, a.nonce), kind 1 on the
// table a.cdt, formed in registers and recomputed for every limb -- it never exists in memory.  a.first_stream is not read.  One thread = 8
// consecutive coefficients (one ChaCha20 block) of one row, grid (blocks of a row, limb, item).  N is a multiple of 8, count <= 65535.
void launch_skenc_finish(const SmallSampleArgs& a, const i32* smp, int count, const EdTable& out, const u64* w, const u64* pt_coeff, const Mod* mods,
                         int limbs, int N, hipStream_t st);

}  // namespace mkhe
