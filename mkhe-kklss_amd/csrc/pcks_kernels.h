// pcks_kernels.h -- the three kernels of the collective key switch to a recipient's public key (include/mkhe.h, "collective public-key switch").
// Party i publishes, for item b, the pair
//     h0 = InvNTT(NTT(c_slot) * sk_i + NTT(u) * pk0) + E,     h1 = InvNTT(NTT(u) * pk1) + e1
// with u ternary (kind 0 of the keystream), e1 a table Gaussian (kind 1), E a wide uniform flood (kind 5) that stands where the e0 of an encryption
// would, and (pk0, pk1) the RECIPIENT's public key; anyone forms (c_0 + sum_i h0_i, sum_i h1_i), an ordinary ciphertext over the recipient's id.
// The transforms in between are the batched kernels of ntt_kernels.hip.  All three kernels are HBM-streaming, per-modulus constants wave-uniform,
// every stored value canonical.  No LDS, no scratch.
#pragma once
#include "encdec_kernels.h"

namespace mkhe {

constexpr int PCKS_MAX_FLOOD = 1024;    // widest flood: 16 streams of 64 bits per coefficient

// The work buffer w [3][count][limbs][N]: on entry w[0] = NTT(c_slot) and w[2] = uh = NTT(u) (canonical, not Montgomery form); on exit
//   w[0] = (w[0] * sk + MForm(uh) * pk0) mod q_j      both products summed as 128-bit integers and reduced once, as decrypt_mac does
//   w[1] = MRed(MForm(uh), pk1)                       bit for bit what encrypt_mul writes
//   w[2] = 0                                          u does not linger
// sk: the Q limbs of the party's secret [..][N]; pk = [2][mtot][N]: pk0 is row j, pk1 row mtot + j.  Stands where decrypt_mac_kernel plus
// encrypt_mul_kernel would.  16-byte accesses, grid (pairs, limb, item).
void launch_pcks_mac(int count, u64* w, const u64* sk, const u64* pk, const Mod* mods, int limbs, int mtot, int N, hipStream_t st);

// Under the call's (a.key, a.nonce): stream b is u_b, stream count + b is e1_b, stream 2 count + b W + w is word w of the flood E_b,
// W = ceil(flood_bits / 64).  With t0 = w[0], t1 = w[1] after their inverse NTT (w [2][count][limbs][N], canonical):
//   shares[b][0][j][n] = (t0[b][j][n] + (E_b[n] mod q_j)) mod q_j          E_b: kind 5, flood_bits wide (0: E = 0, no flood stream is read)
//   shares[b][1][j][n] = (t1[b][j][n] + (e1_b[n] mod q_j)) mod q_j         e1_b: kind 1 on the table a.cdt
// One thread = 8 consecutive coefficients (one ChaCha20 block per stream) of ONE row; grid.y = 2 limbs rows: rows below limbs are limb j of h0,
// the others limb j of h1 -- a wave-uniform split.  Neither E nor e1 ever exists in memory; the blocks are recomputed per limb.  a.first_stream is
// not read.  N is a multiple of 8, count <= 65535.
void launch_pcks_finish(const SmallSampleArgs& a, int flood_bits, int count, u64* shares, const u64* w, const Mod* mods, int limbs, int N, hipStream_t st);

// out[b] = ciphertext [2][limbs][N]: c0 = (c0[b] + sum_i sh[i][b][0]) mod q_j, c1 = (sum_i sh[i][b][1]) mod q_j, canonical.  c0[b]: polynomial 0 of
// input b (any value below 3 q), sh[i]: [count][2][limbs][N] canonical.  One streaming launch, grid.y = 2 limbs rows as in the finish kernel.
void launch_pcks_merge(int count, int nshares, const EdTable& out, const EdTable& c0, const EdTable& sh, const Mod* mods, int limbs, int N, hipStream_t st);

}  // namespace mkhe
