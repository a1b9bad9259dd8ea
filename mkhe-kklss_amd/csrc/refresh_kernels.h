// refresh_kernels.h -- the two kernels of the collective refresh (include/mkhe.h, "collective refresh"; the interactive bootstrapping of
// multiparty RLWE): party i publishes the MASKED share c_i * s_i + M_i and a fresh encryption of -M_i at the output level, anyone forms
// the exact centred lift of c_0 + sum_i share_i from Q_l to the output moduli and adds the re-encryptions.  The product and the encryption are
// the chains of decrypt_share and encrypt_seeded (encdec.hip); what is new is the last step of the share and the whole of the merge.
// Both are HBM-streaming, per-modulus constants wave-uniform, every stored value canonical.  No LDS, no scratch.
#pragma once
#include "encdec_kernels.h"

namespace mkhe {

constexpr int RF_MAX_BITS = 120;   // widest mask: |M| <= 2^119 = two words below 2^60, each a legal operand of mont_mul

// Everything secret the finish kernel reads travels here, in the kernel arguments (StreamKey, chacha.h).
struct RefreshMaskArgs : StreamKey {
    int bits;                      // 0: no mask, the keystream is not read
};

// M_b = kind 3 of the keystream (uniform, a.bits wide, centred) from the streams 2 b (low 64 bits) and 2 b + 1 (high 64 bits) of (key, nonce).
//   share[b][j][n] = (acc[b][j][n] + (M_b[n] mod q_j)) mod q_j   for j < lin:   acc [count][lin][N] the canonical inverse-NTT product
//   pt[b][j][n]    = (-M_b[n]) mod q_j                           for j < lout:  the plaintext [count][lout][N] encrypt_core reads
// One thread = two ChaCha20 blocks = 8 consecutive coefficients of M, formed once in registers (magnitude as two words below 2^60 and a sign
// bit) and reduced once per modulus for both outputs; the sign is folded in by a select.  N is a multiple of 8, count <= 65535.
void launch_refresh_finish(const RefreshMaskArgs& a, int count, u64* share, const u64* acc, u64* pt, const Mod* mods, int lin, int lout, int N,
                           hipStream_t st);

// What the merge reads besides the ciphertexts: tables over the nq moduli of Q (Context::refresh_tables) and a digit scratch.
struct RefreshMergeArgs {
    const u64* garner;             // [nq][nq]  Context::garner_table
    const u64* qmont;              // [nq][nq]  MForm(q_i mod q_j) at i * nq + j
    const u64* qprod;              // [nq][nq]  (q_0 .. q_l) mod q_j at l * nq + j, canonical
    u64* dig;                      // [count][lin][N] mixed-radix digits of R
    const Mod* mods;
    int nq, lin, lout, nshares, count, N;
    int nre;                       // re-encryptions per item: nshares, or 0 = none (mkhe_e2s_merge: re is not read, out[b] is polynomial 0 alone)
};
// R = (c0[b] + sum_i sh[i][b]) mod Q_l by its residues (as share_merge_kernel), its mixed-radix digits (garner_digits), R > (Q_l - 1) / 2 decided
// on the digits (as ck_scale_down_kernel decides its sign), the digits evaluated by Horner under q_j for lin <= j < lout, Q_l mod q_j
// subtracted when negative;  out[b] polynomial 0 = that + sum_i polynomial 0 of re[i * count + b], polynomial 1 + i = polynomial 1 of
// re[i * count + b].  c0[b]: polynomial 0 of input b (any value below 3 q), sh[i]: [count][lin][N] canonical, re: ciphertexts [2][lout][N]
// canonical, out[b]: [1 + nshares][lout][N].  One thread = one coefficient of one item.
void launch_refresh_merge(const RefreshMergeArgs& a, const EdTable& out, const EdTable& c0, const EdTable& sh, const EdTable& re, hipStream_t st);

}  // namespace mkhe
