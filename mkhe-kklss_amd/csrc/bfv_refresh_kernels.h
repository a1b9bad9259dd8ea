// bfv_refresh_kernels.h -- the two kernels of the collective refresh of MK-BFV (include/mkhe.h, "collective refresh for MK-BFV").  Party i
// publishes the share c_i * s_i + up(A_i) + e_i -- A_i uniform mod T (kind 4 of the keystream), e_i a flood of up to 1024 bits (kind 5) -- and a
// fresh encryption of up(-A_i); anyone rounds c_0 + sum_i share_i down to Z_T, which gives (m + sum_i A_i) mod T and drops the noise, scales that
// up again and adds the re-encryptions, which cancel the masks.  Unlike the refresh of refresh_kernels.h, which only moves a ciphertext up the
// modulus chain, this one removes noise.  The product and the encryption are the chains of decrypt_share and encrypt_seeded (encdec.hip); what
// is new is the last step of the share and the whole of the merge.  up / down are scale_up / scale_down of bfv_kernels.h.
// Both kernels are HBM-streaming, per-modulus constants wave-uniform, every stored value canonical.  No LDS, no scratch.
#pragma once
#include "bfv_kernels.h"
#include "encdec_kernels.h"

namespace mkhe {

constexpr int BRF_MAX_FLOOD = 1024;     // widest flood: 16 streams of 64 bits per coefficient

// Everything secret the finish kernel reads travels here, in the kernel arguments (StreamKey, chacha.h).
struct BfvRefreshArgs : StreamKey {
    int mask;                      // 0: A = 0, the mask streams are not read (tests only)
    int flood_bits;                // 0: e = 0, no flood stream is read
};

// Item b owns the S = 2 + W streams b S .. b S + S - 1 of (key, nonce), W = ceil(flood_bits / 64).
//   A_b[n] = ((hi 2^64 + lo) T) >> 128, lo from stream b S, hi from stream b S + 1                               kind 4: uniform mod T
//   e_b[n] = sum_w v_w 2^(64 w) - 2^(flood_bits-1), v_w from stream b S + 2 + w, the top word masked to its low flood_bits - 64 (W - 1) bits   kind 5
//   share[b][j][n] = (acc[b][j][n] + up(A_b[n])[j] + (e_b[n] mod q_j)) mod q_j      acc [count][limbs][N] the canonical inverse-NTT product
//   pt[b][j][n]    = up((T - A_b[n]) mod T)[j]                                      the plaintext [count][limbs][N] encrypt_core reads
// limbs = sc.limbs (every mkbfv ciphertext is at the maximum level).  One thread = 8 consecutive coefficients (one ChaCha20 block per stream) of ONE
// limb: the limb is in the grid, so that a thread holds 8 Horner accumulators and the 8 words of one stream, not 8 x W words; the blocks are
// recomputed per limb.  Neither A nor e ever exists in memory.  N is a multiple of 8, count <= 65535.
void launch_bfv_refresh_finish(const BfvRefreshArgs& a, int count, u64* share, const u64* acc, u64* pt, const BfvScale& sc, hipStream_t st);
// The compile-time variant of the same kernel body for mkhe_bfv_e2s_share (bfv_e2s_finish_kernel): the same streams, blocks and share;
//   secret[b][n] = (T - A_b[n]) mod T                                               [count][N] over Z_T, the caller's; written by the limb-0 row only
// and no plaintext.  up(secret) is the pt of the call above.
void launch_bfv_e2s_finish(const BfvRefreshArgs& a, int count, u64* share, const u64* acc, u64* secret, const BfvScale& sc, hipStream_t st);

// R = (c0[b] + sum_i sh[i][b]) mod Q by its residues (as share_merge_kernel), w = down(R) (its Garner digits into dig [count][limbs][N], Horner mod
// T: bf_scale_down of bfv_kernels.h), then out[b] polynomial 0 = up(w) + sum_i polynomial 0 of re[i * count + b] under every modulus, polynomial
// 1 + i = polynomial 1 of re[i * count + b].  c0[b]: polynomial 0 of input b (any value below 3 q), sh[i]: [count][limbs][N] canonical, re:
// ciphertexts [2][limbs][N] canonical, out[b]: [1 + nshares][limbs][N].  One thread = one coefficient of one item; w stays in a register.
void launch_bfv_refresh_merge(int count, int nshares, u64* dig, const BfvScale& sc, const EdTable& out, const EdTable& c0, const EdTable& sh, const EdTable& re,
                              hipStream_t st);

}  // namespace mkhe
