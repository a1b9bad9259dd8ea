// decshare_kernels.h -- the two kernels of distributed decryption (include/mkhe.h, "distributed decryption"; eprint 2022/347): party i
// publishes the share mu_i = c_i * s_i + e_i with a flooding noise e_i, anyone forms c_0 + sum_i mu_i.  The product is the chain of
// Decrypt with one party (forward NTT, decrypt_mac with k = 1, inverse NTT: encdec_kernels.h); what is new is the last step of each side.
// Both are HBM-streaming, 16-byte accesses, per-modulus constants wave-uniform, every stored value canonical.
#pragma once
#include "encdec_kernels.h"

namespace mkhe {

constexpr int SHF_MAX_BITS = 62;   // widest flooding sample: |e| <= 2^61 keeps the reduction's operand below 2^62 (mont_mul_lazy)

// Everything secret the finish kernel reads travels here, in the kernel arguments (StreamKey, chacha.h).
struct ShareFloodArgs : StreamKey {
    int bits;                      // 0: no flood, the keystream is not read
};

// out[b][j][n] = (acc[b][j][n] + (e_b[n] mod q_j)) mod q_j with acc [count][limbs][N] the canonical inverse-NTT result and e_b kind 2 of the
// keystream (uniform, a.bits wide, centred) on stream b of (key, nonce).  One thread = one ChaCha20 block = 8 consecutive coefficients, formed
// once in registers and added to every limb the thread owns: limb j = blockIdx.y, + rows, ... (rows = limbs: one limb per thread and the block
// recomputed per limb; rows = 1: one thread walks all limbs).  The bits do not depend on rows.  N is a multiple of 8, count <= 65535.
void launch_share_finish(const ShareFloodArgs& a, int count, u64* out, const u64* acc, const Mod* mods, int limbs, int rows, int N, hipStream_t st);

// pt[b][j][n] = (c0[b][j][n] + sum_{i < nshares} sh[i][b][j][n]) mod q_j, canonical: c0[b] = polynomial 0 of ciphertext b (any value below 3 q),
// sh[i] = the share buffer [count][limbs][N] of party i, canonical, so that one conditional subtraction per addend suffices.
void launch_share_merge(int count, int nshares, u64* pt, const EdTable& c0, const EdTable& sh, const Mod* mods, int limbs, int N, hipStream_t st);

}  // namespace mkhe
