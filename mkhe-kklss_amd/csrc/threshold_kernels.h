// threshold_kernels.h -- the three kernels of t-out-of-n threshold secret keys (include/mkhe.h, "threshold secret keys").  A secret key is a buffer
// [R][N], R = nQ + nP rows under the moduli m_j = mods[j] (Q then P), NTT domain, Montgomery form.  Shamir sharing is linear over Z_{m_j}, so it is
// applied to the stored words as they are: a share, an additive key and a folded buffer are again buffers of that shape and representation.
//     share_p[j][i] = (S[j][i] + sum_{k=1}^{t-1} c_k[j][i] x_p^k) mod m_j          c_k: kind 7 of the keystream (uniform mod m_j, SECRET key)
//     add_p[j][i]   = share_p[j][i] lambda_p[j] mod m_j                            lambda_p[j]: the Lagrange coefficient at 0, from the host
//     dst[b][j][i]  = sum_s src_s[b][j][i] mod m_j
// Per-modulus constants wave-uniform, every stored value canonical, no sample-dependent branch or address.  No LDS, no scratch.
#pragma once
#include "encdec_kernels.h"

namespace mkhe {

constexpr int THR_MAX = 32;        // holders of one sharing, points of an active set, sources of a fold
constexpr int THR_G = 4;           // points per thread of threshold_share_kernel (8 G accumulators; G = 8 leaves one wave per SIMD)
constexpr int THR_MAX_ROWS = 64;   // rows whose Lagrange coefficients travel in the kernel arguments of threshold_scale_kernel (a context has at most NTT_MAX_SLOTS)

// Everything the share kernel reads besides S: the SECRET (key, nonce) of the coefficient polynomials, the public points and the output buffers, all
// in the kernel arguments (scalar loads) -- nothing is staged, whatever n is.
struct ThresholdShareArgs : StreamKey {
    int t, n;                      // threshold and number of holders, 1 <= t <= n <= THR_MAX
    u32 x[THR_MAX];                // x_p, pairwise distinct, 1 <= x_p < every m_j
    u64* out[THR_MAX];             // share_p [R][N]
};
// out[p][j][i] for every p < n, j < R, i < N as defined above.  Coefficient polynomial k (1 <= k <= t - 1), row j owns the streams 2 ((k-1) R + j) (lo)
// and 2 ((k-1) R + j) + 1 (hi) of (a.key, a.nonce); c_k[j][i] = ((hi 2^64 + lo) m_j) >> 128, the product of kind 6.  One thread = 8 consecutive
// coefficients of one row for a GROUP of THR_G points: grid (blocks of a row, row, group).  Horner from k = t - 1 down to 1, then S: per step two
// ChaCha20 blocks form c_k once for the group, and acc_p = acc_p x_p + c_k for each of its points, x_p in Montgomery form (formed here, wave-uniform).
// The c_k exist in registers only.  t = 1 reads no stream and copies S.  N is a multiple of 8; sk and every out[p] 16-byte aligned and pairwise distinct.
void launch_threshold_share(const ThresholdShareArgs& a, const u64* sk, const Mod* mods, int rows, int N, hipStream_t st);

struct ThresholdScaleArgs { u64 lam[THR_MAX_ROWS]; };     // MForm(lambda_p[j])
// out[j][i] = MRed(share[j][i], MForm(lambda[j])) = share[j][i] lambda[j] mod m_j, canonical; out may equal share.  rows <= THR_MAX_ROWS.
void launch_threshold_scale(const ThresholdScaleArgs& a, u64* out, const u64* share, const Mod* mods, int rows, int N, hipStream_t st);

// dst[b][j][i] = sum_{s < nsrc} src[s][b][j][i] mod mods[j], canonical, for canonical sources [count][limbs][N]; dst may equal one source exactly
// (every lane reads its pair of every source before it writes).  nsrc > ED_INLINE: src is a staged table.
void launch_limbs_sum(int count, int limbs, int nsrc, const EdTable& src, u64* dst, const Mod* mods, int N, hipStream_t st);

}  // namespace mkhe
