// ckks_kernels.h -- the CKKS encoder on the device: the canonical embedding between n = N/2 complex slots and N real coefficients
// (full packing; sparse packing, n < N/2, is the same embedding for the ring of degree 2n on a grid of the coefficients: below), and the scaling
// between real coefficients and RNS polynomials.  What mkckks/encryptor.go:42-64 and
// mkckks/decryptor.go:34-43 reach through lattigo's ckks.Encoder; that encoder is not part of the reference tree, so what is restated
// here is the embedding itself, not lattigo's code path.  Every kernel takes a batch count (grid.y).
//
// Embedding.  zeta_j = exp(i pi 5^j / N); slot j is the evaluation of the coefficient vector m at zeta_j.  zeta_j^n = i (5^j = 1 mod 4),
// so with w_k = m_k + i m_{k+n}, xi = exp(i pi / N), omega = exp(2 pi i / n) and t_j = (5^j mod 2N - 1) / 4 (a permutation of 0 .. n-1)
//     project:  z_j = sum_{k<n} (w_k xi^k) omega^(t_j k)        twist, forward FFT of n points, gather by t
//     embed:    its inverse                                      scatter by t, inverse FFT, 1/n, untwist, split Re / Im
// The FFT is radix-2 decimation in frequency (project) / in time (embed), in place, so position p holds X[bitrev(p)]: the bit reversal
// is folded into the permutation table pos (position p <-> slot pos[p], t_(pos[p]) = bitrev(p)), and twist and permutation are
// part of the first load and the last store.  Arithmetic is IEEE float64 without contraction; the tables are rounded once from long double.
//
// The transform itself is the tile transform of tile_transform.h (one workgroup per tile of 2^logt points in LDS, one launch for n up to the LDS
// limit, else two) on complex float64 elements: 16-byte LDS accesses, 8 elements per thread.
// LDS layout: element l = 16 c + k (chunk c, k < 16) sits in 16-byte slot k ^ f(c & 15) of its chunk, f(c) = c ^ ((c & 4) << 1).  The LDS
// serves a 16-byte read (ds_read_b128) in four groups of 16 lanes, {0-3,12-15,20-27}, {4-11,16-19,28-31} and the same + 32, each out of
// the 16 slots of the 256-byte bank row, and a 16-byte write in groups of 8 adjacent lanes out of 8 slots.  Write A for the slots
// {0-3,12-15} (bits 2 and 3 equal) and B for {4-11}; an XOR by d maps A to A and B to B when bits 2 and 3 of d are equal.  The access shapes:
//   tail16     lane t reads element k of chunk c0 + t: slot k ^ f(c); f is a bijection of the low four chunk bits, so the 16 chunks of a
//              group (c0 + {0-3,12-15,20-27}, c0 a multiple of 64) are on 16 slots; 8 adjacent lanes differ in f(c) & 7 = c & 7
//   stage passes   32 aligned adjacent lanes read 16 adjacent elements of a chunk c (lanes 0-15: A and B of it) and 16 of the chunk
//              c ^ 1 (span >= 32), c ^ 2 (the single stage of span 16) or c ^ 4 (the two-stage pass over the spans 32 and 16); a group
//              takes A ^ f(c) from the first and B ^ f(c) ^ f(d) from the second, disjoint since f(1) = 1, f(2) = 2 and f(4) = 12
//              keep B.  (With the plain XOR by c the last case, d = 4, put B onto A: a two-way conflict.)
//   load / store   lane t handles elements 2t, 2t + 1: a group reads slots {0,2,4,6}, {8..14} ^ 1, {8..14} ^ 2, {0..6} ^ 3 (relative to f(c))
// all conflict-free for the reads; the load phase's writes of stride two are two-way.  The XOR costs no LDS, so 2^13 points fit 128 KiB.
#pragma once
#include "modarith.h"
#include "tile_pass.h"

namespace mkhe {

constexpr int CK_TILE_LOG_BIG = 13;     // largest tile: 2^13 points = 128 KiB of LDS, above the 64 KiB a kernel gets without asking
constexpr int CK_TILE_LOG = 11;         // tile of the two-launch form and largest tile when the request for more LDS is refused (32 KiB)

struct CkFft {
    const double* in;       // first launch: embed: slots [count][n][2]; project: coeffs [count][2n]
    double* out;            // last launch: embed: coeffs; project: slots
    double2* work;          // [count][n], between the two launches
    const double2* w;       // [n/2]: omega^k
    const double2* twist;   // [n]: xi^k
    const u32* pos;         // [n]: slot index of position p
    TilePass p;             // logn = log2 n
};

// asks for CK_TILE_LOG_BIG tiles (dynamic LDS beyond the default limit); false: the runtime refused, keep to CK_TILE_LOG
bool ck_fft_big_lds();
// inverse = embed direction.  Launches n / 2^logt tiles per message.
void launch_ck_fft(bool inverse, const CkFft& a, int count, hipStream_t st);

// pt[b][l][n] = residue mod q_l of r = rint(coeffs[b][n] * scale) (one IEEE multiply, ties to even), for every size of r: up to 2^62 the
// integer itself is reduced, above it r = M * 2^e with the 53-bit mantissa M and the residue is (M mod q)(2^e mod q); negated for r < 0;
// +-0 give 0.  NaN and +-inf (as inputs or as the product) are the caller's error: the output is then unspecified.
// One thread per coefficient, looping over the limbs.
void launch_ck_scale_up(int count, const double* coeffs, double scale, u64* pt, const Mod* mods, int limbs, int N, hipStream_t st);

// coeffs[b][n] = (centred lift of pt[b][.][n] to (-Q/2, Q/2), Q = q_0 .. q_(limbs-1)) / scale without big integers: mixed-radix (Garner)
// digits d_i of x (x = d_0 + d_1 q_0 + d_2 q_0 q_1 + ..) into dig [count][limbs][N]; the digits of Q-1-x are q_i-1-d_i, and Q is odd,
// so x > Q/2 <=> x > Q-1-x, decided exactly by comparing digits from the top; the magnitude x or (Q-1-x)+1 is summed by Horner in
// float64 from the top digit, signed and divided by scale.  Roundings on the largest term: the conversion of the top digit; per lower
// limb the conversion of q_i (q_i < 2^60 is not a double), the multiply and the add; the + 1 of a negative value; the division: 3 limbs in
// all (the lower digits' conversions are relative to smaller terms), every term non-negative, so the relative error is below
// (1 + u)^(3 limbs) - 1 < 4 limbs 2^-53.  A magnitude beyond the range of float64 gives +-inf, never NaN.  garner: Context::garner_table.
// pt must hold canonical residues.
void launch_ck_scale_down(int count, const u64* pt, double scale, double* coeffs, u64* dig, const u64* garner, int nq, const Mod* mods, int limbs, int N,
                          hipStream_t st);

// ---- sparse packing: n = 2^logSlots < N/2 slots.  The message is a polynomial in X^g, g = N / 2n = 2^gap_log: m[k g] = m'[k], k < 2n, with m'
// the embedding of the ring of degree 2n (the transform above with logn = logSlots and that ring's tables), and exactly zero elsewhere.  The
// transforms work on COMPACT arrays [count][2n] that hold m'; these kernels move between them and the grid of the full-length arrays.
// pt[b][l][i] = the residues of launch_ck_scale_up for compact[b][i / g] on the grid, 0 off it: every word of pt is written.  One thread per (i, b).
void launch_ck_sparse_scale_up(int count, const double* compact, double scale, u64* pt, const Mod* mods, int limbs, int N, int gap_log, hipStream_t st);
// compact[b][c] = the value of launch_ck_scale_down for the coefficient c g of pt[b]; off-grid words of pt are not read.  dig [count][limbs][2n].
void launch_ck_sparse_scale_down(int count, const u64* pt, double scale, double* compact, u64* dig, const u64* garner, int nq, const Mod* mods, int limbs,
                                 int N, int gap_log, hipStream_t st);
// coeffs[b][c g] = compact[b][c], 0.0 elsewhere / compact[b][c] = coeffs[b][c g]
void launch_ck_spread(int count, const double* compact, double* coeffs, int N, int gap_log, hipStream_t st);
void launch_ck_pick(int count, const double* coeffs, double* compact, int N, int gap_log, hipStream_t st);
// n = 2^logn < 16 slots (the register tail of the tile transform takes 16 points): the embedding as a direct sum of n products per output, one thread
// per output.  root [n][n]: zeta_j^k = exp(i pi 5^j k / 2n).  inverse (embed): in slots [count][n][2], out compact [count][2n]; else the reverse.
void launch_ck_direct(bool inverse, int count, const double* in, double* out, const double2* root, int logn, hipStream_t st);

}  // namespace mkhe
