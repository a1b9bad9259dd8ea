// bfv_kernels.h -- the BFV batch encoder on the device: N slots over Z_T <-> coefficients over Z_T <-> RNS plaintext over Q.  What
// mkbfv/encryptor.go:38-41 (EncryptMsg = EncodeInt, Encrypt) and mkbfv/decryptor.go:52-54 (DecodeInt) reach through lattigo's bfv.Encoder; that
// encoder is not part of the reference tree, so what is restated here is the mathematics of the encoder (include/mkhe.h, "BFV batch encoder"), not
// lattigo's code path.  Every stage is integer arithmetic: every output is exact.  Every kernel takes a batch count (grid.y).
//
// Transform.  psi: the primitive 2N-th root of unity mod T of the engine's rule (default_psi), omega = psi^2.  Slot j is m(psi^(e_j)), e_j = 5^j mod 2N
// for j < N/2 and 2N - 5^(j - N/2) above; with t_j = (e_j - 1) / 2 (a permutation of 0 .. N-1)
//     coeffs_to_slots:  z_j = sum_k (m_k psi^k) omega^(t_j k)          twist, forward NTT of N points, gather by t
//     slots_to_coeffs:  its inverse                                     scatter by t, inverse NTT, times psi^-k / N
// The NTT is radix-2 decimation in frequency (forward) / in time (inverse), in place, so position p holds X[bitrev(p)]: the bit reversal is folded
// into the permutation table pos (position p <-> slot pos[p], t_(pos[p]) = bitrev(p)); twist (with 1/N), permutation, the reduction of the int64
// message values and the centring are part of the first load and the last store.  In the fused calls so are scale_down (load of the forward
// transform) and scale_up (store of the inverse one) when one workgroup holds the polynomial: the coefficients then never reach global memory.
//
// Arithmetic.  T < 2^32 is any prime = 1 mod 2N; 2T need not fit 32 bits.  Values in LDS and in registers are canonical residues in 32-bit words;
// sums are formed in 64 bits, differences wrap mod 2^32 (a - b + T is exact for a < b), products are Shoup products: a table entry is the pair
// (w, floor(w 2^32 / T)), q = hi32(a w'), r = a w - q T in [0, 2T) as a 64-bit value, one conditional subtraction.  Nothing is lazy.
//
// The transform itself is the tile transform of tile_transform.h (one workgroup per tile of 2^logt points in LDS, one launch for N up to the LDS limit
// -- 2^15 words = 128 KiB, or 2^14 when the runtime grants no more than the default -- or a lowered limit, else two) on 32-bit words: 16 elements per
// thread, the register stages with four 16-byte LDS accesses each way.
// LDS layout: element l = 16 c + 4 u + e (chunk c, 16-byte unit u < 4) sits in unit u ^ f(c) of its chunk, f(c) = ((c >> 2) & 3) ^ (c & 2).
//   16-byte reads are served in four groups of 16 lanes ({0-3,12-15,20-27}, {4-11,16-19,28-31} and the same + 32) out of the 16 units of a 256-byte
//   bank row: lane c reads unit 4 (c & 3) + (u ^ f(c)); among the lanes of a group with equal c & 3 (c >> 2 is {0,3,5,6} or {1,2,4,7}) (c >> 2) & 3
//   takes four values and c & 2 is fixed: 16 units.  16-byte writes go in groups of 8 adjacent lanes out of 8 units (bank = dword mod 32): unit
//   4 (c & 1) + (u ^ f(c)); the four lanes with equal c & 1 have f = {j, j ^ 2, j ^ 1, j ^ 3}: 8 units.
//   The stage passes access single words, 32 adjacent lanes adjacent elements of a run of the span: conflict-free for spans >= 32 (f permutes
//   units inside a chunk); the one pass over the spans 32 and 16 of a contiguous tile puts two chunks of equal parity under 32 lanes: two-way.
#pragma once
#include "modarith.h"
#include "tile_pass.h"

namespace mkhe {

constexpr int BF_TILE_LOG_BIG = 15;     // largest tile: 2^15 words = 128 KiB of LDS, above the 64 KiB a kernel gets without asking
constexpr int BF_TILE_LOG_DEF = 14;     // largest tile when the request for more LDS is refused (64 KiB)
constexpr int BF_TILE_LOG_MULTI = 12;   // largest tile of the two-launch form (16 KiB: several workgroups per CU)
constexpr int BF_TILE_LOG_MIN = 10;     // smallest tile mkhe_ctx_set_bfv_tile accepts (N = 2^16 then has 2^6 rows: column tiles of 16 columns)

// constants of the plaintext modulus; x_s = floor(x 2^32 / T) is the Shoup companion of x
struct BfvT {
    u32 T, half;                // half = floor(T / 2)
    u32 qmod, qmod_s;           // Q mod T
    u32 qinv, qinv_s;           // Q^-1 mod T
    u32 hq;                     // floor(Q / 2) mod T
    u32 c32, c32_s;             // 2^32 mod T
    u32 one_s;                  // floor(2^32 / T): the companion of 1 (reduces a 32-bit word)
};
// what scale_up / scale_down need besides; all per limb l of Q
struct BfvScale {
    BfvT t;
    const Mod* mods;
    const u64* tinv_mont;       // [limbs]  MForm(T^-1 mod q_l)
    const u64* t_mont;          // [limbs]  MForm(T mod q_l)
    const u64* garner;          // [limbs][limbs]  Context::garner_table (limbs = nq)
    const uint2* qlt;           // [limbs]  (q_l mod T, companion)
    int limbs, N;
};

constexpr int BF_FUSE_NONE = 0, BF_FUSE_SCALE = 1, BF_FUSE_LIFT = 2;
struct BfvNtt {
    const u64* in;          // first launch: inverse: slots int64 [count][N]; forward: coeffs uint64 [count][N] (fuse: pt [count][limbs][N])
    u64* out;               // last launch: inverse: coeffs uint64 [count][N] (fuse: pt); forward: slots int64 [count][N]
    u32* work;              // [count][N], between the two launches
    u64* dig;               // fused forward: digit scratch [count][limbs][N]
    const uint2* w;         // [N/2]: omega^k (forward) / omega^-k (inverse) with companions
    const uint2* twist;     // [N]: psi^k (forward) / psi^-k N^-1 (inverse) with companions
    const u32* pos;         // [N]: slot index of position p
    TilePass p;             // logn = log2 N
    int fuse;               // single-launch only: BF_FUSE_SCALE = scale_down on the load (forward) / scale_up on the store (inverse);
                            // BF_FUSE_LIFT (inverse only) = the lift of launch_bf_lift on the store, out = ptmul [count][limbs][N]
    BfvScale sc;
};

// asks for BF_TILE_LOG_BIG tiles (dynamic LDS beyond the default limit); false: the runtime refused, keep to BF_TILE_LOG_DEF
bool bf_ntt_big_lds();
// inverse = slots_to_coeffs direction.  Launches N / 2^logt tiles per message.
void launch_bf_ntt(bool inverse, const BfvNtt& a, int count, hipStream_t st);

// ---- slot map (include/mkhe.h, "BFV slot map"; no reference counterpart): coeffs_out = slots_to_coeffs(map(coeffs_to_slots(coeffs_in))) for
// out_slot[i] = mult[i] * in_slot[index[i]] mod T.  After the forward stages position p holds slot pos[p], so in positions the map is
//     y[p] = mult[pos[p]] * x[src[p]],   src[p] = pos^-1[index[pos[p]]],
// and the prepared map (Context::bfv_slot_map_prepare) is one word per position: src[p] in the low 32 bits and, above it, the Shoup companion
// floor(m 2^32 / T) of m = mult[pos[p]] mod T.  The multiplier itself is not stored: m = ceil(companion * T / 2^32), one multiplication.  The kernels read
// position (word & (N - 1)) whatever the word holds, and write values below T whatever it holds.
struct BfvSlotMap {
    const u64* in;          // coeffs uint64 [count][N], any 64-bit value (taken mod T)
    u64* out;               // coeffs uint64 [count][N], < T; may be in
    const u64* map;         // [N], as above
    const uint2 *w, *winv;  // [N/2]: omega^k, omega^-k with companions
    const uint2 *twist, *itwist;    // [N]: psi^k, psi^-k N^-1 with companions
    int logn;
    BfvT t;
};
// single-workgroup form, N = 2^logn at most the tile: one launch, one workgroup per message, the transform pair and the gather on one tile in LDS
void launch_bf_slot_map(const BfvSlotMap& a, int count, hipStream_t st);
// two-launch form: dst[b][p] = src[b][map[p] & (n - 1)] * m_p mod T between the forward and the inverse launches, over the 32-bit work buffers
void launch_bf_slot_gather(const u32* src, u32* dst, const u64* map, int n, u32 T, int count, hipStream_t st);

// pt[b][l][n] = floor((Q m + floor(T/2)) / T) mod q_l =(floor(T/2) - r) T^-1 mod q_l, r = (Q m + floor(T/2)) mod T (Q = 0 mod q_l), m = coeffs[b][n] mod T.
// One thread per coefficient, looping over the limbs.
void launch_bf_scale_up(int count, const u64* coeffs, u64* pt, const BfvScale& sc, hipStream_t st);

// coeffs[b][n] = floor((T x + floor(Q/2)) / Q) mod T for x in [0, Q) given by the canonical residues pt[b][.][n], for EVERY x: r = (T x + floor(Q/2))
// mod Q limb by limb (floor(Q/2) = (q_l - 1) / 2 mod q_l as Q is odd), its mixed-radix (Garner) digits d_i into dig [count][limbs][N]
// (r = d_0 + d_1 q_0 + d_2 q_0 q_1 + ..), r mod T by Horner over the digits, result (floor(Q/2) - r) Q^-1 mod T.  No floating point.
void launch_bf_scale_down(int count, const u64* pt, u64* coeffs, u64* dig, const BfvScale& sc, hipStream_t st);


// ---- plaintext operands (include/mkhe.h, "BFV plaintext operands"; no reference counterpart)
// ptmul[b][l][n] = MForm(c mod q_l), c the centred representative of m = coeffs[b][n] mod T (c = m for m <= floor(T/2), else m - T): the
// multiplication plaintext in the coefficient domain, in the engine's 2^64 Montgomery form.  |c| is reduced by the Montgomery product itself
// (|c| 2^128 2^-64 mod q_l), so q_l may be smaller than T.  One thread per PAIR of coefficients (16-byte accesses), looping over the limbs.
void launch_bf_lift(int count, const u64* coeffs, u64* ptmul, const BfvScale& sc, hipStream_t st);

// w[z][l][n] = MRed(w[z][l][n], pt[(z / per_item) * pt_stride + l * N + n]) for npolys polynomials w of L limbs, in place: the NTT-domain product
// of every component of every ciphertext of a batch (per_item = 1 + k components each) with its prepared plaintext; pt_stride = 0: one
// plaintext for all.  pt is in Montgomery form, so the result is the plain canonical product.  The batch is grid.z: one launch.
void launch_bf_mul_prepared(u64* w, const u64* pt, long pt_stride, const Mod* mods, int L, int N, int per_item, int npolys, hipStream_t st);

}  // namespace mkhe
