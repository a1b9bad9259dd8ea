// encdec_kernels.h -- elementwise kernels of public-key encryption and of decryption: mkrlwe/encryptor.go:55-118 (the
// coefficient-domain branch :95-112) and mkrlwe/decryptor.go:26-66.  All HBM-streaming, two coefficients (16 bytes) per lane
// and access, per-modulus constants wave-uniform; the NTTs in between are the batched kernels of ntt_kernels.hip.  Every
// stored value is the canonical representative in [0, q).  Every kernel takes a leading batch count (grid.z).
//
// Two linearity arguments (the transforms are Z_q-linear, and a canonical residue is determined by its class):
//   Encrypt  the reference adds e0, e1 and the plaintext to InvNTT(u*pk) one ring.Add (CRed) at a time; any order of canonical
//            additions of the same summands gives the same residue.  A plaintext that arrives in the NTT domain is inverse-
//            transformed on its own (encryptor.go:107-109): here it rides in the same batched inverse NTT as the two slots.
//   Decrypt  the reference computes InvNTT(MRed(NTT(c_i), sk_i)) per party and adds the k results to c_0 (decryptor.go:31-41).
//            Summing the k products in the NTT domain and doing ONE inverse transform gives the same canonical residues:
//            InvNTT(sum_i x_i) = sum_i InvNTT(x_i) mod q.
#pragma once
#include "chacha.h"

namespace mkhe {

constexpr int ED_INLINE = 16;      // pointers per table that travel in the kernel arguments (F2_MAX_P parties); longer tables are staged on the device

// a table of per-item base pointers: entry i is dev ? dev[i] : p[i]
struct EdTable {
    const u64* p[ED_INLINE];
    const u64* const* dev;
};

// slots 0 / 1 of the work buffer w [3][count][limbs][N] <- MRed(MForm(uh), pk0), MRed(MForm(uh), pk1) with uh = w[2] = NTT(u)
// (encryptor.go:66-72); pk = [2][mtot][N], Q limbs 0 .. limbs-1 read.  pt_ntt != null (plaintexts [count][limbs][N] in the NTT domain):
// w[2] <- pt behind the read of uh, so that ONE inverse NTT of 3 * count polynomials follows; null: w[2] <- 0 (u does not linger).
void launch_encrypt_mul(int count, u64* w, const u64* pk, const u64* pt_ntt, const Mod* mods, int limbs, int mtot, int N, hipStream_t st);

// out[b] = ciphertext [2][limbs][N]: c0 = CRed(CRed(t0 + e0_q) + pt), c1 = CRed(t1 + e1_q) with t = w[0], w[1] after their inverse NTT,
// e_q = e >= 0 ? e : q - |e| expanded here from the int32 samples smp [count][3][N] (u, e0, e1), pt = pt_coeff [count][limbs][N] or,
// when that is null, w[2] (encryptor.go:96-110)
void launch_encrypt_finish(int count, const EdTable& out, const u64* w, const i32* smp, const u64* pt_coeff, const Mod* mods, int limbs, int N, hipStream_t st);

// acc[b][j][n] = sum_{i < k} MRed(ch[b*k + i][j][n], sk[b*k + i][j][n]) mod q_j, canonical: the k <= 32 products are summed as 128-bit integers
// and reduced once (decryptor.go:35 for every party at once).  ch: NTT of the party polynomials [limbs][N]; sk: Q limbs of the secrets.
void launch_decrypt_mac(int count, int k, u64* acc, const EdTable& ch, const EdTable& sk, const Mod* mods, int limbs, int N, hipStream_t st);

// out[b][j][n] = c0[b][j][n] + acc[b][j][n] after the inverse NTT of acc: one CRed (ring.Add, decryptor.go:41) or, with reduce, the canonical
// residue for any c0 <= 2q (ring.Reduce, decryptor.go:65).  Strides in words.
void launch_decrypt_finish(int count, u64* out, long out_stride, const u64* c0, long c0_stride, const u64* acc, const Mod* mods, int limbs, int N,
                           bool reduce, hipStream_t st);

// ---- small-norm samples from a ChaCha20 keystream (include/mkhe.h, "device-side sampling": the definition of the stream and of the kinds)
constexpr int SMP_MAX_CDT = 64;    // thresholds of a table (kind 1)
constexpr int SMP_KIND_ENCRYPT = 2;    // launch_small_sample only: polynomial p is kind (p % 3 != 0), the layout u, e0, e1 of mkhe_encrypt's samples
// Everything secret the kernel reads travels here, in the kernel arguments (StreamKey, chacha.h).
struct SmallSampleArgs : StreamKey {
    u32 first_stream;
    int ncdt;
    u64 cdt[SMP_MAX_CDT];
};
// out [polys][N] int32: polynomial p = stream first_stream + p of (key, nonce).  kind 0 / 1 for every polynomial, or SMP_KIND_ENCRYPT; with
// u_rows != null (SMP_KIND_ENCRYPT only) polynomial 3 b is stored a second time at u_rows [b][N]: the gathered rows small_expand reads.
// N is a multiple of 8; out and u_rows are 16-byte aligned.
void launch_small_sample(const SmallSampleArgs& a, int kind, int polys, i32* out, i32* u_rows, int N, hipStream_t st);

}  // namespace mkhe
