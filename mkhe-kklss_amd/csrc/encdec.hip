// encdec.hip -- Context methods for public-key encryption and decryption (mkrlwe/encryptor.go:55-118, mkrlwe/decryptor.go:26-66;
// mkckks/encryptor.go, mkckks/decryptor.go, mkbfv/encryptor.go and mkbfv/decryptor.go call exactly these).
//
// Ciphertexts of this engine are coefficient domain, so Encrypt is the reference's else branch (encryptor.go:95-112).  B plaintexts under
// one public key are ONE launch set over the work buffer w [3][B][L][N] (L = level + 1):
//   small_expand of the B polynomials u into w[2]; one forward NTT of B*L limbs; encrypt_mul (w[0], w[1] <- MForm(NTT(u)) * pk0, pk1);
//   one inverse NTT of 2*B*L limbs (3*B*L when the plaintexts arrive in the NTT domain: they ride along in w[2]); encrypt_finish.
// Decrypt of a ciphertext over k parties: ONE forward NTT of the k party polynomials, decrypt_mac (all k products summed in the NTT
// domain), one inverse NTT of a single polynomial, decrypt_finish.  PartialDecrypt is the same with k = 1 and a plain ring.Add at the end.
// The samples u, e0, e1 are drawn on the host (like the secrets and errors of key generation) or, in encrypt_seeded, on the device from a
// ChaCha20 keystream (small_sample_kernel); either way they are wiped from the device scratch behind their last use, and so is everything
// computed from u alone.
#include "engine.h"
#include "host_modarith.h"

namespace mkhe {

// v as a kernel-argument table, or -- longer than ED_INLINE -- staged at entry tab_offset of ed_tab_ (the caller has sized ed_tab_: one word per entry)
EdTable Context::ed_table(const std::vector<const u64*>& v, size_t tab_offset) {
    EdTable t{};
    if (v.size() <= (size_t)ED_INLINE) { for (size_t i = 0; i < v.size(); ++i) t.p[i] = v[i]; return t; }
    if (tab_offset + v.size() > ed_tab_.words) throw Error("mkhe: pointer table scratch too small");
    const u64** tab = reinterpret_cast<const u64**>(ed_tab_.p) + tab_offset;
    MKHE_HIP(hipMemcpyAsync(tab, v.data(), v.size() * sizeof(const u64*), hipMemcpyHostToDevice, stream));
    sync();                                             // v is pageable and about to go out of scope
    t.dev = tab;
    return t;
}

void Context::need_unmasked(const char* what) const {
    if (masked_) throw Error(std::string(what) + ": not available on a context that owns a subset of the moduli");
}

// Key-bearing arguments of one launch.  stream_fill writes the StreamKey every such struct derives from (the key words are zero when the launch
// reads no stream); wipe overwrites the host copy behind the launch (the runtime has copied the arguments).
static void stream_fill(StreamKey& a, const u32* key, u64 nonce, bool reads = true) {
    for (int i = 0; i < 8; ++i) a.key[i] = reads ? key[i] : 0;
    a.nonce_lo = (u32)nonce; a.nonce_hi = (u32)(nonce >> 32);
}
template <class T> static void wipe(T& a) {
    auto* p = reinterpret_cast<volatile unsigned char*>(&a);
    for (size_t i = 0; i < sizeof(a); ++i) p[i] = 0;
}
static void sample_args_fill(SmallSampleArgs& a, const u32* key, u64 nonce, u32 first_stream, const u64* cdt, int ncdt) {
    stream_fill(a, key, nonce);
    a.first_stream = first_stream; a.ncdt = ncdt;
    for (int t = 0; t < SMP_MAX_CDT; ++t) a.cdt[t] = t < ncdt ? cdt[t] : ~0ull;
}

void Context::encrypt(int level, int count, const u64* pk, const u64* pt, bool pt_is_ntt, const int32_t* samples, u64* const* outs) {
    check_level(level);
    need_unmasked("mkhe_encrypt");
    const int L = level + 1;
    const size_t pw = (size_t)count * L * N, sn = (size_t)count * N;
    u64* w = scratch(ed_w_, 3 * pw);
    int32_t* small = reinterpret_cast<int32_t*>(scratch(ed_small_, 2 * sn));          // 4 sn int32 (N is even)
    scratch(ed_tab_, (size_t)count);
    const EdTable ot = ed_table(std::vector<const u64*>(outs, outs + count), 0);
    // the samples as given, [count][3][N], for encrypt_finish; behind them the count rows of u gathered into [count][N] for small_expand
    int32_t* du = small + 3 * sn;
    MKHE_HIP(hipMemcpyAsync(small, samples, 3 * sn * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    MKHE_HIP(hipMemcpy2DAsync(du, (size_t)N * sizeof(int32_t), samples, 3 * (size_t)N * sizeof(int32_t), (size_t)N * sizeof(int32_t), count,
                              hipMemcpyHostToDevice, stream));
    sync();                                             // the host array may be pageable: do not return before it is consumed
    encrypt_core(level, count, pk, pt, pt_is_ntt, w, small, ot);
}

void Context::encrypt_core(int level, int count, const u64* pk, const u64* pt, bool pt_is_ntt, u64* w, int32_t* small, const EdTable& ot) {
    const int L = level + 1;
    const size_t pw = (size_t)count * L * N, sn = (size_t)count * N;
    int32_t* du = small + 3 * sn;
    {
        ProfScope ps(this, PROF_OTHER, (double)count * N * (4.0 + 8.0 * L));
        launch_small_expand(w + 2 * pw, du, d_mods, count, L, N, s_);
    }
    MKHE_HIP(hipMemsetAsync(du, 0, sn * sizeof(int32_t), s_));
    ntt(w + 2 * pw, w + 2 * pw, count, L, 0, false, false);
    {
        ProfScope ps(this, PROF_OTHER, 8.0 * N * L * (count * (pt_is_ntt ? 5.0 : 4.0) + 2.0));
        launch_encrypt_mul(count, w, pk, pt_is_ntt ? pt : nullptr, d_mods, L, mtot, N, s_);
    }
    ntt(w, w, (pt_is_ntt ? 3 : 2) * count, L, 0, true, false);
    {
        ProfScope ps(this, PROF_OTHER, (double)count * N * (8.0 + 8.0 * L * 5.0));
        launch_encrypt_finish(count, ot, w, small, pt_is_ntt ? nullptr : pt, d_mods, L, N, s_);
    }
    MKHE_HIP(hipMemsetAsync(small, 0, 3 * sn * sizeof(int32_t), s_));
    MKHE_HIP(hipMemsetAsync(w, 0, 2 * pw * sizeof(u64), s_));             // u * pk1 gives u away: it does not outlive the call
    MKHE_HIP(hipGetLastError());
}

// u, e0, e1 of count encryptions from the keystream, then encrypt_core.  The sampler writes [count][3][N] straight into small and, in the same
// launch, the rows of u a second time behind it (the layout the two copies of encrypt() produce): no upload, no extra launch, and nothing for the
// host to wait for.
void Context::encrypt_sampled(int level, int count, const u64* pk, const u64* pt, bool pt_is_ntt, const u32* key, u64 nonce, const u64* cdt, int ncdt,
                              u64* w, int32_t* small, const EdTable& ot) {
    SmallSampleArgs a;
    sample_args_fill(a, key, nonce, 0, cdt, ncdt);
    {
        ProfScope ps(this, PROF_OTHER, 16.0 * count * N);
        launch_small_sample(a, SMP_KIND_ENCRYPT, 3 * count, small, small + 3 * (size_t)count * N, N, s_);
    }
    wipe(a);
    encrypt_core(level, count, pk, pt, pt_is_ntt, w, small, ot);
}

void Context::sample_small(int kind, int count, const u32* key, u64 nonce, u32 first_stream, const u64* cdt, int ncdt, int32_t* dev_out) {
    need_unmasked("mkhe_sample_small");
    SmallSampleArgs a;
    sample_args_fill(a, key, nonce, first_stream, kind == 1 ? cdt : nullptr, kind == 1 ? ncdt : 0);
    {
        ProfScope ps(this, PROF_OTHER, 4.0 * count * N);
        launch_small_sample(a, kind, count, dev_out, nullptr, N, s_);
    }
    wipe(a);
    MKHE_HIP(hipGetLastError());
}

void Context::encrypt_seeded(int level, int count, const u64* pk, const u64* pt, bool pt_is_ntt, const u32* key, u64 nonce, const u64* cdt, int ncdt,
                             u64* const* outs) {
    check_level(level);
    need_unmasked("mkhe_encrypt_seeded");
    const int L = level + 1;
    const size_t pw = (size_t)count * L * N, sn = (size_t)count * N;
    u64* w = scratch(ed_w_, 3 * pw);
    int32_t* small = reinterpret_cast<int32_t*>(scratch(ed_small_, 2 * sn));
    scratch(ed_tab_, (size_t)count);
    const EdTable ot = ed_table(std::vector<const u64*>(outs, outs + count), 0);     // count > ED_INLINE: staged, which synchronises
    encrypt_sampled(level, count, pk, pt, pt_is_ntt, key, nonce, cdt, ncdt, w, small, ot);
}

// acc [limbs][N] <- sum_i NTT-domain products of the k polynomials at ch [k][limbs][N] with the secrets sks[i]
void Context::ed_mac(int k, const u64* ch, const u64* const* sks, int limbs, u64* acc) {
    std::vector<const u64*> c(k), s(sks, sks + k);
    for (int i = 0; i < k; ++i) c[i] = ch + (size_t)i * limbs * N;
    scratch(ed_tab_, 2 * (size_t)k);
    const EdTable ct = ed_table(c, 0), st = ed_table(s, (size_t)k);
    ProfScope ps(this, PROF_OTHER, 8.0 * N * limbs * (2.0 * k + 1.0));
    launch_decrypt_mac(1, k, acc, ct, st, d_mods, limbs, N, s_);
}

void Context::partial_decrypt(const Ct& in, int slot, const u64* sk, Ct& out) {
    need_unmasked("mkhe_partial_decrypt");
    if (slot < 1 || slot > in.n) throw Error("mkhe_partial_decrypt: slot out of range (party slots are 1 .. n)");
    if (out.limbs != in.limbs) throw Error("mkhe_partial_decrypt: out must be at the level of in");
    std::vector<int> rest(in.ids);
    rest.erase(rest.begin() + (slot - 1));
    if (out.n != in.n - 1 || out.ids != rest) throw Error("mkhe_partial_decrypt: out must be over the ids of in without the one at slot");
    const int L = in.limbs;
    const size_t pw = (size_t)L * N;
    u64* w = scratch(ed_w_, 2 * pw);
    ntt(in.d + (size_t)slot * pw, w, 1, L, 0, false, false);
    ed_mac(1, w, &sk, L, w + pw);
    ntt(w + pw, w + pw, 1, L, 0, true, false);
    {
        ProfScope ps(this, PROF_OTHER, 24.0 * N * L);
        launch_decrypt_finish(1, out.d, 0, in.d, 0, w + pw, d_mods, L, N, false, s_);
    }
    if (slot > 1) MKHE_HIP(hipMemcpyAsync(out.d + pw, in.d + pw, (size_t)(slot - 1) * pw * sizeof(u64), hipMemcpyDeviceToDevice, s_));
    if (slot < in.n) MKHE_HIP(hipMemcpyAsync(out.d + (size_t)slot * pw, in.d + (size_t)(slot + 1) * pw, (size_t)(in.n - slot) * pw * sizeof(u64),
                                             hipMemcpyDeviceToDevice, s_));
    MKHE_HIP(hipMemsetAsync(w + pw, 0, pw * sizeof(u64), s_));            // the decryption share stays in the caller's ciphertext only
    MKHE_HIP(hipGetLastError());
}

void Context::decrypt(const Ct& ct, const u64* const* sks, u64* pt_out) {
    need_unmasked("mkhe_decrypt");
    const int k = ct.n, L = ct.limbs;
    const size_t pw = (size_t)L * N;
    u64* w = scratch(ed_w_, (size_t)(k + 1) * pw);
    u64* acc = w + (size_t)k * pw;
    if (k > 0) {
        ntt(ct.d + pw, w, k, L, 0, false, false);
        ed_mac(k, w, sks, L, acc);
        ntt(acc, acc, 1, L, 0, true, false);
    } else MKHE_HIP(hipMemsetAsync(acc, 0, pw * sizeof(u64), s_));
    {
        ProfScope ps(this, PROF_OTHER, 24.0 * N * L);
        launch_decrypt_finish(1, pt_out, 0, ct.d, 0, acc, d_mods, L, N, true, s_);
    }
    MKHE_HIP(hipMemsetAsync(acc, 0, pw * sizeof(u64), s_));
    MKHE_HIP(hipGetLastError());
}

// ---- distributed decryption.  A share is PartialDecrypt's product with the flooding noise added before it leaves the scratch: one launch set
// for count ciphertexts -- the forward NTT gathers polynomial slots[b] of every input into w [count][L][N], decrypt_mac (k = 1) and the inverse
// NTT run in place, share_finish_kernel adds e_b and writes the caller's buffer.  The unflooded product c_i * s_i gives the key away (c_i is
// public): it is wiped from w behind the finish kernel.
void Context::share_product(const std::vector<const Ct*>& ins, const int* slots, const u64* sk, u64* w) {
    const int count = (int)ins.size(), L = ins[0]->limbs;
    const size_t pw = (size_t)L * N;
    scratch(ed_tab_, 2 * (size_t)count);
    std::vector<const u64*> c(count), s(count, sk);
    for (int b = 0; b < count; ++b) c[b] = w + (size_t)b * pw;
    const EdTable ct = ed_table(c, 0), st = ed_table(s, (size_t)count);    // count > ED_INLINE: staged, which synchronises
    share_gather_ntt(ins, slots, w);
    {
        ProfScope ps(this, PROF_OTHER, 24.0 * N * L * count);
        launch_decrypt_mac(count, 1, w, ct, st, d_mods, L, N, s_);
    }
    ntt(w, w, count, L, 0, true, false);
}

void Context::share_gather_ntt(const std::vector<const Ct*>& ins, const int* slots, u64* w) {
    const int count = (int)ins.size(), L = ins[0]->limbs;
    std::vector<const u64*> src(count);
    for (int b = 0; b < count; ++b) src[b] = ins[b]->d + (size_t)slots[b] * L * N;
    gather_ntt(src, L, w);
}

void Context::gather_ntt(const std::vector<const u64*>& src, int L, u64* w) {
    const size_t pw = (size_t)L * N;
    std::vector<u64*> dst(src.size());
    for (size_t b = 0; b < dst.size(); ++b) dst[b] = w + b * pw;
    ntt_items(false, src, (long)pw, dst, (long)pw, 1, L);
}

void Context::decrypt_share(const std::vector<const Ct*>& ins, const int* slots, const u64* sk, const u32* key, u64 nonce, int bits, u64* shares) {
    need_unmasked("mkhe_decrypt_share");
    const int count = (int)ins.size(), L = ins[0]->limbs;
    const size_t pw = (size_t)L * N;
    u64* w = scratch(ed_w_, (size_t)count * pw);
    share_product(ins, slots, sk, w);
    ShareFloodArgs a;
    stream_fill(a, key, nonce, bits > 0);
    a.bits = bits;
    {
        ProfScope ps(this, PROF_OTHER, 16.0 * N * L * count);
        // one limb per grid row: the ChaCha20 block is recomputed per limb, and every launch has limbs times the waves (profiles/README.md)
        launch_share_finish(a, count, shares, w, d_mods, L, MKHE_AB_INT("MKHE_SHARE_ROWS", L), N, s_);
    }
    wipe(a);
    MKHE_HIP(hipMemsetAsync(w, 0, (size_t)count * pw * sizeof(u64), s_));
    MKHE_HIP(hipGetLastError());
}

void Context::decrypt_merge(const std::vector<const Ct*>& ins, const std::vector<const u64*>& shares, u64* pt) {
    need_unmasked("mkhe_decrypt_merge");
    const int count = (int)ins.size(), L = ins[0]->limbs;
    std::vector<const u64*> c(count);
    for (int b = 0; b < count; ++b) c[b] = ins[b]->d;
    scratch(ed_tab_, (size_t)count + shares.size());
    const EdTable ct = ed_table(c, 0), st = ed_table(shares, (size_t)count);
    {
        ProfScope ps(this, PROF_OTHER, 8.0 * N * L * count * (2.0 + (double)shares.size()));
        launch_share_merge(count, (int)shares.size(), pt, ct, st, d_mods, L, N, s_);
    }
    MKHE_HIP(hipGetLastError());
}

// ---- collective refresh.  The party side is the share chain with refresh_finish_kernel in the place of share_finish_kernel, then the chain of
// encrypt_seeded on the plaintext -M that kernel left in the scratch.  ed_w_ holds, in this order, the work buffer of encrypt_core
// [3][count][Lout][N], the plaintext [count][Lout][N] and the product [count][Lin][N]; ed_tab_ the two tables of the product and the outputs'.
// Sized once, in front: a scratch that grows moves.  The product, the plaintext and the samples are wiped behind their last use.
// finish(prod, pt) launches the kernel that turns the product into the public share and the plaintext; finish_bytes is what its ProfScope counts
template <class F> void Context::refresh_share_chain(const std::vector<const Ct*>& ins, const int* slots, const u64* sk, const u64* pk, const u32* key,
                                                     u64 nonce_enc, const u64* cdt, int ncdt, int lout, u64* const* outs, double finish_bytes, F finish) {
    const int count = (int)ins.size(), lin = ins[0]->limbs;
    const size_t pin = (size_t)count * lin * N, pout = (size_t)count * lout * N, sn = (size_t)count * N;
    u64* w = scratch(ed_w_, 4 * pout + pin);
    u64 *pt = w + 3 * pout, *prod = pt + pout;
    int32_t* small = reinterpret_cast<int32_t*>(scratch(ed_small_, 2 * sn));
    scratch(ed_tab_, 3 * (size_t)count);
    const EdTable ot = ed_table(std::vector<const u64*>(outs, outs + count), 2 * (size_t)count);
    share_product(ins, slots, sk, prod);
    {
        ProfScope ps(this, PROF_OTHER, finish_bytes);
        finish(prod, pt);
    }
    MKHE_HIP(hipMemsetAsync(prod, 0, pin * sizeof(u64), s_));
    encrypt_sampled(lout - 1, count, pk, pt, false, key, nonce_enc, cdt, ncdt, w, small, ot);      // wipes the samples and u * pk
    MKHE_HIP(hipMemsetAsync(pt, 0, pout * sizeof(u64), s_));                // the plaintext with the public share gives the product away
    MKHE_HIP(hipGetLastError());
}

void Context::refresh_share(const std::vector<const Ct*>& ins, const int* slots, const u64* sk, const u64* pk, const u32* key, u64 nonce_mask,
                            u64 nonce_enc, int bits, const u64* cdt, int ncdt, u64* shares, int lout, u64* const* outs) {
    need_unmasked("mkhe_refresh_share");
    check_level(lout - 1);
    const int count = (int)ins.size(), lin = ins[0]->limbs;
    refresh_share_chain(ins, slots, sk, pk, key, nonce_enc, cdt, ncdt, lout, outs, 8.0 * N * count * (2.0 * lin + lout), [&](u64* prod, u64* pt) {
        RefreshMaskArgs m;
        stream_fill(m, key, nonce_mask, bits > 0);
        m.bits = bits;
        launch_refresh_finish(m, count, shares, prod, pt, d_mods, lin, lout, N, s_);
        wipe(m);
    });
}

// ---- encryption to shares (include/mkhe.h, "encryption to shares"): the share chain of the refresh with its seam open.  The same product, the same
// finish kernel -- which writes the plaintext -M into the CALLER's buffer, the party's additive share, instead of the scratch -- and no encryption.
// Only the unmasked product is the engine's to wipe.
void Context::e2s_share(const std::vector<const Ct*>& ins, const int* slots, const u64* sk, const u32* key, u64 nonce_mask, int bits, u64* shares,
                        int secret_limbs, u64* secret) {
    need_unmasked("mkhe_e2s_share");
    check_level(secret_limbs - 1);
    const int count = (int)ins.size(), lin = ins[0]->limbs;
    const size_t pin = (size_t)count * lin * N;
    u64* prod = scratch(ed_w_, pin);
    share_product(ins, slots, sk, prod);
    RefreshMaskArgs m;
    stream_fill(m, key, nonce_mask, bits > 0);
    m.bits = bits;
    {
        ProfScope ps(this, PROF_OTHER, 8.0 * N * count * (2.0 * lin + secret_limbs));
        launch_refresh_finish(m, count, shares, prod, secret, d_mods, lin, secret_limbs, N, s_);
    }
    wipe(m);
    MKHE_HIP(hipMemsetAsync(prod, 0, pin * sizeof(u64), s_));
    MKHE_HIP(hipGetLastError());
}

// the pointer tables of a merge in ed_tab_: [outs][polynomial 0 of ins][shares][reenc]
Context::MergeTables Context::merge_tables(const std::vector<const Ct*>& ins, const std::vector<const u64*>& shares, const std::vector<const u64*>& reenc,
                                           u64* const* outs) {
    const size_t count = ins.size(), k = shares.size();
    std::vector<const u64*> c(count);
    for (size_t b = 0; b < count; ++b) c[b] = ins[b]->d;
    scratch(ed_tab_, 2 * count + k + reenc.size());
    MergeTables t;
    t.ot = ed_table(std::vector<const u64*>(outs, outs + count), 0); t.ct = ed_table(c, count);     // count or nshares > ED_INLINE: staged, which synchronises
    t.st = ed_table(shares, 2 * count); t.rt = ed_table(reenc, 2 * count + k);
    return t;
}

void Context::refresh_merge(const std::vector<const Ct*>& ins, const std::vector<const u64*>& shares, const std::vector<const u64*>& reenc, int lout,
                            u64* const* outs) {
    need_unmasked("mkhe_refresh_merge");
    refresh_merge_launch(ins, shares, reenc, lout, outs);
}

// E2S, anyone's side: the merge of the refresh without its re-encryptions -- R~ alone into pt [count][lout][N]
void Context::e2s_merge(const std::vector<const Ct*>& ins, const std::vector<const u64*>& shares, int lout, u64* pt) {
    need_unmasked("mkhe_e2s_merge");
    std::vector<u64*> o(ins.size());
    for (size_t b = 0; b < o.size(); ++b) o[b] = pt + b * (size_t)lout * N;
    refresh_merge_launch(ins, shares, {}, lout, o.data());
}

// reenc empty: no re-encryption is added and outs[b] is the one polynomial [lout][N]
void Context::refresh_merge_launch(const std::vector<const Ct*>& ins, const std::vector<const u64*>& shares, const std::vector<const u64*>& reenc, int lout,
                                   u64* const* outs) {
    check_level(lout - 1);
    const int count = (int)ins.size(), lin = ins[0]->limbs, k = (int)shares.size();
    if (!d_rf_tab_) {
        std::vector<u64> t(2 * (size_t)nq * nq, 0);
        for (int j = 0; j < nq; ++j) {
            u64 prod = 1;
            for (int i = 0; i < nq; ++i) {
                t[(size_t)i * nq + j] = to_mont(moduli[i] % moduli[j], moduli[j]);
                prod = mulmod(prod, moduli[i] % moduli[j], moduli[j]);
                t[(size_t)(nq + i) * nq + j] = prod;
            }
        }
        garner_table();
        d_rf_tab_ = mem_.upload(t);
    }
    RefreshMergeArgs a;
    a.garner = garner_table(); a.qmont = d_rf_tab_; a.qprod = d_rf_tab_ + (size_t)nq * nq;
    a.dig = scratch(rf_dig_, (size_t)count * lin * N);
    a.mods = d_mods; a.nq = nq; a.lin = lin; a.lout = lout; a.nshares = k; a.count = count; a.N = N;
    a.nre = reenc.empty() ? 0 : k;
    const MergeTables t = merge_tables(ins, shares, reenc, outs);
    {
        ProfScope ps(this, PROF_OTHER, 8.0 * N * count * (lin * (1.0 + k) + (lout > lin ? 2.0 * lin : 0.0) + lout * (1.0 + 3.0 * a.nre)));
        launch_refresh_merge(a, t.ot, t.ct, t.st, t.rt, s_);
    }
    MKHE_HIP(hipGetLastError());
}

// ---- collective refresh for MK-BFV: the same two chains at the maximum level (Lin = Lout = nq), with bfv_refresh_finish_kernel behind the product
// and bfv_refresh_merge_kernel as the merge.  The scaling tables are the encoder's (bf_init); ed_w_ and ed_tab_ are laid out as in refresh_share.
int Context::flood_room(int limbs, u64 t) const {
    // Q div 2 T in 32-bit words, little endian: the product of the moduli, then one long division (2 T < 2^33)
    std::vector<u32> w{1};
    for (int l = 0; l < limbs; ++l) {
        const u64 m[2] = {moduli[l] & 0xffffffffull, moduli[l] >> 32};
        std::vector<u32> r(w.size() + 2, 0);
        for (int h = 0; h < 2; ++h) {
            u64 carry = 0;
            for (size_t i = 0; i < w.size(); ++i) {
                const u64 t = (u64)w[i] * m[h] + r[i + h] + carry;
                r[i + h] = (u32)t;
                carry = t >> 32;
            }
            r[w.size() + h] += (u32)carry;          // (the word is still zero in the first round and takes no carry out in the second: the product fits)
        }
        w.swap(r);
    }
    const unsigned __int128 d = 2 * (unsigned __int128)t;
    unsigned __int128 rem = 0;
    int bits = 0;
    for (size_t i = w.size(); i-- > 0;) {
        rem = (rem << 32) | w[i];
        const u32 qd = (u32)(rem / d);
        rem %= d;
        if (!bits && qd) bits = (int)i * 32 + (64 - __builtin_clzll((u64)qd));
    }
    return bits - 1;
}

void Context::bfv_refresh_share(const std::vector<const Ct*>& ins, const int* slots, const u64* sk, const u64* pk, const u32* key, u64 nonce_mask,
                                u64 nonce_enc, int mask, int flood_bits, const u64* cdt, int ncdt, u64* shares, u64* const* outs) {
    bf_init("mkhe_bfv_refresh_share");
    const int count = (int)ins.size(), W = (flood_bits + 63) / 64;
    refresh_share_chain(ins, slots, sk, pk, key, nonce_enc, cdt, ncdt, nq, outs, 24.0 * N * count * nq + 64.0 * (N / 8) * count * nq * (2.0 + W),
                        [&](u64* prod, u64* pt) {
        BfvRefreshArgs m;
        stream_fill(m, key, nonce_mask, mask || flood_bits > 0);
        m.mask = mask; m.flood_bits = flood_bits;
        launch_bfv_refresh_finish(m, count, shares, prod, pt, bf_scale(), s_);
        wipe(m);
    });
}

// E2S for MK-BFV: the same chain with bfv_e2s_finish_kernel, the SECRET variant of bfv_refresh_finish_kernel's body, which writes (T - A) mod T over Z_T into the caller's buffer
void Context::bfv_e2s_share(const std::vector<const Ct*>& ins, const int* slots, const u64* sk, const u32* key, u64 nonce_mask, int flood_bits, u64* shares,
                            u64* secret) {
    bf_init("mkhe_bfv_e2s_share");
    const int count = (int)ins.size(), W = (flood_bits + 63) / 64;
    const size_t pin = (size_t)count * nq * N;
    u64* prod = scratch(ed_w_, pin);
    share_product(ins, slots, sk, prod);
    BfvRefreshArgs m;
    stream_fill(m, key, nonce_mask);
    m.mask = 1; m.flood_bits = flood_bits;
    {
        ProfScope ps(this, PROF_OTHER, 16.0 * N * count * nq + 8.0 * N * count + 64.0 * (N / 8) * count * nq * (2.0 + W));
        launch_bfv_e2s_finish(m, count, shares, prod, secret, bf_scale(), s_);
    }
    wipe(m);
    MKHE_HIP(hipMemsetAsync(prod, 0, pin * sizeof(u64), s_));
    MKHE_HIP(hipGetLastError());
}

void Context::bfv_refresh_merge(const std::vector<const Ct*>& ins, const std::vector<const u64*>& shares, const std::vector<const u64*>& reenc,
                                u64* const* outs) {
    bf_init("mkhe_bfv_refresh_merge");
    const int count = (int)ins.size(), k = (int)shares.size();
    u64* dig = scratch(rf_dig_, (size_t)count * nq * N);
    const MergeTables t = merge_tables(ins, shares, reenc, outs);
    {
        // every digit is written once and read by each later limb and by the sum
        ProfScope ps(this, PROF_OTHER, 8.0 * N * count * nq * ((1.0 + k) + (2.0 + (nq - 1) / 2.0) + (1.0 + 3.0 * k)));
        launch_bfv_refresh_merge(count, k, dig, bf_scale(), t.ot, t.ct, t.st, t.rt, s_);
    }
    MKHE_HIP(hipGetLastError());
}

// ---- collective key switch to a recipient's public key.  One launch set over the work buffer w [3][count][L][N]: u sampled (kind 0) into
// ed_small_, small_expand into w[2] and its forward NTT; the gathering forward NTT of the c_slot into w[0]; pcks_mac (w[0] <- c^ sk + u^ pk0,
// w[1] <- u^ pk1, w[2] <- 0); one inverse NTT of 2 count polynomials; pcks_finish adds the flood and e1 from registers and writes the caller's
// buffer.  No pointer table: nothing is staged and the call never waits for the host.  c_i s_i gives the key away and u pk1 gives u away: the int32
// u, w[0] and w[1] are wiped behind their last use (w[2] by the product kernel).
void Context::pcks_share(const std::vector<const Ct*>& ins, const int* slots, const u64* sk, const u64* pk, const u32* key, u64 nonce, int flood_bits,
                         const u64* cdt, int ncdt, u64* shares) {
    need_unmasked("mkhe_pcks_share");
    const int count = (int)ins.size(), L = ins[0]->limbs;
    const size_t pw = (size_t)count * L * N, sn = (size_t)count * N;
    u64* w = scratch(ed_w_, 3 * pw);
    int32_t* du = reinterpret_cast<int32_t*>(scratch(ed_small_, (sn + 1) / 2));
    SmallSampleArgs a;
    sample_args_fill(a, key, nonce, 0, cdt, ncdt);
    {
        ProfScope ps(this, PROF_OTHER, 4.0 * count * N);
        launch_small_sample(a, 0, count, du, nullptr, N, s_);
    }
    {
        ProfScope ps(this, PROF_OTHER, (double)count * N * (4.0 + 8.0 * L));
        launch_small_expand(w + 2 * pw, du, d_mods, count, L, N, s_);
    }
    MKHE_HIP(hipMemsetAsync(du, 0, sn * sizeof(int32_t), s_));
    ntt(w + 2 * pw, w + 2 * pw, count, L, 0, false, false);
    share_gather_ntt(ins, slots, w);
    {
        ProfScope ps(this, PROF_OTHER, 8.0 * N * L * (count * 5.0 + 3.0));
        launch_pcks_mac(count, w, sk, pk, d_mods, L, mtot, N, s_);
    }
    ntt(w, w, 2 * count, L, 0, true, false);
    {
        const int W = (flood_bits + 63) / 64;
        ProfScope ps(this, PROF_OTHER, 32.0 * N * L * count + 64.0 * (N / 8) * count * L * (1.0 + W));
        launch_pcks_finish(a, flood_bits, count, shares, w, d_mods, L, N, s_);
    }
    wipe(a);
    MKHE_HIP(hipMemsetAsync(w, 0, 2 * pw * sizeof(u64), s_));
    MKHE_HIP(hipGetLastError());
}

void Context::pcks_merge(const std::vector<const Ct*>& ins, const std::vector<const u64*>& shares, u64* const* outs) {
    need_unmasked("mkhe_pcks_merge");
    const int count = (int)ins.size(), L = ins[0]->limbs;
    const MergeTables t = merge_tables(ins, shares, {}, outs);
    {
        ProfScope ps(this, PROF_OTHER, 8.0 * N * L * count * (3.0 + 2.0 * (double)shares.size()));
        launch_pcks_merge(count, (int)shares.size(), t.ot, t.ct, t.st, d_mods, L, N, s_);
    }
    MKHE_HIP(hipGetLastError());
}

// ---- secret-key encryption with a seeded c1 (include/mkhe.h; skenc_kernels.h).  One launch set whatever count is: uniform_sample writes a_b
// straight into polynomial 1 of outs[b]; the gathering forward NTT reads it into w [count][L][N]; skenc_mul (w <- w * sk, or pt - w * sk for a
// plaintext in the NTT domain); one inverse NTT; skenc_finish writes polynomial 0.  NTT(c1) * s gives s away (c1 is public and invertible with
// overwhelming probability): w, and the staged e of the host-sample call, are wiped behind the finish kernel.
void Context::sample_uniform(int limbs, int count, const u32* key, u64 nonce, u64* dev_out) {
    need_unmasked("mkhe_sample_uniform");
    std::vector<const u64*> o(count);
    for (int b = 0; b < count; ++b) o[b] = dev_out + (size_t)b * limbs * N;
    scratch(ed_tab_, (size_t)count);
    const EdTable ot = ed_table(o, 0);                                      // count > ED_INLINE: staged, which synchronises
    UniformArgs a;
    stream_fill(a, key, nonce);
    {
        ProfScope ps(this, PROF_OTHER, 8.0 * count * limbs * N);
        launch_uniform_sample(a, count, ot, 0, d_mods, limbs, nq, N, s_);
    }
    MKHE_HIP(hipGetLastError());
}

void Context::ct_expand_seeded(int count, int limbs, const u32* key, u64 nonce, u64* const* outs) {
    need_unmasked("mkhe_ct_expand_seeded");
    scratch(ed_tab_, (size_t)count);
    const EdTable ot = ed_table(std::vector<const u64*>(outs, outs + count), 0);
    UniformArgs a;
    stream_fill(a, key, nonce);
    {
        ProfScope ps(this, PROF_OTHER, 8.0 * count * limbs * N);
        launch_uniform_sample(a, count, ot, (long)limbs * N, d_mods, limbs, nq, N, s_);
    }
    MKHE_HIP(hipGetLastError());
}

void Context::encrypt_sk(int level, int count, const u64* sk, const u64* pt, bool pt_is_ntt, const u32* a_key, u64 a_nonce, const int32_t* e,
                         const u32* e_key, u64 e_nonce, const u64* cdt, int ncdt, u64* const* outs, const char* what) {
    check_level(level);
    need_unmasked(what);
    const int L = level + 1;
    const size_t pw = (size_t)count * L * N, sn = (size_t)count * N;
    u64* w = scratch(ed_w_, pw);
    int32_t* small = e ? reinterpret_cast<int32_t*>(scratch(ed_small_, (sn + 1) / 2)) : nullptr;
    scratch(ed_tab_, (size_t)count);
    const std::vector<const u64*> o(outs, outs + count);
    const EdTable ot = ed_table(o, 0);                                      // count > ED_INLINE: staged, which synchronises
    if (e) {
        MKHE_HIP(hipMemcpyAsync(small, e, sn * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        sync();                                                             // the host array may be pageable: do not return before it is consumed
    }
    UniformArgs ua;
    stream_fill(ua, a_key, a_nonce);
    {
        ProfScope ps(this, PROF_OTHER, 8.0 * count * L * N);
        launch_uniform_sample(ua, count, ot, (long)L * N, d_mods, L, nq, N, s_);
    }
    std::vector<const u64*> c1(count);
    for (int b = 0; b < count; ++b) c1[b] = o[b] + (size_t)L * N;
    gather_ntt(c1, L, w);
    {
        ProfScope ps(this, PROF_OTHER, 8.0 * N * L * (count * (pt_is_ntt ? 3.0 : 2.0) + 1.0));
        launch_skenc_mul(count, w, sk, pt_is_ntt ? pt : nullptr, d_mods, L, N, s_);
    }
    ntt(w, w, count, L, 0, true, false);
    SmallSampleArgs a{};                                                    // (not read when the samples are in memory)
    if (!e) sample_args_fill(a, e_key, e_nonce, 0, cdt, ncdt);
    {
        ProfScope ps(this, PROF_OTHER, (double)count * N * L * (pt_is_ntt ? 16.0 : 24.0) + (e ? 4.0 * count * N * L : 64.0 * (N / 8) * count * L));
        launch_skenc_finish(a, small, count, ot, w, pt_is_ntt ? nullptr : pt, d_mods, L, N, s_);
    }
    wipe(a);
    if (e) MKHE_HIP(hipMemsetAsync(small, 0, sn * sizeof(int32_t), s_));
    MKHE_HIP(hipMemsetAsync(w, 0, pw * sizeof(u64), s_));
    MKHE_HIP(hipGetLastError());
}

// ---- threshold secret keys (include/mkhe.h; threshold_kernels.h).  Three single launches.  Shares and additive keys are key material of the
// caller's, written to the caller's buffers only: the engine has no scratch to wipe here, and the key of kind 7 is overwritten behind its launch.
void Context::threshold_gen_shares(const u64* sk, int t, int n, const u32* points, const u32* key, u64 nonce, u64* const* outs) {
    need_unmasked("mkhe_threshold_gen_shares");
    ThresholdShareArgs a{};
    stream_fill(a, key, nonce, t > 1);
    a.t = t; a.n = n;
    for (int p = 0; p < n; ++p) { a.x[p] = points[p]; a.out[p] = outs[p]; }
    {
        // S once per group of points, every share once; 2 (t - 1) ChaCha20 blocks per thread and group
        const double groups = (double)((n + THR_G - 1) / THR_G);
        ProfScope ps(this, PROF_OTHER, 8.0 * N * mtot * (groups + n));
        launch_threshold_share(a, sk, d_mods, mtot, N, s_);
    }
    wipe(a);
    MKHE_HIP(hipGetLastError());
}

void Context::threshold_additive_key(const u64* share, u32 point, int nactive, const u32* active, u64* out) {
    need_unmasked("mkhe_threshold_additive_key");
    ThresholdScaleArgs a{};
    for (int j = 0; j < mtot; ++j) {
        const u64 m = moduli[j];
        u64 num = 1, den = 1;
        for (int i = 0; i < nactive; ++i) {
            if (active[i] == point) continue;
            num = mulmod(num, active[i], m);
            den = mulmod(den, (active[i] + m - point) % m, m);
        }
        a.lam[j] = to_mont(mulmod(num, powmod(den, m - 2, m), m), m);        // m is prime and den a unit: the points are distinct and below m
    }
    {
        ProfScope ps(this, PROF_OTHER, 16.0 * N * mtot);
        launch_threshold_scale(a, out, share, d_mods, mtot, N, s_);
    }
    MKHE_HIP(hipGetLastError());
}

void Context::limbs_sum(int count, int limbs, const std::vector<const u64*>& src, u64* dst) {
    need_unmasked("mkhe_limbs_sum");
    if (src.size() > (size_t)ED_INLINE) scratch(ed_tab_, src.size());
    const EdTable st = ed_table(src, 0);                                    // more than ED_INLINE sources: staged, which synchronises
    {
        ProfScope ps(this, PROF_OTHER, 8.0 * N * limbs * count * (1.0 + (double)src.size()));
        launch_limbs_sum(count, limbs, (int)src.size(), st, dst, d_mods, N, s_);
    }
    MKHE_HIP(hipGetLastError());
}

void Context::mod_raise(const Ct& in, Ct& out) {
    need_unmasked("mkhe_ct_mod_raise");
    {
        ProfScope ps(this, PROF_OTHER, 8.0 * N * (1 + in.n) * (1.0 + out.limbs));
        launch_mod_raise(1 + in.n, out.d, in.d, d_mods, out.limbs, N, s_);
    }
    MKHE_HIP(hipGetLastError());
}

// ---- noise measurement (include/mkhe.h; noise_kernels.h).  rf_dig_ holds the digit scratch [count][limbs][N] and behind it the candidates of the
// workgroups [count][blocks][limbs + 1].  Both are the noise of the ciphertext, which depends on the keys: wiped behind the second launch, as
// decrypt_share wipes its unflooded product.  The result itself is the caller's.
void Context::noise_norm(int kind, int limbs, int count, const u64* phase, const u64* ref, long ref_stride, u64* out) {
    need_unmasked("mkhe_noise_norm");
    NoiseArgs a{};
    a.phase = phase; a.ref = ref; a.ref_stride = ref_stride;
    a.tmont = kind == 1 ? d_bf_tmont : nullptr;
    a.garner = garner_table(); a.mods = d_mods; a.out = out;
    a.nq = nq; a.limbs = limbs; a.N = N; a.blocks = nz_blocks(N);
    const size_t dw = (size_t)count * limbs * N, pw = (size_t)count * a.blocks * (limbs + 1);
    a.dig = scratch(rf_dig_, dw + pw);
    a.part = a.dig + dw;
    {
        // the inputs once; every digit is written once, read by each later limb, by the sign, by the complement (which writes it again) and by the selection
        const double refs = ref ? (ref_stride ? (double)count : 1.0) : 0.0;
        ProfScope ps(this, PROF_OTHER, 8.0 * N * limbs * (count * (1.0 + 5.0 + (limbs - 1) / 2.0) + refs));
        launch_noise_norm(a, count, s_);
    }
    MKHE_HIP(hipMemsetAsync(a.dig, 0, (dw + pw) * sizeof(u64), s_));
    MKHE_HIP(hipGetLastError());
}

}  // namespace mkhe
