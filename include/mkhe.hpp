// mkhe.hpp -- C++ host-side mirror of the reference packages mkrlwe / mkckks / mkbfv over the C ABI (mkhe.h).
//
// The reference is Go; this image has no Go toolchain, so the compiled-language host layer a user of the reference
// would program against is given here in C++ (header-only, C++17): the same type and method names, argument meaning
// and error behaviour as the Go API (a Go `panic` becomes a thrown mkhe::Error carrying the same text), all polynomial
// data resident in HBM behind RAII handles.  Reference file:line per item; the un-built cgo equivalent is shim/go/.
// (mkhe-kklss_amd/*.py is the same mirror for the Python tests and the bench.)
#pragma once
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>
#include "mkhe.h"

namespace mkhe {
struct Error : std::runtime_error { using std::runtime_error::runtime_error; };
inline void check(int rc) { if (rc) throw Error(mkhe_last_error()); }
}  // namespace mkhe

namespace mkrlwe {
using mkhe::check;
using mkhe::Error;
typedef std::set<std::string> IDSet;                                   // mkrlwe/idset.go

class SwitchingKey;

// mkrlwe.Parameters (params.go:8-12): ring parameters + CRS map + gamma, plus the engine context
// (= NewKeySwitcher state, keyswitch.go:33-47).
class Parameters {
  public:
    Parameters(int logN, std::vector<uint64_t> Q, std::vector<uint64_t> P, int gamma = 2, int device = 0)
        : logN_(logN), Q_(std::move(Q)), P_(std::move(P)), gamma_(gamma) {
        check(mkhe_ctx_create(&ctx, logN, Q_.data(), (int)Q_.size(), P_.data(), (int)P_.size(), gamma, nullptr, nullptr, device));
    }
    virtual ~Parameters() { CRS.clear(); if (ctx) mkhe_ctx_destroy(ctx); }
    Parameters(const Parameters&) = delete;
    Parameters& operator=(const Parameters&) = delete;

    int N() const { return 1 << logN_; }
    int LogN() const { return logN_; }
    int QCount() const { return (int)Q_.size(); }
    int PCount() const { return (int)P_.size(); }
    int MaxLevel() const { return QCount() - 1; }
    int Gamma() const { return gamma_; }
    int Alpha() const { return PCount() / gamma_; }                                     // params.go:63-65
    int Beta(int levelQ) const { return (levelQ + 1 + Alpha() - 1) / Alpha(); }          // params.go:67-71
    size_t SwkWords() const { return mkhe_ctx_swk_words(ctx); }
    const std::vector<uint64_t>& Q() const { return Q_; }
    const std::vector<uint64_t>& P() const { return P_; }
    uint64_t GaloisElementForColumnRotationBy(int k) const {
        const uint64_t m = 2ull * N();
        uint64_t r = 1, b = 5, e = (uint64_t)(((k % (int)m) + (int)m) % (int)m);
        for (; e; e >>= 1) { if (e & 1) r = r * b % m; b = b * b % m; }
        return r;
    }
    uint64_t GaloisElementForRowRotation() const { return 2ull * N() - 1; }
    // params.AddCRS / NewParameters CRS slots (params.go:37-61): uniform polys (NTT + Montgomery form), uploaded once
    std::shared_ptr<SwitchingKey> AddCRS(int idx, const uint64_t* host_swk);
    // the same slot expanded on the device from a public seed (mkhe_crs_expand): nothing is uploaded
    std::shared_ptr<SwitchingKey> AddCRS(int idx, uint64_t seed);
    int party_index(const std::string& id) {
        if (id == "0") throw Error("Cannot IDSet Add : 0 cannot be used");                // idset.go:12-16
        auto it = ids_.find(id);
        if (it != ids_.end()) return it->second;
        const int v = (int)ids_.size();
        ids_[id] = v;
        return v;
    }
    void sync() { check(mkhe_ctx_sync(ctx)); }
    // work issued through this context from now on starts after everything issued through `other` so far (another context
    // over the same ring on the same device: own stream and scratch pools, all handles shared) -- mkhe_ctx_wait_for
    void wait_for(const Parameters& other) { check(mkhe_ctx_wait_for(ctx, other.ctx)); }

    mkhe_ctx* ctx = nullptr;
    std::map<int, std::shared_ptr<SwitchingKey>> CRS;                                    // params.go:37-46

  protected:
    Parameters(int logN, std::vector<uint64_t> Q, std::vector<uint64_t> P, int gamma, bool /*no context yet*/)
        : logN_(logN), Q_(std::move(Q)), P_(std::move(P)), gamma_(gamma) {}
    int logN_;
    std::vector<uint64_t> Q_, P_;
    int gamma_;
    std::map<std::string, int> ids_;
};

// mkrlwe.SwitchingKey (keys.go:23-25): host layout uint64[beta][nQ+nP][N]
class SwitchingKey {
  public:
    explicit SwitchingKey(Parameters& p, const uint64_t* host = nullptr) : params(p) {
        check(mkhe_swk_create(p.ctx, &h));
        if (host) upload(host);
    }
    ~SwitchingKey() { if (h) mkhe_swk_destroy(params.ctx, h); }
    SwitchingKey(const SwitchingKey&) = delete;
    SwitchingKey& operator=(const SwitchingKey&) = delete;
    void upload(const uint64_t* host) { check(mkhe_swk_upload(params.ctx, h, host)); }
    void download(uint64_t* host) const { check(mkhe_swk_download(params.ctx, h, host)); }
    Parameters& params;
    mkhe_swk* h = nullptr;
};
inline std::shared_ptr<SwitchingKey> NewSwitchingKey(Parameters& p) { return std::make_shared<SwitchingKey>(p); }   // keys.go:245-255
inline std::shared_ptr<SwitchingKey> Parameters::AddCRS(int idx, const uint64_t* host_swk) {
    return CRS[idx] = std::make_shared<SwitchingKey>(*this, host_swk);
}

inline std::shared_ptr<SwitchingKey> Parameters::AddCRS(int idx, uint64_t seed) {
    auto k = std::make_shared<SwitchingKey>(*this);
    check(mkhe_crs_expand(ctx, seed, idx, k->h));
    return CRS[idx] = k;
}

// raw device words behind mkhe_buf_* (secret / public keys: PolyQP buffers)
class DeviceWords {
  public:
    DeviceWords(Parameters& p, size_t words_) : params(p), words(words_) { check(mkhe_buf_alloc(p.ctx, words, &d)); }
    ~DeviceWords() { if (d) mkhe_buf_free(params.ctx, d); }
    DeviceWords(const DeviceWords&) = delete;
    DeviceWords& operator=(const DeviceWords&) = delete;
    void download(uint64_t* host) const { check(mkhe_buf_download(params.ctx, d, host, words)); }
    void upload(const uint64_t* host) { check(mkhe_buf_upload(params.ctx, d, host, words)); }
    Parameters& params;
    size_t words;
    void* d = nullptr;
};
// mkrlwe.SecretKey keys.go:9-12 / PublicKey :15-18: PolyQP (NTT, Montgomery form) resp. two of them, on the device
struct SecretKey {
    SecretKey(Parameters& p, std::string id) : ID(std::move(id)), Value(p, (size_t)(p.QCount() + p.PCount()) * p.N()) {}
    std::string ID;
    DeviceWords Value;
};
struct PublicKey {
    PublicKey(Parameters& p, std::string id) : ID(std::move(id)), Value(p, 2 * (size_t)(p.QCount() + p.PCount()) * p.N()) {}
    std::string ID;
    DeviceWords Value;
};

// keys.go:34-37: Value = (b, d, v)
struct RelinearizationKey {
    RelinearizationKey(Parameters& p, std::string id, const uint64_t* b, const uint64_t* d, const uint64_t* v) : ID(std::move(id)) {
        Value[0] = std::make_shared<SwitchingKey>(p, b); Value[1] = std::make_shared<SwitchingKey>(p, d); Value[2] = std::make_shared<SwitchingKey>(p, v);
    }
    std::string ID;
    std::shared_ptr<SwitchingKey> Value[3];
};
// keys.go:53-57,165-198
struct RelinearizationKeySet {
    void AddRelinearizationKey(std::shared_ptr<RelinearizationKey> k) { Value[k->ID] = std::move(k); }
    void DelRelinearizationKey(const std::string& id) { Value.erase(id); }
    RelinearizationKey& GetRelinearizationKey(const std::string& id) {
        auto it = Value.find(id);
        if (it == Value.end()) throw Error("cannot GetRelinearizationKey: there is no relinearization key with given id");
        return *it->second;
    }
    std::map<std::string, std::shared_ptr<RelinearizationKey>> Value;
};
// keys.go:40-44,60-62,128-162
struct RotationKey {
    RotationKey(Parameters& p, int rotidx, std::string id, const uint64_t* v) : ID(std::move(id)), RotIdx(rotidx), Value(std::make_shared<SwitchingKey>(p, v)) {}
    std::string ID; int RotIdx; std::shared_ptr<SwitchingKey> Value;
};
struct RotationKeySet {
    void AddRotationKey(std::shared_ptr<RotationKey> k) { Value[k->ID][k->RotIdx] = std::move(k); }
    RotationKey& GetRotationKey(const std::string& id, int rotidx) {
        auto it = Value.find(id);
        if (it == Value.end() || !it->second.count(rotidx)) throw Error("cannot GetRotationKeys: there is no rotation key with given id");
        return *it->second[rotidx];
    }
    std::map<std::string, std::map<int, std::shared_ptr<RotationKey>>> Value;
};
// keys.go:47-50,65-67,200-228
struct ConjugationKey {
    ConjugationKey(Parameters& p, std::string id, const uint64_t* v) : ID(std::move(id)), Value(std::make_shared<SwitchingKey>(p, v)) {}
    std::string ID; std::shared_ptr<SwitchingKey> Value;
};
struct ConjugationKeySet {
    void AddConjugationKey(std::shared_ptr<ConjugationKey> k) { Value[k->ID] = std::move(k); }
    ConjugationKey& GetConjugationKey(const std::string& id) {
        auto it = Value.find(id);
        if (it == Value.end()) throw Error("cannot GetConjugationKey: there is no conjugation key with given id");
        return *it->second;
    }
    std::map<std::string, std::shared_ptr<ConjugationKey>> Value;
};
// elements.go:5-15
struct HoistedCiphertext { std::map<std::string, std::shared_ptr<SwitchingKey>> Value; };

// mkrlwe.Ciphertext (elements.go:17-33): Value["0"] + one poly per id; device layout uint64[1+n][level+1][N], ids sorted
class Ciphertext {
  public:
    Ciphertext(Parameters& p, const IDSet& idset, int level, bool zero = true) : params(p), ids(idset.begin(), idset.end()), level_(level) {
        std::vector<int> dense;
        for (auto& s : ids) dense.push_back(p.party_index(s));
        check((zero ? mkhe_ct_create : mkhe_ct_create_uninit)(p.ctx, (int)ids.size(), dense.data(), level + 1, &h));
    }
    virtual ~Ciphertext() { if (h) mkhe_ct_destroy(params.ctx, h); }
    Ciphertext(const Ciphertext&) = delete;
    Ciphertext& operator=(const Ciphertext&) = delete;
    IDSet IDSet_() const { return IDSet(ids.begin(), ids.end()); }
    int Level() const { return level_; }
    int slot(const std::string& id) const {
        if (id == "0") return 0;
        auto it = std::find(ids.begin(), ids.end(), id);
        if (it == ids.end()) throw Error("mkhe: ciphertext has no component of that id");
        return 1 + (int)(it - ids.begin());
    }
    size_t words() const { return (size_t)(1 + ids.size()) * (level_ + 1) * params.N(); }
    void upload(const uint64_t* host) { check(mkhe_ct_upload(params.ctx, h, host)); }
    void download(uint64_t* host) const { check(mkhe_ct_download(params.ctx, h, host)); }
    Parameters& params;
    std::vector<std::string> ids;
    mkhe_ct* h = nullptr;
  protected:
    int level_;
};

// mkrlwe.KeySwitcher (keyswitch.go:8-47); the reference's pools are engine-internal device buffers
class KeySwitcher {
  public:
    explicit KeySwitcher(Parameters& p) : params(p) {}
    void Decompose(int levelQ, const Ciphertext& ct, const std::string& id, SwitchingKey& ad, bool isNTT = false) {     // keyswitch.go:49-73
        check(mkhe_decompose(params.ctx, levelQ, isNTT ? 1 : 0, ct.h, ct.slot(id), ad.h));
    }
    void ExternalProduct(int levelQ, const Ciphertext& ct, const std::string& id, const SwitchingKey& bg, Ciphertext& out, const std::string& out_id, bool isNTT = false) {
        check(mkhe_external_product(params.ctx, levelQ, isNTT ? 1 : 0, ct.h, ct.slot(id), bg.h, out.h, out.slot(out_id)));      // keyswitch.go:79-118
    }
    void ExternalProductHoisted(int levelQ, const SwitchingKey& aHoisted, const SwitchingKey& bg, Ciphertext& out, const std::string& out_id) {
        check(mkhe_external_product_hoisted(params.ctx, levelQ, aHoisted.h, bg.h, out.h, out.slot(out_id)));                    // keyswitch_hoisted.go:10-40
    }
    void MulAndRelin(const Ciphertext& op0, const Ciphertext& op1, RelinearizationKeySet& rlkSet, Ciphertext& ctOut) {          // keyswitch.go:122-230
        MulAndRelinHoisted(op0, op1, nullptr, nullptr, rlkSet, ctOut);
    }
    // rescaled = true: ctOut is one level below the product and receives Rescale(MulAndRelin(..)) in one engine call (mkhe_mul_relin_rescale)
    void MulAndRelinHoisted(const Ciphertext& op0, const Ciphertext& op1, const HoistedCiphertext* op0Hoisted, const HoistedCiphertext* op1Hoisted,
                            RelinearizationKeySet& rlkSet, Ciphertext& ctOut, bool rescaled = false) {                          // keyswitch_hoisted.go:44-179
        const int lvl = ctOut.Level() + (rescaled ? 1 : 0);
        if (op0.Level() < lvl || op1.Level() < lvl) throw Error("Cannot MulAndRelin: op0 and op1 have different levels");
        if (!params.CRS.count(-1)) throw Error("mkhe: CRS[-1] (u) has not been uploaded");
        std::vector<const mkhe_swk*> d0, v0, b1, h0, h1;
        for (auto& i : op0.ids) { auto& k = rlkSet.GetRelinearizationKey(i); d0.push_back(k.Value[1]->h); v0.push_back(k.Value[2]->h); }
        for (auto& i : op1.ids) b1.push_back(rlkSet.GetRelinearizationKey(i).Value[0]->h);
        if (op0Hoisted) for (auto& i : op0.ids) h0.push_back(op0Hoisted->Value.at(i)->h);
        if (op1Hoisted) for (auto& i : op1.ids) h1.push_back(op1Hoisted->Value.at(i)->h);
        check((rescaled ? mkhe_mul_relin_rescale : mkhe_mul_and_relin)(params.ctx, op0.h, op1.h, op0Hoisted ? h0.data() : nullptr, op1Hoisted ? h1.data() : nullptr,
                                 b1.data(), d0.data(), v0.data(), params.CRS[-1]->h, ctOut.h));
    }
    void Rotate(const Ciphertext& ctIn, int rotidx, RotationKeySet& rkSet, Ciphertext& ctOut) { RotateHoisted(ctIn, rotidx, nullptr, rkSet, ctOut); }   // keyswitch.go:234-298
    void RotateHoisted(const Ciphertext& ctIn, int rotidx, const HoistedCiphertext* ctInHoisted, RotationKeySet& rkSet, Ciphertext& ctOut) {        // keyswitch_hoisted.go:183-247
        if (ctIn.Level() < ctOut.Level()) throw Error("Cannot Rotate: ctIn and ctOut have different levels");
        const int n2 = params.N() / 2;
        while (rotidx < 0) rotidx += n2;                                                                                                             // keyswitch.go:246-249
        if (!params.CRS.count(rotidx)) throw Error("mkhe: no CRS for this rotation index");
        std::vector<const mkhe_swk*> rk, hs;
        for (auto& i : ctIn.ids) rk.push_back(rkSet.GetRotationKey(i, rotidx).Value->h);
        if (ctInHoisted) for (auto& i : ctIn.ids) hs.push_back(ctInHoisted->Value.at(i)->h);
        check(mkhe_rotate(params.ctx, params.GaloisElementForColumnRotationBy(rotidx), ctIn.h, ctInHoisted ? hs.data() : nullptr, rk.data(),
                          params.CRS[rotidx]->h, ctOut.h));
    }
    void Conjugate(const Ciphertext& ctIn, ConjugationKeySet& ckSet, Ciphertext& ctOut) {                                                           // keyswitch.go:302-332
        if (ctIn.Level() < ctOut.Level()) throw Error("Cannot Conjugate: ctIn and ctOut have different levels");
        std::vector<const mkhe_swk*> ck;
        for (auto& i : ctIn.ids) ck.push_back(ckSet.GetConjugationKey(i).Value->h);
        check(mkhe_conjugate(params.ctx, params.GaloisElementForRowRotation(), ctIn.h, ck.data(), params.CRS.at(-2)->h, ctOut.h));
    }
    Parameters& params;
};
inline IDSet Union(const IDSet& a, const IDSet& b) { IDSet r = a; r.insert(b.begin(), b.end()); return r; }

// mkrlwe.KeyGenerator (keygen.go:13-40) on the device.  The small-norm SAMPLES (what lattigo's ternary / Gaussian samplers
// draw) are arguments: int32, N per polynomial, from the caller's CSPRNG -- secret randomness never comes from the GPU.
class KeyGenerator {
  public:
    explicit KeyGenerator(Parameters& p) : params(p) {}
    std::unique_ptr<SecretKey> GenSecretKey(const std::string& id, const int32_t* s) {                                   // keygen.go:44-76
        auto sk = std::make_unique<SecretKey>(params, id);
        check(mkhe_keygen_secret(params.ctx, s, sk->Value.d));
        return sk;
    }
    std::unique_ptr<PublicKey> GenPublicKey(const SecretKey& sk, const int32_t* e) {                                     // keygen.go:88-109
        auto pk = std::make_unique<PublicKey>(params, sk.ID);
        check(mkhe_keygen_public_key(params.ctx, sk.Value.d, e, crs(0)->h, pk->Value.d));
        return pk;
    }
    void GenSwitchingKey(const SecretKey& skIn, SwitchingKey& swk, const int32_t* e) {                                   // keygen.go:270-327
        check(mkhe_keygen_switching_key(params.ctx, skIn.Value.d, e, swk.h));
    }
    std::shared_ptr<RelinearizationKey> GenRelinearizationKey(const SecretKey& sk, const SecretKey& r, const int32_t* e) {   // keygen.go:137-187
        if (params.PCount() == 0) throw Error("modulus P is empty");
        auto rlk = std::make_shared<RelinearizationKey>(params, sk.ID, nullptr, nullptr, nullptr);
        check(mkhe_keygen_relin_key(params.ctx, sk.Value.d, r.Value.d, e, crs(0)->h, crs(-1)->h, rlk->Value[0]->h, rlk->Value[1]->h, rlk->Value[2]->h));
        return rlk;
    }
    std::shared_ptr<RotationKey> GenRotationKey(int rotidx, const SecretKey& sk, const int32_t* e) {                     // keygen.go:190-229
        if (!params.CRS.count(rotidx)) throw Error("Cannot GenRotationKey: CRS for given rot idx is not generated");
        auto a = params.CRS.at(rotidx);
        while (rotidx < 0) rotidx += params.N() / 2;
        auto rk = std::make_shared<RotationKey>(params, rotidx, sk.ID, nullptr);
        check(mkhe_keygen_rotation_key(params.ctx, params.GaloisElementForColumnRotationBy(rotidx), sk.Value.d, e, a->h, rk->Value->h));
        return rk;
    }
    std::shared_ptr<ConjugationKey> GenConjugationKey(const SecretKey& sk, const int32_t* e) {                           // keygen.go:240-268
        auto ck = std::make_shared<ConjugationKey>(params, sk.ID, nullptr);
        check(mkhe_keygen_conjugation_key(params.ctx, sk.Value.d, e, crs(-2)->h, ck->Value->h));
        return ck;
    }
    Parameters& params;

  protected:
    std::shared_ptr<SwitchingKey> crs(int idx) {
        auto it = params.CRS.find(idx);
        if (it == params.CRS.end()) throw Error("mkhe: CRS[" + std::to_string(idx) + "] is not generated");
        return it->second;
    }
};

// mkrlwe.SecretKeySet keys.go:70-94 (the keys stay with their owner: the set only names them)
struct SecretKeySet {
    std::map<std::string, const SecretKey*> Value;
    void AddSecretKey(const SecretKey& sk) { Value[sk.ID] = &sk; }
    void DelSecretKey(const std::string& id) { Value.erase(id); }
    const SecretKey& GetSecretKey(const std::string& id) const {
        auto it = Value.find(id);
        if (it == Value.end()) throw Error("cannot GetPublicKey: there is no public key with given id");                 // keys.go:91
        return *it->second;
    }
};

// The table of mkhe_sample_small / mkhe_encrypt_seeded (kind 1) for round(N(0, sigma)) truncated at +-B, B = int(6 sigma) by default (bound < 0):
// with Phi(x) = erfc(-x / (sigma sqrt 2)) / 2, lo = Phi(-B - 1/2), hi = Phi(B + 1/2):  T_k = min(2^64 - 1, floor((Phi(k + 1/2) - lo) / (hi - lo) * 2^64)),
// k = -B .. B - 1 (mkrlwe.small_cdt of the Python mirror, float64 like it).
inline std::vector<uint64_t> small_cdt(double sigma, int bound = -1) {
    if (!(sigma > 0.0) || !std::isfinite(sigma)) throw Error("small_cdt: sigma must be finite and positive");
    const int B = bound < 0 ? (int)(6 * sigma) : bound;
    if (B < 1 || 2 * B > 64) throw Error("small_cdt: the table has 2 * bound entries and holds 2 .. 64");
    auto phi = [sigma](double x) { return std::erfc(-x / (sigma * std::sqrt(2.0))) / 2.0; };
    const double lo = phi(-B - 0.5), hi = phi(B + 0.5);
    std::vector<uint64_t> t;
    for (int k = -B; k < B; ++k) {
        const double x = std::floor((phi(k + 0.5) - lo) / (hi - lo) * 18446744073709551616.0);
        t.push_back(x >= 18446744073709551616.0 ? ~0ull : (uint64_t)x);
        if (t.size() > 1 && t[t.size() - 1] <= t[t.size() - 2]) throw Error("small_cdt: the table is not strictly increasing (sigma too small for this bound)");
    }
    return t;
}

// Encryption randomness drawn on the device from a ChaCha20 key (include/mkhe.h, "device-side sampling"): the key is 32 bytes from the caller's
// CSPRNG, like the samples of KeyGenerator; every engine call consumes one nonce of a 64-bit counter, so that a (key, nonce) pair never
// serves two calls.  For Encryptor only: key generation keeps its host samples.
class DeviceSampler {
  public:
    explicit DeviceSampler(const uint32_t key[8], double sigma = 3.2) : cdt(small_cdt(sigma)) { std::copy(key, key + 8, key_); }
    ~DeviceSampler() { volatile uint32_t* k = key_; for (int i = 0; i < 8; ++i) k[i] = 0; }
    DeviceSampler(const DeviceSampler&) = delete;
    DeviceSampler& operator=(const DeviceSampler&) = delete;
    uint64_t NextNonce() {
        std::lock_guard<std::mutex> g(m_);
        if (counter_ == ~0ull) throw Error("DeviceSampler: the 64-bit call counter is exhausted -- use a fresh key");
        return counter_++;
    }
    // two consecutive nonces for ONE mkhe_refresh_share call (mask, encryption): the first of the pair
    uint64_t NextNoncePair() {
        std::lock_guard<std::mutex> g(m_);
        if (counter_ >= ~0ull - 1) throw Error("DeviceSampler: the 64-bit call counter is exhausted -- use a fresh key");
        counter_ += 2;
        return counter_ - 2;
    }
    uint64_t Counter() const { return counter_; }
    const uint32_t* Key() const { return key_; }
    const std::vector<uint64_t> cdt;
  private:
    uint32_t key_[8];
    uint64_t counter_ = 0;
    std::mutex m_;
};

// mkrlwe.Encryptor (encryptor.go:8-52) on the device.  Like the samples of KeyGenerator, u (ternary) and e0, e1 (Gaussian) are
// arguments: samples = int32[count][3][N] from the caller's CSPRNG -- or a DeviceSampler, from whose key the engine draws them itself
// (mkhe_encrypt_seeded).  Plaintexts are device buffers uint64[count][level+1][N].
class Encryptor {
  public:
    explicit Encryptor(Parameters& p) : params(p) {}
    void Encrypt(const void* dev_pt, const PublicKey& pk, Ciphertext& ctOut, DeviceSampler& sampler, bool ptIsNTT = false) {
        if (ctOut.ids.size() != 1 || ctOut.ids[0] != pk.ID) throw Error("Cannot Encrypt: ctOut must be a ciphertext over the id of pk alone");
        mkhe_ct* out[1] = {ctOut.h};
        check(mkhe_encrypt_seeded(params.ctx, ctOut.Level(), 1, pk.Value.d, dev_pt, ptIsNTT ? 1 : 0, sampler.Key(), sampler.NextNonce(),
                                  sampler.cdt.data(), (int)sampler.cdt.size(), out));
    }
    std::vector<std::shared_ptr<Ciphertext>> EncryptBatch(int level, int count, const void* dev_pt, const PublicKey& pk, DeviceSampler& sampler, bool ptIsNTT = false) {
        std::vector<std::shared_ptr<Ciphertext>> cts;
        std::vector<mkhe_ct*> out;
        for (int b = 0; b < count; ++b) { cts.push_back(std::make_shared<Ciphertext>(params, IDSet{pk.ID}, level, false)); out.push_back(cts.back()->h); }
        check(mkhe_encrypt_seeded(params.ctx, level, count, pk.Value.d, dev_pt, ptIsNTT ? 1 : 0, sampler.Key(), sampler.NextNonce(),
                                  sampler.cdt.data(), (int)sampler.cdt.size(), out.data()));
        return cts;
    }
    void Encrypt(const void* dev_pt, const PublicKey& pk, Ciphertext& ctOut, const int32_t* samples, bool ptIsNTT = false) {   // encryptor.go:55-118
        if (ctOut.ids.size() != 1 || ctOut.ids[0] != pk.ID) throw Error("Cannot Encrypt: ctOut must be a ciphertext over the id of pk alone");
        mkhe_ct* out[1] = {ctOut.h};
        check(mkhe_encrypt(params.ctx, ctOut.Level(), 1, pk.Value.d, dev_pt, ptIsNTT ? 1 : 0, samples, out));
    }
    // count plaintexts under one public key as one engine call
    std::vector<std::shared_ptr<Ciphertext>> EncryptBatch(int level, int count, const void* dev_pt, const PublicKey& pk, const int32_t* samples, bool ptIsNTT = false) {
        std::vector<std::shared_ptr<Ciphertext>> cts;
        std::vector<mkhe_ct*> out;
        for (int b = 0; b < count; ++b) { cts.push_back(std::make_shared<Ciphertext>(params, IDSet{pk.ID}, level, false)); out.push_back(cts.back()->h); }
        check(mkhe_encrypt(params.ctx, level, count, pk.Value.d, dev_pt, ptIsNTT ? 1 : 0, samples, out.data()));
        return cts;
    }
    Parameters& params;
};

// `count` fresh ciphertexts of party `id` at `level` in their half-size form (include/mkhe.h, "secret-key encryption"): the c0 polynomials -- polynomial 0
// of `count` device ciphertexts whose polynomial 1 is not yet written -- plus the PUBLIC (Key, Nonce) that c1 is expanded from.  download gives what
// travels (uint64[count][level+1][N] and the seed); the receiver builds one with upload and calls Expand.  Only fresh ciphertexts have a seed.
class SeededCiphertext {
  public:
    // over ready (uninitialised) ciphertexts of one party at one level: what the scheme wrappers pass in their own Ciphertext type
    SeededCiphertext(Parameters& p, std::string id, int level, std::vector<std::shared_ptr<Ciphertext>> cts_)
        : params(p), ID(std::move(id)), Level(level), Count((int)cts_.size()), cts(std::move(cts_)) {
        if (Count < 1 || Count > 65535) throw Error("SeededCiphertext: count must be 1 .. 65535");
    }
    SeededCiphertext(Parameters& p, std::string id, int level, int count = 1) : SeededCiphertext(p, id, level, fresh(p, id, level, count)) {}
    void SetSeed(const uint32_t key[8], uint64_t nonce) { std::copy(key, key + 8, Key); Nonce = nonce; seeded_ = true; }
    size_t words() const { return (size_t)Count * (Level + 1) * params.N(); }
    void download(uint64_t* c0) const {
        if (!seeded_) throw Error("SeededCiphertext: nothing to download (no seed yet)");
        for (int b = 0; b < Count; ++b) { auto rows = limbs(c0, b); check(mkhe_ct_download_poly_limbs(params.ctx, cts[b]->h, 0, rows.data())); }
    }
    void upload(const uint64_t* c0, const uint32_t key[8], uint64_t nonce) {
        if (expanded_) throw Error("SeededCiphertext: already expanded");
        SetSeed(key, nonce);
        for (int b = 0; b < Count; ++b) { auto rows = limbs(const_cast<uint64_t*>(c0), b); check(mkhe_ct_upload_poly_limbs(params.ctx, cts[b]->h, 0, rows.data())); }
    }
    // mkhe_ct_expand_seeded writes polynomial 1: the ciphertexts that hold c0 become ordinary ciphertexts over {ID}, no copy
    const std::vector<std::shared_ptr<Ciphertext>>& Expand() {
        if (!seeded_) throw Error("SeededCiphertext: nothing to expand (no seed yet)");
        if (!expanded_) {
            std::vector<mkhe_ct*> out;
            for (auto& c : cts) out.push_back(c->h);
            check(mkhe_ct_expand_seeded(params.ctx, Count, Key, Nonce, out.data()));
            expanded_ = true;
        }
        return cts;
    }
    void MarkExpanded() { expanded_ = true; }             // (an encrypt call has written polynomial 1 as well)
    static std::vector<std::shared_ptr<Ciphertext>> fresh(Parameters& p, const std::string& id, int level, int count) {
        std::vector<std::shared_ptr<Ciphertext>> v;
        for (int b = 0; b < count; ++b) v.push_back(std::make_shared<Ciphertext>(p, IDSet{id}, level, false));
        return v;
    }
    // what a fresh ciphertext costs on the wire: c0 + 32 bytes of seed + 8 of nonce, or both polynomials
    static size_t WireBytes(int limbs, int N, bool seeded) { return seeded ? (size_t)limbs * N * 8 + 40 : 2 * (size_t)limbs * N * 8; }
    Parameters& params;
    std::string ID;
    int Level, Count;
    uint32_t Key[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t Nonce = 0;
    std::vector<std::shared_ptr<Ciphertext>> cts;
  private:
    template <class T> std::vector<T*> limbs(T* c0, int b) const {
        std::vector<T*> rows;
        for (int l = 0; l <= Level; ++l) rows.push_back(c0 + ((size_t)b * (Level + 1) + l) * params.N());
        return rows;
    }
    bool seeded_ = false, expanded_ = false;
};

// Encryption under the party's OWN secret key with c1 expanded from a public seed: c1 = a, c0 = pt + e - a s (include/mkhe.h, "secret-key
// encryption"; no reference counterpart).  seed: 32 PUBLIC bytes from the caller's CSPRNG; every engine call takes one value of the encryptor's own
// locked 64-bit counter as the nonce of a, so that an (a_key, a_nonce) pair serves one call.  e: int32[count][N] from the caller's CSPRNG -- or a
// DeviceSampler, from whose key the engine forms it in registers (mkhe_encrypt_sk_seeded).  Plaintexts are device buffers uint64[count][level+1][N].
class SecretKeyEncryptor {
  public:
    SecretKeyEncryptor(Parameters& p, const SecretKey& sk_, const uint32_t seed[8]) : params(p), sk(sk_) { std::copy(seed, seed + 8, seed_); }
    SecretKeyEncryptor(const SecretKeyEncryptor&) = delete;
    SecretKeyEncryptor& operator=(const SecretKeyEncryptor&) = delete;
    uint64_t NextNonce() {
        std::lock_guard<std::mutex> g(m_);
        if (counter_ == ~0ull) throw Error("SecretKeyEncryptor: the 64-bit call counter is exhausted -- use a fresh seed");
        return counter_++;
    }
    uint64_t Counter() const { return counter_; }
    const uint32_t* Seed() const { return seed_; }
    void Encrypt(const void* dev_pt, Ciphertext& ctOut, DeviceSampler& sampler, bool ptIsNTT = false) {
        own(ctOut);
        mkhe_ct* out[1] = {ctOut.h};
        call(ctOut.Level(), 1, dev_pt, ptIsNTT, &sampler, nullptr, out);
    }
    void Encrypt(const void* dev_pt, Ciphertext& ctOut, const int32_t* e, bool ptIsNTT = false) {
        own(ctOut);
        mkhe_ct* out[1] = {ctOut.h};
        call(ctOut.Level(), 1, dev_pt, ptIsNTT, nullptr, e, out);
    }
    std::vector<std::shared_ptr<Ciphertext>> EncryptBatch(int level, int count, const void* dev_pt, DeviceSampler& sampler, bool ptIsNTT = false) {
        auto cts = SeededCiphertext::fresh(params, sk.ID, level, count);
        into(cts, level, dev_pt, ptIsNTT, &sampler, nullptr);
        return cts;
    }
    std::vector<std::shared_ptr<Ciphertext>> EncryptBatch(int level, int count, const void* dev_pt, const int32_t* e, bool ptIsNTT = false) {
        auto cts = SeededCiphertext::fresh(params, sk.ID, level, count);
        into(cts, level, dev_pt, ptIsNTT, nullptr, e);
        return cts;
    }
    // the same call, returned in the half-size form
    std::shared_ptr<SeededCiphertext> EncryptSeededBatch(int level, int count, const void* dev_pt, DeviceSampler& sampler, bool ptIsNTT = false) {
        return seeded(std::make_shared<SeededCiphertext>(params, sk.ID, level, count), dev_pt, ptIsNTT, &sampler, nullptr);
    }
    std::shared_ptr<SeededCiphertext> EncryptSeededBatch(int level, int count, const void* dev_pt, const int32_t* e, bool ptIsNTT = false) {
        return seeded(std::make_shared<SeededCiphertext>(params, sk.ID, level, count), dev_pt, ptIsNTT, nullptr, e);
    }
    Parameters& params;
    const SecretKey& sk;
  protected:
    // one engine call into ready ciphertexts (any subclass of Ciphertext); returns the nonce of a it used
    template <class Ct> uint64_t into(const std::vector<std::shared_ptr<Ct>>& cts, int level, const void* dev_pt, bool ptIsNTT, DeviceSampler* sampler, const int32_t* e) {
        std::vector<mkhe_ct*> out;
        for (auto& c : cts) out.push_back(c->h);
        return call(level, (int)cts.size(), dev_pt, ptIsNTT, sampler, e, out.data());
    }
    std::shared_ptr<SeededCiphertext> seeded(std::shared_ptr<SeededCiphertext> sc, const void* dev_pt, bool ptIsNTT, DeviceSampler* sampler, const int32_t* e) {
        const uint64_t nonce = into(sc->cts, sc->Level, dev_pt, ptIsNTT, sampler, e);
        sc->SetSeed(seed_, nonce);
        sc->MarkExpanded();
        return sc;
    }
  private:
    void own(const Ciphertext& ct) const {
        if (ct.ids.size() != 1 || ct.ids[0] != sk.ID) throw Error("Cannot Encrypt: ctOut must be a ciphertext over the id of sk alone");
    }
    uint64_t call(int level, int count, const void* dev_pt, bool ptIsNTT, DeviceSampler* sampler, const int32_t* e, mkhe_ct* const* out) {
        const uint64_t nonce = NextNonce();
        if (sampler)
            check(mkhe_encrypt_sk_seeded(params.ctx, level, count, sk.Value.d, dev_pt, ptIsNTT ? 1 : 0, seed_, nonce, sampler->Key(), sampler->NextNonce(),
                                         sampler->cdt.data(), (int)sampler->cdt.size(), out));
        else
            check(mkhe_encrypt_sk(params.ctx, level, count, sk.Value.d, dev_pt, ptIsNTT ? 1 : 0, seed_, nonce, e, out));
        return nonce;
    }
    uint32_t seed_[8];
    uint64_t counter_ = 0;
    std::mutex m_;
};

// What one party publishes in distributed decryption (include/mkhe.h, "distributed decryption"): mu = c_id * s_id + e for `count` ciphertexts at
// `level`, uint64[count][level+1][N] on the device.  Shares travel between parties: Value.download on one side, Value.upload on the other.
struct DecryptionShare {
    DecryptionShare(Parameters& p, std::string id, int level, int count = 1)
        : ID(std::move(id)), Level(level), Count(count), Value(p, (size_t)count * (level + 1) * p.N()) {}
    std::string ID;
    int Level, Count;
    DeviceWords Value;
};

// A noise norm as mkhe_noise_norm measures it (include/mkhe.h, "noise measurement"): the integer itself as its digit vector -- Words, little endian,
// base 2^64, no leading zero word (empty = 0) -- with a long double beside it (Value(): the words summed from the top in long double arithmetic, so
// exact up to its 64-bit mantissa) and its exact bit length (Bits(), Python's int.bit_length()); Index = the smallest coefficient that attains it
// (-1 for a value derived from one).
struct NoiseValue {
    std::vector<uint64_t> Words;
    long Index = -1;
    int Bits() const { return Words.empty() ? 0 : (int)(64 * (Words.size() - 1)) + 64 - __builtin_clzll(Words.back()); }
    long double Value() const {
        long double v = 0;
        for (size_t i = Words.size(); i-- > 0;) v = v * 18446744073709551616.0L + (long double)Words[i];
        return v;
    }
    // this * m + a, and floor(this / d) (m, a, d < 2^64, d > 0)
    NoiseValue& MulAdd(uint64_t m, uint64_t a) {
        unsigned __int128 carry = a;
        for (auto& w : Words) { carry += (unsigned __int128)w * m; w = (uint64_t)carry; carry >>= 64; }
        if (carry) Words.push_back((uint64_t)carry);
        return *this;
    }
    NoiseValue& Div(uint64_t d) {
        unsigned __int128 rem = 0;
        for (size_t i = Words.size(); i-- > 0;) { rem = (rem << 64) | Words[i]; Words[i] = (uint64_t)(rem / d); rem %= d; }
        while (!Words.empty() && !Words.back()) Words.pop_back();
        return *this;
    }
    // r = d_0 + d_1 q_0 + d_2 q_0 q_1 + .. by Horner from the top digit
    static NoiseValue FromMixedRadix(const uint64_t* digits, const uint64_t* q, int limbs, long index) {
        NoiseValue v;
        v.Index = index;
        for (int i = limbs - 1; i >= 0; --i) v.MulAdd(i + 1 < limbs ? q[i] : 1, digits[i]);
        while (!v.Words.empty() && !v.Words.back()) v.Words.pop_back();
        return v;
    }
};

// mkrlwe.Decryptor (decryptor.go:8-23) on the device.  Between parties, decryption is ShareNew (each party, on its own key) and MergeShares (anyone):
// Decrypt needs every key in one place, and the output of PartialDecrypt gives the key away.
class Decryptor {
  public:
    explicit Decryptor(Parameters& p) : params(p) {}
    // The exact centred max norm of `count` phases uint64[count][limbs][N] (what Decrypt or MergeSharesBatch wrote) as ONE engine call
    // (mkhe_noise_norm).  kind 0: of phase - ref (dev_ref the same shape, refStrideWords = limbs * N, or one reference for all with 0; null: of the
    // phase); kind 1 (BFV contexts, limbs = nQ, no reference): of T * phase, the invariant noise.  Only the digits and the index come down.
    std::vector<NoiseValue> NoiseNormBatch(int limbs, int count, const void* dev_phase, const void* dev_ref = nullptr, long refStrideWords = 0, int kind = 0) {
        const size_t row = (size_t)limbs + 1;
        DeviceWords out(params, (size_t)(count > 0 ? count : 1) * row);
        check(mkhe_noise_norm(params.ctx, kind, limbs, count, dev_phase, dev_ref, refStrideWords, out.d));
        std::vector<uint64_t> host(out.words);
        out.download(host.data());
        std::vector<NoiseValue> res;
        for (int b = 0; b < count; ++b) res.push_back(NoiseValue::FromMixedRadix(&host[b * row], params.Q().data(), limbs, (long)host[b * row + limbs]));
        return res;
    }
    // Decrypt, then the norm of the residual against dev_ref uint64[level+1][N] (the plaintext ct is expected to hold; null: of the phase itself).
    // Its Bits() is what the floodBits of ShareNew must exceed.
    NoiseValue NoiseNorm(const Ciphertext& ct, const SecretKeySet& skSet, const void* dev_ref = nullptr, int kind = 0) {
        DeviceWords pt(params, (size_t)(ct.Level() + 1) * params.N());
        Decrypt(ct, skSet, pt.d);
        return NoiseNormBatch(ct.Level() + 1, 1, pt.d, dev_ref, 0, kind)[0];
    }
    // what a merge of `parties` shares with floodBits bits adds to a coefficient, at most: parties * 2^(floodBits - 1) (0 bits: 0)
    static long double FloodBound(int parties, int floodBits) { return floodBits == 0 ? 0.0L : (long double)parties * std::ldexp(1.0L, floodBits - 1); }
    // The shares of the party of sk for the ciphertexts cts (one level; their id sets may differ) as one engine call.  floodBits = 1 .. 62: the width of
    // the flooding noise, drawn on the device under one nonce of `sampler`; no default -- it must exceed the noise of the ciphertext by the statistical
    // security parameter, which the engine cannot know.  floodBits = 0 (sampler may be null) is for tests only: such a share reveals sk.
    std::shared_ptr<DecryptionShare> ShareBatch(const std::vector<const Ciphertext*>& cts, const SecretKey& sk, int floodBits, DeviceSampler* sampler) {
        if (cts.empty()) throw Error("Cannot ShareBatch: no ciphertext");
        if (floodBits > 0 && !sampler) throw Error("Cannot Share: the flooding noise is drawn on the device -- pass a DeviceSampler");
        std::vector<const mkhe_ct*> in;
        std::vector<int> slots;
        for (auto* ct : cts) { in.push_back(ct->h); slots.push_back(ct->slot(sk.ID)); }
        auto out = std::make_shared<DecryptionShare>(params, sk.ID, cts[0]->Level(), (int)cts.size());
        check(mkhe_decrypt_share(params.ctx, (int)cts.size(), in.data(), slots.data(), sk.Value.d, floodBits > 0 ? sampler->Key() : nullptr,
                                 floodBits > 0 ? sampler->NextNonce() : 0, floodBits, out->Value.d));
        return out;
    }
    std::shared_ptr<DecryptionShare> ShareNew(const Ciphertext& ct, const SecretKey& sk, int floodBits, DeviceSampler* sampler) {
        return ShareBatch({&ct}, sk, floodBits, sampler);
    }
    // dev_pt_out = uint64[count][level+1][N] <- c_0 + the shares of ALL parties (one DecryptionShare of count cts.size() per party, in any order), for
    // ciphertexts over the same ids at one level: what Decrypt gives, plus the sum of the flooding noises
    void MergeSharesBatch(const std::vector<const Ciphertext*>& cts, const std::vector<const DecryptionShare*>& shares, void* dev_pt_out) {
        if (cts.empty()) throw Error("Cannot MergeShares: no ciphertext");
        std::vector<const mkhe_ct*> in;
        for (auto* ct : cts) in.push_back(ct->h);
        std::vector<const void*> ordered;
        for (auto& id : cts[0]->ids) {
            const DecryptionShare* found = nullptr;
            for (auto* sh : shares)
                if (sh->ID == id) { if (found) throw Error("Cannot MergeShares: two shares of one party"); found = sh; }
            if (!found) throw Error("Cannot MergeShares: the share of a party is missing");
            if (found->Level != cts[0]->Level() || found->Count != (int)cts.size()) throw Error("Cannot MergeShares: a share is at another level or for another batch size");
            ordered.push_back(found->Value.d);
        }
        if (shares.size() != ordered.size()) throw Error("Cannot MergeShares: a share of a party the ciphertext does not have");
        check(mkhe_decrypt_merge(params.ctx, (int)cts.size(), in.data(), (int)ordered.size(), ordered.data(), dev_pt_out));
    }
    void MergeShares(const Ciphertext& ct, const std::vector<const DecryptionShare*>& shares, void* dev_pt_out) { MergeSharesBatch({&ct}, shares, dev_pt_out); }
    // The shares that the t holders of ONE absent party's key made with their additive keys (Combiner::AdditiveKey; same id, level and count) -> one
    // DecryptionShare of that id, their sum (mkhe_limbs_sum); MergeShares* then works unchanged.  A party covered by t holders contributes t floods:
    // FloodBound / FloodSlotBound are called with k - 1 + t in the place of k.
    std::shared_ptr<DecryptionShare> FoldShares(const std::vector<const DecryptionShare*>& shares) {
        if (shares.empty()) throw Error("Cannot FoldShares: no share");
        std::vector<const void*> src;
        for (auto* sh : shares) {
            if (sh->ID != shares[0]->ID) throw Error("Cannot FoldShares: shares of different parties (a fold is over the holders of ONE party's key)");
            if (sh->Level != shares[0]->Level || sh->Count != shares[0]->Count) throw Error("Cannot FoldShares: shares at different levels or for different batch sizes");
            src.push_back(sh->Value.d);
        }
        auto out = std::make_shared<DecryptionShare>(params, shares[0]->ID, shares[0]->Level, shares[0]->Count);
        check(mkhe_limbs_sum(params.ctx, shares[0]->Count, shares[0]->Level + 1, (int)src.size(), src.data(), out->Value.d));
        return out;
    }
    // decryptor.go:26-43; the Go version works in place and deletes ct.Value[sk.ID]: here the result is a new ciphertext over the remaining ids.
    // WARNING: the result REVEALS sk to anyone who sees it (c_0 and c_id are public, c_id is invertible with overwhelming probability): it is for a
    // process that holds every key, as in the reference's tests.  Between parties use ShareNew / MergeShares.
    std::shared_ptr<Ciphertext> PartialDecrypt(const Ciphertext& ct, const SecretKey& sk) {
        IDSet rest = ct.IDSet_();
        rest.erase(sk.ID);
        auto out = std::make_shared<Ciphertext>(params, rest, ct.Level(), false);
        check(mkhe_partial_decrypt(params.ctx, ct.h, ct.slot(sk.ID), sk.Value.d, out->h));
        return out;
    }
    // decryptor.go:48-66: dev_pt_out = uint64[level+1][N], canonical residues, coefficient domain
    void Decrypt(const Ciphertext& ct, const SecretKeySet& skSet, void* dev_pt_out) {
        std::vector<const void*> sks;
        for (auto& id : ct.ids) {
            auto it = skSet.Value.find(id);
            if (it == skSet.Value.end()) throw Error("Cannot Decrypt: there is a missing secretkey");                     // decryptor.go:61-63
            sks.push_back(it->second->Value.d);
        }
        check(mkhe_decrypt(params.ctx, ct.h, sks.data(), dev_pt_out));
    }
    Parameters& params;
};

// What one party publishes in a collective refresh (include/mkhe.h, "collective refresh") of `count` ciphertexts: Share, the MASKED products
// c_id * s_id + M at levelIn, and Reenc, `count` ciphertexts over the party's id alone at levelOut that encrypt -M.  Both travel between parties
// (Share.Value.download / upload, Ciphertext::download / upload).
struct RefreshShare {
    RefreshShare(Parameters& p, const std::string& id, int levelIn, int levelOut, int count = 1) : ID(id), LevelOut(levelOut), Share(p, id, levelIn, count) {
        for (int b = 0; b < count; ++b) Reenc.push_back(std::make_shared<Ciphertext>(p, IDSet{id}, levelOut, false));
    }
    std::string ID;
    int LevelOut;
    DecryptionShare Share;
    std::vector<std::shared_ptr<Ciphertext>> Reenc;
};

// The collective refresh between parties: ShareNew (each party, on its own keys and its own DeviceSampler) and MergeNew (anyone) give a ciphertext of
// the same message over the same parties at levelOut.  The caller chooses maskBits: maskBits minus the bit size of the message is the statistical
// hiding it gets, and parties * 2^(maskBits-1) plus the message must stay below Q_level / 2 (the Python mirror's Refresher.MaxMaskBits).
class Refresher {
  public:
    explicit Refresher(Parameters& p) : params(p) {}
    // maskBits = 1 .. 120; 0 (no mask) is for tests only: such a share reveals sk.  Two nonces of `sampler` serve the call.
    std::shared_ptr<RefreshShare> ShareBatch(const std::vector<const Ciphertext*>& cts, const SecretKey& sk, const PublicKey& pk, int maskBits,
                                             DeviceSampler& sampler, int levelOut = -1) {
        if (cts.empty()) throw Error("Cannot RefreshShare: no ciphertext");
        if (sk.ID != pk.ID) throw Error("Cannot RefreshShare: sk and pk belong to different parties");
        if (maskBits < 0 || maskBits > 120) throw Error("Cannot RefreshShare: maskBits must be 0 .. 120");
        if (levelOut < 0) levelOut = params.MaxLevel();
        std::vector<const mkhe_ct*> in;
        std::vector<int> slots;
        for (auto* ct : cts) { in.push_back(ct->h); slots.push_back(ct->slot(sk.ID)); }
        auto out = std::make_shared<RefreshShare>(params, sk.ID, cts[0]->Level(), levelOut, (int)cts.size());
        std::vector<mkhe_ct*> re;
        for (auto& c : out->Reenc) re.push_back(c->h);
        const uint64_t nonce = sampler.NextNoncePair();
        check(mkhe_refresh_share(params.ctx, (int)cts.size(), in.data(), slots.data(), sk.Value.d, pk.Value.d, sampler.Key(), nonce, nonce + 1, maskBits,
                                 sampler.cdt.data(), (int)sampler.cdt.size(), out->Share.Value.d, re.data()));
        return out;
    }
    std::shared_ptr<RefreshShare> ShareNew(const Ciphertext& ct, const SecretKey& sk, const PublicKey& pk, int maskBits, DeviceSampler& sampler, int levelOut = -1) {
        return ShareBatch({&ct}, sk, pk, maskBits, sampler, levelOut);
    }
    // one RefreshShare of count cts.size() per party, in any order, for ciphertexts over the same ids at one level -> the refreshed ciphertexts
    std::vector<std::shared_ptr<Ciphertext>> MergeBatch(const std::vector<const Ciphertext*>& cts, const std::vector<const RefreshShare*>& shares) {
        if (cts.empty()) throw Error("Cannot RefreshMerge: no ciphertext");
        std::vector<const mkhe_ct*> in;
        for (auto* ct : cts) in.push_back(ct->h);
        std::vector<const void*> ordered;
        std::vector<const mkhe_ct*> re;
        int levelOut = params.MaxLevel();
        for (auto& id : cts[0]->ids) {
            const RefreshShare* found = nullptr;
            for (auto* sh : shares)
                if (sh->ID == id) { if (found) throw Error("Cannot MergeShares: two shares of one party"); found = sh; }
            if (!found) throw Error("Cannot MergeShares: the share of a party is missing");
            if (found->Share.Level != cts[0]->Level() || found->Share.Count != (int)cts.size()) throw Error("Cannot MergeShares: a share is at another level or for another batch size");
            if (!ordered.empty() && found->LevelOut != levelOut) throw Error("Cannot RefreshMerge: the shares are for different output levels");
            levelOut = found->LevelOut;
            ordered.push_back(found->Share.Value.d);
            for (auto& c : found->Reenc) re.push_back(c->h);
        }
        if (shares.size() != ordered.size()) throw Error("Cannot MergeShares: a share of a party the ciphertext does not have");
        std::vector<std::shared_ptr<Ciphertext>> outs;
        std::vector<mkhe_ct*> oh;
        for (size_t b = 0; b < cts.size(); ++b) { outs.push_back(std::make_shared<Ciphertext>(params, cts[0]->IDSet_(), levelOut, false)); oh.push_back(outs.back()->h); }
        check(mkhe_refresh_merge(params.ctx, (int)cts.size(), in.data(), (int)ordered.size(), ordered.data(), re.data(), oh.data()));
        return outs;
    }
    std::shared_ptr<Ciphertext> MergeNew(const Ciphertext& ct, const std::vector<const RefreshShare*>& shares) { return MergeBatch({&ct}, shares)[0]; }
    Parameters& params;
};
// An ADDITIVE share of the plaintexts of `count` ciphertexts (include/mkhe.h, "encryption to shares"): uint64[count][limbs][N] on the device, the id of the
// party that holds it (empty: the public share, which anyone can compute) and the level (-1 where the share is over Z_T: mkbfv, limbs = 1).  A
// party's share is as secret as its mask and travels to nobody.  Wipe() overwrites the device buffer with zeros and then frees it.
struct SecretShare {
    SecretShare(Parameters& p, std::string id, int level, int count = 1, int limbs = -1)
        : ID(std::move(id)), Level(level), Count(count), Limbs(limbs < 0 ? level + 1 : limbs), Value(p, (size_t)count * (limbs < 0 ? level + 1 : limbs) * p.N()) {}
    void Wipe() {
        if (!Value.d) return;
        const std::vector<uint64_t> zero(Value.words, 0);
        Value.upload(zero.data());
        mkhe_buf_free(Value.params.ctx, Value.d);
        Value.d = nullptr;
    }
    std::string ID;
    int Level, Count, Limbs;
    DeviceWords Value;
};

// HE <-> additive secret sharing between parties, exact over R_Q in the coefficient domain (the Python mirror's mkrlwe.ShareConverter).  E2S: every party
// runs E2SShareBatch on its own key and DeviceSampler, publishes the DecryptionShare (Refresher::ShareBatch's, bit for bit) and KEEPS the SecretShare;
// anyone runs E2SMergeBatch, which gives the public share.  public + the sum of the secret shares is the plaintext of Decrypt modulo every prime of
// the input level, whatever maskBits is.  S2E: the holder of the public share folds it into its own (FoldPublic: mkhe_limbs_sum) BEFORE it encrypts;
// every party encrypts its share under its own public key (S2EShareBatch); S2EMergeNew is the AddNew chain over the parties' ciphertexts.
class ShareConverter {
  public:
    explicit ShareConverter(Parameters& p) : params(p) {}
    virtual ~ShareConverter() = default;
    // one nonce of `sampler`; levelOut: the level of the secret share (default: the maximum level)
    std::pair<std::shared_ptr<DecryptionShare>, std::shared_ptr<SecretShare>> E2SShareBatch(const std::vector<const Ciphertext*>& cts, const SecretKey& sk, int maskBits,
                                                                                            DeviceSampler& sampler, int levelOut = -1) {
        if (cts.empty()) throw Error("Cannot E2SShare: no ciphertext");
        if (maskBits < 0 || maskBits > 120) throw Error("Cannot E2SShare: maskBits must be 0 .. 120");
        if (levelOut < 0) levelOut = params.MaxLevel();
        std::vector<const mkhe_ct*> in;
        std::vector<int> slots;
        for (auto* ct : cts) { in.push_back(ct->h); slots.push_back(ct->slot(sk.ID)); }
        auto pub = std::make_shared<DecryptionShare>(params, sk.ID, cts[0]->Level(), (int)cts.size());
        auto sec = std::make_shared<SecretShare>(params, sk.ID, levelOut, (int)cts.size());
        check(mkhe_e2s_share(params.ctx, (int)cts.size(), in.data(), slots.data(), sk.Value.d, sampler.Key(), sampler.NextNonce(), maskBits, pub->Value.d,
                             levelOut + 1, sec->Value.d));
        return {pub, sec};
    }
    // one DecryptionShare of count cts.size() per party, in any order, for ciphertexts over the same ids at one level -> the public share (ID empty)
    std::shared_ptr<SecretShare> E2SMergeBatch(const std::vector<const Ciphertext*>& cts, const std::vector<const DecryptionShare*>& shares, int levelOut = -1) {
        if (cts.empty()) throw Error("Cannot E2SMerge: no ciphertext");
        if (levelOut < 0) levelOut = params.MaxLevel();
        std::vector<const mkhe_ct*> in;
        for (auto* ct : cts) in.push_back(ct->h);
        const std::vector<const void*> ordered = orderShares(*cts[0], (int)cts.size(), shares);
        auto out = std::make_shared<SecretShare>(params, std::string(), levelOut, (int)cts.size());
        check(mkhe_e2s_merge(params.ctx, (int)cts.size(), in.data(), (int)ordered.size(), ordered.data(), levelOut + 1, out->Value.d));
        return out;
    }
    std::shared_ptr<SecretShare> FoldPublic(const SecretShare& secret, const SecretShare& pub) {
        if (secret.Count != pub.Count || secret.Limbs != pub.Limbs) throw Error("Cannot FoldPublic: the shares differ in count or level");
        auto out = std::make_shared<SecretShare>(params, secret.ID, secret.Level, secret.Count, secret.Limbs);
        const void* src[2] = {secret.Value.d, pub.Value.d};
        check(mkhe_limbs_sum(params.ctx, secret.Count, secret.Limbs, 2, src, out->Value.d));
        return out;
    }
    // the party of pk encrypts its share as a plaintext under its own public key (mkhe_encrypt_seeded, one nonce): Count ciphertexts over its id
    std::vector<std::shared_ptr<Ciphertext>> S2EShareBatch(const SecretShare& secret, const PublicKey& pk, DeviceSampler& sampler) {
        if (!secret.ID.empty() && secret.ID != pk.ID) throw Error("Cannot S2EShare: the share and pk belong to different parties");
        std::vector<std::shared_ptr<Ciphertext>> cts;
        std::vector<mkhe_ct*> out;
        for (int b = 0; b < secret.Count; ++b) { cts.push_back(newCt(IDSet{pk.ID}, secret.Limbs - 1)); out.push_back(cts.back()->h); }
        check(mkhe_encrypt_seeded(params.ctx, secret.Limbs - 1, secret.Count, pk.Value.d, secret.Value.d, 0, sampler.Key(), sampler.NextNonce(),
                                  sampler.cdt.data(), (int)sampler.cdt.size(), out.data()));
        return cts;
    }
    // the AddNew chain over the parties' ciphertexts (one each) -> one ciphertext over all their ids
    std::shared_ptr<Ciphertext> S2EMergeNew(const std::vector<const Ciphertext*>& ctsByParty) {
        if (ctsByParty.empty()) throw Error("Cannot S2EMerge: no ciphertext");
        std::shared_ptr<Ciphertext> acc;
        const Ciphertext* cur = ctsByParty[0];
        for (size_t i = 1; i < ctsByParty.size(); ++i) {
            auto out = newCt(Union(cur->IDSet_(), ctsByParty[i]->IDSet_()), cur->Level());
            check(mkhe_ct_add(params.ctx, cur->h, ctsByParty[i]->h, out->h));
            acc = out;
            cur = acc.get();
        }
        if (!acc) { acc = newCt(cur->IDSet_(), cur->Level()); check(mkhe_ct_copy(params.ctx, cur->h, acc->h)); }
        return acc;
    }
    // the shares of a merge in the slot order of a ciphertext; throws on a missing, duplicate or foreign share, another level or batch size
    static std::vector<const void*> orderShares(const Ciphertext& like, int count, const std::vector<const DecryptionShare*>& shares) {
        std::vector<const void*> ordered;
        for (auto& id : like.ids) {
            const DecryptionShare* found = nullptr;
            for (auto* sh : shares)
                if (sh->ID == id) { if (found) throw Error("Cannot MergeShares: two shares of one party"); found = sh; }
            if (!found) throw Error("Cannot MergeShares: the share of a party is missing");
            if (found->Level != like.Level() || found->Count != count) throw Error("Cannot MergeShares: a share is at another level or for another batch size");
            ordered.push_back(found->Value.d);
        }
        if (shares.size() != ordered.size()) throw Error("Cannot MergeShares: a share of a party the ciphertext does not have");
        return ordered;
    }
    Parameters& params;
  protected:
    virtual std::shared_ptr<Ciphertext> newCt(const IDSet& ids, int level) { return std::make_shared<Ciphertext>(params, ids, level, false); }
};
// What one party publishes in a collective key switch to a recipient's public key (include/mkhe.h, "collective public-key switch") of `count`
// ciphertexts at `level`: the pairs (h0, h1), uint64[count][2][level+1][N] on the device.  Shares travel between parties: Value.download on one
// side, Value.upload on the other.
struct PublicKeySwitchShare {
    PublicKeySwitchShare(Parameters& p, std::string id, int level, int count = 1)
        : ID(std::move(id)), Level(level), Count(count), Value(p, (size_t)count * 2 * (level + 1) * p.N()) {}
    std::string ID;
    int Level, Count;
    DeviceWords Value;
};

// The collective key switch to a recipient's public key between parties: ShareNew (each party, on its own secret key, the RECIPIENT's public key and
// its own DeviceSampler) and MergeNew (anyone) give an ordinary ciphertext of the same message over the recipient's id alone.  The caller chooses
// floodBits: floodBits minus the bit size of the ciphertext's noise is the statistical hiding of that noise, and NoiseBound plus that noise must
// stay below the decryption margin.  The engine cannot check whose key pkRecipient is.
class PublicKeySwitcher {
  public:
    explicit PublicKeySwitcher(Parameters& p) : params(p) {}
    // what a switch adds to a coefficient of the phase, at most: parties * (2^(floodBits-1) + 2 N bound) (the Python mirror gives the exact integer)
    static long double NoiseBound(int parties, int floodBits, int N, int bound = 19) {
        return (long double)parties * ((floodBits > 0 ? std::ldexp(1.0L, floodBits - 1) : 0.0L) + 2.0L * N * bound);
    }
    // floodBits = 0 .. 1024, at most bitlen(Q_level div 2T') - 1; 0 (no flood) is for tests only: such a share gives sk away.  One nonce of `sampler`.
    std::shared_ptr<PublicKeySwitchShare> ShareBatch(const std::vector<const Ciphertext*>& cts, const SecretKey& sk, const PublicKey& pkRecipient, int floodBits,
                                                     DeviceSampler& sampler) {
        if (cts.empty()) throw Error("Cannot SwitchShare: no ciphertext");
        if (floodBits < 0 || floodBits > 1024) throw Error("Cannot SwitchShare: floodBits must be 0 .. 1024");
        std::vector<const mkhe_ct*> in;
        std::vector<int> slots;
        for (auto* ct : cts) { in.push_back(ct->h); slots.push_back(ct->slot(sk.ID)); }
        auto out = std::make_shared<PublicKeySwitchShare>(params, sk.ID, cts[0]->Level(), (int)cts.size());
        check(mkhe_pcks_share(params.ctx, (int)cts.size(), in.data(), slots.data(), sk.Value.d, pkRecipient.Value.d, sampler.Key(), sampler.NextNonce(), floodBits,
                              sampler.cdt.data(), (int)sampler.cdt.size(), out->Value.d));
        return out;
    }
    std::shared_ptr<PublicKeySwitchShare> ShareNew(const Ciphertext& ct, const SecretKey& sk, const PublicKey& pkRecipient, int floodBits, DeviceSampler& sampler) {
        return ShareBatch({&ct}, sk, pkRecipient, floodBits, sampler);
    }
    // one PublicKeySwitchShare of count cts.size() per party, in any order, for ciphertexts over the same ids at one level -> ciphertexts over {recipient}
    std::vector<std::shared_ptr<Ciphertext>> MergeBatch(const std::vector<const Ciphertext*>& cts, const std::vector<const PublicKeySwitchShare*>& shares,
                                                        const std::string& recipient) {
        std::vector<std::shared_ptr<Ciphertext>> outs;
        for (size_t b = 0; b < cts.size(); ++b) outs.push_back(std::make_shared<Ciphertext>(params, IDSet{recipient}, cts[0]->Level(), false));
        merge(cts, shares, outs);
        return outs;
    }
    std::shared_ptr<Ciphertext> MergeNew(const Ciphertext& ct, const std::vector<const PublicKeySwitchShare*>& shares, const std::string& recipient) {
        return MergeBatch({&ct}, shares, recipient)[0];
    }
    Parameters& params;
  protected:
    // the engine call of a merge into ready outputs (any subclass of Ciphertext)
    template <class Ct> void merge(const std::vector<const Ciphertext*>& cts, const std::vector<const PublicKeySwitchShare*>& shares,
                                   const std::vector<std::shared_ptr<Ct>>& outs) {
        if (cts.empty()) throw Error("Cannot SwitchMerge: no ciphertext");
        std::vector<const mkhe_ct*> in;
        for (auto* ct : cts) in.push_back(ct->h);
        std::vector<const void*> ordered;
        for (auto& id : cts[0]->ids) {
            const PublicKeySwitchShare* found = nullptr;
            for (auto* sh : shares)
                if (sh->ID == id) { if (found) throw Error("Cannot MergeShares: two shares of one party"); found = sh; }
            if (!found) throw Error("Cannot MergeShares: the share of a party is missing");
            if (found->Level != cts[0]->Level() || found->Count != (int)cts.size()) throw Error("Cannot MergeShares: a share is at another level or for another batch size");
            ordered.push_back(found->Value.d);
        }
        if (shares.size() != ordered.size()) throw Error("Cannot MergeShares: a share of a party the ciphertext does not have");
        std::vector<mkhe_ct*> oh;
        for (auto& o : outs) oh.push_back(o->h);
        check(mkhe_pcks_merge(params.ctx, (int)cts.size(), in.data(), (int)ordered.size(), ordered.data(), oh.data()));
    }
};

// ---- threshold secret keys (include/mkhe.h, "threshold secret keys")
// The Shamir share of the secret key of party ID that Holder keeps, at the public point Point, under a t-of-n sharing with t = Threshold:
// uint64[nQ+nP][N] on the device, in the representation of SecretKey::Value.  Fewer than t shares say nothing about the key, but the t shares of an
// active set together ARE the key: a share is key material and travels only to its holder, over a private channel (Value.download / upload).
struct SecretKeyShare {
    SecretKeyShare(Parameters& p, std::string id, std::string holder, uint32_t point, int threshold)
        : ID(std::move(id)), Holder(std::move(holder)), Point(point), Threshold(threshold), Value(p, (size_t)(p.QCount() + p.PCount()) * p.N()) {}
    std::string ID, Holder;
    uint32_t Point;
    int Threshold;
    DeviceWords Value;
};
// The party side of t-out-of-n thresholdisation (lattigo's drlwe.Thresholdizer): Shamir-shares a secret key among n holders as ONE engine call
// (mkhe_threshold_gen_shares).  The coefficient polynomials are drawn on the device under one nonce of `sampler` and exist in registers only.
// threshold = 1 hands every holder the key itself (tests only).
class Thresholdizer {
  public:
    explicit Thresholdizer(Parameters& p) : params(p) {}
    std::map<std::string, std::shared_ptr<SecretKeyShare>> GenShares(const SecretKey& sk, int threshold, const std::map<std::string, uint32_t>& points,
                                                                      DeviceSampler& sampler) {
        std::map<std::string, std::shared_ptr<SecretKeyShare>> out;
        std::vector<uint32_t> xs;
        std::vector<void*> bufs;
        for (auto& hp : points) {
            auto sh = std::make_shared<SecretKeyShare>(params, sk.ID, hp.first, hp.second, threshold);
            xs.push_back(hp.second);
            bufs.push_back(sh->Value.d);
            out[hp.first] = sh;
        }
        check(mkhe_threshold_gen_shares(params.ctx, sk.Value.d, threshold, (int)xs.size(), xs.data(), sampler.Key(), sampler.NextNonce(), bufs.data()));
        return out;
    }
    Parameters& params;
};
// The holder side (lattigo's drlwe.Combiner): from a Shamir share to the additive key for one active set.
class Combiner {
  public:
    explicit Combiner(Parameters& p) : params(p) {}
    // share times its Lagrange coefficient for the active set activePoints (the points of at least t holders, share.Point among them) -> a SecretKey
    // with ID = share.ID (mkhe_threshold_additive_key).  The additive keys of the active set sum to the key of party share.ID, so Decryptor, Refresher
    // and PublicKeySwitcher ShareBatch take it unchanged and the holders' outputs add up to that party's share (Decryptor::FoldShares).  It is key
    // material of the same rank as a key, and a share made from it must be FLOODED exactly like one made from a key.
    std::shared_ptr<SecretKey> AdditiveKey(const SecretKeyShare& share, const std::vector<uint32_t>& activePoints) {
        auto out = std::make_shared<SecretKey>(params, share.ID);
        check(mkhe_threshold_additive_key(params.ctx, share.Value.d, share.Point, (int)activePoints.size(), activePoints.data(), out->Value.d));
        return out;
    }
    // the sum of the additive keys of ONE active set (mkhe_limbs_sum over the nQ+nP rows) -> the SecretKey of their party.  For tests and key
    // recovery: in the protocols the additive keys never meet.
    std::shared_ptr<SecretKey> Reconstruct(const std::vector<const SecretKey*>& keys) {
        if (keys.empty()) throw Error("Cannot Reconstruct: no key");
        std::vector<const void*> src;
        for (auto* k : keys) {
            if (k->ID != keys[0]->ID) throw Error("Cannot Reconstruct: additive keys of different parties");
            src.push_back(k->Value.d);
        }
        auto out = std::make_shared<SecretKey>(params, keys[0]->ID);
        check(mkhe_limbs_sum(params.ctx, 1, params.QCount() + params.PCount(), (int)src.size(), src.data(), out->Value.d));
        return out;
    }
    Parameters& params;
};
}  // namespace mkrlwe

namespace mkckks {
using mkhe::check;
using mkhe::Error;

// mkckks.Parameters (params.go:11-24): mkrlwe parameters with gamma = 2 + default scale
class Parameters : public mkrlwe::Parameters {
  public:
    Parameters(int logN, std::vector<uint64_t> Q, std::vector<uint64_t> P, double scale, int device = 0)
        : mkrlwe::Parameters(logN, std::move(Q), std::move(P), 2, device), scale_(scale) {}
    double Scale() const { return scale_; }
  private:
    double scale_;
};
// mkckks.Ciphertext (elements.go:5-17)
class Ciphertext : public mkrlwe::Ciphertext {
  public:
    Ciphertext(Parameters& p, const mkrlwe::IDSet& idset, int level, double scale, bool zero = true) : mkrlwe::Ciphertext(p, idset, level, zero), Scale(scale) {}
    double ScalingFactor() const { return Scale; }
    double Scale;
};
typedef std::unique_ptr<Ciphertext> CiphertextPtr;

// mkckks.Evaluator (evaluator.go:13-39)
class Evaluator {
  public:
    explicit Evaluator(Parameters& p) : params(p), ksw(p) {}
    CiphertextPtr AddNew(const Ciphertext& op0, const Ciphertext& op1) { return binary(op0, op1, mkhe_ct_add); }      // evaluator.go:316-327
    CiphertextPtr SubNew(const Ciphertext& op0, const Ciphertext& op1) { return binary(op0, op1, mkhe_ct_sub); }      // evaluator.go:329-357
    // evaluator.go:376-384
    int nbRescales(const Ciphertext& ctIn, double minScale, double* scaleOut) const {
        double scale = ctIn.Scale; int nb = 0;
        while (ctIn.Level() - nb >= 0 && scale / (double)params.Q()[ctIn.Level() - nb] >= minScale / 2) { scale /= (double)params.Q()[ctIn.Level() - nb]; ++nb; }
        *scaleOut = scale;
        return nb;
    }
    // evaluator.go:96-114: keep the first Level()+1-levels limbs of every component
    CiphertextPtr DropLevelNew(const Ciphertext& ct0, int levels) {
        auto out = std::make_unique<Ciphertext>(params, ct0.IDSet_(), ct0.Level() - levels, ct0.Scale, false);
        std::vector<uint64_t> one;
        for (int i = 0; i <= out->Level(); ++i) one.push_back((uint64_t)((((unsigned __int128)1) << 64) % params.Q()[i]));     // MForm(1)
        check(mkhe_ct_mul_const(params.ctx, ct0.h, one.data(), one.data(), out->h));
        return out;
    }
    // mkhe_ct_lincomb as it is (no reference counterpart): the caller encodes dev_consts [cts.size() + 1][2][ctOut.Level() + 1 + nb_rescale] and sets ctOut.Scale
    void LinComb(const std::vector<const mkhe_ct*>& cts, const void* dev_consts, int nb_rescale, Ciphertext& ctOut) { check(mkhe_ct_lincomb(params.ctx, (int)cts.size(), cts.data(), dev_consts, nb_rescale, ctOut.h)); }
    // mkhe_ct_lincomb_multi as it is (no reference counterpart): outs[g] = row g of mkhe_ct_lincomb for every g as one launch.  dev_consts: device
    // uint64[outs.size()][cts.size() + 1][2][Level(outs) + 1 + nb_rescale]; the caller sets the Scale of every output
    void LinCombs(const std::vector<const mkhe_ct*>& cts, const void* dev_consts, int nb_rescale, const std::vector<mkhe_ct*>& outs) {
        check(mkhe_ct_lincomb_multi(params.ctx, (int)cts.size(), cts.data(), (int)outs.size(), dev_consts, nb_rescale, outs.data()));
    }
    // mkhe_mul_relin_sum as it is (no reference counterpart): ctOut = [Rescale] sum_k ops0[k] * ops1[k] under one relinearisation tail.  Every ops0[k]
    // carries the ids of ops0[0], every ops1[k] those of ops1[0]; hoisted0 / hoisted1: one form per pair, or empty (the engine hoists that side); the
    // caller sets ctOut.Scale
    void MulRelinSum(const std::vector<const Ciphertext*>& ops0, const std::vector<const Ciphertext*>& ops1, const std::vector<const mkrlwe::HoistedCiphertext*>& hoisted0,
                     const std::vector<const mkrlwe::HoistedCiphertext*>& hoisted1, mkrlwe::RelinearizationKeySet& rlkSet, bool rescale, Ciphertext& ctOut) {
        if (ops0.empty() || ops0.size() != ops1.size()) throw Error("MulRelinSum: as many first operands as second ones, at least one pair");
        if ((!hoisted0.empty() && hoisted0.size() != ops0.size()) || (!hoisted1.empty() && hoisted1.size() != ops1.size())) throw Error("MulRelinSum: one hoisted form per pair");
        if (!params.CRS.count(-1)) throw Error("mkhe: CRS[-1] (u) has not been uploaded");
        std::vector<const mkhe_ct*> a, b;
        std::vector<const mkhe_swk*> d0, v0, b1, h0, h1;
        for (auto* c : ops0) a.push_back(c->h);
        for (auto* c : ops1) b.push_back(c->h);
        for (auto& i : ops0[0]->ids) { auto& k = rlkSet.GetRelinearizationKey(i); d0.push_back(k.Value[1]->h); v0.push_back(k.Value[2]->h); }
        for (auto& i : ops1[0]->ids) b1.push_back(rlkSet.GetRelinearizationKey(i).Value[0]->h);
        for (auto* h : hoisted0) for (auto& i : ops0[0]->ids) h0.push_back(h->Value.at(i)->h);
        for (auto* h : hoisted1) for (auto& i : ops1[0]->ids) h1.push_back(h->Value.at(i)->h);
        check(mkhe_mul_relin_sum(params.ctx, (int)a.size(), a.data(), b.data(), hoisted0.empty() ? nullptr : h0.data(), hoisted1.empty() ? nullptr : h1.data(),
                                 b1.data(), d0.data(), v0.data(), params.CRS[-1]->h, rescale ? 1 : 0, ctOut.h));
    }
    // mkhe_ptxt_prepare / mkhe_ct_ptxt_dot as they are (no reference counterpart): the prepared plaintexts lie compactly in (giant, baby) order; the caller
    // sets the scales of the outputs
    void PtxtPrepare(int limbs, int count, const void* dev_pt, void* dev_ptntt) { check(mkhe_ptxt_prepare(params.ctx, limbs, count, dev_pt, dev_ptntt)); }
    void PtxtDot(const std::vector<const mkhe_ct*>& cts, const std::vector<uint32_t>& masks, const void* dev_ptntt, int pt_limbs, const std::vector<mkhe_ct*>& outs) {
        if (masks.size() != outs.size()) throw Error("PtxtDot: one mask per output");
        check(mkhe_ct_ptxt_dot(params.ctx, (int)cts.size(), cts.data(), (int)outs.size(), masks.data(), dev_ptntt, pt_limbs, outs.data()));
    }
    // evaluator.go:465-481: dev_pt = the plaintext polynomial uint64[Level()+1][N] resident on the device (mkhe_buf_*), pt_scale its scale
    CiphertextPtr MulPtxtNew(const Ciphertext& ct, const void* dev_pt, double pt_scale) {
        auto out = std::make_unique<Ciphertext>(params, ct.IDSet_(), ct.Level(), ct.Scale * pt_scale, false);
        check(mkhe_ct_mul_ptxt(params.ctx, ct.h, dev_pt, out->h));
        if (out->Level() == 0) return out;
        double scale; const int nb = nbRescales(*out, params.Scale(), &scale);
        if (nb == 0) return out;
        auto res = std::make_unique<Ciphertext>(params, out->IDSet_(), out->Level() - nb, scale, false);
        check(mkhe_rescale(params.ctx, out->h, nb, res->h));
        return res;
    }
    CiphertextPtr RescaleNew(const Ciphertext& ct0, double threshold) {                                                 // evaluator.go:359-414
        if (threshold <= 0) throw Error("cannot Rescale: minScale is 0");
        if (ct0.Scale == 0) throw Error("cannot Rescale: ciphertext scale is 0");
        if (ct0.Level() == 0) throw Error("cannot Rescale: input Ciphertext already at level 0");
        double scale; const int nb = nbRescales(ct0, threshold, &scale);
        auto out = std::make_unique<Ciphertext>(params, ct0.IDSet_(), ct0.Level() - nb, scale, false);
        check(mkhe_rescale(params.ctx, ct0.h, nb, out->h));
        return out;
    }
    std::unique_ptr<mkrlwe::HoistedCiphertext> HoistedForm(const Ciphertext& ct) {                                      // evaluator.go:543-553
        auto h = std::make_unique<mkrlwe::HoistedCiphertext>();
        std::vector<mkhe_swk*> outs;
        for (auto& id : ct.ids) { h->Value[id] = mkrlwe::NewSwitchingKey(params); outs.push_back(h->Value[id]->h); }
        check(mkhe_hoisted_form(params.ctx, ct.Level(), ct.h, outs.data()));          // all party components in one batched launch
        return h;
    }
    CiphertextPtr MulRelinNew(const Ciphertext& op0, const Ciphertext& op1, mkrlwe::RelinearizationKeySet& rlkSet) {      // evaluator.go:416-443
        return MulRelinHoistedNew(op0, op1, nullptr, nullptr, rlkSet);
    }
    CiphertextPtr MulRelinHoistedNew(const Ciphertext& op0, const Ciphertext& op1, const mkrlwe::HoistedCiphertext* h0, const mkrlwe::HoistedCiphertext* h1,
                                     mkrlwe::RelinearizationKeySet& rlkSet) {                                            // evaluator.go:558-581
        {   // the usual single Rescale rides on the engine call (the number of rescales depends on scales and moduli only)
            const int level = std::min(op0.Level(), op1.Level());
            double sc = op0.ScalingFactor() * op1.ScalingFactor(); int nb1 = 0;
            while (level - nb1 >= 0 && sc / (double)params.Q()[level - nb1] >= params.Scale() / 2) { sc /= (double)params.Q()[level - nb1]; ++nb1; }
            if (nb1 == 1 && level >= 1) {
                auto res = std::make_unique<Ciphertext>(params, mkrlwe::Union(op0.IDSet_(), op1.IDSet_()), level - 1, sc, false);
                ksw.MulAndRelinHoisted(op0, op1, h0, h1, rlkSet, *res, true);
                return res;
            }
        }
        auto ctOut = std::make_unique<Ciphertext>(params, mkrlwe::Union(op0.IDSet_(), op1.IDSet_()), std::min(op0.Level(), op1.Level()),
                                                  op0.ScalingFactor() * op1.ScalingFactor(), false);
        ksw.MulAndRelinHoisted(op0, op1, h0, h1, rlkSet, *ctOut);
        double scale; const int nb = nbRescales(*ctOut, params.Scale(), &scale);
        if (nb == 0 || ctOut->Level() == 0) return ctOut;
        auto res = std::make_unique<Ciphertext>(params, ctOut->IDSet_(), ctOut->Level() - nb, scale, false);
        check(mkhe_rescale(params.ctx, ctOut->h, nb, res->h));
        return res;
    }
    CiphertextPtr RotateNew(const Ciphertext& ct0, int rotidx, mkrlwe::RotationKeySet& rkSet) {                          // evaluator.go:485-525
        const int n2 = params.N() / 2;
        rotidx = ((rotidx % n2) + n2) % n2;
        if (rotidx == 0) return copy(ct0);
        if (params.CRS.count(rotidx)) { auto out = like(ct0); ksw.Rotate(ct0, rotidx, rkSet, *out); return out; }
        CiphertextPtr cur; const Ciphertext* src = &ct0;
        for (int k = 1; rotidx > 0; k *= 2, rotidx /= 2) {                                                                // power-of-two decomposition, :516-523
            if (rotidx % 2 == 0) continue;
            auto nxt = like(ct0);
            ksw.Rotate(*src, k, rkSet, *nxt);
            cur = std::move(nxt); src = cur.get();
        }
        return cur;
    }
    CiphertextPtr RotateHoistedNew(const Ciphertext& ct0, int rotidx, const mkrlwe::HoistedCiphertext& hoisted, mkrlwe::RotationKeySet& rkSet) {   // evaluator.go:585-617
        const int n2 = params.N() / 2;
        rotidx = ((rotidx % n2) + n2) % n2;
        if (rotidx == 0) return copy(ct0);
        if (!params.CRS.count(rotidx)) throw Error("Hoisted rotation only works for precomputed rotation keys");
        auto out = like(ct0);
        ksw.RotateHoisted(ct0, rotidx, &hoisted, rkSet, *out);
        return out;
    }
    CiphertextPtr ConjugateNew(const Ciphertext& ct0, mkrlwe::ConjugationKeySet& ckSet) {                                // evaluator.go:527-541
        auto out = like(ct0);
        ksw.Conjugate(ct0, ckSet, *out);
        return out;
    }
    // mkhe_ct_mod_raise (no reference counterpart): the level-0 ciphertext ct0, read as its centred representatives mod Q[0], at `level` >= 1; Scale unchanged
    CiphertextPtr ModRaiseNew(const Ciphertext& ct0, int level) {
        auto out = std::make_unique<Ciphertext>(params, ct0.IDSet_(), level, ct0.Scale, false);
        check(mkhe_ct_mod_raise(params.ctx, ct0.h, out->h));
        return out;
    }
    Parameters& params;
    mkrlwe::KeySwitcher ksw;

  private:
    CiphertextPtr like(const Ciphertext& c) { return std::make_unique<Ciphertext>(params, c.IDSet_(), c.Level(), c.Scale, false); }
    CiphertextPtr copy(const Ciphertext& c) {
        auto out = like(c);
        check(mkhe_ct_copy(params.ctx, c.h, out->h));
        return out;
    }
    // the operand times an integer factor (MultByConst with an integer-valued float64: constant scale 1, evaluator.go:117-199), scale unchanged
    CiphertextPtr timesInteger(const Ciphertext& op, double f) {
        if (!(f < 9223372036854775808.0)) throw Error("mkhe: scale ratio beyond 2^63");
        const uint64_t fi = (uint64_t)f;
        std::vector<uint64_t> c;
        for (int i = 0; i <= op.Level(); ++i) { const uint64_t q = params.Q()[i]; c.push_back((uint64_t)((((unsigned __int128)(fi % q)) << 64) % q)); }     // MForm(f mod q_i)
        auto tmp = like(op);
        check(mkhe_ct_mul_const(params.ctx, op.h, c.data(), c.data(), tmp->h));
        return tmp;
    }
    // AddNew / SubNew with the scale matching of evaluateInPlace (evaluator.go:214-281, the fresh-ctOut branch): the operand with the
    // smaller scale is first multiplied by floor(ratio) when that is > 1; the result carries max(s0, s1) like the reference's
    template <typename F> CiphertextPtr binary(const Ciphertext& op0, const Ciphertext& op1, F fn) {
        const double s0 = op0.Scale, s1 = op1.Scale;
        CiphertextPtr t0, t1;
        if (s1 > s0 && std::floor(s1 / s0) > 1) t0 = timesInteger(op0, std::floor(s1 / s0));
        else if (s0 > s1 && std::floor(s0 / s1) > 1) t1 = timesInteger(op1, std::floor(s0 / s1));
        const Ciphertext& a = t0 ? *t0 : op0;
        const Ciphertext& b = t1 ? *t1 : op1;
        auto out = std::make_unique<Ciphertext>(params, mkrlwe::Union(op0.IDSet_(), op1.IDSet_()), std::min(op0.Level(), op1.Level()), std::max(s0, s1), false);
        check(fn(params.ctx, a.h, b.h, out->h));
        return out;
    }
};

// The CKKS encoder on the device (mkhe_ckks_encode_sparse / mkhe_ckks_decode_sparse): the message layer of mkckks/encryptor.go:42-64 and
// mkckks/decryptor.go:34-43.  lattigo's ckks.Encoder, which those lines call, is not in the reference tree: this is the canonical
// embedding, not lattigo's code path.  Slots() = 2^logSlots complex values per message; the default is full packing, logSlots = logN - 1,
// below it the packing is sparse (include/mkhe.h: the message is a polynomial in X^(N / 2 Slots())).  Messages cross the bus as slots;
// plaintexts are device buffers uint64[count][level+1][N], coefficient domain: what mkrlwe::Encryptor takes and Decryptor writes.
class Encoder {
  public:
    explicit Encoder(Parameters& p, int logSlots = -1) : params(p), logSlots_(logSlots < 0 ? p.LogN() - 1 : logSlots) {
        if (logSlots_ > p.LogN() - 1) throw Error("mkckks::Encoder: logSlots must lie between 0 and logN - 1");
    }
    int LogSlots() const { return logSlots_; }
    int Slots() const { return 1 << logSlots_; }
    // count messages (host: count * Slots() values) at `level` and `scale` -> dev_pt, as one launch set
    void Encode(int count, const std::complex<double>* values, int level, double scale, void* dev_pt) {
        mkrlwe::DeviceWords z(params, 2 * (size_t)count * Slots());
        check(mkhe_buf_upload(params.ctx, z.d, reinterpret_cast<const uint64_t*>(values), z.words));
        check(mkhe_ckks_encode_sparse(params.ctx, level, logSlots_, count, z.d, scale, dev_pt));
    }
    // count plaintexts of `limbs` limbs at `scale` -> values (host: count * Slots())
    void Decode(int limbs, int count, const void* dev_pt, double scale, std::complex<double>* values) {
        mkrlwe::DeviceWords z(params, 2 * (size_t)count * Slots());
        check(mkhe_ckks_decode_sparse(params.ctx, limbs, logSlots_, count, dev_pt, scale, z.d));
        z.download(reinterpret_cast<uint64_t*>(values));
    }
    Parameters& params;
  private:
    int logSlots_;
};
// mkrlwe::Decryptor with the noise of a ciphertext against the message it should hold: the residual of the phase against the device encoder's plaintext
// of msg (Slots() values) at the level and scale of ct.  NoiseBits is what the floodBits of a ShareNew must exceed.
class Decryptor : public mkrlwe::Decryptor {
  public:
    explicit Decryptor(Parameters& p) : mkrlwe::Decryptor(p), ckks(p) {}
    using mkrlwe::Decryptor::NoiseNorm;
    mkrlwe::NoiseValue NoiseNorm(const Ciphertext& ct, const mkrlwe::SecretKeySet& skSet, const std::complex<double>* msg) {
        mkrlwe::DeviceWords ref(ckks, (size_t)(ct.Level() + 1) * ckks.N());
        Encoder(ckks).Encode(1, msg, ct.Level(), ct.Scale, ref.d);
        return mkrlwe::Decryptor::NoiseNorm(ct, skSet, ref.d);
    }
    int NoiseBits(const Ciphertext& ct, const mkrlwe::SecretKeySet& skSet, const std::complex<double>* msg) { return NoiseNorm(ct, skSet, msg).Bits(); }
  private:
    Parameters& ckks;
};
// mkrlwe::ShareConverter on mkckks ciphertexts.  The shares are over R_Q in the coefficient domain and carry no scale (a 120-bit mask does not survive a
// float64 decode, so there is no slot form): the caller sets Scale to that of the ciphertexts E2S started from, and S2E gives mkckks::Ciphertexts with it.
class ShareConverter : public mkrlwe::ShareConverter {
  public:
    explicit ShareConverter(Parameters& p, double scale = 0.0) : mkrlwe::ShareConverter(p), Scale(scale), ckks(p) {}
    double Scale;
  protected:
    std::shared_ptr<mkrlwe::Ciphertext> newCt(const mkrlwe::IDSet& ids, int level) override { return std::make_shared<Ciphertext>(ckks, ids, level, Scale, false); }
  private:
    Parameters& ckks;
};
// The collective key switch of mkrlwe::PublicKeySwitcher on mkckks ciphertexts: the result keeps the input's Scale.
class PublicKeySwitcher : public mkrlwe::PublicKeySwitcher {
  public:
    explicit PublicKeySwitcher(Parameters& p) : mkrlwe::PublicKeySwitcher(p), ckks(p) {}
    // how far a switch moves a slot, at most: N * NoiseBound / scale
    long double SwitchSlotBound(int parties, int floodBits, double scale, int bound = 19) const {
        return (long double)ckks.N() * NoiseBound(parties, floodBits, ckks.N(), bound) / scale;
    }
    std::vector<std::shared_ptr<Ciphertext>> MergeBatch(const std::vector<const Ciphertext*>& cts, const std::vector<const mkrlwe::PublicKeySwitchShare*>& shares,
                                                        const std::string& recipient) {
        std::vector<std::shared_ptr<Ciphertext>> outs;
        std::vector<const mkrlwe::Ciphertext*> base(cts.begin(), cts.end());
        for (size_t b = 0; b < cts.size(); ++b) outs.push_back(std::make_shared<Ciphertext>(ckks, mkrlwe::IDSet{recipient}, cts[0]->Level(), cts[0]->Scale, false));
        merge(base, shares, outs);
        return outs;
    }
    std::shared_ptr<Ciphertext> MergeNew(const Ciphertext& ct, const std::vector<const mkrlwe::PublicKeySwitchShare*>& shares, const std::string& recipient) {
        return MergeBatch({&ct}, shares, recipient)[0];
    }
  private:
    Parameters& ckks;
};
// mkrlwe::SeededCiphertext over mkckks ciphertexts with `scale`: ExpandCkks gives them in their own type
class SeededCiphertext : public mkrlwe::SeededCiphertext {
  public:
    SeededCiphertext(Parameters& p, const std::string& id, int level, int count, double scale)
        : mkrlwe::SeededCiphertext(p, id, level, fresh_ckks(p, id, level, count, scale)), Scale(scale) {}
    std::vector<std::shared_ptr<Ciphertext>> ExpandCkks() {
        std::vector<std::shared_ptr<Ciphertext>> out;
        for (auto& c : Expand()) out.push_back(std::static_pointer_cast<Ciphertext>(c));
        return out;
    }
    double Scale;
  private:
    static std::vector<std::shared_ptr<mkrlwe::Ciphertext>> fresh_ckks(Parameters& p, const std::string& id, int level, int count, double scale) {
        std::vector<std::shared_ptr<mkrlwe::Ciphertext>> v;
        for (int b = 0; b < count; ++b) v.push_back(std::make_shared<Ciphertext>(p, mkrlwe::IDSet{id}, level, scale, false));
        return v;
    }
};
// mkrlwe::SecretKeyEncryptor on mkckks ciphertexts (plaintexts at `level` with `scale`: the output of Encoder::Encode on the device)
class SecretKeyEncryptor : public mkrlwe::SecretKeyEncryptor {
  public:
    SecretKeyEncryptor(Parameters& p, const mkrlwe::SecretKey& sk_, const uint32_t seed[8]) : mkrlwe::SecretKeyEncryptor(p, sk_, seed), ckks(p) {}
    std::vector<std::shared_ptr<Ciphertext>> EncryptPtxtBatch(int level, int count, const void* dev_pt, double scale, mkrlwe::DeviceSampler& sampler) {
        std::vector<std::shared_ptr<Ciphertext>> cts;
        for (int b = 0; b < count; ++b) cts.push_back(std::make_shared<Ciphertext>(ckks, mkrlwe::IDSet{sk.ID}, level, scale, false));
        into(cts, level, dev_pt, false, &sampler, nullptr);
        return cts;
    }
    std::shared_ptr<SeededCiphertext> EncryptPtxtSeeded(int level, int count, const void* dev_pt, double scale, mkrlwe::DeviceSampler& sampler) {
        auto sc = std::make_shared<SeededCiphertext>(ckks, sk.ID, level, count, scale);
        seeded(sc, dev_pt, false, &sampler, nullptr);
        return sc;
    }
  private:
    Parameters& ckks;
};
}  // namespace mkckks

namespace mkbfv {
using mkhe::check;
using mkhe::Error;

// mkbfv.Parameters (params.go:21-76): rings Q, QMul, R = Q || QMul, P, plaintext modulus T; gamma = 2
class Parameters : public mkrlwe::Parameters {
  public:
    Parameters(int logN, std::vector<uint64_t> Q, std::vector<uint64_t> QMul, std::vector<uint64_t> P, uint64_t T, int device = 0)
        : mkrlwe::Parameters(logN, std::move(Q), std::move(P), 2, true), QMul_(std::move(QMul)), T_(T) {
        if (Q_.size() != QMul_.size()) throw Error("cannot NewParametersFromLiteral: length of Q & QMul is not equal");            // params.go:30-32
        check(mkhe_ctx_create_bfv(&ctx, logN, Q_.data(), QMul_.data(), (int)Q_.size(), P_.data(), (int)P_.size(), 2, T, device));
    }
    uint64_t T() const { return T_; }
  private:
    std::vector<uint64_t> QMul_;
    uint64_t T_;
};
// mkbfv.Ciphertext (elements.go:5-11): always at MaxLevel, coefficient domain
class Ciphertext : public mkrlwe::Ciphertext {
  public:
    Ciphertext(Parameters& p, const mkrlwe::IDSet& idset, bool zero = true) : mkrlwe::Ciphertext(p, idset, p.MaxLevel(), zero) {}
};
typedef std::unique_ptr<Ciphertext> CiphertextPtr;
// mkbfv.RelinearizationKey (keys.go:6-9): Value[0] = (b1, d1, v), Value[1] = (b2, d2, -)
struct RelinearizationKey {
    RelinearizationKey(Parameters& p, std::string id, const uint64_t* b1, const uint64_t* b2, const uint64_t* d1, const uint64_t* d2, const uint64_t* v) : ID(id) {
        Value[0] = std::make_shared<mkrlwe::RelinearizationKey>(p, id, b1, d1, v);
        Value[1] = std::make_shared<mkrlwe::RelinearizationKey>(p, id, b2, d2, nullptr);
    }
    std::string ID;
    std::shared_ptr<mkrlwe::RelinearizationKey> Value[2];
};
struct RelinearizationKeySet {                                                                                                     // keys.go:11-21,33-82
    void AddRelinearizationKey(std::shared_ptr<RelinearizationKey> k) { Value[k->ID] = std::move(k); }
    RelinearizationKey& GetRelinearizationKey(const std::string& id) {
        auto it = Value.find(id);
        if (it == Value.end()) throw Error("cannot GetRelinearizationKey: there is no relinearization key with given id");
        return *it->second;
    }
    std::map<std::string, std::shared_ptr<RelinearizationKey>> Value;
};
// A Z_T-linear map on the two slot rows of a BFV message, encoded once for Evaluator::LinearTransformNew (no reference counterpart; include/mkhe.h,
// "BFV plaintext linear transform"; the Python mirror's mkbfv.LinearTransform).  With n = N/2: (M z)[r][j] = sum_k d_k[r][j] z[r][(j+k) mod n] +
// sum_k e_k[r][j] z[1-r][(j+k) mod n].  A diagonal is 2 n values, row 0 then row 1, taken mod T; indices are taken mod n.  diagonals keep the rows,
// swapped exchange them.  n1 = 0: the power of two <= 16 with the fewest rotations over the union of both index sets (ties to the smaller).  All
// pre-rotated diagonals of both parts go through ONE mkhe_bfv_encode_mul into the compact block of mkhe_bfv_ct_ptxt_dot; masks holds the giants of
// the row-preserving part, then those of the row-swapping part.
class LinearTransform {
  public:
    typedef std::map<int, std::vector<int64_t>> Diagonals;
    LinearTransform(Parameters& p, const Diagonals& diagonals, const Diagonals& swapped = Diagonals(), int n1_ = 0) : params(p), n(p.N() / 2) {
        if (diagonals.empty() && swapped.empty()) throw Error("mkbfv::LinearTransform: no diagonal");
        if (n1_ < 0 || n1_ > 16 || (n1_ & (n1_ - 1))) throw Error("mkbfv::LinearTransform: n1 must be a power of two, at most 16");
        std::map<int, const std::vector<int64_t>*> part[2];
        const Diagonals* src[2] = {&diagonals, &swapped};
        std::set<int> idx;
        for (int s = 0; s < 2; ++s)
            for (auto& kv : *src[s]) {
                const int k = ((kv.first % n) + n) % n;
                if (kv.second.size() != 2 * (size_t)n) throw Error("mkbfv::LinearTransform: a diagonal holds 2 * N/2 values (row 0, then row 1)");
                if (!part[s].emplace(k, &kv.second).second) throw Error("mkbfv::LinearTransform: a diagonal is given twice (indices are taken mod N/2)");
                idx.insert(k);
            }
        long best = -1;
        for (int m = n1_ ? n1_ : 1; m <= (n1_ ? n1_ : 16); m *= 2) {
            std::set<int> b, g;
            for (int k : idx) { b.insert(k % m); g.insert(k - k % m); }
            const long cost = (long)(b.size() - b.count(0) + g.size() - g.count(0));
            if (g.size() <= 64 && (best < 0 || cost < best)) { best = cost; n1 = m; babies.assign(b.begin(), b.end()); }
        }
        if (best < 0) throw Error("mkbfv::LinearTransform: more than 64 giant steps");
        std::vector<uint64_t> rows;
        for (int s = 0; s < 2; ++s) {
            std::set<int> g;
            for (auto& kv : part[s]) g.insert(kv.first - kv.first % n1);
            (s ? giantsE : giantsD).assign(g.begin(), g.end());
            for (int gi : g) {
                uint32_t mask = 0;
                for (size_t i = 0; i < babies.size(); ++i) {
                    auto it = part[s].find(gi + babies[i]);
                    if (it == part[s].end()) continue;
                    mask |= 1u << i;
                    // roll(d_(g+b), g) along each row; the swapped part with its rows exchanged (e~_k[r] = e_k[1 - r])
                    for (int r = 0; r < 2; ++r) {
                        const int64_t* d = it->second->data() + (size_t)(s ? 1 - r : r) * n;
                        for (int j = 0; j < n; ++j) rows.push_back((uint64_t)d[(j - gi + n) % n]);
                    }
                }
                masks.push_back(mask);
            }
        }
        if (masks.size() > 64) throw Error("mkbfv::LinearTransform: more than 64 giant steps over the two parts");
        nnz = (int)(rows.size() / (2 * (size_t)n));
        mkrlwe::DeviceWords z(p, rows.size());
        z.upload(rows.data());
        pt = std::make_unique<mkrlwe::DeviceWords>(p, (size_t)nnz * p.QCount() * p.N());
        check(mkhe_bfv_encode_mul(p.ctx, nnz, z.d, pt->d));
    }
    // the sorted non-zero baby and giant indices: what AddCRS and the rotation keys must cover
    std::vector<int> Rotations() const {
        std::set<int> r(babies.begin(), babies.end());
        r.insert(giantsD.begin(), giantsD.end()); r.insert(giantsE.begin(), giantsE.end());
        r.erase(0);
        return std::vector<int>(r.begin(), r.end());
    }
    // whether a conjugation key per party and CRS[-2] are needed
    bool NeedsConjugation() const { return !giantsE.empty(); }
    Parameters& params;
    int n, n1 = 1, nnz = 0;
    std::vector<int> babies, giantsD, giantsE;
    std::vector<uint32_t> masks;
    std::unique_ptr<mkrlwe::DeviceWords> pt;
};
// mkbfv.Evaluator (evaluator.go:7-20)
class Evaluator {
  public:
    explicit Evaluator(Parameters& p) : params(p), ksw(p) {}
    CiphertextPtr AddNew(const Ciphertext& op0, const Ciphertext& op1) { auto o = bin(op0, op1); check(mkhe_ct_add(params.ctx, op0.h, op1.h, o->h)); return o; }   // :44-52
    CiphertextPtr SubNew(const Ciphertext& op0, const Ciphertext& op1) { auto o = bin(op0, op1); check(mkhe_ct_sub(params.ctx, op0.h, op1.h, o->h)); return o; }   // :54-76
    // evaluator.go:95-113 -> KeySwitcher.MulAndRelinBFV (keyswitch.go:115-251): the non-hoisted twin on its own device path
    CiphertextPtr mulRelin(const Ciphertext& op0, const Ciphertext& op1, RelinearizationKeySet& rlkSet) { return MulRelinNew(op0, op1, rlkSet, false); }
    CiphertextPtr MulRelinNew(const Ciphertext& op0, const Ciphertext& op1, RelinearizationKeySet& rlkSet, bool hoisted = true) {  // evaluator.go:78-82,118-140
        if (!params.CRS.count(-1)) throw Error("mkhe: CRS[-1] (u) has not been uploaded");
        auto out = bin(op0, op1);
        std::vector<const mkhe_swk*> b1, b2, d1, d2, v;
        for (auto& i : op1.ids) { auto& k = rlkSet.GetRelinearizationKey(i); b1.push_back(k.Value[0]->Value[0]->h); b2.push_back(k.Value[1]->Value[0]->h); }
        for (auto& i : op0.ids) {
            auto& k = rlkSet.GetRelinearizationKey(i);
            d1.push_back(k.Value[0]->Value[1]->h); d2.push_back(k.Value[1]->Value[1]->h); v.push_back(k.Value[0]->Value[2]->h);
        }
        check((hoisted ? mkhe_bfv_mul_relin : mkhe_bfv_mul_relin_unhoisted)(params.ctx, op0.h, op1.h, b1.data(), b2.data(), d1.data(), d2.data(), v.data(), params.CRS[-1]->h, out->h));
        return out;
    }
    // mkhe_bfv_mul_relin_sum as it is (no reference counterpart): ctOut = sum_k ops0[k] * ops1[k] under one Quantize and one relinearisation tail.
    // Every ops0[k] carries the ids of ops0[0], every ops1[k] those of ops1[0]; 1 to 16 pairs; ctOut carries the union of the ids
    void MulRelinSum(const std::vector<const Ciphertext*>& ops0, const std::vector<const Ciphertext*>& ops1, RelinearizationKeySet& rlkSet, Ciphertext& ctOut) {
        if (ops0.empty() || ops0.size() != ops1.size()) throw Error("MulRelinSum: as many first operands as second ones, at least one pair");
        if (!params.CRS.count(-1)) throw Error("mkhe: CRS[-1] (u) has not been uploaded");
        std::vector<const mkhe_ct*> a, b;
        std::vector<const mkhe_swk*> b1, b2, d1, d2, v;
        for (auto* c : ops0) a.push_back(c->h);
        for (auto* c : ops1) b.push_back(c->h);
        for (auto& i : ops1[0]->ids) { auto& k = rlkSet.GetRelinearizationKey(i); b1.push_back(k.Value[0]->Value[0]->h); b2.push_back(k.Value[1]->Value[0]->h); }
        for (auto& i : ops0[0]->ids) {
            auto& k = rlkSet.GetRelinearizationKey(i);
            d1.push_back(k.Value[0]->Value[1]->h); d2.push_back(k.Value[1]->Value[1]->h); v.push_back(k.Value[0]->Value[2]->h);
        }
        check(mkhe_bfv_mul_relin_sum(params.ctx, (int)a.size(), a.data(), b.data(), b1.data(), b2.data(), d1.data(), d2.data(), v.data(), params.CRS[-1]->h, ctOut.h));
    }
    CiphertextPtr MulRelinSumNew(const std::vector<const Ciphertext*>& ops0, const std::vector<const Ciphertext*>& ops1, RelinearizationKeySet& rlkSet) {
        if (ops0.empty() || ops0.size() != ops1.size()) throw Error("MulRelinSum: as many first operands as second ones, at least one pair");
        auto out = bin(*ops0[0], *ops1[0]);
        MulRelinSum(ops0, ops1, rlkSet, *out);
        return out;
    }
    // mkhe_bfv_ct_lincomb as it is (no reference counterpart; include/mkhe.h, "BFV weighted sums"): outs[g] = sum_b W[g][b] cts[b] + C[g] for every g as
    // one launch.  dev_consts: device uint64[outs.size()][cts.size() + 1][nQ], row 0 of an output its constant (plain), rows 1 .. its weights (Montgomery form)
    void LinCombs(const std::vector<const mkhe_ct*>& cts, const void* dev_consts, const std::vector<mkhe_ct*>& outs) {
        check(mkhe_bfv_ct_lincomb(params.ctx, (int)cts.size(), cts.data(), (int)outs.size(), dev_consts, outs.data()));
    }
    CiphertextPtr RotateNew(const Ciphertext& ct0, int rotidx, mkrlwe::RotationKeySet& rkSet) {                                    // evaluator.go:142-180 (precomputed indices)
        auto out = std::make_unique<Ciphertext>(params, ct0.IDSet_(), false);
        ksw.Rotate(ct0, rotidx, rkSet, *out);
        return out;
    }
    CiphertextPtr ConjugateNew(const Ciphertext& ct0, mkrlwe::ConjugationKeySet& ckSet) {                                          // evaluator.go:182-192
        auto out = std::make_unique<Ciphertext>(params, ct0.IDSet_(), false);
        ksw.Conjugate(ct0, ckSet, *out);
        return out;
    }
    // Plaintext operands (no reference counterpart; include/mkhe.h, "BFV plaintext operands").  The result carries the ids of ct: no party is added.
    // dev_ptmul: the prepared plaintext of Encoder::EncodeMul; dev_pt: the scaled plaintext of Encoder::Encode.  uint64[nQ][N] each.
    CiphertextPtr MulPtxtNew(const Ciphertext& ct, const void* dev_ptmul) {
        auto out = std::make_unique<Ciphertext>(params, ct.IDSet_(), false);
        const mkhe_ct* in = ct.h; mkhe_ct* o = out->h;
        check(mkhe_bfv_ct_mul_ptxt(params.ctx, 1, &in, dev_ptmul, 0, &o));
        return out;
    }
    CiphertextPtr AddPtxtNew(const Ciphertext& ct, const void* dev_pt) { return addPtxt(0, ct, dev_pt); }
    CiphertextPtr SubPtxtNew(const Ciphertext& ct, const void* dev_pt) { return addPtxt(1, ct, dev_pt); }
    // Hoisted rotations, as mkckks::Evaluator has them: every mkrlwe-level call works on a BFV context.  The same ciphertext as RotateNew, bit for bit.
    std::unique_ptr<mkrlwe::HoistedCiphertext> HoistedForm(const Ciphertext& ct) {
        auto h = std::make_unique<mkrlwe::HoistedCiphertext>();
        std::vector<mkhe_swk*> outs;
        for (auto& id : ct.ids) { h->Value[id] = mkrlwe::NewSwitchingKey(params); outs.push_back(h->Value[id]->h); }
        check(mkhe_hoisted_form(params.ctx, ct.Level(), ct.h, outs.data()));
        return h;
    }
    CiphertextPtr RotateHoistedNew(const Ciphertext& ct0, int rotidx, const mkrlwe::HoistedCiphertext& hoisted, mkrlwe::RotationKeySet& rkSet) {
        const int n2 = params.N() / 2;
        rotidx = ((rotidx % n2) + n2) % n2;
        auto out = std::make_unique<Ciphertext>(params, ct0.IDSet_(), false);
        if (rotidx == 0) { check(mkhe_ct_copy(params.ctx, ct0.h, out->h)); return out; }
        if (!params.CRS.count(rotidx)) throw Error("Hoisted rotation only works for precomputed rotation keys");
        ksw.RotateHoisted(ct0, rotidx, &hoisted, rkSet, *out);
        return out;
    }
    // M z for the diagonals of lt (no reference counterpart; the fused form of the Python mirror's LinearTransformNew): HoistedForm, the non-zero baby
    // rotations as lanes of one mkhe_rotate_multi, ONE mkhe_bfv_ct_ptxt_dot, the non-zero giant rotations as lanes of one mkhe_rotate_multi, mkhe_ct_sum
    // per part in groups of 16, mkhe_conjugate of the row-swapping sum, mkhe_ct_add.  Throws before any engine call when a CRS or a key is missing.
    CiphertextPtr LinearTransformNew(const Ciphertext& ct, const LinearTransform& lt, mkrlwe::RotationKeySet& rkSet, mkrlwe::ConjugationKeySet* ckSet = nullptr) {
        if (&lt.params != &params) throw Error("LinearTransform: the transform was encoded for other parameters");
        for (int r : lt.Rotations()) {
            if (!params.CRS.count(r)) throw Error("LinearTransform: no CRS for rotation index " + std::to_string(r));
            for (auto& i : ct.ids) rkSet.GetRotationKey(i, r);
        }
        if (lt.NeedsConjugation()) {
            if (!ckSet) throw Error("LinearTransform: the transform swaps the slot rows: pass the conjugation keys (ckSet)");
            if (!params.CRS.count(-2)) throw Error("LinearTransform: no CRS for the conjugation (CRS[-2])");
            for (auto& i : ct.ids) ckSet->GetConjugationKey(i);
        }
        std::vector<int> nzb;
        for (int b : lt.babies) if (b) nzb.push_back(b);
        std::vector<CiphertextPtr> rotated;
        if (!nzb.empty()) {
            auto hoisted = HoistedForm(ct);
            rotated = rotateLanes(std::vector<const Ciphertext*>(nzb.size(), &ct), nzb, hoisted.get(), rkSet);
        }
        std::vector<const mkhe_ct*> in;
        for (size_t i = 0, k = 0; i < lt.babies.size(); ++i) in.push_back(lt.babies[i] ? rotated[k++]->h : ct.h);
        std::vector<CiphertextPtr> inner;
        std::vector<mkhe_ct*> outs;
        for (size_t g = 0; g < lt.masks.size(); ++g) { inner.push_back(std::make_unique<Ciphertext>(params, ct.IDSet_(), false)); outs.push_back(inner.back()->h); }
        check(mkhe_bfv_ct_ptxt_dot(params.ctx, 1, (int)in.size(), in.data(), (int)outs.size(), lt.masks.data(), lt.pt->d, outs.data()));
        std::vector<int> giants(lt.giantsD);
        giants.insert(giants.end(), lt.giantsE.begin(), lt.giantsE.end());
        std::vector<const Ciphertext*> gsrc;
        std::vector<int> grot;
        for (size_t g = 0; g < giants.size(); ++g) if (giants[g]) { gsrc.push_back(inner[g].get()); grot.push_back(giants[g]); }
        if (!grot.empty()) {
            auto moved = rotateLanes(gsrc, grot, nullptr, rkSet);
            for (size_t g = 0, k = 0; g < giants.size(); ++g) if (giants[g]) inner[g] = std::move(moved[k++]);
        }
        CiphertextPtr total;
        const size_t nd = lt.giantsD.size();
        if (nd) total = summed(std::vector<CiphertextPtr>(std::make_move_iterator(inner.begin()), std::make_move_iterator(inner.begin() + nd)));
        if (lt.NeedsConjugation()) {
            auto sw = ConjugateNew(*summed(std::vector<CiphertextPtr>(std::make_move_iterator(inner.begin() + nd), std::make_move_iterator(inner.end()))), *ckSet);
            total = total ? AddNew(*total, *sw) : std::move(sw);
        }
        return total;
    }
    Parameters& params;
    mkrlwe::KeySwitcher ksw;
  private:
    // srcs[i] rotated by rots[i] != 0 as lanes of one mkhe_rotate_multi; hoist: the hoisted form every lane shares, or null
    std::vector<CiphertextPtr> rotateLanes(const std::vector<const Ciphertext*>& srcs, const std::vector<int>& rots, const mkrlwe::HoistedCiphertext* hoist,
                                           mkrlwe::RotationKeySet& rkSet) {
        std::vector<CiphertextPtr> res;
        std::vector<uint64_t> gal;
        std::vector<const mkhe_ct*> in;
        std::vector<mkhe_ct*> out;
        std::vector<const mkhe_swk*> hs, rk, crs;
        for (size_t l = 0; l < srcs.size(); ++l) {
            res.push_back(std::make_unique<Ciphertext>(params, srcs[l]->IDSet_(), false));
            gal.push_back(params.GaloisElementForColumnRotationBy(rots[l]));
            in.push_back(srcs[l]->h); out.push_back(res.back()->h); crs.push_back(params.CRS.at(rots[l])->h);
            for (auto& i : srcs[l]->ids) { rk.push_back(rkSet.GetRotationKey(i, rots[l]).Value->h); if (hoist) hs.push_back(hoist->Value.at(i)->h); }
        }
        check(mkhe_rotate_multi(params.ctx, (int)srcs.size(), gal.data(), in.data(), hoist ? hs.data() : nullptr, rk.data(), crs.data(), nullptr, out.data()));
        return res;
    }
    // the sum of 1 .. 64 ciphertexts of one shape: mkhe_ct_sum in groups of 16
    CiphertextPtr summed(std::vector<CiphertextPtr> terms) {
        while (terms.size() > 1) {
            std::vector<CiphertextPtr> next;
            for (size_t i = 0; i < terms.size(); i += 16) {
                std::vector<const mkhe_ct*> grp;
                for (size_t k = i; k < std::min(terms.size(), i + 16); ++k) grp.push_back(terms[k]->h);
                next.push_back(std::make_unique<Ciphertext>(params, terms[i]->IDSet_(), false));
                check(mkhe_ct_sum(params.ctx, (int)grp.size(), grp.data(), next.back()->h));
            }
            terms = std::move(next);
        }
        return std::move(terms[0]);
    }
    CiphertextPtr bin(const Ciphertext& a, const Ciphertext& b) { return std::make_unique<Ciphertext>(params, mkrlwe::Union(a.IDSet_(), b.IDSet_()), false); }
    CiphertextPtr addPtxt(int op, const Ciphertext& ct, const void* dev_pt) {
        auto out = std::make_unique<Ciphertext>(params, ct.IDSet_(), false);
        const mkhe_ct* in = ct.h; mkhe_ct* o = out->h;
        check(mkhe_bfv_ct_add_ptxt(params.ctx, op, 1, &in, dev_pt, 0, &o));
        return out;
    }
};
// The batch encoder on the device (mkhe_bfv_encode / mkhe_bfv_decode): EncodeInt of mkbfv/encryptor.go:38-41 and DecodeInt of
// mkbfv/decryptor.go:52-54.  lattigo's bfv.Encoder, which those lines call, is not in the reference tree: this is the mathematics of slot
// batching over Z_T (include/mkhe.h: Slots() = N int64 values per message, two rows of N/2), not lattigo's code path.  Messages cross the bus
// as slots; plaintexts are device buffers uint64[count][nQ][N], coefficient domain: what mkrlwe::Encryptor takes and Decryptor writes.
class Encoder {
  public:
    explicit Encoder(Parameters& p) : params(p) {}
    int Slots() const { return params.N(); }
    // the 2N-th root of unity mod T of the slot definition; throws where the plaintext modulus is not supported
    uint64_t SlotPsi() {
        const uint64_t psi = mkhe_ctx_bfv_slot_psi(params.ctx);
        if (!psi) throw Error(mkhe_last_error());
        return psi;
    }
    // count messages (host: count * Slots() values, any int64) -> dev_pt, as one launch set
    void Encode(int count, const int64_t* values, void* dev_pt) {
        mkrlwe::DeviceWords z(params, (size_t)count * params.N());
        check(mkhe_buf_upload(params.ctx, z.d, reinterpret_cast<const uint64_t*>(values), z.words));
        check(mkhe_bfv_encode(params.ctx, count, z.d, dev_pt));
    }
    // count messages -> dev_ptmul uint64[count][nQ][N], the prepared multiplication plaintexts (NTT over Q of the centred lift, Montgomery form):
    // the operand of Evaluator::MulPtxtNew.  No reference counterpart.
    void EncodeMul(int count, const int64_t* values, void* dev_ptmul) {
        mkrlwe::DeviceWords z(params, (size_t)count * params.N());
        check(mkhe_buf_upload(params.ctx, z.d, reinterpret_cast<const uint64_t*>(values), z.words));
        check(mkhe_bfv_encode_mul(params.ctx, count, z.d, dev_ptmul));
    }
    // count plaintexts -> values (host: count * Slots()), centred in (-T/2, T/2]
    void Decode(int count, const void* dev_pt, int64_t* values) {
        mkrlwe::DeviceWords z(params, (size_t)count * params.N());
        check(mkhe_bfv_decode(params.ctx, count, dev_pt, z.d));
        z.download(reinterpret_cast<uint64_t*>(values));
    }
    Parameters& params;
};
// mkrlwe::Decryptor with the noise measures of BFV (include/mkhe.h, "noise measurement").  InvariantNoise: r = max |[T phase]_Q| (kind 1), no message
// needed.  NoiseBudget = bitlen(Q) - bitlen(r) - 1 >= 0.  NoiseNorm with a message (Slots() values): max |e| exactly, the residual against
// mkhe_bfv_encode(msg); without: the bound (r + T / 2) / T + 1, which lies in [max |e|, max |e| + 2] while the noise has not wrapped.  NoiseBits is
// what the floodBits of a ShareNew must exceed.
class Decryptor : public mkrlwe::Decryptor {
  public:
    explicit Decryptor(Parameters& p) : mkrlwe::Decryptor(p), bfv(p) {}
    mkrlwe::NoiseValue InvariantNoise(const mkrlwe::Ciphertext& ct, const mkrlwe::SecretKeySet& skSet) { return mkrlwe::Decryptor::NoiseNorm(ct, skSet, nullptr, 1); }
    int NoiseBudget(const mkrlwe::Ciphertext& ct, const mkrlwe::SecretKeySet& skSet) {
        mkrlwe::NoiseValue q;
        q.Words.push_back(1);
        for (uint64_t m : bfv.Q()) q.MulAdd(m, 0);
        return q.Bits() - InvariantNoise(ct, skSet).Bits() - 1;
    }
    mkrlwe::NoiseValue NoiseNorm(const mkrlwe::Ciphertext& ct, const mkrlwe::SecretKeySet& skSet, const int64_t* msg = nullptr) {
        if (msg) {
            mkrlwe::DeviceWords ref(bfv, (size_t)bfv.QCount() * bfv.N());
            Encoder(bfv).Encode(1, msg, ref.d);
            return mkrlwe::Decryptor::NoiseNorm(ct, skSet, ref.d);
        }
        mkrlwe::NoiseValue r = InvariantNoise(ct, skSet);
        r.Index = -1;
        return r.MulAdd(1, bfv.T() / 2).Div(bfv.T()).MulAdd(1, 1);
    }
    int NoiseBits(const mkrlwe::Ciphertext& ct, const mkrlwe::SecretKeySet& skSet, const int64_t* msg = nullptr) { return NoiseNorm(ct, skSet, msg).Bits(); }
  private:
    Parameters& bfv;
};

// mkrlwe::SecretShare over Z_T (include/mkhe.h, "encryption to shares"): coefficients uint64[count][N], each below T, in the format mkhe_bfv_scale_down
// writes; no level.  Slots() is the share of the SLOTS: additive mod T slot by slot, as the transform is Z_T-linear.
struct SecretShare : mkrlwe::SecretShare {
    SecretShare(Parameters& p, std::string id, int count = 1) : mkrlwe::SecretShare(p, std::move(id), -1, count, 1), bfv(p) {}
    // -> values (host: Count * N), centred
    void Slots(int64_t* values) const {
        mkrlwe::DeviceWords z(bfv, Value.words);
        check(mkhe_bfv_coeffs_to_slots(bfv.ctx, Count, Value.d, z.d));
        z.download(reinterpret_cast<uint64_t*>(values));
    }
    // the inverse: count * N slots (any int64) -> the share whose Slots() they are mod T
    static std::shared_ptr<SecretShare> FromSlots(Parameters& p, int count, const int64_t* values, std::string id = std::string()) {
        auto out = std::make_shared<SecretShare>(p, std::move(id), count);
        mkrlwe::DeviceWords z(p, out->Value.words);
        z.upload(reinterpret_cast<const uint64_t*>(values));
        check(mkhe_bfv_slots_to_coeffs(p.ctx, count, z.d, out->Value.d));
        return out;
    }
    Parameters& bfv;
};

// out_slot[i] = mult[i] * in_slot[index[i]] mod T for 0 <= i < N (include/mkhe.h, "BFV slot map"), slots numbered as the batch encoder numbers them (two
// rows of N/2): any permutation, replication or slot-wise scaling.  index: N values in 0 .. N-1, any function; mult: N values taken mod T, empty = all
// ones.  Prepared once, in the constructor (mkhe_bfv_slot_map_prepare, which refuses an index >= N).
class SlotMap {
  public:
    SlotMap(Parameters& p, std::vector<uint32_t> index_, std::vector<uint64_t> mult_ = {}) : params(p), index(std::move(index_)), mult(std::move(mult_)), map_(p, (size_t)p.N()) {
        const size_t N = (size_t)p.N();
        if (index.size() != N || (!mult.empty() && mult.size() != N)) throw Error("mkbfv::SlotMap: index and mult have N entries");
        if (mult.empty()) mult.assign(N, 1);
        for (auto& m : mult) m %= p.T();
        mkrlwe::DeviceWords in(p, N + N / 2);                              // mult, then the index as uint32[N]
        std::vector<uint64_t> host(N + N / 2, 0);
        std::copy(mult.begin(), mult.end(), host.begin());
        std::memcpy(host.data() + N, index.data(), N * sizeof(uint32_t));
        in.upload(host.data());
        check(mkhe_bfv_slot_map_prepare(p.ctx, static_cast<const uint64_t*>(in.d) + N, in.d, map_.d));
    }
    static std::shared_ptr<SlotMap> Permutation(Parameters& p, const std::vector<uint32_t>& perm) {
        std::vector<char> seen(perm.size(), 0);
        for (uint32_t v : perm) { if (v >= perm.size() || seen[v]) throw Error("mkbfv::SlotMap: Permutation takes a permutation of 0 .. N-1"); seen[v] = 1; }
        return std::make_shared<SlotMap>(p, perm);
    }
    // what RotateNew(ct, k) does to the slots: slot i + k moves to slot i within each row of N/2; swapRows: and the rows change places
    static std::shared_ptr<SlotMap> Rotation(Parameters& p, int k, bool swapRows = false) {
        const int N = p.N(), half = N / 2;
        std::vector<uint32_t> idx(N);
        for (int i = 0; i < N; ++i) idx[i] = (uint32_t)((((i / half) ^ (swapRows ? 1 : 0)) * half) + (((i % half + k) % half + half) % half));
        return std::make_shared<SlotMap>(p, std::move(idx));
    }
    // the host definition: (mult * values[index]) mod T, centred (one message of N slots)
    std::vector<int64_t> Apply(const int64_t* values) const {
        const int64_t T = (int64_t)params.T();
        std::vector<int64_t> out(index.size());
        for (size_t i = 0; i < out.size(); ++i) {
            const uint64_t v = (uint64_t)(((values[index[i]] % T) + T) % T);
            const int64_t r = (int64_t)(v * mult[i] % (uint64_t)T);         // both below 2^32: the product fits
            out[i] = r > T / 2 ? r - T : r;
        }
        return out;
    }
    // the map applied to a SecretShare -> a new SecretShare of the same party: one engine call
    std::shared_ptr<SecretShare> MapCoeffs(const SecretShare& s) const {
        auto out = std::make_shared<SecretShare>(params, s.ID, s.Count);
        check(mkhe_bfv_slot_map(params.ctx, s.Count, s.Value.d, map_.d, out->Value.d));
        return out;
    }
    const void* dev() const { return map_.d; }
    Parameters& params;
    std::vector<uint32_t> index;
    std::vector<uint64_t> mult;
  private:
    mkrlwe::DeviceWords map_;
};

// HE <-> additive secret sharing over Z_T for MK-BFV, exact slot by slot (the Python mirror's mkbfv.ShareConverter).  E2S: every party runs
// E2SShareBatch, publishes the DecryptionShare (Refresher::ShareBatch's, bit for bit) and KEEPS the SecretShare (T - A); anyone runs E2SMergeBatch
// (mkhe_decrypt_merge, then mkhe_bfv_scale_down), which gives the public share w = (m + sum A_i) mod T.  S2E: every party encrypts its share
// (mkhe_bfv_scale_up, mkhe_encrypt_seeded), S2EMergeNew is the AddNew chain, and the public share, scaled up, is added to the result as a plaintext.
class ShareConverter {
  public:
    explicit ShareConverter(Parameters& p) : params(p) {}
    std::pair<std::shared_ptr<mkrlwe::DecryptionShare>, std::shared_ptr<SecretShare>> E2SShareBatch(const std::vector<const mkrlwe::Ciphertext*>& cts, const mkrlwe::SecretKey& sk,
                                                                                                    int floodBits, mkrlwe::DeviceSampler& sampler) {
        if (cts.empty()) throw Error("Cannot E2SShare: no ciphertext");
        if (floodBits < 0 || floodBits > 1024) throw Error("Cannot E2SShare: floodBits must be 0 .. 1024");
        std::vector<const mkhe_ct*> in;
        std::vector<int> slots;
        for (auto* ct : cts) { in.push_back(ct->h); slots.push_back(ct->slot(sk.ID)); }
        auto pub = std::make_shared<mkrlwe::DecryptionShare>(params, sk.ID, params.MaxLevel(), (int)cts.size());
        auto sec = std::make_shared<SecretShare>(params, sk.ID, (int)cts.size());
        check(mkhe_bfv_e2s_share(params.ctx, (int)cts.size(), in.data(), slots.data(), sk.Value.d, sampler.Key(), sampler.NextNonce(), floodBits, pub->Value.d,
                                 sec->Value.d));
        return {pub, sec};
    }
    std::shared_ptr<SecretShare> E2SMergeBatch(const std::vector<const mkrlwe::Ciphertext*>& cts, const std::vector<const mkrlwe::DecryptionShare*>& shares) {
        if (cts.empty()) throw Error("Cannot E2SMerge: no ciphertext");
        std::vector<const mkhe_ct*> in;
        for (auto* ct : cts) in.push_back(ct->h);
        const std::vector<const void*> ordered = mkrlwe::ShareConverter::orderShares(*cts[0], (int)cts.size(), shares);
        mkrlwe::DeviceWords pt(params, (size_t)cts.size() * params.QCount() * params.N());
        check(mkhe_decrypt_merge(params.ctx, (int)cts.size(), in.data(), (int)ordered.size(), ordered.data(), pt.d));
        auto out = std::make_shared<SecretShare>(params, std::string(), (int)cts.size());
        check(mkhe_bfv_scale_down(params.ctx, (int)cts.size(), pt.d, out->Value.d));
        return out;
    }
    std::vector<std::shared_ptr<Ciphertext>> S2EShareBatch(const SecretShare& secret, const mkrlwe::PublicKey& pk, mkrlwe::DeviceSampler& sampler) {
        if (!secret.ID.empty() && secret.ID != pk.ID) throw Error("Cannot S2EShare: the share and pk belong to different parties");
        mkrlwe::SecretShare pt(params, secret.ID, params.MaxLevel(), secret.Count);
        std::vector<std::shared_ptr<Ciphertext>> cts;
        std::vector<mkhe_ct*> out;
        for (int b = 0; b < secret.Count; ++b) { cts.push_back(std::make_shared<Ciphertext>(params, mkrlwe::IDSet{pk.ID}, false)); out.push_back(cts.back()->h); }
        check(mkhe_bfv_scale_up(params.ctx, secret.Count, secret.Value.d, pt.Value.d));
        const int rc = mkhe_encrypt_seeded(params.ctx, params.MaxLevel(), secret.Count, pk.Value.d, pt.Value.d, 0, sampler.Key(), sampler.NextNonce(), sampler.cdt.data(),
                                           (int)sampler.cdt.size(), out.data());
        pt.Wipe();
        check(rc);
        return cts;
    }
    std::shared_ptr<Ciphertext> S2EMergeNew(const std::vector<const Ciphertext*>& ctsByParty, const SecretShare* pub = nullptr) {
        if (ctsByParty.empty()) throw Error("Cannot S2EMerge: no ciphertext");
        if (pub && pub->Count != 1) throw Error("Cannot S2EMerge: the public share of one ciphertext expected");
        mkrlwe::IDSet ids = ctsByParty[0]->IDSet_();
        auto acc = std::make_shared<Ciphertext>(params, ids, false);
        check(mkhe_ct_copy(params.ctx, ctsByParty[0]->h, acc->h));
        for (size_t i = 1; i < ctsByParty.size(); ++i) {
            ids = mkrlwe::Union(ids, ctsByParty[i]->IDSet_());
            auto out = std::make_shared<Ciphertext>(params, ids, false);
            check(mkhe_ct_add(params.ctx, acc->h, ctsByParty[i]->h, out->h));
            acc = out;
        }
        if (pub) {
            mkrlwe::DeviceWords pt(params, (size_t)params.QCount() * params.N());
            check(mkhe_bfv_scale_up(params.ctx, 1, pub->Value.d, pt.d));
            auto out = std::make_shared<Ciphertext>(params, ids, false);
            const mkhe_ct* in = acc->h; mkhe_ct* o = out->h;
            check(mkhe_bfv_ct_add_ptxt(params.ctx, 0, 1, &in, pt.d, 0, &o));
            acc = out;
        }
        return acc;
    }
    Parameters& params;
};

// The collective refresh of MK-BFV between parties (include/mkhe.h, "collective refresh for MK-BFV"): ShareNew (each party, on its own keys and its
// own DeviceSampler) and MergeNew (anyone) give a ciphertext of the same message over the same parties with the noise of a fresh encryption.  What
// travels is mkrlwe::RefreshShare, with both levels the maximum level.  The caller chooses floodBits: floodBits minus the bit size of the
// ciphertext's noise is the statistical hiding of that noise, and the noise plus parties * 2^(floodBits-1) must stay below Q / (2T) (the Python
// mirror's Refresher.MaxFloodBits).  The mask is always on.
class Refresher {
  public:
    explicit Refresher(Parameters& p) : params(p) {}
    // floodBits = 0 .. 1024, at most bitlen(Q div 2T) - 1.  Two nonces of `sampler` serve the call.
    std::shared_ptr<mkrlwe::RefreshShare> ShareBatch(const std::vector<const mkrlwe::Ciphertext*>& cts, const mkrlwe::SecretKey& sk, const mkrlwe::PublicKey& pk,
                                                     int floodBits, mkrlwe::DeviceSampler& sampler) {
        if (cts.empty()) throw Error("Cannot RefreshShare: no ciphertext");
        if (sk.ID != pk.ID) throw Error("Cannot RefreshShare: sk and pk belong to different parties");
        if (floodBits < 0 || floodBits > 1024) throw Error("Cannot RefreshShare: floodBits must be 0 .. 1024");
        std::vector<const mkhe_ct*> in;
        std::vector<int> slots;
        for (auto* ct : cts) { in.push_back(ct->h); slots.push_back(ct->slot(sk.ID)); }
        const int level = params.MaxLevel();
        auto out = std::make_shared<mkrlwe::RefreshShare>(params, sk.ID, level, level, (int)cts.size());
        std::vector<mkhe_ct*> re;
        for (auto& c : out->Reenc) re.push_back(c->h);
        const uint64_t nonce = sampler.NextNoncePair();
        check(mkhe_bfv_refresh_share(params.ctx, (int)cts.size(), in.data(), slots.data(), sk.Value.d, pk.Value.d, sampler.Key(), nonce, nonce + 1, 1, floodBits,
                                     sampler.cdt.data(), (int)sampler.cdt.size(), out->Share.Value.d, re.data()));
        return out;
    }
    std::shared_ptr<mkrlwe::RefreshShare> ShareNew(const mkrlwe::Ciphertext& ct, const mkrlwe::SecretKey& sk, const mkrlwe::PublicKey& pk, int floodBits,
                                                   mkrlwe::DeviceSampler& sampler) {
        return ShareBatch({&ct}, sk, pk, floodBits, sampler);
    }
    // one RefreshShare of count cts.size() per party, in any order, for ciphertexts over the same ids -> the refreshed ciphertexts
    std::vector<std::shared_ptr<Ciphertext>> MergeBatch(const std::vector<const mkrlwe::Ciphertext*>& cts, const std::vector<const mkrlwe::RefreshShare*>& shares) {
        if (cts.empty()) throw Error("Cannot RefreshMerge: no ciphertext");
        std::vector<const mkhe_ct*> in;
        for (auto* ct : cts) in.push_back(ct->h);
        std::vector<const void*> ordered;
        std::vector<const mkhe_ct*> re;
        for (auto& id : cts[0]->ids) {
            const mkrlwe::RefreshShare* found = nullptr;
            for (auto* sh : shares)
                if (sh->ID == id) { if (found) throw Error("Cannot MergeShares: two shares of one party"); found = sh; }
            if (!found) throw Error("Cannot MergeShares: the share of a party is missing");
            if (found->Share.Count != (int)cts.size()) throw Error("Cannot MergeShares: a share is for another batch size");
            ordered.push_back(found->Share.Value.d);
            for (auto& c : found->Reenc) re.push_back(c->h);
        }
        if (shares.size() != ordered.size()) throw Error("Cannot MergeShares: a share of a party the ciphertext does not have");
        std::vector<std::shared_ptr<Ciphertext>> outs;
        std::vector<mkhe_ct*> oh;
        for (size_t b = 0; b < cts.size(); ++b) { outs.push_back(std::make_shared<Ciphertext>(params, cts[0]->IDSet_(), false)); oh.push_back(outs.back()->h); }
        check(mkhe_bfv_refresh_merge(params.ctx, (int)cts.size(), in.data(), (int)ordered.size(), ordered.data(), re.data(), oh.data()));
        return outs;
    }
    std::shared_ptr<Ciphertext> MergeNew(const mkrlwe::Ciphertext& ct, const std::vector<const mkrlwe::RefreshShare*>& shares) { return MergeBatch({&ct}, shares)[0]; }
    // The refresh that applies a slot map: the result encrypts map.Apply(message), with no rotation key and no key switch.  The map is Z_T-linear, so it
    // commutes with the masks.  ShareMapBatch = mkhe_bfv_e2s_share -> mkhe_bfv_slot_map -> mkhe_bfv_scale_up -> mkhe_encrypt_seeded on the two nonces
    // ShareBatch takes; with the identity map it is ShareBatch's, bit for bit.  The intermediate secret buffers are zeroed behind their last use.
    std::shared_ptr<mkrlwe::RefreshShare> ShareMapBatch(const std::vector<const mkrlwe::Ciphertext*>& cts, const mkrlwe::SecretKey& sk, const mkrlwe::PublicKey& pk,
                                                        int floodBits, mkrlwe::DeviceSampler& sampler, const SlotMap& map) {
        if (cts.empty()) throw Error("Cannot RefreshShare: no ciphertext");
        if (sk.ID != pk.ID) throw Error("Cannot RefreshShare: sk and pk belong to different parties");
        if (floodBits < 0 || floodBits > 1024) throw Error("Cannot RefreshShare: floodBits must be 0 .. 1024");
        std::vector<const mkhe_ct*> in;
        std::vector<int> slots;
        for (auto* ct : cts) { in.push_back(ct->h); slots.push_back(ct->slot(sk.ID)); }
        const int level = params.MaxLevel(), B = (int)cts.size();
        auto out = std::make_shared<mkrlwe::RefreshShare>(params, sk.ID, level, level, B);
        std::vector<mkhe_ct*> re;
        for (auto& c : out->Reenc) re.push_back(c->h);
        const uint64_t nonce = sampler.NextNoncePair();
        SecretShare sec(params, sk.ID, B);
        mkrlwe::SecretShare pt(params, sk.ID, level, B);
        int rc = mkhe_bfv_e2s_share(params.ctx, B, in.data(), slots.data(), sk.Value.d, sampler.Key(), nonce, floodBits, out->Share.Value.d, sec.Value.d);
        if (!rc) rc = mkhe_bfv_slot_map(params.ctx, B, sec.Value.d, map.dev(), sec.Value.d);
        if (!rc) rc = mkhe_bfv_scale_up(params.ctx, B, sec.Value.d, pt.Value.d);
        if (!rc) rc = mkhe_encrypt_seeded(params.ctx, level, B, pk.Value.d, pt.Value.d, 0, sampler.Key(), nonce + 1, sampler.cdt.data(), (int)sampler.cdt.size(), re.data());
        const std::string err = rc ? mkhe_last_error() : "";
        sec.Wipe();
        pt.Wipe();
        if (rc) throw Error(err);
        return out;
    }
    std::shared_ptr<mkrlwe::RefreshShare> ShareMapNew(const mkrlwe::Ciphertext& ct, const mkrlwe::SecretKey& sk, const mkrlwe::PublicKey& pk, int floodBits,
                                                      mkrlwe::DeviceSampler& sampler, const SlotMap& map) {
        return ShareMapBatch({&ct}, sk, pk, floodBits, sampler, map);
    }
    // MergeBatch for shares made by ShareMapBatch with the same map: E2SMergeBatch -> mkhe_bfv_slot_map -> mkhe_bfv_scale_up, added (mkhe_bfv_ct_add_ptxt)
    // into c_0 of the sum of the re-encryptions (mkhe_ct_add over the unions).  With the identity map it is MergeBatch's, bit for bit.
    std::vector<std::shared_ptr<Ciphertext>> MergeMapBatch(const std::vector<const mkrlwe::Ciphertext*>& cts, const std::vector<const mkrlwe::RefreshShare*>& shares,
                                                           const SlotMap& map) {
        if (cts.empty()) throw Error("Cannot RefreshMerge: no ciphertext");
        if (cts[0]->ids.empty()) throw Error("Cannot RefreshMerge: ciphertexts without parties have nothing to refresh");
        const int B = (int)cts.size();
        std::vector<const mkrlwe::RefreshShare*> ordered;
        std::vector<const mkrlwe::DecryptionShare*> pubs;
        for (auto& id : cts[0]->ids) {
            const mkrlwe::RefreshShare* found = nullptr;
            for (auto* sh : shares)
                if (sh->ID == id) { if (found) throw Error("Cannot MergeShares: two shares of one party"); found = sh; }
            if (!found) throw Error("Cannot MergeShares: the share of a party is missing");
            ordered.push_back(found);
            pubs.push_back(&found->Share);
        }
        if (shares.size() != ordered.size()) throw Error("Cannot MergeShares: a share of a party the ciphertext does not have");
        auto w = ShareConverter(params).E2SMergeBatch(cts, pubs);
        mkrlwe::DeviceWords pt(params, (size_t)B * params.QCount() * params.N());
        check(mkhe_bfv_slot_map(params.ctx, B, w->Value.d, map.dev(), w->Value.d));
        check(mkhe_bfv_scale_up(params.ctx, B, w->Value.d, pt.d));
        std::vector<std::shared_ptr<Ciphertext>> outs;
        for (int b = 0; b < B; ++b) {
            mkrlwe::IDSet ids{ordered[0]->ID};
            std::shared_ptr<mkrlwe::Ciphertext> acc = ordered[0]->Reenc[b];
            for (size_t i = 1; i < ordered.size(); ++i) {
                ids.insert(ordered[i]->ID);
                auto next = std::make_shared<Ciphertext>(params, ids, false);
                check(mkhe_ct_add(params.ctx, acc->h, ordered[i]->Reenc[b]->h, next->h));
                acc = next;
            }
            outs.push_back(std::make_shared<Ciphertext>(params, cts[0]->IDSet_(), false));
            const mkhe_ct* in = acc->h; mkhe_ct* o = outs.back()->h;
            check(mkhe_bfv_ct_add_ptxt(params.ctx, 0, 1, &in, static_cast<const uint64_t*>(pt.d) + (size_t)b * params.QCount() * params.N(), 0, &o));
        }
        return outs;
    }
    std::shared_ptr<Ciphertext> MergeMapNew(const mkrlwe::Ciphertext& ct, const std::vector<const mkrlwe::RefreshShare*>& shares, const SlotMap& map) {
        return MergeMapBatch({&ct}, shares, map)[0];
    }
    Parameters& params;
};
// The collective key switch of mkrlwe::PublicKeySwitcher on mkbfv ciphertexts: the message stays exact as long as NoiseBound plus the noise of
// the input is below Q / (2T).
class PublicKeySwitcher : public mkrlwe::PublicKeySwitcher {
  public:
    explicit PublicKeySwitcher(Parameters& p) : mkrlwe::PublicKeySwitcher(p), bfv(p) {}
    std::vector<std::shared_ptr<Ciphertext>> MergeBatch(const std::vector<const mkrlwe::Ciphertext*>& cts, const std::vector<const mkrlwe::PublicKeySwitchShare*>& shares,
                                                        const std::string& recipient) {
        std::vector<std::shared_ptr<Ciphertext>> outs;
        for (size_t b = 0; b < cts.size(); ++b) outs.push_back(std::make_shared<Ciphertext>(bfv, mkrlwe::IDSet{recipient}, false));
        merge(cts, shares, outs);
        return outs;
    }
    std::shared_ptr<Ciphertext> MergeNew(const mkrlwe::Ciphertext& ct, const std::vector<const mkrlwe::PublicKeySwitchShare*>& shares, const std::string& recipient) {
        return MergeBatch({&ct}, shares, recipient)[0];
    }
  private:
    Parameters& bfv;
};
// mkrlwe::SeededCiphertext over mkbfv ciphertexts (always at the maximum level): ExpandBfv gives them in their own type
class SeededCiphertext : public mkrlwe::SeededCiphertext {
  public:
    SeededCiphertext(Parameters& p, const std::string& id, int count = 1) : mkrlwe::SeededCiphertext(p, id, p.MaxLevel(), fresh_bfv(p, id, count)) {}
    std::vector<std::shared_ptr<Ciphertext>> ExpandBfv() {
        std::vector<std::shared_ptr<Ciphertext>> out;
        for (auto& c : Expand()) out.push_back(std::static_pointer_cast<Ciphertext>(c));
        return out;
    }
  private:
    static std::vector<std::shared_ptr<mkrlwe::Ciphertext>> fresh_bfv(Parameters& p, const std::string& id, int count) {
        std::vector<std::shared_ptr<mkrlwe::Ciphertext>> v;
        for (int b = 0; b < count; ++b) v.push_back(std::make_shared<Ciphertext>(p, mkrlwe::IDSet{id}, false));
        return v;
    }
};
// mkrlwe::SecretKeyEncryptor on mkbfv ciphertexts (plaintexts: the output of Encoder::Encode on the device)
class SecretKeyEncryptor : public mkrlwe::SecretKeyEncryptor {
  public:
    SecretKeyEncryptor(Parameters& p, const mkrlwe::SecretKey& sk_, const uint32_t seed[8]) : mkrlwe::SecretKeyEncryptor(p, sk_, seed), bfv(p) {}
    std::vector<std::shared_ptr<Ciphertext>> EncryptPtxtBatch(int count, const void* dev_pt, mkrlwe::DeviceSampler& sampler) {
        std::vector<std::shared_ptr<Ciphertext>> cts;
        for (int b = 0; b < count; ++b) cts.push_back(std::make_shared<Ciphertext>(bfv, mkrlwe::IDSet{sk.ID}, false));
        into(cts, bfv.MaxLevel(), dev_pt, false, &sampler, nullptr);
        return cts;
    }
    std::shared_ptr<SeededCiphertext> EncryptPtxtSeeded(int count, const void* dev_pt, mkrlwe::DeviceSampler& sampler) {
        auto sc = std::make_shared<SeededCiphertext>(bfv, sk.ID, count);
        seeded(sc, dev_pt, false, &sampler, nullptr);
        return sc;
    }
  private:
    Parameters& bfv;
};
}  // namespace mkbfv
