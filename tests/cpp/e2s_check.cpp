// Uses the mirrors of "encryption to shares" and the BFV slot map of include/mkhe.hpp: mkrlwe::ShareConverter / SecretShare, mkckks::ShareConverter,
// mkbfv::ShareConverter / SecretShare / SlotMap and the map methods of mkbfv::Refresher, and the five C entry points (tests/test_cpp_e2s.py).  Without an
// argument it makes no engine call, which needs no GPU.  With one it runs, three parties at N = 2^10: the identity-map refresh against mkbfv::Refresher
// bit for bit, one permuted refresh against SlotMap::Apply, and on a CKKS context (public + sum of the secret shares) == Decrypt under the input moduli.
#include "mkhe.hpp"
#include <cstdio>

static std::vector<int32_t> ternary(int n, uint64_t seed) {
    std::vector<int32_t> s(n);
    for (int i = 0; i < n; ++i) { seed = seed * 6364136223846793005ULL + 1442695040888963407ULL; s[i] = (int32_t)((seed >> 40) % 3) - 1; }
    return s;
}
static bool fail(const char* what) { std::printf("FAILED: %s\n", what); return false; }

static bool bfv_part() {
    std::vector<uint64_t> Q{0x3fffffffd60001ULL, 0x3fffffff6d0001ULL, 0x3fffffff550001ULL}, QMul{0x3fffffffca0001ULL, 0x3fffffff5d0001ULL, 0x3fffffff390001ULL};
    std::vector<uint64_t> P{0xffffffffffc0001ULL, 0xfffffffff840001ULL};
    mkbfv::Parameters params(10, Q, QMul, P, 65537);
    params.AddCRS(0, (uint64_t)1);
    const int N = params.N(), nQ = params.QCount(), T = 65537;
    const std::vector<std::string> names{"a", "b", "c"};
    mkrlwe::KeyGenerator kgen(params);
    std::vector<std::unique_ptr<mkrlwe::SecretKey>> sks;
    std::vector<std::unique_ptr<mkrlwe::PublicKey>> pks;
    mkrlwe::SecretKeySet skSet;
    const uint32_t key[8] = {1, 2, 3, 4, 5, 6, 7, 8}, other[8] = {8, 7, 6, 5, 4, 3, 2, 1};
    mkrlwe::DeviceSampler fresh(other);
    mkbfv::Encoder encoder(params);
    mkrlwe::Encryptor enc(params);
    mkbfv::Evaluator ev(params);
    mkbfv::Decryptor dec(params);
    std::vector<int64_t> msg(N, 0), got(N);
    std::unique_ptr<mkbfv::Ciphertext> ct;
    for (size_t i = 0; i < names.size(); ++i) {
        sks.push_back(kgen.GenSecretKey(names[i], ternary(N, 11 + i).data()));
        pks.push_back(kgen.GenPublicKey(*sks[i], ternary(N, 21 + i).data()));
        skSet.AddSecretKey(*sks[i]);
        std::vector<int64_t> m(N);
        for (int n = 0; n < N; ++n) { m[n] = (int64_t)((n * 2654435761ULL + 977 * i) % T) - T / 2; msg[n] += m[n]; }
        mkrlwe::DeviceWords pt(params, (size_t)nQ * N);
        encoder.Encode(1, m.data(), pt.d);
        mkbfv::Ciphertext c(params, mkrlwe::IDSet{names[i]}, false);
        enc.Encrypt(pt.d, *pks[i], c, fresh);
        if (!ct) { ct = std::make_unique<mkbfv::Ciphertext>(params, mkrlwe::IDSet{names[i]}, false); mkhe::check(mkhe_ct_copy(params.ctx, c.h, ct->h)); }
        else ct = ev.AddNew(*ct, c);
    }
    for (auto& v : msg) { v = ((v % T) + T) % T; if (v > T / 2) v -= T; }
    auto decode = [&](const mkrlwe::Ciphertext& c) {
        mkrlwe::DeviceWords pt(params, (size_t)nQ * N);
        dec.Decrypt(c, skSet, pt.d);
        encoder.Decode(1, pt.d, got.data());
    };
    decode(*ct);
    if (got != msg) return fail("the sum of three fresh encryptions decrypts to the sum of the messages");

    // twin samplers: the Refresher on one, the map refresh with the identity map on the other
    mkbfv::Refresher ref(params);
    std::vector<uint32_t> id(N), perm(N);
    std::vector<uint64_t> mult(N);
    for (int n = 0; n < N; ++n) { id[n] = (uint32_t)n; perm[n] = (uint32_t)((n * 5 + 3) % N); mult[n] = (uint64_t)(n * 7919 + 1); }
    mkbfv::SlotMap ident(params, id), moved(params, perm, mult);
    const int flood = 60;
    std::vector<std::shared_ptr<mkrlwe::RefreshShare>> plain, mapped, permuted;
    std::vector<std::unique_ptr<mkrlwe::DeviceSampler>> sa, sb;
    for (size_t i = 0; i < names.size(); ++i) {
        sa.push_back(std::make_unique<mkrlwe::DeviceSampler>(key));
        sb.push_back(std::make_unique<mkrlwe::DeviceSampler>(key));
        plain.push_back(ref.ShareNew(*ct, *sks[i], *pks[i], flood, *sa[i]));
        mapped.push_back(ref.ShareMapNew(*ct, *sks[i], *pks[i], flood, *sb[i], ident));
        std::vector<uint64_t> x((size_t)nQ * N), y(x.size()), u((size_t)2 * nQ * N), v(u.size());
        plain[i]->Share.Value.download(x.data()); mapped[i]->Share.Value.download(y.data());
        plain[i]->Reenc[0]->download(u.data()); mapped[i]->Reenc[0]->download(v.data());
        if (x != y || u != v || sa[i]->Counter() != 2 || sb[i]->Counter() != 2) return fail("ShareMapNew with the identity map is ShareNew, bit for bit");
        permuted.push_back(ref.ShareMapNew(*ct, *sks[i], *pks[i], flood, *sb[i], moved));
    }
    auto want = ref.MergeNew(*ct, {plain[0].get(), plain[1].get(), plain[2].get()});
    auto same = ref.MergeMapNew(*ct, {mapped[2].get(), mapped[0].get(), mapped[1].get()}, ident);
    std::vector<uint64_t> x(want->words()), y(same->words());
    want->download(x.data()); same->download(y.data());
    if (x != y) return fail("MergeMapNew with the identity map is MergeNew, bit for bit");
    auto res = ref.MergeMapNew(*ct, {permuted[0].get(), permuted[1].get(), permuted[2].get()}, moved);
    decode(*res);
    if (got != moved.Apply(msg.data())) return fail("the permuted refresh decrypts to SlotMap::Apply of the message");
    if (mkbfv::SlotMap::Rotation(params, 5, true)->index[0] != (uint32_t)(N / 2 + 5)) return fail("Rotation(5, swapRows)");

    // E2S / S2E: public + the secret shares = the message slot by slot; fresh encryptions of the shares decrypt to it again
    mkbfv::ShareConverter conv(params);
    std::vector<std::shared_ptr<mkrlwe::DecryptionShare>> pubs;
    std::vector<std::shared_ptr<mkbfv::SecretShare>> secs;
    for (size_t i = 0; i < names.size(); ++i) { auto p = conv.E2SShareBatch({ct.get()}, *sks[i], flood, *sb[i]); pubs.push_back(p.first); secs.push_back(p.second); }
    auto pub = conv.E2SMergeBatch({ct.get()}, {pubs[1].get(), pubs[2].get(), pubs[0].get()});
    std::vector<int64_t> sum(N), part(N);
    pub->Slots(sum.data());
    for (auto& s : secs) { s->Slots(part.data()); for (int n = 0; n < N; ++n) sum[n] += part[n]; }
    for (auto& v : sum) { v = ((v % T) + T) % T; if (v > T / 2) v -= T; }
    if (sum != msg) return fail("public + secret shares = the message, slot by slot");
    std::vector<std::shared_ptr<mkbfv::Ciphertext>> back;
    for (size_t i = 0; i < names.size(); ++i) back.push_back(conv.S2EShareBatch(*secs[i], *pks[i], *sb[i])[0]);
    auto again = conv.S2EMergeNew({back[0].get(), back[1].get(), back[2].get()}, pub.get());
    decode(*again);
    if (got != msg) return fail("S2E decrypts to the message");
    auto round = mkbfv::SecretShare::FromSlots(params, 1, msg.data());
    round->Slots(got.data());
    secs[0]->Wipe();
    return got == msg && !secs[0]->Value.d ? true : fail("FromSlots / Slots / Wipe");
}

static bool ckks_part() {
    std::vector<uint64_t> Q{0x3fffffffd60001ULL, 0x3fffffff6d0001ULL, 0x3fffffff550001ULL}, P{0xffffffffffc0001ULL, 0xfffffffff840001ULL};
    const double scale = 1099511627776.0;                                  // 2^40
    mkckks::Parameters params(10, Q, P, scale);
    params.AddCRS(0, (uint64_t)1);
    const int N = params.N();
    const std::vector<std::string> names{"a", "b", "c"};
    mkrlwe::KeyGenerator kgen(params);
    std::vector<std::unique_ptr<mkrlwe::SecretKey>> sks;
    mkrlwe::SecretKeySet skSet;
    const uint32_t key[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    for (size_t i = 0; i < names.size(); ++i) { sks.push_back(kgen.GenSecretKey(names[i], ternary(N, 31 + i).data())); skSet.AddSecretKey(*sks[i]); }
    // any ciphertext will do: the identity holds for every c, whatever it decrypts to.  Level 1 of 2.
    mkckks::Ciphertext ct(params, mkrlwe::IDSet{"a", "b", "c"}, 1, scale);
    std::vector<uint64_t> host(ct.words());
    uint64_t seed = 5;
    for (size_t i = 0; i < host.size(); ++i) { seed = seed * 6364136223846793005ULL + 1442695040888963407ULL; host[i] = (seed >> 11) % Q[(i / N) % 2]; }
    ct.upload(host.data());
    mkckks::ShareConverter conv(params, scale);
    std::vector<std::shared_ptr<mkrlwe::DecryptionShare>> pubs;
    std::vector<std::shared_ptr<mkrlwe::SecretShare>> secs;
    for (size_t i = 0; i < names.size(); ++i) {
        mkrlwe::DeviceSampler s(key);
        auto p = conv.E2SShareBatch({&ct}, *sks[i], 100, s);
        if (s.Counter() != 1 || p.second->Level != params.MaxLevel()) return fail("E2SShareBatch takes one nonce and shares at the maximum level");
        pubs.push_back(p.first); secs.push_back(p.second);
    }
    auto pub = conv.E2SMergeBatch({&ct}, {pubs[2].get(), pubs[0].get(), pubs[1].get()});
    const size_t L = (size_t)params.MaxLevel() + 1;
    std::vector<uint64_t> total(L * N), part(L * N), plain((size_t)2 * N);
    pub->Value.download(total.data());
    for (auto& s : secs) { s->Value.download(part.data()); for (size_t j = 0; j < 2; ++j) for (int n = 0; n < N; ++n) total[j * N + n] = (total[j * N + n] + part[j * N + n]) % Q[j]; }
    mkrlwe::DeviceWords pt(params, (size_t)2 * N);
    mkrlwe::Decryptor(params).Decrypt(ct, skSet, pt.d);
    pt.download(plain.data());
    for (size_t i = 0; i < plain.size(); ++i) if (plain[i] != total[i]) return fail("R~ + sum of the secret shares == mkhe_decrypt under the input moduli");
    auto folded = conv.FoldPublic(*secs[1], *pub);
    return folded->Count == 1 && folded->ID == "b" ? true : fail("FoldPublic");
}

int main(int argc, char**) {
    if (argc < 2) {
        std::printf("%p %p %p %p %p\n", (void*)&mkhe_e2s_share, (void*)&mkhe_e2s_merge, (void*)&mkhe_bfv_e2s_share, (void*)&mkhe_bfv_slot_map_prepare, (void*)&mkhe_bfv_slot_map);
        std::printf("e2s mirror links\n");
        return 0;                                                       // nothing below runs without a GPU
    }
    try {
        if (!bfv_part() || !ckks_part()) return 1;
    } catch (const std::exception& e) {
        std::printf("FAILED: %s\n", e.what());
        return 1;
    }
    std::printf("e2s mirror runs\n");
    return 0;
}
