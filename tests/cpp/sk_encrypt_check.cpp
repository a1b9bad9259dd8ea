// Uses mkrlwe::SecretKeyEncryptor and mkrlwe::SeededCiphertext of include/mkhe.hpp with their mkckks and mkbfv wrappers, and the four C entry points
// of secret-key encryption with a seeded c1 (compile-and-link check: tests/test_cpp_sk_encrypt.py).  Without an argument it makes no engine call,
// which needs no GPU.
#include "mkhe.hpp"
#include <cstdio>

int main(int argc, char**) {
    if (argc < 2) {
        std::printf("%p %p %p %p\n", (void*)&mkhe_sample_uniform, (void*)&mkhe_encrypt_sk, (void*)&mkhe_encrypt_sk_seeded, (void*)&mkhe_ct_expand_seeded);
        std::printf("%zu %zu\n", mkrlwe::SeededCiphertext::WireBytes(14, 1 << 15, false), mkrlwe::SeededCiphertext::WireBytes(14, 1 << 15, true));
        std::printf("sk encrypt mirror links\n");
        return 0;                                                       // nothing below runs without a GPU
    }
    std::vector<uint64_t> Q{0x3fffffffd60001ULL, 0x3fffffff6d0001ULL, 0x3fffffff550001ULL}, QMul{0x3fffffffca0001ULL, 0x3fffffff5d0001ULL, 0x3fffffff390001ULL};
    std::vector<uint64_t> P{0xffffffffffc0001ULL, 0xfffffffff840001ULL};
    const uint32_t key[8] = {1, 2, 3, 4, 5, 6, 7, 8}, seed[8] = {8, 7, 6, 5, 4, 3, 2, 1};
    {
        mkbfv::Parameters params(10, Q, QMul, P, 65537);
        const int N = params.N();
        std::vector<int32_t> s(N, 1), e(2 * (size_t)N, 0);
        mkrlwe::KeyGenerator kgen(params);
        auto sk = kgen.GenSecretKey("a", s.data());
        mkrlwe::DeviceSampler smp(key);
        mkbfv::SecretKeyEncryptor enc(params, *sk, seed);
        mkrlwe::DeviceWords pt(params, (size_t)2 * 3 * N);
        auto cts = enc.EncryptPtxtBatch(2, pt.d, smp);
        auto sc = enc.EncryptPtxtSeeded(2, pt.d, smp);
        std::vector<uint64_t> wire(sc->words());
        sc->download(wire.data());
        mkbfv::SeededCiphertext moved(params, "a", 2);
        moved.upload(wire.data(), sc->Key, sc->Nonce);
        auto out = moved.ExpandBfv();
        mkrlwe::SecretKeyEncryptor plain(params, *sk, seed);
        mkrlwe::Ciphertext one(params, mkrlwe::IDSet{"a"}, params.MaxLevel(), false);
        plain.Encrypt(pt.d, one, e.data());
        plain.Encrypt(pt.d, one, smp);
        auto host = plain.EncryptSeededBatch(params.MaxLevel(), 2, pt.d, e.data());
        auto both = plain.EncryptBatch(params.MaxLevel(), 2, pt.d, smp);
        std::printf("%d %d %d %llu %llu\n", (int)cts.size(), (int)out.size(), (int)host->Expand().size() + (int)both.size(), (unsigned long long)enc.Counter(),
                    (unsigned long long)smp.Counter());
    }
    {
        mkckks::Parameters params(10, Q, P, 18014398509481984.0);
        const int N = params.N();
        std::vector<int32_t> s(N, 1);
        mkrlwe::KeyGenerator kgen(params);
        auto sk = kgen.GenSecretKey("a", s.data());
        mkrlwe::DeviceSampler smp(key);
        mkckks::SecretKeyEncryptor enc(params, *sk, seed);
        mkrlwe::DeviceWords pt(params, (size_t)2 * N);
        auto cts = enc.EncryptPtxtBatch(1, 1, pt.d, params.Scale(), smp);
        auto sc = enc.EncryptPtxtSeeded(1, 1, pt.d, params.Scale(), smp);
        std::vector<uint64_t> wire(sc->words());
        sc->download(wire.data());
        mkckks::SeededCiphertext moved(params, "a", 1, 1, sc->Scale);
        moved.upload(wire.data(), sc->Key, sc->Nonce);
        auto out = moved.ExpandCkks();
        std::printf("%d %g %d\n", out[0]->Level(), out[0]->Scale, cts[0]->Level());
    }
    return 0;
}
