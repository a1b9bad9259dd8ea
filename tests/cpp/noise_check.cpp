// Uses the noise measures of include/mkhe.hpp -- mkrlwe::Decryptor::NoiseNormBatch / NoiseNorm, mkckks::Decryptor::NoiseNorm / NoiseBits,
// mkbfv::Decryptor::InvariantNoise / NoiseBudget / NoiseNorm / NoiseBits, mkrlwe::NoiseValue -- and the C entry point mkhe_noise_norm
// (compile-and-link check: tests/test_cpp_noise.py).  Without an argument it makes no engine call, which needs no GPU: it checks the host
// arithmetic of NoiseValue and the refusal of a null context.
#include "mkhe.hpp"
#include <cstdio>
#include <cstring>

int main(int argc, char**) {
    std::vector<uint64_t> Q{0x3fffffffd60001ULL, 0x3fffffff6d0001ULL, 0x3fffffff550001ULL}, QMul{0x3fffffffca0001ULL, 0x3fffffff5d0001ULL, 0x3fffffff390001ULL};
    std::vector<uint64_t> P{0xffffffffffc0001ULL, 0xfffffffff840001ULL};
    if (argc < 2) {
        std::printf("%p\n", (void*)&mkhe_noise_norm);
        // (Q - 1) / 2 has the digits (q_i - 1) / 2 and bitlen(Q) - 1 bits; Q = 2 * that + 1
        const uint64_t half[3] = {(Q[0] - 1) / 2, (Q[1] - 1) / 2, (Q[2] - 1) / 2};
        mkrlwe::NoiseValue h = mkrlwe::NoiseValue::FromMixedRadix(half, Q.data(), 3, 5), q;
        q.Words.push_back(1);
        for (uint64_t m : Q) q.MulAdd(m, 0);
        mkrlwe::NoiseValue twice = h;
        twice.MulAdd(2, 1);
        if (twice.Words != q.Words || h.Bits() != q.Bits() - 1 || h.Index != 5 || q.Bits() != 162) { std::printf("NoiseValue: wrong product\n"); return 1; }
        mkrlwe::NoiseValue back = q;
        back.Div(Q[1]).Div(Q[0]).Div(Q[2]);
        if (back.Words != std::vector<uint64_t>{1} || mkrlwe::NoiseValue().Bits() != 0) { std::printf("NoiseValue: wrong quotient\n"); return 1; }
        const uint64_t small[3] = {41, 0, 0};
        const mkrlwe::NoiseValue s = mkrlwe::NoiseValue::FromMixedRadix(small, Q.data(), 3, 0);
        if (s.Words != std::vector<uint64_t>{41} || s.Bits() != 6 || s.Value() != 41.0L) { std::printf("NoiseValue: wrong small value\n"); return 1; }
        std::printf("%d %.0Lf\n", h.Bits(), h.Value() / 1e40L);
        alignas(16) uint64_t word[2] = {0, 0};
        if (mkhe_noise_norm(nullptr, 0, 1, 1, word, nullptr, 0, word) != 1 || std::strcmp(mkhe_last_error(), "mkhe_noise_norm: null context")) {
            std::printf("mkhe_noise_norm: a null context is not refused by name\n");
            return 1;
        }
        std::printf("noise mirror links\n");
        return 0;                                                       // nothing below runs without a GPU
    }
    const uint32_t key[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    {
        mkbfv::Parameters params(10, Q, QMul, P, 65537);
        params.AddCRS(0, (uint64_t)1);
        const int N = params.N();
        std::vector<int32_t> s(N, 1), e(N, 0);
        mkrlwe::KeyGenerator kgen(params);
        auto sk = kgen.GenSecretKey("a", s.data());
        auto pk = kgen.GenPublicKey(*sk, e.data());
        mkrlwe::SecretKeySet skSet;
        skSet.AddSecretKey(*sk);
        mkrlwe::DeviceSampler smp(key);
        std::vector<int64_t> msg(N, 3);
        mkrlwe::DeviceWords pt(params, (size_t)3 * N);
        mkbfv::Encoder(params).Encode(1, msg.data(), pt.d);
        mkbfv::Ciphertext ct(params, mkrlwe::IDSet{"a"});
        mkrlwe::Encryptor(params).Encrypt(pt.d, *pk, ct, smp);
        mkbfv::Decryptor dec(params);
        const mkrlwe::NoiseValue r = dec.InvariantNoise(ct, skSet), exact = dec.NoiseNorm(ct, skSet, msg.data()), bound = dec.NoiseNorm(ct, skSet);
        std::printf("%d %d %d %d %d %ld %Lg\n", r.Bits(), dec.NoiseBudget(ct, skSet), exact.Bits(), bound.Bits(), dec.NoiseBits(ct, skSet), exact.Index, bound.Value());
        mkrlwe::DeviceWords phases(params, (size_t)2 * 3 * N);
        auto both = dec.NoiseNormBatch(3, 2, phases.d, pt.d, 0);
        std::printf("%d\n", (int)both.size());
    }
    {
        mkckks::Parameters params(10, Q, P, 18014398509481984.0);
        params.AddCRS(0, (uint64_t)1);
        const int N = params.N();
        std::vector<int32_t> s(N, 1), e(N, 0);
        mkrlwe::KeyGenerator kgen(params);
        auto sk = kgen.GenSecretKey("a", s.data());
        mkrlwe::SecretKeySet skSet;
        skSet.AddSecretKey(*sk);
        std::vector<std::complex<double>> msg(N / 2, {0.5, -0.25});
        mkckks::Ciphertext ct(params, mkrlwe::IDSet{"a"}, 1, params.Scale());
        mkckks::Decryptor dec(params);
        std::printf("%d %d\n", dec.NoiseBits(ct, skSet, msg.data()), dec.NoiseNorm(ct, skSet).Bits());
    }
    return 0;
}
