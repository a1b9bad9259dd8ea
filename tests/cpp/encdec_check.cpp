// Uses every member of mkrlwe::Encryptor / Decryptor / SecretKeySet of include/mkhe.hpp (compile-and-link check: tests/test_cpp_encdec.py).
#include "mkhe.hpp"
#include <cstdio>

int main(int argc, char**) {
    if (argc < 2) { std::printf("encdec mirror links\n"); return 0; }      // nothing below runs without a GPU
    std::vector<uint64_t> Q{0xfffffffff6a0001ULL, 0x3fffffffd60001ULL}, P{0x7ffffffffe70001ULL, 0x7ffffffffe10001ULL};
    mkrlwe::Parameters params(10, Q, P, 2, 0);
    params.AddCRS(0, (uint64_t)1);
    const int N = params.N();
    std::vector<int32_t> s(N, 1), e(N, 0), smp(2 * 3 * N, 0);
    mkrlwe::KeyGenerator kgen(params);
    auto sk = kgen.GenSecretKey("a", s.data());
    auto pk = kgen.GenPublicKey(*sk, e.data());
    mkrlwe::DeviceWords pt(params, 2 * (size_t)Q.size() * N), res(params, (size_t)Q.size() * N);
    mkrlwe::Encryptor enc(params);
    mkrlwe::Decryptor dec(params);
    mkrlwe::Ciphertext ct(params, mkrlwe::IDSet{"a"}, 1, false);
    enc.Encrypt(pt.d, *pk, ct, smp.data());
    auto cts = enc.EncryptBatch(1, 2, pt.d, *pk, smp.data(), true);
    mkrlwe::SecretKeySet skSet;
    skSet.AddSecretKey(*sk);
    dec.Decrypt(*cts[1], skSet, res.d);
    auto part = dec.PartialDecrypt(ct, skSet.GetSecretKey("a"));
    skSet.DelSecretKey("a");
    std::printf("%d\n", (int)part->ids.size());
    return 0;
}
