// Uses DecryptionShare and the share / merge methods of mkrlwe::Decryptor of include/mkhe.hpp, and both C entry points of distributed decryption
// (compile-and-link check: tests/test_cpp_decrypt_share.py).  Without an argument it makes no engine call, which needs no GPU.
#include "mkhe.hpp"
#include <cstdio>

int main(int argc, char**) {
    if (argc < 2) {
        std::printf("%p %p\n", (void*)&mkhe_decrypt_share, (void*)&mkhe_decrypt_merge);
        std::printf("decrypt share mirror links\n");
        return 0;                                                       // nothing below runs without a GPU
    }
    std::vector<uint64_t> Q{0xfffffffff6a0001ULL, 0x3fffffffd60001ULL}, P{0x7ffffffffe70001ULL, 0x7ffffffffe10001ULL};
    mkrlwe::Parameters params(10, Q, P, 2, 0);
    params.AddCRS(0, (uint64_t)1);
    const int N = params.N();
    std::vector<int32_t> s(N, 1);
    mkrlwe::KeyGenerator kgen(params);
    auto ska = kgen.GenSecretKey("a", s.data());
    auto skb = kgen.GenSecretKey("b", s.data());
    const uint32_t key[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    mkrlwe::DeviceSampler sampler(key);
    mkrlwe::Decryptor dec(params);
    mkrlwe::Ciphertext ct(params, mkrlwe::IDSet{"a", "b"}, 1), ct2(params, mkrlwe::IDSet{"a", "b"}, 1);
    auto sa = dec.ShareNew(ct, *ska, 40, &sampler);
    auto sb = dec.ShareNew(ct, *skb, 0, nullptr);
    auto batch_a = dec.ShareBatch({&ct, &ct2}, *ska, 40, &sampler), batch_b = dec.ShareBatch({&ct, &ct2}, *skb, 40, &sampler);
    std::vector<uint64_t> wire((size_t)2 * N);
    sb->Value.download(wire.data());
    mkrlwe::DecryptionShare moved(params, "b", 1);
    moved.Value.upload(wire.data());
    mkrlwe::DeviceWords pt(params, 2 * (size_t)Q.size() * N);
    dec.MergeShares(ct, {&moved, sa.get()}, pt.d);
    dec.MergeSharesBatch({&ct, &ct2}, {batch_a.get(), batch_b.get()}, pt.d);
    std::printf("%d %llu\n", batch_a->Count, (unsigned long long)sampler.Counter());
    return 0;
}
