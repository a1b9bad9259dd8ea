// Uses mkrlwe::small_cdt, DeviceSampler and the seeded overloads of mkrlwe::Encryptor of include/mkhe.hpp, and both C entry points of the device
// sampler (compile-and-link check: tests/test_cpp_device_sampler.py).  Without an argument it prints small_cdt(3.2), which needs no GPU.
#include "mkhe.hpp"
#include <cstdio>

int main(int argc, char**) {
    const std::vector<uint64_t> cdt = mkrlwe::small_cdt(3.2);
    if (argc < 2) {
        for (uint64_t t : cdt) std::printf("%llu\n", (unsigned long long)t);
        bool refused = false;
        try { mkrlwe::small_cdt(6.0); } catch (const mkhe::Error&) { refused = true; }
        std::printf("device sampler mirror links%s\n", refused && mkrlwe::small_cdt(3.2, 4).size() == 8 ? "" : " (small_cdt arguments!)");
        return 0;                                                       // nothing below runs without a GPU
    }
    std::vector<uint64_t> Q{0xfffffffff6a0001ULL, 0x3fffffffd60001ULL}, P{0x7ffffffffe70001ULL, 0x7ffffffffe10001ULL};
    mkrlwe::Parameters params(10, Q, P, 2, 0);
    params.AddCRS(0, (uint64_t)1);
    const int N = params.N();
    std::vector<int32_t> s(N, 1), e(N, 0);
    mkrlwe::KeyGenerator kgen(params);
    auto sk = kgen.GenSecretKey("a", s.data());
    auto pk = kgen.GenPublicKey(*sk, e.data());
    mkrlwe::DeviceWords pt(params, 2 * (size_t)Q.size() * N), smp(params, (size_t)N);
    const uint32_t key[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    mkrlwe::DeviceSampler sampler(key);
    mkrlwe::Encryptor enc(params);
    mkrlwe::Ciphertext ct(params, mkrlwe::IDSet{"a"}, 1, false);
    enc.Encrypt(pt.d, *pk, ct, sampler);
    auto cts = enc.EncryptBatch(1, 2, pt.d, *pk, sampler, true);
    mkhe::check(mkhe_sample_small(params.ctx, 1, 2, sampler.Key(), sampler.NextNonce(), 0, sampler.cdt.data(), (int)sampler.cdt.size(), smp.d));
    std::printf("%d %llu\n", (int)cts.size(), (unsigned long long)sampler.Counter());
    return 0;
}
