// Uses every member of mkbfv::Encoder of include/mkhe.hpp (compile-and-link check: tests/test_cpp_bfv_encoder.py).
#include "mkhe.hpp"
#include <cstdio>

int main(int argc, char**) {
    if (argc < 2) { std::printf("bfv encoder mirror links\n"); return 0; }      // nothing below runs without a GPU
    std::vector<uint64_t> Q{0x3fffffffd60001ULL, 0x3fffffff6d0001ULL}, QMul{0x3fffffffca0001ULL, 0x3fffffff5d0001ULL};
    std::vector<uint64_t> P{0xffffffffffc0001ULL, 0xfffffffff840001ULL};
    mkbfv::Parameters params(10, Q, QMul, P, 65537, 0);
    mkbfv::Encoder enc(params);
    const int n = enc.Slots(), count = 2;
    std::vector<int64_t> v((size_t)count * n, -7), back(v.size());
    mkrlwe::DeviceWords pt(params, (size_t)count * Q.size() * params.N());
    enc.Encode(count, v.data(), pt.d);
    enc.Decode(count, pt.d, back.data());
    std::printf("%lld psi %llu\n", (long long)back[0], (unsigned long long)enc.SlotPsi());
    return 0;
}
