// Uses every member of mkckks::Encoder of include/mkhe.hpp (compile-and-link check: tests/test_cpp_encoder.py).
#include "mkhe.hpp"
#include <cstdio>

int main(int argc, char**) {
    if (argc < 2) { std::printf("encoder mirror links\n"); return 0; }      // nothing below runs without a GPU
    std::vector<uint64_t> Q{0xfffffffff6a0001ULL, 0x3fffffffd60001ULL}, P{0x7ffffffffe70001ULL, 0x7ffffffffe10001ULL};
    mkckks::Parameters params(10, Q, P, 1099511627776.0, 0);
    mkckks::Encoder enc(params);
    const int n = enc.Slots(), count = 2;
    std::vector<std::complex<double>> z((size_t)count * n, std::complex<double>(0.5, -0.25)), back(z.size());
    mkrlwe::DeviceWords pt(params, (size_t)count * Q.size() * params.N());
    enc.Encode(count, z.data(), (int)Q.size() - 1, params.Scale(), pt.d);
    enc.Decode((int)Q.size(), count, pt.d, params.Scale(), back.data());
    std::printf("%g %g\n", back[0].real(), back[0].imag());
    return 0;
}
