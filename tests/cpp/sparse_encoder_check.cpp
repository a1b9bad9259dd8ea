// Uses mkckks::Encoder of include/mkhe.hpp with a slot count below full packing (compile-and-link check: tests/test_cpp_sparse_encoder.py).
#include "mkhe.hpp"
#include <cstdio>

int main(int argc, char**) {
    if (argc < 2) { std::printf("sparse encoder mirror links\n"); return 0; }      // nothing below runs without a GPU
    std::vector<uint64_t> Q{0xfffffffff6a0001ULL, 0x3fffffffd60001ULL}, P{0x7ffffffffe70001ULL, 0x7ffffffffe10001ULL};
    mkckks::Parameters params(10, Q, P, 1099511627776.0, 0);
    mkckks::Encoder full(params), sparse(params, 4), one(params, 0);
    if (full.Slots() != 512 || full.LogSlots() != 9 || sparse.Slots() != 16 || one.Slots() != 1) return 1;
    const int count = 2;
    mkrlwe::DeviceWords pt(params, (size_t)count * Q.size() * params.N());
    for (mkckks::Encoder* enc : {&sparse, &one, &full}) {
        std::vector<std::complex<double>> z((size_t)count * enc->Slots(), std::complex<double>(0.5, -0.25)), back(z.size());
        enc->Encode(count, z.data(), (int)Q.size() - 1, params.Scale(), pt.d);
        enc->Decode((int)Q.size(), count, pt.d, params.Scale(), back.data());
        std::printf("%d slots: %g %g\n", enc->Slots(), back[0].real(), back[0].imag());
    }
    try { mkckks::Encoder bad(params, 10); return 1; } catch (const mkhe::Error&) {}
    return 0;
}
