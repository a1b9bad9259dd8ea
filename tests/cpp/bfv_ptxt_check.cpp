// Uses mkbfv::Encoder::EncodeMul and mkbfv::Evaluator::MulPtxtNew / AddPtxtNew / SubPtxtNew of include/mkhe.hpp (compile-and-link check:
// tests/test_cpp_bfv_ptxt.py).
#include "mkhe.hpp"
#include <cstdio>

int main(int argc, char**) {
    if (argc < 2) { std::printf("bfv ptxt mirror links\n"); return 0; }      // nothing below runs without a GPU
    std::vector<uint64_t> Q{0x3fffffffd60001ULL, 0x3fffffff6d0001ULL}, QMul{0x3fffffffca0001ULL, 0x3fffffff5d0001ULL};
    std::vector<uint64_t> P{0xffffffffffc0001ULL, 0xfffffffff840001ULL};
    mkbfv::Parameters params(10, Q, QMul, P, 65537, 0);
    mkbfv::Encoder enc(params);
    mkbfv::Evaluator ev(params);
    const int n = enc.Slots();
    std::vector<int64_t> v((size_t)n, -7);
    const size_t words = Q.size() * (size_t)params.N();
    mkrlwe::DeviceWords pt(params, words), ptmul(params, words);
    enc.Encode(1, v.data(), pt.d);
    enc.EncodeMul(1, v.data(), ptmul.d);
    mkbfv::Ciphertext ct(params, mkrlwe::IDSet{"user0", "user1"});
    auto prod = ev.MulPtxtNew(ct, ptmul.d);
    auto sum = ev.AddPtxtNew(*prod, pt.d);
    auto diff = ev.SubPtxtNew(*sum, pt.d);
    std::printf("%d parties\n", mkhe_ct_nparties(diff->h));
    return 0;
}
