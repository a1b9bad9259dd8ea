// Uses mkbfv::Refresher of include/mkhe.hpp with mkrlwe::RefreshShare, and both C entry points of the collective refresh of MK-BFV
// (compile-and-link check: tests/test_cpp_bfv_refresh.py).  Without an argument it makes no engine call, which needs no GPU.
#include "mkhe.hpp"
#include <cstdio>

int main(int argc, char**) {
    if (argc < 2) {
        std::printf("%p %p\n", (void*)&mkhe_bfv_refresh_share, (void*)&mkhe_bfv_refresh_merge);
        std::printf("bfv refresh mirror links\n");
        return 0;                                                       // nothing below runs without a GPU
    }
    std::vector<uint64_t> Q{0x3fffffffd60001ULL, 0x3fffffff6d0001ULL, 0x3fffffff550001ULL}, QMul{0x3fffffffca0001ULL, 0x3fffffff5d0001ULL, 0x3fffffff390001ULL};
    std::vector<uint64_t> P{0xffffffffffc0001ULL, 0xfffffffff840001ULL};
    mkbfv::Parameters params(10, Q, QMul, P, 65537);
    params.AddCRS(0, (uint64_t)1);
    const int N = params.N();
    std::vector<int32_t> s(N, 1), e(N, 0);
    mkrlwe::KeyGenerator kgen(params);
    auto ska = kgen.GenSecretKey("a", s.data());
    auto skb = kgen.GenSecretKey("b", s.data());
    auto pka = kgen.GenPublicKey(*ska, e.data());
    auto pkb = kgen.GenPublicKey(*skb, e.data());
    const uint32_t key[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    mkrlwe::DeviceSampler sa(key), sb(key);
    mkbfv::Refresher ref(params);
    mkbfv::Ciphertext ct(params, mkrlwe::IDSet{"a", "b"}), ct2(params, mkrlwe::IDSet{"a", "b"});
    auto ra = ref.ShareNew(ct, *ska, *pka, 100, sa);
    auto rb = ref.ShareNew(ct, *skb, *pkb, 100, sb);
    auto batch_a = ref.ShareBatch({&ct, &ct2}, *ska, *pka, 40, sa), batch_b = ref.ShareBatch({&ct, &ct2}, *skb, *pkb, 40, sb);
    std::vector<uint64_t> wire((size_t)3 * N);
    rb->Share.Value.download(wire.data());
    mkrlwe::RefreshShare moved(params, "b", params.MaxLevel(), params.MaxLevel());
    moved.Share.Value.upload(wire.data());
    auto out = ref.MergeNew(ct, {&moved, ra.get()});
    auto outs = ref.MergeBatch({&ct, &ct2}, {batch_b.get(), batch_a.get()});
    std::printf("%d %d %d %llu\n", out->Level(), (int)outs.size(), rb->LevelOut, (unsigned long long)sa.Counter());
    return 0;
}
