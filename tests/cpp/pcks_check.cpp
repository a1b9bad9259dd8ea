// Uses mkrlwe::PublicKeySwitcher, mkckks::PublicKeySwitcher and mkbfv::PublicKeySwitcher of include/mkhe.hpp with mkrlwe::PublicKeySwitchShare, and both
// C entry points of the collective key switch to a recipient's public key (compile-and-link check: tests/test_cpp_pcks.py).  Without an argument
// it makes no engine call, which needs no GPU.
#include "mkhe.hpp"
#include <cstdio>

int main(int argc, char**) {
    if (argc < 2) {
        std::printf("%p %p\n", (void*)&mkhe_pcks_share, (void*)&mkhe_pcks_merge);
        std::printf("%.1Lf\n", mkrlwe::PublicKeySwitcher::NoiseBound(3, 10, 1024));
        std::printf("pcks mirror links\n");
        return 0;                                                       // nothing below runs without a GPU
    }
    std::vector<uint64_t> Q{0x3fffffffd60001ULL, 0x3fffffff6d0001ULL, 0x3fffffff550001ULL}, QMul{0x3fffffffca0001ULL, 0x3fffffff5d0001ULL, 0x3fffffff390001ULL};
    std::vector<uint64_t> P{0xffffffffffc0001ULL, 0xfffffffff840001ULL};
    const uint32_t key[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    {
        mkbfv::Parameters params(10, Q, QMul, P, 65537);
        params.AddCRS(0, (uint64_t)1);
        const int N = params.N();
        std::vector<int32_t> s(N, 1), e(N, 0);
        mkrlwe::KeyGenerator kgen(params);
        auto ska = kgen.GenSecretKey("a", s.data());
        auto skb = kgen.GenSecretKey("b", s.data());
        auto skc = kgen.GenSecretKey("carol", s.data());
        auto pkc = kgen.GenPublicKey(*skc, e.data());
        mkrlwe::DeviceSampler sa(key), sb(key);
        mkbfv::PublicKeySwitcher sw(params);
        mkbfv::Ciphertext ct(params, mkrlwe::IDSet{"a", "b"}), ct2(params, mkrlwe::IDSet{"a", "b"});
        auto ha = sw.ShareNew(ct, *ska, *pkc, 100, sa);
        auto hb = sw.ShareNew(ct, *skb, *pkc, 100, sb);
        auto batch_a = sw.ShareBatch({&ct, &ct2}, *ska, *pkc, 40, sa), batch_b = sw.ShareBatch({&ct, &ct2}, *skb, *pkc, 40, sb);
        std::vector<uint64_t> wire((size_t)2 * 3 * N);
        hb->Value.download(wire.data());
        mkrlwe::PublicKeySwitchShare moved(params, "b", params.MaxLevel());
        moved.Value.upload(wire.data());
        auto out = sw.MergeNew(ct, {&moved, ha.get()}, "carol");
        auto outs = sw.MergeBatch({&ct, &ct2}, {batch_b.get(), batch_a.get()}, "carol");
        std::printf("%d %d %d %llu\n", out->Level(), (int)outs.size(), (int)out->ids.size(), (unsigned long long)sa.Counter());
    }
    {
        mkckks::Parameters params(10, Q, P, 18014398509481984.0);
        params.AddCRS(0, (uint64_t)1);
        const int N = params.N();
        std::vector<int32_t> s(N, 1), e(N, 0);
        mkrlwe::KeyGenerator kgen(params);
        auto ska = kgen.GenSecretKey("a", s.data());
        auto skc = kgen.GenSecretKey("carol", s.data());
        auto pkc = kgen.GenPublicKey(*skc, e.data());
        mkrlwe::DeviceSampler sa(key);
        mkckks::PublicKeySwitcher sw(params);
        mkckks::Ciphertext ct(params, mkrlwe::IDSet{"a"}, 1, params.Scale());
        auto ha = sw.ShareNew(ct, *ska, *pkc, 30, sa);
        auto out = sw.MergeNew(ct, {ha.get()}, "carol");
        mkrlwe::PublicKeySwitcher plain(params);
        auto out2 = plain.MergeNew(ct, {ha.get()}, "carol");
        std::printf("%d %g %d %Lg\n", out->Level(), out->Scale, out2->Level(), sw.SwitchSlotBound(1, 30, out->Scale));
    }
    return 0;
}
