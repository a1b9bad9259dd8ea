// Uses mkrlwe::SecretKeyShare, mkrlwe::Thresholdizer, mkrlwe::Combiner and Decryptor::FoldShares of include/mkhe.hpp (through mkrlwe, mkckks and mkbfv
// Decryptors) and the three C entry points of the threshold secret keys (compile-and-link check: tests/test_cpp_threshold.py).  Without an argument
// it makes no engine call, which needs no GPU.
#include "mkhe.hpp"
#include <cstdio>

int main(int argc, char**) {
    if (argc < 2) {
        std::printf("%p %p %p\n", (void*)&mkhe_threshold_gen_shares, (void*)&mkhe_threshold_additive_key, (void*)&mkhe_limbs_sum);
        std::printf("%.1f\n", (double)mkrlwe::Decryptor::FloodBound(2 - 1 + 2, 10));      // one of two parties covered by t = 2 holders: three floods
        std::printf("threshold mirror links\n");
        return 0;                                                       // nothing below runs without a GPU
    }
    std::vector<uint64_t> Q{0x3fffffffd60001ULL, 0x3fffffff6d0001ULL, 0x3fffffff550001ULL}, QMul{0x3fffffffca0001ULL, 0x3fffffff5d0001ULL, 0x3fffffff390001ULL};
    std::vector<uint64_t> P{0xffffffffffc0001ULL, 0xfffffffff840001ULL};
    const uint32_t key[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    const std::map<std::string, uint32_t> points{{"bob", 1}, {"carol", 7}, {"dave", 4294967295u}};
    {
        mkbfv::Parameters params(10, Q, QMul, P, 65537);
        params.AddCRS(0, (uint64_t)1);
        const int N = params.N();
        std::vector<int32_t> s(N, 1);
        mkrlwe::KeyGenerator kgen(params);
        auto ska = kgen.GenSecretKey("alice", s.data());
        auto skb = kgen.GenSecretKey("bob", s.data());
        mkrlwe::DeviceSampler sa(key);
        mkrlwe::Thresholdizer th(params);
        mkrlwe::Combiner cb(params);
        auto shares = th.GenShares(*ska, 2, points, sa);
        const mkrlwe::SecretKeyShare& carol = *shares.at("carol");
        std::vector<uint64_t> wire(carol.Value.words);
        carol.Value.download(wire.data());
        mkrlwe::SecretKeyShare moved(params, carol.ID, carol.Holder, carol.Point, carol.Threshold);
        moved.Value.upload(wire.data());
        const std::vector<uint32_t> active{7, 4294967295u};
        auto addc = cb.AdditiveKey(moved, active), addd = cb.AdditiveKey(*shares.at("dave"), active);
        auto back = cb.Reconstruct({addc.get(), addd.get()});
        mkbfv::Ciphertext ct(params, mkrlwe::IDSet{"alice", "bob"});
        mkbfv::Decryptor dec(params);
        auto hc = dec.ShareNew(ct, *addc, 40, &sa), hd = dec.ShareNew(ct, *addd, 40, &sa), hb = dec.ShareNew(ct, *skb, 40, &sa);
        auto ha = dec.FoldShares({hc.get(), hd.get()});
        mkrlwe::DeviceWords pt(params, (size_t)3 * N);
        dec.MergeShares(ct, {ha.get(), hb.get()}, pt.d);
        std::printf("%s %s %u %d %s %d %llu\n", moved.ID.c_str(), moved.Holder.c_str(), moved.Point, moved.Threshold, back->ID.c_str(), ha->Level,
                    (unsigned long long)sa.Counter());
    }
    {
        mkckks::Parameters params(10, Q, P, 18014398509481984.0);
        params.AddCRS(0, (uint64_t)1);
        std::vector<int32_t> s(params.N(), 1);
        mkrlwe::KeyGenerator kgen(params);
        auto ska = kgen.GenSecretKey("alice", s.data());
        mkrlwe::DeviceSampler sa(key);
        auto shares = mkrlwe::Thresholdizer(params).GenShares(*ska, 3, points, sa);
        auto add = mkrlwe::Combiner(params).AdditiveKey(*shares.at("bob"), {1, 7, 4294967295u});
        mkckks::Ciphertext ct(params, mkrlwe::IDSet{"alice"}, 1, params.Scale());
        mkckks::Decryptor dec(params);
        auto h = dec.ShareNew(ct, *add, 30, &sa);
        auto folded = dec.FoldShares({h.get()});
        mkrlwe::Decryptor plain(params);
        auto again = plain.FoldShares({folded.get(), h.get()});
        std::printf("%d %d %s\n", folded->Level, again->Count, add->ID.c_str());
    }
    return 0;
}
