// Uses mkbfv::LinearTransform and mkbfv::Evaluator::HoistedForm / RotateHoistedNew / LinearTransformNew of include/mkhe.hpp.  Without an argument:
// compile-and-link check only (tests/test_cpp_bfv_lintrans.py).  With one, on a GPU: RotateHoistedNew against RotateNew, and LinearTransformNew
// against the same schedule through RotateNew, MulPtxtNew (a plaintext addressed inside the block), AddNew and ConjugateNew, bit for bit.
#include "mkhe.hpp"
#include <cstdio>

static uint64_t next(uint64_t& s) { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return s >> 11; }

static std::vector<uint64_t> words(const mkbfv::Ciphertext& ct) {
    std::vector<uint64_t> w(ct.words());
    ct.download(w.data());
    return w;
}

int main(int argc, char**) {
    if (argc < 2) { std::printf("bfv lintrans mirror links\n"); return 0; }      // nothing below runs without a GPU
    std::vector<uint64_t> Q{0x3fffffffd60001ULL, 0x3fffffff6d0001ULL}, QMul{0x3fffffffca0001ULL, 0x3fffffff5d0001ULL};
    std::vector<uint64_t> P{0xffffffffffc0001ULL, 0xfffffffff840001ULL};
    mkbfv::Parameters params(10, Q, QMul, P, 65537, 0);
    mkbfv::Evaluator ev(params);
    const int N = params.N(), n = N / 2;
    uint64_t seed = 2026;
    mkbfv::LinearTransform::Diagonals diagonals, swapped;
    for (int k : {0, 1, 5, 17}) { auto& d = diagonals[k]; for (int j = 0; j < 2 * n; ++j) d.push_back((int64_t)(next(seed) % 65537) - 32768); }
    { auto& e = swapped[3]; for (int j = 0; j < 2 * n; ++j) e.push_back((int64_t)(next(seed) % 65537) - 32768); }
    mkbfv::LinearTransform lt(params, diagonals, swapped, 8);
    std::printf("n1 %d, %d plaintexts, %d rotations, conjugation %d\n", lt.n1, lt.nnz, (int)lt.Rotations().size(), (int)lt.NeedsConjugation());
    if (lt.n1 != 8 || lt.nnz != 5 || !lt.NeedsConjugation() || lt.masks.size() != lt.giantsD.size() + lt.giantsE.size()) return 1;

    // keys: ternary secrets, zero errors (the check is an equality of ciphertext bits, not a decryption)
    mkrlwe::KeyGenerator kgen(params);
    mkrlwe::RotationKeySet rks;
    mkrlwe::ConjugationKeySet cks;
    params.AddCRS(-2, (uint64_t)7);
    for (int r : lt.Rotations()) params.AddCRS(r, (uint64_t)(100 + r));
    const std::vector<int32_t> zero((size_t)params.Beta(params.MaxLevel()) * N, 0);
    const std::vector<std::string> names{"user0", "user1"};
    for (auto& id : names) {
        std::vector<int32_t> s((size_t)N);
        for (auto& v : s) v = (int32_t)(next(seed) % 3) - 1;
        auto sk = kgen.GenSecretKey(id, s.data());
        for (int r : lt.Rotations()) rks.AddRotationKey(kgen.GenRotationKey(r, *sk, zero.data()));
        cks.AddConjugationKey(kgen.GenConjugationKey(*sk, zero.data()));
    }
    mkbfv::Ciphertext ct(params, mkrlwe::IDSet{"user0", "user1"});
    {
        std::vector<uint64_t> host(ct.words());
        for (size_t i = 0; i < host.size(); ++i) host[i] = next(seed) % Q[(i / N) % Q.size()];
        ct.upload(host.data());
    }

    auto hoisted = ev.HoistedForm(ct);
    for (int r : lt.Rotations())
        if (words(*ev.RotateHoistedNew(ct, r, *hoisted, rks)) != words(*ev.RotateNew(ct, r, rks))) { std::printf("RotateHoistedNew(%d) differs\n", r); return 1; }

    auto fused = ev.LinearTransformNew(ct, lt, rks, &cks);
    // the same schedule, one call per step
    std::map<int, mkbfv::CiphertextPtr> rot;
    for (int b : lt.babies) if (b) rot[b] = ev.RotateNew(ct, b, rks);
    std::vector<int> giants(lt.giantsD);
    giants.insert(giants.end(), lt.giantsE.begin(), lt.giantsE.end());
    const size_t ptWords = Q.size() * (size_t)N;
    mkbfv::CiphertextPtr part[2];
    size_t index = 0;
    for (size_t g = 0; g < giants.size(); ++g) {
        mkbfv::CiphertextPtr inner;
        for (size_t i = 0; i < lt.babies.size(); ++i) {
            if (!((lt.masks[g] >> i) & 1)) continue;
            const mkbfv::Ciphertext& src = lt.babies[i] ? *rot[lt.babies[i]] : ct;
            auto prod = ev.MulPtxtNew(src, static_cast<const uint64_t*>(lt.pt->d) + ptWords * index++);
            inner = inner ? ev.AddNew(*inner, *prod) : std::move(prod);
        }
        if (giants[g]) inner = ev.RotateNew(*inner, giants[g], rks);
        auto& acc = part[g < lt.giantsD.size() ? 0 : 1];
        acc = acc ? ev.AddNew(*acc, *inner) : std::move(inner);
    }
    auto chain = ev.AddNew(*part[0], *ev.ConjugateNew(*part[1], cks));
    if ((int)index != lt.nnz || words(*fused) != words(*chain)) { std::printf("LinearTransformNew differs from the chain\n"); return 1; }

    // a missing conjugation key set is refused before any engine call
    try { ev.LinearTransformNew(ct, lt, rks); std::printf("missing ckSet accepted\n"); return 1; }
    catch (const mkhe::Error&) {}
    std::printf("%d parties\nbfv lintrans mirror ok\n", mkhe_ct_nparties(fused->h));
    return 0;
}
