// Uses mkckks::Evaluator::MulRelinSum of include/mkhe.hpp (compile-and-link check without an argument; with one, on a GPU: the wrapper against the C
// call mkhe_mul_relin_sum on the same seeded uniform inputs, with and without caller-supplied hoisted forms and the rescale: tests/test_cpp_mulrelin_sum.py).
#include "mkhe.hpp"
#include <cstdio>

typedef std::vector<uint64_t> vec;
static uint64_t rng_state = 0x53554D4Dull;
static uint64_t next64() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static void fill_poly(uint64_t* p, const vec& mods, size_t N) { for (size_t l = 0; l < mods.size(); ++l) for (size_t i = 0; i < N; ++i) p[l * N + i] = next64() % mods[l]; }
static vec rand_swk(const vec& Q, const vec& P, size_t N) {
    vec QP(Q); QP.insert(QP.end(), P.begin(), P.end());
    vec s(Q.size() * QP.size() * N);                      // alpha = 1: beta = nQ digits
    for (size_t i = 0; i < Q.size(); ++i) fill_poly(&s[i * QP.size() * N], QP, N);
    return s;
}
static vec rand_ct(const vec& Q, int n, size_t N) { vec c((1 + n) * Q.size() * N); for (int s = 0; s <= n; ++s) fill_poly(&c[s * Q.size() * N], Q, N); return c; }
static int fails = 0;
static void expect(bool ok, const char* what) { std::printf("%-64s %s\n", what, ok ? "ok" : "MISMATCH"); if (!ok) ++fails; }

int main(int argc, char**) {
    if (argc < 2) { std::printf("mulrelin sum mirror links\n"); return 0; }      // nothing below runs without a GPU
    const vec Q = {0xfffffffff6a0001ull, 0x3fffffffd60001ull, 0x3fffffffca0001ull, 0x3fffffff6d0001ull};
    const vec P = {0x7ffffffffe70001ull, 0x7ffffffffe10001ull};
    const int logN = 10, K = 3, level = (int)Q.size() - 1;
    const size_t N = 1u << logN;
    const double scale = 18014398509481984.0;   // 2^54
    mkckks::Parameters params(logN, Q, P, scale);
    mkckks::Evaluator eval(params);
    vec u = rand_swk(Q, P, N);
    params.AddCRS(-1, u.data());
    const std::vector<std::string> names = {"alice", "bob", "carol"};
    mkrlwe::RelinearizationKeySet rlkSet;
    for (auto& n : names) {
        vec b = rand_swk(Q, P, N), d = rand_swk(Q, P, N), v = rand_swk(Q, P, N);
        rlkSet.AddRelinearizationKey(std::make_shared<mkrlwe::RelinearizationKey>(params, n, b.data(), d.data(), v.data()));
    }
    const mkrlwe::IDSet ids0{"alice", "bob"}, ids1{"bob", "carol"}, ido{"alice", "bob", "carol"};
    std::vector<std::unique_ptr<mkckks::Ciphertext>> c0, c1;
    std::vector<std::unique_ptr<mkrlwe::HoistedCiphertext>> f0, f1;
    std::vector<const mkckks::Ciphertext*> ops0, ops1;
    std::vector<const mkrlwe::HoistedCiphertext*> hs0, hs1;
    for (int k = 0; k < K; ++k) {
        c0.push_back(std::make_unique<mkckks::Ciphertext>(params, ids0, level, scale)); c0.back()->upload(rand_ct(Q, 2, N).data());
        c1.push_back(std::make_unique<mkckks::Ciphertext>(params, ids1, level, scale)); c1.back()->upload(rand_ct(Q, 2, N).data());
        f0.push_back(eval.HoistedForm(*c0.back())); f1.push_back(eval.HoistedForm(*c1.back()));
        ops0.push_back(c0.back().get()); ops1.push_back(c1.back().get()); hs0.push_back(f0.back().get()); hs1.push_back(f1.back().get());
    }
    // the C call, no hoisted forms
    std::vector<const mkhe_ct*> a, b;
    std::vector<const mkhe_swk*> d0, v0, b1;
    for (auto* c : ops0) a.push_back(c->h);
    for (auto* c : ops1) b.push_back(c->h);
    for (auto& i : ops0[0]->ids) { auto& k = rlkSet.GetRelinearizationKey(i); d0.push_back(k.Value[1]->h); v0.push_back(k.Value[2]->h); }
    for (auto& i : ops1[0]->ids) b1.push_back(rlkSet.GetRelinearizationKey(i).Value[0]->h);
    for (int rescale = 0; rescale < 2; ++rescale) {
        mkckks::Ciphertext want(params, ido, level - rescale, scale * scale), got(params, ido, level - rescale, scale * scale), got_h(params, ido, level - rescale, scale * scale);
        mkhe::check(mkhe_mul_relin_sum(params.ctx, K, a.data(), b.data(), nullptr, nullptr, b1.data(), d0.data(), v0.data(), params.CRS[-1]->h, rescale, want.h));
        eval.MulRelinSum(ops0, ops1, {}, {}, rlkSet, rescale != 0, got);
        eval.MulRelinSum(ops0, ops1, hs0, hs1, rlkSet, rescale != 0, got_h);
        vec w(want.words()), g(got.words()), gh(got_h.words());
        want.download(w.data()); got.download(g.data()); got_h.download(gh.data());
        expect(g == w, rescale ? "mkckks::Evaluator::MulRelinSum, rescaled" : "mkckks::Evaluator::MulRelinSum");
        expect(gh == w, rescale ? "... with hoisted forms, rescaled" : "... with hoisted forms");
    }
    bool threw = false;
    try { mkckks::Ciphertext out(params, ido, level, scale); eval.MulRelinSum(ops0, {}, {}, {}, rlkSet, false, out); } catch (const mkhe::Error&) { threw = true; }
    expect(threw, "MulRelinSum refuses lists of different lengths");
    std::printf("%s\n", fails ? "FAILED" : "mulrelin sum mirror ok");
    return fails ? 1 : 0;
}
