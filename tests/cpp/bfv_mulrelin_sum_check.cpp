// Uses mkbfv::Evaluator::MulRelinSum / MulRelinSumNew of include/mkhe.hpp (compile-and-link check without an argument; with one, on a GPU: the wrapper
// against the C call mkhe_bfv_mul_relin_sum on the same seeded uniform inputs: tests/test_cpp_bfv_mulrelin_sum.py).
#include "mkhe.hpp"
#include <cstdio>

typedef std::vector<uint64_t> vec;
static uint64_t rng_state = 0x42465653ull;
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
    if (argc < 2) { std::printf("bfv mulrelin sum mirror links\n"); return 0; }      // nothing below runs without a GPU
    const vec Q = {0x3fffffffd60001ull, 0x3fffffff6d0001ull, 0x3fffffff550001ull};
    const vec QMul = {0x3fffffffca0001ull, 0x3fffffff5d0001ull, 0x3fffffff390001ull};
    const vec P = {0xffffffffffc0001ull, 0xfffffffff840001ull};
    const int logN = 10, K = 3;
    const size_t N = 1u << logN;
    mkbfv::Parameters params(logN, Q, QMul, P, 65537);
    mkbfv::Evaluator eval(params);
    vec u = rand_swk(Q, P, N);
    params.AddCRS(-1, u.data());
    const std::vector<std::string> names = {"alice", "bob", "carol"};
    mkbfv::RelinearizationKeySet rlkSet;
    for (auto& n : names) {
        vec b1 = rand_swk(Q, P, N), b2 = rand_swk(Q, P, N), d1 = rand_swk(Q, P, N), d2 = rand_swk(Q, P, N), v = rand_swk(Q, P, N);
        rlkSet.AddRelinearizationKey(std::make_shared<mkbfv::RelinearizationKey>(params, n, b1.data(), b2.data(), d1.data(), d2.data(), v.data()));
    }
    const mkrlwe::IDSet ids0{"alice", "bob"}, ids1{"bob", "carol"}, ido{"alice", "bob", "carol"};
    std::vector<std::unique_ptr<mkbfv::Ciphertext>> c0, c1;
    std::vector<const mkbfv::Ciphertext*> ops0, ops1;
    for (int k = 0; k < K; ++k) {
        c0.push_back(std::make_unique<mkbfv::Ciphertext>(params, ids0)); c0.back()->upload(rand_ct(Q, 2, N).data());
        c1.push_back(std::make_unique<mkbfv::Ciphertext>(params, ids1)); c1.back()->upload(rand_ct(Q, 2, N).data());
        ops0.push_back(c0.back().get()); ops1.push_back(c1.back().get());
    }
    // the C call
    std::vector<const mkhe_ct*> a, b;
    std::vector<const mkhe_swk*> b1, b2, d1, d2, v;
    for (auto* c : ops0) a.push_back(c->h);
    for (auto* c : ops1) b.push_back(c->h);
    for (auto& i : ops1[0]->ids) { auto& k = rlkSet.GetRelinearizationKey(i); b1.push_back(k.Value[0]->Value[0]->h); b2.push_back(k.Value[1]->Value[0]->h); }
    for (auto& i : ops0[0]->ids) {
        auto& k = rlkSet.GetRelinearizationKey(i);
        d1.push_back(k.Value[0]->Value[1]->h); d2.push_back(k.Value[1]->Value[1]->h); v.push_back(k.Value[0]->Value[2]->h);
    }
    mkbfv::Ciphertext want(params, ido), got(params, ido);
    mkhe::check(mkhe_bfv_mul_relin_sum(params.ctx, K, a.data(), b.data(), b1.data(), b2.data(), d1.data(), d2.data(), v.data(), params.CRS[-1]->h, want.h));
    eval.MulRelinSum(ops0, ops1, rlkSet, got);
    auto fresh = eval.MulRelinSumNew(ops0, ops1, rlkSet);
    vec w(want.words()), g(got.words()), f(fresh->words());
    want.download(w.data()); got.download(g.data()); fresh->download(f.data());
    expect(g == w, "mkbfv::Evaluator::MulRelinSum");
    expect(fresh->ids == want.ids && f == w, "mkbfv::Evaluator::MulRelinSumNew");
    // one pair is MulRelinNew
    auto one = eval.MulRelinSumNew({ops0[0]}, {ops1[0]}, rlkSet), ref = eval.MulRelinNew(*ops0[0], *ops1[0], rlkSet);
    vec o(one->words()), r(ref->words());
    one->download(o.data()); ref->download(r.data());
    expect(o == r, "one pair equals MulRelinNew");
    bool threw = false;
    try { eval.MulRelinSum(ops0, {}, rlkSet, got); } catch (const mkhe::Error&) { threw = true; }
    expect(threw, "MulRelinSum refuses lists of different lengths");
    threw = false;
    try { eval.MulRelinSumNew({}, {}, rlkSet); } catch (const mkhe::Error&) { threw = true; }
    expect(threw, "MulRelinSumNew refuses empty lists");
    std::printf("%s\n", fails ? "FAILED" : "bfv mulrelin sum mirror ok");
    return fails ? 1 : 0;
}
