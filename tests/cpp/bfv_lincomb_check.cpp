// Uses mkbfv::Evaluator::LinCombs of include/mkhe.hpp (compile-and-link check without an argument; with one, on a GPU: the wrapper against the C call
// mkhe_bfv_ct_lincomb on the same seeded uniform inputs, and one output against 128-bit host arithmetic: tests/test_cpp_bfv_lincomb.py).
#include "mkhe.hpp"
#include <cstdio>

typedef std::vector<uint64_t> vec;
static uint64_t rng_state = 0x4c494e43ull;
static uint64_t next64() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static void fill_poly(uint64_t* p, const vec& mods, size_t N) { for (size_t l = 0; l < mods.size(); ++l) for (size_t i = 0; i < N; ++i) p[l * N + i] = next64() % mods[l]; }
static vec rand_ct(const vec& Q, int n, size_t N) { vec c((1 + n) * Q.size() * N); for (int s = 0; s <= n; ++s) fill_poly(&c[s * Q.size() * N], Q, N); return c; }
static uint64_t mulmod(uint64_t a, uint64_t b, uint64_t q) { return (uint64_t)((unsigned __int128)a * b % q); }
static uint64_t mform(uint64_t a, uint64_t q) { return (uint64_t)((((unsigned __int128)a) << 64) % q); }
static int fails = 0;
static void expect(bool ok, const char* what) { std::printf("%-64s %s\n", what, ok ? "ok" : "MISMATCH"); if (!ok) ++fails; }

int main(int argc, char**) {
    if (argc < 2) { std::printf("bfv lincomb mirror links\n"); return 0; }      // nothing below runs without a GPU
    const vec Q = {0x3fffffffd60001ull, 0x3fffffff6d0001ull, 0x3fffffff550001ull};
    const vec QMul = {0x3fffffffca0001ull, 0x3fffffff5d0001ull, 0x3fffffff390001ull};
    const vec P = {0xffffffffffc0001ull, 0xfffffffff840001ull};
    const int logN = 10, NIN = 5, NOUT = 3;
    const size_t N = 1u << logN, nQ = Q.size();
    mkbfv::Parameters params(logN, Q, QMul, P, 65537);
    mkbfv::Evaluator eval(params);
    const mkrlwe::IDSet ids{"alice", "bob"};
    std::vector<vec> host;
    std::vector<std::unique_ptr<mkbfv::Ciphertext>> cts, want, got;
    std::vector<const mkhe_ct*> in;
    std::vector<mkhe_ct*> ow, og;
    for (int b = 0; b < NIN; ++b) {
        host.push_back(rand_ct(Q, 2, N));
        cts.push_back(std::make_unique<mkbfv::Ciphertext>(params, ids)); cts.back()->upload(host.back().data());
        in.push_back(cts.back()->h);
    }
    for (int g = 0; g < NOUT; ++g) {
        want.push_back(std::make_unique<mkbfv::Ciphertext>(params, ids)); ow.push_back(want.back()->h);
        got.push_back(std::make_unique<mkbfv::Ciphertext>(params, ids)); og.push_back(got.back()->h);
    }
    // plain residues W[g][b][l], C[g][l]; output 1 has a zero weight under limb 1 only
    vec plain((size_t)NOUT * (NIN + 1) * nQ), consts(plain.size());
    for (int g = 0; g < NOUT; ++g)
        for (int r = 0; r <= NIN; ++r)
            for (size_t l = 0; l < nQ; ++l) {
                const size_t i = ((size_t)g * (NIN + 1) + r) * nQ + l;
                plain[i] = (g == 1 && r == 2 && l == 1) ? 0 : next64() % Q[l];
                consts[i] = r ? mform(plain[i], Q[l]) : plain[i];
            }
    mkrlwe::DeviceWords dev(params, (consts.size() + 1) & ~(size_t)1);
    vec padded(dev.words, 0);
    std::copy(consts.begin(), consts.end(), padded.begin());
    dev.upload(padded.data());
    mkhe::check(mkhe_bfv_ct_lincomb(params.ctx, NIN, in.data(), NOUT, dev.d, ow.data()));
    eval.LinCombs(in, dev.d, og);
    bool same = true, right = true;
    for (int g = 0; g < NOUT; ++g) {
        vec w(want[g]->words()), o(got[g]->words());
        want[g]->download(w.data()); got[g]->download(o.data());
        same = same && o == w;
        for (size_t p = 0; p < 3; ++p)
            for (size_t l = 0; l < nQ; ++l)
                for (size_t j = 0; j < N; ++j) {
                    const size_t at = (p * nQ + l) * N + j;
                    uint64_t acc = (p == 0 && j == 0) ? plain[((size_t)g * (NIN + 1)) * nQ + l] : 0;
                    for (int b = 0; b < NIN; ++b) acc = (acc + mulmod(plain[((size_t)g * (NIN + 1) + 1 + b) * nQ + l], host[b][at], Q[l])) % Q[l];
                    right = right && o[at] == acc;
                }
    }
    expect(same, "mkbfv::Evaluator::LinCombs equals mkhe_bfv_ct_lincomb");
    expect(right, "... and the sums in 128-bit host arithmetic");
    bool threw = false;
    try { eval.LinCombs(in, dev.d, {og[0], og[0]}); } catch (const mkhe::Error&) { threw = true; }
    expect(threw, "LinCombs refuses equal outputs");
    threw = false;
    try { eval.LinCombs({}, dev.d, og); } catch (const mkhe::Error&) { threw = true; }
    expect(threw, "LinCombs refuses an empty input list");
    eval.LinCombs(in, dev.d, og);                                              // the context is still usable
    std::printf("%s\n", fails ? "FAILED" : "bfv lincomb mirror ok");
    return fails ? 1 : 0;
}
