// ckks_encode.hip -- Context methods of the CKKS encoder (ckks_kernels.h): slots <-> real coefficients <-> RNS plaintext, the message
// layer of mkckks/encryptor.go:42-64 (EncryptMsg, EncodeMsgNew) and mkckks/decryptor.go:34-43 (Decrypt).  lattigo's ckks.Encoder, which
// those lines call, is not in the reference tree: what is restated is the canonical embedding with full packing, not lattigo's code path.
//
// Launch sets (count messages each):
//   embed / project   one FFT launch for n up to the LDS limit (2^13 points, or 2^11 when the runtime grants no more than the default
//                     LDS), else two launches around the work buffer ck_work_ [count][n] complex
//   scale_up          one launch;   scale_down   one launch, with the digit scratch ck_dig_ [count][limbs][N]
//   encode = scale_up(embed), decode = project(scale_down): the same launches around the coefficient scratch ck_coeff_ [count][N]
// ck_work_, ck_dig_ and ck_coeff_ hold message-derived values and are zeroed behind their last use.  The tables (twiddles, twist,
// permutation; the Garner constants of Context::garner_table) are built at the first call: the calls allocate and upload, so the C ABI refuses them inside a capture.
#include "engine.h"
#include "host_modarith.h"
#include <cmath>

namespace mkhe {

// exp(2 pi i k / M), M a power of two >= 8: the angle is reduced to the first octant as an integer, then cosl / sinl once, rounded once
static void unit_root(long k, long M, double& re, double& im) {
    k &= M - 1;
    const long quarter = M / 4, quad = k / quarter;
    long r = k % quarter;                                  // angle r / M of a turn in [0, 1/4)
    const bool swap = r > M / 8;
    if (swap) r = quarter - r;                             // cos(pi/2 - x) = sin(x)
    const long double ang = 2.0L * 3.14159265358979323846264338327950288L * (long double)r / (long double)M;
    long double c = cosl(ang), s = sinl(ang);
    if (swap) std::swap(c, s);
    switch (quad) {                                        // times i^quad
        case 0: re = (double)c; im = (double)s; break;
        case 1: re = (double)-s; im = (double)c; break;
        case 2: re = (double)-c; im = (double)-s; break;
        default: re = (double)s; im = (double)-c; break;
    }
}

void Context::ck_init(const char* what) {
    if (masked_) throw Error(std::string(what) + ": not available on a context that owns a subset of the moduli");
    if (ck_ready_) return;
    MKHE_HIP(hipSetDevice(device));
    const int logn = logN - 1;
    const long n = 1L << logn;
    std::vector<double> w(n), twist(2 * n);
    for (long k = 0; k < n / 2; ++k) unit_root(k, n, w[2 * k], w[2 * k + 1]);
    for (long k = 0; k < n; ++k) unit_root(k, 4 * n, twist[2 * k], twist[2 * k + 1]);          // xi = exp(i pi / N) = exp(2 pi i / 4n)
    garner_table();
    const size_t mark = mem_.mark();
    try { d_ck_w = mem_.upload(w); d_ck_twist = mem_.upload(twist); d_ck_pos = mem_.upload(slot_positions(logN, 2, false)); }
    catch (...) { mem_.rollback(mark); throw; }
    ck_tile_.log = ck_tile_.granted = ck_fft_big_lds() ? CK_TILE_LOG_BIG : CK_TILE_LOG;
    ck_ready_ = true;
}
int Context::ckks_tile() {
    ck_init("mkhe_ctx_ckks_tile");
    return ck_tile_.log;
}
void Context::ckks_set_tile(int log_points) {
    ck_init("mkhe_ctx_set_ckks_tile");
    ck_tile_.set(log_points, CK_TILE_LOG, CK_TILE_LOG, "mkhe_ctx_set_ckks_tile: the limit is " + std::to_string(CK_TILE_LOG) + ", ");
}

// the transform of `count` messages: in / out as CkFft::in / out
void Context::ck_fft(bool inverse, int count, const double* in, double* out) {
    const int logn = logN - 1;
    const long n = 1L << logn;
    CkFft a{};
    a.in = in; a.out = out;
    a.w = reinterpret_cast<const double2*>(d_ck_w); a.twist = reinterpret_cast<const double2*>(d_ck_twist); a.pos = d_ck_pos;
    a.p.logn = logn;
    const double io = 32.0 * n * count + 16.0 * n + 8.0 * n + 4.0 * n;        // slots + coefficients; twist, twiddles, permutation
    if (logn <= ck_tile_.log) {
        a.p.logt = logn; a.p.first = a.p.last = 1;
        ProfScope ps(this, PROF_OTHER, io);
        launch_ck_fft(inverse, a, count, s_);
        return;
    }
    a.work = reinterpret_cast<double2*>(scratch(ck_work_, 2 * (size_t)n * count));
    a.p.logt = CK_TILE_LOG;
    tile_two_pass(a.p, inverse, logn - CK_TILE_LOG, [&] {
        ProfScope ps(this, PROF_OTHER, io / 2 + 16.0 * n * count);
        launch_ck_fft(inverse, a, count, s_);
    });
    MKHE_HIP(hipMemsetAsync(ck_work_.p, 0, 2 * (size_t)n * count * sizeof(u64), s_));
}

void Context::ckks_embed(int count, const double* slots, double* coeffs) {
    ck_init("mkhe_ckks_embed");
    ck_fft(true, count, slots, coeffs);
    MKHE_HIP(hipGetLastError());
}
void Context::ckks_project(int count, const double* coeffs, double* slots) {
    ck_init("mkhe_ckks_project");
    ck_fft(false, count, coeffs, slots);
    MKHE_HIP(hipGetLastError());
}
void Context::ck_scale_up(int level, int count, const double* coeffs, double scale, u64* pt) {
    const int L = level + 1;
    ProfScope ps(this, PROF_OTHER, (double)count * N * (8.0 + 8.0 * L));
    launch_ck_scale_up(count, coeffs, scale, pt, d_mods, L, N, s_);
}
void Context::ck_scale_down(int limbs, int count, const u64* pt, double scale, double* coeffs) {
    const size_t words = (size_t)count * limbs * N;
    u64* dig = scratch(ck_dig_, words);
    {
        // every digit is written once and read by each later limb, by the sign decision and by the sum
        ProfScope ps(this, PROF_OTHER, (double)count * N * (8.0 + 8.0 * limbs * (2.0 + (limbs - 1) / 2.0 + 2.0)));
        launch_ck_scale_down(count, pt, scale, coeffs, dig, d_garner_, nq, d_mods, limbs, N, s_);
    }
    MKHE_HIP(hipMemsetAsync(dig, 0, words * sizeof(u64), s_));
}
void Context::ckks_scale_up(int level, int count, const double* coeffs, double scale, u64* pt) {
    check_level(level);
    ck_init("mkhe_ckks_scale_up");
    ck_scale_up(level, count, coeffs, scale, pt);
    MKHE_HIP(hipGetLastError());
}
void Context::ckks_scale_down(int limbs, int count, const u64* pt, double scale, double* coeffs) {
    check_level(limbs - 1);
    ck_init("mkhe_ckks_scale_down");
    ck_scale_down(limbs, count, pt, scale, coeffs);
    MKHE_HIP(hipGetLastError());
}
void Context::ckks_encode(int level, int count, const double* slots, double scale, u64* pt) {
    check_level(level);
    ck_init("mkhe_ckks_encode");
    const size_t words = (size_t)count * N;
    double* m = reinterpret_cast<double*>(scratch(ck_coeff_, words));
    ck_fft(true, count, slots, m);
    ck_scale_up(level, count, m, scale, pt);
    MKHE_HIP(hipMemsetAsync(m, 0, words * sizeof(double), s_));
    MKHE_HIP(hipGetLastError());
}
void Context::ckks_decode(int limbs, int count, const u64* pt, double scale, double* slots) {
    check_level(limbs - 1);
    ck_init("mkhe_ckks_decode");
    const size_t words = (size_t)count * N;
    double* m = reinterpret_cast<double*>(scratch(ck_coeff_, words));
    ck_scale_down(limbs, count, pt, scale, m);
    ck_fft(false, count, m, slots);
    MKHE_HIP(hipMemsetAsync(m, 0, words * sizeof(double), s_));
    MKHE_HIP(hipGetLastError());
}

}  // namespace mkhe
