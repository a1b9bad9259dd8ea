// ckks_encode.hip -- Context methods of the CKKS encoder (ckks_kernels.h): slots <-> real coefficients <-> RNS plaintext, the message
// layer of mkckks/encryptor.go:42-64 (EncryptMsg, EncodeMsgNew) and mkckks/decryptor.go:34-43 (Decrypt).  lattigo's ckks.Encoder, which
// those lines call, is not in the reference tree: what is restated is the canonical embedding with full packing, not lattigo's code path.
//
// Launch sets (count messages each):
//   embed / project   one FFT launch for n up to the LDS limit (2^13 points, or 2^11 when the runtime grants no more than the default
//                     LDS), else two launches around the work buffer ck_work_ [count][n] complex
//   scale_up          one launch;   scale_down   one launch, with the digit scratch ck_dig_ [count][limbs][N]
//   encode = scale_up(embed), decode = project(scale_down): the same launches around the coefficient scratch ck_coeff_ [count][N]
// Sparse packing (n = 2^logSlots < N/2 slots, ckks_kernels.h): the same transform with logn = logSlots on compact coefficients [count][2n] in ck_coeff_
//   embed_sparse      transform, then one launch that spreads the 2n values over the grid of [count][N] and zeroes the rest
//   project_sparse    one launch that picks the grid, then the transform
//   encode_sparse     transform, one sparse scale_up launch (N threads: residues on the grid, zeros off it)
//   decode_sparse     one sparse scale_down launch (2n threads, digit scratch [count][limbs][2n]), transform
//   n < 16            the transform is one launch of a direct sum (ck_direct_kernel): the register tail of the tile transform takes 16 points
// ck_work_, ck_dig_ and ck_coeff_ hold message-derived values and are zeroed behind their last use.  The tables (twiddles, twist,
// permutation per slot count; the Garner constants of Context::garner_table) are built at the first call that needs them: the calls allocate and upload, so the C ABI refuses them inside a capture.
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
    ck_tab_.resize(logN);
    garner_table();
    ck_tables(logN - 1);
    ck_tile_.log = ck_tile_.granted = ck_fft_big_lds() ? CK_TILE_LOG_BIG : CK_TILE_LOG;
    ck_ready_ = true;
}
// the tables of the ring of degree 2n, n = 2^logn slots
const Context::CkTables& Context::ck_tables(int logn) {
    CkTables& t = ck_tab_[logn];
    if (t.ready) return t;
    const long n = 1L << logn;
    const size_t mark = mem_.mark();
    try {
        if (logn >= 4) {
            std::vector<double> w(n), twist(2 * n);
            for (long k = 0; k < n / 2; ++k) unit_root(k, n, w[2 * k], w[2 * k + 1]);
            for (long k = 0; k < n; ++k) unit_root(k, 4 * n, twist[2 * k], twist[2 * k + 1]);          // xi = exp(i pi / 2n) = exp(2 pi i / 4n)
            t.w = mem_.upload(w); t.twist = mem_.upload(twist); t.pos = mem_.upload(slot_positions(logn + 1, 2, false));
        } else {
            // zeta_j^k = exp(2 pi i 5^j k / 4n), as a 64th root: unit_root wants M >= 8
            std::vector<double> root(2 * n * n);
            long e = 1;
            for (long j = 0; j < n; ++j, e = e * 5 % (4 * n))
                for (long k = 0; k < n; ++k) unit_root(e * k % (4 * n) * (16 / n), 64, root[2 * (j * n + k)], root[2 * (j * n + k) + 1]);
            t.root = mem_.upload(root);
        }
    } catch (...) { mem_.rollback(mark); throw; }
    t.ready = true;
    return t;
}
int Context::ckks_tile() {
    ck_init("mkhe_ctx_ckks_tile");
    return ck_tile_.log;
}
void Context::ckks_set_tile(int log_points) {
    ck_init("mkhe_ctx_set_ckks_tile");
    ck_tile_.set(log_points, CK_TILE_LOG, CK_TILE_LOG, "mkhe_ctx_set_ckks_tile: the limit is " + std::to_string(CK_TILE_LOG) + ", ");
}

// the transform of `count` messages of n = 2^logn slots: in / out as CkFft::in / out (coefficients: [count][2n])
void Context::ck_fft(bool inverse, int logn, int count, const double* in, double* out) {
    const CkTables& t = ck_tables(logn);
    const long n = 1L << logn;
    if (logn < 4) {
        ProfScope ps(this, PROF_OTHER, 32.0 * n * count + 16.0 * n * n);
        launch_ck_direct(inverse, count, in, out, reinterpret_cast<const double2*>(t.root), logn, s_);
        return;
    }
    CkFft a{};
    a.in = in; a.out = out;
    a.w = reinterpret_cast<const double2*>(t.w); a.twist = reinterpret_cast<const double2*>(t.twist); a.pos = t.pos;
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
    ck_fft(true, logN - 1, count, slots, coeffs);
    MKHE_HIP(hipGetLastError());
}
void Context::ckks_project(int count, const double* coeffs, double* slots) {
    ck_init("mkhe_ckks_project");
    ck_fft(false, logN - 1, count, coeffs, slots);
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
    ck_fft(true, logN - 1, count, slots, m);
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
    ck_fft(false, logN - 1, count, m, slots);
    MKHE_HIP(hipMemsetAsync(m, 0, words * sizeof(double), s_));
    MKHE_HIP(hipGetLastError());
}

// ---- sparse packing (ckks_kernels.h): the transform of the ring of degree 2n on the compact scratch ck_coeff_ [count][2n], and the moves between it
// and the grid.  log_slots = logN - 1 is full packing: the calls above.
int Context::ck_sparse_init(const char* what, int log_slots) {
    ck_init(what);
    if (log_slots < 0 || log_slots > logN - 1) throw Error(std::string(what) + ": log_slots must be 0 .. " + std::to_string(logN - 1));
    return logN - 1 - log_slots;
}
void Context::ckks_embed_sparse(int log_slots, int count, const double* slots, double* coeffs) {
    const int gap_log = ck_sparse_init("mkhe_ckks_embed_sparse", log_slots);
    if (!gap_log) return ckks_embed(count, slots, coeffs);
    const size_t words = (size_t)count << (log_slots + 1);
    double* m = reinterpret_cast<double*>(scratch(ck_coeff_, words));
    ck_fft(true, log_slots, count, slots, m);
    {
        ProfScope ps(this, PROF_OTHER, 8.0 * words + 8.0 * count * N);
        launch_ck_spread(count, m, coeffs, N, gap_log, s_);
    }
    MKHE_HIP(hipMemsetAsync(m, 0, words * sizeof(double), s_));
    MKHE_HIP(hipGetLastError());
}
void Context::ckks_project_sparse(int log_slots, int count, const double* coeffs, double* slots) {
    const int gap_log = ck_sparse_init("mkhe_ckks_project_sparse", log_slots);
    if (!gap_log) return ckks_project(count, coeffs, slots);
    const size_t words = (size_t)count << (log_slots + 1);
    double* m = reinterpret_cast<double*>(scratch(ck_coeff_, words));
    {
        ProfScope ps(this, PROF_OTHER, 16.0 * words);
        launch_ck_pick(count, coeffs, m, N, gap_log, s_);
    }
    ck_fft(false, log_slots, count, m, slots);
    MKHE_HIP(hipMemsetAsync(m, 0, words * sizeof(double), s_));
    MKHE_HIP(hipGetLastError());
}
void Context::ckks_encode_sparse(int level, int log_slots, int count, const double* slots, double scale, u64* pt) {
    check_level(level);
    const int gap_log = ck_sparse_init("mkhe_ckks_encode_sparse", log_slots);
    if (!gap_log) return ckks_encode(level, count, slots, scale, pt);
    const size_t words = (size_t)count << (log_slots + 1);
    double* m = reinterpret_cast<double*>(scratch(ck_coeff_, words));
    ck_fft(true, log_slots, count, slots, m);
    {
        ProfScope ps(this, PROF_OTHER, 8.0 * words + 8.0 * count * N * (level + 1));
        launch_ck_sparse_scale_up(count, m, scale, pt, d_mods, level + 1, N, gap_log, s_);
    }
    MKHE_HIP(hipMemsetAsync(m, 0, words * sizeof(double), s_));
    MKHE_HIP(hipGetLastError());
}
void Context::ckks_decode_sparse(int limbs, int log_slots, int count, const u64* pt, double scale, double* slots) {
    check_level(limbs - 1);
    const int gap_log = ck_sparse_init("mkhe_ckks_decode_sparse", log_slots);
    if (!gap_log) return ckks_decode(limbs, count, pt, scale, slots);
    const size_t words = (size_t)count << (log_slots + 1);
    double* m = reinterpret_cast<double*>(scratch(ck_coeff_, words));
    u64* dig = scratch(ck_dig_, words * limbs);
    {
        ProfScope ps(this, PROF_OTHER, (double)words * (8.0 + 8.0 * limbs * (2.0 + (limbs - 1) / 2.0 + 2.0)));
        launch_ck_sparse_scale_down(count, pt, scale, m, dig, d_garner_, nq, d_mods, limbs, N, gap_log, s_);
    }
    MKHE_HIP(hipMemsetAsync(dig, 0, words * limbs * sizeof(u64), s_));
    ck_fft(false, log_slots, count, m, slots);
    MKHE_HIP(hipMemsetAsync(m, 0, words * sizeof(double), s_));
    MKHE_HIP(hipGetLastError());
}

}  // namespace mkhe
