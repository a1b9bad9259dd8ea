// bfv_encode.hip -- Context methods of the BFV batch encoder (bfv_kernels.h): slots over Z_T <-> coefficients over Z_T <-> RNS plaintext, the
// message layer of mkbfv/encryptor.go:38-41 (EncryptMsg = EncodeInt, Encrypt) and mkbfv/decryptor.go:52-54 (DecodeInt).  lattigo's bfv.Encoder,
// which those lines call, is not in the reference tree: what is restated is the mathematics of the encoder, not lattigo's code path.
//
// Launch sets (count messages each):
//   slots_to_coeffs / coeffs_to_slots   one NTT launch for N up to the LDS limit (2^15 words, or 2^14 when the runtime grants no more than the
//                     default LDS), else two launches around the work buffer bf_work_ [count][N] of 32-bit words
//   scale_up          one launch;   scale_down   one launch, with the digit scratch bf_dig_ [count][nq][N]
//   encode, decode    single-workgroup form: ONE launch, scale_up in the store of the inverse transform resp. scale_down in the load of the
//                     forward one; two-launch form: the stage launches around the coefficient scratch bf_coeff_ [count][N].  The same bits.
//   encode_mul        the inverse transform with the lift (launch_bf_lift) in its store -- or, two-launch form, the lift as its own launch behind
//                     bf_coeff_ -- into bf_lift_ [count][nq][N], then ONE forward NTT over Q (Context::ntt) of its count * nq limbs into the caller's
//                     buffer.  That NTT is Z_q-linear, so the lift is written in Montgomery form at once and the prepared plaintext needs no
//                     launch of its own for it.
// bf_work_, bf_dig_, bf_coeff_ and bf_lift_ hold message-derived values and are zeroed behind their last use.  The tables (twiddles, twists, permutation,
// scaling constants; the Garner constants of Context::garner_table) are built at the first call: the calls allocate and upload, so the C ABI refuses them inside a capture.
#include "engine.h"
#include "host_modarith.h"

namespace mkhe {

static uint2 shoup(u64 w, u64 T) { return uint2{(u32)w, (u32)((w << 32) / T)}; }

void Context::bf_init(const char* what) {
    const std::string w(what);
    if (!is_bfv()) throw Error(w + ": the BFV encoder needs a BFV context");
    if (masked_) throw Error(w + ": not available on a context that owns a subset of the moduli");
    if (bf_ready_) return;
    const u64 T = bfv_t, n = (u64)N;
    if (T >= (1ull << 32)) throw Error(w + ": the plaintext modulus must be below 2^32");
    if (!is_prime(T)) throw Error(w + ": the plaintext modulus must be prime");
    if ((T - 1) % (2 * n) != 0) throw Error(w + ": the plaintext modulus must be 1 mod 2N");
    for (int l = 0; l < nq; ++l) if (moduli[l] == T) throw Error(w + ": the plaintext modulus must differ from the primes of Q");
    MKHE_HIP(hipSetDevice(device));
    const u64 psi = default_psi(T, n), psi_inv = powmod(psi, T - 2, T), n_inv = powmod(n, T - 2, T);
    const u64 om = mulmod(psi, psi, T), om_inv = mulmod(psi_inv, psi_inv, T);
    std::vector<uint2> tw(n / 2), twi(n / 2), twist(n), itwist(n);
    u64 a = 1, b = 1;
    for (u64 k = 0; k < n / 2; ++k, a = mulmod(a, om, T), b = mulmod(b, om_inv, T)) { tw[k] = shoup(a, T); twi[k] = shoup(b, T); }
    a = 1; b = n_inv;
    for (u64 k = 0; k < n; ++k, a = mulmod(a, psi, T), b = mulmod(b, psi_inv, T)) { twist[k] = shoup(a, T); itwist[k] = shoup(b, T); }
    // per limb of Q: MForm(T^-1), MForm(T), q_l mod T
    std::vector<u64> tinv(nq), tmont(nq);
    std::vector<uint2> qlt(nq);
    u64 qmod = 1;
    for (int l = 0; l < nq; ++l) {
        const u64 q = moduli[l];
        tinv[l] = to_mont(powmod(T % q, q - 2, q), q);
        tmont[l] = to_mont(T % q, q);
        qlt[l] = shoup(q % T, T);
        qmod = mulmod(qmod, q % T, T);
    }
    BfvT t{};
    t.T = (u32)T; t.half = (u32)(T / 2);
    t.qmod = (u32)qmod; t.qmod_s = shoup(qmod, T).y;
    const u64 qinv = powmod(qmod, T - 2, T);
    t.qinv = (u32)qinv; t.qinv_s = shoup(qinv, T).y;
    t.hq = (u32)mulmod((qmod + T - 1) % T, (T + 1) / 2, T);                       // (Q - 1) / 2 mod T: Q is odd
    const u64 c32 = (1ull << 32) % T;
    t.c32 = (u32)c32; t.c32_s = shoup(c32, T).y;
    t.one_s = shoup(1, T).y;
    garner_table();
    const size_t mark = mem_.mark();
    try {
        d_bf_w = mem_.upload(tw); d_bf_winv = mem_.upload(twi); d_bf_twist = mem_.upload(twist); d_bf_itwist = mem_.upload(itwist); d_bf_qlt = mem_.upload(qlt);
        d_bf_pos = mem_.upload(slot_positions(logN, 1, true)); d_bf_tinv = mem_.upload(tinv); d_bf_tmont = mem_.upload(tmont);
    } catch (...) { mem_.rollback(mark); throw; }
    bf_t_ = t; bf_psi_ = psi;
    bf_tile_.log = bf_tile_.granted = bf_ntt_big_lds() ? BF_TILE_LOG_BIG : BF_TILE_LOG_DEF;
    bf_ready_ = true;
}
int Context::bfv_tile() {
    bf_init("mkhe_ctx_bfv_tile");
    return bf_tile_.log;
}
void Context::bfv_set_tile(int log_points) {
    bf_init("mkhe_ctx_set_bfv_tile");
    bf_tile_.set(log_points, BF_TILE_LOG_MIN, bf_tile_.granted, "mkhe_ctx_set_bfv_tile: the limit is " + std::to_string(BF_TILE_LOG_MIN) + " .. ");
}
u64 Context::bfv_slot_psi() {
    bf_init("mkhe_ctx_bfv_slot_psi");
    return bf_psi_;
}
BfvScale Context::bf_scale() const {
    BfvScale sc{};
    sc.t = bf_t_; sc.mods = d_mods; sc.tinv_mont = d_bf_tinv; sc.t_mont = d_bf_tmont; sc.garner = d_garner_; sc.qlt = d_bf_qlt;
    sc.limbs = nq; sc.N = N;
    return sc;
}

// the transform of `count` messages: in / out as BfvNtt::in / out.  fuse (BF_FUSE_*): in (forward) resp. out (inverse) is the RNS plaintext,
// BF_FUSE_LIFT (inverse only): out is the multiplication plaintext in the coefficient domain.
void Context::bf_ntt(bool inverse, int fuse, int count, const u64* in, u64* out) {
    const size_t n = (size_t)N;
    BfvNtt a{};
    a.w = inverse ? d_bf_winv : d_bf_w; a.twist = inverse ? d_bf_itwist : d_bf_twist; a.pos = d_bf_pos;
    a.p.logn = logN; a.sc = bf_scale();
    const double tables = 8.0 * n + 4.0 * n + 4.0 * n;                          // twist, twiddles, permutation
    if (logN <= bf_tile_.log) {
        a.in = in; a.out = out;
        a.p.logt = logN; a.p.first = a.p.last = 1; a.fuse = fuse;
        const size_t words = (size_t)count * nq * n;
        if (fuse && !inverse) a.dig = scratch(bf_dig_, words);
        {
            // fused forward: every digit is written once and read by each later limb and by the sum
            const double rns = 8.0 * nq * n * count * (fuse && !inverse ? 3.0 + (nq - 1) / 2.0 : 1.0);
            ProfScope ps(this, PROF_OTHER, 8.0 * n * count + (fuse ? rns : 8.0 * n * count) + tables);
            launch_bf_ntt(inverse, a, count, s_);
        }
        if (fuse && !inverse) MKHE_HIP(hipMemsetAsync(a.dig, 0, words * sizeof(u64), s_));
        return;
    }
    // two launches; the scalings run as their own launches around the coefficient scratch
    const size_t cwords = (size_t)count * n;
    u64* coeff = fuse ? scratch(bf_coeff_, cwords) : nullptr;
    if (fuse && !inverse) { bf_scale_down(count, in, coeff); in = coeff; }
    a.in = in; a.out = fuse && inverse ? coeff : out;
    const size_t wwords = (cwords + 1) / 2;                                     // 32-bit words
    a.work = reinterpret_cast<u32*>(scratch(bf_work_, wwords));
    a.p.logt = std::min(bf_tile_.log, BF_TILE_LOG_MULTI);
    tile_two_pass(a.p, inverse, logN - a.p.logt, [&] {
        ProfScope ps(this, PROF_OTHER, 8.0 * n * count + 4.0 * n * count + tables / 2);
        launch_bf_ntt(inverse, a, count, s_);
    });
    MKHE_HIP(hipMemsetAsync(a.work, 0, wwords * sizeof(u64), s_));
    if (fuse == BF_FUSE_LIFT) bf_lift(count, coeff, out);
    else if (fuse && inverse) bf_scale_up(count, coeff, out);
    if (fuse) MKHE_HIP(hipMemsetAsync(coeff, 0, cwords * sizeof(u64), s_));
}
void Context::bf_scale_up(int count, const u64* coeffs, u64* pt) {
    ProfScope ps(this, PROF_OTHER, (double)count * N * (8.0 + 8.0 * nq));
    launch_bf_scale_up(count, coeffs, pt, bf_scale(), s_);
}
void Context::bf_lift(int count, const u64* coeffs, u64* ptmul) {
    ProfScope ps(this, PROF_OTHER, (double)count * N * (8.0 + 8.0 * nq));
    launch_bf_lift(count, coeffs, ptmul, bf_scale(), s_);
}
void Context::bf_scale_down(int count, const u64* pt, u64* coeffs) {
    const size_t words = (size_t)count * nq * N;
    u64* dig = scratch(bf_dig_, words);
    {
        // every digit is written once and read by each later limb and by the sum
        ProfScope ps(this, PROF_OTHER, (double)count * N * (8.0 + 8.0 * nq * (3.0 + (nq - 1) / 2.0)));
        launch_bf_scale_down(count, pt, coeffs, dig, bf_scale(), s_);
    }
    MKHE_HIP(hipMemsetAsync(dig, 0, words * sizeof(u64), s_));
}

void Context::bfv_slots_to_coeffs(int count, const u64* slots, u64* coeffs) {
    bf_init("mkhe_bfv_slots_to_coeffs");
    bf_ntt(true, BF_FUSE_NONE, count, slots, coeffs);
    MKHE_HIP(hipGetLastError());
}
void Context::bfv_coeffs_to_slots(int count, const u64* coeffs, u64* slots) {
    bf_init("mkhe_bfv_coeffs_to_slots");
    bf_ntt(false, BF_FUSE_NONE, count, coeffs, slots);
    MKHE_HIP(hipGetLastError());
}
void Context::bfv_scale_up(int count, const u64* coeffs, u64* pt) {
    bf_init("mkhe_bfv_scale_up");
    bf_scale_up(count, coeffs, pt);
    MKHE_HIP(hipGetLastError());
}
void Context::bfv_scale_down(int count, const u64* pt, u64* coeffs) {
    bf_init("mkhe_bfv_scale_down");
    bf_scale_down(count, pt, coeffs);
    MKHE_HIP(hipGetLastError());
}
void Context::bfv_encode(int count, const u64* slots, u64* pt) {
    bf_init("mkhe_bfv_encode");
    bf_ntt(true, BF_FUSE_SCALE, count, slots, pt);
    MKHE_HIP(hipGetLastError());
}
void Context::bfv_decode(int count, const u64* pt, u64* slots) {
    bf_init("mkhe_bfv_decode");
    bf_ntt(false, BF_FUSE_SCALE, count, pt, slots);
    MKHE_HIP(hipGetLastError());
}
// ---- slot map (bfv_kernels.h).  prepare validates on the host from a synchronous download and uploads one word per position.
void Context::bfv_slot_map_prepare(const u32* dev_index, const u64* dev_mult, u64* dev_map) {
    bf_init("mkhe_bfv_slot_map_prepare");
    const size_t n = (size_t)N;
    const u64 T = bfv_t;
    std::vector<u32> index(n);
    std::vector<u64> mult(n, 1), map(n);
    MKHE_HIP(hipMemcpyAsync(index.data(), dev_index, n * sizeof(u32), hipMemcpyDeviceToHost, stream));
    if (dev_mult) MKHE_HIP(hipMemcpyAsync(mult.data(), dev_mult, n * sizeof(u64), hipMemcpyDeviceToHost, stream));
    sync();
    for (size_t i = 0; i < n; ++i)
        if (index[i] >= n) throw Error("mkhe_bfv_slot_map_prepare: index[" + std::to_string(i) + "] = " + std::to_string(index[i]) + " is not a slot (0 .. N - 1)");
    const std::vector<u32> pos = slot_positions(logN, 1, true);
    std::vector<u32> inv(n);
    for (size_t p = 0; p < n; ++p) inv[pos[p]] = (u32)p;
    for (size_t p = 0; p < n; ++p) map[p] = ((u64)shoup(mult[pos[p]] % T, T).y << 32) | inv[index[pos[p]]];
    MKHE_HIP(hipMemcpyAsync(dev_map, map.data(), n * sizeof(u64), hipMemcpyHostToDevice, stream));
    sync();                                                                     // map is pageable and about to go out of scope
}
void Context::bfv_slot_map(int count, const u64* coeffs_in, const u64* dev_map, u64* coeffs_out) {
    bf_init("mkhe_bfv_slot_map");
    const size_t n = (size_t)N;
    const double tables = 2.0 * (8.0 * n + 4.0 * n) + 8.0 * n;                  // both twists, both twiddle tables, the map
    if (logN <= bf_tile_.log) {
        BfvSlotMap m{};
        m.in = coeffs_in; m.out = coeffs_out; m.map = dev_map;
        m.w = d_bf_w; m.winv = d_bf_winv; m.twist = d_bf_twist; m.itwist = d_bf_itwist;
        m.logn = logN; m.t = bf_t_;
        {
            ProfScope ps(this, PROF_OTHER, 16.0 * n * count + tables);
            launch_bf_slot_map(m, count, s_);
        }
        MKHE_HIP(hipGetLastError());
        return;
    }
    // two-launch form: forward into the first work buffer (position order: neither launch is the `last` one, whose store would scatter the
    // slots), the gather into the second, the inverse from there (neither launch the `first` one, whose load would gather slots)
    const size_t cwords = (size_t)count * n;                                    // two buffers of 32-bit words
    u32* work = reinterpret_cast<u32*>(scratch(bf_work_, cwords));
    u32* work2 = work + cwords;
    BfvNtt a{};
    a.pos = d_bf_pos; a.p.logn = logN; a.sc = bf_scale();
    a.p.logt = std::min(bf_tile_.log, BF_TILE_LOG_MULTI);
    a.w = d_bf_w; a.twist = d_bf_twist; a.in = coeffs_in; a.work = work;
    tile_two_pass(a.p, false, logN - a.p.logt, [&] {
        a.p.last = 0;
        ProfScope ps(this, PROF_OTHER, (a.p.first ? 8.0 : 4.0) * n * count + 4.0 * n * count + tables / 4);
        launch_bf_ntt(false, a, count, s_);
    });
    {
        ProfScope ps(this, PROF_OTHER, 8.0 * n * count + 8.0 * n);
        launch_bf_slot_gather(work, work2, dev_map, N, bf_t_.T, count, s_);
    }
    a.w = d_bf_winv; a.twist = d_bf_itwist; a.in = nullptr; a.out = coeffs_out; a.work = work2;
    tile_two_pass(a.p, true, logN - a.p.logt, [&] {
        a.p.first = 0;
        ProfScope ps(this, PROF_OTHER, 4.0 * n * count + (a.p.last ? 8.0 : 4.0) * n * count + tables / 4);
        launch_bf_ntt(true, a, count, s_);
    });
    MKHE_HIP(hipMemsetAsync(work, 0, cwords * sizeof(u64), s_));
    MKHE_HIP(hipGetLastError());
}

void Context::bfv_lift(int count, const u64* coeffs, u64* ptmul_coeff) {
    bf_init("mkhe_bfv_lift");
    bf_lift(count, coeffs, ptmul_coeff);
    MKHE_HIP(hipGetLastError());
}
void Context::bfv_encode_mul(int count, const u64* slots, u64* ptmul) {
    bf_init("mkhe_bfv_encode_mul");
    const size_t words = (size_t)count * nq * N;
    u64* lift = scratch(bf_lift_, words);                       // (the forward NTT is not asked to run in place)
    bf_ntt(true, BF_FUSE_LIFT, count, slots, lift);
    ntt(lift, ptmul, count, nq, 0, false, false);
    MKHE_HIP(hipMemsetAsync(lift, 0, words * sizeof(u64), s_));
    MKHE_HIP(hipGetLastError());
}

}  // namespace mkhe
