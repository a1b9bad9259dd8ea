// engine_bfv_sum.hip -- Context::bfv_mul_relin_sum: K MK-BFV products under ONE Quantize and ONE relinearisation tail (no reference counterpart: the
// reference relinearises every product, mkbfv/evaluator.go:78-140).  Up to the Quantize and up to step F2 MulAndRelinBFVHoisted
// (keyswitch_hoisted.go:36-206) is linear in the pair: the tensor terms of all pairs are summed over R in the NTT domain before one Quantize, the
// t_i = ExtB(h(c0_i), y) of all pairs before one F2 (include/mkhe.h, mkhe_bfv_mul_relin_sum: the definition).
//
// Launch set.  Per pair, on the main stream: ModUpQtoR / Rescale into ONE coefficient-domain block (reused: the next pair's conversion waits for the
// side stream's transform of this one), DecomposeBFV of the party components, x / y -- by-products of the F1 kernel wherever bfv_mul_relin takes them
// that way -- the F1 kernel, whose ModDown accumulates into tbuf (t_i += ..), and step E, whose ModDown accumulates into ebuf (e_j += ..).  Beside
// it on the side stream: ntt_r of the pair into its own block of the K-fold NTT scratch, and behind the last one ONE tensor_sum_kernel (modulus
// through d_map_r, scale MForm(t)), ONE inverse ntt_r and ONE basis conversion: out_o = Quantize(z_o).  Then once, on the main stream behind that
// store: out_j += e_j (one elementwise launch) and F2 as bfv_mr_finish runs it (ntt16_f2_kernel where f2_fused_ok holds, Decompose elsewhere).
// Every sum is one of canonical residues: K = 1 is bfv_mul_relin bit for bit and the order of the pairs is immaterial.
#include "engine.h"
#include <algorithm>

namespace mkhe {

void Context::bfv_mul_relin_sum(const std::vector<const Ct*>& op0, const std::vector<const Ct*>& op1, const Swk* const* rlk_b1,
                                const Swk* const* rlk_b2, const Swk* const* rlk_d1, const Swk* const* rlk_d2, const Swk* const* rlk_v,
                                const Swk& crs_u, Ct& out) {
    const int K = (int)op0.size();
    if (!is_bfv()) throw Error("mkhe_bfv_mul_relin_sum: BFV contexts only (mkhe_mul_relin_sum is the CKKS / mkrlwe call)");
    if (masked_) throw Error("mkhe_bfv_mul_relin_sum: this context owns a subset of the moduli");
    if (K < 1 || K > TSUM_MAX_K || (int)op1.size() != K) throw Error("mkhe_bfv_mul_relin_sum: takes 1 to " + std::to_string(TSUM_MAX_K) + " pairs");
    // the tensor accumulator: 2 K <= 32 products of canonical residues in 128 bits and one redc128
    for (int l = 0; l < 2 * nq; ++l)
        if (moduli[l < nq ? l : mtot + (l - nq)] >> 60) throw Error("mkhe_bfv_mul_relin_sum: every prime of Q and QMul must be below 2^60");
    const int level = nq - 1, L = nq, n0 = op0[0]->n, n1 = op1[0]->n;
    for (int k = 0; k < K; ++k) {
        if (op0[k]->ids != op0[0]->ids || op0[k]->n != n0 || op1[k]->ids != op1[0]->ids || op1[k]->n != n1) throw Error("mkhe_bfv_mul_relin_sum: every pair must carry the ids of the first");
        if (op0[k]->limbs != nq || op1[k]->limbs != nq) throw Error("mkhe_bfv_mul_relin_sum: BFV ciphertexts live at the maximum level");
        if (op0[k]->d == out.d || op1[k]->d == out.d) throw Error("mkhe_bfv_mul_relin_sum: out must be distinct from every operand");
    }
    std::vector<int> slot0, slot1;
    // (out at the maximum level, its ids the union; the C entry point names the call)
    if (out.limbs != nq) throw Error("mkhe: BFV ciphertexts live at the maximum level");
    if (n0 > 32 || n1 > 32 || out.n > 32) throw Error("mkhe: too many parties");
    union_slots(*op0[0], *op1[0], out, "mkhe: ctOut", slot0, slot1);
    if (n0 > MAX_TERMS || n1 > MAX_TERMS) throw Error("mkhe_bfv_mul_relin_sum: too many parties");
    for (int a = 0; a < n0; ++a) if (!rlk_d1[a] || !rlk_d2[a] || !rlk_v[a]) throw Error("mkhe_bfv_mul_relin_sum: cannot GetRelinearizationKey: there is no relinearization key with given id");
    for (int a = 0; a < n1; ++a) if (!rlk_b1[a] || !rlk_b2[a]) throw Error("mkhe_bfv_mul_relin_sum: cannot GetRelinearizationKey: there is no relinearization key with given id");

    const size_t PR = 2 * (size_t)nq * N, PQ = (size_t)nq * N, item_words = (size_t)mtot * N;
    const int npair = 2 + n0 + n1, npo = 1 + out.n;        // polynomials of a pair: c0_0, c0_i, c1_0, c1_j
    // x, y and step E inside the F1 kernel wherever bfv_mul_relin takes them that way
    const bool fuse_x = ab_fuse_x() && n0 >= 1 && n0 <= 4;
    const bool fuse_y = fuse_x && ab_fuse_y() && n1 >= 1 && n1 <= 4;
    const bool fuse_e = fuse_y && ab_fuse_e() && 2 * n0 + n1 <= EXT_MAX_ITEMS;

    // ---- what the call needs; inside a capture nothing may be allocated (a block that grows waits for the stream and moves)
    const size_t want_r = (size_t)((K + 1) * npair + npo) * PR, want_t = (size_t)std::max(n0 + n1, 1) * PQ;
    const char* in_capture = "mkhe_bfv_mul_relin_sum: not available inside mkhe_capture_begin .. mkhe_capture_end before a call of this shape outside one (the call allocates)";
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(stream, &cs);
    const bool capturing = cs != hipStreamCaptureStatusNone;
    // (the schedule of ntt16_f2_kernel is built, in device memory, at the first question about its shape)
    if (capturing && fuse_e && n0 >= 2 && logN == 15 && f2_sched_.find(((long)n0 << 8) | level) == f2_sched_.end()) throw Error(in_capture);
    const bool f2 = fuse_e && n0 >= 2 && f2_fused_ok(level, n0, n1);
    const int f2_extra = f2 ? 2 * n0 * (f2_schedule(n0, level).parts - 1) : 0;
    const size_t want_c = (size_t)std::max(std::max(n0 + 2 * n1, 2 * n0 + f2_extra), 1) * item_words;
    if (capturing) {
        const int nh[5] = {n0, n1, f2 ? 0 : n0, n0, n1};
        bool grows = rbuf_.words < want_r || tbuf_.words < want_t || c1b_.words < want_c;
        for (int w = 0; w < 5; ++w) grows = grows || (int)hoist_pool_[w].size() < nh[w];
        if (grows) throw Error(in_capture);
    }
    u64* rb = scratch(rbuf_, want_r);
    u64 *r0 = rb, *r1 = rb + (size_t)(1 + n0) * PR, *fb = rb + (size_t)npair * PR, *tz = fb + (size_t)K * npair * PR;
    u64* tbuf = scratch(tbuf_, want_t);
    u64* ebuf = tbuf + (size_t)n0 * PQ;
    scratch(c1b_, want_c);
    std::vector<const u64*> h0a(n0), h0b(n0), h1a(n1), h1b(n1);
    for (int a = 0; a < n0; ++a) { h0a[a] = hoist_slot(0, a).d; h0b[a] = hoist_slot(3, a).d; if (!f2) hoist_slot(2, a); }
    for (int a = 0; a < n1; ++a) { h1a[a] = hoist_slot(1, a).d; h1b[a] = hoist_slot(4, a).d; }

    for (int k = 0; k < K; ++k) {
        // ---- the pair over R (coefficient domain: this pair only) and its transforms (kept: the tensor kernel reads all K)
        if (k) join_side(1);                               // the side stream has read the previous pair out of r0, r1
        bfv_modup_q_to_r(op0[k]->d, r0, 1 + n0);
        bfv_rescale(op1[k]->d, r1, 1 + n1);
        fork_side(1);
        s_ = overlap ? stream2 : stream;
        ntt_r(r0, fb + (size_t)k * npair * PR, npair, false);
        side_done(1);
        s_ = stream;
        // ---- DecomposeBFV of the party components (evaluator.go:126-133)
        {
            std::vector<const u64*> src; std::vector<u64*> d1, d2;
            for (int a = 0; a < n0; ++a) { src.push_back(r0 + (size_t)(1 + a) * PR); d1.push_back(hoist_slot(0, a).d); d2.push_back(hoist_slot(3, a).d); }
            for (int a = 0; a < n1; ++a) { src.push_back(r1 + (size_t)(1 + a) * PR); d1.push_back(hoist_slot(1, a).d); d2.push_back(hoist_slot(4, a).d); }
            if (!src.empty()) bfv_decompose_batch(src, d1, d2, true);
        }
        // ---- x1, x2, y1, y2 that the F1 kernel does not produce (keyswitch_hoisted.go:86-134): y on the main stream, x on the side stream
        bool x_on_side = false;
        for (int which = fuse_y ? 1 : 3; which >= (fuse_x ? 2 : 0); --which) {
            const int side = which >> 1, half = which & 1;
            const int n = side ? n1 : n0;
            std::vector<const u64*> keys(n);
            for (int a = 0; a < n; ++a) keys[a] = (side ? (half ? rlk_b2[a] : rlk_b1[a]) : (half ? rlk_d2[a] : rlk_d1[a]))->d;
            const bool on_side = side == 0 && overlap;
            if (which == 1 && on_side) fork_side(2);
            if (on_side) { s_ = stream2; x_on_side = true; }
            key_inner_product(keys.data(), (side ? (half ? h1b : h1a) : (half ? h0b : h0a)).data(), n, side ? (half ? y2_ : y_) : (half ? x2_ : x_), level, beta_max, true);
            if (on_side) s_ = stream;
            if (which == 0 && on_side) side_done(2);
        }
        // ---- F1: t_i += ExtB(h(c0_i), y1, y2)
        std::vector<ExtItem> items;
        for (int a = 0; a < n0; ++a) {
            ExtItem it{h0a[a], y_, tbuf + (size_t)a * PQ, k > 0}; it.ah2 = h0b[a]; it.bg2 = y2_;
            if (fuse_x) { it.xkey = rlk_d1[a]->d; it.xkey2 = rlk_d2[a]->d; }
            items.push_back(it);
        }
        ExtFuse fuse;
        if (fuse_x) { fuse.xout = x_; fuse.xout2 = x2_; }
        if (fuse_y) for (int a = 0; a < n1; ++a) { fuse.ykeys.push_back(rlk_b1[a]->d); fuse.ykeys2.push_back(rlk_b2[a]->d); fuse.yh.push_back(h1a[a]); fuse.yh2.push_back(h1b[a]); }
        // (step E in the thread: its products land behind the slots of both batches of this pair and are copied into the E batch's)
        if (fuse_e) fuse.e_slot = n0 + n1;
        if (!items.empty()) ext_batch(level, items, -1, 0, 0, fuse);
        // ---- E: e_j += ExtB(h(c1_j), x1, x2)
        items.clear();
        for (int a = 0; a < n1; ++a) {
            ExtItem it{h1a[a], x_, ebuf + (size_t)a * PQ, k > 0}; it.ah2 = h1b[a]; it.bg2 = x2_;
            if (fuse_e) { it.pre = true; it.pre_src = c1b_.p + (size_t)(n0 + n1 + a) * item_words; }
            items.push_back(it);
        }
        if (x_on_side) join_side(2);
        if (!items.empty()) ext_batch(level, items);
    }

    // ---- once, on the side stream behind the last pair's transform: z_o = t * sum_k (tensor terms), out_o = Quantize(z_o)
    s_ = overlap ? stream2 : stream;
    {
        TensorSumArgs ta{};
        ta.in = fb; ta.out = tz; ta.mods = d_mods; ta.map = d_map_r; ta.scale = d_t_mont; ta.pair_words = (long)npair * (long)PR;
        ta.K = K; ta.nout = out.n; ta.L = 2 * nq; ta.N = N;
        tensor_sum_terms(ta, n0, n1, slot0, slot1, out.n);
        { ProfScope ps(this, PROF_TENSOR, 8.0 * N * 2 * nq * ((double)K * npair + npo)); launch_tensor_sum(ta, s_); }
        ntt_r(tz, tz, npo, true);
        // conv.Quantize behind its MulScalar (basis_extension.go:66-80): ModDownQPtoQ with QMul as "P"
        BasisConvArgs qa{};
        quantize_tail_args(qa, *this, tz, out.d, npo);
        { ProfScope ps(this, PROF_BASISCONV, 8.0 * N * npo * 3.0 * nq); launch_basis_conv(qa, s_); }
    }
    side_done(1);
    s_ = stream;

    // ---- F2, once: h(t_i) beside the Quantize chain, then out_j += e_j ; out_0 += ExtH(h(t_i), v_i) ; out_i += ExtH(h(t_i), u) behind its store
    ExtFuse tail;
    {
        std::vector<const u64*> dsrc; std::vector<u64*> ddst;
        for (int a = 0; a < n0; ++a) { dsrc.push_back(tbuf + (size_t)a * PQ); if (!f2) ddst.push_back(hoist_slot(2, a).d); }
        if (f2) tail.f2_src = dsrc;
        else if (n0) decompose_batch(level, dsrc, ddst, true);
    }
    join_side(1);
    if (n1) {
        CtBinArgs ba{};
        ba.mods = d_mods; ba.L = L; ba.N = N; ba.ncomp = n1;
        for (int a = 0; a < n1; ++a) { ba.dst[a] = out.d + (size_t)(1 + slot1[a]) * PQ; ba.a[a] = ba.dst[a]; ba.b[a] = ebuf + (size_t)a * PQ; ba.mode[a] = 0; }
        { ProfScope ps(this, PROF_OTHER, 8.0 * N * L * 3.0 * n1); launch_ct_binary(ba, s_); }
    }
    std::vector<ExtItem> items;
    for (int a = 0; a < n0; ++a) {
        const u64* ht = f2 ? tbuf + (size_t)a * PQ : hoist_slot(2, a).d;
        items.push_back(ExtItem{ht, rlk_v[a]->d, out.d, true});
        if (f2) { items.back().f2_party = a; items.back().f2_key = 0; }
        items.push_back(ExtItem{ht, crs_u.d, out.d + (size_t)(1 + slot0[a]) * PQ, true});
        if (f2) { items.back().f2_party = a; items.back().f2_key = 1; }
    }
    if (!items.empty()) ext_batch(level, items, -1, 0, 0, tail);
    MKHE_HIP(hipGetLastError());
}

}  // namespace mkhe
