// engine_mulrelin_sum.hip -- Context::mul_relin_sum: K products under ONE relinearisation tail (no reference counterpart: the reference relinearises
// every product, cnn/cnn.go:16-31,51-61).  The second half of MulAndRelinHoisted (keyswitch_hoisted.go:156-178) is linear in t_i = <h(c0_i), y>_P up to
// gadget noise, so the t_i^k of the K pairs are summed first and step F2 (Decompose, the products with v_i and u, their inverse NTT and ModDown) runs once.
//
// Launch set.  One forward NTT launch per operand and ONE tensor_sum_kernel for the tensor terms of all pairs (side stream; NTT domain, times P: the
// ExtItem::qadd of the first product that reaches each output slot).  Then per pair, through the one-pair path's own kernels: hoisting when the caller
// did not, the F1 kernel -- with x^k, y^k and step E computed in it wherever mul_and_relin would (same switches, same shapes) -- whose products the
// ModDown accumulates into tbuf (t_i += ..), and step E's products into out.  Then mr_f2_hoist and mr_finish_tail as they are, on each ring's own
// launch set (the F2 products out of the Decompose NTT at N = 2^15, staged digits at N = 2^14).  Every sum is a sum of separately ModDown'd products,
// canonical: K = 1 is mul_and_relin bit for bit and the order of the pairs is immaterial.
#include "engine.h"
#include <algorithm>

namespace mkhe {

void tensor_sum_terms(TensorSumArgs& ta, int n0, int n1, const std::vector<int>& slot0, const std::vector<int>& slot1, int nout) {
    const unsigned A0 = 0, B0 = 1 + n0, none = 255;
    std::vector<unsigned> ta_a(1 + nout, none), ta_b(1 + nout, none);
    for (int a = 0; a < n0; ++a) ta_a[1 + slot0[a]] = 1 + a;
    for (int a = 0; a < n1; ++a) ta_b[1 + slot1[a]] = 2 + n0 + a;
    ta.term[0] = A0 | B0 << 8 | none << 16 | none << 24;
    for (int o = 1; o <= nout; ++o) {
        if (ta_a[o] != none && ta_b[o] != none) ta.term[o] = B0 | ta_a[o] << 8 | A0 << 16 | ta_b[o] << 24;
        else if (ta_a[o] != none) ta.term[o] = B0 | ta_a[o] << 8 | none << 16 | none << 24;
        else ta.term[o] = A0 | ta_b[o] << 8 | none << 16 | none << 24;
    }
}

void Context::mul_relin_sum(const std::vector<const Ct*>& op0, const std::vector<const Ct*>& op1, const std::vector<const Swk*>& hoist0,
                            const std::vector<const Swk*>& hoist1, const Swk* const* rlk_b1, const Swk* const* rlk_d0, const Swk* const* rlk_v0,
                            const Swk& crs_u, bool rescale_out, Ct& out) {
    const int K = (int)op0.size();
    if (is_bfv()) throw Error("mkhe_mul_relin_sum: CKKS / mkrlwe contexts only (mkbfv carries a double gadget)");
    if (masked_) throw Error("mkhe_mul_relin_sum: this context owns a subset of the moduli");
    if (K < 1 || (int)op1.size() != K) throw Error("mkhe_mul_relin_sum: internal: the lists of a call hold one entry per pair");      // (1 .. TSUM_MAX_K: the C entry point's check, and launch_tensor_sum's)
    if (rescale_out) {
        // the product one level up in a pooled temporary, then Rescale: the integers mkhe_rescale gives (the tail's ModDown is not the only writer of
        // op1's slots here, so the division does not ride on its store)
        const int L = out.limbs + 1;
        if (out.limbs < 1 || L > nq) throw Error("mkhe_mul_relin_sum: cannot Rescale: the product would be at level 0 or above the top");
        Ct full; full.n = out.n; full.limbs = L; full.ids = out.ids;
        const size_t words = (size_t)(1 + out.n) * L * N;
        full.d = pool_alloc(words);
        const HandleUsers none;            // (never left this context: see mul_relin_rescale)
        try {
            mul_relin_sum(op0, op1, hoist0, hoist1, rlk_b1, rlk_d0, rlk_v0, crs_u, false, full);
            rescale(full, 1, out);
        } catch (...) { pool_free(full.d, words, &none); throw; }
        pool_free(full.d, words, &none);
        return;
    }
    MrPlan& p = plan_;
    p = MrPlan{};
    p.level = out.limbs - 1; p.L = p.level + 1;
    check_level(p.level);
    const int level = p.level, L = p.L, n0 = op0[0]->n, n1 = op1[0]->n;
    p.n0 = n0; p.n1 = n1; p.nout = out.n;
    if (n0 > 32 || n1 > 32 || out.n > 32) throw Error("mkhe_mul_relin_sum: too many parties");
    for (int k = 0; k < K; ++k) {
        if (op0[k]->ids != op0[0]->ids || op0[k]->n != n0 || op1[k]->ids != op1[0]->ids || op1[k]->n != n1) throw Error("mkhe_mul_relin_sum: every pair must carry the ids of the first");
        if (op0[k]->limbs < L || op1[k]->limbs < L) throw Error("mkhe_mul_relin_sum: an operand has fewer limbs than the product");
        if (op0[k]->d == out.d || op1[k]->d == out.d) throw Error("mkhe_mul_relin_sum: out must be distinct from every operand");
    }
    if (!hoist0.empty() && (int)hoist0.size() != K * n0) throw Error("mkhe_mul_relin_sum: hoist0 must hold one form per pair and party");
    if (!hoist1.empty() && (int)hoist1.size() != K * n1) throw Error("mkhe_mul_relin_sum: hoist1 must hold one form per pair and party");
    // out ids = the union of the operand id sets (mr_prepare)
    union_slots(*op0[0], *op1[0], out, "mkhe_mul_relin_sum: out", p.slot0, p.slot1);
    for (int a = 0; a < n0; ++a) if (!rlk_d0[a] || !rlk_v0[a]) throw Error("mkhe_mul_relin_sum: cannot GetRelinearizationKey: there is no relinearization key with given id");
    for (int a = 0; a < n1; ++a) if (!rlk_b1[a]) throw Error("mkhe_mul_relin_sum: cannot GetRelinearizationKey: there is no relinearization key with given id");
    if (n0 > MAX_TERMS || n1 > MAX_TERMS) throw Error("mkhe_mul_relin_sum: too many parties");

    const size_t PO = (size_t)L * N, item_words = (size_t)mtot * N;
    const int npair = 2 + n0 + n1;                         // polynomials of a pair: c0_0, c0_i, c1_0, c1_j
    // as in mr_prepare: the tensor term stays in the NTT domain, times P, and joins the summed Q parts of the first product of its slot
    const bool fold = n0 >= 1 && 2 * n0 + n1 <= EXT_MAX_ITEMS && ext_merge_members(level) >= 2;
    // the F1 kernel forms wherever mul_and_relin takes them: x as its by-product, y inside it, step E inside it
    const bool fuse_all = ab_fuse_x() && ab_fuse_y() && ab_fuse_e() && n0 >= 1 && n1 >= 1 && (n0 <= 4 ? n1 <= 4 : (n0 <= 8 && n1 == n0)) && 2 * n0 + n1 <= EXT_MAX_ITEMS;
    // every scratch block before the first launch that names one (a block that grows waits for the stream and moves)
    u64* nb_ = scratch(nttbuf_, (size_t)K * npair * PO);
    u64* tbuf = scratch(tbuf_, (size_t)std::max(n0, 1) * PO);
    u64* tens = fold ? scratch(tens_, (size_t)(1 + out.n) * PO) : out.d;
    if (fuse_all) scratch(c1b_, (size_t)(n0 + 2 * n1) * item_words);

    // ---- D: the tensor terms of all pairs, on the side stream: meets the main chain at the first product that carries them
    fork_side(1);
    s_ = overlap ? stream2 : stream;
    {
        for (int k = 0; k < K; ++k)
            for (int side = 0; side < 2; ++side) {
                const Ct& c = side ? *op1[k] : *op0[k];
                NttBatch b{};
                b.mods = d_mods; b.psi = d_psi; b.aux = d_inv_aux; slots_q_owned(b, L);
                b.src_inner = b.dst_inner = N; b.dst_outer = (long)PO;
                b.src = c.d; b.src_outer = (long)c.limbs * N; b.dst = nb_ + ((size_t)k * npair + (side ? 1 + n0 : 0)) * PO; b.nouter = 1 + c.n;
                ntt_fwd_launch(b, false);
            }
        TensorSumArgs ta{};
        ta.in = nb_; ta.out = tens; ta.mods = d_mods; ta.scale = fold ? d_pmodq : nullptr; ta.pair_words = (long)npair * (long)PO;
        ta.K = K; ta.nout = out.n; ta.L = L; ta.N = N;
        tensor_sum_terms(ta, n0, n1, p.slot0, p.slot1, out.n);
        { ProfScope ps(this, PROF_TENSOR, 8.0 * N * L * ((double)K * npair + 1 + out.n)); launch_tensor_sum(ta, s_); }
        if (!fold) ntt(out.d, out.d, 1 + out.n, L, 0, true, false);
    }
    side_done(1);
    s_ = stream;
    bool tensor_joined = false;

    // ---- per pair: hoist, x^k / y^k, F1 (t_i += ..) and E (out_j += ..)
    const int nb = beta(level);
    std::vector<char> e_written(n1, 0);
    for (int k = 0; k < K; ++k) {
        const Ct& c0 = *op0[k]; const Ct& c1 = *op1[k];
        const bool same = &c0 == &c1 && hoist0.empty() && hoist1.empty();
        p.h0.assign(n0, nullptr); p.h1.assign(n1, nullptr);
        std::vector<const u64*> dsrc; std::vector<u64*> ddst;
        for (int a = 0; a < n0; ++a) {
            if (!hoist0.empty()) p.h0[a] = hoist0[(size_t)k * n0 + a]->d;
            else { Swk& s = hoist_slot(0, a); dsrc.push_back(c0.d + (size_t)(1 + a) * c0.limbs * N); ddst.push_back(s.d); p.h0[a] = s.d; }
        }
        for (int a = 0; a < n1; ++a) {
            if (!hoist1.empty()) p.h1[a] = hoist1[(size_t)k * n1 + a]->d;
            else if (same) p.h1[a] = p.h0[a];
            else { Swk& s = hoist_slot(1, a); dsrc.push_back(c1.d + (size_t)(1 + a) * c1.limbs * N); ddst.push_back(s.d); p.h1[a] = s.d; }
        }
        if (!dsrc.empty()) decompose_batch(level, dsrc, ddst, true);
        std::vector<ExtItem> f1, e;
        for (int a = 0; a < n0; ++a) f1.push_back(ExtItem{p.h0[a], y_, tbuf + (size_t)a * PO, k > 0});
        for (int a = 0; a < n1; ++a) {
            u64* dst = out.d + (size_t)(1 + p.slot1[a]) * PO;
            e.push_back(ExtItem{p.h1[a], x_, dst, true});
            if (fold && !e_written[a]) { e.back().accumulate = false; e.back().qadd = tens + (dst - out.d); e_written[a] = 1; }
        }
        const bool carries_tensor = !tensor_joined && !e.empty();      // (not folded: every E product accumulates onto the tensor term in out)
        if (fuse_all) {
            // F1 with x, y and step E in the thread: the E products land behind the slots of both batches of this pair and are copied into theirs
            ExtFuse fuse;
            fuse.xout = x_;
            for (int a = 0; a < n0; ++a) f1[a].xkey = rlk_d0[a]->d;
            for (int a = 0; a < n1; ++a) { fuse.ykeys.push_back(rlk_b1[a]->d); fuse.yh.push_back(p.h1[a]); }
            fuse.e_slot = n0 + n1;
            ext_batch(level, f1, -1, 0, 0, fuse);
            for (int a = 0; a < n1; ++a) { e[a].pre = true; e[a].pre_src = c1b_.p + (size_t)(n0 + n1 + a) * item_words; }
            if (carries_tensor) { join_side(1); tensor_joined = true; }
            ext_batch(level, e);
        } else {
            for (int side = 1; side >= 0; --side) {
                const int n = side ? n1 : n0;
                std::vector<const u64*> keys(n);
                for (int a = 0; a < n; ++a) keys[a] = (side ? rlk_b1[a] : rlk_d0[a])->d;
                key_inner_product(keys.data(), (side ? p.h1 : p.h0).data(), n, side ? y_ : x_, level, nb, true);
            }
            f1.insert(f1.end(), e.begin(), e.end());
            if (carries_tensor) { join_side(1); tensor_joined = true; }
            if (!f1.empty()) ext_batch(level, f1);
        }
    }
    if (!tensor_joined && !fold) join_side(1);             // (no E product at all: out holds the tensor term alone so far)

    // ---- F2 and the tail, once: h(t_i) ; out_0 += <h(t_i), v_i>_P ; out_i += <h(t_i), u>_P
    if (n0 == 0) { MKHE_HIP(hipGetLastError()); return; }  // (no party in op0: nothing to relinearise, and the term was not folded)
    p.tens = fold ? tens : nullptr;
    p.e_summed = true;
    p.f2_tbuf = tbuf;
    p.f2_fused = p.tens != nullptr && f2_fused_ok(level, n0, n1);
    mr_f2_hoist(true);
    p.valid = true; p.head_done = true;
    mr_finish_tail(*op0[0], *op1[0], x_, rlk_v0, crs_u, out);
}

}  // namespace mkhe
