// engine_ops.hip -- Context: Rotate[Hoisted] / Conjugate, Rescale, the elementwise evaluator operations
#include "engine.h"
#include <algorithm>
#include <cstring>
#include <cstdlib>

namespace mkhe {

// ------------------------------------------------------------------ Rotate[Hoisted] / Conjugate
// keyswitch.go:234-298, keyswitch_hoisted.go:183-247
void Context::rotate(u64 galEl, const Ct& in, const Swk* const* hoist, const Swk* const* rk, const Swk& crs, Ct& out) {
    const int L = out.limbs, n = in.n;
    if (n > 0 && 2 * n <= EXT_MAX_ITEMS && in.d != out.d) {
        // the signed permutation and the + c_0 ride on the ModDown of the external products: no staging copy of the
        // ciphertext, no separate permutation kernel
        rotate_core(in, hoist, rk, crs, true, out, galEl);
        return;
    }
    Ct tmp; tmp.n = n; tmp.limbs = L; tmp.ids = in.ids;
    tmp.d = scratch(ctbuf_, (size_t)(1 + n) * L * N);
    rotate_partial(in, hoist, rk, crs, true, tmp);
    automorphism(galEl, tmp, out);
}

// Rotate without the final permutation: out_0 = [c_0 +] sum_i <h(c_i), rk_i>_P, out_i = <h(c_i), crs>_P
// (keyswitch.go:251-265).  with_c0 = false leaves c_0 out (party-sharded evaluation: one rank adds it).
void Context::rotate_partial(const Ct& in, const Swk* const* hoist, const Swk* const* rk, const Swk& crs, bool with_c0, Ct& out) {
    rotate_core(in, hoist, rk, crs, with_c0, out, 0);
}
void Context::rotate_core(const Ct& in, const Swk* const* hoist, const Swk* const* rk, const Swk& crs, bool with_c0, Ct& out, u64 galEl) {
    const int level = out.limbs - 1, L = level + 1, n = in.n;
    check_level(level);
    if (in.limbs < L) throw Error("Cannot Rotate: ctIn and ctOut have different levels");
    if (out.n != n || out.ids != in.ids) throw Error("mkhe: ctOut must carry the ids of ctIn");
    const size_t PI = (size_t)in.limbs * N, PO = (size_t)L * N;
    u64* tmp = out.d;
    const bool fused = galEl != 0;          // c_0 enters as the addend of the first accumulating item, stores are permuted
    if (fused && !with_c0) throw Error("mkhe: a fused rotation includes c_0");
    if (!fused) {
        if (with_c0) MKHE_HIP(hipMemcpyAsync(tmp, in.d, PO * sizeof(u64), hipMemcpyDeviceToDevice, s_));
        else MKHE_HIP(hipMemsetAsync(tmp, 0, PO * sizeof(u64), s_));
    }
    std::vector<const u64*> h(n);
    bool f2 = false;
    ExtFuse fuse;
    {
        std::vector<const u64*> dsrc; std::vector<u64*> ddst;
        for (int a = 0; a < n; ++a) {
            if (!rk[a]) throw Error("cannot GetRotationKeys: there is no rotation key with given id");
            if (hoist) { if (!hoist[a]) throw Error("mkhe: missing hoisted form"); h[a] = hoist[a]->d; }
            else { Swk& s = hoist_slot(0, a); dsrc.push_back(in.d + (1 + a) * PI); ddst.push_back(s.d); h[a] = s.d; }
        }
        // (a rotation of a ciphertext without a hoisted form: its digits are read once, by the two products below -- small launches finish their
        // transform inside the product kernel; N = 2^15 launches that fill the chip never store them at all: ntt16_f2_kernel, as step F2 of MulAndRelin)
        f2 = !hoist && n >= 2 && f2_fused_ok(level, n, 0);
        const bool stage = !f2 && !hoist && ext_fused_ok(level, (int)dsrc.size());
        if (f2) { fuse.f2_src = dsrc; h = dsrc; }
        else if (!dsrc.empty()) decompose_batch(level, dsrc, ddst, true, stage);
        if (stage) fuse.staged.assign(ddst.begin(), ddst.end());
    }
    std::vector<ExtItem> items;
    for (int a = 0; a < n; ++a) {
        items.push_back(ExtItem{h[a], rk[a]->d, tmp, true});
        if (fused && a == 0) items.back().addend = in.d;
        if (f2) { items.back().f2_party = a; items.back().f2_key = 0; }
        items.push_back(ExtItem{h[a], crs.d, tmp + (size_t)(1 + a) * PO, false});
        if (f2) { items.back().f2_party = a; items.back().f2_key = 1; }
    }
    ext_batch(level, items, -1, 0, galEl, fuse);
    MKHE_HIP(hipGetLastError());
}

// signed coefficient permutation X -> X^galEl of every component (keyswitch.go:267-296)
void Context::automorphism(u64 galEl, const Ct& in, Ct& out) {
    const int L = out.limbs;
    if (in.limbs != L || in.n != out.n) throw Error("mkhe: automorphism operands differ in shape");
    if (in.d == out.d) throw Error("mkhe: automorphism cannot run in place");
    launch_automorphism(out.d, in.d, d_mods, L, logN, galEl, 1 + in.n, s_);
    MKHE_HIP(hipGetLastError());
}

// keyswitch.go:302-332
void Context::conjugate(u64 galEl, const Ct& in, const Swk* const* ck, const Swk& crs, Ct& out) {
    const int level = out.limbs - 1, L = level + 1, n = in.n;
    check_level(level);
    if (in.limbs < L) throw Error("Cannot Conjugate: ctIn and ctOut have different levels");
    if (out.n != n || out.ids != in.ids) throw Error("mkhe: ctOut must carry the ids of ctIn");
    const size_t PI = (size_t)in.limbs * N, PO = (size_t)L * N;
    u64* tmp = scratch(ctbuf_, (size_t)(1 + n) * PO);
    if (in.limbs == L) launch_automorphism(tmp, in.d, d_mods, L, logN, galEl, 1 + n, s_);
    else for (int a = 0; a <= n; ++a) launch_automorphism(tmp + a * PO, in.d + a * PI, d_mods, L, logN, galEl, 1, s_);
    if (n == 0) { MKHE_HIP(hipMemcpyAsync(out.d, tmp, PO * sizeof(u64), hipMemcpyDeviceToDevice, s_)); return; }
    // all parties in one Decompose launch and one batch of external products, like Rotate; sigma(c_0) enters as the addend
    // of the first accumulating item (the permuted polynomials keep q for a sign-flipped 0, exactly what the reference
    // decomposes)
    std::vector<const u64*> dsrc; std::vector<u64*> ddst;
    for (int a = 0; a < n; ++a) {
        if (!ck[a]) throw Error("cannot GetConjugationKey: there is no conjugation key with given id");
        dsrc.push_back(tmp + (size_t)(1 + a) * PO); ddst.push_back(hoist_slot(0, a).d);
    }
    const bool f2 = n >= 2 && f2_fused_ok(level, n, 0);           // (as Rotate: the digits of the permuted polynomials stay in registers)
    const bool stage = !f2 && ext_fused_ok(level, n);
    ExtFuse fuse;
    if (f2) fuse.f2_src = dsrc;
    else decompose_batch(level, dsrc, ddst, true, stage);
    if (stage) fuse.staged.assign(ddst.begin(), ddst.end());
    std::vector<ExtItem> items;
    for (int a = 0; a < n; ++a) {
        items.push_back(ExtItem{f2 ? dsrc[a] : ddst[a], ck[a]->d, out.d, true});
        if (a == 0) items.back().addend = tmp;
        if (f2) { items.back().f2_party = a; items.back().f2_key = 0; }
        items.push_back(ExtItem{f2 ? dsrc[a] : ddst[a], crs.d, out.d + (size_t)(1 + a) * PO, false});
        if (f2) { items.back().f2_party = a; items.back().f2_key = 1; }
    }
    ext_batch(level, items, -1, 0, 0, fuse);
    MKHE_HIP(hipGetLastError());
}

// ------------------------------------------------------------------ Rescale body
// mkckks/evaluator.go:385-391 -> lattigo DivRoundByLastModulusManyLvl.  The reference's in-place
// "+ (q_L-1)/2" on the dropped limb of ctIn is NOT reproduced (ctIn stays untouched).
void Context::rescale(const Ct& in, int nb, Ct& out) {
    const int level = in.limbs - 1;
    check_level(level);
    if (nb < 0 || nb > level) throw Error("cannot Rescale: input Ciphertext already at level 0");
    if (out.limbs != in.limbs - nb || out.n != in.n) throw Error("mkhe: ctOut shape does not match the rescaled ciphertext");
    const int np_ = 1 + in.n;
    const size_t PI = (size_t)in.limbs * N, PO = (size_t)out.limbs * N;
    if (nb == 0) { if (out.d != in.d) MKHE_HIP(hipMemcpyAsync(out.d, in.d, np_ * PI * sizeof(u64), hipMemcpyDeviceToDevice, s_)); return; }
    // source and destination polynomials have different strides (in.limbs vs out.limbs): in place the threads of one polynomial
    // would overwrite limbs of the next one that other threads still read
    if (out.d == in.d) throw Error("cannot Rescale in place: ctOut must not alias ctIn when levels are dropped");
    if (nb == 1) {
        launch_div_round_last(out.d, in.d, d_mods, d_rescale + (size_t)(level - 1) * nq, level, N, np_, (long)PI, (long)PO, s_);
    } else {
        u64* tmp = scratch(ctbuf_, (size_t)np_ * PI);
        launch_div_round_last(tmp, in.d, d_mods, d_rescale + (size_t)(level - 1) * nq, level, N, np_, (long)PI, (long)PI, s_);
        for (int k = 1; k < nb; ++k) {
            const int lv = level - k;
            const bool last = (k == nb - 1);
            launch_div_round_last(last ? out.d : tmp, tmp, d_mods, d_rescale + (size_t)(lv - 1) * nq, lv, N, np_,
                                  (long)PI, last ? (long)PO : (long)PI, s_);
        }
    }
    MKHE_HIP(hipGetLastError());
}

// ------------------------------------------------------------------ elementwise evaluator ops
// evaluateInPlace of mkckks/evaluator.go:41-70 and mkbfv/evaluator.go:27-62: c_0 and the components both
// operands have are combined, the others are copied (Sub: negated when only op1 has them, :59-66).
void Context::ct_binary(int op, const Ct& a, const Ct& b, Ct& out) {
    const int L = out.limbs;
    if (a.limbs < L || b.limbs < L) throw Error("mkhe: operand level below ctOut level");
    const size_t PA = (size_t)a.limbs * N, PB = (size_t)b.limbs * N, PO = (size_t)L * N;
    auto find = [](const Ct& c, int id) { for (int i = 0; i < c.n; ++i) if (c.ids[i] == id) return i; return -1; };
    if (1 + out.n > CTBIN_MAX) throw Error("mkhe: too many parties in one ciphertext");
    CtBinArgs ba{};
    ba.mods = d_mods; ba.L = L; ba.N = N; ba.ncomp = 1 + out.n;
    double bytes = 0;
    for (int o = -1; o < out.n; ++o) {
        const int ia = o < 0 ? 0 : 1 + find(a, out.ids[o]), ib = o < 0 ? 0 : 1 + find(b, out.ids[o]);
        const bool ha = o < 0 || ia > 0, hb = o < 0 || ib > 0;
        if (!ha && !hb) throw Error("mkhe: ctOut has an id that neither operand has");
        const int c = 1 + o;
        ba.dst[c] = out.d + (size_t)c * PO;
        ba.a[c] = ha ? a.d + ia * PA : nullptr;
        ba.b[c] = hb ? b.d + ib * PB : nullptr;
        ba.mode[c] = (ha && hb) ? (op == 0 ? 0 : 1) : ha ? 2 : (op == 0 ? 3 : 4);
        bytes += 8.0 * N * L * ((ha && hb) ? 3 : 2);
    }
    { ProfScope ps(this, PROF_OTHER, bytes); launch_ct_binary(ba, s_); }
    MKHE_HIP(hipGetLastError());
}

void Context::ct_mul_const(const Ct& in, const u64* c_first, const u64* c_second, Ct& out) {
    const int L = std::min(in.limbs, out.limbs);                   // level := min(ct0.Level(), ctOut.Level()), :119
    if (in.n != out.n || in.ids != out.ids) throw Error("mkhe: ctOut must carry the ids of ct0");
    if (L > 48) throw Error("mkhe: too many limbs");
    MulConstArgs a{};
    a.src = in.d; a.dst = out.d; a.mods = d_mods; a.src_poly = (long)in.limbs * N; a.dst_poly = (long)out.limbs * N;
    a.L = L; a.N = N; a.npolys = 1 + in.n;
    for (int l = 0; l < L; ++l) {
        if (c_first[l] >= moduli[l] || c_second[l] >= moduli[l]) throw Error("mkhe: MultByConst constants must be reduced");
        a.c[0][l] = c_first[l]; a.c[1][l] = c_second[l];
    }
    { ProfScope ps(this, PROF_OTHER, 16.0 * N * L * (1 + in.n)); launch_mul_const_halves(a, s_); }
    MKHE_HIP(hipGetLastError());
}

// Weighted sum with complex weights, an additive constant and an optional Rescale in ONE pass (launch_ct_lincomb): every input limb is read once and
// every output limb written once, (n + 1) * 8 * N * Lc * (1 + parties) bytes -- the chain n x ct_mul_const, ct_sum, rescale moves (3n + 3) of them.
void Context::ct_lincomb(const std::vector<const Ct*>& ins, const u64* dev_consts, int nb_rescale, Ct& out) {
    const int n = (int)ins.size();
    if (n < 1 || n > CTLIN_MAX) throw Error("mkhe: ct_lincomb takes 1 to " + std::to_string(CTLIN_MAX) + " ciphertexts");
    if (!dev_consts) throw Error("mkhe: ct_lincomb: null constants");
    if (nb_rescale != 0 && nb_rescale != 1) throw Error("mkhe: ct_lincomb divides by the last modulus once or not at all");
    const int Lc = out.limbs + nb_rescale;
    if (out.limbs < 1) throw Error("cannot Rescale: input Ciphertext already at level 0");          // (Lc = 1 with a division: nothing would be left)
    check_level(Lc - 1);
    const size_t PO = (size_t)out.limbs * N, out_words = (size_t)(1 + out.n) * PO;
    CtLincombArgs a{};
    for (int k = 0; k < n; ++k) {
        const Ct& c = *ins[k];
        if (c.n != out.n || c.ids != out.ids) throw Error("mkhe: ct_lincomb: every summand and ctOut must carry the same ids");
        if (c.limbs < Lc) throw Error("mkhe: ct_lincomb: a summand has fewer limbs than the sum (limbs(ctOut) + nb_rescale)");
        // every thread stores limbs of out before it has read all limbs of its inputs: no overlap at all
        if (c.d < out.d + out_words && out.d < c.d + (size_t)(1 + c.n) * c.limbs * N) throw Error("mkhe: ct_lincomb: ctOut must not alias a summand");
        a.in[k] = c.d; a.in_poly[k] = (long)c.limbs * N;
    }
    a.dst = out.d; a.dst_poly = (long)PO; a.mods = d_mods; a.consts = dev_consts;
    if (nb_rescale) { a.rescale_row = d_rescale + (size_t)(Lc - 2) * nq; a.rescale_h = a.rescale_row + (size_t)nq * nq; }
    a.n = n; a.Lc = Lc; a.N = N; a.npolys = 1 + out.n;
    { ProfScope ps(this, PROF_OTHER, 8.0 * N * Lc * (n + 1.0) * (1 + out.n)); launch_ct_lincomb(a, s_); }
    MKHE_HIP(hipGetLastError());
}

// outs[g] = sum_b W[g][b] ins[b] + C[g] with integer weights, for all outputs in ONE pass (launch_bfv_ct_lincomb): every input limb is read once and
// every output limb written once, 8 N nQ (1 + k) (nin + nout) bytes -- ct_lincomb once per output moves nout * (nin_g + 1) passes of 8 N nQ (1 + k).
// Every refusal is under `what` (the C entry point) and comes before the launch.
void Context::bfv_ct_lincomb(const char* what, const std::vector<const Ct*>& ins, const u64* dev_consts, const std::vector<Ct*>& outs) {
    const std::string w = std::string(what) + ": ";
    const int nin = (int)ins.size(), nout = (int)outs.size();
    if (nin < 1 || nin > BLIN_MAX_IN) throw Error(w + "nin must be 1 .. " + std::to_string(BLIN_MAX_IN));
    if (nout < 1 || nout > BLIN_MAX_OUT) throw Error(w + "nout must be 1 .. " + std::to_string(BLIN_MAX_OUT));
    if (!dev_consts) throw Error(w + "null argument");
    const Ct& c0 = *ins[0];
    const int L = nq, np_ = 1 + c0.n;
    const size_t CO = (size_t)np_ * L * N;
    BfvLincombArgs a{};
    for (int b = 0; b < nin; ++b) {
        if (ins[b]->n != c0.n || ins[b]->ids != c0.ids) throw Error(w + "the ciphertexts of a list must share their ids");
        if (ins[b]->limbs != L) throw Error(w + "BFV ciphertexts sit at the maximum level (nQ limbs)");
        a.in[b] = ins[b]->d;
    }
    for (int g = 0; g < nout; ++g) {
        if (outs[g]->n != c0.n || outs[g]->ids != c0.ids) throw Error(w + "an output must carry the ids of the inputs");
        if (outs[g]->limbs != L) throw Error(w + "BFV ciphertexts sit at the maximum level (nQ limbs)");
        for (int h = 0; h < g; ++h)
            if (outs[g]->d < outs[h]->d + CO && outs[h]->d < outs[g]->d + CO) throw Error(w + "the outputs must be distinct");
        // a thread stores its word of every output while other threads still read the inputs: no overlap at all
        for (const Ct* c : ins)
            if (c->d < outs[g]->d + CO && outs[g]->d < c->d + CO) throw Error(w + "an output must not alias an input");
        a.out[g] = outs[g]->d;
    }
    a.mods = d_mods; a.consts = dev_consts; a.nin = nin; a.nout = nout; a.L = L; a.N = N; a.npolys = np_;
    { ProfScope ps(this, PROF_OTHER, 8.0 * N * L * np_ * (nin + nout)); launch_bfv_ct_lincomb(a, s_); }
    MKHE_HIP(hipGetLastError());
}

// outs[g] = sum_b (re[g][b] + i im[g][b]) ins[b] + (add_re[g] + i add_im[g]), then nb_rescale divisions by the last modulus, for all outputs in ONE pass
// (launch_ct_lincomb_multi): every input limb is read once and every output limb written once, 8 N (1 + k) (nin Lc + nout L) bytes -- ct_lincomb once
// per output reads the nin inputs nout times.  Every refusal is under `what` (the C entry point) and comes before the launch.
void Context::ct_lincomb_multi(const char* what, const std::vector<const Ct*>& ins, const u64* dev_consts, int nb_rescale, const std::vector<Ct*>& outs) {
    const std::string w = std::string(what) + ": ";
    const int nin = (int)ins.size(), nout = (int)outs.size();
    if (nin < 1 || nin > CTLM_MAX_IN) throw Error(w + "nin must be 1 .. " + std::to_string(CTLM_MAX_IN));
    if (nout < 1 || nout > CTLM_MAX_OUT) throw Error(w + "nout must be 1 .. " + std::to_string(CTLM_MAX_OUT));
    if (nb_rescale != 0 && nb_rescale != 1) throw Error(w + "nb_rescale must be 0 or 1");
    if (!dev_consts) throw Error(w + "null argument");
    const Ct& o0 = *outs[0];
    const int L = o0.limbs, Lc = L + nb_rescale, np_ = 1 + o0.n;
    if (L < 1) throw Error(w + "cannot Rescale: input Ciphertext already at level 0");          // (Lc = 1 with a division: nothing would be left)
    if (Lc > nq) throw Error(w + "level out of range");
    const size_t PO = (size_t)L * N, out_words = (size_t)np_ * PO;
    CtLincombMultiArgs a{};
    for (int g = 0; g < nout; ++g) {
        const Ct& o = *outs[g];
        if (o.n != o0.n || o.ids != o0.ids) throw Error(w + "every input and output must carry the same ids");
        if (o.limbs != L) throw Error(w + "the outputs must have the same number of limbs");
        for (int h = 0; h < g; ++h)
            if (o.d < outs[h]->d + out_words && outs[h]->d < o.d + out_words) throw Error(w + "the outputs must be distinct");
        a.out[g] = o.d;
    }
    for (int b = 0; b < nin; ++b) {
        const Ct& c = *ins[b];
        if (c.n != o0.n || c.ids != o0.ids) throw Error(w + "every input and output must carry the same ids");
        if (c.limbs < Lc) throw Error(w + "an input has fewer limbs than the sums (limbs(out) + nb_rescale)");
        // a thread stores its words of every output while other threads still read the inputs: no overlap at all
        for (int g = 0; g < nout; ++g)
            if (c.d < outs[g]->d + out_words && outs[g]->d < c.d + (size_t)np_ * c.limbs * N) throw Error(w + "an output must not alias an input");
        a.in[b] = c.d; a.in_poly[b] = (long)c.limbs * N;
    }
    a.out_poly = (long)PO; a.mods = d_mods; a.consts = dev_consts;
    if (nb_rescale) { a.rescale_row = d_rescale + (size_t)(Lc - 2) * nq; a.rescale_h = a.rescale_row + (size_t)nq * nq; }
    a.nin = nin; a.nout = nout; a.Lc = Lc; a.N = N; a.npolys = np_;
    { ProfScope ps(this, PROF_OTHER, 8.0 * N * np_ * ((double)nin * Lc + (double)nout * L)); launch_ct_lincomb_multi(a, s_); }
    MKHE_HIP(hipGetLastError());
}

// ct_lincomb_multi for nbatch = ins.size() / nin items in lock step (launch_ct_lincomb_batch): item i sums ins[i * nin ..] into outs[i * nout ..] with the
// constants all items share, 8 N (1 + k) nbatch (nin Lc + nout L) bytes.  The base addresses travel in the kernel arguments -- no table, no pool
// allocation -- and the launcher deals the items to as many launches as that takes.  An output of one launch could be an input of a later one, so no
// output may overlap an input of ANY item.  Every refusal is under `what` (the C entry point) and comes before the first launch.
void Context::ct_lincomb_batch(const char* what, const std::vector<const Ct*>& ins, int nin, const u64* dev_consts, int nb_rescale, const std::vector<Ct*>& outs,
                               int nout) {
    const std::string w = std::string(what) + ": ";
    if (nin < 1 || nin > CTLM_MAX_IN) throw Error(w + "nin must be 1 .. " + std::to_string(CTLM_MAX_IN));
    if (nout < 1 || nout > CTLM_MAX_OUT) throw Error(w + "nout must be 1 .. " + std::to_string(CTLM_MAX_OUT));
    if (nb_rescale != 0 && nb_rescale != 1) throw Error(w + "nb_rescale must be 0 or 1");
    if (ins.empty() || ins.size() % nin || outs.size() != ins.size() / nin * nout) throw Error(w + "nbatch must be at least 1, with nin inputs and nout outputs per item");
    if (!dev_consts) throw Error(w + "null argument");
    const size_t nbatch = ins.size() / nin;
    const Ct& o0 = *outs[0];
    const int L = o0.limbs, Lc = L + nb_rescale, np_ = 1 + o0.n;
    if (L < 1) throw Error(w + "cannot Rescale: input Ciphertext already at level 0");          // (Lc = 1 with a division: nothing would be left)
    if (Lc > nq) throw Error(w + "level out of range");
    const size_t out_words = (size_t)np_ * L * N;
    CtLincombBatchArgs a{};
    const int per = nin + nout;
    std::vector<u64*> sets(nbatch * per);
    std::vector<const u64*> ostart(outs.size());
    for (size_t i = 0; i < outs.size(); ++i) {
        const Ct& o = *outs[i];
        if (o.n != o0.n || o.ids != o0.ids) throw Error(w + "every input and output must carry the same ids");
        if (o.limbs != L) throw Error(w + "the outputs must have the same number of limbs");
        sets[i / nout * per + nin + i % nout] = o.d; ostart[i] = o.d;
    }
    // the outputs are blocks of one size: sorted by their start, two of them overlap only if two neighbours do
    std::sort(ostart.begin(), ostart.end(), std::less<const u64*>());
    for (size_t i = 1; i < ostart.size(); ++i)
        if (ostart[i] < ostart[i - 1] + out_words) throw Error(w + "the outputs must be distinct");
    for (size_t i = 0; i < ins.size(); ++i) {
        const Ct& c = *ins[i];
        const int b = (int)(i % nin);
        if (c.n != o0.n || c.ids != o0.ids) throw Error(w + "every input and output must carry the same ids");
        if (c.limbs < Lc) throw Error(w + "an input has fewer limbs than the sums (limbs(out) + nb_rescale)");
        if (c.limbs != ins[b]->limbs) throw Error(w + "input k must have the same number of limbs in every item");
        // the last output that starts below the end of this input is the only one that can reach into it
        const u64* end = c.d + (size_t)np_ * c.limbs * N;
        const auto it = std::lower_bound(ostart.begin(), ostart.end(), end, std::less<const u64*>());
        if (it != ostart.begin() && c.d < *(it - 1) + out_words) throw Error(w + "an output must not alias an input");
        sets[i / nin * per + b] = c.d;
        if (i < (size_t)nin) a.in_poly[b] = (long)c.limbs * N;
    }
    a.out_poly = (long)L * N; a.mods = d_mods; a.consts = dev_consts;
    if (nb_rescale) { a.rescale_row = d_rescale + (size_t)(Lc - 2) * nq; a.rescale_h = a.rescale_row + (size_t)nq * nq; }
    a.nin = nin; a.nout = nout; a.Lc = Lc; a.N = N; a.npolys = np_;
    { ProfScope ps(this, PROF_OTHER, 8.0 * N * np_ * nbatch * ((double)nin * Lc + (double)nout * L)); launch_ct_lincomb_batch(a, sets.data(), (int)nbatch, s_); }
    MKHE_HIP(hipGetLastError());
}

void Context::ct_mul_ptxt(const Ct& in, const u64* dev_pt, Ct& out) {
    const int L = in.limbs, np_ = 1 + in.n;
    if (out.limbs != L || out.n != in.n || out.ids != in.ids) throw Error("mkhe: ctOut shape does not match ct");
    const size_t PO = (size_t)L * N;
    u64* tmp = scratch(ctbuf_, (size_t)(1 + np_) * PO);
    ntt(dev_pt, tmp, 1, L, 0, false, false);
    ntt(in.d, tmp + PO, np_, L, 0, false, false);
    { ProfScope ps(this, PROF_OTHER, 8.0 * N * L * (2.0 * np_ + 1)); launch_mul_by_poly(tmp + PO, tmp + PO, tmp, d_mods, L, N, np_, s_); }
    ntt(tmp + PO, out.d, np_, L, 0, true, false);
    MKHE_HIP(hipGetLastError());
}

}  // namespace mkhe
