// ntt_route.h -- which kernels an NTT launch runs: the whole decision, in host C++ without a HIP header (tests/cpp/ntt_route_check.cpp
// compiles it alone and prints the route of every threshold; DESIGN.md section 4.1a is that table).
//
// ntt_fwd_route / ntt_inv_route read the shape of a launch (NttShape) and the A/B values (NttSwitches) and return the kernels in launch order.
// What depends on the device -- how many workgroups are resident, where the long jobs go, half-limb jobs -- is decided by the launchers
// (launch_ntt_step and its peers, ntt_kernels.h); Context::ntt_fwd_launch / ntt_inv_launch walk the steps and do nothing else.
#pragma once
#include <stdexcept>

namespace mkhe {

// timing records of the NTT launches: the head of Context's PROF_* classes (engine.h continues the list behind PROF_NTT_CLASSES)
enum { PROF_NTT_DECOMP = 0, PROF_NTT_DECOMP_BIGQ, PROF_NTT_DECOMP_MIXED, PROF_NTT16_DECOMP, PROF_NTT16_FWD, PROF_NTT32_DECOMP, PROF_NTT32_FWD, PROF_NTT14_SPLIT,
       PROF_NTT_FWD, PROF_NTT_FWD_BIGQ, PROF_NTT_INV, PROF_NTT_CLASSES };

#ifndef MKHE_NTT32_DEFAULT
// MKHE_NTT32: 0 = every launch on the two-pass H16 kernel, 1 = the single-pass H32 kernel wherever it applies, 2 (default) = per launch shape the engine
// times a block of launches of each kernel inside the caller's workload, once its clocks have settled, and keeps the faster one (Context::ntt_pick).  Back
// to back H32 is ahead on every part (230 against 244 us for 1792 limbs, same call); inside the MulRelin it is ahead by 2-5 % on most parts (0.526-0.542
// against 0.506-0.519 of the roofline, eight same-call pairs, MulRelin/s + 0-2 %) and BEHIND by 6 % on some (0.46-0.48 against 0.49-0.515, MulRelin/s
// - 1.6 %: parts that sit at 1255 W and 2.09 GHz under it where the others reach 1400 W and 2.2-2.3 GHz, with the same configured cap -- the two-pass
// kernel's in-context time is the same on both kinds): profiles/README.md.
#define MKHE_NTT32_DEFAULT 2
#endif

// Every A/B and configuration value the routes read; ntt_switches() (ntt_kernels.hip) fills it once per process.  Only MKHE_NTT32 is configuration
// (read by every build); the others are their defaults in the product library (switches.h).
struct NttSwitches {
    int ntt32 = MKHE_NTT32_DEFAULT, ntt32_min = 512;                    // MKHE_NTT32, MKHE_NTT32_MIN: H32 from this many limbs (N = 2^15)
    int ntt16 = 1, ntt16_min = 128, ntt14_min = 128;                    // MKHE_NTT16, MKHE_NTT16_MIN (N = 2^15; sub-transforms of N = 2^16: half-limb jobs), MKHE_NTT14_MIN
    int ntt16_inv = 1, ntt16_inv_min = 256, ntt14_inv_min = 129;        // MKHE_NTT16_INV, MKHE_NTT16_INV_MIN (one-pass jobs of 2^14 points), MKHE_NTT14_INV_MIN (limbs)
    int ntt_lds = 1;                                                    // MKHE_NTT_LDS: the LDS sub-transforms of small N = 2^14 / 2^15 launches
    int ntt16_radix4 = 1;                                               // MKHE_NTT16_RADIX4: N = 2^16 as one radix-4 pass + H16 quarters
    int ntt16_halves = 1;                                               // MKHE_NTT16_HALVES: half-limb jobs of ragged Decompose launches (read by the H16 launcher, not by the route)
};

struct NttShape {
    int logN = 0, nslots = 0, nouter = 0;
    int jobs = 0;                                   // vi ? vi_jobs : nslots * nouter (merged inverse launches: the jobs that exist)
    unsigned long long small = 0;                   // bit s: slot s has a modulus with 34 q < 2^63 (the signed never-reduced forward butterflies, MODE 1)
    unsigned long long small16 = 0;                 // bit s: 48 q < 2^62 (no partial reductions in the H16 / H32 kernels)
    unsigned long long u = 0;                       // bit s: the U class (160 q < 2^62)
    int reduce_in = 0, split = 0, prestaged = 0, prestaged_oop = 0, vi = 0;     // NttBatch's fields of these names
    bool decompose = false;                         // the launch is a Decompose (its timing class; reduce_in says what the kernel does)
    bool psi31 = false, psi31b = false, psi31c = false;      // forward pair tables of the context
    bool psiinv31 = false, inv31c = false;                   // inverse ones
    bool no_h16 = false;                            // a modulus outside the ranges of the H16 kernels (or no pair table for this direction)
};

// one value per family of template instantiations; the step's other fields pick the member
enum NttKernel {
    NK_FWD_REG,         // ntt_fwd_kernel<logn, MODE 0 / 1 by class, dec>: register-resident, one pass
    NK_FWD_MIXED,       // ntt_fwd_kernel<15, 2, true>: both classes in one persistent grid
    NK_SPLIT_FWD,       // ntt_split_fwd_kernel<dec>: cross-half radix-2 pass
    NK_PASS4_FWD,       // ntt_pass4_fwd_kernel<dec>: two cross stages in one pass
    NK_PASS8_FWD,       // ntt_pass8_fwd_kernel<dec>: three
    NK_FWD_LDS,         // ntt_fwd_lds_kernel<MODE, logn>: 2^depth sub-transforms of 2^logn points per limb in LDS (logn = 11, 12)
    NK_H16_FWD,         // ntt16_fwd_kernel<dec>: N = 2^15, two passes per limb
    NK_H14_FWD,         // ntt14_fwd_kernel<dec>: N = 2^14, one pass
    NK_H16_SPLIT,       // ntt16_fwd_split_kernel: the 2^15-point halves of N = 2^16
    NK_H14_SPLIT,       // ntt14_fwd_split_kernel: the 2^14-point quarters of N = 2^16
    NK_H32_FWD,         // ntt32_fwd_kernel<dec>: N = 2^15, one pass, one workgroup per CU
    NK_INV_REG,         // ntt_inv_kernel<logn, vi>
    NK_SPLIT_INV, NK_PASS4_INV, NK_PASS8_INV,       // the cross stages of the inverse, in place on dst
    NK_INV_LDS,         // ntt_inv_ldsS_kernel<logn>
    NK_H14_INV,         // ntt14_inv_kernel: one-pass 2^14-point sub-transforms
};
struct NttStep {
    NttKernel kernel;
    int logn;           // points of one transform of this kernel (cross passes: the whole limb)
    int split;          // NttBatch::split as the kernel receives it
    int depth;          // LDS kernels: cross stages in front of (forward) / behind (inverse) the sub-transforms
    int jobs;           // transforms (cross passes: limbs) of the launch
    bool in_place;      // reads dst: an earlier step, or the producer of a prestaged launch, has put the data there
    bool dec;           // reads digits under a foreign modulus (NttBatch::reduce_in; every later step sees reduce_in = 0)
};
// which slots a part takes, in which order (order_slots_by_class): one modulus class, or all slots with the long jobs first
enum NttSlots { NS_AS_IS, NS_SMALL, NS_BIG, NS_BIG_SMALL, NS_BIG16_SMALL16, NS_BIG16_SMALL16_U };
struct NttPart {
    NttSlots slots;
    int prof;           // PROF_*: the timing class its launches are recorded under
    bool side;          // forward, two class parts: this one goes to the side stream (their ragged last rounds fill each other's idle CUs)
    int nsteps;
    NttStep step[2];
};
struct NttRoute {
    bool pick;          // H32 and H16 both qualify and MKHE_NTT32 = 2: part[0] is the H32 launch, part[1] the H16 one, Context::ntt_pick decides
    int nparts;         // otherwise: all of them, in launch order
    NttPart part[2];
};

namespace ntt_route_detail {
inline int popcount(unsigned long long v) { int n = 0; for (; v; v &= v - 1) ++n; return n; }
inline void push(NttPart& p, NttKernel k, int logn, int split, int depth, long jobs, bool in_place, bool dec) { p.step[p.nsteps++] = NttStep{k, logn, split, depth, (int)jobs, in_place, dec}; }
// A limb is one workgroup's work for 60-70 us whatever the batch size, so a launch with fewer limbs than CUs is latency bound at half the chip idle.
// Such launches (and every N = 2^16 launch) run split: cross stages as a streaming pass + sub-transforms (two workgroups per CU fit), which nearly
// halves the latency of the small launches on the critical path (tensor / ExternalProduct inverse NTTs).
inline bool split_launch(int logN, long jobs) { return logN == 16 || (logN >= 13 && jobs <= 128); }     // (at most one sub-transform workgroup per CU: 256 CUs)
// depth of the low-latency path: 0 = register-resident sub-transforms; N = 2^14: four 2^12-point LDS sub-transforms per limb, eight 2^11-point ones
// for launches that would not even give every CU one 2^12-point workgroup; N = 2^15: eight 2^12-point ones behind the radix-8 pass
inline int lds_stages(const NttShape& s, const NttSwitches& w, long jobs) {
    if (!w.ntt_lds || s.prestaged || (s.logN != 14 && s.logN != 15)) return 0;
    return s.logN == 14 && jobs < 64 ? 3 : s.logN - 12;
}
// the job walk of the H16 / H32 kernels divides by multiply-high reciprocals that are exact below 2^16
inline bool walk_ok(const NttShape& s, long limbs) { return s.nslots <= 64 && limbs < 65536 && s.nouter < 65536; }
inline void need_reg(int logn) { if (logn < 10 || logn > 15) throw std::runtime_error("mkhe: internal: an NTT launch of a shape no kernel takes"); }
}  // namespace ntt_route_detail

// one modulus class of a forward launch on the round-1 kernels and the H16 sub-transform kernels
inline NttPart ntt_fwd_class_route(const NttShape& s, const NttSwitches& w, bool small, int nslots) {
    using namespace ntt_route_detail;
    const int logN = s.logN;
    const long limbs = (long)nslots * s.nouter;
    NttPart p{};
    p.slots = small ? NS_SMALL : NS_BIG;
    p.prof = s.prestaged == 2 ? PROF_NTT14_SPLIT : s.decompose ? (small ? PROF_NTT_DECOMP : PROF_NTT_DECOMP_BIGQ) : (small ? PROF_NTT_FWD : PROF_NTT_FWD_BIGQ);
    if (s.prestaged && logN != 16) throw std::runtime_error("mkhe: internal: a prestaged launch outside N = 2^16");
    // H16 on the sub-transforms of N = 2^16 (one modulus class per launch): counted in half-limb jobs
    const bool h16_sub = w.ntt16 && !s.no_h16 && s.psi31 && nslots <= 64 && 2 * limbs >= w.ntt16_min && limbs < 65536 && s.nouter < 65536;
    if (s.prestaged == 2) {
        // both cross stages applied by the producer (decomp_spread_kernel<2>): four one-pass 2^14-point sub-transforms per limb, in place on dst or
        // from the producer's staging buffer
        if (!h16_sub) throw std::runtime_error("mkhe: internal: radix-4 prestaged launch outside the H16 path");
        push(p, NK_H14_SPLIT, 14, 2, 0, limbs << 2, !s.prestaged_oop, false);
        return p;
    }
    if (logN == 16 && !s.prestaged && w.ntt16_radix4 && h16_sub) {
        // without a fused producer (the tensor-step inputs, plain NTTs): both cross stages as ONE streaming pass, then the quarters -- instead of a
        // radix-2 pass and two-pass 2^15-point halves
        push(p, NK_PASS4_FWD, 16, s.split, 0, limbs, false, s.reduce_in != 0);
        push(p, NK_H14_SPLIT, 14, 2, 0, limbs << 2, true, false);
        return p;
    }
    if (!split_launch(logN, limbs)) {
        need_reg(logN);
        push(p, NK_FWD_REG, logN, s.split, 0, limbs << s.split, false, s.reduce_in != 0);
        return p;
    }
    const int d = lds_stages(s, w, limbs);
    if (!s.prestaged) push(p, d == 3 ? NK_PASS8_FWD : d == 2 ? NK_PASS4_FWD : NK_SPLIT_FWD, logN, s.split, 0, limbs, false, s.reduce_in != 0);
    if (d) push(p, NK_FWD_LDS, logN - d, 1, d, limbs << d, true, false);
    else if (logN == 16 && h16_sub) push(p, NK_H16_SPLIT, 15, 1, 0, limbs << 1, !(s.prestaged && s.prestaged_oop), false);
    else {
        // (the register kernels copy nothing: a producer that staged its output elsewhere needs the H16 kernel -- ntt_prestaged_on_h16 is asked first)
        if (s.prestaged && s.prestaged_oop) throw std::runtime_error("mkhe: internal: out-of-place prestaged launch outside the H16 path");
        need_reg(logN - 1);
        push(p, NK_FWD_REG, logN - 1, 1, 0, limbs << 1, true, false);
    }
    return p;
}

inline NttRoute ntt_fwd_route(const NttShape& s, const NttSwitches& w) {
    using namespace ntt_route_detail;
    NttRoute r{};
    if (s.nslots <= 0 || s.nouter <= 0) return r;
    const long limbs = (long)s.nslots * s.nouter;
    const bool whole = !s.no_h16 && s.psi31 && !s.split && !s.prestaged && walk_ok(s, limbs);
    // H32: N = 2^15 launches of several limbs per CU (whole limbs: a launch that does not deal them evenly leaves CUs idle in its last round, where
    // H16 deals half-limb jobs -- which kernel a shape takes is measured)
    const bool ok32 = w.ntt32 && whole && s.logN == 15 && s.psi31c && s.psi31b && limbs >= w.ntt32_min;
    // H16: launches that fill the chip (N = 2^14: one pass, a workgroup has loaded its whole limb before it stores, in place included)
    const bool ok16 = w.ntt16 && whole && ((s.logN == 14 && limbs >= w.ntt14_min) || (s.logN == 15 && limbs >= w.ntt16_min));
    if (ok32) {
        NttPart& p = r.part[r.nparts++];
        p.slots = NS_BIG16_SMALL16_U; p.prof = s.decompose ? PROF_NTT32_DECOMP : PROF_NTT32_FWD;
        push(p, NK_H32_FWD, 15, 0, 0, limbs, false, s.reduce_in != 0);
    }
    r.pick = ok32 && ok16 && w.ntt32 == 2;
    if (ok16 && (!ok32 || r.pick)) {
        NttPart& p = r.part[r.nparts++];
        p.slots = NS_BIG16_SMALL16; p.prof = s.decompose ? PROF_NTT16_DECOMP : PROF_NTT16_FWD;
        push(p, s.logN == 14 ? NK_H14_FWD : NK_H16_FWD, s.logN, 0, 0, limbs, false, s.reduce_in != 0);
    }
    if (r.nparts) return r;
    const unsigned long long all = s.nslots >= 64 ? ~0ull : (1ull << s.nslots) - 1;
    const int nsmall = popcount(s.small & all), nbig = s.nslots - nsmall;
    if (s.decompose && s.logN == 15 && s.reduce_in && !s.split && s.nslots <= 64 && limbs > 512 && nsmall && nbig) {
        // large Decompose launches the H16 kernels do not take: both classes in one persistent grid (no ragged tail of the big-modulus class)
        NttPart& p = r.part[r.nparts++];
        p.slots = NS_BIG_SMALL; p.prof = PROF_NTT_DECOMP_MIXED;
        push(p, NK_FWD_MIXED, 15, 0, 0, limbs, false, true);
        return r;
    }
    // one launch set per modulus class (the kernels are specialised), the big-modulus class first
    if (nbig) r.part[r.nparts++] = ntt_fwd_class_route(s, w, false, nbig);
    if (nsmall) r.part[r.nparts++] = ntt_fwd_class_route(s, w, true, nsmall);
    r.part[0].side = r.nparts == 2;
    return r;
}

// does every class part of this prestaged N = 2^16 launch run on the H16 sub-transform kernel?  (only then may the producer stage its output in
// a separate buffer, NttBatch::prestaged_oop, or apply both cross stages, prestaged = 2)
inline bool ntt_prestaged_on_h16(const NttShape& s, const NttSwitches& w) {
    if (s.logN != 16 || !s.prestaged) return false;
    const NttRoute r = ntt_fwd_route(s, w);
    for (int i = 0; i < r.nparts; ++i)
        if (r.part[i].nsteps != 1 || (r.part[i].step[0].kernel != NK_H16_SPLIT && r.part[i].step[0].kernel != NK_H14_SPLIT)) return false;
    return r.nparts > 0;
}

inline NttRoute ntt_inv_route(const NttShape& s, const NttSwitches& w) {
    using namespace ntt_route_detail;
    NttRoute r{};
    if (s.nslots <= 0 || s.nouter <= 0) return r;
    const int logN = s.logN;
    const long limbs = (long)s.nslots * s.nouter;
    NttPart& p = r.part[r.nparts++];
    p.slots = NS_AS_IS; p.prof = PROF_NTT_INV;              // (the inverse kernels take every class)
    // launches that fill the chip: one-pass 2^14-point sub-transforms on the H16-class inverse kernel (src -> dst, canonical, N^-1 folded in), then
    // the cross stages of the larger rings as one streaming pass.  N = 2^14: up to 128 limbs run as LDS sub-transforms, everything above comes
    // here (the batched evaluation of the small rings lives between 129 and 255 limbs)
    if (w.ntt16_inv && !s.no_h16 && s.psiinv31 && s.inv31c && !s.split && s.nslots <= 64 && logN >= 14 && logN <= 16 && limbs < 65536 &&
        (logN == 14 ? s.jobs >= w.ntt14_inv_min : ((long)s.jobs << (logN - 14)) >= w.ntt16_inv_min)) {
        push(p, NK_H14_INV, 14, logN - 14, 0, limbs << (logN - 14), false, false);
        if (logN == 15) push(p, NK_SPLIT_INV, 15, 0, 0, limbs, true, false);
        if (logN == 16) push(p, NK_PASS4_INV, 16, 0, 0, limbs, true, false);
        return r;
    }
    if (s.split || !split_launch(logN, s.jobs)) {
        need_reg(logN);
        push(p, NK_INV_REG, logN, s.split, 0, limbs << s.split, false, false);
        return r;
    }
    if (const int d = lds_stages(s, w, s.jobs)) {
        push(p, NK_INV_LDS, logN - d, s.split, d, limbs << d, false, false);       // (src -> dst, [0, 2q), N^-1 folded in)
        push(p, d == 3 ? NK_PASS8_INV : NK_PASS4_INV, logN, 1, 0, limbs, true, false);
        return r;
    }
    need_reg(logN - 1);
    push(p, NK_INV_REG, logN - 1, 1, 0, limbs << 1, false, false);                  // src halves -> dst halves, lazy, N^-1 folded in
    push(p, NK_SPLIT_INV, logN, 1, 0, limbs, true, false);
    return r;
}

// the slots a part takes as class masks over the slots of the launch, in the order order_slots_by_class wants them; returns how many classes
inline int ntt_part_classes(const NttShape& s, NttSlots which, unsigned long long cls[3]) {
    const unsigned long long all = s.nslots >= 64 ? ~0ull : (1ull << s.nslots) - 1;
    switch (which) {
        case NS_AS_IS: cls[0] = all; return 1;
        case NS_SMALL: cls[0] = s.small & all; return 1;
        case NS_BIG: cls[0] = ~s.small & all; return 1;
        case NS_BIG_SMALL: cls[0] = ~s.small & all; cls[1] = s.small & all; return 2;
        case NS_BIG16_SMALL16: cls[0] = ~s.small16 & all; cls[1] = s.small16 & all; return 2;
        case NS_BIG16_SMALL16_U: cls[0] = ~s.small16 & all; cls[1] = s.small16 & ~s.u & all; cls[2] = s.small16 & s.u & all; return 3;
    }
    throw std::logic_error("mkhe: internal: NTT part without a slot order");
}

}  // namespace mkhe
