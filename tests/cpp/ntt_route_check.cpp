// Prints the route (csrc/ntt_route.h) of one launch shape per line, on both sides of every size threshold the NTT dispatch has;
// tests/test_ntt_route_host.py holds the expected text.  Host C++ only: no HIP header, no library.
#include <cstdio>
#include <string>

#include "ntt_route.h"

using namespace mkhe;

static const char* kernel_name(NttKernel k) {
    switch (k) {
        case NK_FWD_REG: return "fwd_reg"; case NK_FWD_MIXED: return "fwd_mixed"; case NK_SPLIT_FWD: return "split_fwd"; case NK_PASS4_FWD: return "pass4_fwd";
        case NK_PASS8_FWD: return "pass8_fwd"; case NK_FWD_LDS: return "fwd_lds"; case NK_H16_FWD: return "h16_fwd"; case NK_H14_FWD: return "h14_fwd";
        case NK_H16_SPLIT: return "h16_split"; case NK_H14_SPLIT: return "h14_split"; case NK_H32_FWD: return "h32_fwd"; case NK_INV_REG: return "inv_reg";
        case NK_SPLIT_INV: return "split_inv"; case NK_PASS4_INV: return "pass4_inv"; case NK_PASS8_INV: return "pass8_inv"; case NK_INV_LDS: return "inv_lds";
        case NK_H14_INV: return "h14_inv";
    }
    return "?";
}
static const char* prof_name(int p) {
    static const char* names[PROF_NTT_CLASSES] = {"decomp", "decomp_bigq", "decomp_mixed", "h16_decomp", "h16_fwd", "h32_decomp", "h32_fwd", "h14_split", "fwd", "fwd_bigq", "inv"};
    return p >= 0 && p < PROF_NTT_CLASSES ? names[p] : "?";
}
static const char* slots_name(NttSlots s) {
    switch (s) {
        case NS_AS_IS: return "all"; case NS_SMALL: return "small"; case NS_BIG: return "big"; case NS_BIG_SMALL: return "big+small";
        case NS_BIG16_SMALL16: return "big16+small16"; case NS_BIG16_SMALL16_U: return "big16+small16+u";
    }
    return "?";
}
static std::string text(const NttRoute& r) {
    std::string o = r.pick ? "pick{h32|h16}" : "";
    if (!r.nparts) o += "nothing";
    for (int i = 0; i < r.nparts; ++i) {
        const NttPart& p = r.part[i];
        o += std::string(o.empty() ? "" : " ") + "[" + slots_name(p.slots) + " " + prof_name(p.prof) + (p.side ? " side" : "") + ":";
        for (int k = 0; k < p.nsteps; ++k) {
            const NttStep& s = p.step[k];
            char buf[128];
            snprintf(buf, sizeof buf, " %s%s(2^%d split=%d", kernel_name(s.kernel), s.dec ? "<dec>" : "", s.logn, s.split);
            o += buf;
            if (s.depth) { snprintf(buf, sizeof buf, " depth=%d", s.depth); o += buf; }
            snprintf(buf, sizeof buf, " jobs=%d %s)", s.jobs, s.in_place ? "in-place" : "src->dst");
            o += buf;
        }
        o += "]";
    }
    return o;
}

// one small-class modulus per launch unless `small` says otherwise: the limb count is the class's count
static NttShape shape(int logN, int nslots, int nouter, unsigned long long small = ~0ull) {
    NttShape s;
    s.logN = logN; s.nslots = nslots; s.nouter = nouter; s.jobs = nslots * nouter;
    s.small = s.small16 = small;
    s.psi31 = s.psi31b = s.psi31c = s.psiinv31 = s.inv31c = true;
    return s;
}
static void row(const char* label, bool inverse, const NttShape& s, const NttSwitches& w = NttSwitches()) {
    try { printf("%s: %s\n", label, text(inverse ? ntt_inv_route(s, w) : ntt_fwd_route(s, w)).c_str()); }
    catch (const std::exception& e) { printf("%s: throws %s\n", label, e.what()); }
}

int main() {
    char label[96];
    const int fwd[][2] = {{13, 128}, {13, 129}, {14, 63}, {14, 64}, {14, 127}, {14, 128}, {14, 129}, {15, 127}, {15, 128}, {15, 511}, {15, 512}, {16, 63}, {16, 64}};
    for (const auto& c : fwd) { snprintf(label, sizeof label, "fwd 2^%d limbs=%d", c[0], c[1]); row(label, false, shape(c[0], 1, c[1])); }
    {
        NttShape big = shape(15, 1, 127, 0); row("fwd 2^15 limbs=127 big-modulus class", false, big);
        for (int n : {63, 64}) {
            NttShape s = shape(16, 1, n);
            s.prestaged = 1; snprintf(label, sizeof label, "fwd 2^16 limbs=%d prestaged=1", n); row(label, false, s);
            printf("  prestaged launch on the H16 sub-transform kernel: %s\n", ntt_prestaged_on_h16(s, NttSwitches()) ? "yes" : "no");
            s.prestaged_oop = 1; snprintf(label, sizeof label, "fwd 2^16 limbs=%d prestaged=1 out of place", n); row(label, false, s);
            s.prestaged = 2; s.prestaged_oop = 0; snprintf(label, sizeof label, "fwd 2^16 limbs=%d prestaged=2", n); row(label, false, s);
        }
        // Decompose launches (reduce_in): both kernels qualify -> measured; the job walk's caps; contexts without the H16 tables
        NttShape d = shape(15, 16, 56, 0xfffeull); d.decompose = true; d.reduce_in = 1; row("decompose 2^15 16 slots x 56", false, d);
        d = shape(14, 8, 24, 0xfeull); d.decompose = true; d.reduce_in = 1; row("decompose 2^14 8 slots x 24", false, d);
        row("fwd 2^15 1 slot x 65535", false, shape(15, 1, 65535));
        row("fwd 2^15 1 slot x 65536 (nouter cap)", false, shape(15, 1, 65536));
        row("fwd 2^15 2 slots x 32768 (limb cap)", false, shape(15, 2, 32768));
        row("fwd 2^14 2 slots x 32768 (limb cap)", false, shape(14, 2, 32768));
        row("fwd 2^16 2 slots x 32768 (limb cap)", false, shape(16, 2, 32768));
        for (int n : {128, 129}) {
            d = shape(15, 4, n, 0xeull); d.decompose = true; d.reduce_in = 1; d.no_h16 = true; d.psi31 = d.psi31b = d.psi31c = false;
            snprintf(label, sizeof label, "decompose 2^15 no_h16 1 big + 3 small slots x %d", n); row(label, false, d);
        }
        d = shape(15, 4, 129); d.decompose = true; d.reduce_in = 1; d.no_h16 = true; d.psi31 = d.psi31b = d.psi31c = false;
        row("decompose 2^15 no_h16 4 small slots x 129", false, d);
        d = shape(16, 1, 64); d.no_h16 = true; d.psi31 = false; row("fwd 2^16 limbs=64 no_h16", false, d);
    }
    const int inv[][2] = {{13, 128}, {13, 129}, {14, 63}, {14, 64}, {14, 128}, {14, 129}, {15, 127}, {15, 128}, {16, 63}, {16, 64}};
    for (const auto& c : inv) { snprintf(label, sizeof label, "inv 2^%d limbs=%d", c[0], c[1]); row(label, true, shape(c[0], 1, c[1])); }
    {
        NttShape v = shape(14, 8, 20); v.vi = 1;
        v.jobs = 128; row("inv 2^14 merged 8 slots x 20, 128 jobs", true, v);
        v.jobs = 129; row("inv 2^14 merged 8 slots x 20, 129 jobs", true, v);
        row("inv 2^14 2 slots x 32768 (limb cap)", true, shape(14, 2, 32768));
        NttShape n = shape(15, 1, 128); n.no_h16 = true; n.psiinv31 = false; row("inv 2^15 limbs=128 no_h16", true, n);
    }
    NttSwitches one;       // what tests/test_gpu_forced_paths.py sets
    one.ntt16_min = one.ntt14_min = one.ntt16_inv_min = 1;
    for (int logN : {14, 15, 16}) {
        snprintf(label, sizeof label, "thresholds at 1: fwd 2^%d limbs=1", logN); row(label, false, shape(logN, 1, 1), one);
        snprintf(label, sizeof label, "thresholds at 1: inv 2^%d limbs=1", logN); row(label, true, shape(logN, 1, 1), one);
    }
    return 0;
}
