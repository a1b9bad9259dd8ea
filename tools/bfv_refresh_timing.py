"""What a collective refresh of MK-BFV costs.  BFV_PN14QP439 and BFV_PN15QP880, 2 and 4 parties, count = 1 and 8, uniform
ciphertexts; flood_bits = 62 and the ring's MaxFloodBits(parties).  Device time = HIP events on mkhe_ctx_stream around the calls; the legs of a
comparison alternate in one process, WARM warm-ups, then REPS repetitions each.  Times in microseconds: median, min, quartiles.  Recorded,
not gated.
  share   mkhe_bfv_refresh_share of the party user1 at both flood widths
  merge   mkhe_bfv_refresh_merge of all shares beside the composition it replaces, made of calls older than it: mkhe_decrypt_merge,
          mkhe_bfv_scale_down, mkhe_bfv_scale_up, then the additions -- per item parties - 1 mkhe_ct_add that sum the re-encryptions, and
          one mkhe_bfv_ct_add_ptxt of the batch that adds up(w) to polynomial 0.  The same outputs, bit for bit (checked once per row).

  python tools/bfv_refresh_timing.py [--out FILE] [--reps N]
Needs a GPU."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARM = 5
COUNTS = (1, 8)
PARTIES = (2, 4)
USERS = ["user0", "user1", "user2", "user3"]


def hip_runtime():
    """the HIP runtime the engine library is linked to, as loaded in this process"""
    from mkhe_kklss_amd._abi import lib
    lib()
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime in this process")


def stat(t):
    return dict(median_us=round(float(np.median(t)), 1), min_us=round(float(min(t)), 1), q1_us=round(float(np.percentile(t, 25)), 1),
                q3_us=round(float(np.percentile(t, 75)), 1))


class Setup:
    def __init__(self, name, pset):
        import harness as H
        from mkhe_kklss_amd import mkbfv, mkrlwe
        from mkhe_kklss_amd._abi import lib
        self.name, self.mk, self.bfv, self.L, self.H = name, mkrlwe, mkbfv, lib(), H
        self.pset, self.nq = pset, len(pset["Q"])
        self.params = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], pset["T"])
        self.params.AddCRS(0, seed=1)
        self.N = self.params.N()
        self.rng = np.random.default_rng(15)
        kgen = mkbfv.NewKeyGenerator(self.params, mkrlwe.HostSampler())
        self.sk, self.pk = {}, {}
        for u in USERS:
            self.sk[u], self.pk[u] = kgen.GenKeyPair(u)
        self.sampler = mkrlwe.DeviceSampler()
        self.ref = mkbfv.NewRefresher(self.params)
        self.hip = hip_runtime()
        self.stream = C.c_void_p(self.params.stream())
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        for e in (self.e0, self.e1):
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def device_us(self, f):
        assert self.hip.hipEventRecord(self.e0, self.stream) == 0
        f()
        assert self.hip.hipEventRecord(self.e1, self.stream) == 0 and self.hip.hipEventSynchronize(self.e1) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.e0, self.e1) == 0
        return ms.value * 1e3

    def ciphertexts(self, users, count):
        ks = type("K", (), dict(Q=self.pset["Q"], N=self.N))
        return [self.bfv.Ciphertext(self.params, users).upload(self.H.uniform_ct(self.rng, ks, len(users), self.nq)) for _ in range(count)]

    def share_call(self, cts, who, flood_bits):
        """-> (the call, the RefreshShare it writes)"""
        from mkhe_kklss_amd._abi import check, handle_array
        count, smp, top = len(cts), self.sampler, self.nq - 1
        hs = handle_array([c.h for c in cts])
        slots = (C.c_int * count)(*[c.slot(who) for c in cts])
        rs = self.mk.RefreshShare(self.params, who, top, top, count)
        re = handle_array([c.h for c in rs.Reenc])

        def call():
            key, nm, ne = smp.refresh_args()
            check(self.L.mkhe_bfv_refresh_share(self.params.ctx, count, hs, slots, self.sk[who].Value.devptr(), self.pk[who].Value.devptr(), key, nm, ne, 1,
                                                flood_bits, smp._cdt, len(smp.cdt), rs.Share.Value.devptr(), re))
        call.keep = (hs, slots, re)
        return call, rs

    def merge_calls(self, cts, shares):
        """-> (legs, the outputs of the two legs, whatever has to stay alive)"""
        from mkhe_kklss_amd._abi import check, handle_array
        mk, ctx, count, users, k = self.mk, self.params.ctx, len(cts), cts[0].ids, len(shares)
        hs = handle_array([c.h for c in cts])
        sh = handle_array([s.Share.Value.devptr() for s in shares])
        re = handle_array([c.h for s in shares for c in s.Reenc])
        outs = mk.batch_ciphertexts(self.bfv.Ciphertext, self.params, users, self.nq - 1, count)
        oh = handle_array([c.h for c in outs])
        pt, coeffs, up = mk.DeviceLimbs(self.params, count, self.nq), mk.DeviceLimbs(self.params, count, 1), mk.DeviceLimbs(self.params, count, self.nq)
        # the partial sums of the re-encryptions: over the first 2, 3 .. k parties
        sums = [mk.batch_ciphertexts(self.bfv.Ciphertext, self.params, users[: i + 1], self.nq - 1, count) for i in range(1, k)]
        last = handle_array([c.h for c in sums[-1]])
        comp = mk.batch_ciphertexts(self.bfv.Ciphertext, self.params, users, self.nq - 1, count)
        ch = handle_array([c.h for c in comp])

        def composition():
            check(self.L.mkhe_decrypt_merge(ctx, count, hs, k, sh, pt.devptr()))
            check(self.L.mkhe_bfv_scale_down(ctx, count, pt.devptr(), coeffs.devptr()))
            check(self.L.mkhe_bfv_scale_up(ctx, count, coeffs.devptr(), up.devptr()))
            for b in range(count):
                acc = shares[0].Reenc[b]
                for i in range(1, k):
                    check(self.L.mkhe_ct_add(ctx, acc.h, shares[i].Reenc[b].h, sums[i - 1][b].h))
                    acc = sums[i - 1][b]
            check(self.L.mkhe_bfv_ct_add_ptxt(ctx, 0, count, last, up.devptr(), self.nq * self.N, ch))
        legs = dict(composition=composition, refresh_merge=lambda: check(self.L.mkhe_bfv_refresh_merge(ctx, count, hs, k, sh, re, oh)))
        return legs, (outs, comp), (hs, sh, re, oh, pt, coeffs, up, sums, last, ch)

    def alternate(self, legs, reps):
        """legs: name -> callable; every repetition runs each leg once, in turn"""
        for _ in range(WARM):
            for f in legs.values():
                self.device_us(f)
        t = {k: [] for k in legs}
        for _ in range(reps):
            for k, f in legs.items():
                t[k].append(self.device_us(f))
        return {k: stat(v) for k, v in t.items()}

    def close(self):
        for e in (self.e0, self.e1):
            self.hip.hipEventDestroy(e)
        self.params.close()


def measure(reps):
    import harness_bfv as HB
    rows = []
    for name, pset in (("BFV_PN14QP439", HB.BFV_PN14QP439), ("BFV_PN15QP880", HB.BFV_PN15QP880)):
        s = Setup(name, pset)
        for parties in PARTIES:
            users = USERS[:parties]
            widths = (62, s.ref.MaxFloodBits(parties))
            for count in COUNTS:
                cts = s.ciphertexts(users, count)
                calls = {w: s.share_call(cts, "user1", w) for w in widths}
                a = s.alternate({"flood_%d" % w: c for w, (c, _) in calls.items()}, reps)
                shares = []
                for u in users:
                    call, rs = s.share_call(cts, u, widths[1])
                    call()
                    shares.append(rs)
                legs, (outs, comp), keep = s.merge_calls(cts, shares)
                b = s.alternate(legs, reps)
                same = all((x.download() == y.download()).all() for x, y in zip(outs, comp))
                rows.append(dict(ring=name, logN=pset["logN"], nq=s.nq, parties=parties, count=count, reps=reps, flood_bits=list(widths),
                                 share={"flood_%d" % w: a["flood_%d" % w] for w in widths}, composition=b["composition"], refresh_merge=b["refresh_merge"],
                                 merge_ratio=round(b["refresh_merge"]["median_us"] / b["composition"]["median_us"], 3), same_bits=bool(same)))
                print(json.dumps(rows[-1]), flush=True)
        s.close()
    return dict(legs=dict(share="one mkhe_bfv_refresh_share of count ciphertexts for one party, mask = 1, at flood_bits = 62 and at MaxFloodBits(parties)",
                          composition="mkhe_decrypt_merge + mkhe_bfv_scale_down + mkhe_bfv_scale_up + count * (parties - 1) mkhe_ct_add + one mkhe_bfv_ct_add_ptxt",
                          refresh_merge="one mkhe_bfv_refresh_merge of all shares"),
                rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bfv_refresh_timing.json"))
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("at least 20 repetitions")
    res = measure(args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
