"""What a collective refresh costs.  PN15QP880, four parties, uniform ciphertexts with Lin = 2 limbs, Lout = nQ, count = 1, 4, 16;
device time = HIP events on mkhe_ctx_stream around the calls; the legs of a comparison alternate in one process, WARM warm-ups, then REPS
repetitions each.  Times in microseconds: median, min, quartiles.  Recorded, not gated: no earlier code computes a wide mask or an exact lift.
  share   mkhe_refresh_share (mask_bits = 100) beside the pair mkhe_decrypt_share (62 bits) + mkhe_encrypt_seeded at the top level: unchanged
          code, and the nearest existing work (the same transforms; the pair's plaintext is a resident buffer instead of -M)
  merge   mkhe_refresh_merge of the four shares beside mkhe_decrypt_merge (the sums of step 1 alone, Lin limbs)

  python tools/refresh_timing.py [--out FILE] [--reps N]      the measurement; writes one JSON object and prints its rows
  rocprofv3 --output-format csv --kernel-trace --stats -d DIR -o p -- python tools/refresh_timing.py --kernels
          a run of its own for the kernel times: KWARM + KREPS calls of both entry points per count, nothing timed by the script
  python tools/refresh_timing.py --trace DIR [--out FILE]     reads p_kernel_trace.csv below DIR (the dispatches of the two kernels in time order,
          KWARM + KREPS per count), and adds "kernels" to FILE: median kernel time and achieved bytes/s from the byte model below
The first two need a GPU."""
import argparse
import ctypes as C
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARM, KWARM, KREPS = 5, 3, 20
COUNTS = (1, 4, 16)
LIN, MASK_BITS, FLOOD_BITS = 2, 100, 62
USERS = ["user0", "user1", "user2", "user3"]
LOGN, NQ = 15, 14


def finish_bytes(count, lin, lout, N):
    """refresh_finish_kernel: reads the product, writes the share (Lin limbs each) and the plaintext -M (Lout limbs)"""
    return 8 * N * count * (2 * lin + lout)


def merge_bytes(count, lin, lout, k, N):
    """refresh_merge_kernel: reads c_0 and k shares (Lin limbs), writes and reads back the Lin digits, reads k re-encryptions (2 Lout limbs each),
    writes the 1 + k polynomials of the output (Lout limbs each)"""
    return 8 * N * count * (lin * (1 + k) + (2 * lin if lout > lin else 0) + lout * (1 + 3 * k))


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
    def __init__(self):
        import harness as H
        from mkhe_kklss_amd import mkrlwe
        from mkhe_kklss_amd._abi import lib
        p = H.PN15QP880
        assert p["logN"] == LOGN and len(p["Q"]) == NQ
        self.mk, self.L = mkrlwe, lib()
        self.params = mkrlwe.Parameters(p["logN"], p["Q"], p["P"], 2)
        self.params.AddCRS(0, seed=1)
        self.N, self.top = self.params.N(), NQ - 1
        rng = np.random.default_rng(15)
        kgen = mkrlwe.NewKeyGenerator(self.params, mkrlwe.HostSampler())
        self.sk, self.pk = {}, {}
        for u in USERS:
            self.sk[u], self.pk[u] = kgen.GenKeyPair(u)
        self.sampler = mkrlwe.DeviceSampler()
        ks = type("K", (), dict(Q=p["Q"], N=self.N))
        n = max(COUNTS)
        self.cts = [mkrlwe.Ciphertext(self.params, USERS, LIN - 1).upload(H.uniform_ct(rng, ks, len(USERS), LIN)) for _ in range(n)]
        self.pt = mkrlwe.DeviceLimbs(self.params, n, NQ).upload(np.stack([H.uniform_poly(rng, p["Q"], self.N) for _ in range(n)]))
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

    def calls(self, count, who="user1"):
        """the four calls on `count` ciphertexts for the party `who` -> (callables by leg, the objects they write, kept alive by the caller)"""
        from mkhe_kklss_amd._abi import check, handle_array
        mk, ctx, smp = self.mk, self.params.ctx, self.sampler
        hs = handle_array([c.h for c in self.cts[:count]])
        slots = (C.c_int * count)(*[c.slot(who) for c in self.cts[:count]])
        sk, pk = self.sk[who].Value.devptr(), self.pk[who].Value.devptr()
        rs = mk.RefreshShare(self.params, who, LIN - 1, self.top, count)
        re = handle_array([c.h for c in rs.Reenc])
        plain = mk.DeviceLimbs(self.params, count, LIN)
        encs = mk.batch_ciphertexts(mk.Ciphertext, self.params, [who], self.top, count)
        eh = handle_array([c.h for c in encs])

        def refresh_share():
            key, nm, ne = smp.refresh_args()
            check(self.L.mkhe_refresh_share(ctx, count, hs, slots, sk, pk, key, nm, ne, MASK_BITS, smp._cdt, len(smp.cdt), rs.Share.Value.devptr(), re))

        def pair():
            check(self.L.mkhe_decrypt_share(ctx, count, hs, slots, sk, *smp.share_args(), FLOOD_BITS, plain.devptr()))
            check(self.L.mkhe_encrypt_seeded(ctx, self.top, count, pk, self.pt.devptr(), 0, *smp.encrypt_args(), eh))
        return dict(pair=pair, refresh_share=refresh_share), (rs, plain, encs, hs, slots, re, eh)

    def merges(self, count):
        from mkhe_kklss_amd._abi import check, handle_array
        mk, ctx = self.mk, self.params.ctx
        shares = []
        for u in USERS:
            legs, keep = self.calls(count, u)
            legs["refresh_share"]()
            shares.append(keep[0])
        hs = handle_array([c.h for c in self.cts[:count]])
        sh = handle_array([s.Share.Value.devptr() for s in shares])
        re = handle_array([c.h for s in shares for c in s.Reenc])
        outs = mk.batch_ciphertexts(mk.Ciphertext, self.params, USERS, self.top, count)
        oh = handle_array([c.h for c in outs])
        pt = mk.DeviceLimbs(self.params, count, LIN)
        return dict(decrypt_merge=lambda: check(self.L.mkhe_decrypt_merge(ctx, count, hs, len(USERS), sh, pt.devptr())),
                    refresh_merge=lambda: check(self.L.mkhe_refresh_merge(ctx, count, hs, len(USERS), sh, re, oh))), (shares, outs, pt, hs, sh, re, oh)

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
    s = Setup()
    rows = []
    for count in COUNTS:
        legs, keep = s.calls(count)
        a = s.alternate(legs, reps)
        legs, keep2 = s.merges(count)
        b = s.alternate(legs, reps)
        rows.append(dict(ring="PN15QP880", logN=LOGN, parties=len(USERS), lin=LIN, lout=NQ, count=count, mask_bits=MASK_BITS, reps=reps,
                         decrypt_share_plus_encrypt_seeded=a["pair"], refresh_share=a["refresh_share"],
                         share_ratio=round(a["refresh_share"]["median_us"] / a["pair"]["median_us"], 3),
                         decrypt_merge=b["decrypt_merge"], refresh_merge=b["refresh_merge"]))
        print(json.dumps(rows[-1]), flush=True)
    s.close()
    return dict(legs=dict(pair="mkhe_decrypt_share (62 bits, Lin limbs) + mkhe_encrypt_seeded (top level) of count items, two calls",
                          refresh_share="one mkhe_refresh_share of count ciphertexts, mask_bits = 100, Lin = 2, Lout = 14",
                          decrypt_merge="mkhe_decrypt_merge of four shares (Lin limbs)", refresh_merge="mkhe_refresh_merge of four shares, Lin = 2 -> Lout = 14"),
                rows=rows)


def kernels():
    """the calls only, for a kernel trace: per count KWARM + KREPS shares (party user1) and as many merges"""
    s = Setup()
    for count in COUNTS:
        legs, keep = s.calls(count)
        mlegs, keep2 = s.merges(count)                # (one share per party: four finish dispatches in front of this count's series, dropped by --trace)
        for _ in range(KWARM + KREPS):
            legs["refresh_share"]()
        for _ in range(KWARM + KREPS):
            mlegs["refresh_merge"]()
        s.params.sync()
    s.close()


def trace(directory, out):
    f = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if not f:
        raise SystemExit("no kernel trace below " + directory)
    rows = sorted(csv.DictReader(open(f[0])), key=lambda r: int(r["Start_Timestamp"]))
    res = json.load(open(out)) if os.path.exists(out) else {}
    N, k, kern = 1 << LOGN, len(USERS), {}
    for name, per_count_extra, model in (("refresh_finish_kernel", k, lambda c: finish_bytes(c, LIN, NQ, N)),
                                         ("refresh_merge_kernel", 0, lambda c: merge_bytes(c, LIN, NQ, k, N))):
        t = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
        per = per_count_extra + KWARM + KREPS
        if len(t) != per * len(COUNTS):
            raise SystemExit("%s: %d dispatches in the trace, %d expected" % (name, len(t), per * len(COUNTS)))
        kern[name] = []
        for i, count in enumerate(COUNTS):
            us = t[i * per + per_count_extra + KWARM: (i + 1) * per]
            med = float(np.median(us))
            kern[name].append(dict(count=count, dispatches=len(us), median_us=round(med, 2), min_us=round(min(us), 2), model_bytes=model(count),
                                   achieved_GBps=round(model(count) / med / 1e3, 1)))
            print(name, json.dumps(kern[name][-1]), flush=True)
    res["kernels"] = dict(source="rocprofv3 --kernel-trace --stats, a run of its own (tools/refresh_timing.py --kernels)", **kern)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refresh_timing.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--trace")
    args = ap.parse_args()
    if args.kernels:
        return kernels()
    if args.reps < 20:
        raise SystemExit("at least 20 repetitions")
    res = trace(args.trace, args.out) if args.trace else measure(args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
