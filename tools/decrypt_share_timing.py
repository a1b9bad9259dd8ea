"""What a decryption share and its merge cost.  PN15QP880 at the top level, four parties, uniform ciphertexts; device time =
HIP events on mkhe_ctx_stream around the calls; the legs of a comparison alternate in one process, WARM warm-ups, then REPS repetitions each.
Times in microseconds: median, min, quartiles.
  share   mkhe_decrypt_share of count = 1, 4, 16 ciphertexts with flood_bits = 40 (one call) against count calls of mkhe_partial_decrypt: the
          same transforms in fewer launches, and no copy of the other party polynomials
  merge   mkhe_decrypt_merge of the four shares of one ciphertext against mkhe_decrypt (four keys in one place), for scale

  python tools/decrypt_share_timing.py [--out FILE] [--reps N]     the measurement; writes one JSON object and prints its rows
  MKHE_LIB=.../libmkhe_hip_switches.so python tools/decrypt_share_timing.py --split [--out FILE]
          the limb split of share_finish_kernel: MKHE_SHARE_ROWS = 1 (one thread walks all limbs) against the number of limbs (one limb per grid
          row), the same call alternating; adds "limb_split" to FILE.  Needs the -DMKHE_SWITCHES build: the product library does not read the variable.
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
COUNTS = (1, 4, 16)
BITS = 40
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
    def __init__(self):
        import harness as H
        from mkhe_kklss_amd import mkrlwe
        from mkhe_kklss_amd._abi import lib
        p = H.PN15QP880
        self.mk, self.L = mkrlwe, lib()
        self.params = mkrlwe.Parameters(p["logN"], p["Q"], p["P"], 2)
        self.N, self.level = self.params.N(), len(p["Q"]) - 1
        rng = np.random.default_rng(15)
        kgen = mkrlwe.NewKeyGenerator(self.params, mkrlwe.HostSampler())
        self.sk = {u: kgen.GenSecretKey(u) for u in USERS}
        self.sampler = mkrlwe.DeviceSampler()
        ks = type("K", (), dict(Q=p["Q"], N=self.N))
        self.cts = [mkrlwe.Ciphertext(self.params, USERS, self.level).upload(H.uniform_ct(rng, ks, len(USERS), self.level + 1)) for _ in range(max(COUNTS))]
        self.rest = [mkrlwe.Ciphertext(self.params, [u for u in USERS if u != "user1"], self.level) for _ in range(max(COUNTS))]
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

    def share_call(self, count, who="user1", out=None):
        from mkhe_kklss_amd._abi import check, handle_array
        out = out or self.mk.DeviceLimbs(self.params, count, self.level + 1)
        hs = handle_array([c.h for c in self.cts[:count]])
        slots = (C.c_int * count)(*[c.slot(who) for c in self.cts[:count]])
        sk = self.sk[who].Value.devptr()
        f = lambda: check(self.L.mkhe_decrypt_share(self.params.ctx, count, hs, slots, sk, *self.sampler.share_args(), BITS, out.devptr()))
        return f, (out, hs, slots)

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
    from mkhe_kklss_amd._abi import check, handle_array
    s = Setup()
    rows = []
    for count in COUNTS:
        share, keep = s.share_call(count)
        sk, slot = s.sk["user1"].Value.devptr(), s.cts[0].slot("user1")

        def partial():
            for c, o in zip(s.cts[:count], s.rest[:count]):
                check(s.L.mkhe_partial_decrypt(s.params.ctx, c.h, slot, sk, o.h))
        st = s.alternate(dict(partial=partial, share=share), reps)
        a, b = st["partial"], st["share"]
        iqr = round(a["q3_us"] - a["q1_us"], 1)
        rows.append(dict(ring="PN15QP880", logN=15, limbs=s.level + 1, parties=len(USERS), count=count, flood_bits=BITS, reps=reps,
                         partial_decrypt_calls=a, decrypt_share=b, ratio=round(b["median_us"] / a["median_us"], 3), partial_iqr_us=iqr,
                         share_within_partial_iqr=bool(b["median_us"] <= a["median_us"] + iqr)))
        print(json.dumps(rows[-1]), flush=True)
    # the merge against Decrypt, one ciphertext
    ct = s.cts[0]
    shares = []
    for u in USERS:
        f, keep = s.share_call(1, u)
        f()
        shares.append(keep[0])
    pt, pt2 = s.mk.DeviceLimbs(s.params, 1, s.level + 1), s.mk.DeviceLimbs(s.params, 1, s.level + 1)
    hs, sh = handle_array([ct.h]), handle_array([x.devptr() for x in shares])
    sks = handle_array([s.sk[u].Value.devptr() for u in USERS])
    st = s.alternate(dict(decrypt=lambda: check(s.L.mkhe_decrypt(s.params.ctx, ct.h, sks, pt.devptr())),
                          merge=lambda: check(s.L.mkhe_decrypt_merge(s.params.ctx, 1, hs, len(USERS), sh, pt2.devptr()))), reps)
    merge = dict(ring="PN15QP880", parties=len(USERS), count=1, reps=reps, decrypt=st["decrypt"], decrypt_merge=st["merge"])
    print(json.dumps(merge), flush=True)
    s.close()
    return dict(legs=dict(partial="count calls of mkhe_partial_decrypt (party at slot 2 of 4)", share="one mkhe_decrypt_share of count ciphertexts, flood_bits = 40",
                          decrypt="mkhe_decrypt with the four keys", merge="mkhe_decrypt_merge of four shares"), rows=rows, merge=merge)


def split(reps, out):
    if "switches" not in os.environ.get("MKHE_LIB", ""):
        raise SystemExit("--split needs MKHE_LIB=.../libmkhe_hip_switches.so (the product library does not read MKHE_SHARE_ROWS)")
    s = Setup()
    rows = []
    for count in COUNTS:
        share, keep = s.share_call(count)

        def leg(rows_):
            def f():
                os.environ["MKHE_SHARE_ROWS"] = str(rows_)
                share()
            return f
        st = s.alternate(dict(all_limbs_per_thread=leg(1), one_limb_per_row=leg(s.level + 1)), reps)
        rows.append(dict(count=count, limbs=s.level + 1, **st))
        print(json.dumps(rows[-1]), flush=True)
    os.environ.pop("MKHE_SHARE_ROWS", None)
    s.close()
    res = json.load(open(out)) if os.path.exists(out) else {}
    res["limb_split"] = dict(what="mkhe_decrypt_share, whole call, MKHE_SHARE_ROWS = 1 against the number of limbs (-DMKHE_SWITCHES build)", rows=rows)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decrypt_share_timing.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--split", action="store_true")
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("at least 20 repetitions")
    res = split(args.reps, args.out) if args.split else measure(args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
