"""What a collective key switch to a recipient's public key costs.  PN15QP880 (mkckks context, N = 2^15, 14 limbs), 4 parties,
count = 1 and 16, uniform ciphertexts at the maximum level.  Device time = HIP events on mkhe_ctx_stream around the calls; the legs of a
comparison alternate in one process, WARM warm-ups, then REPS repetitions each.  Times in microseconds: median, min, quartiles.  Recorded, not
gated.
  share   mkhe_pcks_share of the party user1 (flood_bits = 62, and the widest flood the ring takes) beside the composition a user had before it:
          mkhe_decrypt_share (flood_bits = 62) plus mkhe_encrypt_seeded of count zero plaintexts under the recipient's key.  (The composition
          still lacks the addition of the two on the host, and leaves an e0 beside the flood.)
  merge   mkhe_pcks_merge of all shares beside mkhe_decrypt_merge of as many shares: twice the rows.

  python tools/pcks_timing.py [--out FILE] [--reps N]
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
COUNTS = (1, 16)
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
    def __init__(self, pset):
        import harness as H
        from mkhe_kklss_amd import mkckks, mkrlwe
        from mkhe_kklss_amd._abi import lib
        self.mk, self.ck, self.L, self.H = mkrlwe, mkckks, lib(), H
        self.pset, self.nq = pset, len(pset["Q"])
        self.params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], pset["scale"])
        self.params.AddCRS(0, seed=1)
        self.N = self.params.N()
        self.rng = np.random.default_rng(16)
        kgen = mkrlwe.NewKeyGenerator(self.params, mkrlwe.HostSampler())
        self.sk, self.pk = {}, {}
        for u in USERS + ["carol"]:
            self.sk[u], self.pk[u] = kgen.GenKeyPair(u)
        self.sampler = mkrlwe.DeviceSampler()
        self.sw = mkckks.NewPublicKeySwitcher(self.params)
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

    def ciphertexts(self, count):
        ks = type("K", (), dict(Q=self.pset["Q"], N=self.N))
        return [self.ck.NewCiphertext(self.params, USERS, self.nq - 1, self.pset["scale"]).upload(self.H.uniform_ct(self.rng, ks, len(USERS), self.nq))
                for _ in range(count)]

    def share_calls(self, cts, who, widths):
        """-> (legs, the PublicKeySwitchShare of the first width, whatever has to stay alive)"""
        from mkhe_kklss_amd._abi import check, handle_array
        count, smp, ctx, top = len(cts), self.sampler, self.params.ctx, self.nq - 1
        hs = handle_array([c.h for c in cts])
        slots = (C.c_int * count)(*[c.slot(who) for c in cts])
        sk, pk = self.sk[who].Value.devptr(), self.pk["carol"].Value.devptr()
        outs = {w: self.mk.PublicKeySwitchShare(self.params, who, top, count) for w in widths}
        plain = self.mk.DecryptionShare(self.params, who, top, count)
        zero = self.mk.DeviceLimbs(self.params, count, self.nq).upload(np.zeros((count, self.nq, self.N), dtype=np.uint64))
        enc = self.mk.batch_ciphertexts(self.mk.Ciphertext, self.params, ["carol"], top, count)
        eh = handle_array([c.h for c in enc])

        def pcks(w):
            def call():
                key, nonce, cdt, ncdt = smp.switch_args()
                check(self.L.mkhe_pcks_share(ctx, count, hs, slots, sk, pk, key, nonce, w, cdt, ncdt, outs[w].Value.devptr()))
            return call

        def composition():
            key, nonce = smp.share_args()
            check(self.L.mkhe_decrypt_share(ctx, count, hs, slots, sk, key, nonce, 62, plain.Value.devptr()))
            check(self.L.mkhe_encrypt_seeded(ctx, top, count, pk, zero.devptr(), 0, *smp.encrypt_args(), eh))
        legs = {"composition": composition}
        legs.update({"pcks_share_%d" % w: pcks(w) for w in widths})
        return legs, outs[widths[0]], (hs, slots, outs, plain, zero, enc, eh)

    def merge_calls(self, cts, shares):
        from mkhe_kklss_amd._abi import check, handle_array
        ctx, count, k = self.params.ctx, len(cts), len(shares)
        hs = handle_array([c.h for c in cts])
        sh = handle_array([s.Value.devptr() for s in shares])
        outs = self.mk.batch_ciphertexts(self.ck.Ciphertext, self.params, ["carol"], self.nq - 1, count)
        oh = handle_array([c.h for c in outs])
        halves = [self.mk.DeviceLimbs(self.params, count, self.nq).upload(s.download()[:, 0].copy()) for s in shares]
        dh = handle_array([h.devptr() for h in halves])
        pt = self.mk.DeviceLimbs(self.params, count, self.nq)
        legs = dict(decrypt_merge=lambda: check(self.L.mkhe_decrypt_merge(ctx, count, hs, k, dh, pt.devptr())),
                    pcks_merge=lambda: check(self.L.mkhe_pcks_merge(ctx, count, hs, k, sh, oh)))
        return legs, (outs, pt), (hs, sh, oh, halves, dh)

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
    import harness as H
    pset = H.PN15QP880
    s = Setup(pset)
    widths = (62, s.sw.MaxFloodBits())
    rows = []
    for count in COUNTS:
        cts = s.ciphertexts(count)
        legs, _, keep = s.share_calls(cts, "user1", widths)
        a = s.alternate(legs, reps)
        shares = []
        for u in USERS:
            one, sh, keep_u = s.share_calls(cts, u, widths[:1])
            one["pcks_share_%d" % widths[0]]()
            shares.append(sh)
        legs, (outs, pt), keep2 = s.merge_calls(cts, shares)
        b = s.alternate(legs, reps)
        same = all((o.download()[0] == p).all() for o, p in zip(outs, pt.download()))      # polynomial 0 of the merge is mkhe_decrypt_merge's sum
        fused = a["pcks_share_%d" % widths[0]]
        rows.append(dict(ring="PN15QP880", logN=pset["logN"], nq=s.nq, parties=len(USERS), count=count, reps=reps, flood_bits=list(widths),
                         share=dict(composition=a["composition"], **{k: v for k, v in a.items() if k != "composition"}),
                         share_ratio=round(fused["median_us"] / a["composition"]["median_us"], 3),
                         decrypt_merge=b["decrypt_merge"], pcks_merge=b["pcks_merge"],
                         merge_ratio=round(b["pcks_merge"]["median_us"] / b["decrypt_merge"]["median_us"], 3), same_bits=bool(same)))
        print(json.dumps(rows[-1]), flush=True)
    s.close()
    return dict(legs=dict(composition="mkhe_decrypt_share (flood_bits = 62) + mkhe_encrypt_seeded of count zero plaintexts under the recipient's key",
                          pcks_share="one mkhe_pcks_share of count ciphertexts for one party, at flood_bits = 62 and at the widest flood of the ring",
                          decrypt_merge="one mkhe_decrypt_merge of the first halves of all shares", pcks_merge="one mkhe_pcks_merge of all shares"),
                rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcks_timing.json"))
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
