"""What secret-key encryption with a seeded c1 costs.  PN15QP880 (mkckks context, N = 2^15, 14 limbs), count = 1 and 16, uniform
plaintexts at the maximum level.  Device time = HIP events on mkhe_ctx_stream around the calls; the legs of a comparison alternate in one process,
WARM warm-ups, then REPS repetitions each.  Times in microseconds: median, min, quartiles.  Recorded, not gated.
  encrypt  mkhe_encrypt_sk_seeded beside mkhe_encrypt_seeded (the public-key form) of the same plaintexts.
  expand   mkhe_ct_expand_seeded of count ciphertexts beside what it replaces on the receiver: mkhe_ct_upload_poly_limbs of polynomial 1 of each
           from PINNED host memory (the events span the copies; the call waits for them itself).
  sampler  mkhe_sample_uniform alone: bytes written per second, beside the 5.8 TB/s the streaming kernels of this project reach
           (profiles/README.md).

  python tools/sk_encrypt_timing.py [--out FILE] [--reps N]
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
STREAMING_TBS = 5.8
ME = "user0"


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
        from mkhe_kklss_amd import mkckks, mkrlwe
        from mkhe_kklss_amd._abi import lib
        self.mk, self.L = mkrlwe, lib()
        self.pset, self.nq = pset, len(pset["Q"])
        self.params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], pset["scale"])
        self.params.AddCRS(0, seed=1)
        self.N = self.params.N()
        self.rng = np.random.default_rng(17)
        self.sk, self.pk = mkrlwe.NewKeyGenerator(self.params, mkrlwe.HostSampler()).GenKeyPair(ME)
        self.sampler = mkrlwe.DeviceSampler()
        self.seed = (C.c_uint32 * 8)(*[int(x) for x in np.frombuffer(os.urandom(32), dtype=np.uint32)])
        self.nonce = 0
        self.hip = hip_runtime()
        self.hip.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
        self.hip.hipHostFree.argtypes = [C.c_void_p]
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

    def next_nonce(self):
        self.nonce += 1
        return self.nonce

    def encrypt_calls(self, count):
        from mkhe_kklss_amd._abi import check, handle_array
        ctx, top, smp = self.params.ctx, self.nq - 1, self.sampler
        pt = self.mk.DeviceLimbs(self.params, count, self.nq).upload(
            np.stack([self.rng.integers(0, q, (count, self.N), dtype=np.uint64) for q in self.pset["Q"]], axis=1))
        outs = [self.mk.batch_ciphertexts(self.mk.Ciphertext, self.params, [ME], top, count) for _ in range(2)]
        hs = [handle_array([c.h for c in o]) for o in outs]
        sk, pk = self.sk.Value.devptr(), self.pk.Value.devptr()
        legs = dict(encrypt_seeded=lambda: check(self.L.mkhe_encrypt_seeded(ctx, top, count, pk, pt.devptr(), 0, *smp.encrypt_args(), hs[0])),
                    encrypt_sk_seeded=lambda: check(self.L.mkhe_encrypt_sk_seeded(ctx, top, count, sk, pt.devptr(), 0, self.seed, self.next_nonce(),
                                                                                  *smp.sk_encrypt_args(), hs[1])))
        return legs, outs, (pt, hs)

    def expand_calls(self, count):
        from mkhe_kklss_amd._abi import check, handle_array
        ctx, top = self.params.ctx, self.nq - 1
        outs = self.mk.batch_ciphertexts(self.mk.Ciphertext, self.params, [ME], top, count)
        hs = handle_array([c.h for c in outs])
        words = count * self.nq * self.N
        pinned = C.c_void_p()
        assert self.hip.hipHostMalloc(C.byref(pinned), 8 * words, 0) == 0
        host = np.ctypeslib.as_array(C.cast(pinned, C.POINTER(C.c_uint64)), shape=(count, self.nq, self.N))
        host[:] = np.stack([self.rng.integers(0, q, (count, self.N), dtype=np.uint64) for q in self.pset["Q"]], axis=1)
        rows = [(C.c_void_p * self.nq)(*[host[b, j].ctypes.data for j in range(self.nq)]) for b in range(count)]

        def upload():
            for b in range(count):
                check(self.L.mkhe_ct_upload_poly_limbs(ctx, outs[b].h, 1, rows[b]))
        legs = dict(upload_poly_limbs=upload, expand_seeded=lambda: check(self.L.mkhe_ct_expand_seeded(ctx, count, self.seed, self.next_nonce(), hs)))
        return legs, (outs, hs, rows, host), pinned

    def sampler_calls(self, count):
        from mkhe_kklss_amd._abi import check
        buf = self.mk.DeviceLimbs(self.params, count, self.nq)
        return dict(sample_uniform=lambda: check(self.L.mkhe_sample_uniform(self.params.ctx, self.nq, count, self.seed, self.next_nonce(), buf.devptr()))), buf

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
    rows = []
    for count in COUNTS:
        legs, outs, keep = s.encrypt_calls(count)
        a = s.alternate(legs, reps)
        legs, keep2, pinned = s.expand_calls(count)
        b = s.alternate(legs, reps)
        legs, buf = s.sampler_calls(count)
        c = s.alternate(legs, reps)
        s.params.sync()
        assert s.hip.hipHostFree(pinned) == 0
        nbytes = 8 * count * s.nq * s.N
        tbs = nbytes / (c["sample_uniform"]["median_us"] * 1e-6) / 1e12
        rows.append(dict(ring="PN15QP880", logN=pset["logN"], nq=s.nq, count=count, reps=reps,
                         encrypt_seeded=a["encrypt_seeded"], encrypt_sk_seeded=a["encrypt_sk_seeded"],
                         encrypt_ratio=round(a["encrypt_sk_seeded"]["median_us"] / a["encrypt_seeded"]["median_us"], 3),
                         upload_poly_limbs=b["upload_poly_limbs"], expand_seeded=b["expand_seeded"],
                         expand_ratio=round(b["expand_seeded"]["median_us"] / b["upload_poly_limbs"]["median_us"], 3),
                         sample_uniform=c["sample_uniform"], sampler_bytes=nbytes, sampler_TBps=round(tbs, 3),
                         sampler_fraction_of_streaming=round(tbs / STREAMING_TBS, 3),
                         wire_bytes=dict(ciphertext=2 * nbytes, seeded=nbytes + 40 * count)))
        print(json.dumps(rows[-1]), flush=True)
    s.close()
    return dict(legs=dict(encrypt_seeded="one mkhe_encrypt_seeded of count plaintexts under the public key",
                          encrypt_sk_seeded="one mkhe_encrypt_sk_seeded of the same plaintexts under the secret key",
                          upload_poly_limbs="count mkhe_ct_upload_poly_limbs of polynomial 1 from pinned host memory",
                          expand_seeded="one mkhe_ct_expand_seeded of count ciphertexts",
                          sample_uniform="one mkhe_sample_uniform of count * nq rows; sampler_TBps = bytes written / median time, beside %.1f TB/s" % STREAMING_TBS),
                rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sk_encrypt_timing.json"))
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
