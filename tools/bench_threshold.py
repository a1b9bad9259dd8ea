"""What the threshold secret keys cost.  PN15QP880 (mkrlwe context, N = 2^15, R = 14 + 2 rows).  Device time = HIP events on
mkhe_ctx_stream around INNER back-to-back calls (a single call is tens of microseconds: the window has to hold enough work); WARM warm-up
windows, then REPS windows per leg, the legs alternating in one process.  Times in microseconds per call: median, min, quartiles.  Recorded, not
gated.
  gen_shares  mkhe_threshold_gen_shares at (t, n) = (3, 5) and (8, 16).  written GB/s = 8 n R N bytes over the time; ChaCha20 blocks/s =
              2 (t - 1) ceil(n / THR_G) R N / 8 blocks over the time (every group of THR_G points expands the keystream again).
  limbs_sum   mkhe_limbs_sum of nsrc = 8 buffers [count][14][N] at count = 16 (59 MB each: HBM traffic) and count = 1 (cache-resident);
              achieved GB/s = 8 (nsrc + 1) count limbs N bytes over the time.

  python tools/bench_threshold.py [--out FILE] [--reps N]
Needs a GPU."""
import argparse
import ctypes as C
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARM, INNER = 3, 20
SHAPES = ((3, 5), (8, 16))
NSRC, LIMBS, COUNTS = 8, 14, (16, 1)


def hip_runtime():
    """the HIP runtime the engine library is linked to, as loaded in this process"""
    from mkhe_kklss_amd._abi import lib
    lib()
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime in this process")


def group_size():
    src = open(os.path.join(ROOT, "mkhe-kklss_amd", "csrc", "threshold_kernels.h")).read()
    return int(re.search(r"constexpr int THR_G = (\d+);", src).group(1))


def stat(t):
    return dict(median_us=round(float(np.median(t)), 2), min_us=round(float(min(t)), 2), q1_us=round(float(np.percentile(t, 25)), 2),
                q3_us=round(float(np.percentile(t, 75)), 2))


class Setup:
    def __init__(self, pset):
        from mkhe_kklss_amd import mkrlwe
        from mkhe_kklss_amd._abi import lib
        self.mk, self.L = mkrlwe, lib()
        self.params = mkrlwe.Parameters(pset["logN"], pset["Q"], pset["P"])
        self.N, self.R, self.moduli = self.params.N(), len(pset["Q"]) + len(pset["P"]), list(pset["Q"]) + list(pset["P"])
        self.rng = np.random.default_rng(17)
        self.sk = mkrlwe.NewKeyGenerator(self.params, mkrlwe.HostSampler()).GenSecretKey("alice")
        self.sampler = mkrlwe.DeviceSampler()
        self.hip = hip_runtime()
        self.stream = C.c_void_p(self.params.stream())
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        for e in (self.e0, self.e1):
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def window_us(self, f):
        """device time of INNER calls of f, per call"""
        assert self.hip.hipEventRecord(self.e0, self.stream) == 0
        for _ in range(INNER):
            f()
        assert self.hip.hipEventRecord(self.e1, self.stream) == 0 and self.hip.hipEventSynchronize(self.e1) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.e0, self.e1) == 0
        return ms.value * 1e3 / INNER

    def gen_call(self, t, n):
        from mkhe_kklss_amd._abi import check, handle_array
        outs = [self.mk.DeviceLimbs(self.params, 1, self.R) for _ in range(n)]
        oh, xs = handle_array([o.devptr() for o in outs]), (C.c_uint32 * n)(*range(1, n + 1))

        def call():
            key, nonce = self.sampler.threshold_args()
            check(self.L.mkhe_threshold_gen_shares(self.params.ctx, self.sk.Value.devptr(), t, n, xs, key, nonce, oh))
        return call, (outs, oh, xs)

    def sum_call(self, count):
        from mkhe_kklss_amd._abi import check, handle_array
        host = np.stack([self.rng.integers(0, q, (count, self.N), dtype=np.uint64) for q in self.moduli[:LIMBS]], axis=1)
        srcs = [self.mk.DeviceLimbs(self.params, count, LIMBS).upload(np.roll(host, s, axis=2)) for s in range(NSRC)]
        dst = self.mk.DeviceLimbs(self.params, count, LIMBS)
        sh = handle_array([s.devptr() for s in srcs])
        return (lambda: check(self.L.mkhe_limbs_sum(self.params.ctx, count, LIMBS, NSRC, sh, dst.devptr()))), (srcs, dst, sh)

    def alternate(self, legs, reps):
        for _ in range(WARM):
            for f in legs.values():
                self.window_us(f)
        t = {k: [] for k in legs}
        for _ in range(reps):
            for k, f in legs.items():
                t[k].append(self.window_us(f))
        return {k: stat(v) for k, v in t.items()}

    def close(self):
        for e in (self.e0, self.e1):
            self.hip.hipEventDestroy(e)
        self.params.close()


def measure(reps):
    import harness as H
    pset, G = H.PN15QP880, group_size()
    s = Setup(pset)
    legs, keep = {}, []
    for t, n in SHAPES:
        legs["gen_shares_%d_of_%d" % (t, n)], k = s.gen_call(t, n)
        keep.append(k)
    for count in COUNTS:
        legs["limbs_sum_count_%d" % count], k = s.sum_call(count)
        keep.append(k)
    res = s.alternate(legs, reps)
    rows = []
    for t, n in SHAPES:
        st = res["gen_shares_%d_of_%d" % (t, n)]
        sec = st["median_us"] * 1e-6
        blocks = 2 * (t - 1) * -(-n // G) * s.R * s.N // 8
        rows.append(dict(call="mkhe_threshold_gen_shares", ring="PN15QP880", logN=pset["logN"], rows=s.R, threshold=t, nshares=n, group=G, reps=reps, inner=INNER,
                         time=st, written_bytes=8 * n * s.R * s.N, written_GBps=round(8 * n * s.R * s.N / sec / 1e9, 1), chacha_blocks=blocks,
                         chacha_blocks_per_s=float("%.4g" % (blocks / sec))))
    for count in COUNTS:
        st = res["limbs_sum_count_%d" % count]
        moved = 8 * (NSRC + 1) * count * LIMBS * s.N
        rows.append(dict(call="mkhe_limbs_sum", ring="PN15QP880", logN=pset["logN"], limbs=LIMBS, count=count, nsrc=NSRC, reps=reps, inner=INNER, time=st,
                         moved_bytes=moved, achieved_GBps=round(moved / (st["median_us"] * 1e-6) / 1e9, 1)))
    for r in rows:
        print(json.dumps(r), flush=True)
    s.close()
    return dict(legs=dict(gen_shares="one mkhe_threshold_gen_shares: n shares of a 16-row secret key, t - 1 coefficient polynomials from the keystream",
                          limbs_sum="one mkhe_limbs_sum of 8 buffers [count][14][N] into a ninth"), rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "threshold_timing.json"))
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
