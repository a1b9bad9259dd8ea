"""What the encryption samples cost, on the host and on the device:
  (a) host    mkhe_encrypt on samples drawn beforehand with mkrlwe.HostSampler (os.urandom): two uploads and a stream synchronise in front
              of the five launches.  Device time = HIP events on mkhe_ctx_stream around the call; wall time = draw + call + synchronise.
  (b) seeded  mkhe_encrypt_seeded: one sampler launch in front of the same five.  Device time as above; wall time = call + synchronise.
and the host draw alone.  PN15QP880 at the top level, count = 1, 4, 16 plaintexts under one public key; the two legs alternate in one process,
WARM warm-ups, then REPS repetitions each.  Times in microseconds: median, min, quartiles.  The two legs encrypt under different samples, so
nothing is compared here: tests/test_gpu_device_sampler.py pins the bits.

  python tools/encrypt_sampler_timing.py [--out FILE] [--reps N]      the measurement; writes one JSON object and prints it
  python tools/encrypt_sampler_timing.py --trace-leg                  10 seeded calls per count and nothing else: the run to put under
                                                                      rocprofv3 --kernel-trace (a run of its own: tracing slows the host)
  python tools/encrypt_sampler_timing.py --merge-trace CSV --out FILE   adds the durations of small_sample_kernel from that trace to FILE
Needs a GPU (the last form does not)."""
import argparse
import ctypes as C
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARM = 5
COUNTS = (1, 4, 16)
KERNEL = "small_sample_kernel"


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
        self.name, self.H, self.mk, self.L = "PN15QP880", H, mkrlwe, lib()
        self.params = mkrlwe.Parameters(p["logN"], p["Q"], p["P"], 2)
        self.params.AddCRS(0, seed=5)
        self.N, self.level, self.rng = self.params.N(), len(p["Q"]) - 1, np.random.default_rng(15)
        self.host = mkrlwe.HostSampler()                                    # os.urandom, as a user has it
        self.dev = mkrlwe.DeviceSampler()
        _, self.pk = mkrlwe.NewKeyGenerator(self.params, self.host).GenKeyPair("user0")

    def case(self, count):
        from mkhe_kklss_amd._abi import check, handle_array, s32p
        pts = np.stack([self.H.uniform_poly(self.rng, self.params.Q, self.N) for _ in range(count)])
        d = self.mk.DeviceLimbs(self.params, count, self.level + 1).upload(pts)
        outs = [self.mk.Ciphertext(self.params, ["user0"], self.level) for _ in range(count)]
        hs = handle_array([c.h for c in outs])
        args = (self.params.ctx, self.level, count, self.pk.Value.devptr(), d.devptr(), 0)
        draw = lambda: np.ascontiguousarray(np.stack([np.concatenate([self.host.ternary(self.N, 0.5)[None], self.host.gaussian(2, self.N)])
                                                      for _ in range(count)]), dtype=np.int32)
        host = lambda smp: check(self.L.mkhe_encrypt(*args, smp.ctypes.data_as(s32p), hs))
        seeded = lambda: check(self.L.mkhe_encrypt_seeded(*args, *self.dev.encrypt_args(), hs))
        return (d, outs, hs), draw, host, seeded


def measure(reps):
    s = Setup()
    hip = hip_runtime()
    stream = C.c_void_p(s.params.stream())
    e0, e1 = C.c_void_p(), C.c_void_p()
    for e in (e0, e1):
        assert hip.hipEventCreate(C.byref(e)) == 0

    def device_us(f):
        assert hip.hipEventRecord(e0, stream) == 0
        f()
        assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        return ms.value * 1e3

    def wall_us(f):
        s.params.sync()
        t0 = time.perf_counter()
        f()
        s.params.sync()
        return (time.perf_counter() - t0) * 1e6

    rows = []
    for count in COUNTS:
        keep, draw, host, seeded = s.case(count)
        for _ in range(WARM):
            smp = draw()
            device_us(lambda: host(smp)); device_us(seeded); wall_us(lambda: host(draw())); wall_us(seeded)
        t = dict(a_dev=[], b_dev=[], a_wall=[], b_wall=[], draw=[])
        for _ in range(reps):
            smp = draw()
            t["a_dev"].append(device_us(lambda: host(smp)))
            t["b_dev"].append(device_us(seeded))
            t["a_wall"].append(wall_us(lambda: host(draw())))
            t["b_wall"].append(wall_us(seeded))
            t0 = time.perf_counter()
            draw()
            t["draw"].append((time.perf_counter() - t0) * 1e6)
        st = {k: stat(v) for k, v in t.items()}
        a, b = st["a_dev"], st["b_dev"]
        rows.append(dict(ring=s.name, logN=15, limbs=s.level + 1, count=count, reps=reps, sample_bytes_host=12 * s.N * count,
                         host_device=a, seeded_device=b, host_wall=st["a_wall"], seeded_wall=st["b_wall"], host_draw_alone=st["draw"],
                         device_ratio=round(b["median_us"] / a["median_us"], 3), wall_ratio=round(st["b_wall"]["median_us"] / st["a_wall"]["median_us"], 3),
                         host_device_iqr_us=round(a["q3_us"] - a["q1_us"], 1),
                         seeded_within_host_iqr=bool(b["median_us"] <= a["median_us"] + (a["q3_us"] - a["q1_us"]))))
        print(json.dumps(rows[-1]), flush=True)
    for e in (e0, e1):
        hip.hipEventDestroy(e)
    s.params.close()
    return dict(legs=dict(host="mkhe_encrypt on HostSampler samples (os.urandom) drawn beforehand; wall includes the draw",
                          seeded="mkhe_encrypt_seeded (DeviceSampler)"), rows=rows)


def trace_leg():
    s = Setup()
    for count in COUNTS:
        keep, draw, host, seeded = s.case(count)
        for _ in range(10):
            seeded()
        s.params.sync()
    s.params.close()


def merge_trace(path, out):
    """median duration of the sampler kernel per count from a rocprofv3 kernel trace (grid.y = 3 * count polynomials)"""
    by = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if KERNEL in row.get("Kernel_Name", ""):
                by.setdefault(int(row["Grid_Size_Y"]) // 3, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    if not by:
        raise SystemExit("no %s dispatch in %s" % (KERNEL, path))
    res = json.load(open(out))
    for row in res["rows"]:
        if row["count"] in by:
            row["sampler_kernel_trace"] = dict(stat(by[row["count"]]), dispatches=len(by[row["count"]]))
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({c: stat(v) for c, v in sorted(by.items())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encrypt_sampler_timing.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--trace-leg", action="store_true")
    ap.add_argument("--merge-trace")
    args = ap.parse_args()
    if args.trace_leg:
        return trace_leg()
    if args.merge_trace:
        return merge_trace(args.merge_trace, args.out)
    if args.reps < 20:
        raise SystemExit("at least 20 repetitions")
    res = measure(args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
