"""What measuring the noise of one ciphertext costs.  PN15QP880 (mkckks context, N = 2^15), level 13 = 14 limbs, count = 1, a uniform
phase and a uniform reference on the device.  Recorded, not gated.
  device   mkhe_noise_norm alone: HIP events on mkhe_ctx_stream around the call, WARM warm-ups, then REPS repetitions; microseconds: median, min, quartiles
  call     Decryptor.NoiseNormBatch as a user calls it: the call, the download of limbs + 1 words and the host's multiplication of the digits,
           host clock (the download synchronises), same repetitions
  by_hand  what the tests did before: download phase and reference (2 x 8 limbs N bytes), CRT every coefficient in Python integers, centre, take the
           maximum -- host clock, HAND_REPS runs
The two routes must give the same integer at the same index.

  python tools/noise_timing.py [--out FILE] [--reps N]
Needs a GPU."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARM, HAND_REPS = 5, 3


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


def measure(reps):
    import harness as H
    from mkhe_kklss_amd import mkckks, mkrlwe
    from mkhe_kklss_amd._abi import check, lib
    pset = H.PN15QP880
    qs, L = pset["Q"], len(pset["Q"])
    params = mkckks.Parameters(pset["logN"], qs, pset["P"], pset["scale"])
    N, rng = params.N(), np.random.default_rng(17)
    host_phase, host_ref = H.uniform_poly(rng, qs, N)[None], H.uniform_poly(rng, qs, N)[None]
    phase, ref = mkrlwe.DeviceLimbs(params, 1, L).upload(host_phase), mkrlwe.DeviceLimbs(params, 1, L).upload(host_ref)
    out, dec = mkrlwe.DeviceLimbs(params, 1, 1), mkrlwe.NewDecryptor(params)
    hip, stream, e0, e1 = hip_runtime(), C.c_void_p(params.stream()), C.c_void_p(), C.c_void_p()
    for e in (e0, e1):
        assert hip.hipEventCreate(C.byref(e)) == 0

    def device_us():
        assert hip.hipEventRecord(e0, stream) == 0
        check(lib().mkhe_noise_norm(params.ctx, 0, L, 1, phase.devptr(), ref.devptr(), 0, out.devptr()))
        assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        return ms.value * 1e3

    def call_us():
        t = time.perf_counter()
        r = dec.NoiseNormBatch(phase, ref)
        return (time.perf_counter() - t) * 1e6, r[0]

    def by_hand_us():
        t = time.perf_counter()
        d = (phase.download()[0].astype(object) - ref.download()[0].astype(object)) % np.array(qs, dtype=object)[:, None]
        c = [abs(v) for v in H.crt_center(d.astype(np.uint64), qs)[0]]
        r = max(c)
        return (time.perf_counter() - t) * 1e6, (r, c.index(r))

    for _ in range(WARM):
        device_us()
        call_us()
    dev, call, hand = [], [], []
    for _ in range(reps):
        dev.append(device_us())
        call.append(call_us())
    for _ in range(HAND_REPS):
        hand.append(by_hand_us())
    same = all(r == hand[0][1] for _, r in call + hand)
    for e in (e0, e1):
        hip.hipEventDestroy(e)
    params.close()
    return dict(ring="PN15QP880", logN=pset["logN"], limbs=L, count=1, reps=reps, hand_reps=HAND_REPS,
                device=stat(dev), call=stat([t for t, _ in call]), by_hand=stat([t for t, _ in hand]), same_result=bool(same),
                bytes_down=dict(call=8 * (L + 1), by_hand=2 * 8 * L * N))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise_timing.json"))
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("at least 20 repetitions")
    res = measure(args.reps)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
