"""Device time of mkhe_bfv_encode / mkhe_bfv_decode and of their stage pairs at N = 2^15, nQ = 14 (BFV_PN15QP880), T = 65537, count = 1 and 64
(profiles/README.md, "BFV batch encoder"): HIP events on mkhe_ctx_stream around 20 back-to-back calls, 5 warm-up calls first, median of 7
such measurements (min .. max), with the compulsory bytes of each call and their rate.  Beside it the wall time of the host conversion the
calls replace (mkbfv.ScaleUp / ScaleDown, Python integers, one polynomial).  Needs a GPU:  python tools/bfv_encoder_timing.py"""
import os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import harness_bfv as HB
from mkhe_kklss_amd import mkbfv, mkrlwe
from mkhe_kklss_amd._abi import check, lib

p = HB.BFV_PN15QP880
params = mkbfv.Parameters(p["logN"], p["Q"], p["QMul"], p["P"], p["T"])
N, nQ, T = params.N(), len(p["Q"]), p["T"]
stream = torch.cuda.ExternalStream(lib().mkhe_ctx_stream(params.ctx))
print("tile 2^%d words; N = 2^%d, nQ = %d, T = %d" % (lib().mkhe_ctx_bfv_tile(params.ctx), p["logN"], nQ, T))

def timed(f, reps=20):
    for _ in range(5):
        f()
    ts = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            f()
        e1.record(stream); e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / reps)
    ts.sort()
    return ts[3], ts[0], ts[-1]

rng = np.random.default_rng(0)
for count in (1, 64):
    v = rng.integers(-2 ** 63, 2 ** 63 - 1, (count, 1, N), dtype=np.int64)
    slots = mkrlwe.DeviceLimbs(params, count, 1).upload(v.view(np.uint64))
    coeffs, back = mkrlwe.DeviceLimbs(params, count, 1), mkrlwe.DeviceLimbs(params, count, 1)
    pt = mkrlwe.DeviceLimbs(params, count, nQ)
    L, c = lib(), params.ctx
    legs = {
        "encode (fused)": lambda: check(L.mkhe_bfv_encode(c, count, slots.devptr(), pt.devptr())),
        "encode (stage pair)": lambda: (check(L.mkhe_bfv_slots_to_coeffs(c, count, slots.devptr(), coeffs.devptr())), check(L.mkhe_bfv_scale_up(c, count, coeffs.devptr(), pt.devptr()))),
        "decode (fused)": lambda: check(L.mkhe_bfv_decode(c, count, pt.devptr(), back.devptr())),
        "decode (stage pair)": lambda: (check(L.mkhe_bfv_scale_down(c, count, pt.devptr(), coeffs.devptr())), check(L.mkhe_bfv_coeffs_to_slots(c, count, coeffs.devptr(), back.devptr()))),
    }
    bytes_ = 8.0 * N * count * (1 + nQ)          # encode: reads 8 N count, writes 8 nQ N count; decode: the other way round
    for name, f in legs.items():
        med, lo, hi = timed(f)
        print("count %2d  %-20s us median %9.1f (min %9.1f max %9.1f)   compulsory %6.2f MB -> %7.1f GB/s" % (count, name, med, lo, hi, bytes_ / 1e6, bytes_ / med / 1e3))
    assert (back.download().view(np.int64)[:, 0] == np.where(v[:, 0] % T > T // 2, v[:, 0] % T - T, v[:, 0] % T)).all()
# the host conversion of ONE polynomial that the calls replace
m = rng.integers(0, T, N)
t0 = time.perf_counter(); hp = mkbfv.ScaleUp(m, params); t1 = time.perf_counter(); mkbfv.ScaleDown(hp, params); t2 = time.perf_counter()
print("host, one polynomial: mkbfv.ScaleUp %.1f ms, mkbfv.ScaleDown %.1f ms" % ((t1 - t0) * 1e3, (t2 - t1) * 1e3))
params.close()
