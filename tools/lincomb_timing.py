"""Device time of one weighted sum with a Rescale, fused and as the chain it replaces ("Polynomial evaluation"):
  fused  mkhe_ct_lincomb(n, .., nb_rescale = 1)
  chain  n x mkhe_ct_mul_const (c_first = c_second) + mkhe_ct_sum + mkhe_rescale(1)
on N = 2^14, 8 limbs, 4 parties, n = 7 real weights, no constant -- where the two compute the same ciphertext, which is checked first.  HIP events on
mkhe_ctx_stream around each leg, the legs alternating, 50 repetitions each after 5 warm-ups, in one process.  Writes one JSON object (times in
microseconds, the engine's byte model for both legs) to --out and prints it.  Needs a GPU:  python tools/lincomb_timing.py [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import harness as H  # noqa: E402
from mkhe_kklss_amd import _abi, mkrlwe  # noqa: E402
from mkhe_kklss_amd._abi import check, handle_array, lib  # noqa: E402

LOGN, LIMBS, PARTIES, TERMS, REPS, WARM = 14, 8, 4, 7, 50, 5


def hip_runtime():
    """the HIP runtime the engine library is linked to, as loaded in this process"""
    lib()
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime in this process")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lincomb_timing.json"))
    args = ap.parse_args()
    pset = H.small_ckks(LOGN, nq=LIMBS)
    Q, N = pset["Q"], 1 << LOGN
    params = mkrlwe.Parameters(LOGN, Q, pset["P"], 2)
    rng = np.random.default_rng(14)
    ids = ["p%d" % i for i in range(PARTIES)]
    new = lambda limbs: mkrlwe.NewCiphertext(params, ids, limbs - 1)
    ins = [new(LIMBS).upload(np.stack([H.uniform_poly(rng, Q, N) for _ in range(1 + PARTIES)])) for _ in range(TERMS)]
    weights = [[int(rng.integers(1, q)) for q in Q] for _ in range(TERMS)]
    mont = [np.array([w * (1 << 64) % q for w, q in zip(ws, Q)], dtype=np.uint64) for ws in weights]
    consts = np.zeros((TERMS + 1, 2, LIMBS), dtype=np.uint64)
    for k in range(TERMS):
        consts[k + 1, 0] = mont[k]
    buf = mkrlwe.DeviceLimbs(params, 1, 1).upload(np.concatenate([consts.ravel(), np.zeros(N - consts.size, dtype=np.uint64)]).reshape(1, 1, N))
    fused_out, prods, summed, chain_out = new(LIMBS - 1), [new(LIMBS) for _ in range(TERMS)], new(LIMBS), new(LIMBS - 1)
    hin, hprods = handle_array([c.h for c in ins]), handle_array([c.h for c in prods])
    L, ctx = lib(), params.ctx

    def fused():
        check(L.mkhe_ct_lincomb(ctx, TERMS, hin, buf.devptr(), 1, fused_out.h))

    def chain():
        for c, m, p in zip(ins, mont, prods):
            check(L.mkhe_ct_mul_const(ctx, c.h, m.ctypes.data_as(_abi.u64p), m.ctypes.data_as(_abi.u64p), p.h))
        check(L.mkhe_ct_sum(ctx, TERMS, hprods, summed.h))
        check(L.mkhe_rescale(ctx, summed.h, 1, chain_out.h))

    fused(); chain()
    assert (fused_out.download() == chain_out.download()).all(), "the fused call and the chain disagree"

    hip = hip_runtime()
    stream = C.c_void_p(params.stream())
    e0, e1 = C.c_void_p(), C.c_void_p()
    for e in (e0, e1):
        assert hip.hipEventCreate(C.byref(e)) == 0

    def timed(f):
        assert hip.hipEventRecord(e0, stream) == 0
        f()
        assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        return ms.value * 1e3

    for _ in range(WARM):
        timed(fused); timed(chain)
    tf, tc = [], []
    for _ in range(REPS):
        tf.append(timed(fused)); tc.append(timed(chain))
    for e in (e0, e1):
        hip.hipEventDestroy(e)
    stat = lambda t: dict(median_us=round(float(np.median(t)), 2), min_us=round(float(min(t)), 2), max_us=round(float(max(t)), 2))
    unit = 8 * N * LIMBS * (1 + PARTIES)
    res = dict(shape=dict(logN=LOGN, limbs=LIMBS, parties=PARTIES, n=TERMS, reps=REPS),
               fused=dict(stat(tf), launches=1, model_bytes=(TERMS + 1) * unit),
               chain=dict(stat(tc), launches=TERMS + 2, model_bytes=(3 * TERMS + 3) * unit),
               model_ratio=round((TERMS + 1) / (3 * TERMS + 3), 3),
               measured_ratio=round(float(np.median(tf) / np.median(tc)), 3))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    params.close()


if __name__ == "__main__":
    main()
