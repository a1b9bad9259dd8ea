"""Device time of K MK-BFV products under one Quantize and one relinearisation tail, and of the chain the call replaces:
  sum    mkhe_bfv_mul_relin_sum(K, ..)
  chain  K x mkhe_bfv_mul_relin + mkhe_ct_sum
on BFV PN15QP880 with four parties in both operands (K = 2, 4, 8) and on BFV PN14QP439 with two parties (K = 2, 4, 8), uniform material.  The two
legs compute different ciphertexts of the same sum (one rounding and one gadget noise of step F2 instead of K), so nothing is compared here:
tests/test_gpu_bfv_mulrelin_sum.py pins the bits.  HIP events on mkhe_ctx_stream around each leg, the legs alternating, REPS repetitions each after
WARM warm-ups, in one process.  Writes one JSON object (times in microseconds: median, min, quartiles) to --out and prints it.
Needs a GPU:  python tools/bfv_mulrelin_sum_timing.py [--out FILE] [--reps N]"""
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
import harness_bfv as HB  # noqa: E402
from mkhe_kklss_amd import mkbfv  # noqa: E402
from mkhe_kklss_amd._abi import check, handle_array, lib  # noqa: E402

WARM = 5


def hip_runtime():
    """the HIP runtime the engine library is linked to, as loaded in this process"""
    lib()
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime in this process")


def uniform_swk(rng, Q, P, N):
    return np.stack([H.uniform_poly(rng, Q + P, N) for _ in range(len(Q))])        # (alpha = 1: one digit per limb of Q)


def measure(hip, name, pset, ids, Ks, reps):
    L = lib()
    Q, P, N = pset["Q"], pset["P"], 1 << pset["logN"]
    params = mkbfv.Parameters(pset["logN"], Q, pset["QMul"], P, pset["T"])
    ctx, rng = params.ctx, np.random.default_rng(pset["logN"])
    for n in ids:
        params.party_index(n)
    rlk = mkbfv.NewRelinearizationKeyKeySet(params)
    for n in ids:
        rlk.AddRelinearizationKey(mkbfv.RelinearizationKey(params, n, *(uniform_swk(rng, Q, P, N) for _ in range(5))))
    params.AddCRS(-1, uniform_swk(rng, Q, P, N))
    key = lambda i, g, j: rlk.GetRelinearizationKey(i).Value[g].Value[j].h
    b1, b2 = handle_array([key(i, 0, 0) for i in ids]), handle_array([key(i, 1, 0) for i in ids])
    d1, d2 = handle_array([key(i, 0, 1) for i in ids]), handle_array([key(i, 1, 1) for i in ids])
    v, u = handle_array([key(i, 0, 2) for i in ids]), params.CRS[-1].h
    Kmax = max(Ks)
    new = lambda: mkbfv.NewCiphertext(params, ids)
    ct = lambda: new().upload(np.stack([H.uniform_poly(rng, Q, N) for _ in range(1 + len(ids))]))
    ops0, ops1 = [ct() for _ in range(Kmax)], [ct() for _ in range(Kmax)]
    prods, chain_out, sum_out = [new() for _ in range(Kmax)], new(), new()
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

    rows = []
    for K in Ks:
        a, b = handle_array([c.h for c in ops0[:K]]), handle_array([c.h for c in ops1[:K]])
        hp = handle_array([p.h for p in prods[:K]])

        def summed():
            check(L.mkhe_bfv_mul_relin_sum(ctx, K, a, b, b1, b2, d1, d2, v, u, sum_out.h))

        def chain():
            for k in range(K):
                check(L.mkhe_bfv_mul_relin(ctx, ops0[k].h, ops1[k].h, b1, b2, d1, d2, v, u, prods[k].h))
            check(L.mkhe_ct_sum(ctx, K, hp, chain_out.h))

        for _ in range(WARM):
            timed(summed); timed(chain)
        ts, tc = [], []
        for _ in range(reps):
            ts.append(timed(summed)); tc.append(timed(chain))
        stat = lambda t: dict(median_us=round(float(np.median(t)), 1), min_us=round(float(min(t)), 1),
                              q1_us=round(float(np.percentile(t, 25)), 1), q3_us=round(float(np.percentile(t, 75)), 1))
        s, c = stat(ts), stat(tc)
        rows.append(dict(ring=name, logN=pset["logN"], limbs=len(Q), parties=len(ids), K=K, reps=reps, sum=s, chain=c,
                         saved_us=round(c["median_us"] - s["median_us"], 1), saved_per_extra_pair_us=round((c["median_us"] - s["median_us"]) / (K - 1), 1),
                         chain_iqr_us=round(c["q3_us"] - c["q1_us"], 1), ratio=round(s["median_us"] / c["median_us"], 3)))
        print(json.dumps(rows[-1]), flush=True)
    for e in (e0, e1):
        hip.hipEventDestroy(e)
    params.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bfv_mulrelin_sum_timing.json"))
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("at least 20 repetitions")
    hip = hip_runtime()
    rows = measure(hip, "BFV PN15QP880", HB.BFV_PN15QP880, ["p0", "p1", "p2", "p3"], (2, 4, 8), args.reps)
    rows += measure(hip, "BFV PN14QP439", HB.BFV_PN14QP439, ["p0", "p1"], (2, 4, 8), args.reps)
    res = dict(legs=dict(sum="mkhe_bfv_mul_relin_sum(K)", chain="K x mkhe_bfv_mul_relin + mkhe_ct_sum"), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
