"""Device time of K products under one relinearisation tail, and of the chain the call replaces:
  sum    mkhe_mul_relin_sum(K, .., rescale = 1)
  chain  K x mkhe_mul_relin_rescale + mkhe_ct_sum
on PN15QP880 with four parties in both operands (K = 2, 4, 8; hoisted forms NULL and given) and on the CNN's ring PN14QP433 with one party per operand
(K = 4, 8; hoisted forms given, as cnn.Convolution / FC1Layer supply them), uniform material at the top level.  The two legs compute different
ciphertexts of the same sum (one gadget noise of step F2 instead of K), so nothing is compared here: tests/test_gpu_mulrelin_sum.py pins the bits.
HIP events on mkhe_ctx_stream around each leg, the legs alternating, REPS repetitions each after WARM warm-ups, in one process.  Writes one JSON object
(times in microseconds: median, min, quartiles) to --out and prints it.  Needs a GPU:  python tools/mulrelin_sum_timing.py [--out FILE] [--reps N]"""
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
from mkhe_kklss_amd import mkrlwe  # noqa: E402
from mkhe_kklss_amd._abi import check, handle_array, lib  # noqa: E402

WARM = 5


def cnn_ring():
    import harness_cnn as HC
    return HC.PN14QP433


def hip_runtime():
    """the HIP runtime the engine library is linked to, as loaded in this process"""
    lib()
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime in this process")


def uniform_swk(rng, Q, P, N):
    return np.stack([H.uniform_poly(rng, Q + P, N) for _ in range(len(Q))])        # (alpha = 1 on both rings: one digit per limb of Q)


def measure(hip, name, pset, ids0, ids1, Ks, hoist_modes, reps):
    L = lib()
    Q, P, N = pset["Q"], pset["P"], 1 << pset["logN"]
    params = mkrlwe.Parameters(pset["logN"], Q, P, 2)
    ctx, rng, top = params.ctx, np.random.default_rng(pset["logN"]), len(Q) - 1
    names = sorted(set(ids0) | set(ids1))
    for n in names:
        params.party_index(n)
    rlk = mkrlwe.RelinearizationKeySet(params)
    for n in names:
        rlk.AddRelinearizationKey(mkrlwe.RelinearizationKey(params, n, *(uniform_swk(rng, Q, P, N) for _ in range(3))))
    params.AddCRS(-1, uniform_swk(rng, Q, P, N))
    key = lambda i, j: rlk.GetRelinearizationKey(i).Value[j].h
    b1, d0, v0 = handle_array([key(i, 0) for i in ids1]), handle_array([key(i, 1) for i in ids0]), handle_array([key(i, 2) for i in ids0])
    u = params.CRS[-1].h
    Kmax = max(Ks)
    new = lambda ids, level: mkrlwe.NewCiphertext(params, ids, level)
    ct = lambda ids: new(ids, top).upload(np.stack([H.uniform_poly(rng, Q, N) for _ in range(1 + len(ids))]))
    ops0, ops1 = [ct(ids0) for _ in range(Kmax)], [ct(ids1) for _ in range(Kmax)]

    def hoisted(c):
        ks = [mkrlwe.NewSwitchingKey(params) for _ in c.ids]
        check(L.mkhe_hoisted_form(ctx, top, c.h, handle_array([k.h for k in ks])))
        return ks
    f0, f1 = [hoisted(c) for c in ops0], [hoisted(c) for c in ops1]
    prods, chain_out, sum_out = [new(names, top - 1) for _ in range(Kmax)], new(names, top - 1), new(names, top - 1)
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
        for given in hoist_modes:
            a, b = handle_array([c.h for c in ops0[:K]]), handle_array([c.h for c in ops1[:K]])
            h0 = handle_array([k.h for ks in f0[:K] for k in ks]) if given else None
            h1 = handle_array([k.h for ks in f1[:K] for k in ks]) if given else None
            per = [(handle_array([k.h for k in f0[k]]) if given else None, handle_array([k.h for k in f1[k]]) if given else None) for k in range(K)]
            hp = handle_array([p.h for p in prods[:K]])

            def summed():
                check(L.mkhe_mul_relin_sum(ctx, K, a, b, h0, h1, b1, d0, v0, u, 1, sum_out.h))

            def chain():
                for k in range(K):
                    check(L.mkhe_mul_relin_rescale(ctx, ops0[k].h, ops1[k].h, per[k][0], per[k][1], b1, d0, v0, u, prods[k].h))
                check(L.mkhe_ct_sum(ctx, K, hp, chain_out.h))

            for _ in range(WARM):
                timed(summed); timed(chain)
            ts, tc = [], []
            for _ in range(reps):
                ts.append(timed(summed)); tc.append(timed(chain))
            stat = lambda t: dict(median_us=round(float(np.median(t)), 1), min_us=round(float(min(t)), 1),
                                  q1_us=round(float(np.percentile(t, 25)), 1), q3_us=round(float(np.percentile(t, 75)), 1))
            s, c = stat(ts), stat(tc)
            rows.append(dict(ring=name, logN=pset["logN"], limbs=len(Q), parties0=len(ids0), parties1=len(ids1), K=K, hoisted="given" if given else "NULL", reps=reps,
                             sum=s, chain=c, saved_us=round(c["median_us"] - s["median_us"], 1), chain_iqr_us=round(c["q3_us"] - c["q1_us"], 1),
                             ratio=round(s["median_us"] / c["median_us"], 3)))
            print(json.dumps(rows[-1]), flush=True)
    for e in (e0, e1):
        hip.hipEventDestroy(e)
    params.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mulrelin_sum_timing.json"))
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("at least 20 repetitions")
    hip = hip_runtime()
    four = ["p0", "p1", "p2", "p3"]
    rows = measure(hip, "PN15QP880", H.PN15QP880, four, four, (2, 4, 8), (False, True), args.reps)
    rows += measure(hip, "PN14QP433 (cnn)", cnn_ring(), ["dataOwner"], ["modelOwner"], (4, 8), (True,), args.reps)
    res = dict(legs=dict(sum="mkhe_mul_relin_sum(K, rescale = 1)", chain="K x mkhe_mul_relin_rescale + mkhe_ct_sum"), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
