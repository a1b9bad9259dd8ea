"""Device time of the MK-BFV polynomial evaluation and of its weighted-sum kernel, on BFV PN15QP880 with four parties, uniform
material:
  poly15, poly63   Evaluator.EvaluatePolyNew (one mkhe_bfv_ct_lincomb for every inner sum, one mkhe_bfv_mul_relin_sum for the giant products, one
                   mkhe_ct_add) against fused=False (one mkhe_ct_lincomb per inner sum, one mkhe_bfv_mul_relin per giant product, mkhe_ct_add), dense
                   full-range coefficients of degree 15 and 63; both legs compute the powers with the same mkhe_bfv_mul_relin calls, and both
                   include the host's encoding and upload of the constants
  kernel           mkhe_bfv_ct_lincomb(nin, nout) against nout x mkhe_ct_lincomb(nin), constants resident, for the shapes of degree 15, 63 and 255
                   (nin = m - 1 baby powers, nout = g inner sums) and for (16, 64)
The fused and the plain evaluation give different ciphertexts of the same values and the two kernel legs the same bits; nothing is compared here:
tests/test_gpu_bfv_lincomb.py and tests/test_gpu_bfv_polyeval_e2e.py pin both.  HIP events on mkhe_ctx_stream around each leg, the legs alternating,
REPS repetitions each after WARM warm-ups.  Every leg runs in a process of its own under its own `timeout`; the first failure stops the script.
Writes one JSON object (times in microseconds: median, min, quartiles; launch and byte counts as derived in DESIGN.md) to --out and prints it.
Needs a GPU:  python tools/bfv_polyeval_timing.py [--out FILE] [--reps N]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARM = 3
LEGS = {"poly15": 300, "poly63": 400, "kernel": 300}             # leg -> its time limit in seconds
IDS = ["p0", "p1", "p2", "p3"]


def hip_runtime(lib):
    """the HIP runtime the engine library is linked to, as loaded in this process"""
    lib()
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime in this process")


def stat(t):
    return dict(median_us=round(float(np.median(t)), 1), min_us=round(float(min(t)), 1),
                q1_us=round(float(np.percentile(t, 25)), 1), q3_us=round(float(np.percentile(t, 75)), 1))


def run_leg(leg, reps):
    import harness as H
    import harness_bfv as HB
    from mkhe_kklss_amd import mkbfv, mkckks, mkrlwe
    from mkhe_kklss_amd._abi import check, handle_array, lib
    hip = hip_runtime(lib)
    pset = HB.BFV_PN15QP880
    Q, P, N, T = pset["Q"], pset["P"], 1 << pset["logN"], pset["T"]
    params = mkbfv.Parameters(pset["logN"], Q, pset["QMul"], P, T)
    rng = np.random.default_rng(15)
    for n in IDS:
        params.party_index(n)
    ev = mkbfv.NewEvaluator(params)
    new = lambda: mkbfv.NewCiphertext(params, IDS)
    ct = lambda: new().upload(np.stack([H.uniform_poly(rng, Q, N) for _ in range(1 + len(IDS))]))
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

    def alternate(a, b):
        for _ in range(WARM):
            timed(a); timed(b)
        ta, tb = [], []
        for _ in range(reps):
            ta.append(timed(a)); tb.append(timed(b))
        return stat(ta), stat(tb)

    words = 8.0 * N * len(Q) * (1 + len(IDS))                     # bytes of one ciphertext
    rows = []
    if leg.startswith("poly"):
        degree = int(leg[4:])
        swk = lambda: np.stack([H.uniform_poly(rng, Q + P, N) for _ in range(len(Q))])        # (alpha = 1: one digit per limb of Q)
        rlk = mkbfv.NewRelinearizationKeyKeySet(params)
        for n in IDS:
            rlk.AddRelinearizationKey(mkbfv.RelinearizationKey(params, n, *(swk() for _ in range(5))))
        params.AddCRS(-1, swk())
        x = ct()
        coeffs = [int(c) or 1 for c in rng.integers(-(T // 2), T // 2 + 1, degree + 1)]
        plan = mkckks.poly_eval_plan(degree)
        fused, plain = alternate(lambda: ev.EvaluatePolyNew(x, coeffs, rlk), lambda: ev.EvaluatePolyNew(x, coeffs, rlk, fused=False))
        g, nin = plan.g, plan.m - 1
        rows.append(dict(leg=leg, ring="BFV PN15QP880", parties=len(IDS), degree=degree, m=plan.m, g=g, reps=reps, fused=fused, plain=plain,
                         power_products=len(plan.products),
                         fused_calls=dict(mkhe_bfv_ct_lincomb=1, mkhe_bfv_mul_relin_sum=1, mkhe_ct_add=1),
                         plain_calls=dict(mkhe_ct_lincomb=g, mkhe_bfv_mul_relin=g - 1, mkhe_ct_add=g - 1),
                         sum_bytes_fused=words * (nin + g), sum_bytes_plain=words * g * (nin + 1),
                         saved_us=round(plain["median_us"] - fused["median_us"], 1), ratio=round(fused["median_us"] / plain["median_us"], 3)))
        print(json.dumps(rows[-1]), flush=True)
    else:
        L = lib()
        ins, outs = [ct() for _ in range(16)], mkrlwe.batch_ciphertexts(mkbfv.Ciphertext, params, set(IDS), params.MaxLevel(), 64)
        for nin, nout in ((3, 4), (7, 8), (15, 16), (16, 64)):
            weights = rng.integers(-(T // 2), T // 2 + 1, (nout, nin))
            weights[weights == 0] = 1
            consts = mkbfv.bfv_lincomb_consts(Q, T, weights.tolist(), list(range(nout)))
            block = ev._consts_buffer(consts)
            singles = [ev._consts_buffer(np.stack([c, np.zeros_like(c)], axis=1)) for c in consts]
            hin, hout = handle_array([c.h for c in ins[:nin]]), handle_array([c.h for c in outs[:nout]])

            def fused_call():
                check(L.mkhe_bfv_ct_lincomb(params.ctx, nin, hin, nout, block.devptr(), hout))

            def per_output():
                for g in range(nout):
                    check(L.mkhe_ct_lincomb(params.ctx, nin, hin, singles[g].devptr(), 0, outs[g].h))

            one, many = alternate(fused_call, per_output)
            b_one, b_many = words * (nin + nout), words * nout * (nin + 1)
            rows.append(dict(leg=leg, ring="BFV PN15QP880", parties=len(IDS), nin=nin, nout=nout, reps=reps, one_launch=one, per_output=many,
                             launches=dict(one_launch=1, per_output=nout), bytes=dict(one_launch=b_one, per_output=b_many),
                             gbps=dict(one_launch=round(b_one / one["median_us"] / 1e3, 1), per_output=round(b_many / many["median_us"] / 1e3, 1)),
                             ratio=round(one["median_us"] / many["median_us"], 3)))
            print(json.dumps(rows[-1]), flush=True)
    for e in (e0, e1):
        hip.hipEventDestroy(e)
    params.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bfv_polyeval_timing.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--leg", choices=sorted(LEGS), help="run this leg in this process and print its rows (what the script starts for every leg)")
    args = ap.parse_args()
    if args.reps < 10:
        raise SystemExit("at least 10 repetitions")
    if args.leg:
        print("ROWS " + json.dumps(run_leg(args.leg, args.reps)), flush=True)
        return
    rows = []
    for leg, limit in LEGS.items():               # a fresh process per leg, each under its own time limit; the first failure ends the script
        out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--reps", str(args.reps)],
                             capture_output=True, text=True)
        sys.stdout.write(out.stdout)
        if out.returncode != 0:
            sys.stderr.write(out.stderr[-4000:])
            raise SystemExit("leg %s failed with status %d: stopping" % (leg, out.returncode))
        rows += json.loads([line for line in out.stdout.splitlines() if line.startswith("ROWS ")][-1][5:])
    res = dict(legs=dict(fused="EvaluatePolyNew", plain="EvaluatePolyNew(fused=False)", one_launch="mkhe_bfv_ct_lincomb(nin, nout)",
                         per_output="nout x mkhe_ct_lincomb(nin)"), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
