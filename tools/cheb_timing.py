"""Device time of the MK-CKKS Chebyshev evaluation and of its many-sums kernel ("Chebyshev evaluation"), on PN15QP880 with four parties,
uniform material:
  cheb15, cheb63, cheb255   Evaluator.EvaluateChebyshevNew on (-8, 8) with fused=True (the inner sums of the giant products in one
                            mkhe_ct_lincomb_multi) against fused=False (one mkhe_ct_lincomb each: only kernels that existed before the many-sums
                            kernel), dense coefficients; both legs build the powers with the same calls, and both include the host's encoding and
                            upload of the constants
  kernel                    mkhe_ct_lincomb_multi(nin, nout) against nout x mkhe_ct_lincomb(nin), constants resident, real weights (a Chebyshev
                            series) and complex ones, with the fused rescale, at (nin, nout) = (7, 7) and (15, 15) and at 6 and 14 limbs
  batch_kernel              mkhe_ct_lincomb_batch on nbatch = 2 and 8 items against nbatch calls of mkhe_ct_lincomb_multi, constants resident, real
                            weights, with the fused rescale, at (nin, nout) = (7, 7) and (15, 15) and 6 limbs
  batch_cheb31              BatchEvaluator.EvaluateChebyshevNew of degree 31 on B = 2 and 8 inputs against B evaluations on the single Evaluator
The two legs of a row give the same bits; nothing is compared here: tests/test_gpu_lincomb_multi.py, tests/test_gpu_chebyshev_e2e.py,
tests/test_gpu_lincomb_batch.py and tests/test_gpu_batch_polyeval.py pin that.
HIP events on mkhe_ctx_stream around each leg, the legs alternating, REPS repetitions each after WARM warm-ups.  Every leg runs in a process of its
own under its own `timeout`; the first failure stops the script.  Writes one JSON object (times in microseconds: median, min, quartiles; launch and
byte counts as derived in DESIGN.md) to --out and prints it.
Needs a GPU:  python tools/cheb_timing.py [--out FILE] [--reps N] [--legs a,b]"""
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
LEGS = {"cheb15": 300, "cheb63": 300, "cheb255": 400, "kernel": 300, "batch_kernel": 300, "batch_cheb31": 400}             # leg -> its time limit in seconds
IDS = ["p0", "p1", "p2", "p3"]
INTERVAL = (-8.0, 8.0)


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
    from mkhe_kklss_amd import mkckks, mkrlwe
    from mkhe_kklss_amd._abi import check, handle_array, lib
    hip = hip_runtime(lib)
    pset = H.PN15QP880
    Q, P, N = pset["Q"], pset["P"], 1 << pset["logN"]
    params = mkckks.Parameters(pset["logN"], Q, P, pset["scale"])
    rng = np.random.default_rng(15)
    for n in IDS:
        params.party_index(n)
    ev = mkckks.NewEvaluator(params)
    host = lambda limbs: np.stack([H.uniform_poly(rng, Q[:limbs], N) for _ in range(1 + len(IDS))])
    ct = lambda limbs: mkckks.NewCiphertext(params, IDS, limbs - 1, pset["scale"]).upload(host(limbs))
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

    poly = 8.0 * N * (1 + len(IDS))                               # bytes of one limb of a ciphertext
    rows = []
    if leg.startswith("cheb") or leg == "batch_cheb31":
        swk = lambda: np.stack([H.uniform_poly(rng, Q + P, N) for _ in range(len(Q))])        # (alpha = 1: one digit per limb of Q)
        rlk = mkrlwe.RelinearizationKeySet(params)
        for n in IDS:
            rlk.AddRelinearizationKey(mkrlwe.RelinearizationKey(params, n, swk(), swk(), swk()))
        params.AddCRS(-1, swk())
    if leg == "batch_cheb31":
        degree = 31
        coeffs = rng.uniform(-1, 1, degree + 1)
        for B in (2, 8):
            x = mkckks.BatchCiphertext([ct(len(Q)) for _ in range(B)])
            bev = mkckks.BatchEvaluator(params, B, ev=ev)
            batch, single = alternate(lambda: bev.EvaluateChebyshevNew(x, coeffs, INTERVAL, rlk),
                                      lambda: [ev.EvaluateChebyshevNew(c, coeffs, INTERVAL, rlk) for c in x.cts])
            rows.append(dict(leg=leg, ring="PN15QP880", parties=len(IDS), degree=degree, interval=INTERVAL, B=B, reps=reps, batch=batch, per_item=single,
                             ratio=round(batch["median_us"] / single["median_us"], 3)))
            print(json.dumps(rows[-1]), flush=True)
    elif leg.startswith("cheb"):
        degree = int(leg[4:])
        x = ct(len(Q))
        coeffs = rng.uniform(-1, 1, degree + 1)
        plan = mkckks.poly_eval_plan(degree)
        fused, plain = alternate(lambda: ev.EvaluateChebyshevNew(x, coeffs, INTERVAL, rlk, fused=True),
                                 lambda: ev.EvaluateChebyshevNew(x, coeffs, INTERVAL, rlk, fused=False))
        g, nin = plan.g, plan.m - 1
        Lc = len(Q) - 1 - 1 - (degree.bit_length() + 1) + 2 + 1       # limbs of the inner sums i >= 1 before their rescale (l_out + 2, plus one)
        rows.append(dict(leg=leg, ring="PN15QP880", parties=len(IDS), degree=degree, interval=INTERVAL, m=plan.m, g=g, reps=reps, fused=fused,
                         plain=plain, power_products=len(plan.products), giant_products=g - 1, inner_sum_limbs=Lc,
                         fused_calls=dict(mkhe_ct_lincomb_multi=1 if g > 1 else 0, mkhe_ct_lincomb=2 + len(plan.products)),
                         plain_calls=dict(mkhe_ct_lincomb=2 + len(plan.products) + g - 1),
                         sum_bytes_fused=poly * (nin * Lc + (g - 1) * (Lc - 1)), sum_bytes_plain=poly * (g - 1) * (nin * Lc + Lc - 1),
                         saved_us=round(plain["median_us"] - fused["median_us"], 1), ratio=round(fused["median_us"] / plain["median_us"], 3)))
        print(json.dumps(rows[-1]), flush=True)
    elif leg == "batch_kernel":
        L, Lc = lib(), 6
        ins = [[ct(Lc) for _ in range(15)] for _ in range(8)]
        outs = [[mkckks.NewCiphertext(params, IDS, Lc - 2, pset["scale"]) for _ in range(15)] for _ in range(8)]
        for nin, nout in ((7, 7), (15, 15)):
            res = lambda: [int(rng.integers(1, q)) for q in Q[:Lc]]
            block = np.array([[[res(), res()]] + [[res(), [0] * Lc] for _ in range(nin)] for _ in range(nout)], dtype=np.uint64)
            buf = mkckks._upload_consts(params, block)
            for nbatch in (2, 8):
                hin = [handle_array([c.h for c in ins[b][:nin]]) for b in range(nbatch)]
                hout = [handle_array([c.h for c in outs[b][:nout]]) for b in range(nbatch)]
                hin_all = handle_array([c.h for b in range(nbatch) for c in ins[b][:nin]])
                hout_all = handle_array([c.h for b in range(nbatch) for c in outs[b][:nout]])

                def lock_step():
                    check(L.mkhe_ct_lincomb_batch(params.ctx, nbatch, nin, hin_all, nout, buf.devptr(), 1, hout_all))

                def per_item():
                    for b in range(nbatch):
                        check(L.mkhe_ct_lincomb_multi(params.ctx, nin, hin[b], nout, buf.devptr(), 1, hout[b]))

                one, many = alternate(lock_step, per_item)
                nbytes = poly * nbatch * (nin * Lc + nout * (Lc - 1))
                rows.append(dict(leg=leg, ring="PN15QP880", parties=len(IDS), nbatch=nbatch, nin=nin, nout=nout, limbs=Lc, nb_rescale=1, weights="real",
                                 reps=reps, batch=one, per_item=many, launches=dict(batch=1, per_item=nbatch), bytes=nbytes,
                                 gbps=dict(batch=round(nbytes / one["median_us"] / 1e3, 1), per_item=round(nbytes / many["median_us"] / 1e3, 1)),
                                 ratio=round(one["median_us"] / many["median_us"], 3)))
                print(json.dumps(rows[-1]), flush=True)
    else:
        L = lib()
        for Lc in (6, 14):
            ins = [ct(Lc) for _ in range(15)]
            outs = [mkckks.NewCiphertext(params, IDS, Lc - 2, pset["scale"]) for _ in range(15)]
            for nin, nout in ((7, 7), (15, 15)):
                for kind in ("real", "complex"):
                    res = lambda: [int(rng.integers(1, q)) for q in Q[:Lc]]
                    block = np.array([[[res(), res()]] + [[res(), res() if kind == "complex" else [0] * Lc] for _ in range(nin)] for _ in range(nout)],
                                     dtype=np.uint64)
                    assert block.shape == (nout, nin + 1, 2, Lc)
                    buf = mkckks._upload_consts(params, block)
                    row_ptr = [C.c_void_p(buf.devptr().value + 8 * g * (nin + 1) * 2 * Lc) for g in range(nout)]
                    hin, hout = handle_array([c.h for c in ins[:nin]]), handle_array([c.h for c in outs[:nout]])

                    def fused_call():
                        check(L.mkhe_ct_lincomb_multi(params.ctx, nin, hin, nout, buf.devptr(), 1, hout))

                    def per_output():
                        for g in range(nout):
                            check(L.mkhe_ct_lincomb(params.ctx, nin, hin, row_ptr[g], 1, outs[g].h))

                    one, many = alternate(fused_call, per_output)
                    b_one, b_many = poly * (nin * Lc + nout * (Lc - 1)), poly * nout * (nin * Lc + Lc - 1)
                    rows.append(dict(leg=leg, ring="PN15QP880", parties=len(IDS), nin=nin, nout=nout, limbs=Lc, nb_rescale=1, weights=kind, reps=reps,
                                     one_launch=one, per_output=many, launches=dict(one_launch=1, per_output=nout),
                                     bytes=dict(one_launch=b_one, per_output=b_many),
                                     gbps=dict(one_launch=round(b_one / one["median_us"] / 1e3, 1), per_output=round(b_many / many["median_us"] / 1e3, 1)),
                                     ratio=round(one["median_us"] / many["median_us"], 3)))
                    print(json.dumps(rows[-1]), flush=True)
    for e in (e0, e1):
        hip.hipEventDestroy(e)
    params.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cheb_timing.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--legs", default=",".join(LEGS), help="comma-separated subset of " + ", ".join(LEGS))
    ap.add_argument("--leg", choices=sorted(LEGS), help="run this leg in this process and print its rows (what the script starts for every leg)")
    args = ap.parse_args()
    if args.reps < 10:
        raise SystemExit("at least 10 repetitions")
    if args.leg:
        print("ROWS " + json.dumps(run_leg(args.leg, args.reps)), flush=True)
        return
    rows = []
    for leg, limit in ((leg, LEGS[leg]) for leg in args.legs.split(",")):               # a fresh process per leg, each under its own time limit; the first failure ends the script
        out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--reps", str(args.reps)],
                             capture_output=True, text=True)
        sys.stdout.write(out.stdout)
        if out.returncode != 0:
            sys.stderr.write(out.stderr[-4000:])
            raise SystemExit("leg %s failed with status %d: stopping" % (leg, out.returncode))
        rows += json.loads([line for line in out.stdout.splitlines() if line.startswith("ROWS ")][-1][5:])
    try:
        device = subprocess.run(["rocminfo"], capture_output=True, text=True, timeout=60).stdout
    except (OSError, subprocess.TimeoutExpired):
        device = ""
    names = sorted({line.split(":", 1)[1].strip() for line in device.splitlines() if "Marketing Name" in line and "Instinct" in line})
    res = dict(device=names, host=os.uname().nodename,
               legs=dict(fused="EvaluateChebyshevNew(fused=True)", plain="EvaluateChebyshevNew(fused=False)",
                         one_launch="mkhe_ct_lincomb_multi(nin, nout)", per_output="nout x mkhe_ct_lincomb(nin)",
                         batch="mkhe_ct_lincomb_batch(nbatch, nin, nout) / BatchEvaluator.EvaluateChebyshevNew on B inputs",
                         per_item="nbatch x mkhe_ct_lincomb_multi(nin, nout) / B x Evaluator.EvaluateChebyshevNew"), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
