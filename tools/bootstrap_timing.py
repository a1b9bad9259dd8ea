"""Device time of mkckks.Bootstrapper.BootstrapNew and of mkhe_ct_mod_raise alone ("Bootstrapping"), on PN16QP1761 (N = 2^16, 34 moduli of Q,
ratio = 2^10), uniform material -- the times do not depend on the values:
  modraise       mkhe_ct_mod_raise of a level-0 ciphertext to the top, 2 and 4 parties, against its byte count 8 N (1 + k) (1 + L)
  boot-S-k       one BootstrapNew at logSlots = S with k parties, from level 0 to level 33 - Depth(); stages timed apart in the same run: ModRaise +
                 SubSum, CoeffsToSlots, the two EvalMod, SlotsToCoeffs
  boot-S-k@A/B   the same with Bootstrapper(.., factors=(A, B)), the groups of each transform joined by dots: boot-10-2@5.5/5.5, boot-15-2@5.5.5/5.5.5
  pair-S-k       BootstrapNew(pair=True), the two halves through EvalMod as a batch of two, against BootstrapNew(pair=False), alternating in one process
Every party's rotation keys are ONE uniform switching key shared by all its rotation indices (83 indices at logSlots = 10 would otherwise be 28 GB
per party); the CRS slots are expanded on the device.  The transforms are encoded in the warm-ups and are not part of the times.
HIP events on mkhe_ctx_stream around each call, REPS repetitions after WARM warm-ups; a call's time includes the host's constant uploads between
its launches.  Every leg runs in a process of its own under its own `timeout`; the first failure stops the script, what was measured is kept.
Writes one JSON object (times in microseconds: median, min, quartiles) to --out and prints it.
Needs a GPU:  python tools/bootstrap_timing.py [--out FILE] [--reps N] [--legs a,b]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARM = 2
LEGS = {"modraise": 120, "boot-4-2": 240, "boot-4-4": 300, "boot-10-2": 400, "boot-10-4": 400, "pair-4-2": 300}      # leg -> its time limit in seconds
FACTORED = {"boot-10-2": 300, "boot-15-2": 400}          # legs that only exist with @A/B (more than 1024 slots), and the limit of a factored leg


def split_leg(leg):
    """'boot-10-2@5.5/5.5' -> ('boot-10-2', ((5, 5), (5, 5))); a leg without '@' -> (leg, None)"""
    base, _, spec = leg.partition("@")
    if not spec:
        return base, None
    groups = tuple(tuple(int(g) for g in part.split(".")) for part in spec.split("/"))
    if len(groups) != 2 or not base.startswith("boot-"):
        raise SystemExit("factors go on a boot-S-k leg as @A/B, as in boot-10-2@5.5/5.5: %r" % leg)
    return base, groups


def time_limit(leg):
    base, groups = split_leg(leg)
    table = LEGS if groups is None else dict(LEGS, **FACTORED)
    if base not in table:
        raise SystemExit("unknown leg %r" % leg)
    return table[base]


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
    from mkhe_kklss_amd._abi import check, lib
    hip = hip_runtime(lib)
    pset = H.PN16QP1761
    Q, P, N = pset["Q"], pset["P"], 1 << pset["logN"]
    rng = np.random.default_rng(16)
    e0, e1 = C.c_void_p(), C.c_void_p()
    for e in (e0, e1):
        assert hip.hipEventCreate(C.byref(e)) == 0

    def timed(stream, f):
        assert hip.hipEventRecord(e0, stream) == 0
        out = f()
        assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        return ms.value * 1e3, out

    def level0(params, ids):
        host = np.stack([H.uniform_poly(rng, Q[:1], N) for _ in range(1 + len(ids))])
        return mkckks.NewCiphertext(params, ids, 0, pset["scale"]).upload(host)

    rows = []
    if leg == "modraise":
        params = mkckks.Parameters(pset["logN"], Q, P, pset["scale"], logSlots=4)
        stream, top = C.c_void_p(params.stream()), len(Q) - 1
        for k in (2, 4):
            ids = ["p%d" % i for i in range(k)]
            ct, out = level0(params, ids), mkckks.NewCiphertext(params, ids, top, pset["scale"])
            call = lambda: check(lib().mkhe_ct_mod_raise(params.ctx, ct.h, out.h))
            for _ in range(WARM):
                timed(stream, call)
            t = stat([timed(stream, call)[0] for _ in range(reps)])
            nbytes = 8.0 * N * (1 + k) * (1 + len(Q))
            rows.append(dict(leg=leg, ring="PN16QP1761", parties=k, limbs_out=len(Q), reps=reps, bytes=nbytes, gbps=round(nbytes / t["median_us"] / 1e3, 1), **t))
            print(json.dumps(rows[-1]), flush=True)
        params.close()
    else:
        base, factors = split_leg(leg)
        logSlots, k = (int(v) for v in base.split("-")[1:])
        ids = ["p%d" % i for i in range(k)]
        params = mkckks.Parameters(pset["logN"], Q, P, pset["scale"], logSlots=logSlots)
        stream = C.c_void_p(params.stream())
        boot = mkckks.Bootstrapper(params, factors=factors)
        for idx in [-1, -2] + boot.Rotations():
            params.AddCRS(idx, seed=16)
        swk = lambda: np.stack([H.uniform_poly(rng, Q + P, N) for _ in range(params.Beta(params.MaxLevel()))])
        rlk, rks, cks = mkrlwe.RelinearizationKeySet(params), mkrlwe.RotationKeySet(), mkrlwe.ConjugationKeySet()
        for name in ids:
            rlk.AddRelinearizationKey(mkrlwe.RelinearizationKey(params, name, swk(), swk(), swk()))
            shared = mkrlwe.ConjugationKey(params, name, swk())
            cks.AddConjugationKey(shared)
            for r in boot.Rotations():
                rks.AddRotationKey(types.SimpleNamespace(ID=name, RotIdx=r, Value=shared.Value))
        ev, ct = mkckks.NewEvaluator(params), level0(params, ids)
        ratio = Q[0] / pset["scale"]

        def staged():
            t0, sub = timed(stream, lambda: ev.SubSumNew(ev.ModRaiseNew(ct), rks))
            sub.Scale = sub.Scale * (boot.K * ratio)
            t1, (lo, hi) = timed(stream, lambda: boot.CoeffsToSlotsNew(sub, rks, cks, ev))
            t2, (lo, hi) = timed(stream, lambda: (boot.EvalModNew(lo, rlk, ratio, ev), boot.EvalModNew(hi, rlk, ratio, ev)))
            t3, out = timed(stream, lambda: boot.SlotsToCoeffsNew(lo, hi, rks, ev))
            assert out.Level() == params.MaxLevel() - boot.Depth()
            return t0, t1, t2, t3

        common = dict(leg=leg, ring="PN16QP1761", logSlots=logSlots, parties=k, level_in=params.MaxLevel(), level_out=params.MaxLevel() - boot.Depth(), reps=reps)
        if leg.startswith("pair"):
            legs = {name: (lambda p=p: boot.BootstrapNew(ct, rlk, rks, cks, ev, pair=p)) for name, p in (("pair", True), ("default", False))}
            for _ in range(WARM):
                for f in legs.values():
                    timed(stream, f)
            t = {name: [] for name in legs}
            for _ in range(reps):
                for name, f in legs.items():
                    t[name].append(timed(stream, f)[0])
            t = {name: stat(v) for name, v in t.items()}
            rows.append(dict(common, pair=t["pair"], default=t["default"], ratio=round(t["pair"]["median_us"] / t["default"]["median_us"], 3)))
        else:
            whole = lambda: boot.BootstrapNew(ct, rlk, rks, cks, ev)
            for _ in range(WARM):
                timed(stream, whole)
                staged()
            total = stat([timed(stream, whole)[0] for _ in range(reps)])
            parts = np.array([staged() for _ in range(reps)])
            lts = [t.transforms if factors else [t] for t in (boot._lts[0], boot._lts[1])]          # encoded in the warm-ups
            plans = [[lt.plan for lt in group] for group in lts]
            shape = dict(factors=factors, depth=boot.Depth(),
                         diagonals=[[len(lt.order) for lt in group] for group in lts],
                         key_switches=[sum(1 for p in group for r in p.babies + p.giants if r) for group in plans],
                         plaintext_bytes=[sum(8 * N * (lt.level + 1) * len(lt.order) for lt in group) for group in lts])
            rows.append(dict(common, **shape, rotations=len(boot.Rotations()), bootstrap=total,
                             stages={name: stat(parts[:, i]) for i, name in enumerate(["modraise_subsum", "coeffs_to_slots", "eval_mod_x2", "slots_to_coeffs"])}))
        print(json.dumps(rows[-1]), flush=True)
        params.close()
    for e in (e0, e1):
        hip.hipEventDestroy(e)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bootstrap_timing.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--legs", default=",".join(LEGS), help="comma-separated subset of " + ", ".join(LEGS))
    ap.add_argument("--leg", help="run this leg in this process and print its rows (what the script starts for every leg)")
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("at least 5 repetitions")
    for leg in [args.leg] if args.leg else args.legs.split(","):
        time_limit(leg)
    if args.leg:
        print("ROWS " + json.dumps(run_leg(args.leg, args.reps)), flush=True)
        return
    rows, failed = [], None
    for leg in args.legs.split(","):              # a fresh process per leg, each under its own time limit; the first failure ends the measurements
        out = subprocess.run(["timeout", "-k", "10", str(time_limit(leg)), sys.executable, os.path.abspath(__file__), "--leg", leg, "--reps", str(args.reps)],
                             capture_output=True, text=True)
        sys.stdout.write(out.stdout)
        if out.returncode != 0:
            sys.stderr.write(out.stderr[-4000:])
            failed = "leg %s failed with status %d: stopping" % (leg, out.returncode)
            break
        rows += json.loads([line for line in out.stdout.splitlines() if line.startswith("ROWS ")][-1][5:])
    try:
        device = subprocess.run(["rocminfo"], capture_output=True, text=True, timeout=60).stdout
    except (OSError, subprocess.TimeoutExpired):
        device = ""
    names = sorted({line.split(":", 1)[1].strip() for line in device.splitlines() if "Marketing Name" in line and "Instinct" in line})
    res = dict(device=names, warmups=WARM, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    if failed:
        raise SystemExit(failed)


if __name__ == "__main__":
    main()
