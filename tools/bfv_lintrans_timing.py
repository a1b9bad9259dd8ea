"""Device time of the MK-BFV plaintext linear transform, fused against fused=False ("MK-BFV plaintext linear transform"): two parties,
the 16 diagonals 0 .. 15 (n1 = 4: 3 baby and 3 giant rotations), nbatch 1 and 8, at small_bfv(11, 3) and at the full BFV set PN15QP880.  Keys are
generated on the device, the inputs are real encryptions, and the noise budgets of input and result are printed.  Each pair computes the same
ciphertexts, which is checked first.  HIP events on mkhe_ctx_stream around each leg, the two legs of a pair alternating, in one process, after
warm-ups of both; median of 20.  Writes one JSON object (times in microseconds) to --out and prints it.
Needs a GPU:  python tools/bfv_lintrans_timing.py [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import harness_bfv as HB  # noqa: E402
from mkhe_kklss_amd import mkbfv, mkrlwe  # noqa: E402
from mkhe_kklss_amd._abi import lib  # noqa: E402

DIAGONALS, REPS, WARM, NAMES = 16, 20, 3, ["user0", "user1"]


def hip_runtime():
    """the HIP runtime the engine library is linked to, as loaded in this process"""
    lib()
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime in this process")


def measure(name, pset, hip):
    T, N = pset["T"], 1 << pset["logN"]
    n = N // 2
    params = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], T)
    rng = np.random.default_rng(pset["logN"])
    diag = {k: rng.integers(-(T // 2), T // 2 + 1, (2, n)).astype(np.int64) for k in range(DIAGONALS)}
    lt = mkbfv.LinearTransform(params, diag)
    for idx in [0] + lt.Rotations():
        params.AddCRS(idx, seed=99)
    sampler = mkrlwe.HostSampler(np.random.default_rng(2026), insecure_test_only=True)
    kgen, rks, pks, sks = mkbfv.NewKeyGenerator(params, sampler), mkrlwe.RotationKeySet(), {}, mkrlwe.NewSecretKeySet()
    for who in NAMES:
        sk, pks[who] = kgen.GenKeyPair(who)
        sks.AddSecretKey(sk)
        for r in lt.Rotations():
            rks.AddRotationKey(kgen.GenRotationKey(r, sk))
    enc, dec, ev = mkbfv.NewEncryptor(params, sampler, encoder="device"), mkbfv.NewDecryptor(params, encoder="device"), mkbfv.NewEvaluator(params)

    def fresh():
        z = rng.integers(-(T // 2), T // 2 + 1, N).astype(np.int64)
        return ev.AddNew(enc.EncryptMsgNew(mkbfv.Message(z), pks[NAMES[0]]), enc.EncryptMsgNew(mkbfv.Message(np.zeros(N, dtype=np.int64)), pks[NAMES[1]]))

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

    stat = lambda t: dict(median_us=round(float(np.median(t)), 1), min_us=round(float(min(t)), 1), max_us=round(float(max(t)), 1))
    out = dict(shape=dict(logN=pset["logN"], limbs=len(pset["Q"]), parties=len(NAMES), diagonals=DIAGONALS, n1=lt.plan.n1,
                          rotations=len(lt.Rotations())))
    for nbatch in (1, 8):
        cts, res = [fresh() for _ in range(nbatch)], {}

        def leg(fused):
            def run():
                res[fused] = ev.LinearTransformBatch(cts, lt, rks, fused=fused)
            return run

        fused, chain = leg(True), leg(False)
        fused(); chain()
        for a, b in zip(res[True], res[False]):
            assert (a.download() == b.download()).all(), "the fused transform and the chain disagree"
        budgets = dict(input=dec.NoiseBudget(cts[0], sks), result=min(dec.NoiseBudget(c, sks) for c in res[True]))
        for _ in range(WARM):
            timed(fused); timed(chain)
        tf, tc = [], []
        for _ in range(REPS):
            tf.append(timed(fused)); tc.append(timed(chain))
        out["nbatch%d" % nbatch] = dict(fused=stat(tf), chain=stat(tc), ratio=round(float(np.median(tf) / np.median(tc)), 3), noise_budget_bits=budgets)
        print(name, "nbatch", nbatch, json.dumps(out["nbatch%d" % nbatch]), flush=True)
    for e in (e0, e1):
        hip.hipEventDestroy(e)
    params.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bfv_lintrans_timing.json"))
    args = ap.parse_args()
    hip = hip_runtime()
    out = {"small_bfv_11_3": measure("small_bfv(11, 3)", HB.small_bfv(11, 3), hip), "PN15QP880": measure("PN15QP880", HB.BFV_PN15QP880, hip)}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
