"""Device time of a plaintext linear transform, fused and as the chains it replaces ("Plaintext linear transform"), on N = 2^14, 8 limbs,
4 parties, 64 diagonals 0 .. 63 with n1 = 8 (8 babies, 8 giants):
  dot        mkhe_ct_ptxt_dot(8 inputs, 8 giants, all 64 plaintexts present)
  dot chain  64 x mkhe_ct_mul_ptxt + 8 x mkhe_ct_sum on the coefficient-domain plaintexts
  transform  Evaluator.LinearTransformNew(fused=True) against fused=False, device keygen for the 14 rotation keys per party
Each pair computes the same ciphertexts, which is checked first.  HIP events on mkhe_ctx_stream around each leg, the two legs of a pair alternating,
in one process, after warm-ups of both.  Writes one JSON object (times in microseconds, the byte model of the middle kernel) to --out and prints it.
--kernel-only N: N calls of `dot` and nothing else, for a kernel trace in a run of its own (rocprofv3 --kernel-trace --stats -- python tools/..).
Needs a GPU:  python tools/lintrans_timing.py [--out FILE]"""
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
from mkhe_kklss_amd import mkckks, mkrlwe  # noqa: E402
from mkhe_kklss_amd._abi import check, handle_array, lib  # noqa: E402

LOGN, LIMBS, PARTIES, N1, GIANTS, REPS_DOT, REPS_LT, WARM = 14, 8, 4, 8, 8, 30, 10, 3


def hip_runtime():
    """the HIP runtime the engine library is linked to, as loaded in this process"""
    lib()
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime in this process")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lintrans_timing.json"))
    ap.add_argument("--kernel-only", type=int, default=0)
    args = ap.parse_args()
    pset = H.small_ckks(LOGN, nq=LIMBS)
    Q, N, n = pset["Q"], 1 << LOGN, 1 << (LOGN - 1)
    params = mkckks.Parameters(LOGN, Q, pset["P"], pset["scale"])
    rng = np.random.default_rng(14)
    ids = ["p%d" % i for i in range(PARTIES)]
    level, nnz, L, ctx = LIMBS - 1, N1 * GIANTS, lib(), params.ctx
    new = lambda: mkrlwe.NewCiphertext(params, ids, level)
    uniform = lambda: np.stack([H.uniform_poly(rng, Q, N) for _ in range(1 + PARTIES)])

    # ---- the dot product on uniform residues
    ins = [new().upload(uniform()) for _ in range(N1)]
    pt = mkrlwe.DeviceLimbs(params, nnz, LIMBS).upload(np.stack([H.uniform_poly(rng, Q, N) for _ in range(nnz)]))
    ptntt = mkrlwe.DeviceLimbs(params, nnz, LIMBS)
    check(L.mkhe_ptxt_prepare(ctx, LIMBS, nnz, pt.devptr(), ptntt.devptr()))
    outs, prods, sums = [new() for _ in range(GIANTS)], [new() for _ in range(N1)], [new() for _ in range(GIANTS)]
    hin, hout, hprods = handle_array([c.h for c in ins]), handle_array([c.h for c in outs]), handle_array([c.h for c in prods])
    masks = (C.c_uint32 * GIANTS)(*[(1 << N1) - 1] * GIANTS)
    words = LIMBS * N

    def dot():
        check(L.mkhe_ct_ptxt_dot(ctx, N1, hin, GIANTS, masks, ptntt.devptr(), LIMBS, hout))

    def dot_chain():
        for g in range(GIANTS):
            for b in range(N1):
                check(L.mkhe_ct_mul_ptxt(ctx, ins[b].h, C.c_void_p(pt.devptr().value + 8 * words * (g * N1 + b)), prods[b].h))
            check(L.mkhe_ct_sum(ctx, N1, hprods, sums[g].h))

    if args.kernel_only:
        for _ in range(args.kernel_only):
            dot()
        check(L.mkhe_ctx_sync(ctx))
        params.close()
        return
    dot(); dot_chain()
    for a, b in zip(outs, sums):
        assert (a.download() == b.download()).all(), "mkhe_ct_ptxt_dot and the chain disagree"

    # ---- the whole transform on a ciphertext under device-generated keys
    params.GenDefaultCRS(seed=4321)
    sampler = mkrlwe.HostSampler(np.random.default_rng(2025), insecure_test_only=True)
    kgen, rks, ev = mkrlwe.NewKeyGenerator(params, sampler), mkrlwe.RotationKeySet(), mkckks.NewEvaluator(params)
    diag = {k: np.exp(2j * np.pi * rng.uniform(0, 1, n)) * rng.uniform(0, 1, n) for k in range(nnz)}
    lt = mkckks.LinearTransform(params, diag, level, n1=N1, keep_coeff=True)
    sks = [kgen.GenSecretKey(i) for i in ids]
    for r in lt.Rotations():
        if r not in params.CRS:
            params.AddCRS(r, seed=4321)
        for sk in sks:
            rks.AddRotationKey(kgen.GenRotationKey(r, sk))
    ct = mkckks.NewCiphertext(params, ids, level, params.Scale()).upload(uniform())
    res = {}

    def transform(fused):
        def run():
            res[fused] = ev.LinearTransformNew(ct, lt, rks, fused=fused)
        return run

    fused, chain = transform(True), transform(False)
    fused(); chain()
    assert (res[True].download() == res[False].download()).all(), "the fused transform and the chain disagree"

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

    def pair(f, g, reps):
        for _ in range(WARM):
            timed(f); timed(g)
        tf, tg = [], []
        for _ in range(reps):
            tf.append(timed(f)); tg.append(timed(g))
        return tf, tg

    stat = lambda t: dict(median_us=round(float(np.median(t)), 2), min_us=round(float(min(t)), 2), max_us=round(float(max(t)), 2))
    td, tdc = pair(dot, dot_chain, REPS_DOT)
    tl, tlc = pair(fused, chain, REPS_LT)
    for e in (e0, e1):
        hip.hipEventDestroy(e)
    np_, nrot = 1 + PARTIES, len(lt.Rotations())
    out = dict(shape=dict(logN=LOGN, limbs=LIMBS, parties=PARTIES, diagonals=nnz, n1=N1, giants=GIANTS),
               dot=dict(stat(td), launches=3, reps=REPS_DOT,
                        kernel_compulsory_bytes=8 * N * LIMBS * (np_ * N1 + nnz + np_ * GIANTS),
                        kernel_bytes_with_rereads=8 * N * LIMBS * (np_ * N1 + np_ * nnz + np_ * GIANTS)),
               dot_chain=dict(stat(tdc), launches=4 * nnz + GIANTS, reps=REPS_DOT),
               dot_ratio=round(float(np.median(td) / np.median(tdc)), 3),
               transform=dict(stat(tl), key_switches=nrot, reps=REPS_LT),
               transform_chain=dict(stat(tlc), key_switches=nrot, reps=REPS_LT),
               transform_ratio=round(float(np.median(tl) / np.median(tlc)), 3))
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    params.close()


if __name__ == "__main__":
    main()
