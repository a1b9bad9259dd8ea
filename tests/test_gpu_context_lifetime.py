"""Create, exercise, close -- three times over, MK-CKKS and MK-BFV (-m gpu): what a GPU run can catch of the ownership of a Context's device memory
(csrc/device_memory.h).  Free-memory readings of a shared device mean nothing and none is asserted: leaks are the business of
test_cpp_device_memory.py and test_device_memory_static.py.  A double free or a use after free on the paths that free -- the rollback of a lazy build,
the replaced maps of mkhe_ctx_set_owned, a scratch buffer that grows after its old block was used, the release of the whole context -- shows here as a
fault, or as bits that differ between two runs that must agree.

One party, logN = 10, three primes in Q and two in P: the smallest shapes that reach every owner (tables of init, keygen scratch, both encoders' lazy
tables, encryption / decryption scratch, hoist pools, the profiler's events).  Per cycle, with the same seeds every time:
GenDefaultCRS, key pair, relinearization key, one rotation key; EncryptMsgBatch (device encoder) of one message, then of four with the same first
message and samples; MulRelinNew and RotateNew on both first ciphertexts; Decrypt (device encoder).  MK-CKKS only: mkhe_ctx_set_owned with a subset of the
moduli and with none, twice; one MulRelinNew under the profiler."""
import ctypes as C

import numpy as np
import pytest

import harness as H
import harness_bfv as HB

pytestmark = pytest.mark.gpu

LOGN, N = 10, 1 << 10
CKKS, BFV = H.small_ckks(LOGN, 3), HB.small_bfv(LOGN, 3)
T = BFV["T"]
assert len(CKKS["Q"]) == len(BFV["Q"]) == 3 and len(CKKS["P"]) == len(BFV["P"]) == 2 and T == 65537


def centre(v):
    r = np.mod(np.asarray(v, dtype=np.int64), T)
    return np.where(r > T // 2, r - T, r)


def cycle(scheme):
    """one context from creation to close; every array a later cycle has to reproduce bit for bit"""
    from mkhe_kklss_amd import mkbfv, mkckks, mkrlwe
    from mkhe_kklss_amd._abi import check, lib
    ckks = scheme == "ckks"
    mk = mkckks if ckks else mkbfv
    params = mkckks.Parameters(LOGN, CKKS["Q"], CKKS["P"], CKKS["scale"]) if ckks else mkbfv.Parameters(LOGN, BFV["Q"], BFV["QMul"], BFV["P"], T)
    try:
        params.GenDefaultCRS(seed=1234)
        sampler = mkrlwe.HostSampler(np.random.default_rng(99), insecure_test_only=True)
        kgen = mkrlwe.NewKeyGenerator(params, sampler) if ckks else mkbfv.NewKeyGenerator(params, sampler)
        sk, pk = kgen.GenKeyPair("user0")
        skSet, rlk, rks = mkrlwe.NewSecretKeySet(), (mkrlwe if ckks else mkbfv).RelinearizationKeySet(params), mkrlwe.RotationKeySet()
        skSet.AddSecretKey(sk)
        rlk.AddRelinearizationKey(kgen.GenRelinearizationKey(sk, kgen.GenSecretKey("user0")))
        rks.AddRotationKey(kgen.GenRotationKey(1, sk))
        enc, dec, ev = mk.NewEncryptor(params, sampler, encoder="device"), mk.NewDecryptor(params, encoder="device"), mk.NewEvaluator(params)

        rng = np.random.default_rng(5)
        if ckks:
            values = [rng.uniform(-1, 1, N // 2) + 1j * rng.uniform(-1, 1, N // 2) for _ in range(4)]
        else:
            values = [rng.integers(-(T // 2), T // 2 + 1, N).astype(np.int64) for _ in range(4)]
        samples = np.stack([np.concatenate([sampler.ternary(N, 0.5)[None], sampler.gaussian(2, N)]) for _ in range(4)])
        msgs = [mk.Message(v) for v in values]
        one = enc.EncryptMsgBatch(msgs[:1], pk, samples[:1])          # sizes the encryption scratch and uses it ...
        four = enc.EncryptMsgBatch(msgs, pk, samples)                 # ... and the larger batch replaces the used blocks
        assert len(one) == 1 and len(four) == 4

        def chain(ct):
            prod = ev.MulRelinNew(ct, ct, rlk)
            return dict(ct=ct.download(), prod=prod.download(), rot=ev.RotateNew(prod, 1, rks).download(), dec=np.asarray(dec.Decrypt(prod, skSet).Value))

        out, again = chain(one[0]), chain(four[0])
        for k in out:
            assert out[k].shape == again[k].shape and (out[k] == again[k]).all(), "%s: %s after the batch of four differs from the single-message run" % (scheme, k)
        if not ckks:
            assert out["dec"].dtype == np.int64 and (out["dec"] == centre(values[0] ** 2)).all()
        else:
            mtot = len(CKKS["Q"]) + len(CKKS["P"])
            own = (C.c_int * 3)(0, 2, mtot - 1)
            for _ in range(2):
                check(lib().mkhe_ctx_set_owned(params.ctx, own, 3))
                check(lib().mkhe_ctx_set_owned(params.ctx, own, 0))
            ncls = lib().mkhe_prof_nclass()
            ms, cnt, byt = (C.c_double * ncls)(), (C.c_long * ncls)(), (C.c_double * ncls)()
            check(lib().mkhe_prof_enable(params.ctx, 1))
            timed = ev.MulRelinNew(one[0], one[0], rlk)
            check(lib().mkhe_prof_collect(params.ctx, ms, cnt, byt))
            assert sum(cnt) > 0
            out["timed"] = timed.download()
            assert (out["timed"] == out["prod"]).all(), "ckks: MulRelinNew under the profiler, after set_owned and back, differs"
        return out
    finally:
        params.close()


@pytest.mark.parametrize("scheme", ["ckks", "bfv"])
def test_three_cycles_of_create_exercise_close(scheme):
    first = cycle(scheme)
    cycle(scheme)
    third = cycle(scheme)
    assert sorted(first) == sorted(third)
    for k in first:
        assert first[k].shape == third[k].shape and (first[k] == third[k]).all(), "%s: %s of cycle 3 differs from cycle 1" % (scheme, k)
