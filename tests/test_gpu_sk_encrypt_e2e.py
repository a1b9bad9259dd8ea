"""Secret-key encryption with a seeded c1 end to end (-m gpu), N = 2^10.

mkckks: two parties each encrypt their slots under their own secret key (EncryptMsgSeeded); what travels is download() -- c0, 32 bytes and a
nonce, half the bytes of the ciphertext -- into a SeededCiphertext on a SECOND Parameters object, the evaluator's, whose Expand() gives, bit for
bit, what the encryptor's own EncryptMsgBatch gives on the same seed, nonce and samples.  The product of the two expanded ciphertexts decrypts
within the slot tolerance tests/test_gpu_encdec_e2e.py applies to the public-key path (Scenario.precision_bound, 12 bits for MulRelin): the noise
of a secret-key ciphertext is e alone, not larger.

mkbfv: the same round trip; Decrypt(MulRelinNew(..)) is a * b mod T exactly, and a collective refresh (mkbfv.Refresher) of an sk-encrypted
ciphertext still decrypts exactly."""
import types

import numpy as np
import pytest

import harness as H
import harness_bfv as HB
from scenario import Scenario

pytestmark = pytest.mark.gpu

LOGN = 10
N = 1 << LOGN
NAMES = ["user0", "user1"]


def _max_log2_err(a, b):
    d = np.abs(np.asarray(a) - np.asarray(b))
    return float(np.log2(max(d.real.max(), d.imag.max(), 1e-300)))


def _travel(sc, make):
    """the wire: download on the sender, a new SeededCiphertext on the receiver's Parameters, upload -> (the receiver's object, bytes moved)"""
    c0, key, nonce = sc.download()
    assert isinstance(key, bytes) and len(key) == 32 and c0.dtype == np.uint64
    return make().upload(c0.copy(), key, nonce), c0.nbytes + len(key) + 8


def test_two_parties_ship_half_size_ckks_ciphertexts_to_an_evaluator():
    from mkhe_kklss_amd import mkckks, mkrlwe
    from mkhe_kklss_amd._abi import MkheError
    pset = H.small_ckks(LOGN, nq=4)
    scale, n = pset["scale"], N // 2
    params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], scale)              # the parties' (one process stands for both)
    evaluator = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], scale)           # the evaluator's: another context
    evaluator.GenDefaultCRS(seed=4325)
    kgen = mkrlwe.NewKeyGenerator(params, mkrlwe.HostSampler(np.random.default_rng(2032), insecure_test_only=True))
    rng = np.random.default_rng(59)
    level = params.MaxLevel()
    sks, secrets, zs, arrived, own = {}, {}, {}, {}, {}
    for i, p in enumerate(NAMES):
        secrets[p] = rng.integers(-1, 2, N).astype(np.int32)
        sks[p] = kgen.GenSecretKey(p, secrets[p])
        zs[p] = [np.full(n, complex(0.1, 1.0) / 2) + rng.uniform(-0.05, 0.05, n) for _ in range(2)]      # mkckks_test.go:330-340
        msgs = [mkckks.Message(z) for z in zs[p]]
        seed, e_key = bytes(range(i, 32 + i)), bytes(range(100 + i, 132 + i))
        # a HostSampler (e drawn on the host) for one party, a DeviceSampler (e formed on the device) for the other; device encoder for one
        sampler = lambda: (mkrlwe.HostSampler(np.random.default_rng(77), insecure_test_only=True) if i == 0 else mkrlwe.DeviceSampler(e_key, insecure_test_only=True))
        enc = mkckks.NewSecretKeyEncryptor(params, sks[p], sampler(), encoder="host" if i == 0 else "device", seed=seed, insecure_test_only=True)
        sc = enc.EncryptMsgSeeded(msgs)
        assert sc.ID == p and sc.count == 2 and sc.Level() == level and sc.Nonce == 0 and sc.Key == seed and enc.counter == 1
        arrived[p], moved = _travel(sc, lambda: mkckks.SeededCiphertext(evaluator, p, level, 2, scale))
        full = 2 * 2 * (level + 1) * N * 8
        print("%s: %d bytes on the wire for 2 ciphertexts of %d" % (p, moved, full))
        assert moved == full // 2 + 40
        # the encryptor's own EncryptMsgBatch on the same seed, nonce and samples
        again = mkckks.NewSecretKeyEncryptor(params, sks[p], sampler(), encoder="host" if i == 0 else "device", seed=seed, insecure_test_only=True)
        own[p] = again.EncryptMsgBatch(msgs)
    cts = {}
    for p in NAMES:
        cts[p] = arrived[p].Expand()
        assert len(cts[p]) == 2
        for c, mine in zip(cts[p], own[p]):
            assert isinstance(c, mkckks.Ciphertext) and c.params is evaluator and c.ids == [p] and c.Level() == level and c.Scale == scale
            assert (c.download() == mine.download()).all()      # bit for bit
        assert arrived[p].Expand() is cts[p]                    # expanding twice is the same ciphertexts
        with pytest.raises(MkheError, match="already expanded"):
            arrived[p].upload(np.zeros((2, level + 1, N), dtype=np.uint64), bytes(32), 0)
        assert arrived[p].Key == bytes(range(NAMES.index(p), 32 + NAMES.index(p))) and arrived[p].Nonce == 0       # ... and the refusal left the seed alone
    lower = arrived["user0"].Expand(level=1)                    # a lower level: the leading limbs of both polynomials
    assert lower[0].Level() == 1 and (lower[1].download() == own["user0"][1].download()[:, :2]).all()

    # the evaluator computes on what arrived.  This process stands for everyone: the same secrets, as keys on the evaluator's context, make the
    # relinearisation keys and decrypt
    rlk = mkrlwe.RelinearizationKeySet(evaluator)
    kgen_ev = mkrlwe.NewKeyGenerator(evaluator, mkrlwe.HostSampler(np.random.default_rng(2034), insecure_test_only=True))
    skSet_ev = mkrlwe.NewSecretKeySet()
    for p in NAMES:
        sk = kgen_ev.GenSecretKey(p, secrets[p])
        skSet_ev.AddSecretKey(sk)
        rlk.AddRelinearizationKey(kgen_ev.GenRelinearizationKey(sk, kgen_ev.GenSecretKey(p)))
    ev, dec = mkckks.NewEvaluator(evaluator), mkckks.NewDecryptor(evaluator)
    bound = lambda extra: Scenario.precision_bound(types.SimpleNamespace(scale=scale, logN=LOGN), extra)
    for k in range(2):
        a, b = cts["user0"][k], cts["user1"][k]
        assert _max_log2_err(dec.Decrypt(a, skSet_ev).Value, zs["user0"][k]) <= bound(8)
        res = ev.MulRelinNew(a, b, rlk)
        err = _max_log2_err(dec.Decrypt(res, skSet_ev).Value, zs["user0"][k] * zs["user1"][k])
        print("MulRelinNew of two expanded ciphertexts: log2 error %.2f (bound %.2f)" % (err, bound(12)))
        assert res.ids == NAMES and err <= bound(12)
    params.close()
    evaluator.close()


def test_two_parties_ship_half_size_bfv_ciphertexts_and_refresh_one():
    from mkhe_kklss_amd import mkbfv, mkrlwe
    pset = HB.small_bfv(LOGN, 3)
    T = pset["T"]
    centre = lambda v: np.where(np.mod(v, T) > T // 2, np.mod(v, T) - T, np.mod(v, T))
    params = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], T)
    evaluator = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], T)
    evaluator.GenDefaultCRS(seed=4326)
    kgen = mkbfv.NewKeyGenerator(evaluator, mkrlwe.HostSampler(np.random.default_rng(2033), insecure_test_only=True))
    kgen_p = mkbfv.NewKeyGenerator(params, mkrlwe.HostSampler(np.random.default_rng(2033), insecure_test_only=True))
    rng = np.random.default_rng(61)
    sks, pks, skSet, rlk, ms, cts = {}, {}, mkrlwe.NewSecretKeySet(), mkbfv.RelinearizationKeySet(evaluator), {}, {}
    for i, p in enumerate(NAMES):
        secret = rng.integers(-1, 2, N).astype(np.int32)
        sks[p] = kgen.GenSecretKey(p, secret)                   # on the evaluator's context: decryption, relinearisation and the refresh run there
        pks[p] = kgen.GenPublicKey(sks[p])
        mine = kgen_p.GenSecretKey(p, secret)                   # the same secret as a key on the party's context
        skSet.AddSecretKey(sks[p])
        rlk.AddRelinearizationKey(kgen.GenRelinearizationKey(sks[p], kgen.GenSecretKey(p)))
        ms[p] = rng.integers(-(T // 2), T // 2 + 1, N).astype(np.int64)
        sampler = mkrlwe.DeviceSampler() if i == 0 else None    # None: the default HostSampler, os.urandom
        enc = mkbfv.NewSecretKeyEncryptor(params, mine, sampler, encoder="device" if i == 0 else "host")
        sc = enc.EncryptMsgSeeded([mkbfv.Message(ms[p])])
        arrived, moved = _travel(sc, lambda: mkbfv.SeededCiphertext(evaluator, p, 1))
        assert moved == 3 * N * 8 + 40
        cts[p] = arrived.Expand()[0]
        assert isinstance(cts[p], mkbfv.Ciphertext) and cts[p].ids == [p] and cts[p].Level() == evaluator.MaxLevel()
        assert (cts[p].download()[0] == sc.download()[0][0]).all() and (cts[p].download() == sc.Expand()[0].download()).all()
    ev, dec = mkbfv.NewEvaluator(evaluator), mkbfv.NewDecryptor(evaluator, encoder="device")
    for p in NAMES:
        assert (dec.Decrypt(cts[p], skSet).Value == ms[p]).all()
    prod = ev.MulRelinNew(cts["user0"], cts["user1"], rlk)
    assert prod.ids == NAMES and (dec.Decrypt(prod, skSet).Value == centre(ms["user0"] * ms["user1"])).all()       # a * b mod T, exactly

    # a collective refresh of an sk-encrypted ciphertext (one party): the flood 20 bits above its noise, |e| <= 19
    ref, p = mkbfv.NewRefresher(evaluator), "user1"
    flood_bits = (19).bit_length() + 20
    assert flood_bits <= ref.MaxFloodBits(1)
    sh = ref.ShareNew(cts[p], sks[p], pks[p], flood_bits, mkrlwe.DeviceSampler())
    fresh = ref.MergeNew(cts[p], [sh])
    assert fresh.ids == [p] and (dec.Decrypt(fresh, skSet).Value == ms[p]).all()
    params.close()
    evaluator.close()
