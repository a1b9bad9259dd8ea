"""Everything on the device (-m gpu): keygen -> EncryptMsgNew -> AddNew / MulRelinNew / RotateNew -> Decrypt with the default
HostSampler (seeded, insecure_test_only=True); no key, sample or ciphertext is made by the host harness.  The results are within
the reference's precision bounds (mkckks_test.go:221,357: Scenario.precision_bound with the extras of test_reference_properties.py:
8 bits for encrypt / decrypt, additions and rotations, 12 for MulRelin) of the plaintext computation."""
import types

import numpy as np
import pytest

import harness as H
from scenario import Scenario

pytestmark = pytest.mark.gpu

PSET = H.small_ckks(11, 4)


def _max_log2_err(a, b):
    d = np.abs(np.asarray(a) - np.asarray(b))
    return float(np.log2(max(d.real.max(), d.imag.max(), 1e-300)))


def bound(extra):
    return Scenario.precision_bound(types.SimpleNamespace(scale=PSET["scale"], logN=PSET["logN"]), extra)


@pytest.fixture(scope="module", params=[2, 4])
def world(request):
    from mkhe_kklss_amd import mkckks, mkrlwe
    k = request.param
    params = mkckks.Parameters(PSET["logN"], PSET["Q"], PSET["P"], PSET["scale"])
    params.GenDefaultCRS(seed=1234 + k)
    sampler = mkrlwe.HostSampler(np.random.default_rng(99 + k), insecure_test_only=True)
    kgen = mkrlwe.NewKeyGenerator(params, sampler)
    w = types.SimpleNamespace(params=params, names=["user%d" % i for i in range(k)], rng=np.random.default_rng(7 + k),
                              enc=mkckks.NewEncryptor(params, sampler), dec=mkckks.NewDecryptor(params), ev=mkckks.NewEvaluator(params),
                              skSet=mkrlwe.NewSecretKeySet(), pkSet=mkrlwe.NewPublicKeyKeySet(), rlk=mkrlwe.RelinearizationKeySet(params),
                              rks=mkrlwe.RotationKeySet(), mkckks=mkckks)
    for n in w.names:
        sk, pk = kgen.GenKeyPair(n)
        w.skSet.AddSecretKey(sk)
        w.pkSet.AddPublicKey(pk)
        w.rlk.AddRelinearizationKey(kgen.GenRelinearizationKey(sk, kgen.GenSecretKey(n)))
        for rot in (1, 4):
            w.rks.AddRotationKey(kgen.GenRotationKey(rot, sk))
    return w


def encrypt_sum(w, zs):
    ct = None
    for n in w.names:
        c = w.enc.EncryptMsgNew(w.mkckks.Message(zs[n]), w.pkSet.GetPublicKey(n))
        assert c.ids == [n] and c.Level() == w.params.MaxLevel() and c.Scale == w.params.Scale()
        ct = c if ct is None else w.ev.AddNew(ct, c)
    return ct


def test_encrypt_add_decrypt(world):
    w, n = world, 1 << (PSET["logN"] - 1)
    zs = {p: w.rng.uniform(-1, 1, n) + 1j * w.rng.uniform(-1, 1, n) for p in w.names}
    one = w.enc.EncryptMsgNew(w.mkckks.Message(zs[w.names[0]]), w.pkSet.GetPublicKey(w.names[0]))
    assert _max_log2_err(w.dec.Decrypt(one, w.skSet).Value, zs[w.names[0]]) <= bound(8)
    ct = encrypt_sum(w, zs)
    assert ct.ids == sorted(w.names)
    assert _max_log2_err(w.dec.Decrypt(ct, w.skSet).Value, sum(zs.values())) <= bound(8)


def test_encrypt_mulrelin_decrypt(world):
    w, n, k = world, 1 << (PSET["logN"] - 1), len(world.names)
    zs = {p: np.full(n, complex(0.1 / k, 1.0 / k)) + w.rng.uniform(-0.05, 0.05, n) for p in w.names}      # mkckks_test.go:330-340
    ct = encrypt_sum(w, zs)
    res = w.ev.MulRelinNew(ct, ct, w.rlk)
    assert _max_log2_err(w.dec.Decrypt(res, w.skSet).Value, sum(zs.values()) ** 2) <= bound(12)


def test_encrypt_rotate_decrypt(world):
    w, n = world, 1 << (PSET["logN"] - 1)
    zs = {p: w.rng.uniform(-1, 1, n) + 1j * w.rng.uniform(-1, 1, n) for p in w.names}
    ct = encrypt_sum(w, zs)
    for rot in (1, 4, 5):
        res = w.ev.RotateNew(ct, rot, w.rks)
        assert _max_log2_err(w.dec.Decrypt(res, w.skSet).Value, np.roll(sum(zs.values()), -rot)) <= bound(8)
