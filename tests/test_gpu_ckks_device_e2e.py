"""The message layer on the device (-m gpu): keygen -> EncryptMsgNew(encoder="device") -> AddNew / MulRelinNew -> Decrypt(encoder="device"),
EncryptMsgBatch, and a device-encoded plaintext through MulPtxtNew.  Setting and bounds of test_gpu_encdec_e2e.py: seeded HostSampler
(insecure_test_only), Scenario.precision_bound with 8 extra bits for encrypt / decrypt and additions, 12 for products."""
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


@pytest.fixture(scope="module")
def world():
    from mkhe_kklss_amd import mkckks, mkrlwe
    params = mkckks.Parameters(PSET["logN"], PSET["Q"], PSET["P"], PSET["scale"])
    params.GenDefaultCRS(seed=4321)
    sampler = mkrlwe.HostSampler(np.random.default_rng(2024), insecure_test_only=True)
    kgen = mkrlwe.NewKeyGenerator(params, sampler)
    w = types.SimpleNamespace(params=params, names=["user0", "user1"], rng=np.random.default_rng(17), n=1 << (PSET["logN"] - 1),
                              enc=mkckks.NewEncryptor(params, sampler, encoder="device"), dec=mkckks.NewDecryptor(params, encoder="device"),
                              enc_host=mkckks.NewEncryptor(params, sampler), dec_host=mkckks.NewDecryptor(params),
                              ev=mkckks.NewEvaluator(params), skSet=mkrlwe.NewSecretKeySet(), pkSet=mkrlwe.NewPublicKeyKeySet(),
                              rlk=mkrlwe.RelinearizationKeySet(params), mkckks=mkckks, mkrlwe=mkrlwe)
    for n in w.names:
        sk, pk = kgen.GenKeyPair(n)
        w.skSet.AddSecretKey(sk)
        w.pkSet.AddPublicKey(pk)
        w.rlk.AddRelinearizationKey(kgen.GenRelinearizationKey(sk, kgen.GenSecretKey(n)))
    return w


def encrypt_sum(w, zs):
    ct = None
    for n in w.names:
        c = w.enc.EncryptMsgNew(w.mkckks.Message(zs[n]), w.pkSet.GetPublicKey(n))
        assert c.ids == [n] and c.Level() == w.params.MaxLevel() and c.Scale == w.params.Scale()
        ct = c if ct is None else w.ev.AddNew(ct, c)
    return ct


def test_the_encoders_are_the_device_ones(world):
    w = world
    assert isinstance(w.enc.encoder, w.mkckks.DeviceEncoder) and isinstance(w.dec.encoder, w.mkckks.DeviceEncoder)
    assert isinstance(w.enc_host.encoder, w.mkckks.Encoder) and isinstance(w.mkckks.Decryptor(w.params).encoder, w.mkckks.Encoder)
    pt = w.enc.EncodeMsgNew(w.mkckks.Message(np.zeros(w.n)))
    assert isinstance(pt.Value, w.mkrlwe.DeviceLimbs) and pt.Level() == w.params.MaxLevel() and pt.Scale == w.params.Scale()


def test_encrypt_add_decrypt(world):
    w = world
    zs = {p: w.rng.uniform(-1, 1, w.n) + 1j * w.rng.uniform(-1, 1, w.n) for p in w.names}
    ct = encrypt_sum(w, zs)
    assert ct.ids == sorted(w.names)
    got = w.dec.Decrypt(ct, w.skSet).Value
    print("add: 2^%.1f, bound 2^%.1f" % (_max_log2_err(got, sum(zs.values())), bound(8)))
    assert _max_log2_err(got, sum(zs.values())) <= bound(8)
    # and each encoder opens what the other one made
    one = w.enc.EncryptMsgNew(w.mkckks.Message(zs["user0"]), w.pkSet.GetPublicKey("user0"))
    assert _max_log2_err(w.dec_host.Decrypt(one, w.skSet).Value, zs["user0"]) <= bound(8)
    other = w.enc_host.EncryptMsgNew(w.mkckks.Message(zs["user1"]), w.pkSet.GetPublicKey("user1"))
    assert _max_log2_err(w.dec.Decrypt(other, w.skSet).Value, zs["user1"]) <= bound(8)


def test_encrypt_mulrelin_decrypt(world):
    w, k = world, len(world.names)
    zs = {p: np.full(w.n, complex(0.1 / k, 1.0 / k)) + w.rng.uniform(-0.05, 0.05, w.n) for p in w.names}      # mkckks_test.go:330-340
    ct = encrypt_sum(w, zs)
    res = w.ev.MulRelinNew(ct, ct, w.rlk)
    got = w.dec.Decrypt(res, w.skSet).Value
    print("product: 2^%.1f, bound 2^%.1f" % (_max_log2_err(got, sum(zs.values()) ** 2), bound(12)))
    assert _max_log2_err(got, sum(zs.values()) ** 2) <= bound(12)


def test_encrypt_msg_batch(world):
    w = world
    zs = [w.rng.uniform(-1, 1, w.n) + 1j * w.rng.uniform(-1, 1, w.n) for _ in range(3)]
    cts = w.enc.EncryptMsgBatch([w.mkckks.Message(z) for z in zs], w.pkSet.GetPublicKey("user1"))
    assert len(cts) == 3
    for c, z in zip(cts, zs):
        assert c.ids == ["user1"] and c.Level() == w.params.MaxLevel() and c.Scale == w.params.Scale()
        assert _max_log2_err(w.dec.Decrypt(c, w.skSet).Value, z) <= bound(8)


def test_device_plaintext_through_mulptxt(world):
    w = world
    z = w.rng.uniform(-1, 1, w.n) + 1j * w.rng.uniform(-1, 1, w.n)
    p = w.rng.uniform(-1, 1, w.n) + 1j * w.rng.uniform(-1, 1, w.n)
    ct = w.enc.EncryptMsgNew(w.mkckks.Message(z), w.pkSet.GetPublicKey("user0"))
    level, scale = ct.Level(), w.params.Scale()
    dev_pt = w.enc.encoder.Encode(p, level, scale)
    host_pt = w.enc_host.encoder.Encode(p, level, scale)
    a = w.dec.Decrypt(w.ev.MulPtxtNew(ct, dev_pt, scale), w.skSet).Value
    b = w.dec.Decrypt(w.ev.MulPtxtNew(ct, host_pt, scale), w.skSet).Value
    print("ptxt product: device vs host 2^%.1f, vs plain 2^%.1f, bound 2^%.1f" % (_max_log2_err(a, b), _max_log2_err(a, z * p), bound(12)))
    assert _max_log2_err(a, b) <= bound(12) and _max_log2_err(a, z * p) <= bound(12)
    ct2 = w.enc.EncryptMsgNew(w.mkckks.Message(z), w.pkSet.GetPublicKey("user0"))
    outs = w.mkckks.BatchEvaluator(w.params, 2, w.ev).MulPtxtNew(w.mkckks.BatchCiphertext([ct, ct2]), dev_pt, scale)
    for o in outs.cts:
        assert _max_log2_err(w.dec.Decrypt(o, w.skSet).Value, b) <= bound(12)
