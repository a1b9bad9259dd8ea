"""The BFV message layer on the device (-m gpu): keygen -> EncryptMsgNew(encoder="device") -> AddNew / MulRelinNew / RotateNew / ConjugateNew ->
Decrypt(encoder="device"), EncryptMsgBatch, and the same circuit with the host encoder.  Two parties, logN = 11, small_bfv(11, nq = 3), T = 65537,
seeded HostSampler (insecure_test_only).  BFV decryption is exact, so every comparison is an equality of centred values.

Headroom of the product (host oracle, CPU, small_bfv(10, 3), two parties, coefficients uniform in (-T/2, T/2] as encoded slots give them):
|T x - round(T x / Q) Q| after MulRelin is 2^49 against the 2^161 = Q/2 at which decoding fails: nq = 3 leaves over a hundred bits."""
import types

import numpy as np
import pytest

import harness_bfv as HB

pytestmark = pytest.mark.gpu

PSET = HB.small_bfv(11, 3)
N, T = 1 << PSET["logN"], PSET["T"]


def centre(v):
    r = np.mod(np.asarray(v, dtype=np.int64), T)
    return np.where(r > T // 2, r - T, r)


@pytest.fixture(scope="module")
def world():
    from mkhe_kklss_amd import mkbfv, mkrlwe
    params = mkbfv.Parameters(PSET["logN"], PSET["Q"], PSET["QMul"], PSET["P"], T)
    params.GenDefaultCRS(seed=777)
    sampler = mkrlwe.HostSampler(np.random.default_rng(31), insecure_test_only=True)
    kgen = mkbfv.NewKeyGenerator(params, sampler)
    w = types.SimpleNamespace(params=params, names=["user0", "user1"], rng=np.random.default_rng(5), sampler=sampler,
                              enc=mkbfv.NewEncryptor(params, sampler, encoder="device"), dec=mkbfv.NewDecryptor(params, encoder="device"),
                              enc_host=mkbfv.NewEncryptor(params, sampler, encoder="host"), dec_host=mkbfv.NewDecryptor(params),
                              ev=mkbfv.NewEvaluator(params), skSet=mkrlwe.NewSecretKeySet(), pkSet=mkrlwe.NewPublicKeyKeySet(),
                              rlk=mkbfv.RelinearizationKeySet(params), rks=mkrlwe.RotationKeySet(), cks=mkrlwe.ConjugationKeySet(), mkbfv=mkbfv, mkrlwe=mkrlwe)
    for n in w.names:
        sk, pk = kgen.GenKeyPair(n)
        w.skSet.AddSecretKey(sk)
        w.pkSet.AddPublicKey(pk)
        w.rlk.AddRelinearizationKey(kgen.GenRelinearizationKey(sk, kgen.GenSecretKey(n)))
        for rot in (1, 4):
            w.rks.AddRotationKey(kgen.GenRotationKey(rot, sk))
        w.cks.AddConjugationKey(kgen.GenConjugationKey(sk))
    return w


def message(w):
    return w.rng.integers(-(T // 2), T // 2 + 1, N).astype(np.int64)


def encrypt(w, v, name, enc=None):
    c = (enc or w.enc).EncryptMsgNew(w.mkbfv.Message(v), w.pkSet.GetPublicKey(name))
    assert isinstance(c, w.mkbfv.Ciphertext) and c.ids == [name] and c.Level() == w.params.MaxLevel()
    return c


def test_the_encoders_are_the_device_ones(world):
    w = world
    assert isinstance(w.enc.encoder, w.mkbfv.DeviceEncoder) and isinstance(w.dec.encoder, w.mkbfv.DeviceEncoder)
    assert isinstance(w.enc_host.encoder, w.mkbfv.Encoder) and isinstance(w.dec_host.encoder, w.mkbfv.Encoder)
    assert w.mkbfv.NewMessage(w.params).Slots() == N


def test_encrypt_decrypt_and_add(world):
    w = world
    a, b = message(w), message(w)
    a[:4] = [T // 2, -(T // 2), 0, -1]
    ca, cb = encrypt(w, a, "user0"), encrypt(w, b, "user1")
    got = w.dec.Decrypt(ca, w.skSet)
    assert isinstance(got, w.mkbfv.Message) and got.Value.dtype == np.int64 and (got.Value == a).all()
    big = a + T * w.rng.integers(-2 ** 40, 2 ** 40, N)                  # any int64 encodes as its residue
    assert (w.dec.Decrypt(encrypt(w, big, "user0"), w.skSet).Value == a).all()
    s = w.ev.AddNew(ca, cb)
    assert s.ids == ["user0", "user1"] and (w.dec.Decrypt(s, w.skSet).Value == centre(a + b)).all()


def test_mulrelin_multiplies_slot_by_slot(world):
    w = world
    a, b = message(w), message(w)
    res = w.ev.MulRelinNew(encrypt(w, a, "user0"), encrypt(w, b, "user1"), w.rlk)
    assert (w.dec.Decrypt(res, w.skSet).Value == centre(a * b)).all()


def test_rotate_and_conjugate_act_on_the_two_rows(world):
    w = world
    a = message(w)
    ct = w.ev.AddNew(encrypt(w, a, "user0"), encrypt(w, np.zeros(N, dtype=np.int64), "user1"))
    rows = a.reshape(2, N // 2)
    for k in (1, 5):
        got = w.dec.Decrypt(w.ev.RotateNew(ct, k, w.rks), w.skSet).Value
        assert (got.reshape(2, N // 2) == np.roll(rows, -k, axis=1)).all(), k      # slot i of the result = slot (i + k) mod N/2 of the input, per row
    got = w.dec.Decrypt(w.ev.ConjugateNew(ct, w.cks), w.skSet).Value
    assert (got.reshape(2, N // 2) == rows[::-1]).all()


def test_encrypt_msg_batch_equals_one_at_a_time(world):
    w = world
    msgs = [w.mkbfv.Message(message(w)) for _ in range(3)]
    samples = np.stack([np.concatenate([w.sampler.ternary(N, 0.5)[None], w.sampler.gaussian(2, N)]) for _ in range(3)])
    pk = w.pkSet.GetPublicKey("user1")
    batch = w.enc.EncryptMsgBatch(msgs, pk, samples)
    assert len(batch) == 3
    for m, s, c in zip(msgs, samples, batch):
        one = w.enc.EncryptMsgNew(m, pk, s)
        assert (one.download() == c.download()).all()
        assert (w.enc_host.EncryptMsgNew(m, pk, s).download() == c.download()).all()            # the host encoder gives the same plaintext
        assert (w.dec.Decrypt(c, w.skSet).Value == m.Value).all()
    hb = w.enc_host.EncryptMsgBatch(msgs, pk, samples)
    assert all((x.download() == y.download()).all() for x, y in zip(hb, batch))


def test_the_host_encoder_gives_the_same_messages(world):
    w = world
    a, b = message(w), message(w)
    out = {}
    for key, enc, dec in (("device", w.enc, w.dec), ("host", w.enc_host, w.dec_host)):
        ca, cb = encrypt(w, a, "user0", enc), encrypt(w, b, "user1", enc)
        res = w.ev.RotateNew(w.ev.MulRelinNew(w.ev.AddNew(ca, cb), cb, w.rlk), 1, w.rks)
        out[key] = dec.Decrypt(res, w.skSet).Value
    want = np.roll(centre((a + b) * b).reshape(2, N // 2), -1, axis=1).reshape(N)
    assert (out["device"] == want).all() and (out["host"] == want).all()
    # crossed: device-encrypted, host-decoded
    assert (w.dec_host.Decrypt(encrypt(w, a, "user0"), w.skSet).Value == a).all()
