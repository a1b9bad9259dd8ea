"""MK-BFV with plaintext operands end to end (-m gpu): keygen -> EncryptMsgNew -> MulPtxtNew / AddPtxtNew / SubPtxtNew, alone and in a chain with
MulRelinNew and RotateNew -> Decrypt.  Two parties, small_bfv(11, nq = 3), T = 65537, seeded HostSampler (insecure_test_only), device encoder.
BFV decryption is exact, so every comparison is an equality of centred values.

Why the product decrypts (include/mkhe.h, "BFV plaintext operands"): with pt(a) = round(Q a / T) and p the centred lift of b,
pt(a) p = (Q/T) [a b]_T + Q k + eps p, |eps| <= 1/2 per coefficient, so a ciphertext of noise e decrypts after MulPtxt to a b mod T as long as
|e p + eps p| <= N (T/2) (|e| + 1/2) < Q / (2T).  test_mul_ptxt takes |e| from a host decryption of its input and asserts that inequality, in
integers, BEFORE it asserts the equality."""
import types

import numpy as np
import pytest

import harness_bfv as HB

pytestmark = pytest.mark.gpu

PSET = HB.small_bfv(11, 3)
N, T = 1 << PSET["logN"], PSET["T"]
QP = 1
for _q in PSET["Q"]:
    QP *= _q


def centre(v):
    r = np.mod(np.asarray(v, dtype=np.int64), T)
    return np.where(r > T // 2, r - T, r)


@pytest.fixture(scope="module")
def world():
    from mkhe_kklss_amd import mkbfv, mkrlwe
    params = mkbfv.Parameters(PSET["logN"], PSET["Q"], PSET["QMul"], PSET["P"], T)
    params.GenDefaultCRS(seed=778)
    sampler = mkrlwe.HostSampler(np.random.default_rng(41), insecure_test_only=True)
    kgen = mkbfv.NewKeyGenerator(params, sampler)
    w = types.SimpleNamespace(params=params, names=["user0", "user1"], rng=np.random.default_rng(6), sampler=sampler,
                              enc=mkbfv.NewEncryptor(params, sampler, encoder="device"), dec=mkbfv.NewDecryptor(params, encoder="device"),
                              dec_host=mkbfv.NewDecryptor(params), coder=mkbfv.DeviceEncoder(params), host=mkbfv.Encoder(params),
                              ev=mkbfv.NewEvaluator(params), skSet=mkrlwe.NewSecretKeySet(), pkSet=mkrlwe.NewPublicKeyKeySet(),
                              rlk=mkbfv.RelinearizationKeySet(params), rks=mkrlwe.RotationKeySet(), mkbfv=mkbfv, mkrlwe=mkrlwe)
    for n in w.names:
        sk, pk = kgen.GenKeyPair(n)
        w.skSet.AddSecretKey(sk)
        w.pkSet.AddPublicKey(pk)
        w.rlk.AddRelinearizationKey(kgen.GenRelinearizationKey(sk, kgen.GenSecretKey(n)))
        w.rks.AddRotationKey(kgen.GenRotationKey(1, sk))
    return w


def message(w):
    return w.rng.integers(-(T // 2), T // 2 + 1, N).astype(np.int64)


def encrypt(w, v, name):
    return w.enc.EncryptMsgNew(w.mkbfv.Message(v), w.pkSet.GetPublicKey(name))


def decrypt(w, ct):
    return w.dec.Decrypt(ct, w.skSet).Value


def noise_norm(w, ct, a):
    """max |x - pt(a)| over the coefficients, x the centred phase of ct from a HOST decryption (Python integers)"""
    poly = w.dec_host.DecryptPtxt(ct, w.skSet)
    x = np.zeros(N, dtype=object)
    for l, q in enumerate(PSET["Q"]):
        Mi = QP // q
        x = x + poly[l].astype(object) * (Mi * pow(Mi, -1, q))
    m = w.host.SlotsToCoeffs(a)
    worst = 0
    for xi, mi in zip(x, m):
        d = (int(xi) - (QP * int(mi) + T // 2) // T) % QP
        worst = max(worst, min(d, QP - d))
    return worst


def test_mul_ptxt(world):
    w = world
    a, b = message(w), message(w)
    b[:4] = [T // 2, -(T // 2), 0, -1]
    ca = encrypt(w, a, "user0")
    e = noise_norm(w, ca, a)
    print("input noise: %d bits; bound N (T/2) (|e| + 1/2): %d bits of the %d of Q/(2T)"
          % (e.bit_length(), (N * T * (2 * e + 1) // 4).bit_length(), (QP // (2 * T)).bit_length()))
    assert N * T * T * (2 * e + 1) < 2 * QP                             # N (T/2) (|e| + 1/2) < Q / (2T)
    pm = w.coder.EncodeMul(b)
    res = w.ev.MulPtxtNew(ca, pm)
    assert isinstance(res, w.mkbfv.Ciphertext) and res.ids == ["user0"] and res.Level() == w.params.MaxLevel()
    assert (decrypt(w, res) == centre(a * b)).all()
    # a Message is encoded with the device encoder: the same ciphertext
    assert (w.ev.MulPtxtNew(ca, w.mkbfv.Message(b)).download() == res.download()).all()
    # the host encoder's prepared plaintext gives the same ciphertext bits
    hp = w.mkbfv.PlaintextMul(w.params, w.host.EncodeMul(b))
    assert (hp.download() == pm.download()).all()
    assert (w.ev.MulPtxtNew(ca, hp).download() == res.download()).all()


def test_add_and_sub_ptxt(world):
    w = world
    a, b = message(w), message(w)
    ca = encrypt(w, a, "user1")
    pt = w.coder.Encode(b)
    s, d = w.ev.AddPtxtNew(ca, pt), w.ev.SubPtxtNew(ca, pt)
    assert s.ids == ["user1"] and d.ids == ["user1"]
    assert (decrypt(w, s) == centre(a + b)).all()
    assert (decrypt(w, d) == centre(a - b)).all()
    for other in (w.host.Encode(b), w.mkbfv.Message(b)):                # a host plaintext, a Message: the same bits
        assert (w.ev.AddPtxtNew(ca, other).download() == s.download()).all()
        assert (w.ev.SubPtxtNew(ca, other).download() == d.download()).all()


def test_chain_with_mulrelin(world):
    """(a b + c) d: MulRelinNew(AddPtxtNew(MulPtxtNew(ct_a, b), Encode(c)), ct_d), a under user0, d under user1"""
    w = world
    a, b, c, d = (message(w) for _ in range(4))
    t = w.ev.AddPtxtNew(w.ev.MulPtxtNew(encrypt(w, a, "user0"), w.coder.EncodeMul(b)), w.coder.Encode(c))
    assert t.ids == ["user0"]                                           # no party was added
    res = w.ev.MulRelinNew(t, encrypt(w, d, "user1"), w.rlk)
    assert res.ids == ["user0", "user1"]
    assert (decrypt(w, res) == centre(centre(a * b + c) * d)).all()


def test_rotate_after_mul_ptxt(world):
    w = world
    a, b = message(w), message(w)
    ct = w.ev.AddNew(encrypt(w, a, "user0"), encrypt(w, np.zeros(N, dtype=np.int64), "user1"))
    got = decrypt(w, w.ev.RotateNew(w.ev.MulPtxtNew(ct, w.coder.EncodeMul(b)), 1, w.rks))
    assert (got.reshape(2, N // 2) == np.roll(centre(a * b).reshape(2, N // 2), -1, axis=1)).all()


def test_mul_ptxt_batch_equals_one_at_a_time(world):
    w = world
    msgs = [message(w) for _ in range(3)]
    bs = np.stack([message(w) for _ in range(3)])
    cts = [encrypt(w, m, "user0") for m in msgs]
    pms = w.coder.EncodeMulBatch(bs)
    batch = w.ev.MulPtxtBatch(cts, pms)
    shared = w.ev.MulPtxtBatch(cts, w.coder.EncodeMul(bs[1]))
    assert len(batch) == 3 and len(shared) == 3
    for k in range(3):
        one = w.ev.MulPtxtNew(cts[k], w.coder.EncodeMul(bs[k]))
        assert (batch[k].download() == one.download()).all()
        assert (shared[k].download() == w.ev.MulPtxtNew(cts[k], w.coder.EncodeMul(bs[1])).download()).all()
        assert (decrypt(w, batch[k]) == centre(msgs[k] * bs[k])).all()
    sums = w.ev.AddPtxtBatch(cts, w.coder.EncodeBatch(bs))
    for k in range(3):
        assert (sums[k].download() == w.ev.AddPtxtNew(cts[k], w.coder.Encode(bs[k])).download()).all()
        assert (decrypt(w, sums[k]) == centre(msgs[k] + bs[k])).all()
