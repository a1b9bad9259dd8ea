"""Sparse CKKS packing end to end on the device (-m gpu): Parameters with logSlots = 4 and logSlots = 0 at logN = 10, two parties, the host and the
device encoder: keygen -> EncryptMsgNew -> MulRelinNew / RotateNew / ConjugateNew / LinearTransformNew -> Decrypt, and a distributed decryption.
The evaluator is untouched: seen through the full embedding a sparse message is its n slots repeated N / 2n times, so every operation acts on it
slot-wise and RotateNew(ct, k) rotates it by k mod n.

Bounds.  Messages: Scenario.precision_bound(extra), which uses logN - 1, with the extra of the matching full-packing tests (8 for encrypt / decrypt,
12 for products: test_gpu_ckks_device_e2e.py; the linear transform's formula: test_gpu_lintrans_e2e.py) -- NOT a tighter bound from logSlots: the
decoded sparse slot is the mean over the replicas of the full decoding, and every replica meets the full-packing bound, so the mean does; a bound from
logSlots would sit at about 2.5 sigma of fresh noise for n = 1.  The replica identity itself is independent of the noise: the sparse decoding of ANY
polynomial against the replica mean of its full decoding, within the sum of the two transforms' rounding bounds, 8 (logN + 3) 2^-53 sum_k |m_k|."""
import ctypes as C
import math
import types

import numpy as np
import pytest

import harness as H
from scenario import Scenario

pytestmark = pytest.mark.gpu

PSET = H.small_ckks(10, 4)
LOGN, N = PSET["logN"], 1 << PSET["logN"]
ROT = 3


def _max_log2_err(a, b):
    d = np.abs(np.asarray(a) - np.asarray(b))
    return float(np.log2(max(d.real.max(), d.imag.max(), 1e-300)))


def bound(extra):
    return Scenario.precision_bound(types.SimpleNamespace(scale=PSET["scale"], logN=LOGN), extra)


ALL = [(4, "host"), (4, "device"), (0, "host"), (0, "device")]
_worlds = {}


def world(logSlots, encoder):
    """one context, one key set per (logSlots, encoder) for the whole module"""
    if (logSlots, encoder) in _worlds:
        return _worlds[logSlots, encoder]
    from mkhe_kklss_amd import mkckks, mkrlwe
    params = mkckks.Parameters(LOGN, PSET["Q"], PSET["P"], PSET["scale"], logSlots=logSlots)
    params.GenDefaultCRS(seed=4321)
    params.AddCRS(ROT, seed=4321)
    sampler = mkrlwe.HostSampler(np.random.default_rng(2024), insecure_test_only=True)
    kgen = mkrlwe.NewKeyGenerator(params, sampler)
    w = types.SimpleNamespace(params=params, logSlots=logSlots, n=1 << logSlots, names=["user0", "user1"], rng=np.random.default_rng(17 + logSlots),
                              enc=mkckks.NewEncryptor(params, sampler, encoder=encoder), dec=mkckks.NewDecryptor(params, encoder=encoder),
                              ev=mkckks.NewEvaluator(params), skSet=mkrlwe.NewSecretKeySet(), pkSet=mkrlwe.NewPublicKeyKeySet(),
                              rlk=mkrlwe.RelinearizationKeySet(params), rks=mkrlwe.RotationKeySet(), cks=mkrlwe.ConjugationKeySet(), kgen=kgen, sks={},
                              mkckks=mkckks, mkrlwe=mkrlwe, encoder=encoder)
    assert w.enc.encoder.n == w.dec.encoder.n == w.n and mkckks.NewMessage(params).Slots() == w.n
    for name in w.names:
        sk, pk = kgen.GenKeyPair(name)
        w.sks[name] = sk
        w.skSet.AddSecretKey(sk)
        w.pkSet.AddPublicKey(pk)
        w.rlk.AddRelinearizationKey(kgen.GenRelinearizationKey(sk, kgen.GenSecretKey(name)))
        w.rks.AddRotationKey(kgen.GenRotationKey(ROT, sk))
        w.cks.AddConjugationKey(kgen.GenConjugationKey(sk))
    _worlds[logSlots, encoder] = w
    return w


def encrypt(w, z, name):
    c = w.enc.EncryptMsgNew(w.mkckks.Message(z), w.pkSet.GetPublicKey(name))
    assert c.ids == [name] and c.Level() == w.params.MaxLevel() and c.Scale == w.params.Scale()
    return c


def product(w):
    """MulRelinNew of one ciphertext per party, and the cleartext product (the messages of mkckks_test.go:330-340)"""
    zs = [np.full(w.n, complex(0.1, 1.0)) + w.rng.uniform(-0.05, 0.05, w.n) for _ in w.names]
    ct = w.ev.MulRelinNew(encrypt(w, zs[0], w.names[0]), encrypt(w, zs[1], w.names[1]), w.rlk)
    assert ct.ids == sorted(w.names)
    return ct, zs[0] * zs[1]


@pytest.mark.parametrize("logSlots,encoder", ALL)
def test_encrypt_decrypt(logSlots, encoder):
    w = world(logSlots, encoder)
    zs = {p: w.rng.uniform(-1, 1, w.n) + 1j * w.rng.uniform(-1, 1, w.n) for p in w.names}
    ct = w.ev.AddNew(encrypt(w, zs["user0"], "user0"), encrypt(w, zs["user1"], "user1"))
    got = w.dec.Decrypt(ct, w.skSet).Value
    err = _max_log2_err(got, zs["user0"] + zs["user1"])
    print("logSlots %d %s: encrypt -> decrypt 2^%.1f, bound 2^%.1f" % (w.logSlots, w.encoder, err, bound(8)))
    assert got.shape == (w.n,) and err <= bound(8)
    with pytest.raises(w.mkckks.MkheError, match="slots"):
        encrypt(w, np.zeros(N // 2), "user0")                       # a full-packing message is not a message of these parameters


@pytest.mark.parametrize("logSlots,encoder", ALL)
def test_mulrelin_rotate_conjugate(logSlots, encoder):
    w = world(logSlots, encoder)
    ct, z = product(w)
    res = w.ev.ConjugateNew(w.ev.RotateNew(ct, ROT, w.rks), w.cks)
    want = np.conj(np.roll(z, -ROT))                                # the roll is mod n: the identity for n = 1
    if w.n == 1:
        assert want[0] == np.conj(z[0])
    got = w.dec.Decrypt(res, w.skSet).Value
    err = _max_log2_err(got, want)
    print("logSlots %d %s: conj(rot_%d(a * b)) 2^%.1f, bound 2^%.1f" % (w.logSlots, w.encoder, ROT, err, bound(12)))
    assert got.shape == (w.n,) and err <= bound(12)


@pytest.mark.parametrize("logSlots,encoder", ALL)
def test_sparse_decoding_is_the_replica_mean_of_the_full_decoding(logSlots, encoder):
    """the check that pins the semantics, on a decrypted product (message plus noise in every coefficient)"""
    w = world(logSlots, encoder)
    from mkhe_kklss_amd._abi import check, lib
    ct, z = product(w)
    pt = w.dec.DecryptPtxt(ct, w.skSet)
    limbs = pt.Value.shape[0]
    sparse = w.mkckks.DeviceEncoder(w.params).Decode(pt.Value, pt.Scale)
    full = w.mkckks.DeviceEncoder(w.params, logSlots=LOGN - 1).Decode(pt.Value, pt.Scale)
    assert sparse.shape == (w.n,) and full.shape == (N // 2,)
    src, dst = w.mkrlwe.DeviceLimbs(w.params, 1, limbs).upload(pt.Value[None]), w.mkrlwe.DeviceLimbs(w.params, 1, 1)
    check(lib().mkhe_ckks_scale_down(w.params.ctx, limbs, 1, src.devptr(), C.c_double(pt.Scale), dst.devptr()))
    m = dst.download().view(np.float64).ravel()
    mean = full.reshape(N // (2 * w.n), w.n).mean(axis=0)
    err, tol = np.abs(sparse - mean).max(), 8 * (LOGN + 3) * 2.0 ** -53 * np.abs(m).sum()
    print("logSlots %d %s: |sparse - replica mean| %.3g, tolerance %.3g; against the message 2^%.1f" % (w.logSlots, w.encoder, err, tol, _max_log2_err(sparse, z)))
    assert err <= tol
    assert _max_log2_err(sparse, z) <= bound(12)


@pytest.mark.parametrize("encoder", ["host", "device"])
def test_linear_transform_of_a_16_by_16_matrix(encoder):
    w = world(4, encoder)
    M = (w.rng.uniform(-1, 1, (16, 16)) + 1j * w.rng.uniform(-1, 1, (16, 16))) / math.sqrt(2)
    v = [0.5 * np.sqrt(w.rng.uniform(0, 1, 16)) * np.exp(2j * np.pi * w.rng.uniform(0, 1, 16)) for _ in w.names]
    ct = w.ev.AddNew(encrypt(w, v[0], "user0"), encrypt(w, v[1], "user1"))
    lt = w.mkckks.LinearTransform.FromMatrix(w.params, M, ct.Level(), keep_coeff=True)
    diag = w.mkckks.matrix_diagonals(M, 16)
    assert lt.n == 16 and sorted(diag) == list(range(16)) and lt.Rotations() and all(1 <= r < 16 for r in lt.Rotations())
    for r in lt.Rotations():
        if r not in w.params.CRS:
            w.params.AddCRS(r, seed=4321)
        if r != ROT:
            for name in w.names:
                w.rks.AddRotationKey(w.kgen.GenRotationKey(r, w.sks[name]))
    fused = w.ev.LinearTransformNew(ct, lt, w.rks)
    chain = w.ev.LinearTransformNew(ct, lt, w.rks, fused=False)
    for res in (fused, chain):
        assert res.Level() == lt.level - 1 and res.Scale == w.params.Scale() and res.ids == ct.ids
    assert (fused.download() == chain.download()).all()
    giants = sum(1 for g in lt.plan.giants if g)
    tol = bound(12) + math.log2(sum(np.abs(d).max() for d in diag.values()) + giants)
    err = _max_log2_err(w.dec.Decrypt(fused, w.skSet).Value, M @ (v[0] + v[1]))
    print("logSlots 4 %s: M z, n1=%d babies=%d giants=%d: 2^%.1f, bound 2^%.1f" % (w.encoder, lt.plan.n1, sum(1 for b in lt.plan.babies if b), giants, err, tol))
    assert err <= tol
    with pytest.raises(w.mkckks.MkheError):
        w.mkckks.LinearTransform(w.params, {0: np.zeros(N // 2)}, 1)          # diagonals have n slots


@pytest.mark.parametrize("logSlots,encoder", ALL)
def test_distributed_decryption(logSlots, encoder):
    w, bits = world(logSlots, encoder), 30
    zs = [np.full(w.n, complex(0.05, 0.5)) + w.rng.uniform(-0.05, 0.05, w.n) for _ in w.names]
    ct = w.ev.AddNew(encrypt(w, zs[0], "user0"), encrypt(w, zs[1], "user1"))
    shares = [w.dec.ShareNew(ct, w.sks[p], bits, w.mkrlwe.DeviceSampler()) for p in w.names]
    got = w.dec.MergeSharesMsg(ct, shares).Value
    flood = w.dec.FloodSlotBound(2, bits, PSET["scale"])
    d = np.abs(got - w.dec.Decrypt(ct, w.skSet).Value)
    err = float(max(d.real.max(), d.imag.max()))
    print("logSlots %d %s: merge against Decrypt %.3g, flood bound %.3g" % (w.logSlots, w.encoder, err, flood))
    assert got.shape == (w.n,) and err <= flood + 2.0 ** -40
    assert _max_log2_err(got, zs[0] + zs[1]) <= math.log2(2 * 2.0 ** bound(8) + flood)          # each summand's round trip, and the flood
