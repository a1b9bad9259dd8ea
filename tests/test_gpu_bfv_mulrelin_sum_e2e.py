"""MK-BFV inner product end to end (-m gpu): keygen -> EncryptMsgNew -> MulRelinSumNew -> Decrypt, keys, CRS, encoder, encryption and decryption all
on the device.  Two parties, small_bfv(10, nq = 3), T = 65537, K = 3, seeded HostSampler (insecure_test_only), device encoder.  BFV decryption is
exact, so every comparison is an equality of centred values in every slot."""
import types

import numpy as np
import pytest

import harness_bfv as HB

pytestmark = pytest.mark.gpu

PSET = HB.small_bfv(10, 3)
N, T, K = 1 << PSET["logN"], PSET["T"], 3


def centre(v):
    r = np.mod(np.asarray(v, dtype=np.int64), T)
    return np.where(r > T // 2, r - T, r)


@pytest.fixture(scope="module")
def world():
    from mkhe_kklss_amd import mkbfv, mkrlwe
    params = mkbfv.Parameters(PSET["logN"], PSET["Q"], PSET["QMul"], PSET["P"], T)
    params.GenDefaultCRS(seed=779)
    sampler = mkrlwe.HostSampler(np.random.default_rng(43), insecure_test_only=True)
    kgen = mkbfv.NewKeyGenerator(params, sampler)
    w = types.SimpleNamespace(params=params, names=["user0", "user1"], rng=np.random.default_rng(8),
                              enc=mkbfv.NewEncryptor(params, sampler, encoder="device"), dec=mkbfv.NewDecryptor(params, encoder="device"),
                              ev=mkbfv.NewEvaluator(params), skSet=mkrlwe.NewSecretKeySet(), pkSet=mkrlwe.NewPublicKeyKeySet(),
                              rlk=mkbfv.RelinearizationKeySet(params), mkbfv=mkbfv)
    for n in w.names:
        sk, pk = kgen.GenKeyPair(n)
        w.skSet.AddSecretKey(sk)
        w.pkSet.AddPublicKey(pk)
        w.rlk.AddRelinearizationKey(kgen.GenRelinearizationKey(sk, kgen.GenSecretKey(n)))
    yield w
    params.close()


def message(w):
    return w.rng.integers(-(T // 2), T // 2 + 1, N).astype(np.int64)


def encrypt(w, v, name):
    return w.enc.EncryptMsgNew(w.mkbfv.Message(v), w.pkSet.GetPublicKey(name))


def decrypt(w, ct):
    return w.dec.Decrypt(ct, w.skSet).Value


def test_inner_product_of_two_parties(world):
    """a_k under user0, b_k under user1: Decrypt(MulRelinSumNew) = sum_k a_k (.) b_k mod T, exactly, and so does the chain it replaces"""
    w = world
    a, b = [message(w) for _ in range(K)], [message(w) for _ in range(K)]
    ca, cb = [encrypt(w, v, "user0") for v in a], [encrypt(w, v, "user1") for v in b]
    res = w.ev.MulRelinSumNew(ca, cb, w.rlk)
    assert isinstance(res, w.mkbfv.Ciphertext) and res.ids == ["user0", "user1"] and res.Level() == w.params.MaxLevel()
    want = centre(sum(centre(x * y) for x, y in zip(a, b)))
    assert (decrypt(w, res) == want).all()
    chain = w.ev.MulRelinNew(ca[0], cb[0], w.rlk)
    for x, y in zip(ca[1:], cb[1:]):
        chain = w.ev.AddNew(chain, w.ev.MulRelinNew(x, y, w.rlk))
    assert (decrypt(w, chain) == want).all()
    assert (chain.download() != res.download()).any()          # another ciphertext of the same sum


def test_one_single_party_and_one_two_party_operand(world):
    w = world
    a, a2, b = ([message(w) for _ in range(K)] for _ in range(3))
    two = [w.ev.AddNew(encrypt(w, x, "user0"), encrypt(w, y, "user1")) for x, y in zip(a, a2)]
    one = [encrypt(w, v, "user1") for v in b]
    want = centre(sum(centre(centre(x + y) * z) for x, y, z in zip(a, a2, b)))
    for ops0, ops1 in ((two, one), (one, two)):
        res = w.ev.MulRelinSumNew(ops0, ops1, w.rlk)
        assert res.ids == ["user0", "user1"]
        assert (decrypt(w, res) == want).all()


def test_list_checks_come_before_any_engine_call(world):
    from mkhe_kklss_amd._abi import MkheError
    w = world
    c = encrypt(w, message(w), "user0")
    for ops0, ops1 in (([], []), ([c], []), ([c, c], [c]), ([c] * 17, [c] * 17)):
        with pytest.raises(MkheError, match="MulRelinSumNew"):
            w.ev.MulRelinSumNew(ops0, ops1, w.rlk)
    assert (decrypt(w, w.ev.MulRelinSumNew([c], [c], w.rlk)) == decrypt(w, w.ev.MulRelinNew(c, c, w.rlk))).all()
