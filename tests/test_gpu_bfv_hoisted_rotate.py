"""mkhe_hoisted_form and mkhe_rotate_multi on a BFV context (-m gpu): include/mkhe.h says every mkrlwe-level call works on one; here they run.
Two parties with generated keys, small_bfv(10, 3) and small_bfv(11, 3), T = 65537.  mkbfv.Evaluator.RotateHoistedNew equals RotateNew, and three
lanes of mkhe_rotate_multi equal three mkhe_rotate calls, with and without a shared hoisted form: all bit for bit, and the rotation is checked
once against the slots."""
import ctypes as C
import types

import numpy as np
import pytest

import harness_bfv as HB

pytestmark = pytest.mark.gpu

ROTS = [1, 2, 4]


def make_world(logN):
    from mkhe_kklss_amd import mkbfv, mkrlwe
    pset = HB.small_bfv(logN, 3)
    params = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], pset["T"])
    params.GenDefaultCRS(seed=901)
    sampler = mkrlwe.HostSampler(np.random.default_rng(23 + logN), insecure_test_only=True)
    kgen = mkbfv.NewKeyGenerator(params, sampler)
    w = types.SimpleNamespace(params=params, N=1 << logN, T=pset["T"], names=["user0", "user1"], rng=np.random.default_rng(logN), mkbfv=mkbfv,
                              enc=mkbfv.NewEncryptor(params, sampler, encoder="device"), dec=mkbfv.NewDecryptor(params, encoder="device"),
                              ev=mkbfv.NewEvaluator(params), skSet=mkrlwe.NewSecretKeySet(), pkSet=mkrlwe.NewPublicKeyKeySet(),
                              rks=mkrlwe.RotationKeySet())
    for n in w.names:
        sk, pk = kgen.GenKeyPair(n)
        w.skSet.AddSecretKey(sk)
        w.pkSet.AddPublicKey(pk)
        for r in ROTS:
            w.rks.AddRotationKey(kgen.GenRotationKey(r, sk))
    return w


@pytest.fixture(scope="module", params=[10, 11])
def world(request):
    return make_world(request.param)


def two_party_ct(w):
    """-> (ciphertext over both parties, its message)"""
    a, b = (w.rng.integers(-(w.T // 2), w.T // 2 + 1, w.N).astype(np.int64) for _ in range(2))
    ca = w.enc.EncryptMsgNew(w.mkbfv.Message(a), w.pkSet.GetPublicKey("user0"))
    cb = w.enc.EncryptMsgNew(w.mkbfv.Message(b), w.pkSet.GetPublicKey("user1"))
    s = a + b
    s = np.mod(s, w.T)
    return w.ev.AddNew(ca, cb), np.where(s > w.T // 2, s - w.T, s)


def test_rotate_hoisted_equals_rotate(world):
    w = world
    ct, msg = two_party_ct(w)
    before = ct.download()
    hoisted = w.ev.HoistedForm(ct)
    assert sorted(hoisted.Value) == w.names
    for r in ROTS:
        plain, fast = w.ev.RotateNew(ct, r, w.rks), w.ev.RotateHoistedNew(ct, r, hoisted, w.rks)
        assert isinstance(fast, w.mkbfv.Ciphertext) and fast.ids == w.names and fast.Level() == w.params.MaxLevel()
        assert (fast.download() == plain.download()).all(), r
    assert (ct.download() == before).all()
    # the rotation itself: slot j + r moves to slot j in each row
    got = w.dec.Decrypt(w.ev.RotateHoistedNew(ct, 2, hoisted, w.rks), w.skSet).Value
    assert (got.reshape(2, -1) == np.roll(msg.reshape(2, -1), -2, axis=1)).all()
    # index 0 is a copy, an index without a CRS is refused by the mirror
    assert (w.ev.RotateHoistedNew(ct, 0, hoisted, w.rks).download() == before).all()
    from mkhe_kklss_amd._abi import MkheError
    with pytest.raises(MkheError):
        w.ev.RotateHoistedNew(ct, 3, hoisted, w.rks)


@pytest.mark.parametrize("shared", [True, False])
def test_three_lanes_of_rotate_multi_equal_three_rotations(world, shared):
    from mkhe_kklss_amd._abi import check, handle_array, lib
    w = world
    params = w.params
    if shared:
        ct, _ = two_party_ct(w)
        srcs = [ct] * 3
        hoisted = w.ev.HoistedForm(ct)
        hs = handle_array([hoisted.Value[i].h for i in ct.ids] * 3)
    else:
        srcs = [two_party_ct(w)[0] for _ in range(3)]
        hs = None
    ids = srcs[0].ids
    outs = [w.mkbfv.NewCiphertext(params, ids, zero=False) for _ in ROTS]
    gal = (C.c_uint64 * 3)(*[params.GaloisElementForColumnRotationBy(r) for r in ROTS])
    check(lib().mkhe_rotate_multi(params.ctx, 3, gal, handle_array([c.h for c in srcs]), hs,
                                  handle_array([w.rks.GetRotationKey(i, r).Value.h for r in ROTS for i in ids]),
                                  handle_array([params.CRS[r].h for r in ROTS]), None, handle_array([o.h for o in outs])))
    for c, r, o in zip(srcs, ROTS, outs):
        assert (o.download() == w.ev.RotateNew(c, r, w.rks).download()).all(), r
