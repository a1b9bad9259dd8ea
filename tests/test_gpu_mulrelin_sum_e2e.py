"""MulRelinSumNew of mkckks.Evaluator end to end on the device (-m gpu): device keygen (seeded HostSampler, insecure_test_only) -> EncryptMsgNew ->
K = 3 products under one relinearisation tail -> Decrypt, two parties (op0 under user0, op1 under user1), complex slots in the unit square, scale 2^54,
against numpy on the cleartext slots and against the chain it replaces (three MulRelinNew and two AddNew) on the same ciphertexts.

Bound, in bits of log2|delta|: the reference's MulRelin bound -log2(scale) + logSlots + 12 (mkckks_test.go:357), plus log2 K for the K summands.
The single tail adds step F2's gadget noise once instead of K times, so its error may not exceed the chain's by more than one bit.
Measured on an MI355X (log2|delta| of the call / of the chain / bound): logN = 10: -39.6 / -39.6 / -31.4;  logN = 11: -38.7 / -38.7 / -30.4."""
import math
import types

import numpy as np
import pytest

import harness as H

pytestmark = pytest.mark.gpu

K = 3
PSETS = {10: H.small_ckks(10, nq=4, scale_bits=54), 11: H.small_ckks(11, nq=4, scale_bits=54)}


def _max_log2_err(a, b):
    d = np.abs(np.asarray(a) - np.asarray(b))
    return float(np.log2(max(d.real.max(), d.imag.max(), 1e-300)))


@pytest.fixture(scope="module", params=sorted(PSETS))
def world(request):
    from mkhe_kklss_amd import mkckks, mkrlwe
    pset = PSETS[request.param]
    params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], pset["scale"])
    params.GenDefaultCRS(seed=4321)
    sampler = mkrlwe.HostSampler(np.random.default_rng(2025), insecure_test_only=True)
    kgen = mkrlwe.NewKeyGenerator(params, sampler)
    w = types.SimpleNamespace(params=params, pset=pset, names=["user0", "user1"], rng=np.random.default_rng(19), n=1 << (pset["logN"] - 1),
                              enc=mkckks.NewEncryptor(params, sampler, encoder="device"), dec=mkckks.NewDecryptor(params, encoder="device"),
                              ev=mkckks.NewEvaluator(params), skSet=mkrlwe.NewSecretKeySet(), pkSet=mkrlwe.NewPublicKeyKeySet(),
                              rlk=mkrlwe.RelinearizationKeySet(params), mkckks=mkckks)
    for name in w.names:
        sk, pk = kgen.GenKeyPair(name)
        w.skSet.AddSecretKey(sk)
        w.pkSet.AddPublicKey(pk)
        w.rlk.AddRelinearizationKey(kgen.GenRelinearizationKey(sk, kgen.GenSecretKey(name)))
    return w


def test_three_products_under_one_tail(world):
    w, logN = world, world.pset["logN"]
    msg = lambda: w.rng.uniform(-1, 1, w.n) + 1j * w.rng.uniform(-1, 1, w.n)
    zs, ws = [msg() for _ in range(K)], [msg() for _ in range(K)]
    ops0 = [w.enc.EncryptMsgNew(w.mkckks.Message(z), w.pkSet.GetPublicKey("user0")) for z in zs]
    ops1 = [w.enc.EncryptMsgNew(w.mkckks.Message(v), w.pkSet.GetPublicKey("user1")) for v in ws]
    want = sum(z * v for z, v in zip(zs, ws))
    bound = -math.log2(w.pset["scale"]) + (logN - 1) + 12 + math.log2(K)
    res = w.ev.MulRelinSumNew(ops0, ops1, w.rlk)
    chain = None
    for a, b in zip(ops0, ops1):
        p = w.ev.MulRelinNew(a, b, w.rlk)
        chain = p if chain is None else w.ev.AddNew(chain, p)
    assert res.ids == chain.ids == sorted(w.names) and res.Level() == chain.Level() and res.Scale == chain.Scale
    err = _max_log2_err(w.dec.Decrypt(res, w.skSet).Value, want)
    err_chain = _max_log2_err(w.dec.Decrypt(chain, w.skSet).Value, want)
    print("MulRelinSumNew logN=%d K=%d: 2^%.1f, chain 2^%.1f, bound 2^%.1f" % (logN, K, err, err_chain, bound))
    assert err <= bound and err_chain <= bound
    assert err <= err_chain + 1
    # with the caller's hoisted forms: the same ciphertext
    again = w.ev.MulRelinSumNew(ops0, ops1, w.rlk, [w.ev.HoistedForm(c) for c in ops0], [w.ev.HoistedForm(c) for c in ops1])
    assert (again.download() == res.download()).all()
    # fuse_rescale off, as MulRelinHoistedNew honours it: the product at its level and mkhe_rescale after it -- the same ciphertext
    w.ev.fuse_rescale = False
    try:
        two_calls = w.ev.MulRelinSumNew(ops0, ops1, w.rlk)
    finally:
        w.ev.fuse_rescale = True
    assert two_calls.Level() == res.Level() and two_calls.Scale == res.Scale and (two_calls.download() == res.download()).all()


def test_products_of_different_scales_are_refused(world):
    from mkhe_kklss_amd._abi import MkheError
    w = world
    z = w.rng.uniform(-1, 1, w.n) + 0j
    a = w.enc.EncryptMsgNew(w.mkckks.Message(z), w.pkSet.GetPublicKey("user0"))
    b = w.enc.EncryptMsgNew(w.mkckks.Message(z), w.pkSet.GetPublicKey("user1"))
    half = w.mkckks.NewCiphertext(w.params, a.ids, a.Level(), a.Scale / 2).upload(a.download())
    with pytest.raises(MkheError, match="one scale"):
        w.ev.MulRelinSumNew([a, half], [b, b], w.rlk)
    with pytest.raises(MkheError, match="at least one pair"):
        w.ev.MulRelinSumNew([], [], w.rlk)
