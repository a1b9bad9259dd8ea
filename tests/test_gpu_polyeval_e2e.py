"""AddConstNew, LinCombNew and EvaluatePolyNew of mkckks.Evaluator end to end on the device (-m gpu): device keygen (seeded HostSampler,
insecure_test_only) -> EncryptMsgNew -> the operation -> Decrypt, two parties, complex slots with |z| <= 1, against numpy on the cleartext slots.

Bounds, in bits of log2|delta| (Scenario.precision_bound(extra) = -log2(scale) + logSlots + extra, the reference's own: 8 extra bits for encrypt / decrypt
and additions, 12 for a MulRelin):
  AddConstNew      bound(8): the ciphertext part is untouched, the constant is exact to 2^-scale.
  LinCombNew       bound(8) + log2(sum_k |w_k| + 1): every summand brings its encryption error times |w_k|, the Rescale one rounding of that order.
  EvaluatePolyNew  bound(12) + log2(sum_k k |c_k|): the MulRelin bound, propagated to first order through x^k with |x| <= 1.
Measured on an MI355X (log2|delta| / bound): see the table in DESIGN.md, section "Polynomial evaluation"."""
import math
import types

import numpy as np
import pytest

import harness as H
from scenario import Scenario

pytestmark = pytest.mark.gpu

PSETS = {10: H.small_ckks(10, nq=6), 11: H.small_ckks(11, nq=7)}


def _max_log2_err(a, b):
    d = np.abs(np.asarray(a) - np.asarray(b))
    return float(np.log2(max(d.real.max(), d.imag.max(), 1e-300)))


def _disc(rng, n, radius):
    return radius * np.sqrt(rng.uniform(0, 1, n)) * np.exp(2j * np.pi * rng.uniform(0, 1, n))


@pytest.fixture(scope="module", params=sorted(PSETS))
def world(request):
    from mkhe_kklss_amd import mkckks, mkrlwe
    pset = PSETS[request.param]
    params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], pset["scale"])
    params.GenDefaultCRS(seed=4321)
    sampler = mkrlwe.HostSampler(np.random.default_rng(2024), insecure_test_only=True)
    kgen = mkrlwe.NewKeyGenerator(params, sampler)
    w = types.SimpleNamespace(params=params, pset=pset, names=["user0", "user1"], rng=np.random.default_rng(17), n=1 << (pset["logN"] - 1),
                              enc=mkckks.NewEncryptor(params, sampler, encoder="device"), dec=mkckks.NewDecryptor(params, encoder="device"),
                              ev=mkckks.NewEvaluator(params), skSet=mkrlwe.NewSecretKeySet(), pkSet=mkrlwe.NewPublicKeyKeySet(),
                              rlk=mkrlwe.RelinearizationKeySet(params), mkckks=mkckks)
    for name in w.names:
        sk, pk = kgen.GenKeyPair(name)
        w.skSet.AddSecretKey(sk)
        w.pkSet.AddPublicKey(pk)
        w.rlk.AddRelinearizationKey(kgen.GenRelinearizationKey(sk, kgen.GenSecretKey(name)))
    w.bound = lambda extra: Scenario.precision_bound(types.SimpleNamespace(scale=pset["scale"], logN=pset["logN"]), extra)
    return w


def two_party(w, radius=0.5):
    """user0's message plus user1's: a ciphertext under both keys whose slots lie in the disc of radius 2 * radius"""
    zs = [_disc(w.rng, w.n, radius) for _ in w.names]
    cts = [w.enc.EncryptMsgNew(w.mkckks.Message(z), w.pkSet.GetPublicKey(name)) for z, name in zip(zs, w.names)]
    ct = w.ev.AddNew(cts[0], cts[1])
    assert ct.ids == sorted(w.names)
    return ct, zs[0] + zs[1]


def test_add_const(world):
    w = world
    ct, z = two_party(w)
    c = 0.25 - 0.5j
    res = w.ev.AddConstNew(ct, c)
    assert res.Level() == ct.Level() and res.Scale == ct.Scale and res.ids == ct.ids
    got = w.dec.Decrypt(res, w.skSet).Value
    err = _max_log2_err(got, z + c)
    print("AddConstNew logN=%d: 2^%.1f, bound 2^%.1f" % (w.pset["logN"], err, w.bound(8)))
    assert err <= w.bound(8)
    a, b = ct.download(), res.download()
    assert (a[1:] == b[1:]).all() and (a[0] != b[0]).sum() == 2 * a.shape[1]          # two coefficients of c_0 per limb moved, nothing else


def test_lincomb_pins_i_to_the_monomial(world):
    w = world
    (ct, z), (ct2, z2) = two_party(w), two_party(w)
    weights = [1j, -0.5]
    res = w.ev.LinCombNew([ct, ct2], weights, 0.125)
    assert res.Level() == ct.Level() - 1 and res.Scale == w.params.Scale()
    got = w.dec.Decrypt(res, w.skSet).Value
    bound = w.bound(8) + math.log2(sum(abs(x) for x in weights) + 1)
    err = _max_log2_err(got, 1j * z - 0.5 * z2 + 0.125)
    print("LinCombNew logN=%d: 2^%.1f, bound 2^%.1f" % (w.pset["logN"], err, bound))
    assert err <= bound
    # without the rescale, at the summands' scale; a zero weight drops its ciphertext
    res = w.ev.LinCombNew([ct, ct2], [0, 2 - 1j], -1j, scale=ct.Scale, rescale=False)
    assert res.Level() == ct.Level() and res.Scale == ct.Scale
    assert _max_log2_err(w.dec.Decrypt(res, w.skSet).Value, (2 - 1j) * z2 - 1j) <= w.bound(8) + math.log2(abs(2 - 1j) + 1)


CASES = {10: [3, 7], 11: [15]}


def test_evaluate_poly(world):
    w, logN = world, world.pset["logN"]
    ct, z = two_party(w)
    for d in CASES[logN]:
        coeffs = w.rng.uniform(-1, 1, d + 1).astype(np.complex128)
        if d == 15:
            coeffs[6] = 0.5 - 0.75j                                    # one complex coefficient
        need = math.ceil(math.log2(d + 1)) + 1
        res = w.ev.EvaluatePolyNew(ct, coeffs, w.rlk)
        assert res.Level() == ct.Level() - need and res.Scale == w.params.Scale() and res.ids == ct.ids
        got = w.dec.Decrypt(res, w.skSet).Value
        ref = np.polyval(coeffs[::-1], z)
        bound = w.bound(12) + math.log2(sum(k * abs(c) for k, c in enumerate(coeffs)))
        err = _max_log2_err(got, ref)
        print("EvaluatePolyNew logN=%d d=%d: 2^%.1f, bound 2^%.1f" % (logN, d, err, bound))
        assert err <= bound
        from mkhe_kklss_amd._abi import MkheError
        low = w.ev.DropLevelNew(ct, ct.Level() - (need - 1))
        with pytest.raises(MkheError):
            w.ev.EvaluatePolyNew(low, coeffs, w.rlk)
        # and exactly enough levels: the result arrives at level 0
        res = w.ev.EvaluatePolyNew(w.ev.DropLevelNew(ct, ct.Level() - need), coeffs, w.rlk, scale=w.params.Scale() / 2)
        assert res.Level() == 0 and res.Scale == w.params.Scale() / 2
        assert _max_log2_err(w.dec.Decrypt(res, w.skSet).Value, ref) <= bound + 1
