"""EvaluateChebyshevNew, LinCombsNew and EvaluatePolyNew(fused=True) of mkckks.Evaluator end to end on the device (-m gpu), in the manner of
tests/test_gpu_polyeval_e2e.py: device keygen (seeded HostSampler, insecure_test_only) -> EncryptMsgNew -> the operation -> Decrypt, two parties,
real slots in the interval, against numpy.polynomial.chebyshev on the cleartext slots.

Bound, in bits of log2|delta| (Scenario.precision_bound(extra) = -log2(scale) + logSlots + extra, the reference's own, 12 extra bits for a MulRelin):
  EvaluateChebyshevNew  bound(12) + log2(sum_k k^2 |c_k|): the MulRelin bound, propagated to first order through T_k, whose derivative is at most k^2
                        on [-1, 1].  The change of variable divides the input error by (b - a) / 2: nothing is added for b - a > 2, log2(2 / (b - a))
                        for a narrower interval.
  sigmoid               |decrypted - sigmoid(x)| <= E_approx + 2^bound, E_approx = the error of the cleartext series on the same slots.
Measured on an MI355X (log2|delta| / bound): see the table in DESIGN.md, section "Chebyshev evaluation"."""
import math
import types

import numpy as np
import pytest
from numpy.polynomial import chebyshev as NC

import harness as H
from scenario import Scenario

pytestmark = pytest.mark.gpu

PSETS = {(10, 6): H.small_ckks(10, nq=6), (11, 8): H.small_ckks(11, nq=8), (11, 9): H.small_ckks(11, nq=9)}
_WORLDS = {}


def _max_log2_err(a, b):
    d = np.abs(np.asarray(a) - np.asarray(b))
    return float(np.log2(max(d.real.max(), d.imag.max(), 1e-300)))


def world(key):
    """one world per parameter set, built at its first use and shared by the tests of this file"""
    if key in _WORLDS:
        return _WORLDS[key]
    from mkhe_kklss_amd import mkckks, mkrlwe
    pset = PSETS[key]
    params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], pset["scale"])
    params.GenDefaultCRS(seed=4321)
    sampler = mkrlwe.HostSampler(np.random.default_rng(2024), insecure_test_only=True)
    kgen = mkrlwe.NewKeyGenerator(params, sampler)
    w = types.SimpleNamespace(params=params, pset=pset, names=["user0", "user1"], rng=np.random.default_rng(list(key)), n=1 << (pset["logN"] - 1),
                              enc=mkckks.NewEncryptor(params, sampler, encoder="device"), dec=mkckks.NewDecryptor(params, encoder="device"),
                              ev=mkckks.NewEvaluator(params), skSet=mkrlwe.NewSecretKeySet(), pkSet=mkrlwe.NewPublicKeyKeySet(),
                              rlk=mkrlwe.RelinearizationKeySet(params), mkckks=mkckks)
    for name in w.names:
        sk, pk = kgen.GenKeyPair(name)
        w.skSet.AddSecretKey(sk)
        w.pkSet.AddPublicKey(pk)
        w.rlk.AddRelinearizationKey(kgen.GenRelinearizationKey(sk, kgen.GenSecretKey(name)))
    w.bound = lambda extra: Scenario.precision_bound(types.SimpleNamespace(scale=pset["scale"], logN=pset["logN"]), extra)
    _WORLDS[key] = w
    return w


def two_party(w, a, b):
    """user0's message plus user1's: a ciphertext under both keys whose slots are real and lie in [a, b]"""
    zs = [w.rng.uniform(a / 2, b / 2, w.n).astype(np.complex128) for _ in w.names]
    cts = [w.enc.EncryptMsgNew(w.mkckks.Message(z), w.pkSet.GetPublicKey(name)) for z, name in zip(zs, w.names)]
    ct = w.ev.AddNew(cts[0], cts[1])
    assert ct.ids == sorted(w.names)
    return ct, (zs[0] + zs[1]).real


def cheb_bound(w, coeffs, a, b):
    return w.bound(12) + math.log2(sum(k * k * abs(c) for k, c in enumerate(coeffs))) + (math.log2(2 / (b - a)) if b - a < 2 else 0)


def need(d, a, b):
    return (0 if (a, b) == (-1, 1) else 1) + math.ceil(math.log2(d + 1)) + 1


@pytest.mark.parametrize("key,d,a,b", [((10, 6), 7, -1, 1), ((11, 8), 15, -3, 5)], ids=["d7-unit", "d15-m3p5"])
def test_random_series(key, d, a, b):
    w = world(key)
    ct, x = two_party(w, a, b)
    coeffs = w.rng.uniform(-1, 1, d + 1)
    res = w.ev.EvaluateChebyshevNew(ct, coeffs, (a, b), w.rlk)
    assert res.Level() == ct.Level() - need(d, a, b) and res.Scale == w.params.Scale() and res.ids == ct.ids
    got = w.dec.Decrypt(res, w.skSet).Value
    ref = NC.chebval((2 * x - a - b) / (b - a), coeffs)
    err, bound = _max_log2_err(got, ref), cheb_bound(w, coeffs, a, b)
    print("EvaluateChebyshevNew logN=%d d=%d on (%g, %g): 2^%.1f, bound 2^%.1f" % (key[0], d, a, b, err, bound))
    assert err <= bound
    from mkhe_kklss_amd._abi import MkheError
    with pytest.raises(MkheError):
        w.ev.EvaluateChebyshevNew(w.ev.DropLevelNew(ct, ct.Level() - (need(d, a, b) - 1)), coeffs, (a, b), w.rlk)
    # exactly enough levels and another target scale: the result arrives at level 0
    res = w.ev.EvaluateChebyshevNew(w.ev.DropLevelNew(ct, ct.Level() - need(d, a, b)), coeffs, (a, b), w.rlk, scale=w.params.Scale() / 2)
    assert res.Level() == 0 and res.Scale == w.params.Scale() / 2
    assert _max_log2_err(w.dec.Decrypt(res, w.skSet).Value, ref) <= bound + 1


def test_sigmoid_degree_31():
    w, d, a, b = world((11, 9)), 31, -8, 8
    sigmoid = lambda v: 1 / (1 + np.exp(-v))
    coeffs = w.mkckks.chebyshev_approx(sigmoid, a, b, d)
    ct, x = two_party(w, a, b)
    res = w.ev.EvaluateChebyshevNew(ct, coeffs, (a, b), w.rlk)
    assert res.Level() == ct.Level() - need(d, a, b) and res.Scale == w.params.Scale()
    got = w.dec.Decrypt(res, w.skSet).Value
    series = NC.chebval(x / 8, coeffs)
    e_approx, bound = np.abs(series - sigmoid(x)).max(), cheb_bound(w, coeffs, a, b)
    print("sigmoid d=31 on (-8, 8), logN=11: against the series 2^%.1f, bound 2^%.1f; against the sigmoid %.3g, E_approx %.3g"
          % (_max_log2_err(got, series), bound, np.abs(got - sigmoid(x)).max(), e_approx))
    assert np.abs(got - sigmoid(x)).max() <= e_approx + 2.0 ** bound


def _same(a, b):
    return a.Level() == b.Level() and a.Scale == b.Scale and a.ids == b.ids and (a.download() == b.download()).all()


@pytest.mark.parametrize("key,d,a,b", [((10, 6), 7, -1, 1), ((11, 9), 31, -8, 8)], ids=["d7", "d31"])
def test_fused_equals_unfused_bit_for_bit(key, d, a, b):
    w = world(key)
    ct, _ = two_party(w, a, b)
    coeffs = w.rng.uniform(-1, 1, d + 1)
    assert _same(w.ev.EvaluateChebyshevNew(ct, coeffs, (a, b), w.rlk, fused=True), w.ev.EvaluateChebyshevNew(ct, coeffs, (a, b), w.rlk, fused=False))


def test_evaluate_poly_fused_equals_unfused_bit_for_bit():
    w, d = world((11, 8)), 15
    ct, _ = two_party(w, -1, 1)
    coeffs = w.rng.uniform(-1, 1, d + 1).astype(np.complex128)
    coeffs[6] = 0.5 - 0.75j
    fused = w.ev.EvaluatePolyNew(ct, coeffs, w.rlk, fused=True)
    assert fused.Level() == ct.Level() - 5 and _same(fused, w.ev.EvaluatePolyNew(ct, coeffs, w.rlk)) and _same(fused, w.ev.EvaluatePolyNew(ct, coeffs, w.rlk, fused=False))


@pytest.mark.parametrize("rescale", [True, False])
def test_lincombs_rows_equal_lincomb(rescale):
    w = world((10, 6))
    (c0, x0), (c1, x1), (c2, _) = two_party(w, -1, 1), two_party(w, -1, 1), two_party(w, -1, 1)
    c1 = w.ev.DropLevelNew(c1, 1)                                           # inputs at different levels: the work level is the lowest
    rows, consts = [[0.5, -1.25 + 0.5j, 0], [1j, 0, 0]], [0.125, -0.25j]      # c2 is zero in every row: dropped; a zero inside the table stays
    S = w.params.Scale()
    scales = [S, S / 3] if rescale else [c0.Scale, c0.Scale * 2]
    outs = w.ev.LinCombsNew([c0, c1, c2], rows, consts, scales=scales, rescale=rescale)
    assert len(outs) == 2
    for out, r, c, s in zip(outs, rows, consts, scales):
        assert out.Scale == s and out.Level() == c1.Level() - (1 if rescale else 0)
        assert _same(out, w.ev.LinCombNew([c0, c1, c2], r, c, scale=s, rescale=rescale))
    if rescale:                                                             # (without one the weights are rounded at ratio 1 or 2: equality only)
        got = w.dec.Decrypt(outs[0], w.skSet).Value
        assert _max_log2_err(got, 0.5 * x0 + (-1.25 + 0.5j) * x1 + 0.125) <= w.bound(8) + math.log2(0.5 + abs(-1.25 + 0.5j) + 1)
    from mkhe_kklss_amd._abi import MkheError
    for bad in (lambda: w.ev.LinCombsNew([c0, c1], rows, consts), lambda: w.ev.LinCombsNew([c0, c1, c2], rows, consts[:1]),
                lambda: w.ev.LinCombsNew([c0, c1, c2], rows, consts, scales=[S]), lambda: w.ev.LinCombsNew([c0, c1, c2], [rows[0]] * 17, [0] * 17),
                lambda: w.ev.LinCombsNew([], [], [])):
        with pytest.raises(MkheError):
            bad()
