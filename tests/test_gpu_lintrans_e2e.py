"""Evaluator.LinearTransformNew end to end on the device (-m gpu): device keygen (seeded HostSampler, insecure_test_only) -> EncryptMsgNew -> the transform ->
Decrypt, two parties, complex slots with |z| <= 1, against numpy on the cleartext slots; the fused form against the same schedule through the
single-operation entry points (fused=False), bit for bit.

Bound, in bits of log2|delta|: Scenario.precision_bound(12) + log2(sum_k max_j |d_k[j]| + G), G = the non-zero giant steps.  precision_bound(12) = -log2(scale)
+ logSlots + 12 is the reference's bound for MulPtxt (mkckks_test.go:639); to first order each of the D products brings it once, weighted by the largest
entry of its diagonal, and each giant rotation adds one key-switch error of that order.  Derived, not measured.  The naive evaluation with RotateNew /
MulPtxtNew / AddNew on the same ciphertext (none of the new code) is printed beside it.
Measured on an MI355X: see the table in DESIGN.md, section "Plaintext linear transform"."""
import math
import types

import numpy as np
import pytest

import harness as H
from scenario import Scenario

pytestmark = pytest.mark.gpu

INDICES = [0, 1, 5, 8, 17, 300]


def _max_log2_err(a, b):
    d = np.abs(np.asarray(a) - np.asarray(b))
    return float(np.log2(max(d.real.max(), d.imag.max(), 1e-300)))


def _disc(rng, n, radius):
    return radius * np.sqrt(rng.uniform(0, 1, n)) * np.exp(2j * np.pi * rng.uniform(0, 1, n))


@pytest.fixture(scope="module", params=[10, 11])
def world(request):
    from mkhe_kklss_amd import mkckks, mkrlwe
    pset = H.small_ckks(request.param, nq=4)
    params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], pset["scale"])
    params.GenDefaultCRS(seed=4321)
    sampler = mkrlwe.HostSampler(np.random.default_rng(2025), insecure_test_only=True)
    w = types.SimpleNamespace(params=params, pset=pset, names=["user0", "user1"], rng=np.random.default_rng(23), n=1 << (pset["logN"] - 1),
                              enc=mkckks.NewEncryptor(params, sampler, encoder="device"), dec=mkckks.NewDecryptor(params, encoder="device"),
                              ev=mkckks.NewEvaluator(params), skSet=mkrlwe.NewSecretKeySet(), pkSet=mkrlwe.NewPublicKeyKeySet(),
                              rks=mkrlwe.RotationKeySet(), kgen=mkrlwe.NewKeyGenerator(params, sampler), sks={}, mkckks=mkckks, mkrlwe=mkrlwe)
    for name in w.names:
        sk, pk = w.kgen.GenKeyPair(name)
        w.sks[name] = sk
        w.skSet.AddSecretKey(sk)
        w.pkSet.AddPublicKey(pk)
    w.bound = lambda extra: Scenario.precision_bound(types.SimpleNamespace(scale=pset["scale"], logN=pset["logN"]), extra)
    return w


def provide_keys(w, rots):
    """AddCRS / GenRotationKey for the rotation indices that have no key yet"""
    for r in rots:
        if r and (w.names[0] not in w.rks.Value or r not in w.rks.Value[w.names[0]]):
            if r not in w.params.CRS:
                w.params.AddCRS(r, seed=4321)
            for name in w.names:
                w.rks.AddRotationKey(w.kgen.GenRotationKey(r, w.sks[name]))


def two_party(w, z=None, radius=0.5):
    """user0's message plus user1's: a ciphertext under both keys whose slots lie in the unit disc (z given: split into two halves)"""
    zs = [_disc(w.rng, w.n, radius) for _ in w.names] if z is None else [z / 2, z / 2]
    cts = [w.enc.EncryptMsgNew(w.mkckks.Message(v), w.pkSet.GetPublicKey(name)) for v, name in zip(zs, w.names)]
    ct = w.ev.AddNew(cts[0], cts[1])
    assert ct.ids == sorted(w.names)
    return ct, zs[0] + zs[1]


def apply(diag, z):
    return sum(d * np.roll(z, -k) for k, d in diag.items())


def naive(w, ct, diag):
    """one RotateNew, one MulPtxtNew (with its Rescale) and one AddNew per diagonal: the evaluation a caller writes without the transform"""
    level, acc = ct.Level(), None
    q = float(w.params.Q[level])
    provide_keys(w, [1 << i for i in range(w.pset["logN"] - 1) if any(k >> i & 1 for k in diag)])
    for k, d in diag.items():
        pt = w.mkckks.DeviceEncoder(w.params).Encode(d, level, q)
        term = w.ev.MulPtxtNew(w.ev.RotateNew(ct, k, w.rks), pt, q)
        acc = term if acc is None else w.ev.AddNew(acc, term)
    return acc


def check_transform(w, lt, diag, ct, z, label):
    provide_keys(w, lt.Rotations())
    fused = w.ev.LinearTransformNew(ct, lt, w.rks)
    chain = w.ev.LinearTransformNew(ct, lt, w.rks, fused=False)
    for res in (fused, chain):
        assert res.Level() == lt.level - 1 and res.Scale == w.params.Scale() and res.ids == ct.ids
    assert (fused.download() == chain.download()).all()
    want = apply(diag, z)
    giants = sum(1 for g in lt.plan.giants if g)
    bound = w.bound(12) + math.log2(sum(np.abs(d).max() for d in diag.values()) + giants)
    err = _max_log2_err(w.dec.Decrypt(fused, w.skSet).Value, want)
    err_naive = _max_log2_err(w.dec.Decrypt(naive(w, ct, diag), w.skSet).Value, want)
    print("LinearTransformNew %s logN=%d n1=%d babies=%d giants=%d: 2^%.1f, bound 2^%.1f, naive 2^%.1f"
          % (label, w.pset["logN"], lt.plan.n1, sum(1 for b in lt.plan.babies if b), giants, err, bound, err_naive))
    assert err <= bound
    return fused


@pytest.mark.parametrize("n1", [None, 8])
def test_diagonals(world, n1):
    w = world
    diag = {k: _disc(w.rng, w.n, 1.0) for k in INDICES}
    ct, z = two_party(w)
    level = ct.Level()
    lt = w.mkckks.LinearTransform(w.params, diag, level, n1=n1, keep_coeff=True)
    assert lt.plan == w.mkckks.linear_transform_plan(INDICES, w.n, n1) and len(lt.order) == len(INDICES)
    if n1 == 8:
        assert lt.plan.babies == [0, 1, 4, 5] and lt.plan.giants == [0, 8, 16, 296] and lt.Rotations() == [1, 4, 5, 8, 16, 296]
    check_transform(w, lt, diag, ct, z, "diagonals")
    if n1 == 8:
        # a transform encoded one level below the ciphertext: the ciphertext is dropped to it first, in both forms
        low = w.mkckks.LinearTransform(w.params, diag, level - 1, n1=n1, keep_coeff=True)
        res = check_transform(w, low, diag, ct, z, "diagonals, one level down")
        assert res.Level() == level - 2
        # a ciphertext at another scale than the transform was encoded for: the declared scale follows it
        ct2 = w.ev.DropLevelNew(ct, 0)
        ct2.Scale = ct.Scale * 2
        res = w.ev.LinearTransformNew(ct2, lt, w.rks)
        assert res.Scale == ct2.Scale * lt.pt_scale / float(w.params.Q[level]) == 2 * w.params.Scale()
        assert _max_log2_err(w.dec.Decrypt(res, w.skSet).Value, apply(diag, z) / 2) <= w.bound(12) + math.log2(len(INDICES) + 3)


def test_matrix_on_a_replicated_vector(world):
    w, d = world, 8
    M = (w.rng.uniform(-1, 1, (d, d)) + 1j * w.rng.uniform(-1, 1, (d, d))) / math.sqrt(2)
    v = _disc(w.rng, d, 1.0)
    ct, z = two_party(w, np.tile(v, w.n // d))
    lt = w.mkckks.LinearTransform.FromMatrix(w.params, M, ct.Level(), keep_coeff=True)
    diag = w.mkckks.matrix_diagonals(M, w.n)
    assert sorted(diag) == list(range(d)) and lt.plan.n1 == 2 and lt.Rotations() == [1, 2, 4, 6]
    res = check_transform(w, lt, diag, ct, z, "matrix 8x8")
    got = w.dec.Decrypt(res, w.skSet).Value
    assert _max_log2_err(got, np.tile(M @ v, w.n // d)) <= w.bound(12) + math.log2(sum(np.abs(x).max() for x in diag.values()) + 3)


def test_errors_come_before_any_engine_call(world):
    from mkhe_kklss_amd._abi import MkheError
    w = world
    diag = {k: _disc(w.rng, w.n, 1.0) for k in (0, 3)}
    ct, _ = two_party(w)
    lt = w.mkckks.LinearTransform(w.params, diag, ct.Level())
    provide_keys(w, lt.Rotations())
    with pytest.raises(MkheError):
        w.ev.LinearTransformNew(w.ev.DropLevelNew(ct, 1), lt, w.rks)                       # the ciphertext lies below the transform
    with pytest.raises(MkheError):
        w.ev.LinearTransformNew(ct, lt, w.mkrlwe.RotationKeySet())                         # no rotation key
    partial = w.mkrlwe.RotationKeySet()
    partial.AddRotationKey(w.rks.GetRotationKey(w.names[0], 3))
    with pytest.raises(MkheError):
        w.ev.LinearTransformNew(ct, lt, partial)                                           # ... for one of the parties
    with pytest.raises(MkheError):
        w.ev.LinearTransformNew(ct, lt, w.rks, fused=False)                                # the chain needs keep_coeff=True
    lt0 = w.mkckks.LinearTransform(w.params, diag, 0)
    with pytest.raises(MkheError):
        w.ev.LinearTransformNew(ct, lt0, w.rks)                                            # nothing to rescale into
    with pytest.raises(MkheError):
        w.mkckks.LinearTransform(w.params, {0: np.zeros(w.n - 1)}, 1)
    with pytest.raises(MkheError):
        w.mkckks.LinearTransform(w.params, {1: np.zeros(w.n), 1 + w.n: np.zeros(w.n)}, 1)
    assert w.ev.LinearTransformNew(ct, lt, w.rks).Level() == ct.Level() - 1                # and the evaluator still works


def test_a_single_diagonal_is_mul_ptxt_and_rescale(world):
    w = world
    d = _disc(w.rng, w.n, 1.0)
    ct, z = two_party(w)
    lt = w.mkckks.LinearTransform(w.params, {0: d}, ct.Level(), keep_coeff=True)
    assert lt.Rotations() == [] and lt.pt_scale == float(w.params.Q[ct.Level()])
    res = w.ev.LinearTransformNew(ct, lt, w.mkrlwe.RotationKeySet())                       # no rotation key at all
    ref = w.ev.MulPtxtNew(ct, lt.pt_coeff, lt.pt_scale)
    assert ref.Level() == res.Level() == ct.Level() - 1 and ref.Scale == res.Scale == w.params.Scale()
    assert (res.download() == ref.download()).all()
    assert (w.ev.LinearTransformNew(ct, lt, w.mkrlwe.RotationKeySet(), fused=False).download() == ref.download()).all()
    assert _max_log2_err(w.dec.Decrypt(res, w.skSet).Value, d * z) <= w.bound(12)
