"""mkbfv.LinearTransform end to end (-m gpu): keygen -> EncryptMsgNew -> LinearTransformNew / LinearTransformBatch -> Decrypt.  Two parties,
small_bfv(10, 3) and small_bfv(11, 3), T = 65537, seeded HostSampler (insecure_test_only), device encoder.  BFV decryption is exact, so every result
is an equality of centred values against the numpy model of tests/test_bfv_lintrans_host.py (np.roll per slot row, a row swap); the noise budget
of each result is asserted positive, and printed, before the equality.

Noise (include/mkhe.h, "BFV plaintext linear transform"): a baby rotation adds one key-switch error, the product multiplies the noise by at most
N T/2 per diagonal, each giant rotation and the conjugation add one key-switch error; the result is exact while the total stays below Q / (2T)."""
import types

import numpy as np
import pytest

import harness_bfv as HB
import test_bfv_lintrans_host as LH

pytestmark = pytest.mark.gpu

T = LH.T
INDICES, SWAPPED = LH.INDICES, LH.SWAPPED


def centre(v):
    r = np.mod(np.asarray(v, dtype=np.int64), T)
    return np.where(r > T // 2, r - T, r)


def make_world(logN):
    from mkhe_kklss_amd import mkbfv, mkrlwe
    pset = HB.small_bfv(logN, 3)
    assert pset["T"] == T
    params = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], T)
    params.GenDefaultCRS(seed=1234)
    sampler = mkrlwe.HostSampler(np.random.default_rng(50 + logN), insecure_test_only=True)
    kgen = mkbfv.NewKeyGenerator(params, sampler)
    w = types.SimpleNamespace(params=params, N=1 << logN, n=1 << (logN - 1), names=["user0", "user1"], rng=np.random.default_rng(7 * logN),
                              kgen=kgen, enc=mkbfv.NewEncryptor(params, sampler, encoder="device"), dec=mkbfv.NewDecryptor(params, encoder="device"),
                              ev=mkbfv.NewEvaluator(params), skSet=mkrlwe.NewSecretKeySet(), pkSet=mkrlwe.NewPublicKeyKeySet(),
                              rks=mkrlwe.RotationKeySet(), cks=mkrlwe.ConjugationKeySet(), sks={}, mkbfv=mkbfv, mkrlwe=mkrlwe)
    for name in w.names:
        sk, pk = kgen.GenKeyPair(name)
        w.sks[name] = sk
        w.skSet.AddSecretKey(sk)
        w.pkSet.AddPublicKey(pk)
        w.cks.AddConjugationKey(kgen.GenConjugationKey(sk))
    return w


@pytest.fixture(scope="module", params=[10, 11])
def world(request):
    return make_world(request.param)


def provide_keys(w, lt):
    """a CRS and a rotation key of every party for every index of lt.Rotations()"""
    for r in lt.Rotations():
        if r not in w.params.CRS:
            w.params.AddCRS(r, seed=4000 + r)
        for name in w.names:
            if r not in w.rks.Value.get(name, {}):
                w.rks.AddRotationKey(w.kgen.GenRotationKey(r, w.sks[name]))


def rows(w):
    return w.rng.integers(-(T // 2), T // 2 + 1, (2, w.n)).astype(np.int64)


def encrypt(w, z):
    """z [2][n] -> a ciphertext over both parties: the message under user0 plus an encryption of zero under user1"""
    ca = w.enc.EncryptMsgNew(w.mkbfv.Message(z.reshape(-1)), w.pkSet.GetPublicKey("user0"))
    cb = w.enc.EncryptMsgNew(w.mkbfv.Message(np.zeros(w.N, dtype=np.int64)), w.pkSet.GetPublicKey("user1"))
    return w.ev.AddNew(ca, cb)


def check_result(w, what, ct, want):
    """the budget first (printed), then the equality of centred values"""
    assert ct.ids == w.names and ct.Level() == w.params.MaxLevel()
    budget = w.dec.NoiseBudget(ct, w.skSet)
    print("%s, N = %d: noise budget %d bits" % (what, w.N, budget))
    assert budget > 0
    assert (w.dec.Decrypt(ct, w.skSet).Value.reshape(2, w.n) == centre(want)).all(), what


def run(w, what, lt, d, e, z=None, want=None):
    """fused and fused=False give the same ciphertext, and it decrypts to the model"""
    provide_keys(w, lt)
    z = rows(w) if z is None else z
    ct = encrypt(w, z)
    print("%s: input budget %d bits, n1 = %d, babies %r, giants %r + %r" % (what, w.dec.NoiseBudget(ct, w.skSet), lt.plan.n1, lt.plan.babies,
                                                                          lt.giants_d, lt.giants_e))
    fused = w.ev.LinearTransformNew(ct, lt, w.rks, w.cks)
    check_result(w, what, fused, LH.defining_sum(z, d, e) if want is None else want)
    single = w.ev.LinearTransformNew(ct, lt, w.rks, w.cks, fused=False)
    assert (single.download() == fused.download()).all(), what + ": fused=False differs"
    return ct, fused


@pytest.mark.parametrize("n1", [None, 8])
def test_row_preserving_diagonals(world, n1):
    w = world
    d = {k: rows(w) for k in INDICES}
    lt = w.mkbfv.LinearTransform(w.params, d, n1=n1)
    assert not lt.NeedsConjugation() and (n1 is None or lt.plan.n1 == n1)
    provide_keys(w, lt)
    z = rows(w)
    ct = encrypt(w, z)
    out = w.ev.LinearTransformNew(ct, lt, w.rks)                     # no ckSet: none is needed
    check_result(w, "diagonals, n1 = %r" % n1, out, LH.defining_sum(z, d, {}))
    assert (w.ev.LinearTransformNew(ct, lt, w.rks, fused=False).download() == out.download()).all()


def test_swapped_diagonals_alone(world):
    w = world
    e = {k: rows(w) for k in SWAPPED}
    lt = w.mkbfv.LinearTransform(w.params, {}, e)
    assert lt.NeedsConjugation() and not lt.giants_d
    run(w, "swapped alone", lt, {}, e)


@pytest.mark.parametrize("n1", [None, 8])
def test_both_parts_together(world, n1):
    w = world
    d, e = {k: rows(w) for k in INDICES}, {k: rows(w) for k in SWAPPED}
    d[1] = d[1][0]                                                   # a [n] array: the same diagonal in both rows
    lt = w.mkbfv.LinearTransform(w.params, d, e, n1=n1)
    assert lt.NeedsConjugation()
    full = dict(d)
    full[1] = np.stack([d[1], d[1]])
    run(w, "both parts, n1 = %r" % n1, lt, full, e)


def test_from_matrix_8x8(world):
    w, dim = world, 8
    M = w.rng.integers(-(T // 2), T // 2 + 1, (dim, dim)).astype(np.int64)
    v = w.rng.integers(-(T // 2), T // 2 + 1, (2, dim)).astype(np.int64)
    z = np.stack([LH.replicated(v[0], w.n), LH.replicated(v[1], w.n)])
    want = np.stack([LH.replicated(M.astype(object) @ v[r].astype(object) % T, w.n) for r in range(2)]).astype(np.int64)
    lt = w.mkbfv.LinearTransform.FromMatrix(w.params, M)
    assert not lt.NeedsConjugation()
    run(w, "FromMatrix 8 x 8", lt, None, None, z, want)


def test_from_matrix_16x16_blocks(world):
    w, dim = world, 8
    M = w.rng.integers(-(T // 2), T // 2 + 1, (2 * dim, 2 * dim)).astype(np.int64)
    v = w.rng.integers(-(T // 2), T // 2 + 1, 2 * dim).astype(np.int64)
    z = np.stack([LH.replicated(v[:dim], w.n), LH.replicated(v[dim:], w.n)])
    mv = (M.astype(object) @ v.astype(object) % T).astype(np.int64)
    lt = w.mkbfv.LinearTransform.FromMatrix(w.params, M, blocks=True)
    assert lt.NeedsConjugation()
    run(w, "FromMatrix 16 x 16 blocks", lt, None, None, z, np.stack([LH.replicated(mv[:dim], w.n), LH.replicated(mv[dim:], w.n)]))


def test_batch_of_three_equals_three_single_calls(world):
    w = world
    d, e = {k: rows(w) for k in (0, 1, 5, 17)}, {3: rows(w)}
    lt = w.mkbfv.LinearTransform(w.params, d, e, n1=8)
    provide_keys(w, lt)
    zs = [rows(w) for _ in range(3)]
    cts = [encrypt(w, z) for z in zs]
    batch = w.ev.LinearTransformBatch(cts, lt, w.rks, w.cks)
    assert len(batch) == 3
    for k in range(3):
        check_result(w, "batch item %d" % k, batch[k], LH.defining_sum(zs[k], d, e))
        assert (batch[k].download() == w.ev.LinearTransformNew(cts[k], lt, w.rks, w.cks).download()).all(), k
    unfused = w.ev.LinearTransformBatch(cts, lt, w.rks, w.cks, fused=False)
    for k in range(3):
        assert (unfused[k].download() == batch[k].download()).all(), k


def test_missing_keys_raise_before_any_engine_call(world):
    from mkhe_kklss_amd._abi import MkheError
    w = world
    ct = encrypt(w, rows(w))
    before = ct.download()
    lt = w.mkbfv.LinearTransform(w.params, {0: rows(w), 1: rows(w)}, {0: rows(w)})
    provide_keys(w, lt)
    assert w.ev.LinearTransformNew(ct, lt, w.rks, w.cks) is not None
    with pytest.raises(MkheError, match="ckSet"):
        w.ev.LinearTransformNew(ct, lt, w.rks)
    with pytest.raises(MkheError, match="cannot GetConjugationKey"):
        w.ev.LinearTransformNew(ct, lt, w.rks, w.mkrlwe.ConjugationKeySet())
    with pytest.raises(MkheError, match="cannot GetRotationKeys"):
        w.ev.LinearTransformNew(ct, lt, w.mkrlwe.RotationKeySet(), w.cks)
    nokey = w.mkbfv.LinearTransform(w.params, {0: rows(w), 77: rows(w)}, n1=1)       # index 77: no CRS, no key
    assert 77 in nokey.Rotations() and 77 not in w.params.CRS
    for fused in (True, False):
        with pytest.raises(MkheError, match="no CRS for rotation index 77"):
            w.ev.LinearTransformNew(ct, nokey, w.rks, fused=fused)
    one = w.enc.EncryptMsgNew(w.mkbfv.Message(np.zeros(w.N, dtype=np.int64)), w.pkSet.GetPublicKey("user0"))
    with pytest.raises(MkheError, match="same ids"):
        w.ev.LinearTransformBatch([ct, one], lt, w.rks, w.cks)
    pset = HB.small_bfv(10, 3)
    other = w.mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], T)
    foreign = w.mkbfv.LinearTransform(other, {0: np.ones((2, 512), dtype=np.int64)})
    with pytest.raises(MkheError, match="other parameters"):
        w.ev.LinearTransformNew(ct, foreign, w.rks)
    del foreign
    other.close()
    assert (ct.download() == before).all()
