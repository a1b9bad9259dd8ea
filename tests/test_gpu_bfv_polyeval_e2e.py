"""MK-BFV polynomial evaluation end to end (-m gpu): keygen -> device encoder -> EncryptMsgNew -> EvaluatePolyNew -> Decrypt, everything on the device.
Two parties, the input is the sum of one fresh ciphertext from each, T = 65537, seeded HostSampler (insecure_test_only).  Messages and coefficients
are uniform on the full centred range; BFV decryption is exact, so every comparison is an equality with Horner mod T in every slot.

Parameter sets (checked on the CPU at N = 2^10 before this test was written: a product costs about 28 bits of invariant-noise budget, a full-range
weighted sum 14 to 17): degree 7 on small_bfv(10, 3), degree 15 on small_bfv(10, 4), degree 63 on small_bfv(10, 5), with 41, 45 and 34 bits left on
the CPU.  Degree 15 on three primes and degree 63 on four have no budget left.  The test asks for 20 bits: the margin under the lowest CPU figure
absorbs another seed's few bits.

Budgets the device reports (Decryptor.NoiseBudget of the result, the seeds below): degree 7: 35 bits, degree 15: 48 bits, degree 63: 32 bits;
fused=False leaves the same 35 and 48 bits at degrees 7 and 15."""
import types

import numpy as np
import pytest

import harness_bfv as HB

pytestmark = pytest.mark.gpu

T = 65537
N = 1 << 10
CASES = {7: 3, 15: 4, 63: 5}                                     # degree -> primes of Q


def centre(v):
    r = np.mod(np.asarray(v, dtype=np.int64), T)
    return np.where(r > T // 2, r - T, r)


def horner(coeffs, x):
    acc = np.zeros_like(x)
    for c in reversed(coeffs):
        acc = np.mod(acc * x + int(c), T)
    return centre(acc)


def make_world(nq):
    from mkhe_kklss_amd import mkbfv, mkrlwe
    pset = HB.small_bfv(10, nq)
    params = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], T)
    params.GenDefaultCRS(seed=779)
    sampler = mkrlwe.HostSampler(np.random.default_rng(43 + nq), insecure_test_only=True)
    kgen = mkbfv.NewKeyGenerator(params, sampler)
    w = types.SimpleNamespace(params=params, names=["user0", "user1"], rng=np.random.default_rng(8 + nq),
                              enc=mkbfv.NewEncryptor(params, sampler, encoder="device"), dec=mkbfv.NewDecryptor(params, encoder="device"),
                              ev=mkbfv.NewEvaluator(params), skSet=mkrlwe.NewSecretKeySet(), pkSet=mkrlwe.NewPublicKeyKeySet(),
                              rlk=mkbfv.RelinearizationKeySet(params), mkbfv=mkbfv)
    for n in w.names:
        sk, pk = kgen.GenKeyPair(n)
        w.skSet.AddSecretKey(sk)
        w.pkSet.AddPublicKey(pk)
        w.rlk.AddRelinearizationKey(kgen.GenRelinearizationKey(sk, kgen.GenSecretKey(n)))
    return w


@pytest.fixture(scope="module")
def worlds():
    made = {}

    def get(nq):
        if nq not in made:
            made[nq] = make_world(nq)
        return made[nq]
    yield get
    for w in made.values():
        w.params.close()


def reseed(w, tag):
    """every test draws from its own stream, whatever ran before it"""
    w.rng = np.random.default_rng([len(w.params.Q), tag])


def full_range(w, n=N):
    return w.rng.integers(-(T // 2), T // 2 + 1, n).astype(np.int64)


def two_party_input(w, msg=None):
    """-> (message, ciphertext over both parties): the sum of one fresh ciphertext from each"""
    a = full_range(w)
    b = full_range(w) if msg is None else centre(np.asarray(msg, dtype=np.int64) - a)
    ca = w.enc.EncryptMsgNew(w.mkbfv.Message(a), w.pkSet.GetPublicKey("user0"))
    cb = w.enc.EncryptMsgNew(w.mkbfv.Message(b), w.pkSet.GetPublicKey("user1"))
    return centre(a + b), w.ev.AddNew(ca, cb)


def decrypt(w, ct):
    return w.dec.Decrypt(ct, w.skSet).Value


@pytest.mark.parametrize("degree", sorted(CASES))
def test_polynomial_of_a_two_party_ciphertext(worlds, degree):
    w = worlds(CASES[degree])
    reseed(w, degree)
    x, ct = two_party_input(w)
    coeffs = [int(c) for c in full_range(w, degree + 1)]
    res = w.ev.EvaluatePolyNew(ct, coeffs, w.rlk)
    assert isinstance(res, w.mkbfv.Ciphertext) and res.ids == w.names and res.Level() == w.params.MaxLevel()
    want = horner(coeffs, x)
    budget = w.dec.NoiseBudget(res, w.skSet)
    print("degree %d on %d primes: noise budget left %.1f bits" % (degree, CASES[degree], budget))
    assert (decrypt(w, res) == want).all()
    assert budget >= 20
    if degree in (7, 15):
        plain = w.ev.EvaluatePolyNew(ct, coeffs, w.rlk, fused=False)
        print("degree %d, fused=False: noise budget left %.1f bits" % (degree, w.dec.NoiseBudget(plain, w.skSet)))
        assert (decrypt(w, plain) == want).all()
        if degree == 7:         # m = 4, g = 2: ONE giant product, and one pair under mkhe_bfv_mul_relin_sum is mkhe_bfv_mul_relin bit for bit
            assert (plain.download() == res.download()).all()
        else:                   # m = 4, g = 4: three products under one Quantize and one tail -- another ciphertext of the same values
            assert (plain.download() != res.download()).any()


def test_two_polynomials_share_one_call(worlds):
    w = worlds(3)
    reseed(w, 100)
    x, ct = two_party_input(w)
    polys = [[int(c) for c in full_range(w, d + 1)] for d in (7, 5)]
    res = w.ev.EvaluatePolysNew(ct, polys, w.rlk)
    assert len(res) == 2
    for r, p in zip(res, polys):
        assert (decrypt(w, r) == horner(p, x)).all()


def test_lookup_table_by_interpolation(worlds):
    w = worlds(3)
    reseed(w, 101)
    xs = [int(v) for v in w.rng.choice(T, 8, replace=False)]
    ys = [int(v) for v in w.rng.integers(0, T, 8)]
    coeffs = w.mkbfv.interpolate(xs, ys, T)
    assert len(coeffs) == 8
    pick = w.rng.integers(0, 8, N)
    msg, ct = two_party_input(w, np.array(xs, dtype=np.int64)[pick])
    assert (msg == centre(np.array(xs)[pick])).all()
    res = w.ev.EvaluatePolyNew(ct, coeffs, w.rlk)
    assert (decrypt(w, res) == centre(np.array(ys, dtype=np.int64)[pick])).all()


def test_constants_and_weighted_sums_decrypt_exactly(worlds):
    w = worlds(3)
    reseed(w, 102)
    a, ca = two_party_input(w)
    b, cb = two_party_input(w)
    for c in (0, 1, -1, T // 2, -(T // 2), 12345, 3 * T + 2):
        assert (decrypt(w, w.ev.AddConstNew(ca, c)) == centre(a + c)).all(), c
    for k in (1, -1, 2, T // 2, -(T // 2), 257, T + 3):
        assert (decrypt(w, w.ev.MulConstNew(ca, k)) == centre(a * k)).all(), k
    assert (decrypt(w, w.ev.MulConstNew(ca, 0)) == 0).all()
    res = w.ev.LinCombNew([ca, cb], [3, -2], 7)
    assert (decrypt(w, res) == centre(3 * a - 2 * b + 7)).all()
    assert (w.ev.LinCombNew([ca, cb], [3, -2], 7, fused=False).download() == res.download()).all()      # mkhe_ct_lincomb: the same bits
    rows = w.ev.LinCombsNew([ca, cb], [[3, -2], [0, 0], [T // 2, 1]], [7, -5, 0])
    assert (decrypt(w, rows[0]) == centre(3 * a - 2 * b + 7)).all()
    assert (decrypt(w, rows[1]) == -5).all()
    assert (decrypt(w, rows[2]) == centre(centre((T // 2) * a) + b)).all()


def test_add_const_moves_one_coefficient_per_limb(worlds):
    from mkhe_kklss_amd import mkbfv
    w = worlds(3)
    reseed(w, 103)
    _, ct = two_party_input(w)
    before, after = ct.download(), w.ev.AddConstNew(ct, 4242).download()
    want = before.copy()
    up = mkbfv.bfv_lincomb_consts(w.params.Q, T, [[1]], [4242])[0, 0]
    for l, q in enumerate(w.params.Q):
        want[0, l, 0] = (int(before[0, l, 0]) + int(up[l])) % q
    assert (after == want).all()
    assert (after != before).sum() <= len(w.params.Q)


def test_checks_come_before_any_engine_call(worlds):
    from mkhe_kklss_amd._abi import MkheError
    w = worlds(3)
    reseed(w, 104)
    _, ct = two_party_input(w)
    for bad in ([1], [0, 0, 0], [1] * 257):
        with pytest.raises(MkheError, match="EvaluatePolysNew"):
            w.ev.EvaluatePolyNew(ct, bad, w.rlk)
    with pytest.raises(MkheError, match="LinCombsNew"):
        w.ev.LinCombsNew([ct] * 17, [[1] * 17], [0])
    with pytest.raises(MkheError, match="LinCombsNew"):
        w.ev.LinCombsNew([ct], [[1]] * 65, [0] * 65)
    with pytest.raises(MkheError, match="LinCombsNew"):
        w.ev.LinCombsNew([ct], [[1, 2]], [0])
