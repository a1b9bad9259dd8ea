"""The noise measures of the three mirrors end to end (-m gpu): two parties, N = 2^10, the device encoder.

mkbfv, small_bfv(10, 3): on a fresh sum of two encryptions and after one and two MulRelinNew, NoiseNorm against the message is the host
computation of tests/test_gpu_bfv_refresh_e2e.py (restated below: download the phase, walk the coefficients as Python integers), NoiseNorm
without the message lies at most 2 above it, NoiseBudget is the model's and does not grow along the chain; a refresh whose flood is
NoiseBits + 20 stays within MaxFloodBits(2) and returns the message.
Secret-key encryption, mkbfv and mkckks: against the same device plaintext the residual is the error e alone, at most 19.
mkckks, small_ckks(10, 4): NoiseNorm of a public-key encryption and of its square is the model on the downloaded phase and plaintext (no bound
is asserted: none is derived in the project).
Merged shares: NoiseNormBatch on what MergeSharesBatch gives for unflooded shares is NoiseNorm with every key in hand."""
import numpy as np
import pytest

import harness as H
import harness_bfv as HB
import noise_model as M

pytestmark = pytest.mark.gpu

LOGN, N = 10, 1 << 10
NAMES = ["user0", "user1"]


def host_noise(phase, plaintext, qs):
    """max |phase - plaintext| over the coefficients, centred mod Q: what the tests did by hand before mkhe_noise_norm"""
    d = (phase.astype(object) - plaintext.astype(object)) % np.array(qs, dtype=object)[:, None]
    return max(abs(v) for v in H.crt_center(d.astype(np.uint64), qs)[0])


def test_bfv_noise_along_a_chain_of_squarings_and_a_refresh_sized_by_it():
    from mkhe_kklss_amd import mkbfv, mkrlwe
    pset = HB.small_bfv(LOGN, 3)
    T, qs = pset["T"], pset["Q"]
    Q = M.product(qs)
    centre = lambda v: np.where(np.mod(v, T) > T // 2, np.mod(v, T) - T, np.mod(v, T))
    params = mkbfv.Parameters(pset["logN"], qs, pset["QMul"], pset["P"], T)
    params.GenDefaultCRS(seed=4330)
    kgen = mkbfv.NewKeyGenerator(params, mkrlwe.HostSampler(np.random.default_rng(2040), insecure_test_only=True))
    enc, dec, ev = mkbfv.NewEncryptor(params, sampler=mkrlwe.DeviceSampler(), encoder="device"), mkbfv.NewDecryptor(params, encoder="device"), mkbfv.NewEvaluator(params)
    ref, host_encoder = mkbfv.NewRefresher(params), mkbfv.Encoder(params)
    rng = np.random.default_rng(71)
    sks, pks, skSet, rlk, ct, msg = {}, {}, mkrlwe.NewSecretKeySet(), mkbfv.RelinearizationKeySet(params), None, 0
    for p in NAMES:
        sks[p], pks[p] = kgen.GenKeyPair(p)
        skSet.AddSecretKey(sks[p])
        rlk.AddRelinearizationKey(kgen.GenRelinearizationKey(sks[p], kgen.GenSecretKey(p)))
        m = rng.integers(-(T // 2), T // 2 + 1, N).astype(np.int64)
        c = enc.EncryptMsgNew(mkbfv.Message(m), pks[p])
        ct, msg = (c, m) if ct is None else (ev.AddNew(ct, c), centre(msg + m))
    budgets = []
    for depth in range(3):
        if depth:
            ct, msg = ev.MulRelinNew(ct, ct, rlk), centre(msg * msg)
        assert (dec.Decrypt(ct, skSet).Value == msg).all()
        phase = dec.DecryptPtxt(ct, skSet)
        by_hand = host_noise(phase, host_encoder.Encode(msg), qs)
        exact, bound, budget = dec.NoiseNorm(ct, skSet, mkbfv.Message(msg)), dec.NoiseNorm(ct, skSet), dec.NoiseBudget(ct, skSet)
        r = M.noise_norm_crt(1, phase.tolist(), None, qs, T)[0]
        print("depth %d: noise %d bits, bound from the invariant value +%d, budget %d of %d bits" % (depth, exact.bit_length(), bound - exact, budget, Q.bit_length()))
        assert exact == by_hand
        assert by_hand <= bound <= by_hand + 2
        assert dec.InvariantNoise(ct, skSet) == r and budget == M.noise_budget(r, Q) and bound == M.bfv_noise_bound(r, T)
        assert dec.NoiseBits(ct, skSet, mkbfv.Message(msg)) == by_hand.bit_length() and dec.NoiseBits(ct, skSet) == bound.bit_length()
        budgets.append(budget)
    assert budgets[0] >= budgets[1] >= budgets[2] > 0

    # the refresh of the worn ciphertext, its flood sized by the measurement that needs no message
    flood_bits = dec.NoiseBits(ct, skSet) + 20
    assert flood_bits <= ref.MaxFloodBits(2)
    shares = [ref.ShareNew(ct, sks[p], pks[p], flood_bits, mkrlwe.DeviceSampler()) for p in NAMES]
    fresh = ref.MergeNew(ct, shares)
    assert (dec.Decrypt(fresh, skSet).Value == msg).all()
    assert dec.NoiseBudget(fresh, skSet) > budgets[2]

    # merged shares: parties that hold only their own key measure what a holder of every key measures
    rdec = mkrlwe.NewDecryptor(params)
    plain = [rdec.ShareNew(ct, sks[p], 0, None) for p in NAMES]
    merged = rdec.MergeSharesBatch([ct], plain)
    pt = mkbfv.DeviceEncoder(params).Encode(msg)
    assert rdec.NoiseNormBatch(merged, pt)[0][0] == rdec.NoiseNorm(ct, skSet, pt) == dec.NoiseNorm(ct, skSet, mkbfv.Message(msg))
    assert rdec.NoiseNormBatch(merged)[0][0] == rdec.NoiseNorm(ct, skSet)
    assert dec.NoiseNormBatch(merged, kind=1)[0][0] == dec.InvariantNoise(ct, skSet)
    params.close()


def test_secret_key_encryptions_carry_the_error_alone():
    """SecretKeyEncryptor(..., encoder="device"): c0 = pt + e - c1 s, so against the same device plaintext the residual is e, |e| <= 19"""
    from mkhe_kklss_amd import mkbfv, mkckks, mkrlwe
    rng = np.random.default_rng(73)
    bset = HB.small_bfv(LOGN, 3)
    T = bset["T"]
    params = mkbfv.Parameters(bset["logN"], bset["Q"], bset["QMul"], bset["P"], T)
    sk = mkbfv.NewKeyGenerator(params, mkrlwe.HostSampler(np.random.default_rng(2041), insecure_test_only=True)).GenSecretKey("user0")
    skSet = mkrlwe.NewSecretKeySet()
    skSet.AddSecretKey(sk)
    m = mkbfv.Message(rng.integers(-(T // 2), T // 2 + 1, N).astype(np.int64))
    ct = mkbfv.NewSecretKeyEncryptor(params, sk, mkrlwe.DeviceSampler(), encoder="device").EncryptMsgNew(m)
    dec = mkbfv.NewDecryptor(params, encoder="device")
    e = dec.NoiseNorm(ct, skSet, m)
    print("mkbfv secret-key encryption: |e| = %d, the bound without the message %d, budget %d bits" % (e, dec.NoiseNorm(ct, skSet), dec.NoiseBudget(ct, skSet)))
    assert 0 < e <= 19 and e <= dec.NoiseNorm(ct, skSet) <= e + 2
    params.close()

    cset = H.small_ckks(LOGN, 4)
    params = mkckks.Parameters(cset["logN"], cset["Q"], cset["P"], cset["scale"])
    sk = mkrlwe.NewKeyGenerator(params, mkrlwe.HostSampler(np.random.default_rng(2042), insecure_test_only=True)).GenSecretKey("user0")
    skSet = mkrlwe.NewSecretKeySet()
    skSet.AddSecretKey(sk)
    z = mkckks.Message(np.full(N // 2, complex(0.1, 1.0) / 2) + rng.uniform(-0.05, 0.05, N // 2))
    ct = mkckks.NewSecretKeyEncryptor(params, sk, mkrlwe.DeviceSampler(), encoder="device").EncryptMsgNew(z)
    dec = mkckks.NewDecryptor(params, encoder="device")
    e = dec.NoiseNorm(ct, skSet, z)
    print("mkckks secret-key encryption: |e| = %d" % e)
    assert 0 < e <= 19 and dec.NoiseBits(ct, skSet, z) == e.bit_length()
    params.close()


def test_ckks_noise_of_a_public_key_encryption_and_of_its_square_is_the_model():
    from mkhe_kklss_amd import mkckks, mkrlwe
    pset = H.small_ckks(LOGN, 4)
    params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], pset["scale"])
    params.GenDefaultCRS(seed=4331)
    kgen = mkrlwe.NewKeyGenerator(params, mkrlwe.HostSampler(np.random.default_rng(2043), insecure_test_only=True))
    enc, dec, ev = mkckks.NewEncryptor(params, sampler=mkrlwe.DeviceSampler(), encoder="device"), mkckks.NewDecryptor(params, encoder="device"), mkckks.NewEvaluator(params)
    encoder, rng = mkckks.DeviceEncoder(params), np.random.default_rng(79)
    sks, skSet, rlk, ct, z = {}, mkrlwe.NewSecretKeySet(), mkrlwe.RelinearizationKeySet(params), None, 0
    for p in NAMES:
        sks[p], pk = kgen.GenKeyPair(p)
        skSet.AddSecretKey(sks[p])
        rlk.AddRelinearizationKey(kgen.GenRelinearizationKey(sks[p], kgen.GenSecretKey(p)))
        zp = np.full(N // 2, complex(0.1, 1.0) / 2) + rng.uniform(-0.05, 0.05, N // 2)
        c = enc.EncryptMsgNew(mkckks.Message(zp), pk)
        ct, z = (c, zp) if ct is None else (ev.AddNew(ct, c), z + zp)
    for c, want in ((ct, z), (ev.MulRelinNew(ct, ct, rlk), z * z)):
        qs = pset["Q"][:c.Level() + 1]
        phase = mkrlwe.Decryptor.Decrypt(dec, c, skSet).download()[0]
        plaintext = encoder.Encode(want, c.Level(), c.ScalingFactor()).download()[0]
        got = dec.NoiseNorm(c, skSet, mkckks.Message(want))
        print("mkckks level %d, scale 2^%.2f: residual of %d bits" % (c.Level(), np.log2(c.ScalingFactor()), got.bit_length()))
        assert got == M.noise_norm_crt(0, phase.tolist(), plaintext.tolist(), qs)[0] == host_noise(phase, plaintext, qs)
        assert dec.NoiseBits(c, skSet, mkckks.Message(want)) == got.bit_length()
    # merged shares on the CKKS side, two ciphertexts in one call
    shares = [dec.ShareBatch([ct, ct], sks[p], 0, None) for p in NAMES]
    merged = dec.MergeSharesBatch([ct, ct], shares)
    ref = encoder.Encode(z, ct.Level(), ct.ScalingFactor())
    assert [r for r, _ in dec.NoiseNormBatch(merged, ref)] == [dec.NoiseNorm(ct, skSet, mkckks.Message(z))] * 2
    params.close()
