"""Threshold secret keys end to end (-m gpu), N = 2^10: alice's key is shared 2-of-3 among bob, carol and dave, alice goes offline, and a
ciphertext over {alice, bob} (a squared sum: one MulRelinNew) is decrypted without her.  The active holders turn their Shamir shares into additive
keys, publish ordinary flooded decryption shares under alice's id, anyone folds them, bob adds his own share, and the merge runs unchanged.  Once
with exactly t = 2 active holders (carol, dave) and once with all three (a superset of t; bob is then a holder AND a party).

mkckks: every slot within FloodSlotBound(k - 1 + |A|, 40, scale) of Decrypt with both true keys (k = 2 parties, |A| active holders: 3 floods at
|A| = t = 2).  mkbfv (T = 65537): flood_bits = NoiseBits + 20, the decoded values exactly those of Decrypt; the test first asserts that the flood
fits the share call (62 bits) and MaxFloodBits(k - 1 + |A|) of the ring -- tests/test_threshold_model.py checks on the CPU that the smallest ring,
small_bfv(10, 3), is wide enough for that."""
import numpy as np
import pytest

import harness as H
import harness_bfv as HB

pytestmark = pytest.mark.gpu

LOGN = 10
N = 1 << LOGN
HOLDERS = {"bob": 3, "carol": 4294967295, "dave": 77}
ACTIVE = [["carol", "dave"], ["bob", "carol", "dave"]]


def _max_err(a, b):
    d = np.abs(np.asarray(a) - np.asarray(b))
    return float(max(d.real.max(), d.imag.max()))


def _alice_share_from_holders(mkrlwe, params, dec, ct, shares, active, flood_bits):
    """what the active holders publish for the absent alice, folded: each on its own additive key and its own sampler; the Shamir shares and the
    decryption shares travel as host arrays"""
    cb, pts, parts = mkrlwe.NewCombiner(params), {h: HOLDERS[h] for h in active}, []
    for h in active:
        mine = mkrlwe.SecretKeyShare(params, "alice", h, HOLDERS[h], 2).upload(shares[h].download())        # what alice sent to h
        add = cb.AdditiveKey(mine, pts)
        assert isinstance(add, mkrlwe.SecretKey) and add.ID == "alice"
        sampler = mkrlwe.DeviceSampler()
        sh = dec.ShareNew(ct, add, flood_bits, sampler)
        assert sampler.counter == 1 and sh.ID == "alice"
        parts.append(mkrlwe.DecryptionShare(params, "alice", ct.Level(), 1).upload(sh.download()))
    return dec.FoldShares(parts)


def test_ckks_two_of_three_holders_stand_in_for_an_absent_party():
    from mkhe_kklss_amd import mkckks, mkrlwe
    pset = H.small_ckks(LOGN, nq=4)
    scale, n, names = pset["scale"], N // 2, ["alice", "bob"]
    params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], scale)
    params.GenDefaultCRS(seed=4341)
    kgen = mkrlwe.NewKeyGenerator(params, mkrlwe.HostSampler(np.random.default_rng(2051), insecure_test_only=True))
    enc, dec, ev = mkckks.NewEncryptor(params, sampler=mkrlwe.DeviceSampler()), mkckks.NewDecryptor(params), mkckks.NewEvaluator(params)
    rng = np.random.default_rng(61)
    sks, skSet, rlk, ct, total = {}, mkrlwe.NewSecretKeySet(), mkrlwe.RelinearizationKeySet(params), None, 0
    for p in names:
        sks[p], pk = kgen.GenKeyPair(p)
        skSet.AddSecretKey(sks[p])
        rlk.AddRelinearizationKey(kgen.GenRelinearizationKey(sks[p], kgen.GenSecretKey(p)))
        z = rng.uniform(0.5, 1.0, n) * np.exp(2j * np.pi * rng.uniform(0, 1, n)) / 2
        c = enc.EncryptMsgNew(mkckks.Message(z), pk)
        ct, total = (c, z) if ct is None else (ev.AddNew(ct, c), total + z)
    ct = ev.MulRelinNew(ct, ct, rlk)
    assert ct.ids == names and ct.Level() == 2
    want = dec.Decrypt(ct, skSet).Value                             # with both true keys
    assert _max_err(want, total ** 2) < 1e-6

    shares = mkckks.NewThresholdizer(params).GenShares(sks["alice"], 2, HOLDERS, mkrlwe.DeviceSampler())
    assert sorted(shares) == sorted(HOLDERS) and all(s.Threshold == 2 and s.ID == "alice" for s in shares.values())
    del sks["alice"]                                                # alice is absent from here on
    bits = 40
    for active in ACTIVE:
        folded = _alice_share_from_holders(mkrlwe, params, dec, ct, shares, active, bits)
        mine = dec.ShareNew(ct, sks["bob"], bits, mkrlwe.DeviceSampler())
        got = dec.MergeSharesMsg(ct, [mine, folded]).Value
        floods = len(names) - 1 + len(active)
        bound, err = dec.FloodSlotBound(floods, bits, ct.Scale), _max_err(got, want)
        print("%d active holders: the merge is within %.3g of Decrypt (FloodSlotBound(%d, %d, scale) = %.3g)" % (len(active), err, floods, bits, bound))
        assert floods == (3 if len(active) == 2 else 4) and 0 < err <= bound and bound < 0.2
    params.close()


def test_bfv_two_of_three_holders_stand_in_for_an_absent_party_exactly():
    from mkhe_kklss_amd import mkbfv, mkrlwe
    pset = HB.small_bfv(LOGN, 3)
    T = pset["T"]
    centre = lambda v: np.where(np.mod(v, T) > T // 2, np.mod(v, T) - T, np.mod(v, T))
    params = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], T)
    params.GenDefaultCRS(seed=4342)
    kgen = mkbfv.NewKeyGenerator(params, mkrlwe.HostSampler(np.random.default_rng(2052), insecure_test_only=True))
    enc, dec, ev = mkbfv.NewEncryptor(params, sampler=mkrlwe.DeviceSampler(), encoder="device"), mkbfv.NewDecryptor(params, encoder="device"), mkbfv.NewEvaluator(params)
    rng = np.random.default_rng(67)
    names = ["alice", "bob"]
    sks, skSet, rlk, ct, msg = {}, mkrlwe.NewSecretKeySet(), mkbfv.RelinearizationKeySet(params), None, 0
    for p in names:
        sks[p], pk = kgen.GenKeyPair(p)
        skSet.AddSecretKey(sks[p])
        rlk.AddRelinearizationKey(kgen.GenRelinearizationKey(sks[p], kgen.GenSecretKey(p)))
        m = rng.integers(-(T // 2), T // 2 + 1, N).astype(np.int64)
        c = enc.EncryptMsgNew(mkbfv.Message(m), pk)
        ct, msg = (c, m) if ct is None else (ev.AddNew(ct, c), centre(msg + m))
    ct, msg = ev.MulRelinNew(ct, ct, rlk), centre(msg * msg)
    want = dec.Decrypt(ct, skSet).Value                             # with both true keys
    assert ct.ids == names and (want == msg).all()
    flood_bits = dec.NoiseBits(ct, skSet) + 20                      # measured with every key in hand, before alice leaves

    shares = mkbfv.NewThresholdizer(params).GenShares(sks["alice"], 2, HOLDERS, mkrlwe.DeviceSampler())
    del sks["alice"]
    for active in ACTIVE:
        floods = len(names) - 1 + len(active)
        print("%d active holders: flood_bits %d of the 62 a share takes, MaxFloodBits(%d) = %d" % (len(active), flood_bits, floods, dec.MaxFloodBits(floods)))
        assert flood_bits <= 62 and flood_bits <= dec.MaxFloodBits(floods)         # the condition: the message stays exact
        folded = _alice_share_from_holders(mkrlwe, params, dec, ct, shares, active, flood_bits)
        mine = dec.ShareNew(ct, sks["bob"], flood_bits, mkrlwe.DeviceSampler())
        got = dec.MergeSharesMsg(ct, [folded, mine]).Value
        assert (got == want).all()
        noisy = mkrlwe.Decryptor.MergeShares(dec, ct, [folded, mine]).download()[0]
        assert (noisy != dec.DecryptPtxt(ct, skSet)).mean() > 0.99                 # the floods are in it: the phase itself moved
    params.close()
