"""The collective refresh end to end on mkckks (-m gpu): two parties, N = 2^10, the chain of tests/test_gpu_lintrans_e2e.py (4 limbs, scale
2^54).  A ciphertext is squared twice, down to level 1; both parties publish a refresh share under their own DeviceSampler, the shares travel
as host arrays, anyone merges.  The result is at level 3 with the input's Scale, decrypts to the input's slots within RefreshSlotBound, and
can be multiplied again within the tolerance tests/test_gpu_encdec_e2e.py applies to one MulRelinNew (Scenario.precision_bound with 12 extra
bits) -- while the un-refreshed ciphertext, taken down to level 0, is refused by the multiplication with "cannot Rescale".

(At level 0 it is the product WITH its Rescale that is refused: Evaluator.MulRelinOnceNew, the MulRelinNew of a fixed-depth circuit.
Evaluator.MulRelinNew itself counts zero Rescales at level 0 on this chain (scale^2 / q_0 = 2^48 is below scale / 2), so it never reaches the
Rescale that is refused: its product would stay at level 0 with scale 2^108 > q_0, a ciphertext that holds no message.  On the refreshed
ciphertext the two are the same call.)"""
import types

import numpy as np
import pytest

import harness as H
from scenario import Scenario

pytestmark = pytest.mark.gpu

LOGN = 10


def _max_err(a, b):
    d = np.abs(np.asarray(a) - np.asarray(b))
    return float(max(d.real.max(), d.imag.max()))


def test_two_parties_refresh_and_go_on_multiplying():
    from mkhe_kklss_amd import mkckks, mkrlwe
    from mkhe_kklss_amd._abi import MkheError
    pset = H.small_ckks(LOGN, nq=4)
    scale, n, names = pset["scale"], 1 << (LOGN - 1), ["user0", "user1"]
    params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], scale)
    params.GenDefaultCRS(seed=4321)
    kgen = mkrlwe.NewKeyGenerator(params, mkrlwe.HostSampler(np.random.default_rng(2026), insecure_test_only=True))
    enc, dec, ev = mkckks.NewEncryptor(params, sampler=mkrlwe.DeviceSampler()), mkckks.NewDecryptor(params), mkckks.NewEvaluator(params)
    ref = mkckks.NewRefresher(params)
    rng = np.random.default_rng(41)
    z = rng.uniform(0.5, 1.0, n) * np.exp(2j * np.pi * rng.uniform(0, 1, n))                # slots with modulus in [0.5, 1]
    sks, pks, samplers, skSet, rlk, ct = {}, {}, {}, mkrlwe.NewSecretKeySet(), mkrlwe.RelinearizationKeySet(params), None
    for p in names:
        sks[p], pks[p] = kgen.GenKeyPair(p)
        skSet.AddSecretKey(sks[p])
        rlk.AddRelinearizationKey(kgen.GenRelinearizationKey(sks[p], kgen.GenSecretKey(p)))
        samplers[p] = mkrlwe.DeviceSampler()
        c = enc.EncryptMsgNew(mkckks.Message(z / 2), pks[p])
        ct = c if ct is None else ev.AddNew(ct, c)
    assert ct.Level() == 3
    ct = ev.MulRelinNew(ct, ct, rlk)
    ct = ev.MulRelinNew(ct, ct, rlk)
    assert ct.Level() == 1 and ct.ids == names
    before = dec.Decrypt(ct, skSet).Value
    assert _max_err(before, z ** 4) < 1e-6 and np.abs(before).max() <= 1.0 + 1e-6          # (what MaxMaskBits is told: no slot above 1)

    bits = ref.MaxMaskBits(2, 1, ct.Scale)
    wire = []
    for p in names:
        sh = ref.ShareNew(ct, sks[p], pks[p], bits, samplers[p])
        assert samplers[p].counter == 2 and sh.ID == p and sh.Level() == 1 and sh.LevelOut() == 3 and sh.count == 1
        wire.append((p, sh.download()))
    shares = [mkrlwe.RefreshShare(params, p, 1, 3, 1).upload(host) for p, host in reversed(wire)]
    res = ref.MergeNew(ct, shares)
    assert isinstance(res, mkckks.Ciphertext) and res.Level() == 3 and res.Scale == ct.Scale and res.ids == ct.ids

    after = dec.Decrypt(res, skSet).Value
    slot_bound = ref.RefreshSlotBound(2, ct.Scale)
    err = _max_err(after, before)
    print("mask_bits %d; refresh moved a slot by at most %.3g (bound %.3g)" % (bits, err, slot_bound))
    assert err <= slot_bound

    sq = ev.MulRelinNew(res, res, rlk)
    tol = Scenario.precision_bound(types.SimpleNamespace(scale=scale, logN=LOGN), 12)
    err2 = np.log2(max(_max_err(dec.Decrypt(sq, skSet).Value, after ** 2), 1e-300))
    print("MulRelinNew on the refreshed ciphertext: log2 error %.2f (bound %.2f), level %d" % (err2, tol, sq.Level()))
    assert sq.Level() == 2 and err2 <= tol

    low = ev.DropLevelNew(ct, 1)
    assert low.Level() == 0
    with pytest.raises(MkheError, match="cannot Rescale"):
        ev.MulRelinOnceNew(low, low, rlk)
    params.close()
