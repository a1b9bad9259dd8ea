"""The collective key switch to a recipient's public key end to end (-m gpu), N = 2^10.

mkckks: three parties encrypt, the sum is squared (MulRelinNew), and the result is switched to carol, who holds no part of it: every party
publishes a share under its own DeviceSampler and carol's PUBLIC key, the shares travel as host arrays and are merged in another order.  carol
decrypts alone, every slot within SwitchSlotBound of Decrypt with all three keys, and multiplies the result with a fresh ciphertext of her own
under her own relinearisation key.

mkbfv: two parties, a squared sum, the flood 20 bits above the measured noise (as tests/test_gpu_bfv_refresh_e2e.py chooses it).  carol's Decrypt
is the message exactly and the measured extra noise is at most NoiseBound.

Both tests first measure the input (with every key in hand) and assert that NoiseBound plus what they measured stays below the decryption margin
-- Q_l / 2 for the phase of a CKKS ciphertext, Q / (2 T) for the noise of a BFV one -- before they rely on the result."""
import types

import numpy as np
import pytest

import harness as H
import harness_bfv as HB
from scenario import Scenario

pytestmark = pytest.mark.gpu

LOGN = 10
N = 1 << LOGN


def _max_err(a, b):
    d = np.abs(np.asarray(a) - np.asarray(b))
    return float(max(d.real.max(), d.imag.max()))


def _centred(a, b, moduli):
    """the centred integers of a - b mod Q, for residue arrays [limbs][N]"""
    q = np.array(moduli, dtype=object)[:, None]
    return H.crt_center(((np.asarray(a).astype(object) - np.asarray(b).astype(object)) % q).astype(np.uint64), list(moduli))


def test_three_parties_hand_a_ckks_result_to_a_client_who_goes_on_computing():
    from mkhe_kklss_amd import mkckks, mkrlwe
    pset = H.small_ckks(LOGN, nq=4)
    scale, n, names = pset["scale"], N // 2, ["user0", "user1", "user2"]
    params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], scale)
    params.GenDefaultCRS(seed=4323)
    kgen = mkrlwe.NewKeyGenerator(params, mkrlwe.HostSampler(np.random.default_rng(2030), insecure_test_only=True))
    enc, dec, ev = mkckks.NewEncryptor(params, sampler=mkrlwe.DeviceSampler()), mkckks.NewDecryptor(params), mkckks.NewEvaluator(params)
    sw, host_encoder = mkckks.NewPublicKeySwitcher(params), mkckks.Encoder(params)
    rng = np.random.default_rng(47)
    sks, pks, samplers, skSet, rlk, ct, total = {}, {}, {}, mkrlwe.NewSecretKeySet(), mkrlwe.RelinearizationKeySet(params), None, 0
    for p in names:
        sks[p], pks[p] = kgen.GenKeyPair(p)
        skSet.AddSecretKey(sks[p])
        rlk.AddRelinearizationKey(kgen.GenRelinearizationKey(sks[p], kgen.GenSecretKey(p)))
        samplers[p] = mkrlwe.DeviceSampler()
        z = rng.uniform(0.5, 1.0, n) * np.exp(2j * np.pi * rng.uniform(0, 1, n)) / 3
        c = enc.EncryptMsgNew(mkckks.Message(z), pks[p])
        ct, total = (c, z) if ct is None else (ev.AddNew(ct, c), total + z)
    ct = ev.MulRelinNew(ct, ct, rlk)
    assert ct.Level() == 2 and ct.ids == names
    sk_c, pk_c = kgen.GenKeyPair("carol")                       # the recipient: no part of the ciphertext, not online during the switch
    carol, rlk_c = mkrlwe.NewSecretKeySet(), mkrlwe.RelinearizationKeySet(params)
    carol.AddSecretKey(sk_c)
    rlk_c.AddRelinearizationKey(kgen.GenRelinearizationKey(sk_c, kgen.GenSecretKey("carol")))

    before = dec.Decrypt(ct, skSet).Value                      # needs all three keys
    assert _max_err(before, total ** 2) < 1e-6
    Qs = pset["Q"][: ct.Level() + 1]
    phase = dec.DecryptPtxt(ct, skSet).Value
    noise, Q = _centred(phase, host_encoder.Encode(total ** 2, ct.Level(), ct.Scale), Qs)
    e_ct = max(abs(v) for v in noise)
    flood_bits = int(e_ct).bit_length() + 20
    size = max(abs(v) for v in H.crt_center(phase, list(Qs))[0])
    bound = sw.NoiseBound(3, flood_bits, N)
    print("noise of the input: %d bits; flood_bits %d of at most %d; phase %d bits, NoiseBound %d bits, Q_l / 2 %d bits"
          % (int(e_ct).bit_length(), flood_bits, sw.MaxFloodBits(ct.Level()), int(size).bit_length(), bound.bit_length(), (Q // 2).bit_length()))
    assert flood_bits <= sw.MaxFloodBits(ct.Level()) and size + bound < Q // 2          # the condition: the switched phase does not wrap

    wire = []
    for p in names:
        sh = sw.ShareNew(ct, sks[p], pk_c, flood_bits, samplers[p])
        assert samplers[p].counter == 1 and sh.ID == p and sh.count == 1 and sh.Level() == 2
        wire.append((p, sh.download()))
    assert wire[0][1].shape == (1, 2, 3, N)
    shares = [mkrlwe.PublicKeySwitchShare(params, p, 2, 1).upload(host) for p, host in (wire[2], wire[0], wire[1])]
    res = sw.MergeNew(ct, shares, "carol")
    assert isinstance(res, mkckks.Ciphertext) and res.ids == ["carol"] and res.Level() == 2 and res.Scale == ct.Scale

    after = dec.Decrypt(res, carol).Value                      # carol alone
    slot_bound, err = sw.SwitchSlotBound(3, flood_bits, ct.Scale), _max_err(after, before)
    extra = max(abs(v) for v in _centred(dec.DecryptPtxt(res, carol).Value, phase, Qs)[0])
    print("the switch moved a slot by at most %.3g (bound %.3g); extra noise %d bits (NoiseBound %d bits)" % (err, slot_bound, int(extra).bit_length(), bound.bit_length()))
    assert 0 < extra <= bound and err <= slot_bound

    # carol goes on computing: the product with a ciphertext of her own, under her own relinearisation key
    zc = rng.uniform(0.5, 1.0, n) * np.exp(2j * np.pi * rng.uniform(0, 1, n))
    mine = mkckks.NewEncryptor(params, sampler=mkrlwe.DeviceSampler()).EncryptMsgNew(mkckks.Message(zc), pk_c)
    prod = ev.MulRelinNew(res, mine, rlk_c)
    tol = Scenario.precision_bound(types.SimpleNamespace(scale=scale, logN=LOGN), 12)
    err2 = np.log2(max(_max_err(dec.Decrypt(prod, carol).Value, after * zc), 1e-300))
    print("MulRelinNew on the switched ciphertext: log2 error %.2f (bound %.2f), level %d" % (err2, tol, prod.Level()))
    assert prod.ids == ["carol"] and prod.Level() == 1 and err2 <= tol
    params.close()


def test_two_parties_hand_a_bfv_result_to_a_client_exactly():
    from mkhe_kklss_amd import mkbfv, mkrlwe
    pset = HB.small_bfv(LOGN, 3)
    T = pset["T"]
    centre = lambda v: np.where(np.mod(v, T) > T // 2, np.mod(v, T) - T, np.mod(v, T))
    params = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], T)
    params.GenDefaultCRS(seed=4324)
    kgen = mkbfv.NewKeyGenerator(params, mkrlwe.HostSampler(np.random.default_rng(2031), insecure_test_only=True))
    enc, dec, ev = mkbfv.NewEncryptor(params, sampler=mkrlwe.DeviceSampler(), encoder="device"), mkbfv.NewDecryptor(params, encoder="device"), mkbfv.NewEvaluator(params)
    sw, host_encoder = mkbfv.NewPublicKeySwitcher(params), mkbfv.Encoder(params)
    rng = np.random.default_rng(53)
    names = ["user0", "user1"]
    sks, pks, samplers, skSet, rlk, ct, msg = {}, {}, {}, mkrlwe.NewSecretKeySet(), mkbfv.RelinearizationKeySet(params), None, 0
    for p in names:
        sks[p], pks[p] = kgen.GenKeyPair(p)
        skSet.AddSecretKey(sks[p])
        rlk.AddRelinearizationKey(kgen.GenRelinearizationKey(sks[p], kgen.GenSecretKey(p)))
        samplers[p] = mkrlwe.DeviceSampler()
        m = rng.integers(-(T // 2), T // 2 + 1, N).astype(np.int64)
        c = enc.EncryptMsgNew(mkbfv.Message(m), pks[p])
        ct, msg = (c, m) if ct is None else (ev.AddNew(ct, c), centre(msg + m))
    ct, msg = ev.MulRelinNew(ct, ct, rlk), centre(msg * msg)
    assert ct.ids == names and (dec.Decrypt(ct, skSet).Value == msg).all()
    sk_c, pk_c = kgen.GenKeyPair("carol")
    carol = mkrlwe.NewSecretKeySet()
    carol.AddSecretKey(sk_c)

    phase = dec.DecryptPtxt(ct, skSet)                          # with both keys in hand
    noise, Q = _centred(phase, host_encoder.Encode(msg), pset["Q"])
    e_ct = max(abs(v) for v in noise)
    flood_bits = int(e_ct).bit_length() + 20
    bound = sw.NoiseBound(2, flood_bits, N)
    print("noise of the input: %d bits of the %d of Q / (2T); flood_bits %d, MaxFloodBits(2) %d; NoiseBound %d bits"
          % (int(e_ct).bit_length(), (Q // (2 * T)).bit_length(), flood_bits, sw.MaxFloodBits(2), bound.bit_length()))
    assert flood_bits <= sw.MaxFloodBits(2) and e_ct + bound < Q // (2 * T)             # the condition: the message stays exact

    wire = []
    for p in names:
        sh = sw.ShareNew(ct, sks[p], pk_c, flood_bits, samplers[p])
        assert samplers[p].counter == 1 and sh.ID == p and sh.count == 1 and sh.Level() == params.MaxLevel()
        wire.append((p, sh.download()))
    shares = [mkrlwe.PublicKeySwitchShare(params, p, params.MaxLevel(), 1).upload(host) for p, host in reversed(wire)]
    res = sw.MergeNew(ct, shares, "carol")
    assert isinstance(res, mkbfv.Ciphertext) and res.ids == ["carol"] and res.Level() == params.MaxLevel()
    assert (dec.Decrypt(res, carol).Value == msg).all()        # carol alone, exactly
    extra = max(abs(v) for v in _centred(dec.DecryptPtxt(res, carol), phase, pset["Q"])[0])
    print("extra noise of the switch: %d bits (NoiseBound %d bits)" % (int(extra).bit_length(), bound.bit_length()))
    assert 0 < extra <= bound and int(extra).bit_length() >= flood_bits - 8
    params.close()
