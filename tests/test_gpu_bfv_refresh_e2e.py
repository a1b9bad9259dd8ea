"""The collective refresh of MK-BFV end to end on mkbfv (-m gpu): two parties, N = 2^10, small_bfv(10, 3), T = 65537, the device encoder and
DeviceSampler.  A ciphertext over both parties is squared until Decrypt goes wrong, at depth D.  At depth D - 2 its noise is measured with
both keys in hand; both parties publish a refresh share with a flood 20 bits above that noise, each on its own sampler, the shares travel as
host arrays, anyone merges.  The result decrypts to the same message with the noise of fresh encryptions (RefreshNoiseBound) and takes the
two squarings the un-refreshed chain does not survive.  With flood_bits = 0 the merge is, exactly, up of the decryption of the input shifted by
the masks the re-encryptions carry, plus the re-encryptions."""
import numpy as np
import pytest

import harness as H
import harness_bfv as HB

pytestmark = pytest.mark.gpu

PSET = HB.small_bfv(10, 3)
N, T = 1 << PSET["logN"], PSET["T"]
NAMES = ["user0", "user1"]


def centre(v):
    r = np.mod(np.asarray(v, dtype=np.int64), T)
    return np.where(r > T // 2, r - T, r)


def test_two_parties_refresh_away_the_noise_and_go_on_squaring():
    from mkhe_kklss_amd import mkbfv, mkrlwe
    params = mkbfv.Parameters(PSET["logN"], PSET["Q"], PSET["QMul"], PSET["P"], T)
    params.GenDefaultCRS(seed=4322)
    kgen = mkbfv.NewKeyGenerator(params, mkrlwe.HostSampler(np.random.default_rng(2027), insecure_test_only=True))
    enc, dec, ev = mkbfv.NewEncryptor(params, sampler=mkrlwe.DeviceSampler(), encoder="device"), mkbfv.NewDecryptor(params, encoder="device"), mkbfv.NewEvaluator(params)
    ref, host_encoder = mkbfv.NewRefresher(params), mkbfv.Encoder(params)
    rng = np.random.default_rng(43)
    sks, pks, samplers, skSet, rlk, ct, msg = {}, {}, {}, mkrlwe.NewSecretKeySet(), mkbfv.RelinearizationKeySet(params), None, 0
    for p in NAMES:
        sks[p], pks[p] = kgen.GenKeyPair(p)
        skSet.AddSecretKey(sks[p])
        rlk.AddRelinearizationKey(kgen.GenRelinearizationKey(sks[p], kgen.GenSecretKey(p)))
        samplers[p] = mkrlwe.DeviceSampler()
        m = rng.integers(-(T // 2), T // 2 + 1, N).astype(np.int64)
        c = enc.EncryptMsgNew(mkbfv.Message(m), pks[p])
        ct, msg = (c, m) if ct is None else (ev.AddNew(ct, c), centre(msg + m))
    assert ct.ids == NAMES

    def square(c):
        return ev.MulRelinNew(c, c, rlk)

    def noise(c, slots):
        """max |phase - up(coefficients of the message)| over the coefficients, with both keys in hand"""
        d = (dec.DecryptPtxt(c, skSet).astype(object) - host_encoder.Encode(slots).astype(object)) % np.array(PSET["Q"], dtype=object)[:, None]
        return max(abs(v) for v in H.crt_center(d.astype(np.uint64), PSET["Q"])[0])

    # the un-refreshed chain: D = the first depth at which Decrypt differs from the powers mod T
    chain, powers, D = [ct], [msg], None
    for depth in range(1, 9):
        chain.append(square(chain[-1]))
        powers.append(centre(powers[-1] * powers[-1]))
        if not (dec.Decrypt(chain[-1], skSet).Value == powers[-1]).all():
            D = depth
            break
    assert D is not None and 2 <= D <= 8, "squaring must break the message at a depth 2 .. 8, it did at %r" % D
    assert all((dec.Decrypt(c, skSet).Value == p).all() for c, p in zip(chain[:D], powers[:D]))

    worn, want = chain[D - 2], powers[D - 2]
    e_ct = noise(worn, want)
    flood_bits = int(e_ct).bit_length() + 20
    q = 1
    for p in PSET["Q"]:
        q *= p
    print("D = %d; noise at depth %d: %d bits of the %d of Q / (2T); flood_bits %d, MaxFloodBits(2) %d"
          % (D, D - 2, int(e_ct).bit_length(), (q // (2 * T)).bit_length(), flood_bits, ref.MaxFloodBits(2)))
    assert flood_bits <= ref.MaxFloodBits(2)

    wire = []
    for p in NAMES:
        sh = ref.ShareNew(worn, sks[p], pks[p], flood_bits, samplers[p])
        assert samplers[p].counter == 2 and sh.ID == p and sh.count == 1 and sh.Level() == params.MaxLevel() == sh.LevelOut()
        wire.append((p, sh.download()))
    shares = [mkrlwe.RefreshShare(params, p, params.MaxLevel(), params.MaxLevel(), 1).upload(host) for p, host in reversed(wire)]
    fresh = ref.MergeNew(worn, shares)
    assert isinstance(fresh, mkbfv.Ciphertext) and fresh.ids == worn.ids and fresh.Level() == params.MaxLevel()
    assert (dec.Decrypt(fresh, skSet).Value == want).all()                      # the same message
    e_fresh, bound = noise(fresh, want), ref.RefreshNoiseBound(2)
    print("noise after the refresh: %d (bound %.1f)" % (e_fresh, bound))
    assert e_fresh <= bound

    # two more squarings reach depth D, where the un-refreshed chain has lost the message
    again = square(square(fresh))
    assert (dec.Decrypt(again, skSet).Value == powers[D]).all()
    assert not (dec.Decrypt(chain[D], skSet).Value == powers[D]).all()

    # flood_bits = 0: R = phase + sum up(A_i), and the re-encryptions decrypt to up(-A_i) plus their small noise, which says what every A_i is
    plain = [ref.ShareNew(worn, sks[p], pks[p], 0, samplers[p]) for p in NAMES]
    merged = ref.MergeNew(worn, plain)
    qcol = np.array(PSET["Q"], dtype=object)[:, None]
    w = mkbfv.ScaleDown(dec.DecryptPtxt(worn, skSet), params).astype(object)    # the coefficients Decrypt decodes
    rest = dec.DecryptPtxt(merged, skSet).astype(object)
    for sh in plain:
        re = dec.DecryptPtxt(sh.Reenc[0], skSet)
        w = w - mkbfv.ScaleDown(re, params).astype(object)                       # down of that phase is -A_i mod T
        rest = (rest - re.astype(object)) % qcol
    assert (rest.astype(np.uint64) == mkbfv.ScaleUp(w, params)).all()           # the phase of the merge, less the re-encryptions', is up(Decrypt + sum A_i)
    assert (dec.Decrypt(merged, skSet).Value == want).all()
    params.close()
