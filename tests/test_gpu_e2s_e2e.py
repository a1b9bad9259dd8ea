"""Encryption to shares and back end to end on the Python mirrors (-m gpu), three parties, N = 2^10; every party has TWO DeviceSamplers with the
same test key and counter, one for the Refresher and one for the new path, so that the two can be compared bit for bit.

mkckks (small_ckks(10, 4), a ciphertext at level 1): E2S, the public share folded into one party's share, S2E = Refresher.MergeNew of
Refresher.ShareNew, bit for bit, and decrypts to the message within RefreshSlotBound.

mkbfv (small_bfv(10, 3), a fresh product ciphertext, flood_bits = MaxFloodBits(3)): (public + sum of the secret shares) mod T as slots is
Decrypt(ct).Value exactly; ShareMap / MergeMap with the identity map are Refresher's shares and merged ciphertext, bit for bit; with a random
permutation and multipliers, with SlotMap.Rotation(5, swap_rows=True) and with a replicating index Decrypt(MergeMapNew(..)).Value is
slot_map.apply(values) exactly and the noise of the result is at most RefreshNoiseBound(3)."""
import numpy as np
import pytest

import harness as H
import harness_bfv as HB

pytestmark = pytest.mark.gpu

LOGN = 10
NAMES = ["user0", "user1", "user2"]


def sampler_key(p):
    return bytes((17 * NAMES.index(p) + i) % 256 for i in range(32))


def twins(p):
    from mkhe_kklss_amd import mkrlwe
    return tuple(mkrlwe.DeviceSampler(key=sampler_key(p), insecure_test_only=True) for _ in range(2))


def _max_err(a, b):
    d = np.abs(np.asarray(a) - np.asarray(b))
    return float(max(d.real.max(), d.imag.max()))


def test_ckks_e2s_then_s2e_is_the_refresh_bit_for_bit():
    from mkhe_kklss_amd import mkckks, mkrlwe
    from mkhe_kklss_amd._abi import MkheError
    pset = H.small_ckks(LOGN, nq=4)
    scale, n = pset["scale"], 1 << (LOGN - 1)
    params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], scale)
    params.GenDefaultCRS(seed=4321)
    kgen = mkrlwe.NewKeyGenerator(params, mkrlwe.HostSampler(np.random.default_rng(2026), insecure_test_only=True))
    enc, dec, ev = mkckks.NewEncryptor(params, sampler=mkrlwe.DeviceSampler()), mkckks.NewDecryptor(params), mkckks.NewEvaluator(params)
    ref, conv = mkckks.NewRefresher(params), mkckks.NewShareConverter(params)
    rng = np.random.default_rng(41)
    z = rng.uniform(0.5, 1.0, n) * np.exp(2j * np.pi * rng.uniform(0, 1, n))
    sks, pks, skSet, ct, sa, sb = {}, {}, mkrlwe.NewSecretKeySet(), None, {}, {}
    for p in NAMES:
        sks[p], pks[p] = kgen.GenKeyPair(p)
        skSet.AddSecretKey(sks[p])
        sa[p], sb[p] = twins(p)
        c = enc.EncryptMsgNew(mkckks.Message(z / 3), pks[p])
        ct = c if ct is None else ev.AddNew(ct, c)
    ct = ev.DropLevelNew(ct, 2)
    assert ct.Level() == 1 and ct.ids == NAMES
    before = dec.Decrypt(ct, skSet).Value
    assert _max_err(before, z) < 1e-6
    bits = ref.MaxMaskBits(3, 1, ct.Scale)
    assert bits == conv.MaxMaskBits(3, 1, ct.Scale)

    # the Refresher, on the first sampler of every party
    shares = [ref.ShareNew(ct, sks[p], pks[p], bits, sa[p]) for p in NAMES]
    want = ref.MergeNew(ct, shares)

    # E2S on the second: the published shares are the Refresher's, the secret shares stay with their parties
    pub, sec = {}, {}
    for p, sh in zip(NAMES, shares):
        pub[p], sec[p] = conv.E2SShareBatch([ct], sks[p], bits, sb[p])
        assert sb[p].counter == 1 and pub[p].ID == p and sec[p].ID == p and sec[p].Level() == 3 and sec[p].count == 1
        assert (pub[p].download() == sh.Share.download()).all()
    public = conv.E2SMergeBatch([ct], [pub[p] for p in reversed(NAMES)])
    assert public.ID is None and public.Level() == 3
    # the identity under the moduli of the input level: public + sum of the secrets is the plaintext of Decrypt, bit for bit
    q = np.array(pset["Q"][:2], dtype=np.uint64)[:, None]
    total = public.download()[0][:2]
    for p in NAMES:
        total = (total + sec[p].download()[0][:2]) % q
    assert (total == mkrlwe.Decryptor.Decrypt(dec, ct, skSet).download()[0]).all()

    # S2E: user1 holds the public share and folds it into its own before it encrypts
    with pytest.raises(MkheError, match="FoldPublic"):
        conv.S2EMergeNew([], public=public)
    sec["user1"] = conv.FoldPublic(sec["user1"], public)
    back = {p: conv.S2EShareBatch(sec[p], pks[p], sb[p])[0] for p in NAMES}
    assert all(sb[p].counter == 2 == sa[p].counter for p in NAMES)
    for p, sh in zip(NAMES, shares):
        if p != "user1":
            assert (back[p].download() == sh.Reenc[0].download()).all()        # the re-encryption of the refresh itself
    got = conv.S2EMergeNew([back[p] for p in NAMES])
    assert isinstance(got, mkckks.Ciphertext) and got.ids == want.ids and got.Level() == want.Level() == 3 and got.Scale == want.Scale == ct.Scale
    assert (got.download() == want.download()).all()
    err, bound = _max_err(dec.Decrypt(got, skSet).Value, before), ref.RefreshSlotBound(3, ct.Scale)
    print("mask_bits %d; E2S + S2E moved a slot by at most %.3g (bound %.3g)" % (bits, err, bound))
    assert err <= bound
    host = sec["user0"].download()
    sec["user0"].wipe()
    assert sec["user0"].Value is None and host.any()
    params.close()


def test_bfv_shares_are_exact_and_the_refresh_applies_a_slot_map():
    from mkhe_kklss_amd import mkbfv, mkrlwe
    pset = HB.small_bfv(LOGN, 3)
    N, T = 1 << LOGN, pset["T"]
    params = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], T)
    params.GenDefaultCRS(seed=4322)
    kgen = mkbfv.NewKeyGenerator(params, mkrlwe.HostSampler(np.random.default_rng(2027), insecure_test_only=True))
    enc, dec, ev = mkbfv.NewEncryptor(params, sampler=mkrlwe.DeviceSampler(), encoder="device"), mkbfv.NewDecryptor(params, encoder="device"), mkbfv.NewEvaluator(params)
    ref, conv = mkbfv.NewRefresher(params), mkbfv.NewShareConverter(params)
    rng = np.random.default_rng(44)

    def centre(v):
        r = np.mod(np.asarray(v, dtype=np.int64), T)
        return np.where(r > T // 2, r - T, r)

    sks, pks, skSet, rlk, ct, msg = {}, {}, mkrlwe.NewSecretKeySet(), mkbfv.RelinearizationKeySet(params), None, 0
    for p in NAMES:
        sks[p], pks[p] = kgen.GenKeyPair(p)
        skSet.AddSecretKey(sks[p])
        rlk.AddRelinearizationKey(kgen.GenRelinearizationKey(sks[p], kgen.GenSecretKey(p)))
        m = rng.integers(-(T // 2), T // 2 + 1, N).astype(np.int64)
        c = enc.EncryptMsgNew(mkbfv.Message(m), pks[p])
        ct, msg = (c, m) if ct is None else (ev.AddNew(ct, c), centre(msg + m))
    ct, values = ev.MulRelinNew(ct, ct, rlk), centre(msg * msg)                 # a fresh product ciphertext
    assert ct.ids == NAMES and (dec.Decrypt(ct, skSet).Value == values).all()
    flood = ref.MaxFloodBits(3)
    assert flood == conv.MaxFloodBits(3) and dec.NoiseBits(ct, skSet, mkbfv.Message(values)) < flood

    # ---- E2S: exact over Z_T
    sa, sb = {}, {}
    for p in NAMES:
        sa[p], sb[p] = twins(p)
    parts = [conv.E2SShareBatch([ct], sks[p], flood, sb[p]) for p in NAMES]
    public = conv.E2SMergeBatch([ct], [pub for pub, _ in parts])
    total = public.download()
    for _, s in parts:
        assert isinstance(s, mkbfv.SecretShare) and (s.download() < T).all()
        total = (total + s.download()) % np.uint64(T)
    assert (mkbfv.SecretShare(params, None, 1).upload(total).Slots()[0] == values).all()
    slot_sum = centre(public.Slots()[0] + sum(s.Slots()[0] for _, s in parts))   # and slot by slot
    assert (slot_sum == values).all()
    assert (mkbfv.SecretShare.FromSlots(params, values).download() == total).all()
    # S2E: fresh encryptions of the shares, the public share added as a plaintext
    back = conv.S2EMergeNew([conv.S2EShareBatch(s, pks[s.ID], sb[s.ID])[0] for _, s in parts], public=public)
    assert back.ids == NAMES and (dec.Decrypt(back, skSet).Value == values).all()
    assert dec.NoiseNorm(back, skSet, mkbfv.Message(values)) <= ref.RefreshNoiseBound(3)

    # ---- the identity map: the Refresher's shares and merged ciphertext, bit for bit
    sa, sb = {}, {}
    for p in NAMES:
        sa[p], sb[p] = twins(p)
    ident = mkbfv.SlotMap(params, np.arange(N))
    plain = [ref.ShareNew(ct, sks[p], pks[p], flood, sa[p]) for p in NAMES]
    mapped = [ref.ShareMapNew(ct, sks[p], pks[p], flood, sb[p], ident) for p in NAMES]
    for p, a, b in zip(NAMES, plain, mapped):
        assert sa[p].counter == sb[p].counter == 2
        (sh_a, re_a), (sh_b, re_b) = a.download(), b.download()
        assert (sh_a == sh_b).all() and (re_a[0] == re_b[0]).all(), p
    want, got = ref.MergeNew(ct, plain), ref.MergeMapNew(ct, mapped, ident)
    assert isinstance(got, mkbfv.Ciphertext) and got.ids == want.ids and (got.download() == want.download()).all()

    # ---- maps that move slots
    half = N // 2
    replicate = np.concatenate([np.full(half, 3), np.full(half, half + 7)])     # every slot of a row takes one slot of that row
    cases = {
        "permutation with multipliers": mkbfv.SlotMap(params, rng.permutation(N), rng.integers(-(T // 2), T // 2 + 1, N)),
        "rotation by 5, rows swapped": mkbfv.SlotMap.Rotation(params, 5, swap_rows=True),
        "replication": mkbfv.SlotMap(params, replicate),
    }
    bound = ref.RefreshNoiseBound(3)
    for name, sm in cases.items():
        shares = [ref.ShareMapNew(ct, sks[p], pks[p], flood, sb[p], sm) for p in NAMES]
        res = ref.MergeMapNew(ct, list(reversed(shares)), sm)
        expect = sm.apply(values)
        assert (dec.Decrypt(res, skSet).Value == expect).all(), name
        noise = dec.NoiseNorm(res, skSet, mkbfv.Message(expect))
        print("%s: noise %d (bound %.1f)" % (name, noise, bound))
        assert noise <= bound, name
    rot = cases["rotation by 5, rows swapped"].apply(values)
    assert (rot[:half] == np.roll(values[half:], -5)).all() and (rot[half:] == np.roll(values[:half], -5)).all()
    assert not (cases["replication"].apply(values)[:half] != values[3]).any()
    params.close()
