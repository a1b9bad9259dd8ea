"""The model of the collective key switch to a recipient's public key (tests/pcks_model.py) and the parts of its Python mirror that make no
engine call (no GPU): the stream layout of a call, the flood_bits = 0 identity that anchors the parity of mkhe_pcks_share (a share is the plain
decryption share plus an encryption of zero under the recipient's key on the samples (u, 0, e1)), the whole protocol on the oracle's ring at
logN = 10 for 1 and 3 parties -- the merged ciphertext decrypts under the recipient's key ALONE to within NoiseBound of the phase of the input,
for a recipient outside the parties and for one of them -- and the arithmetic of NoiseBound, MaxFloodBits and SwitchSlotBound."""
import types

import numpy as np
import pytest

import bfv_refresh_model as B
import decrypt_share_model as D
import device_sampler_model as M
import harness as H
import harness_bfv as HB
import pcks_model as P
from mkhe_kklss_amd import mkbfv, mkckks, mkrlwe
from oracle import oracle as O

KEY = [0x9E3779B9, 0x7F4A7C15, 0xF39CC060, 0x5CEDC834, 0x1082276B, 0xF3A27251, 0xF86C6A11, 0xD0C18E95]
NONCE = 0xFEDCBA9876543210
PSET = H.small_ckks(10, 3)
CDT = mkrlwe.small_cdt(3.2)
USERS = ["user0", "user1", "user2"]


def word(key, nonce, stream, i):
    w = M.chacha20_block(key, i // 8, nonce & M.M32, nonce >> 32, stream)
    return w[2 * (i % 8)] | (w[2 * (i % 8) + 1] << 32)


@pytest.mark.parametrize("bits", [0, 1, 64, 65, 129])
@pytest.mark.parametrize("count", [1, 3])
def test_stream_layout(count, bits):
    """stream b is u_b, stream count + b is e1_b, stream 2 count + b W + w is word w of the flood of item b"""
    n, W = 16, P.words(bits)
    assert P.streams(count, bits) == 2 * count + count * W
    used = set()
    for b in range(count):
        u, e1, E = P.u_poly(KEY, NONCE, count, b, n), P.e1_poly(KEY, NONCE, count, b, n, CDT), P.flood_poly(KEY, NONCE, count, b, n, bits)
        for i in (0, 7, 8, 15):
            assert u[i] == M.ternary(word(KEY, NONCE, b, i))
            assert e1[i] == M.table(word(KEY, NONCE, count + b, i), CDT)
            assert E[i] == B.flood_value([word(KEY, NONCE, 2 * count + b * W + w, i) for w in range(W)], bits)
        used |= {P.u_stream(count, b), P.e1_stream(count, b)} | {P.flood_stream(count, b, bits, w) for w in range(W)}
        assert all(v in (-1, 0, 1) for v in u) and all(abs(v) <= len(CDT) // 2 for v in e1)
    assert used == set(range(P.streams(count, bits)))           # every stream of the call serves exactly one purpose
    assert P.u_poly(KEY, NONCE, count, 0, n) == M.sample_small(0, 1, KEY, NONCE, 0, n)[0]      # what launch_small_sample(kind 0, first_stream 0) draws
    assert P.flood_poly(None, 0, count, 0, n, 0) == [0] * n     # flood_bits = 0 reads no stream


@pytest.fixture(scope="module")
def world():
    """three parties and a recipient outside them with real keys; one ciphertext over 1 and over 3 parties: a fresh encryption under party 0 whose
    other party polynomials are uniform (the identities hold for any ciphertext)"""
    ks = O.KeySwitcher(PSET["logN"], PSET["Q"], PSET["P"], 2)
    kg = H.KeyGen(ks, seed=23)
    kg.add_crs(0)
    sks, pks = {}, {}
    for n in USERS + ["carol"]:
        sks[n], small = kg.gen_secret_key()
        assert set(np.unique(small).tolist()) <= {-1, 0, 1}     # the secret key is ternary: what NoiseBound assumes of s_R
        pks[n] = kg.gen_public_key(sks[n])
    level = len(PSET["Q"]) - 1
    c0, c1 = kg.encrypt(H.uniform_poly(kg.rng, ks.Q, ks.N), pks["user0"], level)
    cts = {}
    for k in (1, 3):
        cts[k] = {"0": c0, "user0": c1}
        for n in USERS[1:k]:
            cts[k][n] = H.uniform_poly(kg.rng, ks.Q, ks.N)
    return ks, kg, sks, pks, cts


@pytest.mark.parametrize("recipient", ["carol", "user0"])
def test_without_a_flood_a_share_is_the_plain_share_plus_an_encryption_of_zero_without_e0(world, recipient):
    ks, kg, sks, pks, cts = world
    ct, count = cts[3], 2
    q = np.array(ks.Q, dtype=np.uint64)[:, None]
    zero = [0] * ks.N
    for b, who in enumerate(("user1", "user2")):
        u, e1 = P.u_poly(KEY, NONCE, count, b, ks.N), P.e1_poly(KEY, NONCE, count, b, ks.N, CDT)
        got = P.share(ks, ct[who], sks[who], pks[recipient], u, e1, zero)
        enc = P.encrypt_zero(ks, pks[recipient], len(ks.Q), u, zero, e1)
        assert (got[0] == (D.share(ks, ct[who], sks[who], zero) + enc[0]) % q).all()
        assert (got[1] == enc[1]).all()
        # and a flood enters h0 alone, as the same integer in every limb
        E = P.flood_poly(KEY, NONCE, count, b, ks.N, 40)
        wide = P.share(ks, ct[who], sks[who], pks[recipient], u, e1, E)
        assert (wide[1] == got[1]).all()
        for j, m in enumerate(ks.Q):
            assert D.centred((wide[0][j] + np.uint64(m) - got[0][j]) % np.uint64(m), m) == E


@pytest.mark.parametrize("recipient", ["carol", "user0"])
@pytest.mark.parametrize("bits", [0, 40, 100])
@pytest.mark.parametrize("k", [1, 3])
def test_the_merge_decrypts_under_the_recipients_key_alone_within_the_noise_bound(world, k, bits, recipient):
    ks, kg, sks, pks, cts = world
    ct = cts[k]
    shares = []
    for i, who in enumerate(USERS[:k]):
        key = [KEY[0] + i] + KEY[1:]                            # every party draws under its own key
        u, e1, E = P.u_poly(key, NONCE, 1, 0, ks.N), P.e1_poly(key, NONCE, 1, 0, ks.N, CDT), P.flood_poly(key, NONCE, 1, 0, ks.N, bits)
        shares.append(P.share(ks, ct[who], sks[who], pks[recipient], u, e1, E))
    out = P.merge(ks.Q, ct["0"], shares)
    assert (out == P.merge(ks.Q, ct["0"], shares[::-1])).all()  # shares commute
    got = kg.decrypt({"0": out[0], recipient: out[1]}, {recipient: sks[recipient]})
    want = kg.decrypt(ct, sks)                                  # the phase of the input, which needs every key
    q = np.array(ks.Q, dtype=np.uint64)[:, None]
    diff, Q = H.crt_center((got + q - want) % q, ks.Q)
    bound = mkrlwe.PublicKeySwitcher.NoiseBound(k, bits, ks.N)
    assert bound == P.noise_bound(k, bits, ks.N) and 2 * bound < Q
    print("k = %d, flood_bits = %d: extra noise %d bits, bound %d bits" % (k, bits, max(abs(v) for v in diff).bit_length(), bound.bit_length()))
    assert 0 < max(abs(v) for v in diff) <= bound
    if bits >= 40:
        assert max(abs(v) for v in diff) >> (bits - 8)          # the flood is there


def test_noise_bound_is_an_exact_integer():
    nb = mkrlwe.PublicKeySwitcher.NoiseBound
    assert nb(1, 0, 1024) == 2 * 1024 * 19 and nb(3, 1, 1024) == 3 * (1 + 2 * 1024 * 19) and nb(2, 10, 16, bound=6) == 2 * (512 + 192)
    assert nb(4, 1000, 1 << 15) == 4 * ((1 << 999) + 2 * (1 << 15) * 19) and isinstance(nb(4, 1000, 1 << 15), int)
    assert mkrlwe.HostSampler().bound == 19 and len(CDT) // 2 == 19         # the truncation of e_R and of e1 at sigma 3.2


def test_max_flood_bits_and_the_slot_bound():
    Qs = PSET["Q"]
    fake = types.SimpleNamespace(Q=Qs, N=lambda: 1024, MaxLevel=lambda: 2, T=lambda: 65537)
    sw = mkrlwe.PublicKeySwitcher(fake)
    assert sw.MaxFloodBits() == sw.MaxFloodBits(2) == (B.q_product(Qs) // 2).bit_length() - 1
    assert sw.MaxFloodBits(0) == (Qs[0] // 2).bit_length() - 1
    ck = mkckks.PublicKeySwitcher(fake)
    assert ck.SwitchSlotBound(3, 40, 2.0 ** 54) == 1024 * mkrlwe.PublicKeySwitcher.NoiseBound(3, 40, 1024) / 2.0 ** 54
    pset = HB.small_bfv(10, 3)
    bf = mkbfv.PublicKeySwitcher(types.SimpleNamespace(Q=pset["Q"], N=lambda: 1024, MaxLevel=lambda: 2, T=lambda: pset["T"]))
    assert bf.MaxFloodBits(3) == mkbfv.Refresher(bf.params).MaxFloodBits(3) == B.max_flood_bits(pset["Q"], pset["T"], 3)
    assert bf.MaxFloodBits() == bf._most(2) == (B.q_product(pset["Q"]) // (2 * pset["T"])).bit_length() - 1
    wide = mkrlwe.PublicKeySwitcher(types.SimpleNamespace(Q=HB.BFV_PN15QP880["Q"] * 2, MaxLevel=lambda: 27))
    assert wide.MaxFloodBits() == 1024


def test_the_sampler_spends_one_nonce_per_call():
    s = mkrlwe.DeviceSampler(key=KEY, insecure_test_only=True)
    key, nonce, cdt, ncdt = s.switch_args()
    assert nonce == 0 and ncdt == len(CDT) and list(cdt) == CDT and list(key) == KEY
    assert s.share_args()[1] == 1 and s.switch_args()[1] == 2 and s.counter == 3
