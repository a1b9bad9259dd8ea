"""The model of distributed decryption (tests/decrypt_share_model.py), no GPU: kind 2 of the keystream at its extremes, the reduction of a
negative sample, and the two identities that anchor the parity of mkhe_decrypt_share / mkhe_decrypt_merge, on the oracle's ring at
logN = 10 for 1, 2 and 3 parties:
  flood_bits = 0  the merge of all shares is Decrypt (harness.KeyGen.decrypt), bit for bit;
  flood_bits > 0  share - share|bits=0 is e mod q_j of the same integer e in every limb."""
import numpy as np
import pytest

import decrypt_share_model as D
import device_sampler_model as M
import harness as H
from oracle import oracle as O

KEY = [0x9E3779B9, 0x7F4A7C15, 0xF39CC060, 0x5CEDC834, 0x1082276B, 0xF3A27251, 0xF86C6A11, 0xD0C18E95]
PSET = H.small_ckks(10, 3)


@pytest.mark.parametrize("bits", [1, 32, 33, 62])
def test_kind_2_extremes(bits):
    assert D.flood_value(0, bits) == -(1 << (bits - 1))
    assert D.flood_value((1 << 64) - 1, bits) == (1 << (bits - 1)) - 1
    # the last r of the lower half and the first of the upper half: -1 and 0
    assert D.flood_value((1 << 63) - 1, bits) == -1 and D.flood_value(1 << 63, bits) == 0
    # only the top `bits` bits count
    assert D.flood_value((1 << (64 - bits)) - 1, bits) == -(1 << (bits - 1))
    assert D.flood_value(1 << (64 - bits), bits) == -(1 << (bits - 1)) + 1


def test_kind_2_zero_bits_reads_no_stream():
    assert D.flood_value((1 << 64) - 1, 0) == 0
    assert D.flood_poly(None, 0, 0, 16, 0) == [0] * 16          # no key needed


@pytest.mark.parametrize("bits", [1, 7, 32, 33, 62])
def test_kind_2_range_is_symmetric(bits):
    """r -> ~r maps e to -1 - e: the range is [-2^(bits-1), 2^(bits-1)) and every value has its mirror"""
    rng = np.random.default_rng(bits)
    for r in [int(v) for v in rng.integers(0, 1 << 63, 64, dtype=np.uint64)] + [0, 1, (1 << 64) - 1]:
        e = D.flood_value(r, bits)
        assert -(1 << (bits - 1)) <= e < (1 << (bits - 1))
        assert D.flood_value(r ^ ((1 << 64) - 1), bits) == -1 - e
    if bits <= 7:                                               # all values of the top bits: every e exactly once
        assert sorted(D.flood_value(t << (64 - bits), bits) for t in range(1 << bits)) == list(range(-(1 << (bits - 1)), 1 << (bits - 1)))


def test_kind_2_takes_the_words_of_kinds_0_and_1():
    """coefficient i: block i / 8, words 2 (i % 8) and 2 (i % 8) + 1 of stream s"""
    nonce, stream, bits = 0xFEDCBA9876543210, 5, 40
    e = D.flood_poly(KEY, nonce, stream, 24, bits)
    for i in (0, 7, 8, 13, 23):
        w = M.chacha20_block(KEY, i // 8, nonce & M.M32, nonce >> 32, stream)
        r = w[2 * (i % 8)] | (w[2 * (i % 8) + 1] << 32)
        assert e[i] == (r >> 24) - (1 << 39)
    assert D.flood_poly(KEY, nonce, stream + 1, 24, bits) != e and D.flood_poly(KEY, nonce + 1, stream, 24, bits) != e


def test_reduction_of_a_negative_sample():
    q = PSET["Q"][1]
    e = [-1, -q, -q - 1, -(1 << 61), (1 << 61) - 1, 0, q, -3 * q + 2]
    got = D.flood_limbs(e, [q])[0]
    assert [int(v) for v in got] == [q - 1, 0, q - 1, (-(1 << 61)) % q, ((1 << 61) - 1) % q, 0, 0, 2]
    assert all(0 <= int(v) < q for v in got)
    assert D.centred([q - 1, 1, 0, q // 2, q // 2 + 1], q) == [-1, 1, 0, q // 2, q // 2 + 1 - q]


@pytest.fixture(scope="module")
def world():
    """three parties with real keys and one ciphertext over 1, 2 and 3 of them: a fresh encryption under party 0 whose other party
    polynomials are uniform (the identities hold for any ciphertext)"""
    ks = O.KeySwitcher(PSET["logN"], PSET["Q"], PSET["P"], 2)
    kg = H.KeyGen(ks, seed=11)
    kg.add_crs(0)
    names = ["user0", "user1", "user2"]
    sks = {n: kg.gen_secret_key()[0] for n in names}
    level = len(PSET["Q"]) - 1
    pt = H.uniform_poly(kg.rng, ks.Q, ks.N)
    c0, c1 = kg.encrypt(pt, kg.gen_public_key(sks["user0"]), level)
    cts = {}
    for k in (1, 2, 3):
        cts[k] = {"0": c0, "user0": c1}
        for n in names[1:k]:
            cts[k][n] = H.uniform_poly(kg.rng, ks.Q, ks.N)
    return ks, kg, names, sks, cts


@pytest.mark.parametrize("k", [1, 2, 3])
def test_merge_of_unflooded_shares_is_decrypt(world, k):
    ks, kg, names, sks, cts = world
    ct = cts[k]
    shares = [D.share(ks, ct[n], sks[n], [0] * ks.N) for n in names[:k]]
    want = kg.decrypt(ct, sks)
    assert (D.merge(ks, ct["0"], shares) == want).all()
    assert (D.merge(ks, ct["0"], shares[::-1]) == want).all()   # shares commute


@pytest.mark.parametrize("k", [1, 2, 3])
def test_flooded_share_differs_by_e_in_every_limb(world, k):
    ks, kg, names, sks, cts = world
    ct, bits = cts[k], 40
    flooded, es = [], []
    for i, n in enumerate(names[:k]):
        e = D.flood_poly(KEY, 100 + i, 0, ks.N, bits)           # every party under its own nonce
        plain, mu = D.share(ks, ct[n], sks[n], [0] * ks.N), D.share(ks, ct[n], sks[n], e)
        for j, q in enumerate(ks.Q):
            diff = (mu[j] + np.uint64(q) - plain[j]) % np.uint64(q)
            assert D.centred(diff, q) == e                      # 2^39 < q / 2: the centred lift is e itself, the same in every limb
        flooded.append(mu)
        es.append(e)
    # and the merge carries the sum of the noises on top of Decrypt
    want, got = kg.decrypt(ct, sks), D.merge(ks, ct["0"], flooded)
    total = [sum(v) for v in zip(*es)]
    assert max(abs(v) for v in total) <= k << (bits - 1)
    for j, q in enumerate(ks.Q):
        assert D.centred((got[j] + np.uint64(q) - want[j]) % np.uint64(q), q) == total
