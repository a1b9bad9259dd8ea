"""The parts of the Python mirror of distributed decryption that make no engine call (no GPU): the ordering of the shares of a merge and its
refusals, the nonce counter shared with encryption, and the noise-budget helpers."""
import types

import pytest

from mkhe_kklss_amd import mkbfv, mkckks, mkrlwe
from mkhe_kklss_amd._abi import MkheError


def share(id, level=2, count=1):
    return types.SimpleNamespace(ID=id, count=count, Level=lambda: level)


def test_shares_are_ordered_by_the_ids_of_the_ciphertext():
    ids = ["user0", "user1", "user2"]
    a, b, c = share("user0"), share("user1"), share("user2")
    for given in ([a, b, c], [c, a, b], [b, c, a]):
        assert mkrlwe.order_shares(ids, 2, 1, given) == [a, b, c]
    assert mkrlwe.order_shares([], 2, 1, []) == []


def test_missing_duplicate_foreign_and_misfit_shares_are_refused():
    ids = ["user0", "user1"]
    with pytest.raises(MkheError, match="'user1' is missing"):
        mkrlwe.order_shares(ids, 2, 1, [share("user0")])
    with pytest.raises(MkheError, match="two shares of party 'user0'"):
        mkrlwe.order_shares(ids, 2, 1, [share("user0"), share("user1"), share("user0")])
    with pytest.raises(MkheError, match="does not have"):
        mkrlwe.order_shares(ids, 2, 1, [share("user0"), share("user1"), share("user7")])
    with pytest.raises(MkheError, match="at level 1"):
        mkrlwe.order_shares(ids, 2, 1, [share("user0"), share("user1", level=1)])
    with pytest.raises(MkheError, match="for 3 ciphertexts"):
        mkrlwe.order_shares(ids, 2, 1, [share("user0"), share("user1", count=3)])


def test_share_and_encrypt_draw_from_one_counter():
    s = mkrlwe.DeviceSampler(key=bytes(range(32)), insecure_test_only=True)
    key, n0 = s.share_args()
    _, n1, _, _ = s.encrypt_args()
    _, n2 = s.share_args()
    assert (n0, n1, n2) == (0, 1, 2) and s.counter == 3
    assert list(key) == [int.from_bytes(bytes(range(32))[4 * i: 4 * i + 4], "little") for i in range(8)]


def test_flood_bits_are_checked_before_any_engine_call():
    dec = mkrlwe.Decryptor(params=None)
    ct = types.SimpleNamespace(ids=["user0"], Level=lambda: 0)
    sk = types.SimpleNamespace(ID="user0")
    for bad in (-1, 63, 30.0, None):
        with pytest.raises(MkheError, match="flood_bits"):
            dec.ShareNew(ct, sk, bad, None)
    with pytest.raises(MkheError, match="DeviceSampler"):
        dec.ShareNew(ct, sk, 30, mkrlwe.HostSampler())
    with pytest.raises(MkheError, match="no component"):
        dec.ShareNew(ct, types.SimpleNamespace(ID="user1"), 30, None)
    with pytest.raises(TypeError):
        dec.ShareNew(ct, sk)                                    # no default: 0 is passed explicitly


def test_noise_budget_helpers():
    assert mkrlwe.Decryptor.FloodBound(3, 0) == 0
    assert mkrlwe.Decryptor.FloodBound(1, 1) == 1
    assert mkrlwe.Decryptor.FloodBound(3, 62) == 3 << 61
    assert mkckks.Decryptor.FloodBound is mkrlwe.Decryptor.FloodBound and mkbfv.Decryptor.FloodBound is mkrlwe.Decryptor.FloodBound
    ck = types.SimpleNamespace(params=types.SimpleNamespace(N=lambda: 1024), FloodBound=mkrlwe.Decryptor.FloodBound)
    assert mkckks.Decryptor.FloodSlotBound(ck, 2, 30, float(1 << 54)) == 1024 * 2 * 2.0 ** 29 / 2.0 ** 54
    Q, T = [(1 << 40) + 1, (1 << 30) + 3], 65537
    bf = types.SimpleNamespace(params=types.SimpleNamespace(Q=Q, T=lambda: T))
    for k in (1, 2, 3, 16):
        b = mkbfv.Decryptor.MaxFloodBits(bf, k)
        assert (1 << b) * 2 * T * k <= Q[0] * Q[1] < (1 << (b + 1)) * 2 * T * k           # b = floor(log2(Q / (2 T k)))
        assert 2 * mkrlwe.Decryptor.FloodBound(k, b) * 2 * T <= Q[0] * Q[1]                 # k 2^(b-1) <= Q / (4 T)
