"""The model of the collective refresh (tests/refresh_model.py) and the parts of its Python mirror that make no engine call (no GPU): kind 3
of the keystream at its extremes, the two streams of a mask, the merge as CRT / centred / reduced against brute force, MaxMaskBits at its
edge, the arithmetic of RefreshSlotBound, the ordering of the shares of a merge and the nonce pair of a share."""
import types

import pytest

import device_sampler_model as M
import refresh_model as R
from mkhe_kklss_amd import mkckks, mkrlwe
from mkhe_kklss_amd._abi import MkheError

KEY = [0x9E3779B9, 0x7F4A7C15, 0xF39CC060, 0x5CEDC834, 0x1082276B, 0xF3A27251, 0xF86C6A11, 0xD0C18E95]
ONES = (1 << 64) - 1
TOP = 1 << 63


@pytest.mark.parametrize("bits", [1, 63, 64, 65, 120])
def test_kind_3_extremes(bits):
    half = 1 << (bits - 1)
    assert R.wide_value(0, 0, bits) == -half
    assert R.wide_value(ONES, ONES, bits) == half - 1
    # the last r of the lower half and the first of the upper half: -1 and 0
    assert R.wide_value(ONES, TOP - 1, bits) == -1 and R.wide_value(0, TOP, bits) == 0
    # only the top `bits` bits of the 128 count: the first value that moves the result, and the one below it
    step = 1 << (128 - bits)
    assert R.wide_value((step - 1) & ONES, (step - 1) >> 64, bits) == -half
    assert R.wide_value(step & ONES, step >> 64, bits) == -half + 1
    # lo alone reaches the result only when bits > 64
    assert (R.wide_value(ONES, 0, bits) == -half) == (bits <= 64)
    assert R.wide_value(TOP, 0, bits) == -half + ((TOP >> (128 - bits)) if bits > 64 else 0)
    for lo, hi in ((0, ONES), (ONES, 0), (TOP, TOP), (TOP - 1, TOP - 1), (0x0123456789ABCDEF, 0xFEDCBA9876543210)):
        e = R.wide_value(lo, hi, bits)
        assert -half <= e < half and R.wide_value(lo ^ ONES, hi ^ ONES, bits) == -1 - e          # r -> ~r mirrors the range
        assert e == (((hi << 64) + lo) // step) - half


def test_kind_3_zero_bits_reads_no_stream():
    assert R.wide_value(ONES, ONES, 0) == 0
    assert R.mask_poly(None, 0, 3, 16, 0) == [0] * 16           # no key needed


def test_kind_3_at_64_bits_is_the_high_stream_alone_and_below_it_kind_2_of_that_stream():
    import decrypt_share_model as D
    for bits in (1, 33, 62):
        for hi in (0, 1, TOP - 1, TOP, ONES, 0x0123456789ABCDEF):
            assert R.wide_value(0x5555555555555555, hi, bits) == D.flood_value(hi, bits)
    assert R.wide_value(12345, TOP + 5, 64) == 5


def test_the_mask_takes_streams_2b_and_2b_plus_1():
    nonce, bits, n = 0xFEDCBA9876543210, 100, 24
    for b in (0, 1, 5):
        m = R.mask_poly(KEY, nonce, b, n, bits)
        for i in (0, 7, 8, 13, 23):
            wl = M.chacha20_block(KEY, i // 8, nonce & M.M32, nonce >> 32, 2 * b)
            wh = M.chacha20_block(KEY, i // 8, nonce & M.M32, nonce >> 32, 2 * b + 1)
            lo = wl[2 * (i % 8)] | (wl[2 * (i % 8) + 1] << 32)
            hi = wh[2 * (i % 8)] | (wh[2 * (i % 8) + 1] << 32)
            assert m[i] == (((hi << 64) | lo) >> 28) - (1 << 99)
    assert R.mask_poly(KEY, nonce, 0, n, bits) != R.mask_poly(KEY, nonce, 1, n, bits)
    assert R.mask_poly(KEY, nonce, 0, n, bits) != R.mask_poly(KEY, nonce + 1, 0, n, bits)
    lim = R.mask_limbs([-1, 1 << 119, -(1 << 119)], [97])[0]
    neg = R.neg_mask_limbs([-1, 1 << 119, -(1 << 119)], [97])[0]
    assert [int(v) for v in lim] == [96, (1 << 119) % 97, (-(1 << 119)) % 97] and all((int(a) + int(b)) % 97 == 0 for a, b in zip(lim, neg))


def test_merge_is_crt_centred_reduced():
    """every x of Z_35 through the model with lin = 2, lout = 4 over (5, 7, 11, 13): brute force says what the lift is"""
    moduli, xs = [5, 7, 11, 13], list(range(35))
    c0 = [[x % 5 for x in xs], [x % 7 for x in xs]]
    got = R.merge(moduli, 2, 4, c0, [], [])
    for x in xs:
        lifted = x if x <= 17 else x - 35
        assert [int(got[0][j][x]) for j in range(4)] == [lifted % q for q in moduli]
    assert R.crt(c0, [5, 7]) == (xs, 35) and R.centre([0, 17, 18, 34], 35) == [0, 17, -17, -1]
    # shares and re-encryptions are added, c0 may be any representative, polynomial 1 of a re-encryption is copied
    share = [[3] * 35, [4] * 35]
    re = [[[1] * 35, [2] * 35, [3] * 35, [12] * 35], [[4] * 35, [5] * 35, [6] * 35, [7] * 35]]
    got = R.merge(moduli, 2, 4, [[v + 10 for v in c0[0]], c0[1]], [share], [re])
    for x in xs:
        y = R.crt([[(x + 3) % 5], [(x + 4) % 7]], [5, 7])[0][0]
        lifted = y if y <= 17 else y - 35
        assert [int(got[0][j][x]) for j in range(4)] == [(lifted + re[0][j][0]) % q for j, q in enumerate(moduli)]
    assert (got[1] == [[4] * 35, [5] * 35, [6] * 35, [7] * 35]).all()
    # lout = lin: the residues of the sum themselves (mkhe_decrypt_merge)
    same = R.merge(moduli, 2, 2, c0, [share], [[[[0] * 35] * 2, [[0] * 35] * 2]])
    assert [int(v) for v in same[0][0]] == [(x + 3) % 5 for x in xs] and [int(v) for v in same[0][1]] == [(x + 4) % 7 for x in xs]


def test_max_mask_bits_at_its_edge():
    f = mkrlwe.Refresher.MaxMaskBits
    for parties, msg_bits, bits in ((1, 0, 1), (2, 55, 60), (3, 10, 119), (4, 54, 120)):
        q = 2 * ((parties << (bits - 1)) + (1 << msg_bits)) + 1             # equality: parties 2^(bits-1) + 2^msg_bits = (Q - 1) / 2
        assert f(q, parties, msg_bits) == bits
        if bits > 1:
            assert f(q - 2, parties, msg_bits) == bits - 1                   # one less room: that bit is refused
        else:
            with pytest.raises(MkheError, match="no mask fits"):
                f(q - 2, parties, msg_bits)
        if bits < 120:
            bigger = 2 * ((parties << bits) + (1 << msg_bits)) + 1
            assert f(bigger - 2, parties, msg_bits) == bits and f(bigger, parties, msg_bits) == bits + 1
    assert f(1 << 400, 2, 60) == 120                                         # never above 120
    with pytest.raises(MkheError, match="no mask fits"):
        f((1 << 55) + 1, 2, 60)


def test_mkckks_max_mask_bits_and_slot_bound():
    Q = [(1 << 55) + 1, (1 << 54) + 3, (1 << 54) + 5]                        # (the helper multiplies, it does not need primes)
    ref = mkckks.Refresher(types.SimpleNamespace(N=lambda: 1024, Q=Q))
    scale = 2.0 ** 54
    # msg_bits = ceil(log2(scale)) + 1 = 55; the answer is the last bits with 2 * 2^(bits-1) + 2^55 <= (Q_1 - 1) / 2
    bits = ref.MaxMaskBits(2, 1, scale)
    assert bits == mkrlwe.Refresher.MaxMaskBits(Q[0] * Q[1], 2, 55)
    assert (1 << bits) + (1 << 55) <= (Q[0] * Q[1] - 1) // 2 < (1 << (bits + 1)) + (1 << 55) and 100 < bits < 120
    assert ref.MaxMaskBits(2, 1, scale, max_abs_slot=3.0) == mkrlwe.Refresher.MaxMaskBits(Q[0] * Q[1], 2, 57)
    assert ref.MaxMaskBits(4, 0, 2.0 ** 30) == mkrlwe.Refresher.MaxMaskBits(Q[0], 4, 31) == 52
    with pytest.raises(MkheError, match="no mask fits"):
        ref.MaxMaskBits(2, 0, scale)
    assert ref.RefreshSlotBound(2, scale) == 1024 * 2 * 2049 * 19 / scale
    assert ref.RefreshSlotBound(3, 2.0 ** 40, sigma=1.0) == 1024 * 3 * 2049 * 6 / 2.0 ** 40


def share(id, level=1, count=1, level_out=3):
    return types.SimpleNamespace(ID=id, count=count, Level=lambda: level, LevelOut=lambda: level_out)


def test_refresh_shares_are_ordered_and_misfits_refused_before_any_engine_call():
    ct = types.SimpleNamespace(ids=["user0", "user1"], Level=lambda: 1)
    ref = mkrlwe.Refresher(types.SimpleNamespace(MaxLevel=lambda: 3))
    a, b = share("user0"), share("user1")
    assert mkrlwe.order_shares(ct.ids, 1, 1, [b, a]) == [a, b]
    for shares, text in (([a], "'user1' is missing"), ([a, b, a], "two shares of party 'user0'"), ([a, b, share("user7")], "does not have"),
                         ([a, share("user1", level=2)], "at level 2"), ([a, share("user1", count=3)], "for 3 ciphertexts"),
                         ([a, share("user1", level_out=2)], "different output levels")):
        with pytest.raises(MkheError, match=text):
            ref.MergeBatch([ct], shares)
    with pytest.raises(MkheError, match="no ciphertext"):
        ref.MergeBatch([], [a, b])
    with pytest.raises(MkheError, match="same ids"):
        ref.MergeBatch([ct, types.SimpleNamespace(ids=["user0"], Level=lambda: 1)], [a, b])


def test_refresh_args_take_two_nonces_of_the_one_counter():
    s = mkrlwe.DeviceSampler(key=bytes(range(32)), insecure_test_only=True)
    _, n0 = s.share_args()
    key, nm, ne = s.refresh_args()
    _, n3, _, _ = s.encrypt_args()
    assert (n0, nm, ne, n3) == (0, 1, 2, 3) and s.counter == 4 and list(key) == list(s._key)
    s._counter = (1 << 64) - 2
    with pytest.raises(MkheError, match="exhausted"):
        s.refresh_args()


def test_share_batch_refuses_bad_arguments_before_any_engine_call():
    ref = mkrlwe.Refresher(types.SimpleNamespace(MaxLevel=lambda: 3))
    ct = types.SimpleNamespace(ids=["user0", "user1"], Level=lambda: 1)
    sk, pk, other = types.SimpleNamespace(ID="user0"), types.SimpleNamespace(ID="user0"), types.SimpleNamespace(ID="user1")
    smp = mkrlwe.DeviceSampler(key=bytes(range(32)), insecure_test_only=True)
    for args, text in ((([], sk, pk, 100, smp), "no ciphertext"), (([ct], sk, other, 100, smp), "different parties"),
                       (([ct], sk, pk, 121, smp), "mask_bits"), (([ct], sk, pk, -1, smp), "mask_bits"), (([ct], sk, pk, 100, None), "DeviceSampler"),
                       (([ct], sk, pk, 100, smp, 4), "level_out"),
                       (([types.SimpleNamespace(ids=["user1"], Level=lambda: 1)], sk, pk, 100, smp), "no component"),
                       (([ct, types.SimpleNamespace(ids=["user0"], Level=lambda: 2)], sk, pk, 100, smp), "same level")):
        with pytest.raises(MkheError, match=text):
            ref.ShareBatch(*args)
    assert smp.counter == 0                                     # a refused call consumes no nonce
