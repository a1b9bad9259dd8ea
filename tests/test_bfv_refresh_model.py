"""The model of the collective refresh of MK-BFV (tests/bfv_refresh_model.py) and the parts of its Python mirror that make no engine call (no
GPU): kinds 4 and 5 of the keystream with their stream layout, the range of A, the flood at the word boundaries, up / down against
mkbfv.ScaleUp / ScaleDown, the whole protocol in integers for k = 1, 2, 3 at MaxFloodBits with |e_ct| up to Q / (8 T), the wrap past the margin
as a negative control, and the arithmetic of MaxFloodBits and RefreshNoiseBound."""
import random
import types

import numpy as np
import pytest

import bfv_refresh_model as B
import device_sampler_model as M
import harness_bfv as HB
from mkhe_kklss_amd import mkbfv

KEY = [0x9E3779B9, 0x7F4A7C15, 0xF39CC060, 0x5CEDC834, 0x1082276B, 0xF3A27251, 0xF86C6A11, 0xD0C18E95]
NONCE = 0xFEDCBA9876543210
ONES = (1 << 64) - 1
PSET = HB.small_bfv(10, 3)
QS, T = PSET["Q"], PSET["T"]
Q = B.q_product(QS)
BIG_T = 4294957057          # the largest prime = 1 mod 2^11 below 2^32 (tests/test_gpu_bfv_refresh.py finds it by search)
FAKE = types.SimpleNamespace(Q=QS, T=lambda: T, N=lambda: 1024, MaxLevel=lambda: 2)


def word(key, nonce, stream, i):
    w = M.chacha20_block(key, i // 8, nonce & M.M32, nonce >> 32, stream)
    return w[2 * (i % 8)] | (w[2 * (i % 8) + 1] << 32)


@pytest.mark.parametrize("t", [2, 3, 65537, BIG_T, (1 << 32) - 1])
def test_kind_4_is_in_range_monotone_and_needs_no_division(t):
    assert B.mask_value(0, 0, t) == 0 and B.mask_value(ONES, ONES, t) == t - 1
    rng, last = random.Random(4), 0
    for r in sorted(rng.getrandbits(128) for _ in range(200)):
        a = B.mask_value(r & ONES, r >> 64, t)
        assert 0 <= a < t and a >= last and a == r * t // (1 << 128)
        last = a
    # the first r that gives 1: ceil(2^128 / t)
    first = -(-(1 << 128) // t)
    assert B.mask_value((first - 1) & ONES, (first - 1) >> 64, t) == 0 and B.mask_value(first & ONES, first >> 64, t) == 1


@pytest.mark.parametrize("bits", [1, 63, 64, 65, 128, 129])
def test_kind_5_range_and_top_word_mask(bits):
    W, half = B.words(bits), 1 << (bits - 1)
    assert W == (1 if bits <= 64 else 2 if bits <= 128 else 3) and B.streams_per_item(bits) == 2 + W
    assert B.flood_value([0] * W, bits) == -half and B.flood_value([ONES] * W, bits) == half - 1
    top = bits - 64 * (W - 1)
    # bits of the top word above `top` do not reach the result; bit top - 1 does, with weight 2^(bits-1)
    if top < 64:
        assert B.flood_value([0] * (W - 1) + [ONES << top & ONES], bits) == -half
    assert B.flood_value([0] * (W - 1) + [1 << (top - 1)], bits) == 0
    # the low words count in full
    for w in range(W - 1):
        vs = [0] * W
        vs[w] = ONES
        assert B.flood_value(vs, bits) == -half + (ONES << (64 * w))
    rng = random.Random(bits)
    seen = set()
    for _ in range(200):
        vs = [rng.getrandbits(64) for _ in range(W)]
        e = B.flood_value(vs, bits)
        assert -half <= e < half and B.flood_value([v ^ ONES for v in vs], bits) == -1 - e       # v -> ~v mirrors the range
        seen.add(e)
    assert len(seen) == (2 if bits == 1 else 200)


def test_zero_width_and_no_mask_read_no_stream():
    assert B.words(0) == 0 and B.streams_per_item(0) == 2 and B.flood_value([], 0) == 0
    assert B.flood_poly(None, 0, 3, 16, 0) == [0] * 16 and B.mask_poly(None, 0, 3, 16, T, 100, mask=0) == [0] * 16         # no key needed


@pytest.mark.parametrize("bits", [0, 1, 64, 65, 129])
def test_stream_layout(bits):
    """item b owns the streams b S .. b S + S - 1: lo, hi, then the words of the flood from the lowest"""
    n, S, W = 16, B.streams_per_item(bits), B.words(bits)
    for b in (0, 1, 3):
        A, e = B.mask_poly(KEY, NONCE, b, n, T, bits), B.flood_poly(KEY, NONCE, b, n, bits)
        for i in (0, 7, 8, 15):
            assert A[i] == B.mask_value(word(KEY, NONCE, b * S, i), word(KEY, NONCE, b * S + 1, i), T)
            assert e[i] == B.flood_value([word(KEY, NONCE, b * S + 2 + w, i) for w in range(W)], bits)
    assert B.mask_poly(KEY, NONCE, 0, n, T, bits) != B.mask_poly(KEY, NONCE, 1, n, T, bits)
    assert B.mask_poly(KEY, NONCE, 0, n, T, bits) != B.mask_poly(KEY, NONCE + 1, 0, n, T, bits)
    if bits == 65:      # the same stream numbers mean other things at another width: item 1 starts at stream 4, not 3
        assert B.mask_poly(KEY, NONCE, 1, n, T, 65) != B.mask_poly(KEY, NONCE, 1, n, T, 64)


@pytest.mark.parametrize("t", [T, BIG_T])
def test_up_and_down_are_the_scalings_of_mkbfv(t):
    fake = types.SimpleNamespace(Q=QS, T=lambda: t)
    rng = random.Random(9)
    xs = [0, 1, t // 2, t // 2 + 1, t - 1] + [rng.randrange(t) for _ in range(40)]
    assert (B.up_limbs(xs, QS, t) == mkbfv.ScaleUp(np.array(xs, dtype=object), fake)).all()
    Rs = [0, 1, Q // 2, Q // 2 + 1, Q - 1] + [rng.randrange(Q) for _ in range(40)]
    for x in (0, 1, t // 2, t - 1):                 # either side of the rounding boundary (2x + 1) Q / (2t)
        edge = (2 * x + 1) * Q // (2 * t)
        Rs += [edge, edge + 1]
        assert B.down(edge, QS, t) == x and B.down(edge + 1, QS, t) == (x + 1) % t
    poly = np.array([[R % q for R in Rs] for q in QS], dtype=np.uint64)
    assert [w - t if w > t // 2 else w for w in (B.down(R, QS, t) for R in Rs)] == mkbfv.ScaleDown(poly, fake).tolist()
    for x in xs:                                    # |up(x) - Q x / t| <= 1/2, and down undoes up
        assert abs(2 * t * B.up(x, QS, t) - 2 * Q * x) <= t and B.down(B.up(x, QS, t), QS, t) == x


def test_share_addend_and_plaintext_cancel_up_to_the_roundings():
    A = [0, 1, T // 2, T - 1, 12345]
    e = [0, -1, 1 << 100, -(1 << 100), 7]
    add, pt = B.share_addend(A, e, QS, T), B.reenc_plaintext(A, QS, T)
    for i in range(len(A)):
        s = B.crt([[add[j][i]] for j in range(3)], QS)[0] + B.crt([[pt[j][i]] for j in range(3)], QS)[0] - e[i]
        s %= Q                                      # up(A) + up(-A) = Q (A != 0) or 0, up to one unit of rounding
        assert min(s, Q - s) <= 1
    assert not B.reenc_plaintext([0], QS, T).any() and not B.share_addend([0], [0], QS, T).any()


def protocol(k, flood_bits, noise_bound, n=16, seed=1):
    """the refresh of one ciphertext over k parties coefficient by coefficient: the products c_i s_i are random, c_0 makes the phase
    up(m) + e_ct with |e_ct| <= noise_bound, including both extremes; each re-encryption has a random c_1 s product and noise of 20 bits
    -> (m, what the refreshed ciphertext decrypts to, its noise)"""
    rng = random.Random(seed)
    m = [rng.randrange(T) for _ in range(n)]
    e_ct = [noise_bound, -noise_bound] + [rng.randint(-noise_bound, noise_bound) for _ in range(n - 2)]
    prod = [[rng.randrange(Q) for _ in range(n)] for _ in range(k)]
    c0 = [(B.up(m[i], QS, T) + e_ct[i] - sum(p[i] for p in prod)) % Q for i in range(n)]
    limbs = lambda xs: np.array([[x % q for x in xs] for q in QS], dtype=np.uint64)
    shares, reenc, rprod = [], [], []
    for p in range(k):
        key = [KEY[0] + p] + KEY[1:]
        A, e = B.mask_poly(key, NONCE, 0, n, T, flood_bits), B.flood_poly(key, NONCE, 0, n, flood_bits)
        shares.append((limbs(prod[p]).astype(object) + B.share_addend(A, e, QS, T).astype(object)) % np.array(QS, dtype=object)[:, None])
        r = [rng.randrange(Q) for _ in range(n)]
        fresh = [rng.randint(-(1 << 20), 1 << 20) for _ in range(n)]
        pt = B.crt(B.reenc_plaintext(A, QS, T), QS)
        reenc.append(np.stack([limbs([(pt[i] + fresh[i] - r[i]) % Q for i in range(n)]), limbs([0] * n)]))
        rprod.append(r)
    out = B.merge(QS, T, limbs(c0), shares, reenc)
    phase = [(x + sum(r[i] for r in rprod)) % Q for i, x in enumerate(B.crt(out[0], QS))]
    noise = [min((ph - B.up(m[i], QS, T)) % Q, (B.up(m[i], QS, T) - ph) % Q) for i, ph in enumerate(phase)]
    return m, [B.down(ph, QS, T) for ph in phase], max(noise)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_share_merge_decode_gives_the_message_at_max_flood_bits(k):
    ref = mkbfv.Refresher(FAKE)
    bits = ref.MaxFloodBits(k)
    assert bits == B.max_flood_bits(QS, T, k) and k << (bits - 1) <= Q // (4 * T) < k << bits
    m, got, noise = protocol(k, bits, Q // (8 * T))
    assert got == m
    assert noise <= k * (1 << 20) + (k + 1) / 2     # the input's noise and the floods are gone: only the fresh noises and the roundings


def test_max_flood_bits_of_three_parties_on_the_three_prime_chain():
    assert mkbfv.Refresher(FAKE).MaxFloodBits(3) == 143 and mkbfv.Refresher(FAKE).MaxFloodBits(1) == (Q // (2 * T)).bit_length() - 1


def test_a_flood_past_the_margin_wraps():
    """negative control: one party, a flood eight bits wider than the whole margin Q / (2 T) -- the rounding goes wrong in most coefficients"""
    bits = (Q // (2 * T)).bit_length() + 8
    m, got, _ = protocol(1, bits, 0, n=64)
    assert sum(a != b for a, b in zip(m, got)) > 32


def test_refresh_noise_bound_and_the_cap():
    ref = mkbfv.Refresher(FAKE)
    assert ref.RefreshNoiseBound(2) == 2 * 2049 * 19 + 1.5 and ref.RefreshNoiseBound(3, sigma=1.0) == 3 * 2049 * 6 + 2
    wide = types.SimpleNamespace(Q=HB.BFV_PN15QP880["Q"] * 2, T=lambda: T, N=lambda: 1 << 15)
    assert mkbfv.Refresher(wide).MaxFloodBits(2) == 1024
    deep = types.SimpleNamespace(Q=HB.BFV_PN15QP880["Q"], T=lambda: T, N=lambda: 1 << 15)
    assert mkbfv.Refresher(deep).MaxFloodBits(4) == mkbfv.Decryptor.MaxFloodBits(types.SimpleNamespace(params=deep), 4)
