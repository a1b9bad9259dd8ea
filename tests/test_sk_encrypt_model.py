"""The model of secret-key encryption with a seeded c1 (tests/sk_encrypt_model.py) and the parts of its Python mirror that make no engine call
(no GPU): the (r q) >> 128 rule of kind 6 against exact integer arithmetic, the stream pairs of the rows, their independence of the number of
limbs expanded, the numpy keystream against the pure-Python one, and the identity the header states -- decryption gives pt + e exactly."""
import random

import numpy as np
import pytest

import device_sampler_model as M
import sk_encrypt_model as S
from mkhe_kklss_amd import mkrlwe
from mkhe_kklss_amd._abi import MkheError

KEY = [0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0, 0x082EFA98, 0xEC4E6C89]
NONCE = 0x0123456789ABCDEF
PRIMES = [0xffffffffffc0001, 0xfffffffff840001, 0x3fffffffd60001, 0x1fffffffffffd801, 0xffffff7801, 0xfd801]     # 60, 60, 54, 61, 40 and 20 bits


@pytest.mark.parametrize("q", PRIMES)
def test_uniform_rule_is_the_exact_quotient(q):
    rnd = random.Random(q)
    rs = [0, 1, (1 << 64) - 1, 1 << 64, (1 << 128) - 1, (1 << 128) - (1 << 64)] + [rnd.getrandbits(128) for _ in range(2000)]
    for r in rs:
        lo, hi = r & ((1 << 64) - 1), r >> 64
        want = r * q // 2 ** 128
        assert S.uniform_value(lo, hi, q) == want
        assert S.uniform_value_words(lo, hi, q) == want          # the kernel's 64-bit pieces and the carry
        assert 0 <= want < q
    assert S.uniform_value(0, 0, q) == 0 and S.uniform_value((1 << 64) - 1, (1 << 64) - 1, q) == q - 1


def test_rows_use_disjoint_stream_pairs():
    nq = 2
    pairs = [S.row_streams(b, j, nq) for b in range(2) for j in range(2)]
    flat = [s for p in pairs for s in p]
    assert sorted(flat) == list(range(8))                       # two items, two limbs: four pairs, eight streams, none shared
    assert all(hi == lo + 1 and lo % 2 == 0 for lo, hi in pairs)
    assert S.row_streams(1, 0, 4) == (8, 9)                     # the stride is nQ


def test_rows_are_the_named_streams():
    n, moduli = 16, [PRIMES[0], PRIMES[2]]
    a = S.sample_uniform(KEY, NONCE, 2, 2, moduli, n)
    for b in range(2):
        for j in range(2):
            lo = M.stream_values(KEY, NONCE, 2 * (b * 2 + j), n)
            hi = M.stream_values(KEY, NONCE, 2 * (b * 2 + j) + 1, n)
            assert [int(v) for v in a[b, j]] == [((h << 64 | l) * moduli[j]) >> 128 for l, h in zip(lo, hi)]
    assert len({tuple(int(v) for v in a[b, j]) for b in range(2) for j in range(2)}) == 4


def test_rows_do_not_depend_on_the_limbs_expanded():
    n, moduli = 16, [PRIMES[0], PRIMES[1], PRIMES[2]]
    full = S.sample_uniform(KEY, NONCE, 2, 3, moduli, n)
    for limbs in (1, 2):
        assert (S.sample_uniform(KEY, NONCE, 2, limbs, moduli, n) == full[:, :limbs]).all()
    # ... but they do depend on nQ, on the key and on the nonce
    assert not (S.sample_uniform(KEY, NONCE, 2, 2, moduli[:2], n)[1] == full[1, :2]).all()
    assert not (S.sample_uniform(KEY[::-1], NONCE, 1, 1, moduli, n) == full[:1, :1]).all()
    assert not (S.sample_uniform(KEY, NONCE + 1, 1, 1, moduli, n) == full[:1, :1]).all()


@pytest.mark.parametrize("stream", [0, 5, (1 << 32) - 1])
def test_numpy_keystream_is_the_model_keystream(stream):
    n = 64
    assert [int(v) for v in S.stream_values_np(KEY, NONCE, stream, n)] == M.stream_values(KEY, NONCE, stream, n)
    assert (S.sample_uniform(KEY, NONCE, 2, 2, PRIMES[:2], 16, S.stream_values_np) == S.sample_uniform(KEY, NONCE, 2, 2, PRIMES[:2], 16)).all()


def test_model_decryption_gives_pt_plus_e_exactly():
    n, moduli, cdt = 16, [PRIMES[0], PRIMES[2], PRIMES[5]], mkrlwe.small_cdt(3.2)
    rnd = random.Random(7)
    s = [rnd.choice((-1, 0, 1)) for _ in range(n)]
    a = S.sample_uniform(KEY, NONCE, 2, 3, moduli, n)
    for b in range(2):
        e = S.e_poly(KEY[::-1], 99, b, n, cdt)
        assert any(e) and all(abs(v) <= len(cdt) // 2 for v in e)
        pt = [[rnd.randrange(q) for _ in range(n)] for q in moduli]
        rows = [[int(v) for v in a[b, j]] for j in range(3)]
        c0, c1 = S.encrypt(rows, s, pt, e, moduli)
        assert c1 == rows                                       # a IS c1
        dec = S.decrypt(c0, c1, s, moduli)
        assert dec == [[(pt[j][i] + e[i]) % q for i in range(n)] for j, q in enumerate(moduli)]
        # a repeated a with two plaintexts reveals their difference (why an (a_key, a_nonce) pair serves one call)
        pt2 = [[rnd.randrange(q) for _ in range(n)] for q in moduli]
        d0, _ = S.encrypt(rows, s, pt2, e, moduli)
        assert [[(x - y) % q for x, y in zip(c0[j], d0[j])] for j, q in enumerate(moduli)] == \
               [[(x - y) % q for x, y in zip(pt[j], pt2[j])] for j, q in enumerate(moduli)]


def test_negacyclic_product():
    q = 97
    assert S.negacyclic([0, 1, 0, 0], [0, 0, 0, 1], q) == [q - 1, 0, 0, 0]      # X * X^3 = -1
    assert S.negacyclic([1, 2, 3, 4], [1, 0, 0, 0], q) == [1, 2, 3, 4]


def test_wire_bytes_halve():
    limbs, n = 14, 1 << 15
    assert S.wire_bytes(limbs, n, False) == 7340032             # 7.3 MB at PN15QP880
    assert S.wire_bytes(limbs, n, True) == 3670016 + 40


def test_seed_policy_and_sampler_counter():
    with pytest.raises(MkheError, match="insecure_test_only"):
        mkrlwe.SecretKeyEncryptor(None, None, seed=bytes(32))
    with pytest.raises(MkheError, match="32 bytes"):
        mkrlwe.SecretKeyEncryptor(None, None, seed=bytes(31), insecure_test_only=True)
    enc = mkrlwe.SecretKeyEncryptor(None, None, seed=bytes(range(32)), insecure_test_only=True)
    assert list(enc._seed) == [int.from_bytes(bytes(range(32))[4 * i: 4 * i + 4], "little") for i in range(8)]
    assert [enc._next_nonce() for _ in range(3)] == [0, 1, 2] and enc.counter == 3
    fresh = mkrlwe.SecretKeyEncryptor(None, None)
    assert list(fresh._seed) != list(mkrlwe.SecretKeyEncryptor(None, None)._seed)
    smp = mkrlwe.DeviceSampler(key=bytes(32), insecure_test_only=True)
    k, n0, cdt, ncdt = smp.sk_encrypt_args()
    assert n0 == 0 and ncdt == len(smp.cdt) and smp.encrypt_args()[1] == 1      # one counter for every kind of call
