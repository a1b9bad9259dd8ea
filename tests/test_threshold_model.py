"""The model of the threshold secret keys (tests/threshold_model.py) against its own definitions (no GPU): every t-subset of the holders gives
the secret back word for word, a superset does too, t - 1 holders do not; kind 7 of the keystream is the product of kind 6 on its stream pair;
and the C ABI, the binding and the Python mirror carry the three calls."""
import itertools

import numpy as np
import pytest

import device_sampler_model as M
import sk_encrypt_model as SK
import threshold_model as T

KEY = [0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0, 0x082EFA98, 0xEC4E6C89]
NONCE = 0x0123456789ABCDEF
MODULI = [65537, 0x3fffffffd60001]          # a modulus the points nearly fill, and one of the engine's primes
POINTS = [1, 2, 7, 65536, 40000]            # 1, the largest point below the small modulus, non-consecutive values
N = 16


@pytest.fixture(scope="module")
def secret():
    rng = np.random.default_rng(5)
    return np.stack([rng.integers(0, m, N, dtype=np.uint64) for m in MODULI])


def reconstruct(sh, subset):
    active = [POINTS[p] for p in subset]
    return T.fold([T.additive(sh[p], POINTS[p], active, MODULI) for p in subset], MODULI)


@pytest.mark.parametrize("t", [1, 2, 3, 5])
def test_every_t_subset_reconstructs_a_superset_too_and_fewer_do_not(secret, t):
    sh = T.shares(secret, t, POINTS, KEY, NONCE, MODULI)
    assert sh.shape == (5, 2, N) and all((sh[:, j] < m).all() for j, m in enumerate(MODULI))
    for subset in itertools.combinations(range(5), t):
        assert (reconstruct(sh, subset) == secret).all(), subset
    if t < 5:
        for subset in itertools.combinations(range(5), t + 1):
            assert (reconstruct(sh, subset) == secret).all(), subset
    if t > 1:
        for subset in itertools.combinations(range(5), t - 1):
            assert (reconstruct(sh, subset) != secret).any(), subset
    else:
        assert all((sh[p] == secret).all() for p in range(5))      # t = 1: every share is the secret, and no stream is read


def test_shares_are_the_polynomial_at_the_points(secret):
    t, R = 3, len(MODULI)
    sh = T.shares(secret, t, POINTS, KEY, NONCE, MODULI)
    for j, m in enumerate(MODULI):
        c = [T.kind7_row(KEY, NONCE, k, j, R, m, N) for k in (1, 2)]
        for p, x in enumerate(POINTS):
            assert sh[p, j].tolist() == [(int(secret[j, i]) + c[0][i] * x + c[1][i] * x * x) % m for i in range(N)]
    only = T.shares(secret, t, POINTS[1:3], KEY, NONCE, MODULI, rows=[1])
    assert (only[:, 0] == sh[1:3, 1]).all()
    other = T.shares(secret, t, POINTS, KEY, NONCE + 1, MODULI)
    assert (other != sh).mean() > 0.9


def test_kind7_is_the_product_of_kind6_on_its_stream_pair():
    R = 5
    pairs = set()
    for k in (1, 2, 4):
        for j in (0, 3, 4):
            ls, hs = T.kind7_streams(k, j, R)
            assert (ls, hs) == (2 * ((k - 1) * R + j), 2 * ((k - 1) * R + j) + 1)
            pairs.add(ls)
            m = MODULI[j % 2]
            lo, hi = M.stream_values(KEY, NONCE, ls, N), M.stream_values(KEY, NONCE, hs, N)
            row = T.kind7_row(KEY, NONCE, k, j, R, m, N)
            assert row == [SK.uniform_value(l, h, m) for l, h in zip(lo, hi)]
            assert row == [SK.uniform_value_words(l, h, m) for l, h in zip(lo, hi)]
            assert all(0 <= v < m for v in row) and len(set(row)) > 1
            assert row == T.kind7_row(KEY, NONCE, k, j, R, m, N, values=SK.stream_values_np)
    assert len(pairs) == 9
    assert T.kind7_streams(1, 0, R) == SK.row_streams(0, 0, R)      # polynomial 1 sits where item 0 of kind 6 would, over R rows


def test_lagrange_coefficients_interpolate_at_zero():
    m = MODULI[1]
    active = [3, 1, 4294967295, 77]
    lam = [T.lagrange(x, active, m) for x in active]
    for poly in ([5], [5, 9], [5, 9, 1 << 50, 12345]):              # degree below the size of the set
        val = lambda x: sum(c * pow(x, e, m) for e, c in enumerate(poly)) % m
        assert sum(l * val(x) for l, x in zip(lam, active)) % m == poly[0]
    assert T.lagrange(9, [9], m) == 1
    with pytest.raises(AssertionError):
        T.lagrange(5, active, m)


def test_fold_reduces_per_row():
    a = np.array([[[65536, 1]], [[7, 65530]]], dtype=np.uint64).reshape(2, 1, 2)      # two buffers [limbs = 1][2]
    assert T.fold(list(a), MODULI).tolist() == [[6, 65531]]
    big = np.full((3, 2, 4), MODULI[1] - 1, dtype=np.uint64)
    big[:, 0] = 65536
    assert T.fold([big, big, big], MODULI).tolist() == [[[65534] * 4, [MODULI[1] - 3] * 4]] * 3


def test_the_smallest_bfv_ring_has_room_for_the_floods_of_the_end_to_end_test():
    """tests/test_gpu_threshold_e2e.py runs on small_bfv(10, 3) with 3 and 4 floods of NoiseBits + 20 bits each.  A decryption share takes at most
    62 bits, and on this ring MaxFloodBits(4) = floor(log2(Q / (2 T 4))) is far above that: the ring is not what limits the flood, so no larger
    ring of harness_bfv is needed."""
    import types
    import harness_bfv as HB
    from mkhe_kklss_amd import mkbfv
    pset = HB.small_bfv(10, 3)
    me = types.SimpleNamespace(params=types.SimpleNamespace(Q=pset["Q"], T=lambda: pset["T"]))
    Q = pset["Q"][0] * pset["Q"][1] * pset["Q"][2]
    for floods in (3, 4):
        most = mkbfv.Decryptor.MaxFloodBits(me, floods)
        assert floods << (most - 1) <= Q // (4 * pset["T"]) < floods << most
        assert most >= 62 + 64


def test_the_three_calls_are_declared_bound_and_mirrored():
    import os
    from mkhe_kklss_amd import _abi, mkbfv, mkckks, mkrlwe
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mkhe.h")).read()
    for name in ("mkhe_threshold_gen_shares", "mkhe_threshold_additive_key", "mkhe_limbs_sum"):
        assert name in _abi.SIGNATURES and ("int  %s(" % name) in hdr
    for mod in (mkrlwe, mkckks, mkbfv):
        assert mod.Thresholdizer is mkrlwe.Thresholdizer and mod.Combiner is mkrlwe.Combiner and mod.SecretKeyShare is mkrlwe.SecretKeyShare
        assert callable(mod.Decryptor.FoldShares)
    assert "ARE the key" in mkrlwe.SecretKeyShare.__doc__ and "FLOODED exactly like" in mkrlwe.Combiner.AdditiveKey.__doc__
    assert "k - 1 + t" in mkrlwe.Decryptor.FoldShares.__doc__
