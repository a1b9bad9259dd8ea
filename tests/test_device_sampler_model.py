"""The model of the device sampler (tests/device_sampler_model.py) and the host side of the feature, without a GPU: the block function
against RFC 8439 section 2.3.2, the moments of mkrlwe.small_cdt(3.2), the statistics of model draws under a fixed key, and the policy of
DeviceSampler.  Bounds: the table is built in float64, whose relative error of 2^-53 per operation leaves the symmetry and the mean far
inside 2^-50 / 2^-40; the variance of the rounded Gaussian is sigma^2 + 1/12 up to terms below 1e-30 (Poisson summation) minus the mass cut
off beyond 6 sigma, about 4e-7; sample statistics of n = 2^16 deterministic draws are held to 5 standard errors of the table's exact
moments."""
import math
from fractions import Fraction

import pytest

import device_sampler_model as M

KEY = [0x03020100 + 0x04040404 * i for i in range(8)]          # bytes 00 01 .. 1f, little-endian words
TEST_KEY = [0x9E3779B9, 0x7F4A7C15, 0xF39CC060, 0x5CEDC834, 0x1082276B, 0xF3A27251, 0xF86C6A11, 0xD0C18E95]
NCOEF = 1 << 16


def test_block_function_rfc8439_2_3_2():
    want = [int(w, 16) for w in ("e4e7f110 15593bd1 1fdd0f50 c47120a3 c7f4d1c7 0368c033 9aaa2204 4e6cd4c3 "
                                 "466482d2 09aa9f07 05d7c214 a2028bd9 d19c12b5 b94e16de e883d0cb 4e3c50a2").split()]
    assert M.chacha20_block(KEY, 1, 0x09000000, 0x4A000000, 0) == want
    # the same block through the sampler's mapping: nonce = words 13 (low) and 14 (high), stream = word 15, coefficient i of block 1 = 8 + i
    rs = M.stream_values(KEY, 0x4A00000009000000, 0, 16)
    assert rs[8:] == [want[2 * j] | (want[2 * j + 1] << 32) for j in range(8)]


def test_kinds():
    assert [M.ternary(r) for r in (0, 1, 2, 3, 4, 5, 6, 7, (1 << 64) - 1, (1 << 64) - 2, (1 << 64) - 4)] == [-1, 0, 1, 0, -1, 0, 1, 0, 0, 1, -1]
    cdt = [(1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 1]
    got = [M.table(r, cdt) for r in (0, (1 << 32) - 2, (1 << 32) - 1, 1 << 32, (1 << 63) - 1, 1 << 63, (1 << 64) - 2, (1 << 64) - 1)]
    assert got == [-2, -2, -1, 0, 0, 1, 1, 2]
    assert M.encrypt_samples(2, KEY, 5, 8, cdt)[1][2] == M.sample_small(1, 1, KEY, 5, 5, 8, cdt)[0]        # item 1, e1 = stream 3 * 1 + 2


@pytest.fixture(scope="module")
def cdt():
    from mkhe_kklss_amd import mkrlwe
    return mkrlwe.small_cdt(3.2)


def test_small_cdt_moments(cdt):
    sigma = 3.2
    assert len(cdt) == 38 and all(isinstance(t, int) and 0 <= t < 1 << 64 for t in cdt)
    assert all(a < b for a, b in zip(cdt, cdt[1:]))
    prob = M.table_probabilities(cdt)
    assert sorted(prob) == list(range(-19, 20)) and sum(prob.values()) == 1 and all(p > 0 for p in prob.values())
    asym = max(abs(prob[k] - prob[-k]) for k in range(1, 20))
    mean, var = M.moments(prob)
    print("small_cdt(3.2): asymmetry %.3g, mean %.3g, variance %.9f (sigma^2 + 1/12 = %.9f)" % (float(asym), float(mean), float(var), sigma ** 2 + 1 / 12))
    assert asym <= Fraction(1, 1 << 50)
    assert abs(mean) < Fraction(1, 1 << 40)
    assert abs(float(var) - (sigma ** 2 + 1.0 / 12.0)) < 1e-5


def test_small_cdt_arguments(cdt):
    from mkhe_kklss_amd import mkrlwe
    from mkhe_kklss_amd._abi import MkheError
    assert mkrlwe.small_cdt(3.2, 19) == cdt
    assert len(mkrlwe.small_cdt(3.2, 4)) == 8 and len(mkrlwe.small_cdt(5.0)) == 60 and len(mkrlwe.small_cdt(5.0, 32)) == 64
    with pytest.raises(MkheError, match="small_cdt"):
        mkrlwe.small_cdt(6.0)                        # B = 36: 72 entries
    with pytest.raises(MkheError, match="small_cdt"):
        mkrlwe.small_cdt(3.2, 33)
    with pytest.raises(MkheError, match="strictly increasing"):
        mkrlwe.small_cdt(0.4, 32)                    # the tail probabilities fall below 2^-64
    with pytest.raises(MkheError, match="small_cdt"):
        mkrlwe.small_cdt(0.0)


def test_model_draws_ternary():
    v = M.sample_poly(0, TEST_KEY, 1, 0, NCOEF)
    assert set(v) <= {-1, 0, 1}
    zeros, plus, minus = v.count(0), v.count(1), v.count(-1)
    print("ternary: %d zeros, %d / %d of +1 / -1 in %d draws" % (zeros, plus, minus, NCOEF))
    assert abs(zeros - NCOEF / 2) <= 5 * math.sqrt(NCOEF / 4)              # Binomial(n, 1/2)
    assert abs(plus - minus) <= 5 * math.sqrt(NCOEF / 2)                   # sum of n steps of variance 1/2


def test_model_draws_gaussian(cdt):
    v = M.sample_poly(1, TEST_KEY, 1, 1, NCOEF, cdt)
    assert min(v) >= -19 and max(v) <= 19
    prob = M.table_probabilities(cdt)
    mean, var = (float(x) for x in M.moments(prob))
    mu4 = float(sum((k - Fraction(mean)) ** 4 * p for k, p in prob.items()))
    m = sum(v) / NCOEF
    s2 = sum((x - mean) ** 2 for x in v) / NCOEF
    print("gaussian: mean %.5f (se %.5f), variance %.5f against %.5f (se %.5f)" % (m, math.sqrt(var / NCOEF), s2, var, math.sqrt((mu4 - var * var) / NCOEF)))
    assert abs(m - mean) <= 5 * math.sqrt(var / NCOEF)
    assert abs(s2 - var) <= 5 * math.sqrt((mu4 - var * var) / NCOEF)


def test_device_sampler_policy():
    from mkhe_kklss_amd import mkbfv, mkrlwe
    from mkhe_kklss_amd._abi import MkheError
    with pytest.raises(MkheError, match="insecure_test_only"):
        mkrlwe.DeviceSampler(key=bytes(range(32)))
    with pytest.raises(MkheError, match="32 bytes"):
        mkrlwe.DeviceSampler(key=bytes(31), insecure_test_only=True)
    with pytest.raises(MkheError, match="8 words"):
        mkrlwe.DeviceSampler(key=[1 << 32] * 8, insecure_test_only=True)
    a = mkrlwe.DeviceSampler(key=bytes(range(32)), insecure_test_only=True)
    assert list(a._key) == KEY and a.cdt == mkrlwe.small_cdt(3.2) and a.sigma == 3.2
    assert list(mkrlwe.DeviceSampler(key=KEY, insecure_test_only=True)._key) == KEY
    b, c = mkrlwe.DeviceSampler(), mkrlwe.DeviceSampler()                  # os.urandom
    assert list(b._key) != list(c._key)
    for kg in (mkrlwe.KeyGenerator, mkrlwe.NewKeyGenerator, mkbfv.KeyGenerator, mkbfv.NewKeyGenerator):
        with pytest.raises(MkheError, match="KeyGenerator"):
            kg(None, b)                              # refused before the parameters are looked at


def test_device_sampler_counter():
    from mkhe_kklss_amd import mkrlwe
    from mkhe_kklss_amd._abi import MkheError
    s = mkrlwe.DeviceSampler(key=KEY, insecure_test_only=True)
    assert s.counter == 0
    for n in range(3):
        key, nonce, table, ncdt = s.encrypt_args()                         # what one engine call consumes
        assert nonce == n and s.counter == n + 1 and ncdt == 38 and list(table) == s.cdt and list(key) == KEY
    s._counter = (1 << 64) - 2
    assert s.encrypt_args()[1] == (1 << 64) - 2
    with pytest.raises(MkheError, match="counter"):
        s.encrypt_args()                             # the last nonce is never handed out: the counter would wrap behind it
    assert s.counter == (1 << 64) - 1
