"""CPU: the definitions behind the BFV plaintext operands (include/mkhe.h, "BFV plaintext operands") restated in Python integers at N = 16: the
centred lift in Montgomery form (mkbfv.Lift), and the product identity pt(a) p = pt([a b]_T) + small (mod Q) that makes MulPtxt decrypt.

Encoder.EncodeMul does not restate its forward NTT (it calls the engine's mkhe_ntt), so its check against a direct evaluation of the NTT
definition is a GPU test: tests/test_gpu_bfv_ptxt_stages.py::test_encode_mul_is_the_ntt_of_the_lift."""
import numpy as np
import pytest

import harness_bfv as HB
from mkhe_kklss_amd import mkbfv

LOGN, N = 4, 16
T_SMALL = [97, 193, 65537]                                              # primes = 1 mod 32


class StubParams:
    def __init__(self, Q, T):
        self.logN, self.Q, self._T = LOGN, list(Q), T

    def N(self): return N
    def LogN(self): return LOGN
    def T(self): return self._T
    def QCount(self): return len(self.Q)


def centred(m, T):
    m = int(m) % T
    return m - T if m > T // 2 else m


def negacyclic(a, b):
    """a * b mod X^N + 1 over the integers"""
    out = [0] * N
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            k = i + j
            out[k % N] += x * y if k < N else -x * y
    return out


@pytest.mark.parametrize("T", T_SMALL)
def test_lift_is_the_centred_representative_in_montgomery_form(T):
    Q = HB.small_bfv(LOGN, 2)["Q"] + [17, 89]                           # two limbs smaller than (most of) T: no q_l > T assumption
    params = StubParams(Q, T)
    rng = np.random.default_rng(T)
    m = [0, 1, T // 2, T // 2 + 1, T - 1, T, 2 ** 63 + 5, 2 ** 64 - 1] + [int(x) for x in rng.integers(0, T, N - 8)]
    got = mkbfv.Lift(np.array(m, dtype=np.uint64), params)
    assert got.shape == (len(Q), N) and got.dtype == np.uint64
    assert [centred(x, T) for x in m[:6]] == [0, 1, T // 2, -(T // 2), -1, 0]
    for l, q in enumerate(Q):
        for k, x in enumerate(m):
            c = centred(x, T)
            assert int(got[l, k]) < q and int(got[l, k]) == ((c % q) << 64) % q
            assert int(got[l, k]) * pow(1 << 64, -1, q) % q == c % q     # out of Montgomery form: the canonical residue of c
    # the centring is the one the decoder returns
    enc = mkbfv.Encoder(StubParams(HB.small_bfv(LOGN, 2)["Q"], T))
    v = rng.integers(-2 ** 62, 2 ** 62, N)
    assert [centred(x, T) for x in v] == list(enc.CoeffsToSlots(enc.SlotsToCoeffs(v)))


@pytest.mark.parametrize("T", T_SMALL)
def test_product_identity(T):
    """pt(a) p - pt([a b]_T) mod Q, centred, is eps p - eps' with |eps|, |eps'| <= 1/2 per coefficient: at most N (T/2) / 2 + 1/2 in size, and
    there is no Q mod T term -- so MulPtxt decrypts to a b mod T while N (T/2) (|e| + 1/2) < Q / (2T)"""
    Qs = HB.small_bfv(LOGN, 2)["Q"]
    Q = Qs[0] * Qs[1]
    rng = np.random.default_rng(T + 1)
    pt = lambda m: [((int(x) % T) * Q + T // 2) // T for x in m]
    for trial in range(8):
        a = [int(x) for x in rng.integers(0, T, N)]
        b = [int(x) for x in rng.integers(0, T, N)]
        if trial == 0:
            a, b = [T - 1] * N, [T // 2 + 1] * N                        # the largest |p|
        p = [centred(x, T) for x in b]
        ab = [x % T for x in negacyclic(a, b)]
        lhs = negacyclic(pt(a), p)
        for x, y in zip(lhs, pt(ab)):
            d = (x - y) % Q
            d = d - Q if d > Q // 2 else d
            assert 4 * abs(d) <= N * T + 2, (T, trial, d)
        # hence with noise e below the bound the rounding decoder returns a b mod T
        e = [int(x) for x in rng.integers(-1000, 1001, N)]
        assert N * T * T * (2 * 1000 + 1) < 2 * Q
        noisy = negacyclic([x + y for x, y in zip(pt(a), e)], p)
        assert [((T * (x % Q) + Q // 2) // Q) % T for x in noisy] == ab
