"""CPU: the host model of the BFV batch encoder (mkbfv.Encoder) against the slot definition of include/mkhe.h restated in Python integers:
slot i = m(psi^(5^i)), slot N/2 + i = m(psi^(-5^i)) mod T, psi the engine's 2N-th root; Encode / Decode round trips through ScaleUp /
ScaleDown, decoding under noise, and the int64 conventions.  No device: the encoder needs N, T and Q only."""
import numpy as np
import pytest

import harness_bfv as HB
from mkhe_kklss_amd import mkbfv
from mkhe_kklss_amd._abi import MkheError

T_ALL = [65537, 786433, 4293918721]


class StubParams:
    def __init__(self, logN, Q, T):
        self.logN, self.Q, self._T = logN, list(Q), T

    def N(self): return 1 << self.logN
    def LogN(self): return self.logN
    def T(self): return self._T
    def QCount(self): return len(self.Q)


def centred(v, T):
    r = np.array([int(x) % T for x in v], dtype=np.int64)
    return np.where(r > T // 2, r - T, r)


def direct_slots(m, psi, logN, T):
    N = 1 << logN
    e, g = [], 1
    for _ in range(N // 2):
        e.append(g)
        g = g * 5 % (2 * N)
    e += [2 * N - x for x in e]
    out = []
    for k in e:
        x, acc = pow(psi, k, T), 0
        for c in m[::-1]:
            acc = (acc * x + int(c)) % T
        out.append(acc)
    return centred(out, T)


def test_slot_psi_is_the_engines_rule():
    assert mkbfv.slot_psi(65537, 1 << 15) == pow(3, 1, 65537)           # g = 3 generates Z_65537*; (T - 1) / 2N = 1
    for T in T_ALL:
        psi = mkbfv.slot_psi(T, 1 << 10)
        assert pow(psi, 1 << 10, T) == T - 1
    for T, text in ((257, "1 mod 2N"), (2049, "prime"), (4294967311, "below 2.32")):
        with pytest.raises(MkheError, match=text):
            mkbfv.slot_psi(T, 1 << 10)
    assert (mkbfv.slot_exponents(3) == [1, 5, 9, 13, 15, 11, 7, 3]).all()


@pytest.mark.parametrize("T", T_ALL)
@pytest.mark.parametrize("logN", [8, 9, 10])
def test_host_encoder_against_the_direct_evaluation(logN, T):
    enc = mkbfv.Encoder(StubParams(logN, HB.small_bfv(logN, 2)["Q"], T))
    N = 1 << logN
    rng = np.random.default_rng(logN)
    m = rng.integers(0, T, N, dtype=np.uint64)
    assert (enc.CoeffsToSlots(m) == direct_slots(m, enc.psi, logN, T)).all()
    x = np.zeros(N, dtype=np.uint64)
    x[1] = 1                                                            # X: slot j is psi^(e_j) itself
    e = mkbfv.slot_exponents(logN)
    assert (enc.CoeffsToSlots(x) == centred([pow(enc.psi, int(k), T) for k in e], T)).all()
    assert (enc.SlotsToCoeffs(enc.CoeffsToSlots(m)) == m).all()


@pytest.mark.parametrize("T", T_ALL)
@pytest.mark.parametrize("nq,big", [(1, False), (3, False), (3, True)])
def test_encode_decode_round_trip_and_int64_handling(T, nq, big):
    logN = 8
    p = StubParams(logN, HB.small_bfv(logN, nq, big)["Q"], T)
    enc, N = mkbfv.Encoder(p), 1 << logN
    rng = np.random.default_rng(nq)
    v = rng.integers(-2 ** 63, 2 ** 63 - 1, N, dtype=np.int64, endpoint=True)
    v[:8] = [-2 ** 63, 2 ** 63 - 1, -1, 0, T, -T, T // 2, T // 2 + 1]
    want = centred(v, T)
    assert want[2] == -1 and want[3] == want[4] == want[5] == 0 and want[6] == T // 2 and want[7] == T // 2 + 1 - T
    c = enc.SlotsToCoeffs(v)
    assert c.dtype == np.uint64 and (c < T).all()
    pt = enc.Encode(v)
    assert pt.shape == (nq, N) and (pt == mkbfv.ScaleUp(c, p)).all()
    assert (enc.Decode(pt) == want).all()
    # a decrypted phase carries noise: ScaleUp(m) + e with |e| < Q / 4T decodes to the same message
    Q = 1
    for q in p.Q:
        Q *= q
    lim = Q // (4 * T)
    es = [lim - 1, -(lim - 1)] + [int.from_bytes(rng.bytes(8 * nq), "little") % lim * (-1) ** i for i in range(N - 2)]
    noisy = np.array([[(int(x) + e) % q for x, e in zip(pt[l], es)] for l, q in enumerate(p.Q)], dtype=np.uint64)
    assert (enc.Decode(noisy) == want).all()
    with pytest.raises(MkheError):
        enc.Encode(v[:-1])


def test_message_type():
    m = mkbfv.Message([1, -2, 3])
    assert m.Value.dtype == np.int64 and m.Slots() == 3
    assert mkbfv.NewMessage(StubParams(8, [1], 65537)).Slots() == 256
