"""tests/noise_model.py, the definition of mkhe_noise_norm in Python integers, against plain arithmetic (no GPU): digits, the sign on the digits,
the complement with its carry, the lexicographic maximum and its tie rule, on the project's primes with 1, 2 and 4 limbs; the relation between
the BFV invariant value and the noise on random messages and errors."""
import random

import pytest

import harness as H
import harness_bfv as HB
import noise_model as M

QS = H.PN15QP880["Q"]
T = HB.BFV_PN15QP880["T"]


@pytest.mark.parametrize("limbs", [1, 2, 4])
def test_digits_sign_and_complement_are_those_of_the_integer(limbs):
    qs, rnd = QS[:limbs], random.Random(100 + limbs)
    Q = M.product(qs)
    edge = [0, 1, 2, Q - 1, Q - 2, (Q - 1) // 2, (Q + 1) // 2, (Q - 1) // 2 - 1, (Q + 1) // 2 + 1, int(qs[0]), int(qs[0]) - 1, Q - int(qs[0]), Q - M.product(qs[:-1])]
    for x in edge + [rnd.randrange(Q) for _ in range(300)]:
        x %= Q
        d = M.digits_of(x, qs)
        assert all(0 <= di < q for di, q in zip(d, qs)) and M.value_of(d, qs) == x
        assert M.garner([x % q for q in qs], qs) == d
        assert M.is_negative(d, qs) == (x > (Q - 1) // 2)
        if 0 < x:
            c = M.complement(d, qs)
            assert all(0 <= ci < q for ci, q in zip(c, qs)) and M.value_of(c, qs) == Q - x
        assert M.value_of(M.centre(d, qs), qs) == min(x, Q - x)


def test_the_complement_carries_through_zero_digits():
    qs = QS[:4]
    Q = M.product(qs)
    x = Q - int(qs[0]) * int(qs[1])                             # digits (0, 0, q_2 - 1, q_3 - 1): Q - x has the digits (0, 0, 1, 0)
    assert M.digits_of(x, qs) == [0, 0, qs[2] - 1, qs[3] - 1]
    assert M.complement(M.digits_of(x, qs), qs) == [0, 0, 1, 0]


@pytest.mark.parametrize("limbs", [1, 2, 4])
def test_lexicographic_order_of_the_digits_is_the_order_of_the_integers(limbs):
    qs, rnd = QS[:limbs], random.Random(200 + limbs)
    Q = M.product(qs)
    for _ in range(200):
        a, b = rnd.randrange(Q), rnd.randrange(Q)
        if rnd.random() < 0.3:                                  # neighbours, and pairs that differ in one digit only
            b = (a + rnd.choice([1, -1, int(qs[0]), M.product(qs[:-1])])) % Q
        da, db = M.digits_of(a, qs), M.digits_of(b, qs)
        assert (da[::-1] > db[::-1]) == (a > b)


def test_ties_go_to_the_smaller_index_whatever_the_order_of_the_candidates():
    qs = QS[:2]
    c = [(M.digits_of(v, qs), n) for n, v in enumerate([5, 9, 3, 9, 9, 1])]
    for order in ([0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0], [3, 0, 4, 1, 5, 2]):
        assert M.lex_max([c[i] for i in order]) == (M.digits_of(9, qs), 1)


@pytest.mark.parametrize("limbs", [1, 2, 4])
@pytest.mark.parametrize("kind,with_ref", [(0, False), (0, True), (1, False)])
def test_norm_by_digits_equals_norm_by_crt_on_random_residues(limbs, kind, with_ref):
    qs, rnd, N = QS[:limbs], random.Random(300 + 10 * limbs + 2 * kind + with_ref), 64
    phase = [[rnd.randrange(q) for _ in range(N)] for q in qs]
    ref = [[rnd.randrange(q) for _ in range(N)] for q in qs] if with_ref else None
    assert M.noise_norm(kind, phase, ref, qs, T) == M.noise_norm_crt(kind, phase, ref, qs, T)
    # a planted pair of equal maxima: the first one is reported
    Q, e = M.product(qs), [0] * N
    e[40], e[7], e[50] = (Q - 1) // 2, (Q + 1) // 2, 12345 % Q
    base = ref if with_ref else [[0] * N for _ in qs]
    planted = [[(b + v) % q for b, v in zip(row, e)] for row, q in zip(base, qs)]
    if kind == 0:
        assert M.noise_norm(0, planted, ref, qs) == ((Q - 1) // 2, 7) == M.noise_norm_crt(0, planted, ref, qs)


def test_bfv_bound_brackets_the_noise_and_the_budget_is_never_negative():
    rnd = random.Random(7)
    for qs in (HB.BFV_PN15QP880["Q"][:1], HB.BFV_PN15QP880["Q"][:3]):
        Q = M.product(qs)
        for trial in range(3000):
            m = rnd.randrange(T)
            room = Q // (4 * T)
            e = rnd.randint(-room, room) if trial % 3 else rnd.randint(-5, 5)
            phase = (M.scale_up(m, Q, T) + e) % Q
            x = T * phase % Q
            r = min(x, Q - x)
            b = M.bfv_noise_bound(r, T)
            assert abs(e) <= b <= abs(e) + 2, (m, e, b)
            assert M.noise_budget(r, Q) >= 0
        assert M.noise_budget((Q - 1) // 2, Q) == 0 and M.noise_budget(0, Q) == Q.bit_length() - 1
