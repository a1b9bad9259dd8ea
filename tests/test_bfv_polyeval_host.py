"""The host side of the MK-BFV polynomial evaluation (no GPU): bfv_lincomb_consts against Python integers written here from the formulas of
include/mkhe.h ("BFV weighted sums": scale_up for the constant, the centred lift in Montgomery form for a weight), interpolate against the points it was
given, and evaluate_polys -- the body of Evaluator.EvaluatePolysNew -- driven by a cleartext stand-in whose ciphertexts are int arrays mod T.  The
stand-in counts its calls: one LinCombsNew per evaluation, at most one MulRelinSumNew per polynomial, no product for a power nobody uses."""
import types

import numpy as np
import pytest

from mkhe_kklss_amd import mkbfv, mkckks
from mkhe_kklss_amd._abi import MkheError

T = 65537
R = 1 << 64
Q_MIXED = [40961, 0x3ffffffff040001, 0x7ffffffffcc0001]           # one prime below T, two above


def test_consts_follow_the_header_formulas():
    weights = [[T - 1, T // 2, T // 2 + 1, -1, 0], [-(T // 2), 3 * T + 5, -T, 1, 2], [0, 0, 0, 0, 0]]
    consts = [0, T - 1, -7]
    got = mkbfv.bfv_lincomb_consts(Q_MIXED, T, weights, consts)
    assert got.dtype == np.uint64 and got.shape == (3, 6, 3)
    prod = Q_MIXED[0] * Q_MIXED[1] * Q_MIXED[2]
    for g in range(3):
        c = consts[g] % T
        for l, q in enumerate(Q_MIXED):
            assert int(got[g, 0, l]) == ((prod * c + T // 2) // T) % q
            for b, w in enumerate(weights[g]):
                w %= T
                centred = w if w <= T // 2 else w - T
                assert -T // 2 < centred <= T // 2
                assert int(got[g, 1 + b, l]) == (centred % q) * R % q, (g, b, l)
    # spot values: T - 1 is -1, T // 2 stays, T // 2 + 1 is -(T // 2); a zero weight is a zero word; q < T reduces the lift
    q0 = Q_MIXED[0]
    assert int(got[0, 1, 0]) == (q0 - 1) * R % q0 and int(got[0, 2, 0]) == (T // 2 % q0) * R % q0
    assert int(got[0, 3, 1]) == (Q_MIXED[1] - T // 2) * R % Q_MIXED[1]
    assert not got[2, 1:].any() and not got[0, 5].any()
    with pytest.raises(MkheError):
        mkbfv.bfv_lincomb_consts(Q_MIXED, T, [[1, 2], [1]], [0, 0])
    with pytest.raises(MkheError):
        mkbfv.bfv_lincomb_consts(Q_MIXED, T, [[1, 2]], [0, 0])


def horner(coeffs, x):
    acc = np.zeros_like(x)
    for c in reversed(coeffs):
        acc = (acc * x + int(c)) % T
    return acc


def test_interpolate_passes_through_its_points():
    rng = np.random.default_rng(8)
    xs = [int(v) for v in rng.choice(T, 8, replace=False)]
    ys = [int(v) for v in rng.integers(0, T, 8)]
    coeffs = mkbfv.interpolate(xs, ys, T)
    assert len(coeffs) == 8 and all(0 <= c < T for c in coeffs)
    assert [int(v) for v in horner(coeffs, np.array(xs, dtype=object))] == ys
    assert mkbfv.interpolate([5], [9], T) == [9]
    with pytest.raises(MkheError):
        mkbfv.interpolate([1, 2, 1 + T], [0, 0, 0], T)
    with pytest.raises(MkheError):
        mkbfv.interpolate([1, 2], [0], T)


class StandIn:
    """an evaluator over cleartext: a value is an int array mod T (dtype object); every call is counted"""

    def __init__(self, crs=True):
        self.params = types.SimpleNamespace(T=lambda: T, CRS={-1: None} if crs else {})
        self.products, self.lincombs, self.sums, self.adds = [], 0, 0, 0
        self.rows = 0

    def MulRelinNew(self, a, b, rlkSet):
        self.products.append((id(a), id(b)))
        return a * b % T

    def LinCombsNew(self, cts, weight_rows, consts):
        self.lincombs += 1
        self.rows += len(weight_rows)
        assert 1 <= len(cts) <= 16 and 1 <= len(weight_rows) <= 64 and len(consts) == len(weight_rows)
        assert all(len(r) == len(cts) for r in weight_rows)
        return [(sum(int(w) * c for w, c in zip(r, cts)) + int(k)) % T for r, k in zip(weight_rows, consts)]

    def MulRelinSumNew(self, ops0, ops1, rlkSet):
        self.sums += 1
        assert 1 <= len(ops0) == len(ops1) <= 16
        return sum(a * b for a, b in zip(ops0, ops1)) % T

    def AddNew(self, a, b):
        self.adds += 1
        return (a + b) % T


@pytest.fixture(scope="module")
def x():
    rng = np.random.default_rng(65537)
    v = rng.integers(0, T, 64).astype(object)
    v[:4] = [0, 1, T - 1, T // 2]
    return v


def used_powers(polys):
    """the powers the schedule may compute for these polynomials: the babies and giants in use, closed under the plan's products"""
    plan = mkckks.poly_eval_plan(max(len(p) - 1 for p in polys))
    need = set()
    for p in polys:
        for k, c in enumerate(p):
            if c % T:
                need |= {k % plan.m, k - k % plan.m}
    need -= {0, 1}
    for k, a, b in reversed(plan.products):
        if k in need:
            need |= {a, b}
    return need - {0, 1}


def run(polys, x):
    ev = StandIn()
    res = mkbfv.evaluate_polys(ev, x, polys, None)
    assert len(res) == len(polys)
    for r, p in zip(res, polys):
        assert (r == horner(p, x)).all()
    assert ev.lincombs == 1 and ev.sums <= len(polys) and ev.adds <= len(polys)
    assert len(ev.products) == len(used_powers(polys))          # one product per power in use, none for an unused one
    return ev


@pytest.mark.parametrize("d", list(range(1, 21)) + [63, 64, 255])
def test_every_degree_equals_horner(d, x):
    rng = np.random.default_rng(d)
    coeffs = [int(v) for v in rng.integers(1, T, d + 1)]
    ev = run([coeffs], x)
    plan = mkckks.poly_eval_plan(d)
    assert ev.rows == plan.g and ev.sums == (1 if plan.g > 1 else 0)
    assert len(ev.products) == len(plan.products)                # a dense polynomial uses every power of the plan
    # negative and unreduced coefficients are taken mod T
    run([[c - T if c % 2 else c + 3 * T for c in coeffs]], x)


def test_zero_blocks_and_a_lone_constant(x):
    # m = 4, g = 4: block 2 is all zero, block 3 is the lone constant 9 (the term 9 X^12); X^3 is used by nobody
    coeffs = [0] * 16
    coeffs[0], coeffs[5], coeffs[6], coeffs[12] = 5, T - 3, 11, 9
    ev = run([coeffs], x)
    assert ev.rows == 3 and ev.sums == 1 and ev.adds == 1
    assert len(ev.products) == 4                                  # X^2, X^4, X^8, X^12 -- not X^3
    # inner_0 all zero: no AddNew; only giants and constants: the baby list is the ciphertext itself under zero weights
    coeffs = [0] * 16
    coeffs[4], coeffs[8] = 7, 1
    ev = run([coeffs], x)
    assert ev.rows == 2 and ev.adds == 0 and len(ev.products) == 3         # X^2 (for X^4), X^4, X^8


def test_three_polynomials_share_powers_and_the_one_sum_call(x):
    rng = np.random.default_rng(3)
    polys = [[int(v) for v in rng.integers(0, T, d + 1)] for d in (20, 12, 2)]
    ev = run(polys, x)
    plan = mkckks.poly_eval_plan(20)
    assert ev.rows == sum(-(-(len(p)) // plan.m) for p in polys) and ev.sums == 2
    # the one-hot indicators of four points as four polynomials of one call
    pts = [3, 10, 200, 4000]
    polys = [mkbfv.interpolate(pts, [int(i == k) for i in range(4)], T) for k in range(4)]
    msg = np.array(pts * 16, dtype=object)
    res = mkbfv.evaluate_polys(StandIn(), msg, polys, None)
    for k in range(4):
        assert (res[k] == (msg == pts[k]).astype(object)).all()


def test_refused_before_any_call(x):
    for bad in ([[1]], [[]], [[1] * 257], [[0, 0, 0]], [[T, 2 * T]], [], [[1, 2], [0, T]]):
        ev = StandIn()
        with pytest.raises(MkheError):
            mkbfv.evaluate_polys(ev, x, bad, None)
        assert not ev.products and not ev.lincombs
    # 65 inner sums: five dense polynomials of degree 207 have 13 blocks each
    ev = StandIn()
    with pytest.raises(MkheError, match="65 inner sums"):
        mkbfv.evaluate_polys(ev, x, [[1] * 208] * 5, None)
    assert not ev.products and not ev.lincombs
    assert len(mkbfv.evaluate_polys(StandIn(), x, [[1] * 208] * 4 + [[1] * 192], None)) == 5          # 64 are accepted
    # a product is needed and CRS[-1] is missing
    ev = StandIn(crs=False)
    with pytest.raises(MkheError, match="CRS"):
        mkbfv.evaluate_polys(ev, x, [[1, 2, 3]], None)
    assert not ev.products and not ev.lincombs
