"""The Chebyshev evaluation of mkckks on the host (no GPU): chebyshev_blocks and the recurrence on plain floats, evaluate_chebyshev -- the body of
Evaluator.EvaluateChebyshevNew -- run on plain complex numbers by a mock evaluator in the manner of tests/test_polyeval_host.py (a mock ciphertext
is its payload = value * true scale and decodes by its DECLARED scale, so a wrong weight ratio or target scale anywhere in the schedule shows as
a wrong value), and chebyshev_approx on the sigmoid."""
import math
import types

import numpy as np
import pytest
from numpy.polynomial import chebyshev as NC

import harness as H
from mkhe_kklss_amd import mkckks
from mkhe_kklss_amd._abi import MkheError

PSET = H.small_ckks(10, nq=12)
DEGREES = list(range(1, 64)) + [127, 255]
INTERVALS = [(-1, 1), (-8, 8)]


@pytest.mark.parametrize("d", range(1, 256))
def test_blocks_and_recurrence_on_plain_floats(d):
    """sum_i (sum_j B[i][j] T_j) T_(m i), with every T_k built by T_(a+b) = 2 T_a T_b - T_(a-b) on the products of poly_eval_plan, against chebval"""
    rng = np.random.default_rng(d)
    c, x = rng.uniform(-1, 1, d + 1), np.linspace(-1, 1, 50)
    plan = mkckks.poly_eval_plan(d)
    B = mkckks.chebyshev_blocks(c, plan.m)
    assert B.shape == (plan.g, plan.m)
    T = {0: np.ones_like(x), 1: x}
    for k, a, b in plan.products:
        assert a - b in T, (k, a, b)                      # an earlier power, or 0
        T[k] = 2 * T[a] * T[b] - T[a - b]
    value = sum(sum(B[i][j] * T[j] for j in range(plan.m)) * T[plan.m * i] for i in range(plan.g))
    assert np.abs(value - NC.chebval(x, c)).max() <= 1e-9


class MockCt:
    def __init__(self, payload, level, scale):
        self.payload, self._level, self.Scale, self.ids = np.asarray(payload, dtype=np.complex128), level, float(scale), ["a", "b"]

    def Level(self): return self._level
    def ScalingFactor(self): return self.Scale
    def value(self): return self.payload / self.Scale


def _rint(z):
    return np.rint(np.real(z)) + 1j * np.rint(np.imag(z))


class MockEvaluator:
    """level and scale rules of mkckks.Evaluator.MulRelinOnceNew / MulRelinRawNew / LinCombNew / LinCombsNew / SumNew; Rescale divides the payload by
    the dropped modulus"""

    def __init__(self, pset):
        self.Q = pset["Q"]
        self.params = types.SimpleNamespace(Q=self.Q, Scale=lambda: pset["scale"])
        self.calls, self.muls, self.raw, self.multi = 0, 0, 0, 0

    def MulRelinOnceNew(self, op0, op1, rlkSet, scale=None):
        self.calls += 1
        self.muls += 1
        level = min(op0.Level(), op1.Level())
        assert level >= 1
        q = float(self.Q[level])
        res = MockCt(op0.payload * op1.payload / q, level - 1, op0.Scale * op1.Scale / q)
        if scale is not None:
            res.Scale = float(scale)
        return res

    def MulRelinRawNew(self, op0, op1, rlkSet):
        self.calls += 1
        self.muls += 1
        self.raw += 1
        return MockCt(op0.payload * op1.payload, min(op0.Level(), op1.Level()), op0.Scale * op1.Scale)

    def LinCombNew(self, cts, weights, const=0, scale=None, rescale=True, level=None):
        self.calls += 1
        return self._row(cts, weights, const, scale, rescale, level)

    def LinCombsNew(self, cts, weight_rows, consts, scales=None, rescale=True, level=None):
        self.calls += 1
        self.multi += 1
        assert 1 <= len(cts) <= 16 and 1 <= len(weight_rows) <= 16 and len(weight_rows) == len(consts) == len(scales)
        return [self._row(cts, r, c, s, rescale, level) for r, c, s in zip(weight_rows, consts, scales)]

    def _row(self, cts, weights, const, scale, rescale, level):
        lmin = min(c.Level() for c in cts)
        l = lmin if level is None else level
        assert 0 <= l <= lmin and len(cts) == len(weights) and (l >= 1 or not rescale)
        scale = self.params.Scale() if scale is None else float(scale)
        s_mid = scale * float(self.Q[l]) if rescale else scale
        acc = _rint(complex(const) * s_mid) + sum(_rint(complex(w) * (s_mid / c.Scale)) * c.payload for c, w in zip(cts, weights))
        return MockCt(acc / float(self.Q[l]) if rescale else acc, l - (1 if rescale else 0), scale)

    def SumNew(self, cts):
        self.calls += 1
        assert all(c.Level() == cts[0].Level() and c.Scale == cts[0].Scale for c in cts)
        return MockCt(sum(c.payload for c in cts), cts[0].Level(), cts[0].Scale)


def _need(d, interval):
    return (0 if tuple(interval) == (-1, 1) else 1) + math.ceil(math.log2(d + 1)) + 1


@pytest.mark.parametrize("interval", INTERVALS, ids=["unit", "pm8"])
@pytest.mark.parametrize("d", DEGREES)
def test_schedule_on_plain_numbers(d, interval):
    a, b = interval
    rng = np.random.default_rng(2000 + d)
    coeffs, x = rng.uniform(-1, 1, d + 1), rng.uniform(a, b, 64)
    S, top = PSET["scale"], len(PSET["Q"]) - 1
    ref = NC.chebval((2 * x - a - b) / (b - a), coeffs)
    plan = mkckks.poly_eval_plan(d)
    results = []
    for fused in (True, False):
        ev = MockEvaluator(PSET)
        res = mkckks.evaluate_chebyshev(ev, MockCt(x * S, top, S), coeffs, interval, None, fused=fused)
        assert res.Scale == S
        assert res.Level() == top - _need(d, interval)
        assert np.abs(res.value() - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
        # every power of the plan is used by random coefficients: one product each, and one per giant power
        assert ev.raw == len(plan.products) and ev.muls == len(plan.products) + (plan.g - 1)
        assert ev.multi == (1 if fused and plan.g > 1 else 0)
        results.append(res)
    assert (results[0].payload == results[1].payload).all()


def test_monomial_schedule_fused_equals_unfused():
    rng = np.random.default_rng(5)
    S, top = PSET["scale"], len(PSET["Q"]) - 1
    z = rng.uniform(-1, 1, 32) + 1j * rng.uniform(-0.5, 0.5, 32)
    for d in (1, 3, 15, 22, 63):
        coeffs = rng.uniform(-1, 1, d + 1) + 1j * rng.uniform(-1, 1, d + 1)
        evs = [MockEvaluator(PSET), MockEvaluator(PSET)]
        plain = mkckks.evaluate_poly(evs[0], MockCt(z * S, top, S), coeffs, None)
        fused = mkckks.evaluate_poly(evs[1], MockCt(z * S, top, S), coeffs, None, fused=True)
        assert evs[0].multi == 0 and evs[1].multi == (1 if mkckks.poly_eval_plan(d).g > 1 else 0)
        assert plain.Level() == fused.Level() and plain.Scale == fused.Scale and (plain.payload == fused.payload).all()


def test_sparse_series_skips_unused_powers():
    """c_0, c_5 and c_13 at degree 15 (m = 4): T_13 = 2 T_1 T_12 - T_11 leaves -c_13 on T_11 = 2 T_3 T_8 - T_5, that c_13 on T_5 = 2 T_1 T_4 - T_3, that
    -(c_5 + c_13) on T_3.  No block uses T_2; it is built all the same, for T_3 and T_4"""
    coeffs = np.zeros(16)
    coeffs[0], coeffs[5], coeffs[13] = 0.5, -0.25, 1.0
    x = np.linspace(-1, 1, 33)
    S, top = PSET["scale"], len(PSET["Q"]) - 1
    ev = MockEvaluator(PSET)
    res = mkckks.evaluate_chebyshev(ev, MockCt(x * S, top, S), coeffs, (-1, 1), None, scale=S / 4)
    assert res.Scale == S / 4 and res.Level() == top - 5
    assert np.abs(res.value() - NC.chebval(x, coeffs)).max() <= 1e-9
    B = mkckks.chebyshev_blocks(coeffs, 4)
    assert [[j for j in range(4) if B[i][j]] for i in range(4)] == [[0, 3], [1], [3], [1]]
    # T_2, T_3, T_4, T_8, T_12 = 2 T_8 T_4 - T_4; then inner_0, the three other inner sums in one call, three giant products, one sum
    assert ev.raw == 5 and ev.muls == 5 + 3 and ev.calls == 2 * 5 + 1 + 1 + 3 + 1


def test_level_too_low_raises_before_any_call():
    S = PSET["scale"]
    x = np.linspace(-1, 1, 8)
    for d, interval in ((1, (-1, 1)), (3, (-1, 1)), (7, (-8, 8)), (63, (-1, 1)), (255, (-8, 8))):
        need = _need(d, interval)
        ev = MockEvaluator(PSET)
        with pytest.raises(MkheError):
            mkckks.evaluate_chebyshev(ev, MockCt(x * S, need - 1, S), np.ones(d + 1), interval, None)
        assert ev.calls == 0
        assert mkckks.evaluate_chebyshev(MockEvaluator(PSET), MockCt(x * S, need, S), np.ones(d + 1), interval, None).Level() == 0


def test_refused_before_any_call():
    S = PSET["scale"]
    ev, ct = MockEvaluator(PSET), MockCt(np.linspace(-1, 1, 8) * S, 11, S)
    for coeffs, interval in (([1.0], (-1, 1)), (np.ones(257), (-1, 1)), (np.zeros(4), (-1, 1)), (np.ones(4), (1, 1)), (np.ones(4), (2, -2))):
        with pytest.raises(MkheError):
            mkckks.evaluate_chebyshev(ev, ct, coeffs, interval, None)
    assert ev.calls == 0


def test_chebyshev_approx_of_the_sigmoid():
    sigmoid = lambda x: 1 / (1 + np.exp(-x))
    x = np.linspace(-8, 8, 4001)
    for d, bound in ((15, 2e-3), (31, 1e-5)):
        c = mkckks.chebyshev_approx(sigmoid, -8, 8, d)
        assert c.shape == (d + 1,) and c.dtype == np.float64
        err = np.abs(NC.chebval(x / 8, c) - sigmoid(x)).max()
        print("sigmoid on [-8, 8], degree %d: max error %.3g (bound %.0e)" % (d, err, bound))
        assert err <= bound
