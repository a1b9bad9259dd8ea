"""The polynomial evaluation schedule of mkckks on the host (no GPU): poly_eval_plan as a pure function, and evaluate_poly -- the body of
Evaluator.EvaluatePolyNew -- run on plain complex numbers by a mock evaluator that keeps level and scale the way MulRelinNew, LinCombNew and
Rescale do (float64 scales, the moduli of harness.small_ckks).  A mock ciphertext is its payload = value * true scale; it decodes by its DECLARED
scale, so a wrong weight ratio or target scale anywhere in the schedule shows as a wrong value, not only as a wrong label."""
import math
import types

import numpy as np
import pytest

import harness as H
from mkhe_kklss_amd import mkckks
from mkhe_kklss_amd._abi import MkheError

PSET = H.small_ckks(10, nq=9)
DEGREES = list(range(1, 64))


def _bound(plan):
    """multiplications beyond the squarings: (m - 2) + (g - 2) + (g - 1).  For degree 1 (m = 2, g = 1: no giant power whose squaring the g - 2 leaves
    out) the formula gives -1; there is nothing to multiply there, which is what the 0 asks."""
    return max(0, (plan.m - 2) + (plan.g - 2) + (plan.g - 1))


@pytest.mark.parametrize("d", DEGREES)
def test_plan_builds_every_power_from_earlier_ones(d):
    plan = mkckks.poly_eval_plan(d)
    b = math.ceil(math.log2(d + 1))
    assert plan.m == 2 ** math.ceil(b / 2) and plan.g == math.ceil((d + 1) / plan.m) and (plan.g - 1) * plan.m <= d < plan.g * plan.m
    have = {1}
    for k, a, c in plan.products:
        assert a in have and c in have and a + c == k and k not in have, (k, a, c)
        have.add(k)
    assert have == set(range(1, plan.m)) | {plan.m * i for i in range(1, plan.g)}
    for k in have:
        assert plan.depth[k] == math.ceil(math.log2(k)), k
    assert max(plan.depth.values()) <= b               # the deepest giant power still leaves the level of the last product
    beyond_squarings = sum(1 for k, a, c in plan.products if a != c) + (plan.g - 1)
    assert beyond_squarings <= _bound(plan), (beyond_squarings, _bound(plan))


def test_plan_rejects_degree_zero():
    with pytest.raises(MkheError):
        mkckks.poly_eval_plan(0)


class MockCt:
    def __init__(self, payload, level, scale):
        self.payload, self._level, self.Scale, self.ids = np.asarray(payload, dtype=np.complex128), level, float(scale), ["a", "b"]

    def Level(self): return self._level
    def ScalingFactor(self): return self.Scale
    def value(self): return self.payload / self.Scale


def _rint(z):
    return np.rint(np.real(z)) + 1j * np.rint(np.imag(z))


class MockEvaluator:
    """level and scale rules of mkckks.Evaluator.MulRelinOnceNew / LinCombNew / SumNew; Rescale divides the payload by the dropped modulus"""

    def __init__(self, pset):
        self.Q = pset["Q"]
        self.params = types.SimpleNamespace(Q=self.Q, Scale=lambda: pset["scale"])
        self.calls, self.beyond_squarings = 0, 0

    def MulRelinOnceNew(self, op0, op1, rlkSet, scale=None):
        self.calls += 1
        self.beyond_squarings += op0 is not op1
        level = min(op0.Level(), op1.Level())
        assert level >= 1
        q = float(self.Q[level])
        res = MockCt(op0.payload * op1.payload / q, level - 1, op0.Scale * op1.Scale / q)
        if scale is not None:
            res.Scale = float(scale)
        return res

    def LinCombNew(self, cts, weights, const=0, scale=None, rescale=True, level=None):
        self.calls += 1
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


@pytest.fixture(scope="module")
def slots():
    rng = np.random.default_rng(63)
    r, phi = np.sqrt(rng.uniform(0, 1, 64)), rng.uniform(0, 2 * np.pi, 64)
    return r * np.exp(1j * phi)                        # |z| <= 1


@pytest.mark.parametrize("d", DEGREES)
def test_schedule_on_plain_numbers(d, slots):
    rng = np.random.default_rng(1000 + d)
    coeffs = rng.uniform(-1, 1, d + 1) + (1j * rng.uniform(-1, 1, d + 1) if d % 2 else 0)
    ev, S, top = MockEvaluator(PSET), PSET["scale"], len(PSET["Q"]) - 1
    ct = MockCt(slots * S, top, S)
    res = mkckks.evaluate_poly(ev, ct, coeffs, None)
    ref = np.polyval(coeffs[::-1], slots)
    assert res.Scale == S
    assert res.Level() == top - (math.ceil(math.log2(d + 1)) + 1)
    assert np.abs(res.value() - ref).max() <= 1e-9 * np.abs(ref).max()
    assert ev.beyond_squarings <= _bound(mkckks.poly_eval_plan(d))


def test_sparse_polynomial_skips_zero_blocks_and_unused_powers(slots):
    coeffs = np.zeros(16, dtype=np.complex128)
    coeffs[0], coeffs[5], coeffs[13] = 0.5, -0.25j, 1.0            # blocks 0, 1 and 3 of m = 4; block 2 is all zero
    ev, S, top = MockEvaluator(PSET), PSET["scale"], len(PSET["Q"]) - 1
    res = mkckks.evaluate_poly(ev, MockCt(slots * S, top, S), coeffs, None, scale=S / 4)
    ref = np.polyval(coeffs[::-1], slots)
    assert res.Scale == S / 4 and res.Level() == top - 5
    assert np.abs(res.value() - ref).max() <= 1e-9 * np.abs(ref).max()
    # X^2, X^4, X^8, X^12 (X^3 is not needed), 3 inner sums, 2 products with a giant power, 1 final sum
    assert ev.calls == 4 + 3 + 2 + 1


def test_level_too_low_raises_before_any_call(slots):
    ev, S = MockEvaluator(PSET), PSET["scale"]
    for d, level in ((1, 1), (3, 2), (7, 3), (63, 6)):                # one level too low
        with pytest.raises(MkheError):
            mkckks.evaluate_poly(ev, MockCt(slots * S, level, S), np.ones(d + 1), None)
        assert ev.calls == 0
        assert mkckks.evaluate_poly(MockEvaluator(PSET), MockCt(slots * S, level + 1, S), np.ones(d + 1), None).Level() == 0
    for bad in ([1.0], np.ones(65), np.zeros(4)):
        with pytest.raises(MkheError):
            mkckks.evaluate_poly(ev, MockCt(slots * S, 8, S), bad, None)
    assert ev.calls == 0
