"""The plaintext linear transform of mkckks on the host (no GPU): linear_transform_plan as a pure function, the baby-step / giant-step identity with the
pre-rotated diagonals that LinearTransform stores, on plain numpy vectors (rot_k(z) = np.roll(z, -k): what RotateNew(ct, k) does to the slots), and
the diagonals LinearTransform.FromMatrix builds."""
import numpy as np
import pytest

from mkhe_kklss_amd import mkckks
from mkhe_kklss_amd._abi import MkheError


def _nonzero(v):
    return [x for x in v if x]


def test_plan_defaults():
    p = mkckks.linear_transform_plan(range(64), 512)
    assert p.n1 == 8 and len(_nonzero(p.babies)) == 7 and len(_nonzero(p.giants)) == 7
    assert p.babies == list(range(8)) and p.giants == list(range(0, 64, 8))
    p = mkckks.linear_transform_plan([0], 512)
    assert p.babies == [0] and p.giants == [0] and p.n1 == 1                      # no rotation at all; the tie goes to the smallest n1
    p = mkckks.linear_transform_plan([1, 1023], 512)                               # 1023 mod 512 = 511
    assert sorted(b + g for b in p.babies for g in p.giants if b + g in (1, 511)) == [1, 511]
    assert len(_nonzero(p.babies)) + len(_nonzero(p.giants)) == 2                  # two rotations: nothing does better for these two diagonals
    p = mkckks.linear_transform_plan([-1], 512)                                    # negative indices are taken mod n
    assert (p.babies, p.giants) == ([0], [511])


def test_plan_ties_go_to_the_smaller_n1():
    # {0, 1, 2, 3}: n1 = 2 costs one baby and one giant, n1 = 1 three giants, n1 = 4 three babies; {0, 2}: one rotation whatever n1, so n1 = 1
    assert mkckks.linear_transform_plan([0, 1, 2, 3], 512).n1 == 2
    assert mkckks.linear_transform_plan([0, 2], 512).n1 == 1


def test_plan_refuses_more_than_64_giants():
    far = [16 * i for i in range(66)]                      # 66 multiples of the largest n1: 66 giants whatever n1
    with pytest.raises(MkheError):
        mkckks.linear_transform_plan(far, 2048)
    assert len(mkckks.linear_transform_plan(far[:64], 2048).giants) == 64
    with pytest.raises(MkheError):
        mkckks.linear_transform_plan(range(0, 130, 2), 512, n1=2)                 # 65 giants at the forced n1 (the default would take n1 = 16)
    assert mkckks.linear_transform_plan(range(0, 130, 2), 512).n1 == 16
    for bad in (3, 32, 0):
        with pytest.raises(MkheError):
            mkckks.linear_transform_plan([0, 1], 512, n1=bad)
    with pytest.raises(MkheError):
        mkckks.linear_transform_plan([], 512)


@pytest.mark.parametrize("n1", [1, 2, 4, 8, 16])
def test_forced_n1_splits_every_index_exactly_once(n1):
    rng = np.random.default_rng(n1)
    idx = sorted({int(k) for k in rng.integers(0, 256, 40)} | {0, 255})
    p = mkckks.linear_transform_plan(idx, 512, n1=n1)
    assert p.n1 == n1 and all(0 <= b < n1 for b in p.babies) and all(g % n1 == 0 for g in p.giants)
    for k in idx:
        assert [(b, g) for b in p.babies for g in p.giants if b + g == k] == [(k % n1, k - k % n1)]


INDICES = [0, 1, 5, 8, 17, 300]


@pytest.mark.parametrize("n1", [None, 1, 4, 16])
def test_bsgs_identity_with_pre_rotated_diagonals(n1):
    n = 512
    rng = np.random.default_rng(3)
    cplx = lambda: rng.normal(size=n) + 1j * rng.normal(size=n)
    diag, z = {k: cplx() for k in INDICES}, cplx()
    direct = sum(d * np.roll(z, -k) for k, d in diag.items())
    p = mkckks.linear_transform_plan(diag, n, n1)
    got = np.zeros(n, dtype=np.complex128)
    for g in p.giants:
        inner = sum(np.roll(diag[g + b], g) * np.roll(z, -b) for b in p.babies if g + b in diag)
        got = got + np.roll(inner, -g)
    assert np.abs(got - direct).max() <= 1e-12
    # and the direct sum is the matrix with these diagonals: (M z)[j] = sum_k d_k[j] z[(j + k) mod n]
    M = np.zeros((n, n), dtype=np.complex128)
    for k, d in diag.items():
        M[np.arange(n), (np.arange(n) + k) % n] = d
    assert np.abs(M @ z - direct).max() <= 1e-10


@pytest.mark.parametrize("d", [1, 8, 64])
def test_matrix_diagonals_on_a_replicated_vector(d):
    n = 512
    rng = np.random.default_rng(d)
    M = rng.normal(size=(d, d)) + 1j * rng.normal(size=(d, d))
    if d == 8:
        M[np.arange(d), (np.arange(d) + 3) % d] = 0                                # an absent diagonal is left out
    v = rng.normal(size=d) + 1j * rng.normal(size=d)
    diags = mkckks.matrix_diagonals(M, n)
    assert sorted(diags) == [k for k in range(d) if not (d == 8 and k == 3)]
    z = np.tile(v, n // d)
    got = sum(dk * np.roll(z, -k) for k, dk in diags.items())
    assert np.abs(got - np.tile(M @ v, n // d)).max() <= 1e-12


def test_evaluator_has_the_entry_point():
    assert callable(mkckks.Evaluator.LinearTransformNew) and callable(mkckks.LinearTransform.FromMatrix) and callable(mkckks.LinearTransform.Rotations)
