"""The construction of mkbfv.LinearTransform without an engine context (no GPU): plan, masks and pre-rotated diagonals come from pure functions
(mkbfv.linear_transform_layout, mkbfv.matrix_layout), and the baby-step / giant-step formula evaluated with them on a numpy model of the two slot
rows -- np.roll per row for rot_k, a row swap for the conjugation -- must equal the defining sum mod T

    (M z)[r][j] = sum_k d_k[r][j] z[r][(j+k) mod n] + sum_k e_k[r][j] z[1-r][(j+k) mod n].

Everything is integer arithmetic mod T = 65537: the comparisons are equalities."""
import types

import numpy as np
import pytest

T = 65537
N_SLOTS = 512                        # n = N/2 of N = 2^10
INDICES, SWAPPED = [0, 1, 5, 8, 17, 300], [0, 3]


def rot(z, k):
    """rot_k: slot j + k moves to slot j in each row"""
    return np.roll(z, -k, axis=1)


def swap(z):
    return z[::-1]


def defining_sum(z, d, e):
    out = np.zeros_like(z)
    for k, v in d.items():
        out = (out + v * rot(z, k)) % T
    for k, v in e.items():
        out = (out + v * swap(rot(z, k))) % T
    return out


def bsgs(z, lay):
    """sum_g rot_g(sum_b d'_(g,b) (.) rot_b z) per part, then LT_d + swap(LT_e~): the schedule of Evaluator.LinearTransformBatch on the model"""
    babies = lay.plan.babies
    rots = {b: rot(z, b) for b in babies}
    giants, nd = lay.giants_d + lay.giants_e, len(lay.giants_d)
    assert len(giants) == len(lay.masks)
    terms, index = [], 0
    for g, mask in zip(giants, lay.masks):
        assert mask and not mask >> len(babies)
        acc = np.zeros_like(z)
        for i, b in enumerate(babies):
            if mask >> i & 1:
                part, gg, bb = lay.order[index]
                assert (gg, bb) == (g, b) and part == (0 if len(terms) < nd else 1)
                acc = (acc + lay.rows[index] % T * rots[b]) % T
                index += 1
        terms.append(rot(acc, g))
    assert index == len(lay.rows) == len(lay.order)
    zero = np.zeros_like(z)
    return (sum(terms[:nd], zero) + swap(sum(terms[nd:], zero))) % T


def random_rows(rng, n):
    return rng.integers(-(T // 2), T // 2 + 1, (2, n)).astype(np.int64)


@pytest.mark.parametrize("n1", [None, 1, 8, 16])
@pytest.mark.parametrize("which", ["both", "diagonals", "swapped"])
def test_baby_giant_formula_equals_the_defining_sum(n1, which):
    from mkhe_kklss_amd import mkbfv
    rng = np.random.default_rng(17 + (n1 or 0))
    n = N_SLOTS
    d = {k: random_rows(rng, n) for k in INDICES} if which != "swapped" else {}
    e = {k: random_rows(rng, n) for k in SWAPPED} if which != "diagonals" else {}
    if d:
        d[5] = d[5][0]                                              # a [n] array: the same diagonal in both rows
    lay = mkbfv.linear_transform_layout(n, d, e, n1)
    if n1 is not None:
        assert lay.plan.n1 == n1
    assert all(b < lay.plan.n1 for b in lay.plan.babies) and len(lay.plan.babies) <= 16
    assert sorted({g + b for p, g, b in lay.order if p == 0}) == sorted(d) and sorted({g + b for p, g, b in lay.order if p == 1}) == sorted(e)
    z = random_rows(rng, n)
    full = lambda m: {k: (np.stack([v, v]) if v.ndim == 1 else v) for k, v in m.items()}
    assert (bsgs(z, lay) == defining_sum(z, full(d), full(e))).all()


def test_indices_are_taken_mod_n_and_negative_indices_work():
    from mkhe_kklss_amd import mkbfv
    rng = np.random.default_rng(3)
    n = N_SLOTS
    d = {-1: random_rows(rng, n), n + 2: random_rows(rng, n)}
    lay = mkbfv.linear_transform_layout(n, d)
    z = random_rows(rng, n)
    assert (bsgs(z, lay) == defining_sum(z, {n - 1: d[-1], 2: d[n + 2]}, {})).all()


def replicated(v, n):
    return np.tile(v, n // len(v))


def test_from_matrix_8x8_acts_on_each_row():
    from mkhe_kklss_amd import mkbfv
    rng = np.random.default_rng(8)
    n, d = N_SLOTS, 8
    M = rng.integers(-(T // 2), T // 2 + 1, (d, d)).astype(np.int64)
    diags, swapped = mkbfv.matrix_layout(M, n)
    assert sorted(diags) == list(range(d)) and not swapped
    lay = mkbfv.linear_transform_layout(n, diags, swapped)
    v = rng.integers(-(T // 2), T // 2 + 1, (2, d)).astype(np.int64)
    z = np.stack([replicated(v[0], n), replicated(v[1], n)])
    want = np.stack([replicated(M.astype(object) @ v[r].astype(object) % T, n) for r in range(2)]).astype(np.int64)
    assert (bsgs(z, lay) == want).all()


def test_from_matrix_16x16_blocks_mix_the_rows():
    from mkhe_kklss_amd import mkbfv
    rng = np.random.default_rng(16)
    n, d = N_SLOTS, 8
    M = rng.integers(-(T // 2), T // 2 + 1, (2 * d, 2 * d)).astype(np.int64)
    diags, swapped = mkbfv.matrix_layout(M, n, blocks=True)
    assert sorted(diags) == list(range(d)) and sorted(swapped) == list(range(d))
    lay = mkbfv.linear_transform_layout(n, diags, swapped)
    assert lay.giants_d and lay.giants_e
    v = rng.integers(-(T // 2), T // 2 + 1, 2 * d).astype(np.int64)
    z = np.stack([replicated(v[:d], n), replicated(v[d:], n)])
    w = (M.astype(object) @ v.astype(object) % T).astype(np.int64)
    assert (bsgs(z, lay) == np.stack([replicated(w[:d], n), replicated(w[d:], n)])).all()
    # a block that is zero throughout leaves its diagonals out: [[A, 0], [C, D]] swaps through C alone
    M[:d, d:] = 0
    diags, swapped = mkbfv.matrix_layout(M, n, blocks=True)
    assert sorted(swapped) == list(range(d)) and not any(sw[0].any() for sw in swapped.values())
    M[d:, :d] = 0
    assert not mkbfv.matrix_layout(M, n, blocks=True)[1]
    # a sparse matrix: only the diagonals that are not zero
    S = np.zeros((d, d), dtype=np.int64)
    S[np.arange(d), (np.arange(d) + 3) % d] = 7
    assert sorted(mkbfv.matrix_layout(S, n)[0]) == [3]


def test_constructor_arguments_are_refused():
    from mkhe_kklss_amd import mkbfv
    from mkhe_kklss_amd._abi import MkheError
    n = N_SLOTS
    ones = np.ones((2, n), dtype=np.int64)
    lay = mkbfv.linear_transform_layout
    for bad in ((n, {}, None), (n, {}, {}), (n, None, None)):                         # at least one of the two is non-empty
        with pytest.raises(MkheError, match="no diagonal"):
            lay(*bad)
    with pytest.raises(MkheError, match="shape"):
        lay(n, {0: np.ones((2, n - 1), dtype=np.int64)})
    with pytest.raises(MkheError, match="shape"):
        lay(n, {0: ones}, {1: np.ones((3, n), dtype=np.int64)})
    with pytest.raises(MkheError, match="twice"):
        lay(n, {1: ones, n + 1: ones})
    with pytest.raises(MkheError, match="integers"):
        lay(n, {0: np.ones((2, n))})
    for n1 in (3, 32, 0):
        with pytest.raises(MkheError, match="n1"):
            lay(n, {0: ones}, None, n1)
    # 64 giants are the limit, over the two parts together
    wide = np.ones((2, 2048), dtype=np.int64)
    many = {16 * g: wide for g in range(33)}
    with pytest.raises(MkheError, match="giant"):
        lay(2048, many, many)
    assert len(lay(2048, {16 * g: wide for g in range(32)}, {16 * g: wide for g in range(32)}).masks) == 64
    with pytest.raises(MkheError, match="giant"):
        lay(2048, {16 * g: wide for g in range(65)})
    ml = mkbfv.matrix_layout
    with pytest.raises(MkheError, match="zero matrix"):
        ml(np.zeros((8, 8), dtype=np.int64), n)
    with pytest.raises(MkheError, match="zero matrix"):
        ml(np.zeros((16, 16), dtype=np.int64), n, blocks=True)
    for shape in ((8, 4), (6, 6), (2 * n, 2 * n)):
        with pytest.raises(MkheError, match="power of two"):
            ml(np.ones(shape, dtype=np.int64), n)
    with pytest.raises(MkheError, match="power of two"):
        ml(np.ones((12, 12), dtype=np.int64), n, blocks=True)
    with pytest.raises(MkheError, match="integers"):
        ml(np.ones((8, 8)), n)
    # the class refuses the same arguments before it touches a context
    fake = types.SimpleNamespace(N=lambda: 2 * n)
    with pytest.raises(MkheError, match="no diagonal"):
        mkbfv.LinearTransform(fake, {})
    with pytest.raises(MkheError, match="zero matrix"):
        mkbfv.LinearTransform.FromMatrix(fake, np.zeros((4, 4), dtype=np.int64))
