"""The host side of the factored slot / coefficient transforms of mkckks (no GPU): dft_factors against bootstrap_matrices' C0, the inverses, the shape of the
factors, the strided baby-step / giant-step plan, the cleartext pipeline through both bit reversals at 2048 slots, and the constructor of
Bootstrapper(.., factors=..) with its refusals.  Parameters are the stand-ins of tests/test_bootstrap_host.py (no context is opened); the tolerance is
that file's 1e-12."""
import math
import types

import numpy as np
import pytest

import harness as H
from mkhe_kklss_amd import mkckks
from mkhe_kklss_amd._abi import MkheError

TOL = 1e-12
CASES = [(1,), (1, 1), (2, 1), (1, 2), (2, 2), (3, 3), (4,), (5, 5), (1, 1, 1, 1, 1, 1)]
IDS = ["-".join(str(g) for g in c) for c in CASES]


def fake_params(logN, logSlots, nq=16, crs=()):
    Q = H.PN16QP1761["Q"][:nq]
    return types.SimpleNamespace(logN=logN, Q=Q, CRS={i: None for i in crs}, N=lambda: 1 << logN, LogN=lambda: logN, LogSlots=lambda: logSlots,
                                 MaxLevel=lambda: nq - 1, Scale=lambda: float(1 << 45))


def dense(diag, n):
    M = np.zeros((n, n), dtype=np.complex128)
    for k, d in diag.items():
        M[np.arange(n), (np.arange(n) + k) % n] += d
    return M


def apply(diag, z):
    return sum(d * np.roll(z, -k) for k, d in diag.items())


@pytest.mark.parametrize("groups", CASES, ids=IDS)
def test_product_of_the_factors_is_c0(groups):
    s = sum(groups)
    n = 1 << s
    factors, strides = mkckks.dft_factors(s, groups)
    assert len(factors) == len(strides) == len(groups)
    prod = np.eye(n, dtype=np.complex128)[mkckks.bit_reverse(n)]                  # R: (R a)[i] = a[bitrev(i)]
    for F in factors:
        prod = dense(F, n) @ prod
    C0 = mkckks.bootstrap_matrices(fake_params(s + 1, s))[2]
    err = np.abs(prod - C0).max()
    print("groups %r: |F_f .. F_1 R - C0| = %.3g" % (groups, err))
    assert err <= TOL


@pytest.mark.parametrize("groups", CASES, ids=IDS)
def test_inverses(groups):
    s = sum(groups)
    n = 1 << s
    fwd, strides = mkckks.dft_factors(s, groups)
    inv, strides_inv = mkckks.dft_factors(s, groups, inverse=True)
    assert strides_inv == strides and len(inv) == len(fwd)
    for F, G, g in zip(fwd, inv, groups):
        assert np.abs(dense(G, n) @ dense(F, n) - np.eye(n)).max() <= TOL
        assert sorted(G) == sorted((-k) % n for k in F)
        mod = np.abs(np.concatenate(list(G.values())))
        assert np.abs(mod[mod > 0] - 2.0 ** -g).max() <= TOL and (mod > 0).any()


@pytest.mark.parametrize("groups", CASES, ids=IDS)
def test_shape_of_the_factors(groups):
    s = sum(groups)
    n = 1 << s
    factors, strides = mkckks.dft_factors(s, groups)
    assert strides == [1 << sum(groups[:t]) for t in range(len(groups))]
    assert (strides, [sorted(F) for F in factors]) == mkckks.dft_groups(s, groups)          # what the Bootstrapper plans from
    for t, (F, g, stride) in enumerate(zip(factors, groups, strides)):
        assert len(F) == (1 << g if t == len(groups) - 1 else (2 << g) - 1)
        assert all(0 <= k < n and k % stride == 0 for k in F)
        assert all(d.shape == (n,) and d.dtype == np.complex128 for d in F.values())
        mod = np.abs(np.concatenate(list(F.values())))
        assert np.abs(mod[mod > 0] - 1).max() <= TOL


# ---- the strided plan
OLD_SETS = [(range(64), 512), ([0], 512), ([1, 1023], 512), ([-1], 512), ([0, 1, 2, 3], 512), ([0, 2], 512), ([16 * i for i in range(64)], 2048),
            (range(0, 130, 2), 512), ([0, 1, 5, 8, 17, 300], 512)]


def old_plan(indices, n, n1=None):
    """linear_transform_plan as it stood before the stride, restated"""
    idx = sorted({int(k) % n for k in indices})
    best = None
    for m in ([n1] if n1 is not None else [1, 2, 4, 8, 16]):
        babies, giants = sorted({k % m for k in idx}), sorted({k - k % m for k in idx})
        cost = sum(1 for b in babies if b) + sum(1 for g in giants if g)
        if len(giants) <= 64 and (best is None or cost < best[0]):
            best = (cost, (m, babies, giants))
    return best[1]


@pytest.mark.parametrize("case", range(len(OLD_SETS)))
def test_stride_one_is_the_old_plan(case):
    idx, n = OLD_SETS[case]
    for n1 in (None, 16):
        want = old_plan(idx, n, n1)
        for p in (mkckks.linear_transform_plan(idx, n, n1), mkckks.linear_transform_plan(idx, n, n1, stride=1), mkckks.linear_transform_plan(idx, n, n1=n1, stride=1)):
            assert p._fields == ("n1", "babies", "giants") and tuple(p) == want
    assert mkckks.linear_transform_plan([0, 2], 512).n1 == 1                               # the stride is never guessed


def test_strided_plan_of_the_second_factor():
    n = 1024
    factors, strides = mkckks.dft_factors(10, (5, 5))
    assert strides == [1, 32] and len(factors[0]) == 63 and len(factors[1]) == 32
    p = mkckks.linear_transform_plan(factors[1], n, stride=32)
    nzb, nzg = [b for b in p.babies if b], [g for g in p.giants if g]
    print("F_2 of (5,5): n1 = %d, %d babies, %d giants" % (p.n1, len(nzb), len(nzg)))
    assert all(r % 32 == 0 for r in p.babies + p.giants) and len(nzb) + len(nzg) <= 7 + 4
    assert all(b < 32 * p.n1 for b in p.babies) and all(g % (32 * p.n1) == 0 for g in p.giants)
    for k in factors[1]:
        assert [(b, g) for b in p.babies for g in p.giants if b + g == k] == [(k % (32 * p.n1), k - k % (32 * p.n1))]
    unstrided = mkckks.linear_transform_plan(factors[1], n)                                # without the stride every index is a giant
    assert unstrided.babies == [0] and len([g for g in unstrided.giants if g]) == 31
    p1 = mkckks.linear_transform_plan(factors[0], n)
    total = sum(1 for r in p1.babies + p1.giants + p.babies + p.giants if r)
    print("(5,5) at 1024 slots: %d rotations in all, against 78 for the dense transform" % total)
    assert total <= 24


@pytest.mark.parametrize("groups,t,n1", [((5, 5), 1, None), ((5, 5), 0, None), ((3, 3, 2), 1, 2), ((3, 3, 2), 2, None), ((2, 1), 1, None)])
def test_strided_bsgs_identity_with_pre_rotated_diagonals(groups, t, n1):
    s = sum(groups)
    n = 1 << s
    factors, strides = mkckks.dft_factors(s, groups)
    diag, stride = factors[t], strides[t]
    rng = np.random.default_rng([s, t])
    z = rng.normal(size=n) + 1j * rng.normal(size=n)
    p = mkckks.linear_transform_plan(diag, n, n1, stride=stride)
    got = np.zeros(n, dtype=np.complex128)
    for g in p.giants:
        inner = sum(np.roll(diag[g + b], g) * np.roll(z, -b) for b in p.babies if g + b in diag)
        got = got + np.roll(inner, -g)
    assert sum(1 for g in p.giants for b in p.babies if g + b in diag) == len(diag)
    assert np.abs(got - apply(diag, z)).max() <= TOL
    assert np.abs(dense(diag, n) @ z - apply(diag, z)).max() <= 1e-10


def test_an_index_off_the_stride_is_refused():
    with pytest.raises(MkheError, match="stride"):
        mkckks.linear_transform_plan([0, 32, 48], 1024, stride=32)
    with pytest.raises(MkheError, match="stride"):
        mkckks.linear_transform_plan([0, 1], 1024, stride=0)
    p = mkckks.linear_transform_plan([0, 32, -32], 1024, n1=2, stride=32)                  # -32 = 31 * 32 mod 1024: baby 32, giant 30 * 32
    assert (p.babies, p.giants) == ([0, 32], [0, 960])


# ---- both bit reversals cancel: the cleartext pipeline at 2048 slots
def test_cleartext_pipeline_at_2048_slots():
    s, groups, n = 11, (4, 4, 3), 2048
    params = fake_params(12, 11, nq=18)
    enc = mkckks.Encoder(params)
    ratio, K, r = 2.0 ** 10, 16, 3
    rng = np.random.default_rng(2048)
    a = rng.uniform(-1, 1, 2 * n)                                                  # the contract of eval_mod_model: every coefficient in (-1, 1)
    I = rng.integers(-(K - 1), K, 2 * n)
    z = enc.Project(a)                                                             # gap 1: the grid is every coefficient
    assert np.abs(enc.Embed(z) - a).max() <= TOL * 2 * n                           # (sums of 2n terms: these two are checks of the set-up, not the contract)
    inv, _ = mkckks.dft_factors(s, groups, inverse=True)
    fwd, _ = mkckks.dft_factors(s, groups)
    w = z
    for F in inv[::-1]:                                                            # F_f^-1 first, F_1^-1 last
        w = apply(F, w)
    rev = mkckks.bit_reverse(n)
    assert np.abs(w.real - a[:n][rev]).max() <= TOL * 2 * n and np.abs(w.imag - a[n:][rev]).max() <= TOL * 2 * n          # the order of the docstrings
    coeffs = mkckks.eval_mod_coeffs(K, r, 31)
    # what BootstrapNew declares: the slots that enter EvalMod are (a / ratio + I) / K, in whatever order CoeffsToSlots left them
    t_lo, t_hi = w.real / ratio + I[:n][rev], w.imag / ratio + I[n:][rev]
    lo, hi = (mkckks.eval_mod_model(t, K, r, coeffs, ratio) for t in (t_lo, t_hi))
    out = lo + 1j * hi
    for F in fwd:
        out = apply(F, out)
    err, bound = np.abs(out - z).max(), 2 * n * 2 * (2 * np.pi / ratio) ** 2 / 6
    print("cleartext pipeline, n = %d: 2^%.1f, bound 2^%.1f" % (n, math.log2(err), math.log2(bound)))
    assert err <= bound
    wrong = lo[rev] + 1j * hi[rev]                                                 # one reversal too many is an error of order |z|: the bound can fail
    for F in fwd:
        wrong = apply(F, wrong)
    assert np.abs(wrong - z).max() > 100 * bound


# ---- the constructor
def test_constructor_past_1024_slots():
    b = mkckks.Bootstrapper(fake_params(12, 11, nq=18), factors=((4, 4, 3), (4, 4, 3)))
    assert b.Depth() == 16 and b.level == 17 and b.n == 2048 and b.gap == 1
    rots = b.Rotations()
    assert rots and all(0 < r < 2048 for r in rots)
    assert set(rots) == {r for plans in b.plans for p in plans for r in p.babies + p.giants if r}                    # full packing: no SubSum index
    print("(4,4,3) twice at 2048 slots: %d rotation keys" % len(rots))
    sparse = mkckks.Bootstrapper(fake_params(12, 3, nq=18), factors=((2, 1), (1, 2)))
    sub = {8 << i for i in range(8)}
    assert sparse.gap == 256 and sub <= set(sparse.Rotations()) and sparse.Depth() == 14
    assert mkckks.Bootstrapper(fake_params(12, 3, nq=18), factors=((3,), (3,))).Depth() == 12
    plain = mkckks.Bootstrapper(fake_params(10, 3))                                # factors=None is the dense object
    assert plain.Depth() == 12 and plain.groups is None and plain.plan == mkckks.linear_transform_plan(range(8), 8)


def test_refusals_without_a_context():
    big = lambda **kw: fake_params(12, 11, **kw)
    with pytest.raises(MkheError, match="logSlots"):
        mkckks.Bootstrapper(big())                                                 # dense: still at most 1024 slots
    with pytest.raises(MkheError, match="logSlots"):
        mkckks.Bootstrapper(fake_params(10, 0, nq=18), factors=((), ()))           # logSlots < 1
    with pytest.raises(MkheError, match="groups"):
        mkckks.Bootstrapper(big(nq=18), factors=((4, 4, 3, 0), (4, 4, 3)))         # a group below 1
    with pytest.raises(MkheError, match="groups"):
        mkckks.Bootstrapper(big(nq=18), factors=((4, 4, 3), (-1, 12)))
    with pytest.raises(MkheError, match="groups"):
        mkckks.Bootstrapper(big(nq=18), factors=((4, 4, 2), (4, 4, 3)))            # a wrong sum
    with pytest.raises(MkheError, match="groups"):
        mkckks.Bootstrapper(big(nq=18), factors=((4, 4, 3), (4, 4, 4)))
    with pytest.raises(MkheError, match="giant"):
        mkckks.Bootstrapper(big(nq=18), factors=((10, 1), (4, 4, 3)))              # 2047 diagonals at stride 1: 128 giants
    mkckks.Bootstrapper(big(nq=18), factors=((1, 10), (4, 4, 3)))                  # 1024 diagonals in the last factor: 64 giants
    with pytest.raises(MkheError, match="Depth"):
        mkckks.Bootstrapper(big(nq=16), factors=((4, 4, 3), (4, 4, 3)))            # 16 moduli: one short of Depth() + 1 = 17
    mkckks.Bootstrapper(big(nq=17), factors=((4, 4, 3), (4, 4, 3)))
    with pytest.raises(MkheError, match="Depth"):
        mkckks.Bootstrapper(big(nq=18), factors=((4, 4, 3), (4, 4, 3)), level=15)
    with pytest.raises(MkheError, match="Depth"):
        mkckks.Bootstrapper(big(nq=18), factors=((4, 4, 3), (4, 4, 3)), level=18)
