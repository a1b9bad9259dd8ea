"""The host side of mkckks.Bootstrapper (no GPU): the four matrices against the Encoder, the cleartext EvalMod pipeline against the sine's own error, the
sparse secret sampler, and every refusal that needs no context.  Parameters are stand-ins with the accessors the pure functions read: no context is
opened."""
import math
import types

import numpy as np
import pytest

import harness as H
from mkhe_kklss_amd import mkckks, mkrlwe
from mkhe_kklss_amd._abi import MkheError


def fake_params(logN, logSlots, nq=16, crs=()):
    Q = H.PN16QP1761["Q"][:nq]
    return types.SimpleNamespace(logN=logN, Q=Q, CRS={i: None for i in crs}, N=lambda: 1 << logN, LogN=lambda: logN, LogSlots=lambda: logSlots,
                                 MaxLevel=lambda: nq - 1, Scale=lambda: float(1 << 45))


@pytest.mark.parametrize("logN,logSlots", [(10, 3), (10, 9), (6, 5)], ids=["10-3", "10-9", "6-5-full"])
def test_matrices_against_the_encoder(logN, logSlots):
    params, n = fake_params(logN, logSlots), 1 << logSlots
    enc = mkckks.Encoder(params)
    rng = np.random.default_rng([logN, logSlots])
    a = rng.uniform(-1, 1, 2 * n)
    m = np.zeros(1 << logN)
    m[:: enc.gap] = a
    z = enc.Project(m)
    assert np.abs(enc.Embed(z)[:: enc.gap] - a).max() <= 1e-12                  # a and z are one message
    M1, M2, C0, C1 = mkckks.bootstrap_matrices(params)
    assert all(M.shape == (n, n) for M in (M1, M2, C0, C1))
    c2s = np.abs(M1 @ z + M2 @ np.conj(z) - (a[:n] + 1j * a[n:])).max()
    s2c = np.abs(C0 @ a[:n] + C1 @ a[n:] - z).max()
    print("logN %d logSlots %d: coefficients to slots %.3g, slots to coefficients %.3g" % (logN, logSlots, c2s, s2c))
    assert c2s <= 1e-12 and s2c <= 1e-12
    assert not M2.any() and np.abs(C1 - 1j * C0).max() <= 1e-12                 # what SlotsToCoeffsNew and CoeffsToSlotsNew rely on


def _model_error(degree):
    ratio, K, r = 2.0 ** 10, 16, 3
    rng = np.random.default_rng(31)
    I = rng.integers(-15, 16, 4096)
    m = rng.uniform(-1, 1, 4096)
    got = mkckks.eval_mod_model(m / ratio + I, K, r, mkckks.eval_mod_coeffs(K, r, degree), ratio)
    return np.abs(got - m).max(), 2 * (2 * np.pi / ratio) ** 2 / 6


def test_cleartext_pipeline_meets_twice_the_sine_error():
    err, bound = _model_error(31)
    print("eval_mod_model, degree 31: 2^%.1f, bound 2^%.1f, the sine alone 2^%.1f" % (math.log2(err), math.log2(bound), math.log2(bound / 2)))
    assert err <= bound


def test_cleartext_pipeline_fails_at_degree_23():
    """the same assertion must fail for a series that is too short: the test above can fail"""
    err, bound = _model_error(23)
    print("eval_mod_model, degree 23: 2^%.1f, bound 2^%.1f" % (math.log2(err), math.log2(bound)))
    assert err > bound


@pytest.mark.parametrize("h", [0, 1, 32, 1024])
def test_ternary_hw_has_exactly_h_non_zeros(h):
    for sampler in (mkrlwe.HostSampler(np.random.default_rng(5), insecure_test_only=True), mkrlwe.HostSampler()):
        s = sampler.ternary_hw(1024, h)
        assert s.dtype == np.int32 and s.shape == (1024,) and np.count_nonzero(s) == h and set(np.unique(s)) <= {-1, 0, 1}
    with pytest.raises(MkheError):
        sampler.ternary_hw(1024, 1025)


def test_ternary_hw_signs_and_positions_are_spread():
    s = np.stack([mkrlwe.HostSampler(np.random.default_rng(k), insecure_test_only=True).ternary_hw(256, 64) for k in range(200)])
    assert abs(int(s.sum())) <= 6 * math.sqrt(200 * 64)                         # signs: a sum of 12800 fair +-1
    assert (np.abs(s).sum(axis=0) > 0).all()                                    # every position is hit (a miss has probability 256 * 0.75^200)


def test_bootstrapper_shape_and_rotations():
    b = mkckks.Bootstrapper(fake_params(10, 3))
    assert b.Depth() == 12 and b.level == 15 and b.n == 8 and b.gap == 64
    rots = b.Rotations()
    assert {8, 16, 32, 64, 128, 256} <= set(rots) and all(0 < r < 512 for r in rots)
    assert set(rots) - {8, 16, 32, 64, 128, 256} == {r for r in b.plan.babies + b.plan.giants if r}
    full = mkckks.Bootstrapper(fake_params(10, 9))                              # full packing: no SubSum, 16 x 32 diagonals
    assert full.gap == 1 and full.Rotations() == sorted({r for r in full.plan.babies + full.plan.giants if r}) and len(full.plan.giants) == 32
    assert mkckks.Bootstrapper(fake_params(10, 3), double_angle=2, degree=63).Depth() == 2 + 7 + 2 + 1


def test_refusals_without_a_device():
    with pytest.raises(MkheError, match="logSlots"):
        mkckks.Bootstrapper(fake_params(12, 11))
    with pytest.raises(MkheError, match="Depth"):
        mkckks.Bootstrapper(fake_params(10, 3, nq=12))                          # 12 moduli: one short of Depth() + 1
    mkckks.Bootstrapper(fake_params(10, 3, nq=13))
    with pytest.raises(MkheError, match="Depth"):
        mkckks.Bootstrapper(fake_params(10, 3), level=11)
    with pytest.raises(MkheError, match="Depth"):
        mkckks.Bootstrapper(fake_params(10, 3), level=16)
    b = mkckks.Bootstrapper(fake_params(10, 3, crs=[-1, -2] + mkckks.Bootstrapper(fake_params(10, 3)).Rotations()))
    ct = lambda level, scale: types.SimpleNamespace(Level=lambda: level, Scale=scale, ids=["alice", "bob"])
    rlk, rks, cks = mkrlwe.RelinearizationKeySet(None), mkrlwe.RotationKeySet(), mkrlwe.ConjugationKeySet()
    with pytest.raises(MkheError, match="level 0"):
        b.BootstrapNew(ct(1, 2.0 ** 45), rlk, rks, cks)
    with pytest.raises(MkheError, match="below 2\\^8"):
        b.BootstrapNew(ct(0, 2.0 ** 48), rlk, rks, cks)
    with pytest.raises(MkheError, match="rotation key"):                        # the CRS slots are there, the keys are not
        b.BootstrapNew(ct(0, 2.0 ** 45), rlk, rks, cks)
    b2 = mkckks.Bootstrapper(fake_params(10, 3, crs=[-1, -2]))
    with pytest.raises(MkheError, match="no CRS for rotation index"):
        b2.BootstrapNew(ct(0, 2.0 ** 45), rlk, rks, cks)
    with pytest.raises(MkheError, match="no CRS slot -2"):
        mkckks.Bootstrapper(fake_params(10, 3, crs=[-1])).BootstrapNew(ct(0, 2.0 ** 45), rlk, rks, cks)
    key = types.SimpleNamespace(Value=types.SimpleNamespace(h=None))
    for r in b.Rotations():
        rks.Value.setdefault("alice", {})[r] = key
        rks.Value.setdefault("bob", {})[r] = key
    with pytest.raises(MkheError, match="relinearization key"):
        b.BootstrapNew(ct(0, 2.0 ** 45), rlk, rks, cks)
    rlk.Value.update(alice=key, bob=key)
    with pytest.raises(MkheError, match="conjugation key"):
        b.BootstrapNew(ct(0, 2.0 ** 45), rlk, rks, cks)
