"""The compensated key and its planted set, on the CPU (tests/steer_model.py): the plant reaches the reference's ModDown with the intended correction
index, the planted set separates the literal float64 index from four near misses that uniform data does not, and a ModDown result of 0 under a
sign-flipping automorphism is q in the oracle's Rotate.  tests/test_gpu_moddown_edges.py puts the same material through the device."""
import numpy as np
import pytest

import harness as H
import steer_model as S
from oracle import oracle as O

SETS = {
    "alpha1_np2": (H.small_ckks(11, 4), 2),
    "alpha2_np4": (H.small_alpha2(11, 5), 2),
}


def _steered_product(pset, gamma, level, seed):
    """(ks, plan, T, a, bg, out): one external product whose accumulator is NTT(T); the next seed if a digit has a zero"""
    ks = O.KeySwitcher(pset["logN"], pset["Q"], pset["P"], gamma)
    plan = S.Plan(pset["Q"], pset["P"], pset["logN"], level, seed=seed)
    while True:
        rng = np.random.default_rng(seed)
        a = H.uniform_poly(rng, ks.Q[: level + 1], ks.N)
        T = plan.target(rng)
        try:
            bg = S.steer(ks, level, ks.decompose(level, a), rng, T, H.uniform_swk)
        except ValueError:
            seed += 1000
            continue
        return ks, plan, T, a, bg, ks.external_product(level, a, bg)


@pytest.mark.parametrize("drop", [0, 1])
@pytest.mark.parametrize("name", list(SETS))
def test_plant_reaches_the_references_moddown(name, drop, capsys):
    """moddown_literal of the planted (x_Q, x_P) is the oracle's ExternalProduct output at EVERY coefficient of a steered key (the planted ones
    included), the digits and the keys being uniform: the plant reaches ModDown, and the index v the literal form takes at each pattern -- np for
    y = p - 1 everywhere, one above the true floor for the tuples just below an integer -- is the one the reference takes."""
    pset, gamma = SETS[name]
    level = len(pset["Q"]) - 1 - drop
    ks, plan, T, a, bg, out = _steered_product(pset, gamma, level, 11 + drop)
    nq, npr, Ql = len(ks.Q), len(ks.P), ks.Q[: level + 1]
    assert any((bg[i] != 0).any() for i in range(1, ks.beta(level))) or ks.beta(level) == 1
    for n in range(ks.N):
        r, _ = S.moddown_literal(T[: level + 1, n], T[nq:, n], Ql, ks.P)
        assert r == [int(x) for x in out[:, n]], n
    seen = {}
    for n, pat, variant in plan.planted():
        xq, xp = T[: level + 1, n], T[nq:, n]
        r, v = S.moddown_literal(xq, xp, Ql, ks.P)
        y = S.y_of(xp, ks.P)
        fl = S.index_exact(y, ks.P)
        seen.setdefault(pat, []).append(v)
        if pat == "y=p-1 all":
            assert v == npr and fl == npr - 1
        elif pat == "y=0":
            assert v == 0 and y == [0] * npr
        elif pat == "x_P=1":
            assert [int(x) for x in xp] == [1] * npr and v == fl
        elif pat.endswith("alone") or pat.endswith("quotient 1.0"):
            assert v == 1 and fl == 0
        elif pat.endswith("quotient <1"):
            assert v == 0 and fl == 0
        elif pat == "below":
            assert v == fl + 1 and 1 <= v <= npr - 1
        elif pat in ("above", "above_hi"):
            assert v == fl
        if variant == "zero":
            assert r == [0] * len(Ql) and (out[:, n] == 0).all()
        elif variant == "xq0":
            assert (xq == 0).all()
        else:
            assert [int(x) for x in xq] == [q - 1 for q in Ql]
    with capsys.disabled():
        print("\n[%s level %d] pattern: v the reference took x planted coefficients" % (name, level))
        for pat, vs in seen.items():
            print("  %-24s v = %-12s x %d" % (pat, sorted(set(vs)), len(vs)))


@pytest.mark.parametrize("name", list(SETS))
def test_planted_set_separates_the_near_misses_of_the_index(name, capsys):
    """Each of four wrong forms of the index -- the exact floor, y * (1.0 / p), a table clipped at np - 1, the terms added in reverse order -- differs
    from the literal form on at least two planted coefficients (the bar of the arithmetic primitives' probes).  A float sum of TWO terms commutes, so
    the reversed order is the literal form itself when np = 2: it is required from three special primes on.  How many of 2^12 uniform coefficients
    would have caught each is printed only."""
    pset, gamma = SETS[name]
    level = len(pset["Q"]) - 1
    ks = O.KeySwitcher(pset["logN"], pset["Q"], pset["P"], gamma)
    plan = S.Plan(pset["Q"], pset["P"], pset["logN"], level, seed=3)
    rng = np.random.default_rng(3)
    T = plan.target(rng)
    nq, Ql = len(ks.Q), ks.Q[: level + 1]
    planted = [n for n, _, _ in plan.planted()]
    uniform = [n for n in range(ks.N) if n not in set(planted)]
    U = np.stack([rng.integers(0, q, 1 << 12, dtype=np.uint64) for q in Ql + ks.P])
    lines = []
    for mname in S.MUTANTS:
        def differs(xq, xp):
            lit = S.moddown_literal(xq, xp, Ql, ks.P)
            assert S.moddown_with_index(xq, xp, Ql, ks.P) == lit              # (the pluggable restatement is the literal form)
            return S.mutant(mname, xq, xp, Ql, ks.P)[0] != lit[0]
        caught = sum(differs(T[: level + 1, n], T[nq:, n]) for n in planted)
        by_chance = sum(differs(U[: level + 1, k], U[level + 1:, k]) for k in range(1 << 12))
        lines.append("  %-24s planted: %3d of %d   uniform: %d of 4096" % (mname, caught, len(planted), by_chance))
        if mname != "reversed summation" or len(ks.P) >= 3:
            assert caught >= 2, (mname, caught)
        else:
            assert caught == 0
    with capsys.disabled():
        print("\n[%s] coefficients on which a near miss of the index differs from the literal form" % name)
        print("\n".join(lines))
    assert len(uniform) > ks.N // 2                                              # (the polynomial stays mostly uniform)


def test_flipped_zero_is_q_in_the_oracles_rotate():
    """At the planted coefficients every member's ModDown result and c_0 are 0 and the Galois element flips the sign: the oracle's Rotate holds q there
    (keyswitch.go:290), in out_0 (the sum over the members) and in the chosen party's own component; the control coefficient, which no automorphism
    flips, holds 0."""
    pset = H.small_ckks(11, 4)
    level = len(pset["Q"]) - 1
    ks = O.KeySwitcher(pset["logN"], pset["Q"], pset["P"], 2)
    plan = S.Plan(pset["Q"], pset["P"], pset["logN"], level, seed=5)
    rng = np.random.default_rng(5)
    ct, keys, crs = S.rotate_case(ks, plan, level, 2, rng, H)
    for rot in (1, 5):
        gal = pow(5, rot, 2 * ks.N)
        out = ks.rotate(level, gal, [0, 1], ct, keys, crs)
        for n in plan.zero_positions():
            dst = (n * gal) & (ks.N - 1)
            want = [0] * (level + 1) if n == plan.control else ks.Q[: level + 1]
            assert S.flips(n, gal, ks.logN) == (n != plan.control)
            assert [int(x) for x in out[0][:, dst]] == want and [int(x) for x in out[2][:, dst]] == want, (rot, n)
