"""mkhe_ct_mod_raise (-m gpu) bit for bit against its definition in Python integers: three polynomials (two parties) of uniform level-0 words with
the coefficients 0, (q_0 - 1) / 2, (q_0 + 1) / 2 and q_0 - 1 planted, raised to level 1, level 4 and the top of the first 16 moduli of PN16QP1761
(q_0 has 55 bits, the others 45: the reduction is a real one).  N = 2^10 = one workgroup of 128 rows per polynomial; one more case at N = 2^11
has two, the shape every larger ring extends.  A second ciphertext of the
output's shape, filled with a pattern, must come back untouched.  Then every refusal, by its message, each followed by a call that works."""
import numpy as np
import pytest

import harness as H
import harness_bfv as HB

pytestmark = pytest.mark.gpu

LOGN, N = 10, 1 << 10
Q, P = H.PN16QP1761["Q"][:16], H.PN16_P
SCALE = float(1 << 45)
IDS = ["alice", "bob"]


@pytest.fixture(scope="module")
def w():
    import types
    from mkhe_kklss_amd import mkbfv, mkckks, mkrlwe
    from mkhe_kklss_amd._abi import lib
    params = mkckks.Parameters(LOGN, Q, P, SCALE, logSlots=3)
    small = H.small_ckks(LOGN, nq=4)                                            # one special prime per digit: the only kind mkhe_ctx_set_owned shards
    bset = HB.small_bfv(LOGN, 3)
    world = types.SimpleNamespace(params=params, lib=lib(), mkckks=mkckks, mkrlwe=mkrlwe, sharded=mkckks.Parameters(LOGN, small["Q"], small["P"], small["scale"]),
                                  bfv=mkbfv.Parameters(bset["logN"], bset["Q"], bset["QMul"], bset["P"], bset["T"]))
    yield world
    for p in (world.params, world.sharded, world.bfv):
        p.close()


def level0_words():
    """uint64 [3][1][N]: uniform below q_0, the four planted coefficients at the ends of a row of 8, of a workgroup's share and of the polynomial"""
    rng = np.random.default_rng(550)
    q0 = Q[0]
    x = rng.integers(0, q0, (3, 1, N), dtype=np.uint64)
    planted = [0, (q0 - 1) // 2, (q0 + 1) // 2, q0 - 1]
    for p in range(3):
        for i, n in enumerate([0, 7, 8, N - 1][p:] + [0, 7, 8, N - 1][:p]):
            x[p, 0, n] = planted[i]
        x[p, 0, 500 + p: 504 + p] = planted
    return x


def model(x, limbs):
    """the definition: the centred lift of every word, its canonical residue under q_0 .. q_(limbs-1), in Python integers"""
    q0 = Q[0]
    out = np.empty((x.shape[0], limbs, N), dtype=np.uint64)
    for p in range(x.shape[0]):
        v = [int(c) if int(c) <= (q0 - 1) // 2 else int(c) - q0 for c in x[p, 0]]
        for l in range(limbs):
            out[p, l] = [c % Q[l] for c in v]
    return out


@pytest.fixture(scope="module")
def raised_reference():
    x = level0_words()
    return x, model(x, 16)                                                      # a lower level is its first limbs


@pytest.mark.parametrize("level", [1, 4, 15])
def test_bit_for_bit_against_python_integers(w, raised_reference, level):
    x, ref = raised_reference
    ct = w.mkckks.NewCiphertext(w.params, IDS, 0, SCALE).upload(x)
    guard = np.full((3, level + 1, N), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    out = w.mkckks.NewCiphertext(w.params, IDS, level, SCALE).upload(guard)
    other = w.mkckks.NewCiphertext(w.params, IDS, level, SCALE).upload(guard)
    assert w.lib.mkhe_ct_mod_raise(w.params.ctx, ct.h, out.h) == 0, w.lib.mkhe_last_error().decode()
    got = out.download()
    assert got.shape == (3, level + 1, N) and (got == ref[:, : level + 1]).all()
    assert (got[:, 0] == x[:, 0]).all() and (ct.download() == x).all()          # limb 0 is the input, which is not touched
    assert (other.download() == guard).all()
    res = w.mkckks.NewEvaluator(w.params).ModRaiseNew(ct, level)
    assert res.Level() == level and res.Scale == SCALE and res.ids == IDS and (res.download() == got).all()


def test_two_workgroups_per_polynomial():
    """N = 2^11 is 256 rows of 8: the second workgroup of a polynomial (blockIdx.x = 1) writes coefficients 1024 .. 2047 of every limb.  Uniform
    words with the planted coefficients on both sides of the seam; five limbs."""
    from mkhe_kklss_amd import mkckks
    from mkhe_kklss_amd._abi import lib
    n2, q0, rng = 2 * N, Q[0], np.random.default_rng(551)
    params = mkckks.Parameters(LOGN + 1, Q, P, SCALE)
    try:
        x = rng.integers(0, q0, (3, 1, n2), dtype=np.uint64)
        x[:, 0, N - 2: N + 2] = [0, (q0 - 1) // 2, (q0 + 1) // 2, q0 - 1]
        x[:, 0, n2 - 1] = (q0 + 1) // 2
        ref = np.empty((3, 5, n2), dtype=np.uint64)
        for p in range(3):
            v = [int(c) if int(c) <= (q0 - 1) // 2 else int(c) - q0 for c in x[p, 0]]
            for l in range(5):
                ref[p, l] = [c % Q[l] for c in v]
        ct = mkckks.NewCiphertext(params, IDS, 0, SCALE).upload(x)
        out = mkckks.NewCiphertext(params, IDS, 4, SCALE).upload(np.full((3, 5, n2), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64))
        assert lib().mkhe_ct_mod_raise(params.ctx, ct.h, out.h) == 0, lib().mkhe_last_error().decode()
        got = out.download()
        assert (got[:, :, :N] == ref[:, :, :N]).all() and (got[:, :, N:] == ref[:, :, N:]).all()
    finally:
        params.close()


def test_default_level_is_the_top(w, raised_reference):
    x, ref = raised_reference
    res = w.mkckks.NewEvaluator(w.params).ModRaiseNew(w.mkckks.NewCiphertext(w.params, IDS, 0, SCALE).upload(x))
    assert res.Level() == 15 and (res.download() == ref).all()


def test_refusals_each_followed_by_a_good_call(w, raised_reference):
    x, ref = raised_reference
    new = lambda level, ids=IDS, params=None: w.mkckks.NewCiphertext(params or w.params, ids, level, SCALE)
    ct, out = new(0).upload(x), new(4)

    def call(params, a, b):
        rc = w.lib.mkhe_ct_mod_raise(params.ctx if params is not None else None, None if a is None else a.h, None if b is None else b.h)
        return rc, w.lib.mkhe_last_error().decode() if rc else ""

    def works():
        assert call(w.params, ct, out) == (0, "")
        assert (out.download() == ref[:, :5]).all()

    works()
    name = "mkhe_ct_mod_raise: "
    bct = lambda level: w.mkrlwe.Ciphertext(w.bfv, IDS, level)
    rows = [
        ((None, ct, out), "null context"),
        ((w.params, None, out), "null argument"),
        ((w.params, ct, None), "null argument"),
        ((w.params, new(1), out), "in must be at level 0"),
        ((w.params, ct, new(0)), "out must be above level 0"),
        ((w.params, ct, new(4, ["alice", "carol"])), "in and out must carry the same ids"),
        ((w.params, ct, new(4, ["alice"])), "in and out must carry the same ids"),
        ((w.params, ct, ct), "out must not alias in"),
        ((w.bfv, bct(0), bct(2)), "not available on a BFV context (its ciphertexts live at one level)"),
    ]
    for args, message in rows:
        assert call(*args) == (1, name + message), message
        works()
    import ctypes as C
    own = (C.c_int * 2)(0, 2)
    sct, sout = new(0, params=w.sharded), new(2, params=w.sharded)
    assert w.lib.mkhe_ctx_set_owned(w.sharded.ctx, own, 2) == 0, w.lib.mkhe_last_error().decode()
    try:
        got = call(w.sharded, sct, sout)
    finally:
        assert w.lib.mkhe_ctx_set_owned(w.sharded.ctx, own, 0) == 0
    assert got == (1, name + "not available on a context that owns a subset of the moduli")
    assert call(w.sharded, sct, sout) == (0, "")                                # the same context, whole again
    works()
    with pytest.raises(w.mkckks.MkheError, match="level 0"):
        w.mkckks.NewEvaluator(w.params).ModRaiseNew(new(1))
