"""mkhe_ct_lincomb (-m gpu): out = sum_k (re_k + i im_k) in[k] + (add_re + i add_im) with i = X^(N/2), optionally divided by the last modulus, bit for bit
against a model in Python integers written here from the formulas of include/mkhe.h and the rounding rule of DivRoundByLastModulus
(round(x / q_top) = (x + h - ((x + h) mod q_top)) / q_top, h = (q_top - 1) / 2, limb by limb), against mkhe_rescale, and against the chain of
mkhe_ct_mul_const and mkhe_ct_sum that it replaces.  Weights and constants are independent uniform residues per limb: the kernel treats limbs
independently, no encoding is involved at this level."""
import os
import subprocess
import sys

import numpy as np
import pytest

import harness as H

pytestmark = pytest.mark.gpu

CAP = 16                      # CTLIN_MAX of csrc/poly_kernels.h
R = 1 << 64


class World:
    def __init__(self, pset):
        from mkhe_kklss_amd import mkrlwe
        from mkhe_kklss_amd._abi import handle_array, lib
        self.mk, self.lib, self.handle_array = mkrlwe, lib(), handle_array
        self.Q, self.N = pset["Q"], 1 << pset["logN"]
        self.params = mkrlwe.Parameters(pset["logN"], pset["Q"], pset["P"], 2)

    def ct(self, host, ids):
        return self.mk.NewCiphertext(self.params, ids, host.shape[1] - 1).upload(host)

    def new(self, ids, limbs):
        return self.mk.NewCiphertext(self.params, ids, limbs - 1)

    def consts(self, add, weights, Lc):
        """add = (re[l], im[l]) plain; weights = [(re[l], im[l])] plain -> the device block [n + 1][2][Lc], rows 1 .. n in Montgomery form"""
        rows = [[add[0], add[1]]] + [[[w * R % q for w, q in zip(part, self.Q)] for part in (re, im)] for re, im in weights]
        arr = np.array([[[int(v) for v in part[:Lc]] for part in row] for row in rows], dtype=np.uint64)
        assert arr.shape == (len(weights) + 1, 2, Lc)
        buf = self.mk.DeviceLimbs(self.params, 1, -(-arr.size // self.N))
        return buf.upload(np.concatenate([arr.ravel(), np.zeros(buf.words - arr.size, dtype=np.uint64)]).reshape(1, buf.limbs, self.N))

    def lincomb(self, ins, consts, nb, out):
        return self.lib.mkhe_ct_lincomb(self.params.ctx, len(ins), self.handle_array([c.h for c in ins]), consts.devptr(), nb, out.h)

    def error(self):
        return self.lib.mkhe_last_error().decode()


@pytest.fixture(scope="module")
def worlds():
    return {logN: World(H.small_ckks(logN, nq=6)) for logN in (10, 12)}


def model(Q, hosts, add, weights, Lc, nb):
    """hosts: uint64 [polys][limbs >= Lc][N] each -> uint64 [polys][Lc - nb][N]"""
    P, N = hosts[0].shape[0], hosts[0].shape[2]
    h = N // 2
    acc = []
    for l in range(Lc):
        q, a = Q[l], np.zeros((P, N), dtype=object)
        for x, (re, im) in zip(hosts, weights):
            x = x[:, l, :].astype(object)
            a[:, :h] += int(re[l]) * x[:, :h] - int(im[l]) * x[:, h:]
            a[:, h:] += int(re[l]) * x[:, h:] + int(im[l]) * x[:, :h]
        a[0, 0] += int(add[0][l])
        a[0, h] += int(add[1][l])
        acc.append(a % q)
    if nb:
        qt = Q[Lc - 1]
        half = (qt - 1) >> 1
        t = (acc[Lc - 1] + half) % qt
        acc = [(acc[l] + half - t) * pow(qt, -1, Q[l]) % Q[l] for l in range(Lc - 1)]
    return np.stack([a.astype(np.uint64) for a in acc], axis=1)


def draw(rng, Q, N, n, polys, limbs, Lc, real_only=False):
    hosts = [np.stack([H.uniform_poly(rng, Q[:limbs], N) for _ in range(polys)]) for _ in range(n)]
    res = lambda: [int(rng.integers(0, q)) for q in Q[:Lc]]
    weights = [(res(), [0] * Lc if real_only else res()) for _ in range(n)]
    return hosts, (res(), res()), weights


def check(w, hosts, add, weights, Lc, nb, ids):
    ins = [w.ct(x, ids) for x in hosts]
    out = w.new(ids, Lc - nb)
    assert w.lincomb(ins, w.consts(add, weights, Lc), nb, out) == 0, w.error()
    got, ref = out.download(), model(w.Q, hosts, add, weights, Lc, nb)
    assert got.shape == ref.shape and (got == ref).all()
    return ins, got


@pytest.mark.parametrize("Lc,nb", [(1, 0), (2, 0), (2, 1), (4, 0), (4, 1)])          # (one limb cannot be rescaled: test_errors)
@pytest.mark.parametrize("n", [1, 2, 7, CAP])
@pytest.mark.parametrize("parties", [1, 3])
@pytest.mark.parametrize("logN", [10, 12])
def test_basic_shapes(worlds, logN, parties, n, Lc, nb):
    w = worlds[logN]
    rng = np.random.default_rng([logN, parties, n, Lc, nb])
    hosts, add, weights = draw(rng, w.Q, w.N, n, 1 + parties, Lc, Lc)
    check(w, hosts, add, weights, Lc, nb, ["p%d" % i for i in range(parties)])


@pytest.mark.parametrize("nb", [0, 1])
def test_constant_variants(worlds, nb):
    w, Lc, ids = worlds[10], 3, ["p0", "p1"]
    rng = np.random.default_rng(5 + nb)
    zero = [0] * Lc
    # real weights only, with and without the constant
    hosts, add, weights = draw(rng, w.Q, w.N, 3, 3, Lc, Lc, real_only=True)
    check(w, hosts, add, weights, Lc, nb, ids)
    check(w, hosts, (zero, zero), weights, Lc, nb, ids)
    # complex weights; a purely imaginary one: i * x is the negacyclic shift by N/2
    hosts, add, weights = draw(rng, w.Q, w.N, 3, 3, Lc, Lc)
    weights[1] = (zero, weights[1][1])
    check(w, hosts, add, weights, Lc, nb, ids)
    if not nb:
        _, got = check(w, hosts[:1], (zero, zero), [(zero, [1] * Lc)], Lc, 0, ids)
        x, h = hosts[0], w.N // 2
        q = np.array(w.Q[:Lc], dtype=np.uint64)[None, :, None]
        assert (got[..., h:] == x[..., :h]).all() and (got[..., :h] == (q - x[..., h:]) % q).all()
    # the additive constant alone: weights = MForm(1), n = 1 -- the ciphertext comes back with two coefficients of polynomial 0 moved
    hosts, add, _ = draw(rng, w.Q, w.N, 1, 3, Lc, Lc)
    _, got = check(w, hosts, add, [([1] * Lc, zero)], Lc, nb, ids)
    if not nb:
        want, h = hosts[0].copy(), w.N // 2
        for l in range(Lc):
            want[0, l, 0] = (int(want[0, l, 0]) + add[0][l]) % w.Q[l]
            want[0, l, h] = (int(want[0, l, h]) + add[1][l]) % w.Q[l]
        assert (got == want).all()


@pytest.mark.parametrize("nb", [0, 1])
def test_inputs_two_limbs_above_the_sum(worlds, nb):
    w, Lc = worlds[10], 3
    rng = np.random.default_rng(77 + nb)
    hosts, add, weights = draw(rng, w.Q, w.N, 3, 3, Lc + 2, Lc)
    check(w, hosts, add, weights, Lc, nb, ["p0", "p1"])
    # and summands at different levels
    hosts[1] = hosts[1][:, :Lc]
    hosts[2] = hosts[2][:, : Lc + 1]
    check(w, hosts, add, weights, Lc, nb, ["p0", "p1"])


@pytest.mark.parametrize("nb", [0, 1])
def test_worst_case_accumulation(nb):
    """n = cap, every residue, weight and constant q - 1, over the 60-bit prime of PN15QP880 and one 54-bit prime: 2 * cap products of (q - 1)^2 in the
    sum of the upper half of every pair -- the largest value the kernel's accumulator can be asked to hold"""
    pset = H.small_ckks(10, nq=2)
    assert pset["Q"][0].bit_length() == 60 and pset["Q"][1].bit_length() == 54
    w, Lc = World(pset), 2
    host = np.stack([np.stack([np.full(w.N, q - 1, dtype=np.uint64) for q in w.Q]) for _ in range(3)])
    top = [q - 1 for q in w.Q]
    check(w, [host] * CAP, (top, top), [(top, top)] * CAP, Lc, nb, ["p0", "p1"])
    if not nb:
        check(w, [host[:, :1]] * CAP, (top[:1], top[:1]), [(top[:1], top[:1])] * CAP, 1, 0, ["p0", "p1"])


def test_fused_rescale_equals_lincomb_then_rescale(worlds):
    w, Lc, ids = worlds[12], 4, ["p0", "p1", "p2"]
    rng = np.random.default_rng(404)
    hosts, add, weights = draw(rng, w.Q, w.N, 7, 4, Lc, Lc)
    ins, consts = [w.ct(x, ids) for x in hosts], w.consts(add, weights, Lc)
    fused, tmp, two = w.new(ids, Lc - 1), w.new(ids, Lc), w.new(ids, Lc - 1)
    assert w.lincomb(ins, consts, 1, fused) == 0, w.error()
    assert w.lincomb(ins, consts, 0, tmp) == 0, w.error()
    assert w.lib.mkhe_rescale(w.params.ctx, tmp.h, 1, two.h) == 0, w.error()
    assert (fused.download() == two.download()).all()


def test_equals_the_chain_of_mul_const_and_sum(worlds):
    from mkhe_kklss_amd import _abi
    w, Lc, ids = worlds[12], 4, ["p0", "p1", "p2"]
    rng = np.random.default_rng(505)
    hosts, _, weights = draw(rng, w.Q, w.N, 7, 4, Lc, Lc, real_only=True)
    zero = [0] * Lc
    ins, out = [w.ct(x, ids) for x in hosts], w.new(ids, Lc)
    assert w.lincomb(ins, w.consts((zero, zero), weights, Lc), 0, out) == 0, w.error()
    prods = []
    for c, (re, _) in zip(ins, weights):
        m = np.array([v * R % q for v, q in zip(re, w.Q)], dtype=np.uint64)
        prods.append(w.new(ids, Lc))
        assert w.lib.mkhe_ct_mul_const(w.params.ctx, c.h, m.ctypes.data_as(_abi.u64p), m.ctypes.data_as(_abi.u64p), prods[-1].h) == 0, w.error()
    chain = w.new(ids, Lc)
    assert w.lib.mkhe_ct_sum(w.params.ctx, len(prods), w.handle_array([p.h for p in prods]), chain.h) == 0, w.error()
    assert (out.download() == chain.download()).all()


def test_errors(worlds):
    w, Lc, ids = worlds[10], 2, ["p0", "p1"]
    rng = np.random.default_rng(606)
    hosts, add, weights = draw(rng, w.Q, w.N, 2, 3, Lc, Lc)
    ins, consts = [w.ct(x, ids) for x in hosts], w.consts(add, weights, Lc)
    out = w.new(ids, Lc)
    sentinel = np.stack([H.uniform_poly(rng, w.Q[:Lc], w.N) for _ in range(3)])
    out.upload(sentinel)
    harr, ctx = w.handle_array([c.h for c in ins]), w.params.ctx

    def refused(rc):
        assert rc != 0 and w.error(), "accepted"
        return w.error()

    refused(w.lib.mkhe_ct_lincomb(ctx, 0, harr, consts.devptr(), 0, out.h))                       # n < 1
    many = [ins[0]] * (CAP + 1)
    big = w.consts(add, [weights[0]] * (CAP + 1), Lc)
    refused(w.lincomb(many, big, 0, out))                                                          # n above the cap
    other = w.ct(hosts[0], ["p0", "p2"])
    refused(w.lincomb([ins[0], other], consts, 0, out))                                            # id sets differ among the inputs
    refused(w.lincomb(ins, consts, 0, w.new(["p0"], Lc)))                                          # ... and with out
    refused(w.lincomb(ins, consts, 0, w.new(ids, Lc + 1)))                                         # an input with fewer than Lc limbs
    refused(w.lincomb(ins, consts, 1, out))                                                        # the same through the rescale: Lc = limbs(out) + 1
    for nb in (-1, 2):
        refused(w.lincomb(ins, consts, nb, out))                                                   # nb_rescale outside {0, 1}
    low = [w.ct(x[:, :1], ids) for x in hosts]
    refused(w.lincomb(low, consts, 1, w.new(ids, 1)))                                              # nb_rescale = 1 with nothing below the summands' only limb
    refused(w.lincomb([ins[0], out], consts, 0, out))                                              # out aliases an input
    refused(w.lincomb([out], consts, 0, out))
    assert "null context" in refused(w.lib.mkhe_ct_lincomb(None, 2, harr, consts.devptr(), 0, out.h))
    refused(w.lib.mkhe_ct_lincomb(ctx, 2, None, consts.devptr(), 0, out.h))                        # null arguments
    refused(w.lib.mkhe_ct_lincomb(ctx, 2, harr, None, 0, out.h))
    refused(w.lib.mkhe_ct_lincomb(ctx, 2, harr, consts.devptr(), 0, None))
    refused(w.lib.mkhe_ct_lincomb(ctx, 2, w.handle_array([ins[0].h, None]), consts.devptr(), 0, out.h))
    # nothing was launched: out still holds what was uploaded; and the context still works
    assert (out.download() == sentinel).all()
    assert w.lincomb(ins, consts, 0, out) == 0, w.error()
    assert (out.download() == model(w.Q, hosts, add, weights, Lc, 0)).all()


def test_inside_a_captured_graph():
    """mkhe_capture_begin / mkhe_ct_lincomb / mkhe_capture_end / mkhe_graph_launch against the eager call, in a fresh interpreter: a process that has
    imported torch is bound to a HIP runtime in which mkhe_capture_begin refuses to capture (tests/test_gpu_cnn.py)"""
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, os.path.join(here, "lincomb_graph_check.py")], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and "graph replay ok" in out.stdout


@pytest.mark.parametrize("nb", [0, 1])
def test_more_limbs_than_limb_groups(nb):
    """N = 2^15 with four polynomials is the smallest shape at which the launch makes fewer limb groups (four) than output limbs, so that one thread
    walks several limbs: the loop that every smaller shape runs exactly once"""
    w, Lc, ids = World(H.small_ckks(15, nq=6)), 6, ["p0", "p1", "p2"]
    rng = np.random.default_rng(1500 + nb)
    hosts, add, weights = draw(rng, w.Q, w.N, 2, 4, Lc, Lc)
    check(w, hosts, add, weights, Lc, nb, ids)
