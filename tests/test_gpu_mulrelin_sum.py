"""mkhe_mul_relin_sum (-m gpu): K products under one relinearisation tail, bit for bit against the model of tests/mulrelin_sum_model.py (the definition
written with the oracle's own pieces) on uniform material: id shapes, K = 1 .. 16, levels, the rescale, caller-supplied hoisted forms, the order of the
pairs, each ring's own launch set (N = 2^14: staged digits; N = 2^15: the F2 products out of the Decompose NTT), the state it leaves, the errors."""
import ctypes as C

import numpy as np
import pytest

import harness as H
import mulrelin_sum_model as M
from gpu_common import Pair, oracle_mul_and_relin

pytestmark = pytest.mark.gpu

NAMES = ["p1", "p2", "p3", "p4"]


class World:
    def __init__(self, pset, seed=3):
        from mkhe_kklss_amd._abi import handle_array, lib
        self.pair = Pair(pset, seed=seed)
        self.lib, self.handle_array = lib(), handle_array
        self.mk, self.params, self.ks, self.rng = self.pair.mk, self.pair.params, self.pair.ks, self.pair.rng
        for n in NAMES:
            self.params.party_index(n)
        self.rlk_h, self.rlk_d = self.pair.rlk_set(NAMES)
        self.u_h = H.uniform_swk(self.rng, self.ks)
        self.params.AddCRS(-1, self.u_h)
        self.top = self.pair.maxlevel

    def cts(self, ids, K, limbs, fill=None):
        hosts = []
        for _ in range(K):
            h = H.uniform_ct(self.rng, self.ks, len(ids), limbs)
            if fill is not None:
                for l in range(limbs):
                    h[:, l, :] = np.uint64(fill(self.pair.Q[l]))
            hosts.append(h)
        return hosts, [self.mk.NewCiphertext(self.params, ids, limbs - 1).upload(h) for h in hosts]

    def hoist(self, level, cts):
        """flat [k * n + a] handles of mkhe_hoisted_form at `level` (kept alive by the returned keys)"""
        keys = []
        for c in cts:
            ks = [self.mk.NewSwitchingKey(self.params) for _ in c.ids]
            assert self.lib.mkhe_hoisted_form(self.params.ctx, level, c.h, self.handle_array([k.h for k in ks])) == 0, self.error()
            keys += ks
        return keys

    def call(self, d0, d1, out, rescale=0, h0=None, h1=None, K=None, rlk=None, out_h=None):
        ha = self.handle_array
        ids0, ids1 = d0[0].ids, d1[0].ids
        g = lambda i, j: (rlk or self.rlk_d).GetRelinearizationKey(i).Value[j].h
        return self.lib.mkhe_mul_relin_sum(self.params.ctx, len(d0) if K is None else K, ha([c.h for c in d0]), ha([c.h for c in d1]),
                                           ha([k.h for k in h0]) if h0 is not None else None, ha([k.h for k in h1]) if h1 is not None else None,
                                           ha([g(i, 0) for i in ids1]), ha([g(i, 1) for i in ids0]), ha([g(i, 2) for i in ids0]),
                                           self.params.CRS[-1].h, rescale, out.h if out_h is None else out_h)

    def model(self, level, ids0, hosts0, ids1, hosts1):
        idx = {n: k for k, n in enumerate(NAMES)}
        rl = {idx[n]: self.rlk_h[n] for n in NAMES}
        ido, out = M.mul_relin_sum(self.ks, level, [idx[i] for i in ids0], hosts0, [idx[i] for i in ids1], hosts1, rl, self.u_h)
        return [NAMES[i] for i in ido], out

    def error(self):
        return self.lib.mkhe_last_error().decode()


@pytest.fixture(scope="module")
def w():
    return World(H.small_ckks(10, 4))


def names(ids):
    return ["p%d" % i for i in ids]


def run(w, ids0, ids1, K, level=None, limbs=None, fill=None):
    level = w.top if level is None else level
    limbs = level + 1 if limbs is None else limbs
    ids0, ids1 = names(ids0), names(ids1)
    h0, d0 = w.cts(ids0, K, limbs, fill)
    h1, d1 = w.cts(ids1, K, limbs, fill)
    out = w.mk.NewCiphertext(w.params, set(ids0) | set(ids1), level)
    assert w.call(d0, d1, out) == 0, w.error()
    ido, ref = w.model(level, ids0, h0, ids1, h1)
    got = out.download()
    assert ido == out.ids and got.shape == ref.shape and (got == ref).all()
    return (h0, d0, h1, d1), out, got


@pytest.mark.parametrize("ids0,ids1,K", [([1], [2], 2), ([1, 2], [1, 2], 2), ([1, 2], [2, 3], 2), ([1, 2, 3, 4], [1, 2, 3, 4], 2),
                                         ([1, 2], [1, 2], 4), ([1, 2], [2, 3], 5), ([1, 2], [1, 2], 9), ([2, 3], [1], 4)])
def test_matches_the_model(w, ids0, ids1, K):
    run(w, ids0, ids1, K)


@pytest.mark.parametrize("ids0,ids1", [([1], [2]), ([1, 2], [1, 2]), ([1, 2], [2, 3]), ([1, 2, 3, 4], [1, 2, 3, 4])])
def test_one_pair_is_mul_and_relin(w, ids0, ids1):
    (h0, d0, h1, d1), out, got = run(w, ids0, ids1, 1)
    ref = w.mk.NewCiphertext(w.params, out.ids, w.top)
    w.pair.ksw.MulAndRelin(d0[0], d1[0], w.rlk_d, ref)
    assert (ref.download() == got).all()


def test_sixteen_pairs_of_residues_q_minus_one(w):
    """the worst case of the tensor accumulator: 32 products of (q - 1)^2 per output word of a slot that both operands carry"""
    run(w, [1, 2], [1, 2], 16, fill=lambda q: q - 1)
    run(w, [1], [2], 16)


@pytest.mark.parametrize("ids0,ids1", [([1, 2], [2, 3]), ([1], [2])])
def test_level_one_with_operands_that_keep_more_limbs(w, ids0, ids1):
    run(w, ids0, ids1, 2, level=1, limbs=4)
    run(w, ids0, ids1, 3, level=0, limbs=2)


@pytest.mark.parametrize("ids0,ids1,K,level", [([1, 2], [2, 3], 3, None), ([1, 2], [1, 2], 2, 2), ([1], [2], 5, None)])
def test_rescale_is_mkhe_rescale_of_the_product(w, ids0, ids1, K, level):
    level = w.top if level is None else level
    (h0, d0, h1, d1), out, got = run(w, ids0, ids1, K, level=level, limbs=w.top + 1)
    two = w.mk.NewCiphertext(w.params, out.ids, level - 1)
    assert w.lib.mkhe_rescale(w.params.ctx, out.h, 1, two.h) == 0, w.error()
    one = w.mk.NewCiphertext(w.params, out.ids, level - 1)
    assert w.call(d0, d1, one, rescale=1) == 0, w.error()
    assert (one.download() == two.download()).all()
    ref = np.stack([w.ks.ringQ.div_round_last_many(got[s], 1)[0] for s in range(got.shape[0])])
    assert (one.download() == ref).all()


@pytest.mark.parametrize("ids0,ids1,level", [([1, 2], [2, 3], None), ([1, 2, 3, 4], [1, 2, 3, 4], None), ([1], [2], 1)])
def test_hoisted_forms_on_both_sides_one_side_or_neither(w, ids0, ids1, level):
    level = w.top if level is None else level
    (h0, d0, h1, d1), out, got = run(w, ids0, ids1, 3, level=level, limbs=w.top + 1)
    f0, f1 = w.hoist(level, d0), w.hoist(level, d1)
    for a, b in ((f0, f1), (f0, None), (None, f1)):
        again = w.mk.NewCiphertext(w.params, out.ids, level)
        assert w.call(d0, d1, again, h0=a, h1=b) == 0, w.error()
        assert (again.download() == got).all(), (a is not None, b is not None)


def test_order_of_the_pairs(w):
    (h0, d0, h1, d1), out, got = run(w, [1, 2], [2, 3], 5)
    perm = [3, 0, 4, 2, 1]
    again = w.mk.NewCiphertext(w.params, out.ids, w.top)
    assert w.call([d0[k] for k in perm], [d1[k] for k in perm], again) == 0, w.error()
    assert (again.download() == got).all()


def test_one_ciphertext_squared_and_summed(w):
    """op0[k] is op1[k]: the engine hoists the operand once"""
    ids = names([1, 2])
    h, d = w.cts(ids, 2, w.top + 1)
    out = w.mk.NewCiphertext(w.params, ids, w.top)
    assert w.call(d, d, out) == 0, w.error()
    _, ref = w.model(w.top, ids, h, ids, h)
    assert (out.download() == ref).all()


def test_alpha_two_decomposer():
    """small_alpha2: four special primes, two limbs per digit -- the engine's own hoisting goes through the CRT-reconstruction spread"""
    world = World(H.small_alpha2(10, 5), seed=8)
    try:
        run(world, [1, 2], [2, 3], 3)
        run(world, [1], [1], 2, level=2, limbs=5)
    finally:
        world.params.close()


def _launches(world, fn):
    L = world.lib
    ncls = L.mkhe_prof_nclass()
    ms, cnt, byt = (C.c_double * ncls)(), (C.c_long * ncls)(), (C.c_double * ncls)()
    assert L.mkhe_prof_enable(world.params.ctx, 1) == 0
    fn()
    assert L.mkhe_prof_collect(world.params.ctx, ms, cnt, byt) == 0
    assert L.mkhe_prof_enable(world.params.ctx, 0) == 0
    return {L.mkhe_prof_name(i).decode(): cnt[i] for i in range(ncls)}


@pytest.mark.parametrize("logN,nq,ids0,ids1", [(14, 3, [1], [2]), (15, 2, [1], [2]), (14, 3, [1], [1]), (15, 2, [1], [1])])
def test_larger_rings_take_their_own_tail(logN, nq, ids0, ids1):
    """N = 2^14: small_ckks(14, 3).  N = 2^15: f2_fused_ok refuses one party of op0 at three limbs (30 passes: no cut within F2_SLACK of an even deal)
    and accepts it at two (mkhe_f2_schedule_probe(1, 2, 4): 16 workgroups, two parts) -- small_ckks(15, 2) is the smallest shape that goes through
    ntt16_f2_kernel.  ids ([1], [1]): the F2 product with u accumulates onto a slot that step E has written (no tensor term rides on it), at N = 2^15
    with products that arrive in parts.  The hoisted forms are the caller's, so the only Decompose of the call is that of the t_i, and the launch counts
    say which tail ran: N = 2^15 ONE ntt16_f2_kernel launch and no Decompose launch at all; N = 2^14 ONE launch of the cross stages alone (the staged
    digits: class ntt_fwd_kernel<N,1,true>), where the full Decompose of this prime chain would show a launch of the big-modulus class or of the
    16-coefficient kernel."""
    world = World(H.small_ckks(logN, nq), seed=logN)
    try:
        ids0, ids1 = names(ids0), names(ids1)
        h0, d0 = world.cts(ids0, 2, nq)
        h1, d1 = world.cts(ids1, 2, nq)
        f0, f1 = world.hoist(nq - 1, d0), world.hoist(nq - 1, d1)
        out = world.mk.NewCiphertext(world.params, set(ids0) | set(ids1), nq - 1)
        counts = _launches(world, lambda: world.call(d0, d1, out, h0=f0, h1=f1))
        _, ref = world.model(nq - 1, ids0, h0, ids1, h1)
        assert (out.download() == ref).all()
        f2 = sum(v for k, v in counts.items() if k.startswith("ntt16_f2_kernel"))
        decomp = {k: v for k, v in counts.items() if "Decompose" in k and not k.startswith("ntt16_f2_kernel") and v}
        print("logN=%d launches: %r" % (logN, {k: v for k, v in counts.items() if v}))
        if logN == 15:
            assert f2 == 1 and not decomp, counts
        else:
            assert f2 == 0 and list(decomp.values()) == [1] and next(iter(decomp)).startswith("ntt_fwd_kernel<N,1,true>"), counts
        assert counts["tensor_kernel"] == 1, counts
        # and with the engine hoisting: the same bits
        again = world.mk.NewCiphertext(world.params, out.ids, nq - 1)
        assert world.call(d0, d1, again) == 0, world.error()
        assert (again.download() == ref).all()
    finally:
        world.params.close()


def test_the_plan_is_not_left_behind(w):
    """after a call, mkhe_mul_and_relin and mkhe_mul_relin_rescale on the same context still match the oracle"""
    (h0, d0, h1, d1), out, _ = run(w, [1, 2], [2, 3], 3)
    ido, ref = oracle_mul_and_relin(w.pair, w.top, d0[1].ids, h0[1], d1[1].ids, h1[1], w.rlk_h, w.u_h, NAMES)
    plain = w.mk.NewCiphertext(w.params, ido, w.top)
    w.pair.ksw.MulAndRelin(d0[1], d1[1], w.rlk_d, plain)
    assert (plain.download() == ref).all()
    run(w, [1, 2], [1, 2], 2)
    res = w.mk.NewCiphertext(w.params, ido, w.top - 1)
    w.pair.ksw.MulAndRelinHoisted(d0[1], d1[1], None, None, w.rlk_d, res, rescaled=True)
    assert (res.download() == np.stack([w.ks.ringQ.div_round_last_many(ref[s], 1)[0] for s in range(ref.shape[0])])).all()


def test_errors_name_the_function(w):
    ids0, ids1 = names([1, 2]), names([2, 3])
    _, d0 = w.cts(ids0, 2, w.top + 1)
    _, d1 = w.cts(ids1, 2, w.top + 1)
    out = w.mk.NewCiphertext(w.params, set(ids0) | set(ids1), w.top)

    def refused(rc, words):
        assert rc != 0
        msg = w.error()
        assert msg.startswith("mkhe_mul_relin_sum"), msg
        assert words in msg, msg

    refused(w.call(d0, d1, out, K=0), "1 to 16")
    big0, big1 = d0 * 9, d1 * 9
    refused(w.call(big0[:17], big1[:17], out), "1 to 16")
    _, other = w.cts(names([1, 3]), 1, w.top + 1)
    refused(w.call([d0[0], other[0]], d1, out), "ids of the first")
    refused(w.call(d0, [d1[0], other[0]], out), "ids of the first")
    refused(w.call(d0, d1, out, out_h=d0[1].h), "distinct")
    refused(w.call(d0, d1, out, out_h=d1[0].h), "distinct")
    _, short = w.cts(ids0, 2, w.top)
    refused(w.call(short, d1, out), "fewer limbs")
    low = w.mk.NewCiphertext(w.params, set(ids0) | set(ids1), w.top)
    refused(w.call(d0, d1, low, rescale=1), "Rescale")
    refused(w.call(d0, d1, out, rescale=2), "0 or 1")
    wrong = w.mk.NewCiphertext(w.params, names([1, 2]), w.top)
    refused(w.call(d0, d1, wrong), "lacks an id")

    class NullKey:
        def __init__(self, inner):
            self.inner = inner

        def GetRelinearizationKey(self, i):
            k = self.inner.GetRelinearizationKey(i)
            if i != "p2":
                return k
            return type("K", (), {"Value": [k.Value[0], type("S", (), {"h": None})(), k.Value[2]]})()

    refused(w.call(d0, d1, out, rlk=NullKey(w.rlk_d)), "null handle")
    refused(w.lib.mkhe_mul_relin_sum(w.params.ctx, 2, w.handle_array([c.h for c in d0]), w.handle_array([c.h for c in d1]), None, None,
                                     None, None, None, w.params.CRS[-1].h, 0, out.h), "null argument")
    f0 = w.hoist(w.top, d0)
    refused(w.lib.mkhe_mul_relin_sum(w.params.ctx, 2, w.handle_array([c.h for c in d0]), w.handle_array([c.h for c in d1]),
                                     w.handle_array([f0[0].h, None, f0[2].h, f0[3].h]), None,
                                     w.handle_array([w.rlk_d.GetRelinearizationKey(i).Value[0].h for i in ids1]),
                                     w.handle_array([w.rlk_d.GetRelinearizationKey(i).Value[1].h for i in ids0]),
                                     w.handle_array([w.rlk_d.GetRelinearizationKey(i).Value[2].h for i in ids0]),
                                     w.params.CRS[-1].h, 0, out.h), "null handle in hoist0")
    # a context that owns a subset of the moduli
    mtot = len(w.pair.Q) + len(w.pair.P)
    own = (C.c_int * 3)(0, 2, mtot - 1)
    assert w.lib.mkhe_ctx_set_owned(w.params.ctx, own, 3) == 0
    try:
        refused(w.call(d0, d1, out), "subset of the moduli")
    finally:
        assert w.lib.mkhe_ctx_set_owned(w.params.ctx, own, 0) == 0
    # and the context still works
    assert w.call(d0, d1, out) == 0, w.error()


def test_a_bfv_context_is_refused():
    import harness_bfv as HB
    from mkhe_kklss_amd import mkbfv, mkrlwe
    from mkhe_kklss_amd._abi import handle_array, lib
    pset = HB.small_bfv(10)
    params = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], pset["T"])
    try:
        ct = mkrlwe.NewCiphertext(params, ["a"], len(pset["Q"]) - 1)
        out = mkrlwe.NewCiphertext(params, ["a"], len(pset["Q"]) - 1)
        key = mkrlwe.NewSwitchingKey(params)
        one = handle_array([key.h])
        rc = lib().mkhe_mul_relin_sum(params.ctx, 1, handle_array([ct.h]), handle_array([ct.h]), None, None, one, one, one, key.h, 0, out.h)
        msg = lib().mkhe_last_error().decode()
        assert rc != 0 and msg.startswith("mkhe_mul_relin_sum") and "CKKS" in msg, msg
    finally:
        params.close()
