"""mkhe_bfv_mul_relin_sum (-m gpu): K MK-BFV products under one Quantize and one relinearisation tail, bit for bit against the model of
tests/bfv_mulrelin_sum_model.py (the definition written with the oracle's own pieces) on uniform material: id shapes, K = 1 .. 16, the 55-bit tail
primes, the full 14 + 14 + 2 chain, the order of the pairs, N = 2^15 (the F2 products out of the Decompose NTT of a summed t_i), the state it
leaves, the refusals."""
import ctypes as C

import numpy as np
import pytest

import bfv_mulrelin_sum_model as M
import harness as H
import harness_bfv as HB

pytestmark = pytest.mark.gpu

NAMES = ["p1", "p2", "p3", "p4", "p5"]
IDX = {n: k for k, n in enumerate(NAMES)}
ID_SHAPES = [([1], [2]), ([1, 2], [1, 2]), ([1, 2], [2, 3]), ([1, 2, 3, 4], [1, 2, 3, 4])]


class World:
    """uniform material in the BfvPair style of tests/test_gpu_bfv.py: relinearisation keys of the parties and the CRS u, host and device"""

    def __init__(self, pset, seed=5, parties=4):
        from mkhe_kklss_amd import mkbfv, mkrlwe
        from mkhe_kklss_amd._abi import handle_array, lib
        self.mk, self.mkb, self.lib, self.handle_array = mkrlwe, mkbfv, lib(), handle_array
        self.pset, self.bfv = pset, HB.make_bfv(pset)
        self.params = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], pset["T"])
        self.ev = mkbfv.NewEvaluator(self.params)
        self.rng = np.random.default_rng(seed)
        self.N, self.nq, self.Q = 1 << pset["logN"], len(pset["Q"]), pset["Q"]
        self.names = NAMES[:parties]
        for n in self.names:
            self.params.party_index(n)
        self.rlk_h, self.rlk_d = {}, mkbfv.NewRelinearizationKeyKeySet(self.params)
        for n in self.names:
            ks = tuple(H.uniform_swk(self.rng, self.bfv.ks) for _ in range(5))
            self.rlk_h[n] = ks
            self.rlk_d.AddRelinearizationKey(mkbfv.RelinearizationKey(self.params, n, *ks))
        self.u_h = H.uniform_swk(self.rng, self.bfv.ks)
        self.params.AddCRS(-1, self.u_h)

    def cts(self, ids, K, fill=None):
        hosts = []
        for _ in range(K):
            h = H.uniform_ct(self.rng, self.bfv.ks, len(ids), self.nq)
            if fill is not None:
                for l in range(self.nq):
                    h[:, l, :] = np.uint64(fill(self.Q[l]))
            hosts.append(h)
        return hosts, [self.mkb.NewCiphertext(self.params, ids).upload(h) for h in hosts]

    def call(self, d0, d1, out, K=None, rlk=None, out_h=None):
        ha = self.handle_array
        ids0, ids1 = d0[0].ids, d1[0].ids
        key = lambda i, g, j: (rlk or self.rlk_d).GetRelinearizationKey(i).Value[g].Value[j].h
        return self.lib.mkhe_bfv_mul_relin_sum(self.params.ctx, len(d0) if K is None else K, ha([c.h for c in d0]), ha([c.h for c in d1]),
                                               ha([key(i, 0, 0) for i in ids1]), ha([key(i, 1, 0) for i in ids1]),
                                               ha([key(i, 0, 1) for i in ids0]), ha([key(i, 1, 1) for i in ids0]), ha([key(i, 0, 2) for i in ids0]),
                                               self.params.CRS[-1].h, out.h if out_h is None else out_h)

    def rl(self):
        return {IDX[n]: self.rlk_h[n] for n in self.names}

    def model(self, ids0, hosts0, ids1, hosts1):
        ido, out = M.bfv_mul_relin_sum(self.bfv, [IDX[i] for i in ids0], hosts0, [IDX[i] for i in ids1], hosts1, self.rl(), self.u_h)
        return [NAMES[i] for i in ido], out

    def oracle_one(self, ids0, host0, ids1, host1):
        ido, out = self.bfv.mul_relin_new([IDX[i] for i in ids0], host0, [IDX[i] for i in ids1], host1, self.rl(), self.u_h)
        return [NAMES[i] for i in ido], out

    def error(self):
        return self.lib.mkhe_last_error().decode()


@pytest.fixture(scope="module")
def w():
    world = World(HB.small_bfv(10, 3))
    yield world
    world.params.close()


def names(ids):
    return ["p%d" % i for i in ids]


def run(w, ids0, ids1, K, fill=None):
    ids0, ids1 = names(ids0), names(ids1)
    h0, d0 = w.cts(ids0, K, fill)
    h1, d1 = w.cts(ids1, K, fill)
    out = w.mkb.NewCiphertext(w.params, set(ids0) | set(ids1))
    assert w.call(d0, d1, out) == 0, w.error()
    ido, ref = w.model(ids0, h0, ids1, h1)
    got = out.download()
    assert ido == out.ids and got.shape == ref.shape and (got == ref).all()
    for h, d in zip(h0 + h1, d0 + d1):
        assert (d.download() == h).all()           # the operands are unchanged
    return (h0, d0, h1, d1), out, got


@pytest.mark.parametrize("ids0,ids1,K", [(a, b, 2) for a, b in ID_SHAPES] + [([1, 2], [1, 2], 4), ([1, 2], [1, 2], 9), ([2, 3], [1], 5)])
def test_matches_the_model(w, ids0, ids1, K):
    """K = 5 and 9: the chunked loads of the tensor kernel have a last chunk that repeats a pair"""
    run(w, ids0, ids1, K)


@pytest.mark.parametrize("ids0,ids1", [([1, 2, 3, 4, 5], [1, 2]), ([1], [1, 2, 3, 4, 5]), ([1, 2, 3, 4, 5], [1, 2, 3, 4, 5])])
def test_more_parties_than_the_f1_kernel_fuses(ids0, ids1):
    """five parties in op0: x and y come from the inner-product kernel (x on the side stream) and step E is a batch of its own products; five in
    op1 only: x is still the F1 kernel's by-product, y is not computed in it -- the paths bfv_mul_relin takes for these shapes"""
    world = World(HB.small_bfv(10, 2), seed=12, parties=5)
    try:
        run(world, ids0, ids1, 3)
    finally:
        world.params.close()


def test_tail_primes_of_55_bits():
    world = World(HB.small_bfv(12, 4, big=True), seed=6, parties=3)
    try:
        run(world, [1, 2], [2, 3], 3)
    finally:
        world.params.close()


def test_the_full_prime_chain():
    """14 + 14 + 2 primes at a small degree: every ModDown group of the reference chain"""
    world = World(dict(HB.BFV_PN15QP880, logN=11), seed=7, parties=2)
    try:
        run(world, [1, 2], [1, 2], 2)
    finally:
        world.params.close()


@pytest.mark.parametrize("ids0,ids1", ID_SHAPES)
def test_one_pair_is_bfv_mul_relin(w, ids0, ids1):
    (h0, d0, h1, d1), out, got = run(w, ids0, ids1, 1)
    ref = w.ev.MulRelinNew(d0[0], d1[0], w.rlk_d)
    assert ref.ids == out.ids and (ref.download() == got).all()


def test_sixteen_pairs_of_residues_q_minus_one(w):
    """the worst case of the tensor accumulator: every residue of every operand q - 1, K = 16, on slots that both operands carry"""
    run(w, [1, 2], [1, 2], 16, fill=lambda q: q - 1)


def test_order_of_the_pairs(w):
    (h0, d0, h1, d1), out, got = run(w, [1, 2], [2, 3], 5)
    again = w.mkb.NewCiphertext(w.params, out.ids)
    assert w.call(d0[::-1], d1[::-1], again) == 0, w.error()
    assert (again.download() == got).all()


def _launches(world, fn):
    L = world.lib
    ncls = L.mkhe_prof_nclass()
    ms, cnt, byt = (C.c_double * ncls)(), (C.c_long * ncls)(), (C.c_double * ncls)()
    assert L.mkhe_prof_enable(world.params.ctx, 1) == 0
    fn()
    assert L.mkhe_prof_collect(world.params.ctx, ms, cnt, byt) == 0
    assert L.mkhe_prof_enable(world.params.ctx, 0) == 0
    return {L.mkhe_prof_name(i).decode(): cnt[i] for i in range(ncls)}


def test_n_2_15_takes_the_fused_f2_tail():
    """small_bfv(15, 2): two primes in Q and in QMul is the shortest chain for which f2_fused_ok holds with two parties in op0 (the schedule needs
    two digits at least; mkhe_f2_schedule_probe(2, 2, 4, .., -256): 32 workgroups, two parts), so step F2 comes out of the Decompose NTT of the
    summed t_i: ONE ntt16_f2_kernel launch, and ONE tensor launch and ONE Quantize for both pairs."""
    world = World(HB.small_bfv(15, 2), seed=15, parties=2)
    try:
        ids = names([1, 2])
        h0, d0 = world.cts(ids, 2)
        h1, d1 = world.cts(ids, 2)
        out = world.mkb.NewCiphertext(world.params, ids)
        counts = _launches(world, lambda: world.call(d0, d1, out))
        print("launches: %r" % {k: v for k, v in counts.items() if v})
        _, ref = world.model(ids, h0, ids, h1)
        assert (out.download() == ref).all()
        assert sum(v for k, v in counts.items() if k.startswith("ntt16_f2_kernel")) == 1, counts
        assert counts["tensor_kernel"] == 1, counts
    finally:
        world.params.close()


def test_the_plan_and_the_scratch_are_left_clean(w):
    """a mkhe_bfv_mul_relin issued right after the call equals the oracle"""
    (h0, d0, h1, d1), out, _ = run(w, [1, 2], [2, 3], 3)
    ido, ref = w.oracle_one(d0[1].ids, h0[1], d1[1].ids, h1[1])
    plain = w.ev.MulRelinNew(d0[1], d1[1], w.rlk_d)
    assert plain.ids == ido and (plain.download() == ref).all()
    run(w, [1, 2], [1, 2], 2)
    assert (w.ev.MulRelinNew(d0[1], d1[1], w.rlk_d).download() == ref).all()


def test_refusals_name_the_function_and_leave_the_context_usable(w):
    ids0, ids1 = names([1, 2]), names([2, 3])
    h0, d0 = w.cts(ids0, 2)
    h1, d1 = w.cts(ids1, 2)
    out = w.mkb.NewCiphertext(w.params, set(ids0) | set(ids1))
    _, ref = w.model(ids0, h0, ids1, h1)

    def refused(rc, words):
        assert rc != 0
        msg = w.error()
        assert msg.startswith("mkhe_bfv_mul_relin_sum: "), msg
        assert words in msg, msg
        assert w.call(d0, d1, out) == 0, w.error()              # ... and is followed by a call that succeeds
        assert (out.download() == ref).all()

    refused(w.call(d0, d1, out, K=0), "1 to 16")
    refused(w.call((d0 * 9)[:17], (d1 * 9)[:17], out), "1 to 16")
    _, other = w.cts(names([1, 3]), 1)
    refused(w.call([d0[0], other[0]], d1, out), "ids of the first")
    refused(w.call(d0, [d1[0], other[0]], out), "ids of the first")
    refused(w.call(d0, d1, out, out_h=d0[1].h), "distinct")
    refused(w.call(d0, d1, out, out_h=d1[0].h), "distinct")
    refused(w.call(d0, d1, w.mkb.NewCiphertext(w.params, names([1, 2]))), "lacks an id")
    refused(w.call(d0, d1, w.mkb.NewCiphertext(w.params, names([1, 2, 3, 4]))), "neither operand has")

    class NullKey:
        def __init__(self, inner):
            self.inner = inner

        def GetRelinearizationKey(self, i):
            k = self.inner.GetRelinearizationKey(i)
            if i != "p2":
                return k
            null = type("S", (), {"h": None})()
            second = type("K", (), {"Value": [k.Value[1].Value[0], null, None]})()
            return type("R", (), {"Value": [k.Value[0], second]})()

    refused(w.call(d0, d1, out, rlk=NullKey(w.rlk_d)), "null handle in rlk_d2")
    ha = w.handle_array
    refused(w.lib.mkhe_bfv_mul_relin_sum(w.params.ctx, 2, ha([c.h for c in d0]), ha([c.h for c in d1]), None, None, None, None, None,
                                         w.params.CRS[-1].h, out.h), "null argument")
    # a context that owns a subset of the moduli: the engine refuses one ("subset of the moduli"), but no BFV context can be made one through the
    # C ABI -- mkhe_ctx_set_owned itself refuses BFV contexts -- so what can be checked here is that refusal, and that the call still works after it
    own = (C.c_int * 3)(0, 2, len(w.pset["Q"]) + len(w.pset["P"]) - 1)
    assert w.lib.mkhe_ctx_set_owned(w.params.ctx, own, 3) != 0 and "limb sharding" in w.error()
    assert w.call(d0, d1, out) == 0 and (out.download() == ref).all()


def test_a_ckks_context_is_refused():
    from mkhe_kklss_amd import mkckks, mkrlwe
    from mkhe_kklss_amd._abi import handle_array, lib
    pset = H.small_ckks(10, 3)
    params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], pset["scale"])
    try:
        ct = mkrlwe.NewCiphertext(params, ["a"], len(pset["Q"]) - 1)
        out = mkrlwe.NewCiphertext(params, ["a"], len(pset["Q"]) - 1)
        key = mkrlwe.NewSwitchingKey(params)
        one = handle_array([key.h])
        rc = lib().mkhe_bfv_mul_relin_sum(params.ctx, 1, handle_array([ct.h]), handle_array([ct.h]), one, one, one, one, one, key.h, out.h)
        msg = lib().mkhe_last_error().decode()
        assert rc != 0 and msg.startswith("mkhe_bfv_mul_relin_sum: ") and "BFV" in msg, msg
        again = mkrlwe.NewCiphertext(params, ["a"], len(pset["Q"]) - 1)
        assert lib().mkhe_ct_add(params.ctx, ct.h, ct.h, again.h) == 0
    finally:
        params.close()


def test_refused_inside_a_capture_when_the_call_would_allocate():
    """a fresh context has none of the call's scratch (where the runtime of this process can capture at all: tests/test_gpu_cnn.py)"""
    from mkhe_kklss_amd._abi import MkheError
    world = World(HB.small_bfv(10, 2), seed=9, parties=2)
    try:
        ids = names([1, 2])
        h0, d0 = world.cts(ids, 2)
        h1, d1 = world.cts(ids, 2)
        out = world.mkb.NewCiphertext(world.params, ids)
        try:
            with world.params.Capture():
                rc = world.call(d0, d1, out)
                msg = world.error()
            assert rc != 0 and msg.startswith("mkhe_bfv_mul_relin_sum: ") and "capture" in msg, msg
            print("capture: the call that would allocate was refused inside a capture")
        except MkheError as e:
            print("capture: mkhe_capture_begin refused in this process (%s): the refusal inside a capture did not run" % e)
            import gc
            gc.enable()                 # (Graph.__enter__ switched the collector off before the refusal)
            assert "cannot end a multi-stream capture" in str(e)
        assert world.call(d0, d1, out) == 0, world.error()
        _, ref = world.model(ids, h0, ids, h1)
        assert (out.download() == ref).all()
    finally:
        world.params.close()
