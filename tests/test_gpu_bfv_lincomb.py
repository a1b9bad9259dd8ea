"""mkhe_bfv_ct_lincomb (-m gpu): out[g] = sum_b W[g][b] in[b] + C[g] per component and limb mod q_l, C[g] on coefficient 0 of component 0 only, bit for bit
against Python integers written here from the formulas of include/mkhe.h ("BFV weighted sums"), against mkhe_ct_lincomb with real weights and against
the chain of mkhe_ct_mul_const and mkhe_ct_sum.  Ciphertexts, weights and constants are independent uniform residues per limb: the kernel treats limbs
independently, no encoding and no key is involved at this level.  nin = 1, 2, 3, 5, 15, 16 fill the three register layouts (4, 8, 16 slots) partly and
fully."""
import ctypes as C

import numpy as np
import pytest

import harness as H
import harness_bfv as HB

pytestmark = pytest.mark.gpu

NAME = "mkhe_bfv_ct_lincomb"
NAMES = ["user0", "user1", "user2"]
R = 1 << 64


class World:
    def __init__(self, pset):
        from mkhe_kklss_amd import mkbfv, mkrlwe
        from mkhe_kklss_amd._abi import handle_array, lib
        self.mkbfv, self.mk, self.lib, self.handle_array = mkbfv, mkrlwe, lib(), handle_array
        self.Q, self.N, self.nq = pset["Q"], 1 << pset["logN"], len(pset["Q"])
        self.params = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], pset["T"])

    def ct(self, host, ids):
        return self.mkbfv.NewCiphertext(self.params, ids).upload(host)

    def new(self, ids):
        return self.mkbfv.NewCiphertext(self.params, ids)

    def block(self, arr):
        """a uint64 array -> device words (padded to whole limbs)"""
        arr = np.asarray(arr, dtype=np.uint64)
        buf = self.mk.DeviceLimbs(self.params, 1, -(-arr.size // self.N))
        return buf.upload(np.concatenate([arr.ravel(), np.zeros(buf.words - arr.size, dtype=np.uint64)]).reshape(1, buf.limbs, self.N))

    def consts(self, W, Cs):
        """W[g][b][l], Cs[g][l] plain residues -> the device block [nout][nin + 1][nQ]: constants plain, weights in Montgomery form"""
        arr = [[[int(c) for c in Cs[g]]] + [[int(w) * R % q for w, q in zip(W[g][b], self.Q)] for b in range(len(W[g]))] for g in range(len(W))]
        arr = np.array(arr, dtype=np.uint64)
        assert arr.shape == (len(W), len(W[0]) + 1, self.nq)
        return self.block(arr)

    def call(self, ins, consts, outs, nin=None, nout=None, ctx=None):
        h = lambda v: None if v is None else (C.c_void_p * max(1, len(v)))(*[getattr(c, "h", c) for c in v])
        ptr = consts.devptr() if hasattr(consts, "devptr") else consts
        return self.lib.mkhe_bfv_ct_lincomb(self.params.ctx if ctx is None else ctx, len(ins) if nin is None else nin, h(ins),
                                            len(outs) if nout is None else nout, ptr, h(outs))

    def error(self):
        return self.lib.mkhe_last_error().decode()


@pytest.fixture(scope="module")
def world():
    return World(HB.small_bfv(10, 3))


def model(Q, hosts, W, Cs):
    """hosts: uint64 [polys][nQ][N] each -> per output uint64 [polys][nQ][N], in Python integers"""
    xs = [x.astype(object) for x in hosts]
    res = []
    for g in range(len(W)):
        limbs = []
        for l, q in enumerate(Q):
            acc = np.zeros(xs[0][:, l, :].shape, dtype=object)
            for b, x in enumerate(xs):
                if W[g][b][l]:
                    acc = acc + int(W[g][b][l]) * x[:, l, :]
            acc[0, 0] += int(Cs[g][l])
            limbs.append((acc % q).astype(np.uint64))
        res.append(np.stack(limbs, axis=1))
    return res


def draw(rng, w, parties, nin, nout):
    hosts = [H.uniform_ct(rng, w, parties, w.nq) for _ in range(nin)]
    res = lambda: [int(rng.integers(0, q)) for q in w.Q]
    return hosts, [[res() for _ in range(nin)] for _ in range(nout)], [res() for _ in range(nout)]


def check(w, hosts, W, Cs, ids):
    ins = [w.ct(x, ids) for x in hosts]
    outs = [w.new(ids) for _ in W]
    assert w.call(ins, w.consts(W, Cs), outs) == 0, w.error()
    got, ref = [o.download() for o in outs], model(w.Q, hosts, W, Cs)
    for g, (a, b) in enumerate(zip(got, ref)):
        assert a.shape == b.shape and (a == b).all(), "output %d" % g
    for c, x in zip(ins, hosts):
        assert (c.download() == x).all()                        # the inputs are left as they were
    return ins, got


@pytest.mark.parametrize("nin,nout", [(1, 1), (2, 1), (5, 3), (16, 1), (15, 16), (3, 64)])
@pytest.mark.parametrize("parties", [1, 3])
def test_shapes_against_python_integers(world, parties, nin, nout):
    rng = np.random.default_rng([parties, nin, nout])
    hosts, W, Cs = draw(rng, world, parties, nin, nout)
    check(world, hosts, W, Cs, NAMES[:parties])


def test_a_row_of_zero_weights_and_a_weight_that_is_zero_under_one_limb(world):
    w, ids = world, NAMES[:2]
    rng = np.random.default_rng(40)
    hosts, W, Cs = draw(rng, w, 2, 5, 3)
    W[1] = [[0] * w.nq for _ in range(5)]                        # the constant alone
    W[2][3][1] = 0                                               # skipped under limb 1 only
    W[0][0] = [0] * w.nq                                         # a whole input skipped by one output
    _, got = check(w, hosts, W, Cs, ids)
    want = np.zeros_like(got[1])
    want[0, :, 0] = Cs[1]
    assert (got[1] == want).all()


def test_worst_case_accumulation():
    """nin = 16 with every residue, weight and constant q - 1, over a set with the 55-bit prime: 16 products of (q - 1)^2 in one accumulator, plus the
    constant on coefficient 0 -- the largest value the kernel can be asked to hold"""
    w = World(HB.small_bfv(10, 3, big=True))
    assert max(q.bit_length() for q in w.Q) == 55
    host = np.stack([np.stack([np.full(w.N, q - 1, dtype=np.uint64) for q in w.Q]) for _ in range(3)])
    top = [q - 1 for q in w.Q]
    check(w, [host] * 16, [[top] * 16, [top] * 16], [top, top], NAMES[:2])


def test_one_output_equals_ct_lincomb_and_the_chain_of_mul_const_and_sum(world):
    from mkhe_kklss_amd import _abi
    w, ids, nin = world, NAMES[:2], 7
    rng = np.random.default_rng(505)
    hosts, W, Cs = draw(rng, w, 2, nin, 1)
    ins, got = check(w, hosts, W, Cs, ids)
    # mkhe_ct_lincomb on the same context: [n + 1][2][nQ] with im = 0, the constant (C, 0), no division
    zero = [0] * w.nq
    rows = [[Cs[0], zero]] + [[[v * R % q for v, q in zip(W[0][b], w.Q)], zero] for b in range(nin)]
    single = w.new(ids)
    assert w.lib.mkhe_ct_lincomb(w.params.ctx, nin, w.handle_array([c.h for c in ins]), w.block(rows).devptr(), 0, single.h) == 0, w.error()
    assert (single.download() == got[0]).all()
    # the chain, without the constant
    _, plain = check(w, hosts, W, [zero], ids)
    prods = []
    for c, wt in zip(ins, W[0]):
        m = np.array([v * R % q for v, q in zip(wt, w.Q)], dtype=np.uint64)
        prods.append(w.new(ids))
        assert w.lib.mkhe_ct_mul_const(w.params.ctx, c.h, m.ctypes.data_as(_abi.u64p), m.ctypes.data_as(_abi.u64p), prods[-1].h) == 0, w.error()
    chain = w.new(ids)
    assert w.lib.mkhe_ct_sum(w.params.ctx, nin, w.handle_array([p.h for p in prods]), chain.h) == 0, w.error()
    assert (chain.download() == plain[0]).all()


def test_more_limbs_than_limb_groups():
    """The launch makes min(nQ, ceil(2^18 / (N * components))) limb groups, one thread per coefficient of a component: a thread walks several limbs
    only when N * components * (nQ - 1) >= 2^18.  N = 2^13 with four components makes 8 groups, so nQ = 9 is the first limb count at which a group
    owns two limbs; that is 2^15 * 9 words per ciphertext, the fewest of any such shape within the 11 primes of the test chain (N * components = 2^15 is
    the smallest product whose group count, 8, is below 11; 2^16 needs 5 limbs and 2^17 needs 3, both more words).  Every smaller shape runs the limb
    loop exactly once."""
    w = World(HB.small_bfv(13, 9))
    assert w.N * 4 * (w.nq - 1) >= 1 << 18 and -(-(1 << 18) // (w.N * 4)) == 8 < w.nq
    rng = np.random.default_rng(1309)
    hosts, W, Cs = draw(rng, w, 3, 2, 2)
    check(w, hosts, W, Cs, NAMES)


def test_refusals(world):
    from mkhe_kklss_amd import mkckks, mkrlwe
    w, ids = world, NAMES[:2]
    rng = np.random.default_rng(606)
    hosts, W, Cs = draw(rng, w, 2, 2, 2)
    consts = w.consts(W, Cs)
    ins = [w.ct(x, ids) for x in hosts]
    sentinel = H.uniform_ct(rng, w, 2, w.nq)
    outs = [w.new(ids).upload(sentinel) for _ in range(2)]

    def refused(rc, text):
        assert rc != 0
        assert w.error().startswith(NAME + ": ") and text in w.error(), w.error()
        for o in outs:
            assert (o.download() == sentinel).all()              # nothing was enqueued
        for c, x in zip(ins, hosts):
            assert (c.download() == x).all()

    def works():
        fresh = [w.new(ids) for _ in outs]
        assert w.call(ins, consts, fresh) == 0, w.error()
        got, ref = [f.download() for f in fresh], model(w.Q, hosts, W, Cs)
        assert all((a == b).all() for a, b in zip(got, ref))

    works()
    other = w.ct(H.uniform_ct(rng, w, 1, w.nq), NAMES[1:2])
    low = mkrlwe.Ciphertext(w.params, ids, w.params.MaxLevel() - 1)
    refused(w.call([ins[0], other], consts, outs), "share their ids")                      # differing ids, among the inputs and with an output
    refused(w.call(ins, consts, [outs[0], other]), "ids of the inputs")
    assert w.call(ins, consts, [ins[1], outs[1]]) != 0                                      # an output aliasing an input (the inputs stay)
    assert w.error().startswith(NAME + ": ") and "alias" in w.error()
    for c, x in zip(ins, hosts):
        assert (c.download() == x).all()
    refused(w.call(ins, consts, [outs[0], outs[0]]), "distinct")                           # two equal outputs
    refused(w.call([ins[0], None], consts, outs), "null")                                  # null members and null lists
    refused(w.call(ins, consts, [outs[0], None]), "null")
    refused(w.call(None, consts, outs, nin=2), "null")
    refused(w.call(ins, consts, None, nout=2), "null")
    refused(w.call(ins, None, outs), "null")
    refused(w.call(ins, C.c_void_p(consts.devptr().value + 8), outs), "aligned")
    refused(w.call([ins[0], low], consts, outs), "maximum level")                          # a handle below the maximum level
    refused(w.call(ins, consts, [outs[0], low]), "maximum level")
    for nin, nout, text in ((0, 2, "nin"), (17, 2, "nin"), (2, 0, "nout"), (2, 65, "nout")):
        refused(w.call(ins, consts, outs, nin=nin, nout=nout), text)
    assert w.call(ins, consts, outs, ctx=C.c_void_p(None)) != 0 and w.error() == NAME + ": null context"
    works()
    # a non-BFV context
    ck = H.small_ckks(10, 3)
    cparams = mkckks.Parameters(ck["logN"], ck["Q"], ck["P"], ck["scale"])
    cin, cout = mkrlwe.Ciphertext(cparams, ["user0"], 2), mkrlwe.Ciphertext(cparams, ["user0"], 2)
    cbuf = mkrlwe.DeviceLimbs(cparams, 1, 1)
    assert w.call([cin], cbuf, [cout], ctx=cparams.ctx) != 0
    assert w.error() == NAME + ": needs a BFV context"
    del cin, cout, cbuf
    cparams.close()
    for o in outs:
        assert (o.download() == sentinel).all()
    works()
