"""mkhe_ct_lincomb_multi (-m gpu): out[g] = sum_b (re[g][b] + i im[g][b]) in[b] + (add_re[g] + i add_im[g]) with i = X^(N/2), optionally divided by the
last modulus, for nout rows at once -- bit for bit against a model in Python integers written here from the formulas of include/mkhe.h and the
rounding rule of DivRoundByLastModulus (round(x / q_top) = (x + h - ((x + h) mod q_top)) / q_top, h = (q_top - 1) / 2, limb by limb), and against
mkhe_ct_lincomb called once per row on that row of the same constant block.  Weights and constants are independent uniform residues per limb: the
kernel treats limbs independently, no encoding is involved at this level.

The model holds a whole limb of an input as ONE Python integer, a 256-bit slot per coefficient: a weighted sum of limbs is then a handful of
big-integer products by a scalar (32 products below 2^120 fit a slot), and only the final residues are taken coefficient by coefficient."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import harness as H
import harness_bfv as HB

pytestmark = pytest.mark.gpu

CAP_IN, CAP_OUT = 16, 16      # CTLM_MAX_IN, CTLM_MAX_OUT of csrc/poly_kernels.h
R = 1 << 64
NAME = "mkhe_ct_lincomb_multi: "


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

    def consts(self, table, Lc):
        """table[g] = ((add_re[l], add_im[l]), [(re[l], im[l]) per input]) plain -> the device block [nout][nin + 1][2][Lc], weights in Montgomery form"""
        rows = [[[add[0], add[1]]] + [[[w * R % q for w, q in zip(part, self.Q)] for part in (re, im)] for re, im in weights] for add, weights in table]
        arr = np.array([[[[int(v) for v in part[:Lc]] for part in row] for row in out] for out in rows], dtype=np.uint64)
        assert arr.shape == (len(table), len(table[0][1]) + 1, 2, Lc)
        buf = self.mk.DeviceLimbs(self.params, 1, -(-arr.size // self.N))
        return buf.upload(np.concatenate([arr.ravel(), np.zeros(buf.words - arr.size, dtype=np.uint64)]).reshape(1, buf.limbs, self.N))

    def multi(self, ins, consts, nb, outs):
        return self.lib.mkhe_ct_lincomb_multi(self.params.ctx, len(ins), self.handle_array([c.h for c in ins]), len(outs), consts.devptr(), nb,
                                              self.handle_array([c.h for c in outs]))

    def single(self, ins, consts, g, Lc, nb, out):
        """mkhe_ct_lincomb on row g of the multi block, where it lies"""
        row = C.c_void_p(consts.devptr().value + 8 * g * (len(ins) + 1) * 2 * Lc)
        return self.lib.mkhe_ct_lincomb(self.params.ctx, len(ins), self.handle_array([c.h for c in ins]), row, nb, out.h)

    def error(self):
        return self.lib.mkhe_last_error().decode()


@pytest.fixture(scope="module")
def worlds():
    return {logN: World(H.small_ckks(logN, nq=6)) for logN in (10, 12)}


def _pack(x):
    w = np.zeros((x.size, 4), dtype="<u8")
    w[:, 0] = x
    return int.from_bytes(w.tobytes(), "little")


def _unpack(v, n):
    a = np.frombuffer(v.to_bytes(32 * n, "little"), dtype="<u8").reshape(n, 4)
    assert not a[:, 2:].any()
    return a[:, 0].astype(object) + (a[:, 1].astype(object) << 64)


def model(Q, hosts, table, Lc, nb):
    """hosts: uint64 [polys][limbs >= Lc][N] each -> one uint64 [polys][Lc - nb][N] per row of the table"""
    P, N = hosts[0].shape[0], hosts[0].shape[2]
    h = N // 2
    acc = [[] for _ in table]
    for l in range(Lc):
        q = Q[l]
        lo = [_pack(x[:, l, :h].ravel()) for x in hosts]
        hi = [_pack(x[:, l, h:].ravel()) for x in hosts]
        for g, (add, weights) in enumerate(table):
            # acc[j] = sum re x[j] - im x[j + h], acc[j + h] = sum re x[j + h] + im x[j]; -im enters as its residue q - im
            a0 = sum(int(re[l]) * xa + (q - int(im[l])) % q * xb for xa, xb, (re, im) in zip(lo, hi, weights))
            a1 = sum(int(re[l]) * xb + int(im[l]) * xa for xa, xb, (re, im) in zip(lo, hi, weights))
            a = np.concatenate([_unpack(a0, P * h).reshape(P, h), _unpack(a1, P * h).reshape(P, h)], axis=1)
            a[0, 0] += int(add[0][l])
            a[0, h] += int(add[1][l])
            acc[g].append(a % q)
    if nb:
        qt = Q[Lc - 1]
        half = (qt - 1) >> 1
        for g in range(len(table)):
            t = (acc[g][Lc - 1] + half) % qt
            acc[g] = [(acc[g][l] + half - t) * pow(qt, -1, Q[l]) % Q[l] for l in range(Lc - 1)]
    return [np.stack([a.astype(np.uint64) for a in rows], axis=1) for rows in acc]


def draw(rng, Q, N, nin, nout, polys, limbs, Lc):
    hosts = [np.stack([H.uniform_poly(rng, Q[:limbs], N) for _ in range(polys)]) for _ in range(nin)]
    res = lambda: [int(rng.integers(0, q)) for q in Q[:Lc]]
    return hosts, [((res(), res()), [(res(), res()) for _ in range(nin)]) for _ in range(nout)]


def check(w, hosts, table, Lc, nb, ids):
    """the call against the model and against mkhe_ct_lincomb row by row"""
    ins = [w.ct(x, ids) for x in hosts]
    outs = [w.new(ids, Lc - nb) for _ in table]
    consts = w.consts(table, Lc)
    assert w.multi(ins, consts, nb, outs) == 0, w.error()
    got, ref = [o.download() for o in outs], model(w.Q, hosts, table, Lc, nb)
    one = w.new(ids, Lc - nb)
    for g in range(len(table)):
        assert got[g].shape == ref[g].shape and (got[g] == ref[g]).all(), "row %d differs from the model" % g
        assert w.single(ins, consts, g, Lc, nb, one) == 0, w.error()
        assert (one.download() == got[g]).all(), "row %d differs from mkhe_ct_lincomb" % g
    return got


@pytest.mark.parametrize("Lc,nb", [(1, 0), (2, 1), (4, 0), (4, 1)])
@pytest.mark.parametrize("nin,nout", [(1, 1), (2, 7), (5, 2), (16, 16), (9, 16), (16, 1)])          # every NI and NO of the kernel, both ends of nout
@pytest.mark.parametrize("parties", [1, 3])
@pytest.mark.parametrize("logN", [10, 12])
def test_basic_shapes(worlds, logN, parties, nin, nout, Lc, nb):
    w = worlds[logN]
    rng = np.random.default_rng([logN, parties, nin, nout, Lc, nb])
    hosts, table = draw(rng, w.Q, w.N, nin, nout, 1 + parties, Lc, Lc)
    check(w, hosts, table, Lc, nb, ["p%d" % i for i in range(parties)])


@pytest.mark.parametrize("nb", [0, 1])
def test_inputs_with_more_limbs_than_the_sums(worlds, nb):
    w, Lc = worlds[10], 3
    rng = np.random.default_rng(77 + nb)
    hosts, table = draw(rng, w.Q, w.N, 3, 5, 3, Lc + 2, Lc)
    check(w, hosts, table, Lc, nb, ["p0", "p1"])
    # and inputs at different levels
    hosts[1] = hosts[1][:, :Lc]
    hosts[2] = hosts[2][:, : Lc + 1]
    check(w, hosts, table, Lc, nb, ["p0", "p1"])


@pytest.mark.parametrize("nb", [0, 1])
def test_zero_patterns(worlds, nb):
    w, Lc, ids = worlds[10], 3, ["p0", "p1"]
    rng = np.random.default_rng(5 + nb)
    zero = [0] * Lc
    hosts, table = draw(rng, w.Q, w.N, 5, 4, 3, Lc, Lc)
    # row 1: all weights zero, the constant alone
    table[1] = (table[1][0], [(zero, zero)] * 5)
    got = check(w, hosts, table, Lc, nb, ids)
    if not nb:
        want = np.zeros_like(got[1])
        want[0, :, 0], want[0, :, w.N // 2] = table[1][0][0], table[1][0][1]
        assert (got[1] == want).all()
    # a purely real table
    real = [(add, [(re, zero) for re, _ in weights]) for add, weights in table]
    check(w, hosts, real, Lc, nb, ids)
    # purely imaginary weights: row 0 throughout, one weight of row 2; i * x alone is the negacyclic shift by N/2
    imag = list(table)
    imag[0] = (imag[0][0], [(zero, im) for _, im in imag[0][1]])
    imag[2] = (imag[2][0], [imag[2][1][0], (zero, imag[2][1][1][1])] + imag[2][1][2:])
    check(w, hosts, imag, Lc, nb, ids)
    if not nb:
        shift = [((zero, zero), [(zero, [1] * Lc)] + [(zero, zero)] * 4), ((zero, zero), [([1] * Lc, zero)] + [(zero, zero)] * 4)]
        got = check(w, hosts, shift, Lc, 0, ids)
        x, h = hosts[0], w.N // 2
        q = np.array(w.Q[:Lc], dtype=np.uint64)[None, :, None]
        assert (got[0][..., h:] == x[..., :h]).all() and (got[0][..., :h] == (q - x[..., h:]) % q).all() and (got[1] == x).all()
    # weights that are zero under one limb only (re, im, or both), the other limbs random
    holes = []
    for g, (add, weights) in enumerate(table):
        ws = []
        for b, (re, im) in enumerate(weights):
            re, im, l = list(re), list(im), (g + b) % Lc
            if (g + b) % 3 != 1:
                re[l] = 0
            if (g + b) % 3 != 2:
                im[l] = 0
            ws.append((re, im))
        holes.append((add, ws))
    check(w, hosts, holes, Lc, nb, ids)


@pytest.mark.parametrize("nb", [0, 1])
def test_worst_case_accumulation(nb):
    """nin = cap, every residue, weight and constant q - 1, over the 60-bit prime of PN15QP880 and one 54-bit prime: 2 * cap products of (q - 1)^2 in
    the sum of the upper half of every pair -- the largest value an accumulator of the kernel can be asked to hold"""
    pset = H.small_ckks(10, nq=2)
    assert pset["Q"][0].bit_length() == 60 and pset["Q"][1].bit_length() == 54
    w, Lc = World(pset), 2
    host = np.stack([np.stack([np.full(w.N, q - 1, dtype=np.uint64) for q in w.Q]) for _ in range(3)])
    top = [q - 1 for q in w.Q]
    check(w, [host] * CAP_IN, [((top, top), [(top, top)] * CAP_IN)] * 3, Lc, nb, ["p0", "p1"])


@pytest.mark.parametrize("nb", [0, 1])
def test_more_limbs_than_limb_groups(nb):
    """N = 2^15 with four polynomials is the smallest shape at which the launch makes fewer limb groups (four) than output limbs, so that one thread
    walks several limbs -- with a rescale, keeping its rounded top-limb residues: the loop that every smaller shape runs exactly once"""
    w, Lc, ids = World(H.small_ckks(15, nq=6)), 6, ["p0", "p1", "p2"]
    rng = np.random.default_rng(1500 + nb)
    hosts, table = draw(rng, w.Q, w.N, 2, 3, 4, Lc, Lc)
    check(w, hosts, table, Lc, nb, ids)


def test_refusals_on_a_live_context(worlds):
    from mkhe_kklss_amd import mkbfv
    w, Lc, ids = worlds[10], 2, ["p0", "p1"]
    rng = np.random.default_rng(606)
    hosts, table = draw(rng, w.Q, w.N, 2, 2, 3, Lc, Lc)
    ins, consts = [w.ct(x, ids) for x in hosts], w.consts(table, Lc)
    outs = [w.new(ids, Lc), w.new(ids, Lc)]
    sentinel = np.stack([H.uniform_poly(rng, w.Q[:Lc], w.N) for _ in range(3)])
    for o in outs:
        o.upload(sentinel)
    ctx, hin, hout = w.params.ctx, w.handle_array([c.h for c in ins]), w.handle_array([c.h for c in outs])

    def refused(rc, text):
        assert rc != 0, "accepted"
        assert w.error().startswith(NAME) and text in w.error(), w.error()

    other = w.ct(hosts[0], ["p0", "p2"])
    refused(w.multi([ins[0], other], consts, 0, outs), "same ids")                                  # mismatched ids among the inputs
    refused(w.multi(ins, consts, 0, [outs[0], w.new(["p0"], Lc)]), "same ids")                      # ... and of an output
    refused(w.multi(ins, consts, 0, [outs[0], w.new(ids, Lc - 1)]), "same number of limbs")         # unequal output limbs
    refused(w.multi(ins, consts, 0, [w.new(ids, Lc + 1), w.new(ids, Lc + 1)]), "fewer limbs")       # an input with fewer than Lc limbs
    refused(w.multi(ins, consts, 1, outs), "fewer limbs")                                           # the same through the rescale
    refused(w.multi([ins[0], outs[1]], consts, 0, outs), "alias")                                   # an output aliasing an input
    refused(w.multi(ins, consts, 0, [outs[0], outs[0]]), "distinct")                                # two equal outputs
    refused(w.lib.mkhe_ct_lincomb_multi(ctx, 2, None, 2, consts.devptr(), 0, hout), "null argument")
    refused(w.lib.mkhe_ct_lincomb_multi(ctx, 2, hin, 2, None, 0, hout), "null argument")
    refused(w.lib.mkhe_ct_lincomb_multi(ctx, 2, hin, 2, consts.devptr(), 0, None), "null argument")
    refused(w.lib.mkhe_ct_lincomb_multi(ctx, 2, w.handle_array([ins[0].h, None]), 2, consts.devptr(), 0, hout), "null ciphertext")
    refused(w.lib.mkhe_ct_lincomb_multi(ctx, 2, hin, 2, consts.devptr(), 0, w.handle_array([outs[0].h, None])), "null output")
    refused(w.lib.mkhe_ct_lincomb_multi(ctx, CAP_IN + 1, hin, 2, consts.devptr(), 0, hout), "nin must be 1 .. 16")
    refused(w.lib.mkhe_ct_lincomb_multi(ctx, 2, hin, CAP_OUT + 1, consts.devptr(), 0, hout), "nout must be 1 .. 16")
    refused(w.lib.mkhe_ct_lincomb_multi(ctx, 2, hin, 2, consts.devptr(), 2, hout), "nb_rescale must be 0 or 1")
    # a BFV context: the call of that scheme is mkhe_bfv_ct_lincomb
    pset = HB.small_bfv(10, 3)
    bfv = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], pset["T"])
    bins = [mkbfv.NewCiphertext(bfv, ids) for _ in range(2)]
    bouts = [mkbfv.NewCiphertext(bfv, ids) for _ in range(2)]
    block = w.mk.DeviceLimbs(bfv, 1, 1)
    rc = w.lib.mkhe_ct_lincomb_multi(bfv.ctx, 2, w.handle_array([c.h for c in bins]), 2, block.devptr(), 0, w.handle_array([c.h for c in bouts]))
    refused(rc, "needs a CKKS or mkrlwe context")
    # nothing was launched: the outputs still hold what was uploaded; and the context still works
    for o in outs:
        assert (o.download() == sentinel).all()
    assert w.multi(ins, consts, 0, outs) == 0, w.error()
    for o, ref in zip(outs, model(w.Q, hosts, table, Lc, 0)):
        assert (o.download() == ref).all()


def test_inside_a_captured_graph():
    """mkhe_capture_begin / mkhe_ct_lincomb_multi / mkhe_capture_end / mkhe_graph_launch against the eager call, in a fresh interpreter: a process that
    has imported torch is bound to a HIP runtime in which mkhe_capture_begin refuses to capture (tests/test_gpu_cnn.py)"""
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, os.path.join(here, "lincomb_multi_graph_check.py")], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and "graph replay ok" in out.stdout
