"""The MK-BFV basis conversions on their index and carry edges (-m gpu): basis_conv_kernel behind mkhe_bfv_modup_q_to_r, mkhe_bfv_rescale and
mkhe_bfv_quantize, on polynomials that are uniform except for the planted coefficients of tests/bfv_conv_model.py -- every table entry of
vtimesqmodp, the float index one above and one below the exact floor, the largest c0 / c1 column sums (k0 up to 10; k1 = 1 on the 16 x 60-bit set),
the largest lazy representatives -- then the consumers of the lazy outputs (the ring-R forward NTT, DecomposeBFV) and the fused callers (MulRelinNew,
mkhe_bfv_mul_relin_sum).  Everything goes through the C ABI and is compared bit for bit: planted coefficients with the column model, whole arrays
with the C oracle.  The CPU half (what each plant reaches, the mutants it separates) is tests/test_bfv_conv_model.py."""
import functools

import numpy as np
import pytest

import bfv_conv_model as B
import bfv_mulrelin_sum_model as BM
import harness as H
import harness_bfv as HB
from oracle import pymodel as M

pytestmark = pytest.mark.gpu

SETS = list(B.sets())
IN_SITU = ["PN15QP880_N11", "60bit_q16"]


class Dev:
    """one parameter set: the planted inputs, the oracle and the device context, each built once"""

    def __init__(self, name):
        from mkhe_kklss_amd import mkbfv, mkrlwe
        self.name, self.mk, self.mkb = name, mkrlwe, mkbfv
        self.pl = B.plants(name)
        self.bc, pset = self.pl.bc, self.pl.pset
        self.bfv = HB.make_bfv(pset)
        self.params = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], pset["T"])
        self.ev = mkbfv.NewEvaluator(self.params)
        self.N, self.nq = 1 << pset["logN"], len(pset["Q"])
        self.Q, self.QMul = self.bc.Q, self.bc.QMul
        self.R = self.Q + self.QMul
        self.rng = np.random.default_rng(1000 + len(name))

    def planted_q(self, rows, polys=(0, 2), count=3):
        """(x, layout): `count` uniform polynomials over Q with rows[s] at layout.at[s]"""
        x = np.stack([H.uniform_poly(self.rng, self.Q, self.N) for _ in range(count)])
        lay = B.Layout(self.N, len(rows), polys)
        return lay.put(x, rows), lay

    @functools.cached_property
    def modup_in(self):
        return self.planted_q([x for _, _, x in self.pl.modup])

    @functools.cached_property
    def rescale_in(self):
        return self.planted_q([x for _, _, _, x in self.pl.rescale])

    def conv(self, fn, x):
        src = self.mk.DeviceLimbs(self.params, x.shape[0], self.nq).upload(x)
        dst = self.mkb.PolyR(self.params, x.shape[0])
        fn(src, dst)
        return dst.download()

    def ntt_r(self, polys):
        from mkhe_kklss_amd._abi import check, lib
        src = self.mkb.PolyR(self.params, polys.shape[0]).upload(polys)
        dst = self.mkb.PolyR(self.params, polys.shape[0])
        check(lib().mkhe_bfv_ntt_r(self.params.ctx, src.devptr(), dst.devptr(), polys.shape[0], 0))
        return dst.download()

    def swk(self):
        host = H.uniform_swk(self.rng, self.bfv.ks)
        return host, self.mk.SwitchingKey(self.params, host)

    def keys(self, names):
        host, dev = {}, self.mkb.NewRelinearizationKeyKeySet(self.params)
        for i, n in enumerate(names):
            ks = [H.uniform_swk(self.rng, self.bfv.ks) for _ in range(5)]
            host[i] = tuple(ks)
            dev.AddRelinearizationKey(self.mkb.RelinearizationKey(self.params, n, *ks))
        u_h, u_d = self.swk()
        self.params.CRS[-1] = u_d
        return host, dev, u_h

    def operands(self, names):
        """(op0, op1) on the host: uniform ciphertexts that carry the ModUpQtoR plants (op0) and the Rescale plants (op1) in EVERY component"""
        every = tuple(range(1 + len(names)))
        h0, _ = self.planted_q([x for _, _, x in self.pl.modup], every, len(every))
        h1, _ = self.planted_q([x for _, _, _, x in self.pl.rescale], every, len(every))
        return h0, h1


@functools.lru_cache(maxsize=None)
def dev(name):
    return Dev(name)


@pytest.fixture(scope="module", params=SETS)
def w(request):
    return dev(request.param)


def _ratio(got, mods):
    return max(int(z) / m for z, m in zip(got, mods))


def test_modup_q_to_r(w):
    """the Q part is copied (row 0 of the grid only), the QMul part is the lazy lift: the oracle on three whole polynomials, the column model at
    every planted coefficient (first and last polynomial, last coefficients included)"""
    x, lay = w.modup_in
    got = w.conv(w.ev.conv.ModUpQtoR, x)
    worst = 0.0
    for (c, n), (name, y, xx) in zip(lay.at, w.pl.modup):
        want, _ = w.bc.modup_q_to_r(xx)
        assert [int(v) for v in got[c, :, n]] == want, (w.name, name, c, n)
        worst = max(worst, _ratio(got[c, w.nq:, n], w.QMul))
    for c in range(3):
        assert (got[c] == w.bfv.modup_q_to_r(x[c])).all(), (w.name, c)
    assert worst < 3, worst
    print("[%s] ModUpQtoR: largest planted representative / modulus on the device %.4f" % (w.name, worst))


def test_rescale(w):
    """both conversions of Rescale: the plants of the first (Q -> QMul, behind the prescale) and those steered through it onto the second"""
    x, lay = w.rescale_in
    got = w.conv(w.ev.conv.Rescale, x)
    worst = 0.0
    for (c, n), (name, which, y, xx) in zip(lay.at, w.pl.rescale):
        want, _ = w.bc.rescale(xx)
        assert [int(v) for v in got[c, :, n]] == want, (w.name, name, which, c, n)
        worst = max(worst, _ratio(got[c, : w.nq, n], w.Q))
    for c in range(3):
        assert (got[c] == w.bfv.rescale(x[c])).all(), (w.name, c)
    assert worst < 3, worst
    print("[%s] Rescale: largest planted representative / modulus on the device %.4f" % (w.name, worst))


def test_quantize(w):
    """the Quantize tail (the ModDown form of the kernel: xsub and downparam): results 0 and q_j - 1 in every limb, xsub 0 and q_j - 1, over every
    tuple of the QMul basis"""
    rows = [xr for _, _, _, xr in w.pl.quantize]
    xr = np.stack([H.uniform_poly(w.rng, w.R, w.N) for _ in range(3)])
    lay = B.Layout(w.N, len(rows))
    lay.put(xr, rows)
    f = np.stack([w.bfv.ntt_r(xr[c]) for c in range(3)])
    src = w.mkb.PolyR(w.params, 3).upload(f)
    out = w.mk.DeviceLimbs(w.params, 3, w.nq)
    w.ev.conv.Quantize(src, out, w.params.T())
    got = out.download()
    for (c, n), (name, y, variant, row) in zip(lay.at, w.pl.quantize):
        want, _ = w.bc.quantize(row)
        assert [int(v) for v in got[c, :, n]] == want, (w.name, name, variant, c, n)
        if variant == "result 0":
            assert (got[c, :, n] == 0).all()
        elif variant == "result q-1":
            assert [int(v) for v in got[c, :, n]] == [q - 1 for q in w.Q]
    for c in range(3):
        assert (got[c] == w.bfv.quantize(f[c])).all(), (w.name, c)


@pytest.mark.parametrize("kind", ["modup", "rescale"])
def test_lazy_outputs_where_they_are_consumed(w, kind):
    """the ring-R forward NTT and DecomposeBFV on the planted ModUpQtoR / Rescale outputs, the largest representatives found among them"""
    x, lay = w.modup_in if kind == "modup" else w.rescale_in
    ar = np.stack([(w.bfv.modup_q_to_r if kind == "modup" else w.bfv.rescale)(x[c]) for c in range(3)])
    got = w.ntt_r(ar)
    for c in range(3):
        assert (got[c] == w.bfv.ntt_r(ar[c])).all(), (w.name, c)
    for c in (0, 2):
        src = w.mkb.PolyR(w.params, 1).upload(ar[c][None])
        ad1, ad2 = w.mk.NewSwitchingKey(w.params), w.mk.NewSwitchingKey(w.params)
        w.ev.ksw.DecomposeBFV(src, ad1, ad2)
        e1, e2 = w.bfv.decompose(ar[c])
        assert (ad1.download() == e1).all() and (ad2.download() == e2).all(), (w.name, c)


def test_ntt_r_at_the_lazy_bound(w):
    """the ring-R forward NTT (NttBatch::src_lazy) on a polynomial whose every coefficient is 3 m_j - 1, and on one alternating 0 and 3 m_j - 1:
    the oracle on every limb; at N = 2^10 also the transform by definition (pymodel.ntt_def) of the reduced values on the first and the last limb"""
    full = np.stack([np.full(w.N, 3 * m - 1, dtype=np.uint64) for m in w.R])
    alt = full.copy()
    alt[:, 0::2] = 0
    polys = np.stack([full, alt])
    got = w.ntt_r(polys)
    for c in range(2):
        assert (got[c] == w.bfv.ntt_r(polys[c])).all(), (w.name, c)
    if w.N == 1 << 10:
        for l in (0, 2 * w.nq - 1):
            m = w.R[l]
            psi = M.find_psi(m, w.N)
            for c in range(2):
                assert [int(v) for v in got[c, l]] == M.ntt_def([int(v) % m for v in polys[c, l]], m, psi, 10), (w.name, c, l)


@pytest.mark.parametrize("name", IN_SITU)
def test_mul_relin_new_carries_the_plants(name):
    """MulRelinNew of two parties whose operands carry the ModUpQtoR plants (op0) and the Rescale plants (op1) in every component: the fused callers
    of engine_bfv.hip pass the same tables and strides"""
    d = dev(name)
    names = ["a", "b"]
    h0, h1 = d.operands(names)
    rlk_h, rlk_d, u_h = d.keys(names)
    c0, c1 = d.mkb.NewCiphertext(d.params, names).upload(h0), d.mkb.NewCiphertext(d.params, names).upload(h1)
    _, ref = d.bfv.mul_relin_new([0, 1], h0, [0, 1], h1, rlk_h, u_h)
    assert (d.ev.MulRelinNew(c0, c1, rlk_d).download() == ref).all()
    assert (d.ev.mulRelin(c0, c1, rlk_d).download() == ref).all()


def test_mul_relin_sum_carries_the_plants():
    """mkhe_bfv_mul_relin_sum, K = 2, on the 16 x 60-bit set: both pairs carry the plants (engine_bfv_sum.hip)"""
    d = dev("60bit_q16")
    names = ["a", "b"]
    pairs = [d.operands(names) for _ in range(2)]
    rlk_h, rlk_d, u_h = d.keys(names)
    ops0 = [d.mkb.NewCiphertext(d.params, names).upload(h0) for h0, _ in pairs]
    ops1 = [d.mkb.NewCiphertext(d.params, names).upload(h1) for _, h1 in pairs]
    _, ref = BM.bfv_mul_relin_sum(d.bfv, [0, 1], [h0 for h0, _ in pairs], [0, 1], [h1 for _, h1 in pairs], rlk_h, u_h)
    assert (d.ev.MulRelinSumNew(ops0, ops1, rlk_d).download() == ref).all()
