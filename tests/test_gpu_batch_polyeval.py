"""The weighted sums and polynomial evaluations of mkckks.BatchEvaluator (-m gpu) against the single mkckks.Evaluator, item by item: LinCombNew,
LinCombsNew, AddConstNew, MulRelinRawNew, MulRelinOnceNew, EvaluatePolyNew (degree 7, fused and not) and EvaluateChebyshevNew on B = 1, 2, 3 fresh
two-party encryptions give, for every item, the ciphertext of the single evaluator bit for bit, at its level and Scale.  The worlds (two parties,
device keygen from a seeded HostSampler) are those of tests/test_gpu_chebyshev_e2e.py, imported; one decrypt per shape is held against numpy within
that file's bound (cheb_bound: the MulRelin bound propagated through T_k)."""
import numpy as np
import pytest
from numpy.polynomial import chebyshev as NC

import test_gpu_chebyshev_e2e as CE

pytestmark = pytest.mark.gpu


def same(batch, singles):
    """every member of the batch is the single evaluator's ciphertext: words, level, Scale, ids; and the batch declares that Scale"""
    assert len(batch) == len(singles)
    for c, s in zip(batch.cts, singles):
        assert c.Level() == s.Level() and c.Scale == s.Scale and c.ids == s.ids
        assert (c.download() == s.download()).all()
    assert batch.Scale == singles[0].Scale and batch.Level() == singles[0].Level()


@pytest.mark.parametrize("B", [1, 2, 3])
@pytest.mark.parametrize("key,d,a,b", [((10, 6), 7, -1, 1), ((11, 8), 15, -3, 5)], ids=["d7-unit", "d15-m3p5"])
def test_batch_equals_single_item_by_item(key, d, a, b, B):
    w = CE.world(key)
    mk, ev, rlk, S = w.mkckks, w.ev, w.rlk, w.params.Scale()
    bev = mk.BatchEvaluator(w.params, B, ev=ev)
    enc = [CE.two_party(w, a, b) for _ in range(B)]
    unit = [CE.two_party(w, -1, 1) for _ in range(B)]
    x, u = mk.BatchCiphertext([c for c, _ in enc]), mk.BatchCiphertext([c for c, _ in unit])
    shared = ev.DropLevelNew(CE.two_party(w, -1, 1)[0], 1)                         # a broadcast operand, one level down: the work level is the lowest
    # LinCombNew: complex weights and constant, a zero weight, with and without the rescale, at a lower work level
    for kw in (dict(scale=S / 3), dict(rescale=False, scale=x.Scale * 2), dict(level=2)):
        got = bev.LinCombNew([x, shared, u], [0.5, -1.25 + 0.5j, 0], 0.125 - 0.25j, **kw)
        same(got, [ev.LinCombNew([x.cts[i], shared, u.cts[i]], [0.5, -1.25 + 0.5j, 0], 0.125 - 0.25j, **kw) for i in range(B)])
    # LinCombsNew: a column that is zero in every row is dropped, a zero inside the table stays; one scale per row
    rows, consts = [[0.5, -1.25 + 0.5j, 0], [1j, 0, 0], [2, 3, 0]], [0.125, -0.25j, 0]
    for kw in (dict(scales=[S, S / 3, 2 * S]), dict(rescale=False, scales=x.Scale)):
        got = bev.LinCombsNew([x, shared, u], rows, consts, **kw)
        ref = [ev.LinCombsNew([x.cts[i], shared, u.cts[i]], rows, consts, **kw) for i in range(B)]
        assert len(got) == len(rows)
        for g in range(len(rows)):
            same(got[g], [r[g] for r in ref])
    same(bev.AddConstNew(x, 0.75 - 2j), [ev.AddConstNew(c, 0.75 - 2j) for c in x.cts])
    # the products: raw, and with exactly one Rescale -- where the usual count is one and where a small scale would make it none
    same(bev.MulRelinRawNew(x, u, rlk), [ev.MulRelinRawNew(p, q, rlk) for p, q in zip(x.cts, u.cts)])
    same(bev.MulRelinRawNew(x, shared, rlk), [ev.MulRelinRawNew(p, shared, rlk) for p in x.cts])
    same(bev.MulRelinOnceNew(x, u, rlk), [ev.MulRelinOnceNew(p, q, rlk) for p, q in zip(x.cts, u.cts)])
    small = bev.LinCombNew([u], [1], 0, scale=S / 2.0 ** 20)
    same(small, [ev.LinCombNew([c], [1], 0, scale=S / 2.0 ** 20) for c in u.cts])
    same(bev.MulRelinOnceNew(small, x, rlk, scale=S / 7), [ev.MulRelinOnceNew(p, q, rlk, scale=S / 7) for p, q in zip(small.cts, x.cts)])
    # EvaluatePolyNew, degree 7, one complex coefficient
    coeffs = w.rng.uniform(-1, 1, 8).astype(np.complex128)
    coeffs[5] = 0.5 - 0.75j
    for fused in (True, False):
        same(bev.EvaluatePolyNew(u, coeffs, rlk, fused=fused), [ev.EvaluatePolyNew(c, coeffs, rlk, fused=fused) for c in u.cts])
    # EvaluateChebyshevNew on the interval, and one decrypt against numpy
    cheb = w.rng.uniform(-1, 1, d + 1)
    got = bev.EvaluateChebyshevNew(x, cheb, (a, b), rlk)
    same(got, [ev.EvaluateChebyshevNew(c, cheb, (a, b), rlk) for c in x.cts])
    assert got.Level() == x.Level() - CE.need(d, a, b) and got.Scale == S
    dec = w.dec.Decrypt(got.cts[B - 1], w.skSet).Value
    err, bound = CE._max_log2_err(dec, NC.chebval((2 * enc[B - 1][1] - a - b) / (b - a), cheb)), CE.cheb_bound(w, cheb, a, b)
    print("batch EvaluateChebyshevNew logN=%d d=%d B=%d on (%g, %g): 2^%.1f, bound 2^%.1f" % (key[0], d, B, a, b, err, bound))
    assert err <= bound
