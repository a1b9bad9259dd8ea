"""The column model of the MK-BFV basis conversions and its planted set, on the CPU (tests/bfv_conv_model.py): the model is the literal modUpExact
of oracle/pymodel.py, every plant arrives at the conversion it targets, the planted set reads every table entry and reaches the second carry counter
where the parameter set has one, and it separates the kernel's arithmetic from six near misses that uniform data does not.
tests/test_gpu_bfv_conv_edges.py puts the same material through the device."""
import numpy as np
import pytest

import bfv_conv_model as B
import steer_model as S
from oracle import pymodel as M

SETS = B.sets()
UNIFORM = 4096


@pytest.fixture(scope="module", params=list(SETS))
def ps(request):
    p = B.plants(request.param)
    p.name = request.param
    return p


def _directions(p):
    return (("Q->QMul", p.bc.q2m, p.fq), ("QMul->Q", p.bc.m2q, p.fm))


_uniform_cache = {}


def _uniform(name, conv, tag):
    """UNIFORM source vectors of one direction and what the column model makes of them, computed once per set: [(x, y, out, v, cols)]"""
    key = (name, tag)
    if key not in _uniform_cache:
        rng = np.random.default_rng(len(conv.S) * 131 + len(tag))
        U = np.stack([rng.integers(0, q, UNIFORM, dtype=np.uint64) for q in conv.S])
        rows = []
        for k in range(UNIFORM):
            x = [int(v) for v in U[:, k]]
            y = conv.y_of(x)
            rows.append((x, y) + conv.lift_y(y))
        _uniform_cache[key] = rows
    return _uniform_cache[key]


def test_column_model_is_the_literal_form(ps):
    """c0, c1, c2, k0, k1 -> (rlo, rhi) is the 128-bit sum of modup_literal: equal lazy representatives and equal index on every planted tuple and on
    4096 uniform vectors, in both directions"""
    for tag, conv, fam in _directions(ps):
        for name, y in fam:
            x = conv.x_of(y)
            out, v, _ = conv.lift(x)
            assert conv.y_of(x) == y, (tag, name)
            assert (out, v) == M.modup_literal(x, conv.S, conv.T), (tag, name)
        for x, y, out, v, _ in _uniform(ps.name, conv, tag):
            assert (out, v) == M.modup_literal(x, conv.S, conv.T), tag


def test_three_conversions_are_the_bfv_model(ps):
    """ModUpQtoR, Rescale and Quantize built from the column model are BfvModel.modup_q_to_r, rescale and quantize_coeff on every planted input and on
    uniform ones, 2^10 columns at a time"""
    pset, bc = ps.pset, ps.bc
    model = M.BfvModel(10, pset["Q"], pset["QMul"], pset["P"], pset["T"])
    N, nq = model.N, bc.nq
    rng = np.random.default_rng(17)

    def chunks(rows, mods):
        rows = [list(r) for r in rows] + [[int(rng.integers(0, m)) for m in mods] for _ in range(64)]
        while len(rows) % N:
            rows.append([int(rng.integers(0, m)) for m in mods])
        for at in range(0, len(rows), N):
            yield rows[at: at + N]

    for fn, ref, rows, mods in ((bc.modup_q_to_r, model.modup_q_to_r, [x for _, _, x in ps.modup], bc.Q),
                                (bc.rescale, model.rescale, [x for _, _, _, x in ps.rescale], bc.Q),
                                (bc.quantize, model.quantize_coeff, [xr for _, _, _, xr in ps.quantize], bc.Q + bc.QMul)):
        for chunk in chunks(rows, mods):
            poly = [[row[l] for row in chunk] for l in range(len(mods))]
            want = ref(poly)
            for k, row in enumerate(chunk):
                assert fn(row)[0] == [w[k] for w in want], (fn.__name__, k)


def test_every_plant_arrives(ps, capsys):
    """for each planted coefficient the model's y at the conversion it targets is the intended tuple; at most a quarter of the targets of Rescale's
    second conversion has no preimage, and every family keeps a tuple there"""
    bc = ps.bc
    for name, y, x in ps.modup:
        assert all(0 <= v < q for v, q in zip(x, bc.Q))
        assert bc.modup_q_to_r(x)[1][0].y == y, name
    for name, which, y, x in ps.rescale:
        assert all(0 <= v < q for v, q in zip(x, bc.Q))
        assert bc.rescale(x)[1][which].y == y, (name, which)
    for name, y, variant, xr in ps.quantize:
        out, (tr,) = bc.quantize(xr)
        assert tr.y == y, (name, variant)
        tq = [a * bc.T % q for a, q in zip(xr[: bc.nq], bc.Q)]
        if variant == "result 0":
            assert out == [0] * bc.nq
        elif variant == "result q-1":
            assert out == [q - 1 for q in bc.Q]
        elif variant == "xsub 0":
            assert tq == [0] * bc.nq
        elif variant == "xsub q-1":
            assert tq == [q - 1 for q in bc.Q]
    # (targets are counted as distinct tuples: with few limbs several families name the same one)
    second = [name for name, which, _, _ in ps.rescale if which == 1]
    missing = {tuple(y) for _, y in ps.missing}
    total = len({tuple(y) for _, y in ps.fm})
    with capsys.disabled():
        print("\n[%s] Rescale, second conversion: %d of %d targets without a preimage" % (ps.name, len(missing), total))
    assert 4 * len(missing) <= total, (len(missing), total)
    if bc.nq >= 2:
        assert {B.family_of(n) for n, _ in ps.fm} == {B.family_of(n) for n in second}, "a family lost every tuple"
    else:
        # one limb: the source of the second conversion is W = -u / Q + delta mod p with u < Q the input times QMul and delta = 1 only for u
        # within 64 of Q; W = p - 1 asks for u = Q (delta = 0) or u = 2 Q mod p (delta = 1), neither of which is such a u.  Every family
        # that consists of y = [p - 1] alone loses it, and nothing else is lost.
        assert missing == {(bc.QMul[0] - 1,)}, missing


def test_coverage_of_the_planted_set(ps, capsys):
    """per direction: every table entry a tuple can read at all is read by a planted coefficient (0..ns; 0..ns - 1 where primes of 53 bits keep the
    float sum of ns quotients below ns: reachable_top), c2 stays below 2^64 and the representative below 3 moduli on every vector; the 16 x 60-bit
    set reaches k1 >= 1 and holds tuples whose float index is one below the exact floor"""
    bc = ps.bc
    arrived = {"Q->QMul": [bc.modup_q_to_r(x)[1][0] for _, _, x in ps.modup] + [bc.rescale(x)[1][0] for _, w, _, x in ps.rescale if w == 0],
               # (the second conversion of Rescale runs behind the plants of the first one too: whatever it reads there counts)
               "QMul->Q": [bc.rescale(x)[1][1] for _, _, _, x in ps.rescale] + [bc.quantize(xr)[1][0] for _, _, _, xr in ps.quantize]}
    lines = []
    for tag, conv, fam in _directions(ps):
        traces = arrived[tag]
        top = B.reachable_top(conv.S)
        assert top == conv.ns or min(conv.S) < (1 << 53), "only primes of 53 bits or fewer lose the last entry"
        read = sorted({t.v for t in traces})
        k0 = max(c.k0 for t in traces for c in t.cols)
        k1 = max(c.k1 for t in traces for c in t.cols)
        c1 = max(c.c1_sum for t in traces for c in t.cols)
        under = sum(t.v == S.index_exact(t.y, conv.S) - 1 for t in traces)
        over = sum(t.v == S.index_exact(t.y, conv.S) + 1 for t in traces)
        uni = _uniform(ps.name, conv, tag)
        c2 = max([c.c2 for t in traces for c in t.cols] + [c.c2 for row in uni for c in row[4]])
        ratio = max(t.ratio() for t in traces)
        ratio_u = max(max(z / p for z, p in zip(row[2], conv.T)) for row in uni)
        lines.append("  %-8s entries read %s of 0..%d   k0 <= %d   k1 <= %d   c1 / 2^64 <= %.3f   index below floor x %d, above x %d   "
                     "c2 / 2^64 <= %.4f   representative / modulus <= %.4f (uniform: %.4f)"
                     % (tag, "%d..%d" % (read[0], read[-1]), conv.ns, k0, k1, c1 / B.R, under, over, c2 / B.R, ratio, ratio_u))
        msg = lines[-1]
        assert read == list(range(top + 1)), msg
        assert c2 < B.R, msg
        assert max(ratio, ratio_u) < 3, msg
        if ps.name == "60bit_q16":
            assert k1 >= 1 and c1 >= B.R, msg
            assert under >= 1, msg
        assert (k1 >= 1) == (B._max_c1(conv.S, conv.T) >= B.R), msg          # the planted set reaches k1 wherever any tuple can
    with capsys.disabled():
        print("\n[%s] what the planted coefficients reach" % ps.name)
        print("\n".join(lines))


def test_planted_set_separates_the_near_misses(ps, capsys):
    """Six wrong forms -- the exact floor, y * (1.0 / p), the terms added in reverse order, a table clipped at ns - 1, k1 left out of rhi, k1 added at
    weight 2^0 instead of 2^32 -- against the literal form, on the planted tuples and on 4096 uniform vectors, side by side.  Required on the planted
    set: the exact floor everywhere; the reversed order from three terms on; the clipped table wherever entry ns can be read; both k1 mutants
    wherever any tuple carries into k1; y * (1.0 / p) wherever the bounded search of boundary_tuples found a distinguishing tuple (printed)."""
    lines = []
    for tag, conv, fam in _directions(ps):
        planted = [(y,) + conv.lift_y(y) for _, y in fam]
        uni = [row[1:] for row in _uniform(ps.name, conv, tag)]
        searched = any(S.index_reciprocal(y, conv.S) != S.index_literal(y, conv.S) for n, y in fam if n == "rounding")
        for mname in B.MUTANTS:
            kw = conv.mutant_kw(mname)
            differs = lambda row: conv.finish(row[0], row[3], **kw)[0] != row[1]
            caught, by_chance = sum(map(differs, planted)), sum(map(differs, uni))
            line = "  %-8s %-22s planted: %3d of %d   uniform: %d of %d" % (tag, mname, caught, len(planted), by_chance, UNIFORM)
            lines.append(line)
            if mname == "exact floor":
                assert caught >= 1, line
            elif mname == "reversed summation":
                assert caught >= 1 or conv.ns < 3, line
            elif mname == "table clipped at ns-1":
                assert (caught >= 1) == (B.reachable_top(conv.S) == conv.ns), line
            elif mname.startswith("k1"):
                assert (caught >= 1) == (B._max_c1(conv.S, conv.T) >= B.R), line
            else:
                assert caught >= 1 or not searched, line
                lines[-1] += "   (the search found a distinguishing tuple: %s)" % ("yes" if searched else "no")
    with capsys.disabled():
        print("\n[%s] vectors on which a near miss differs from the literal form" % ps.name)
        print("\n".join(lines))


def test_the_60_bit_set_is_what_the_docstring_says():
    full = B._bfv60_full()
    mods = full["Q"] + full["QMul"] + full["P"]
    assert len(set(mods)) == 34 and all(m < (1 << 60) and m % (1 << 11) == 1 and M._is_prime(m) for m in mods)
    c1 = (B._max_c1(full["Q"], full["QMul"]) / B.R, B._max_c1(full["QMul"], full["Q"]) / B.R)
    assert full["seed"] == 0 and ["%.3f" % c for c in c1] == ["1.221", "1.175"], (full["seed"], c1)
    for nq in (1, 7, 8, 15):
        assert B.bfv60(nq)["Q"] == full["Q"][:nq] and B.bfv60(nq)["QMul"] == full["QMul"][:nq]
