"""The device arithmetic of csrc/modarith.h and csrc/h16_arith.h, primitive by primitive, at the edges of the contracts their comments state.

lib/libmkhe_arith_probe.so (tests/hip/arith_probe.hip, test only) runs the project's own inline functions element by element; every result is
compared BIT FOR BIT with the Python-integer model of tests/arith_model.py -- the same signed representative, not just the residue class -- on
the edge vectors crossed with each other plus 2^16 operands drawn over the whole accepted range (fixed seed), for moduli that sit on the class
edges.  The range each comment promises is asserted separately, so that a correct-but-too-wide result is reported as such.  pred and bflyF
take their quotient from a floating-point estimate and are checked against their contract alone: congruent, an integer multiple of q away, within
the stated magnitude.  Each test prints the extreme result / q it saw ("ARITH_PROBE_MAX ..."): DESIGN.md section 3.6 is that table.

The rescale step (div_round_last_kernel and the fused epilogue of mkhe_ct_lincomb) goes through the product ABI with planted residues on the
rounding boundary h = (q_L - 1) / 2, against the exact integer model oracle/pymodel.py div_round_last."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import arith_model as A
import harness as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NRAND = 1 << 16
MAX_CALL = 1 << 18
_lib = None


def probe_lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(os.path.join(ROOT, "mkhe-kklss_amd", "lib", "libmkhe_arith_probe.so"))     # built by build(); missing = an error, not a skip
        _lib.mkhe_arith_probe.restype = C.c_int
        _lib.mkhe_arith_probe.argtypes = [C.c_int, C.c_long, C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(C.c_void_p)]
    return _lib


def run_probe(op, inputs, md, nout):
    """inputs: one list of words per operand (n words each; the SW forms take their twiddles one per BLOCK).  Returns nout lists of n words."""
    n = len(inputs[0])
    sw = op in A.SW_OPS
    outs = [np.empty(n, dtype=np.uint64) for _ in range(nout)]
    modw = np.array(md.words(), dtype=np.uint64)
    for s in range(0, n, MAX_CALL):
        e = min(n, s + MAX_CALL)
        ins = [np.array(inputs[0][s:e], dtype=np.uint64)] + [np.array(x[s:e:A.BLOCK] if sw else x[s:e], dtype=np.uint64) for x in inputs[1:]]
        o = [np.zeros(e - s, dtype=np.uint64) for _ in range(nout)]
        pin = (C.c_void_p * 4)(*([a.ctypes.data for a in ins] + [None] * (4 - len(ins))))
        pout = (C.c_void_p * 2)(*([a.ctypes.data for a in o] + [None] * (2 - nout)))
        rc = probe_lib().mkhe_arith_probe(op, e - s, pin, modw.ctypes.data, pout)
        assert rc == 0, "mkhe_arith_probe(op %d) returned HIP error %d" % (op, rc)
        for k in range(nout):
            outs[k][s:e] = o[k]
    return [x.tolist() for x in outs]


CASES = [(p, q) for p in A.PRIMS for q in A.PRIMS[p]["moduli"]]
# what each comment promises for result / q, as printed beside the observed extremes
DOCUMENTED = {"mont_mul_lazy": "[0, 2)", "mont_mul": "[0, 1)", "mont_mul_sd": "|r| <= 1/2 + 2^-33 + |a| w / (q 2^64)", "mm": "|r| <= 1/2 + 2^-33 + |a| w / (q 2^64)",
              "mont_mul_sdu": "[0, 2)", "mm31": "|T| <= 1 + |a| / 2^64", "mm30u": "(-1, 5)", "pred": "|r| <= 1/2 + (|x| 2^-22 + 2^33) / q",
              "bflyF": "|T| <= 1.25", "redc128": "[0, 1)", "canonF": "[0, 1)"}


@pytest.mark.parametrize("prim,q", CASES, ids=["%s-%#x" % c for c in CASES])
def test_primitive_matches_model_and_contract(prim, q):
    md = A.Mod(q)
    info = A.PRIMS[prim]
    cases = A.edge_cases(prim, q)
    nedge = len(cases)
    cases = cases + A.random_cases(prim, q, random.Random(0x5eed ^ q ^ info["ops"][0]), NRAND)
    if len(info["ops"]) == 2:                                             # SW forms: the runs of one twiddle are whole workgroups
        assert nedge % A.BLOCK == 0 and all(cases[i][1] == cases[i - i % A.BLOCK][1] for i in range(len(cases))), "one twiddle per workgroup"
    inputs = A.device_inputs(prim, cases, md)
    want = [A.model(prim, c, md) for c in cases]
    nout = 2 if prim in ("mul64x64", "mac128", "bflyF") else 1
    lo = hi = None
    for op in info["ops"]:
        outs = run_probe(op, inputs, md, nout)
        got = list(zip(*outs))
        for i, c in enumerate(cases):
            if want[i] is not None:
                assert got[i] == want[i], "%s op %d q %#x %s case %d %r: device %r, model %r" % (
                    prim, op, q, "edge" if i < nedge else "random", i, c, got[i], want[i])
        # the contract's range claim, separately (and the whole reference of pred / bflyF)
        for i, c in enumerate(cases):
            err, m = A.contract(prim, c, got[i], md)
            assert err is None, "%s op %d q %#x %s case %d %r -> %r: %s" % (prim, op, q, "edge" if i < nedge else "random", i, c, got[i], err)
            if m is not None:
                lo, hi = (m, m) if lo is None else (min(lo, m), max(hi, m))
    if lo is not None:
        print("ARITH_PROBE_MAX %-14s q=%#x (%.2f bits) documented %s observed min %.6f max %.6f" % (prim, q, np.log2(float(q)), DOCUMENTED[prim], lo, hi))


def test_contract_edges_named_in_the_comments():
    """the two operand pairs the comments single out: mont_mul_lazy at a1 = 2^31 - 1 with w0 near 2^32 (the one accumulator that can wrap), and
    redc128 at the largest sum it accepts, 32 products (q - 1)^2"""
    for q in (A.Q_TOP, 0xfffffffff6a0001):
        md = A.Mod(q)
        top = (q - 1) >> 32
        cases = [(((1 << 31) - 1) << 32 | lo, (hi << 32) | w0) for lo in A.LOW_WORDS for hi in (top, top - 1, 0)
                 for w0 in (0xffffffff, 0xfffffffe, 0xffff0001) if (hi << 32) | w0 < q]
        out, = run_probe(0, A.device_inputs("mont_mul_lazy", cases, md), md, 1)
        for c, r in zip(cases, out):
            assert r == A.mont_mul_lazy(c[0], c[1], md) and A.check_mont_mul_lazy(c[0], c[1], r, md) is None, (hex(q), c, r)
        s = 32 * (q - 1) ** 2
        assert (s >> 64) < 2 * q
        out, = run_probe(6, [[s >> 64], [s & A.M64]], md, 1)
        assert out[0] == s * pow(1 << 64, -1, q) % q
    for q in A.MODULI_F:                           # the one canonicalisation input no integer stands for: -0.0 is 0
        out, = run_probe(18, [[A.f64_bits(-0.0), A.f64_bits(0.0)]], A.Mod(q), 1)
        assert out == [0, 0]


def test_probe_refuses_oversized_and_unknown_calls():
    one = np.zeros(1, dtype=np.uint64)
    pin = (C.c_void_p * 4)(one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data)
    pout = (C.c_void_p * 2)(one.ctypes.data, one.ctypes.data)
    modw = np.array(A.Mod(A.Q_TOP).words(), dtype=np.uint64)
    assert probe_lib().mkhe_arith_probe(7, MAX_CALL + 1, pin, modw.ctypes.data, pout) != 0
    assert probe_lib().mkhe_arith_probe(99, 1, pin, modw.ctypes.data, pout) != 0
    assert probe_lib().mkhe_arith_probe(7, 0, pin, modw.ctypes.data, pout) != 0


# ---------------------------------------------------------------- the rescale step on its rounding boundary, through the product ABI
def planted_ct(Q, N, npoly):
    """[npoly][len(Q)][N]: top-limb residues {0, 1, h - 1, h, h + 1, q_L - 2, q_L - 1} crossed with lower-limb residues {0, 1, q_i - 1, h mod q_i,
    (h mod q_i) +- 1}, one combination per coefficient, all 42 many times over a polynomial; later polynomials shift the assignment"""
    L = len(Q) - 1
    qL = Q[L]
    h = (qL - 1) // 2
    tops = [0, 1, h - 1, h, h + 1, qL - 2, qL - 1]
    out = np.zeros((npoly, len(Q), N), dtype=np.uint64)
    for s in range(npoly):
        for n in range(N):
            combo = (n + 5 * s) % 42
            out[s, L, n] = tops[combo % 7]
            for i in range(L):
                qi = Q[i]
                lows = [0, 1, qi - 1, h % qi, (h % qi + 1) % qi, (h % qi - 1) % qi]
                out[s, i, n] = lows[(combo // 7 + (i if s else 0)) % 6]
    return out


RESCALE_SETS = {"small_ckks_10_4": lambda: H.small_ckks(10, 4), "small_alpha2_11_5": lambda: H.small_alpha2(11, 5)}
_rescale_ref = {}


def rescale_world(name):
    """the planted ciphertext of a set and its exact DivRoundByLastModulus results for nb = 1, 2 (oracle/pymodel.py), computed once and left alone"""
    if name not in _rescale_ref:
        from oracle import pymodel as M
        pset = RESCALE_SETS[name]()
        Q, N = pset["Q"], 1 << pset["logN"]
        host = planted_ct(Q, N, 2)
        ref = {}
        for nb in (1, 2):
            r = np.zeros((2, len(Q) - nb, N), dtype=np.uint64)
            for s in range(2):
                for n in range(N):
                    x, Qs = [int(host[s, l, n]) for l in range(len(Q))], list(Q)
                    for _ in range(nb):
                        x, Qs = M.div_round_last(x, Qs), Qs[:-1]
                    r[s, :, n] = x
            r.setflags(write=False)
            ref[nb] = r
        host.setflags(write=False)
        _rescale_ref[name] = (pset, host, ref)
    return _rescale_ref[name]


@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("name", sorted(RESCALE_SETS))
def test_rescale_on_the_rounding_boundary(name, nb):
    from mkhe_kklss_amd import mkckks
    from mkhe_kklss_amd._abi import check, lib
    pset, host, ref = rescale_world(name)
    params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], pset["scale"], device=0)
    try:
        level = len(pset["Q"]) - 1
        ct = mkckks.NewCiphertext(params, ["a"], level, pset["scale"]).upload(np.array(host))
        out = mkckks.NewCiphertext(params, ["a"], level - nb, pset["scale"])
        check(lib().mkhe_rescale(params.ctx, ct.h, nb, out.h))
        got = out.download()
        assert got.shape == ref[nb].shape
        bad = np.argwhere(got != ref[nb])
        assert bad.size == 0, "first mismatch (poly, limb, coeff) %r: device %d, model %d" % (tuple(bad[0]), got[tuple(bad[0])], ref[nb][tuple(bad[0])])
        assert (ct.download() == host).all()
    finally:
        params.close()


@pytest.mark.parametrize("name", sorted(RESCALE_SETS))
def test_fused_rescale_of_lincomb_on_the_rounding_boundary(name):
    """the same planted rows through mkhe_ct_lincomb with a single unit weight and its fused rescale: bit for bit the model's (and mkhe_rescale's)"""
    from mkhe_kklss_amd import mkckks
    pset, host, ref = rescale_world(name)
    params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], pset["scale"], device=0)
    try:
        level = len(pset["Q"]) - 1
        s_mid = pset["scale"] * float(pset["Q"][level])                    # declared at the middle scale: the weight 1 is encoded as exactly 1
        ct = mkckks.NewCiphertext(params, ["a"], level, s_mid).upload(np.array(host))
        block = mkckks.lincomb_consts(pset["Q"], s_mid, 0, [s_mid], [1])
        assert all(int(block[1, 0, i]) == (1 << 64) % q and int(block[1, 1, i]) == 0 for i, q in enumerate(pset["Q"])) and not block[0].any()
        res = mkckks.NewEvaluator(params).LinCombNew([ct], [1], const=0, scale=pset["scale"], rescale=True)
        got = res.download()
        bad = np.argwhere(got != ref[1])
        assert bad.size == 0, "first mismatch (poly, limb, coeff) %r: device %d, model %d" % (tuple(bad[0]), got[tuple(bad[0])], ref[1][tuple(bad[0])])
    finally:
        params.close()
