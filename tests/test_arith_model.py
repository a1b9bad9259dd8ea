"""The integer models of tests/arith_model.py against pow() and %, and the teeth of their edge vectors (no GPU).

The GPU test (tests/test_gpu_arith_probe.py) compares the device primitives bit for bit with these models, so the models themselves must be
right -- every one satisfies its congruence and its stated range on the edge set -- and the edge set ALONE (no random operands) must tell
every deliberately wrong variant from the truth."""
import os
import subprocess

import pytest

import arith_model as A

HIPCC = "/opt/rocm/bin/hipcc"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mkhe-kklss_amd", "csrc")


def cases_of(prim, q):
    return A.uniq(A.edge_cases(prim, q))           # (without the zero padding that fills the probe's workgroups)


def stand_in(prim, c, md, mut=None):
    """pred and bflyF have no model: an exact-quotient stand-in (and its mutants) goes through the same contract check as the device's output"""
    if prim == "pred":
        return (A.pred_exact(c[0], md, mut) & A.M64,)
    U, V = A.bflyF_exact(c[0], c[1], c[2], md, mut)
    return (A.f64_bits(float(U)), A.f64_bits(float(V)))


@pytest.mark.parametrize("prim", sorted(A.PRIMS))
def test_model_meets_its_contract_on_the_edge_set(prim):
    """congruence (against % and pow) and the stated range, for every modulus of the primitive"""
    for q in A.PRIMS[prim]["moduli"]:
        md = A.Mod(q)
        for c in cases_of(prim, q):
            out = A.model(prim, c, md) or stand_in(prim, c, md)
            err, _ = A.contract(prim, c, out, md)
            assert err is None, (prim, hex(q), c, err)


def test_plain_models_against_python():
    """the models without a contract function: the value itself"""
    md = A.Mod(A.Q_TOP)
    for a, b in cases_of("mul64x64", A.Q_TOP):
        assert A.model("mul64x64", (a, b), md) == ((a * b) >> 64, (a * b) & A.M64)
    for a, b, h, l in cases_of("mac128", A.Q_TOP):
        s = ((h << 64) + l + a * b) % (1 << 128)
        assert A.model("mac128", (a, b, h, l), md) == (s >> 64, s & A.M64)
    for q in A.MODULI:
        for a, _ in cases_of("csub", q):
            want = a - q if a >= q else a
            assert A.model("csub", (a, q), A.Mod(q)) == (want,) and (a >= 2 * q or want == a % q)
    for h, q in cases_of("mod_by_estimate", A.Q_TOP):
        assert A.model("mod_by_estimate", (h, q), md) == (h % q,)
    for q in A.MODULI_INT:
        md = A.Mod(q)
        rinv = pow(1 << 64, -1, q)
        for hi, lo in cases_of("redc128", q):
            assert A.model("redc128", (hi, lo), md) == (((hi << 64) + lo) * rinv % q,)
        for a, w in cases_of("mont_mul", q)[:2000]:
            assert A.model("mont_mul", (a, w), md) == (a * w * rinv % q,)
    for v, in cases_of("u2d", A.Q_F_MAX):
        assert A.bits_f64(A.u2d(v)) == float(v) and A.d2u(float(v)) == v


def test_packings_follow_their_definitions():
    """sd_split, pack and pair_of (engine.hip): the digits decode to the value they stand for, within the digit ranges the products rely on"""
    for q in A.MODULI_INT:
        md = A.Mod(q)
        assert A.s32(A.hi32(md.qs)) * (1 << 32) + A.s32(A.lo32(md.qs)) == q
        for sh in (30, 31):
            p0, p1 = md.p(sh)
            assert p1 * (1 << sh) + p0 == q and abs(p0) <= 1 << (sh - 1)
        for uc in (False, True):
            if uc and q not in A.MODULI_U:
                continue
            sh = 30 if uc else 31
            for w in A.twiddle_edges(q, "30u" if uc else "31"):
                us, vs = A.pair_of(w, q, uc)
                u0 = A.lo32(us) if uc else A.s32(A.lo32(us))
                u1 = A.hi32(us) if uc else A.s32(A.hi32(us))
                v0, v1 = A.s32(A.lo32(vs)), A.s32(A.hi32(vs))
                assert (u1 * (1 << sh) + u0 - w * (1 << sh)) % q == 0 and (v1 * (1 << sh) + v0 - w * (1 << (sh + 32))) % q == 0
                assert -(1 << (sh - 1)) <= v0 < 1 << (sh - 1) and abs(v1 * (1 << sh) + v0) <= q // 2
                if uc:
                    assert 0 <= u0 < 1 << 30 and 0 <= u1 * (1 << 30) + u0 < q
                else:
                    assert -(1 << 30) <= u0 < 1 << 30 and abs(u1 * (1 << 31) + u0) <= q // 2


def test_extreme_packed_digits_are_reached():
    """the twiddle edges hold what they are for: a packed low digit at either end of its range, and zero, in u and in v"""
    for q in (A.MODULI_INT[1], A.MODULI_U[0]):
        for form, uc in (("31", False), ("30u", True)):
            if uc and q not in A.MODULI_U:
                continue
            sh = 30 if uc else 31
            pairs = [A.pair_of(w, q, uc) for w in A.twiddle_edges(q, form)]
            v0s = {A.s32(A.lo32(v)) for _, v in pairs}
            assert {-(1 << (sh - 1)), (1 << (sh - 1)) - 1, 0} <= v0s
            u0s = {A.lo32(u) if uc else A.s32(A.lo32(u)) for u, _ in pairs}
            assert ({0, (1 << 30) - 1, 1 << 29} if uc else {-(1 << 30), (1 << 30) - 1, 0}) <= u0s


MUTANTS = [(p, m) for p in sorted(A.PRIMS) for m in A.PRIMS[p]["muts"]]


@pytest.mark.parametrize("prim,mut", MUTANTS)
def test_edge_set_alone_catches_the_mutant(prim, mut):
    """a wrong variant of the model differs from the true model on the edge vectors of ONE modulus, without any random operand (pred, bflyF: the
    contract check rejects the wrong variant of the stand-in and accepts the true one)"""
    assert len(A.PRIMS[prim]["muts"]) >= 2
    q = A.PRIMS[prim]["moduli"][0]
    md = A.Mod(q)
    caught = 0
    for c in cases_of(prim, q):
        if A.model(prim, c, md) is None:
            assert A.contract(prim, c, stand_in(prim, c, md), md)[0] is None
            caught += A.contract(prim, c, stand_in(prim, c, md, mut), md)[0] is not None
        else:
            caught += A.model(prim, c, md, mut) != A.model(prim, c, md)
    assert caught > 0, "no edge vector tells %s[%s] from the truth" % (prim, mut)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_probe_source_compiles_for_gfx950(tmp_path):
    out = tmp_path / "arith_probe.o"
    subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-I", CSRC, "-c",
                    os.path.join(ROOT, "tests", "hip", "arith_probe.hip"), "-o", str(out)], check=True, capture_output=True, timeout=300)
    assert out.stat().st_size > 0


def test_probe_restates_no_primitive():
    """the probe instantiates the project's inline functions: it defines none of them itself, and the product ABI does not know it"""
    src = open(os.path.join(ROOT, "tests", "hip", "arith_probe.hip")).read()
    for name in ("mont_mul_lazy", "mont_mul_sd", "mont_mul_sdu", "mont_mul", "mul64x64", "mac128", "redc128", "csub", "mm", "mm31", "mm30u", "pred",
                 "bflyF", "u2d", "d2u", "canonF", "mod_by_estimate"):
        assert ("inline u64 %s(" % name) not in src and ("inline i64 %s(" % name) not in src and ("inline void %s(" % name) not in src
    assert '#include "h16_arith.h"' in src and '#include "poly_kernels.h"' in src
    assert "mkhe_arith_probe" not in open(os.path.join(ROOT, "include", "mkhe.h")).read()
