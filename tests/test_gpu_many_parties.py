"""Nine to thirty-two parties (-m gpu): the C ABI takes ciphertexts of up to 32 parties and the engine changes its launch set at party counts that the
other modules never reach (they stop at 8; test_gpu_parity.py has 10, 13 and 16 on its small rings).  Everything here is bit for bit against the oracle
on uniform operands and keys, and every case says which branch it is there for:

  n0 = parties of op0, n1 = parties of op1
  n0 in 9..16          x is still a by-product of step F1 (ext_inner_xwide_kernel), y is not (csrc/engine_mulrelin.hip: fuse_y needs n0 <= 8): step E
                       is a plain item of the tail batch
  n0 in 9..16, 2^15    ntt16_f2_kernel with f2_max_parts = 3: out_0 has n0 members in ceil(n0 / 4) virtual items, each inverse job within VI_SUMS summands
  n0 = 17              past F2_MAX_P and past the x by-product: Decompose of the t_i, plain products, x and y as inner-product launches
  2 n0 + n1 > 64       no fold (the tensor term gets its own inverse NTT) and ext_batch cuts the tail batch at EXT_MAX_ITEMS
  2^14                 the staged digits (ext_fused_ok, EXTF_MAX_V = 32 vectors)
  mkbfv, n0 > 4        no x / y / E fusion: both gadgets through the generic batch
  17+ components       pointer tables that no longer travel in the kernel arguments (ED_INLINE, CTSUM_MAX)

The case on each side of every step (ids of this module unless another is named):
  n0 = 8 | 9           test_gpu_headline.py::test_pn15_fused_f2_shapes[8-8-13-False] | test_pn15_mulrelin_across_the_thresholds[9x9-l1], [9x9-l5], [9x9-l13]
  parts 2 | 3 (VI_SUMS) test_pn15_mulrelin_across_the_thresholds[16x16-l2] | [9x9-l5]; planned | refused: [16x16-l13] | [9x9-l13], [12x12-l5]
  n0 = 16 | 17         test_pn15_mulrelin_across_the_thresholds[16x16-l2] | [17x17-l2]; test_small_ring_mulrelin[16-2] | [17-2]; test_pn15_rotate_and_conjugate[16-4] | [17-4]
  2 n0 + n1 = 63 | 66  test_pn15_mulrelin_across_the_thresholds[21x21-l1] | [22x22-l1]; test_small_ring_mulrelin[17-2] | [22-2]; the maximum: [32x32-l1], [32-2]
  2^14 staged | not    test_pn14_rotate_and_conjugate[17-1] | [32-1]; 32 staged vectors: [32-0]; MulRelin: test_gpu_parity.py::test_small_ring_mul_and_relin_staged_f2[4-1]
                       | test_pn14_mulrelin_is_not_staged_beyond_eight_parties[9-1]
  mkbfv n0 = 4 | 5     test_gpu_headline.py::test_bfv_pn15_mulrelin_new[4] | test_bfv_mulrelin[5-5]
  16 | 17 components   test_gpu_parity.py::test_mul_and_relin (16 parties) | test_add_sub_sum[17], test_rescale[17], test_lincomb[17], test_decrypt_and_noise_norm[17]

Which path ran is read from the launch counts of the context (mkhe_prof_collect), as tests/test_gpu_mulrelin_sum.py does; whether the planner takes the
fused F2 launch for a shape is asked of mkhe_f2_schedule_probe for the 256 CUs of the MI355X.

The key material of a ring is made once: four uniform switching-key arrays, and party i's key j is array j rotated along the coefficient axis by a
party- and key-specific offset (distinct data per party and key at memcpy speed, as test_pn16_mul_and_relin_eight_parties does).  The oracle is handed
the digits the level uses only (a prefix of the key: it reads nothing beyond), the device the whole key."""
import ctypes as C

import numpy as np
import pytest

import harness as H
from gpu_common import launch_counts, pset_ct, pset_swk

pytestmark = pytest.mark.gpu

F2_SEGS = 3


def _names(ids):
    return ["u%02d" % i for i in ids]          # (a ciphertext sorts its ids: the names sort as the integers do)


class World:
    """one ring on the oracle and on the device, and the bank of per-party keys"""

    def __init__(self, pset, seed):
        from oracle import oracle as O
        from mkhe_kklss_amd import mkckks, mkrlwe
        self.O, self.mk, self.mkr, self.p = O, mkckks, mkrlwe, pset
        self.N, self.top = 1 << pset["logN"], len(pset["Q"]) - 1
        self.ks = O.KeySwitcher(pset["logN"], pset["Q"], pset["P"], 2)
        self.params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], pset["scale"], device=0)
        self.ev, self.ksw = mkckks.NewEvaluator(self.params), mkrlwe.NewKeySwitcher(self.params)
        self.rng = np.random.default_rng(seed)
        self.base = [pset_swk(pset, self.rng, self.ks.beta_max) for _ in range(4)]      # b, d, v of every party and the CRS
        self.rlk = mkrlwe.RelinearizationKeySet(self.params)
        self.digits = {}                      # party -> digits of its device keys that hold data
        self.crs_up = set()

    def close(self):
        self.rlk, self.base = None, None
        self.params.close()

    def _rolled(self, j, off, nd):
        return np.ascontiguousarray(np.roll(self.base[j][:nd], off, axis=2))

    def host(self, i, j, level):
        """key j (0 b, 1 d, 2 v) of party i for the oracle: the digits of `level`"""
        return self._rolled(j, 997 * i + 131 * j + 1, self.ks.beta(level))

    def host_crs(self, idx, level):
        return self._rolled(3, 61 * (idx + 5) + 7, self.ks.beta(level))

    def need(self, ids, level):
        """the device keys of the parties, with at least the digits of `level` (the others zero: never read at that level)"""
        want = self.ks.beta(level)
        nd = self.ks.beta_max if want > 5 else min(5, self.ks.beta_max)      # (two sizes: 17 and more parties only run at the low levels of the large ring)
        shape = self.params.SwkShape()
        for i in ids:
            if self.digits.get(i, 0) >= want:
                continue
            arrs = []
            for j in range(3):
                a = np.zeros(shape, dtype=np.uint64)
                a[:nd] = np.roll(self.base[j][:nd], 997 * i + 131 * j + 1, axis=2)
                arrs.append(a)
            name = _names([i])[0]
            if i in self.digits:
                for j in range(3):
                    self.rlk.Value[name].Value[j].upload(arrs[j])
            else:
                self.rlk.AddRelinearizationKey(self.mkr.RelinearizationKey(self.params, name, *arrs))
            self.digits[i] = nd

    def crs(self, idx):
        if idx not in self.crs_up:
            self.params.AddCRS(idx, self._rolled(3, 61 * (idx + 5) + 7, self.ks.beta_max))
            self.crs_up.add(idx)

    def rlk_host(self, ids, level):
        return {i: tuple(self.host(i, j, level) for j in range(3)) for i in ids}

    def ct(self, ids, level, limbs=None):
        h = pset_ct(self.p, self.rng, len(ids), level + 1 if limbs is None else limbs)
        return h, self.mk.NewCiphertext(self.params, _names(ids), h.shape[1] - 1, self.p["scale"]).upload(h)

    def rotation_keys(self, ids, rot):
        """the rotation key of party i is its key b, the conjugation key its key d (one device array each, shared with the relinearisation key)"""
        rks, cks = self.mkr.RotationKeySet(), self.mkr.ConjugationKeySet()
        for i, n in zip(ids, _names(ids)):
            rk = object.__new__(self.mkr.RotationKey)
            rk.ID, rk.RotIdx, rk.Value = n, rot, self.rlk.Value[n].Value[0]
            rks.AddRotationKey(rk)
            ck = object.__new__(self.mkr.ConjugationKey)
            ck.ID, ck.Value = n, self.rlk.Value[n].Value[1]
            cks.AddConjugationKey(ck)
        return rks, cks

    def counts(self, fn):
        return launch_counts(self.params.ctx, fn)


def _world(pset, seed):
    from oracle import oracle as O
    O.set_threads(16)                 # limb-level threads of the oracle's loops: same integers (tests/test_oracle_vs_model.py)
    w = World(pset, seed)
    try:
        yield w
    finally:
        O.set_threads(1)
        w.close()


@pytest.fixture(scope="module")
def pn15():
    yield from _world(H.PN15QP880, 0x15932)


@pytest.fixture(scope="module")
def pn14():
    yield from _world(H.PN14QP439, 0x14932)


@pytest.fixture(scope="module")
def s11():
    yield from _world(H.small_ckks(11, 3), 0x11932)


@pytest.fixture(scope="module")
def a12():
    yield from _world(H.small_alpha2(12, 3), 0x12932)


@pytest.fixture(scope="module")
def a16():
    yield from _world(H.small_alpha2(16, 3), 0x16932)


# ---------------------------------------------------------------- which path a shape takes, from the engine's own rules
CUS = 256         # the MI355X: the grid ntt16_f2_grid() plans for (another device cuts differently, and the launch counts below would say so)


def _f2_plan(parties, level, nP=2):
    """(workgroups, parts) of the engine's plan for the fused F2 launch of `parties` digit vectors at `level` on the MI355X; (0, 0): not taken"""
    from mkhe_kklss_amd._abi import lib
    grid = CUS
    nb, nslots = level + 1, level + 1 + nP
    w = (C.c_long * nslots)(*([100] * nslots))
    segs = (C.c_ubyte * (grid * F2_SEGS * 8))()
    parts = C.c_int(0)
    nwg = lib().mkhe_f2_schedule_probe(parties, nb, nslots, w, -grid, segs, C.byref(parts))
    return nwg, parts.value


def _f2(counts):
    return sum(v for k, v in counts.items() if k.startswith("ntt16_f2_kernel"))


def _decomp(counts):
    return {k: v for k, v in counts.items() if "Decompose" in k and not k.startswith("ntt16_f2_kernel") and v}


def _inner_launches(n0, n1):
    """key_inner_product launches of one MulAndRelin: y unless the F1 kernel computes it, x unless it is F1's by-product (csrc/engine_mulrelin.hip)"""
    x_fused = 1 <= n0 <= 16
    y_fused = x_fused and n1 >= 1 and (n1 <= 4 if n0 <= 4 else (n0 <= 8 and n1 == n0))
    return (0 if y_fused or n1 == 0 else 1) + (0 if x_fused or n0 == 0 else 1)


def _staged(counts):
    """N = 2^14 with the caller's hoisted forms: the one Decompose of the call left its digits after the cross stages (the staged form) -- a full
    Decompose of this chain has a launch of the big-modulus class or of the 16-coefficient kernel (tests/test_gpu_mulrelin_sum.py)"""
    d = _decomp(counts)
    return list(d.values()) == [1] and next(iter(d)).startswith("ntt_fwd_kernel<N,1,true>")


# ---------------------------------------------------------------- 1. MK-CKKS MulRelin
def _mulrelin(w, ids0, ids1, level, fused=None, batch=False):
    """MulRelinNew, MulRelinHoistedNew on the caller's hoisted forms and the un-rescaled MulAndRelin of one shape against ONE oracle evaluation, each
    twice (the second through the warm pools).  fused: None = not the 2^15 ring; else whether ntt16_f2_kernel has to be the launch that ran."""
    w.need(sorted(set(ids0) | set(ids1)), level)
    w.crs(-1)
    p, ks, ev = w.p, w.ks, w.ev
    n0, n1 = len(ids0), len(ids1)
    (h0, ct0), (h1, ct1) = w.ct(ids0, level), w.ct(ids1, level)
    allids = sorted(set(ids0) | set(ids1))
    oids, ref = ks.mul_and_relin(level, ids0, h0, ids1, h1, w.rlk_host(allids, level), w.host_crs(-1, level))
    assert oids == allids
    nb, _ = ks.ckks_nb_rescales(level, p["scale"] * p["scale"], p["scale"])
    ref_r = np.stack([ks.ringQ.div_round_last_many(ref[s], nb)[0] for s in range(ref.shape[0])]) if nb else ref
    res = {}
    c_new = w.counts(lambda: res.update(new=ev.MulRelinNew(ct0, ct1, w.rlk)))
    assert res["new"].Level() == level - nb and res["new"].ids == _names(allids)
    got = res["new"].download()
    assert got.shape == ref_r.shape and (got == ref_r).all()
    assert (ev.MulRelinNew(ct0, ct1, w.rlk).download() == ref_r).all()                                          # warm pools, same bits
    hf0, hf1 = ev.HoistedForm(ct0), ev.HoistedForm(ct1)
    c_hoisted = w.counts(lambda: res.update(hoisted=ev.MulRelinHoistedNew(ct0, ct1, hf0, hf1, w.rlk)))
    assert (res["hoisted"].download() == ref_r).all()
    assert (ev.MulRelinHoistedNew(ct0, ct1, hf0, hf1, w.rlk).download() == ref_r).all()
    out = w.mkr.NewCiphertext(w.params, _names(allids), level)
    c_plain = w.counts(lambda: w.ksw.MulAndRelin(ct0, ct1, w.rlk, out))
    assert (out.download() == ref).all()
    w.ksw.MulAndRelin(ct0, ct1, w.rlk, out)
    assert (out.download() == ref).all()
    for c in (c_new, c_hoisted, c_plain):
        print("n0=%d n1=%d level=%d launches: %r" % (n0, n1, level, {k.split("  ")[0]: v for k, v in c.items() if v}))
        assert c["inner_product_kernel"] == _inner_launches(n0, n1), c
        assert c["tensor_kernel"] == 1, c
        if fused is not None:
            assert _f2(c) == (1 if fused else 0), c
    if fused is not None:
        # the caller's hoisted forms: the only Decompose left is that of the t_i -- none when their digits stay in registers
        assert (not _decomp(c_hoisted)) == fused, c_hoisted
    if batch:
        # mkhe_mul_relin_batch, B = 2: two inputs of this shape; every output equal to the single evaluation's
        (g0, cb0), (g1, cb1) = w.ct(ids0, level), w.ct(ids1, level)
        b0, b1 = w.mk.BatchCiphertext([ct0, cb0]), w.mk.BatchCiphertext([ct1, cb1])
        single = [ref_r, ev.MulRelinNew(cb0, cb1, w.rlk).download()]
        bev = w.mk.BatchEvaluator(w.params, 2)
        for _ in range(2):
            bo = bev.MulRelinNew(b0, b1, w.rlk)
            for i in range(2):
                assert (bo.cts[i].download() == single[i]).all(), i
    return c_hoisted


PN15_CASES = [
    # (ids0, ids1, level, the planner has to take the fused F2 launch on a 256-CU device)
    pytest.param(range(9), range(9), 1, True, id="9x9-l1"),            # lower edge of the 9..16 band, the floor of f2_plan_schedule (two digits); B = 2 batch
    pytest.param(range(9), range(9), 5, True, id="9x9-l5"),            # three parts per product: 4 members x 3 parts + the tensor term = VI_SUMS at out_0
    pytest.param(range(9), range(9), 13, False, id="9x9-l13"),         # the benchmark's digits and limb slots; the planner refuses: x by-product, step E and the t_i as launches
    pytest.param(range(12), range(12), 5, False, id="12x12-l5"),       # inside the band, refused by the planner: Decompose of the t_i + ext_inner over 36 items
    pytest.param(range(16), range(16), 2, True, id="16x16-l2"),        # upper edge of the band (F2_MAX_P), 48 items + 32 part slots in c1
    pytest.param(range(16), range(16), 13, True, id="16x16-l13"),      # upper edge at the benchmark's level: every workgroup of the chip, one run each
    pytest.param(range(16), range(3), 4, True, id="16x3-l4"),          # wide op0: step E has 3 items, 13 output slots without one
    pytest.param(range(3), range(16), 4, None, id="3x16-l4"),          # wide op1: step E has 16 items (y is a launch: n1 > 4), out_0 has 3 members
    pytest.param(range(13), [11, 12] + list(range(13, 24)), 6, True, id="13x13-two-shared-l6"),      # slots with 2 members (u + tensor), 3 (u + E + tensor) and E alone
    pytest.param(range(17), range(17), 2, False, id="17x17-l2"),       # first shape past F2_MAX_P and past the x by-product: the full unfused launch set
    pytest.param(range(21), range(21), 1, False, id="21x21-l1"),       # 63 items: the last folded tail batch
    pytest.param(range(22), range(22), 1, False, id="22x22-l1"),       # 66 items: no fold, the tensor term's own inverse NTT, the batch cut at 64
    pytest.param(range(32), range(32), 1, False, id="32x32-l1"),       # the maximum: 96 items, 64 Decompose items in one launch
]


@pytest.mark.parametrize("ids0,ids1,level,must_fuse", PN15_CASES)
def test_pn15_mulrelin_across_the_thresholds(pn15, ids0, ids1, level, must_fuse):
    ids0, ids1 = list(ids0), list(ids1)
    n0, n1 = len(ids0), len(ids1)
    plan = _f2_plan(n0, level) if n0 <= 16 and 2 * n0 + n1 <= 64 else (0, 0)
    fused = plan[0] > 0
    print("plan of ntt16_f2_kernel on %d CUs: %r" % (CUS, plan))
    if must_fuse is not None:
        assert fused == must_fuse, plan          # (what the case is there for)
    _mulrelin(pn15, ids0, ids1, level, fused=fused, batch=(n0, level) == (9, 1))


@pytest.mark.parametrize("level", [2, 0])
@pytest.mark.parametrize("n", [9, 16, 17, 22, 32])
def test_small_ring_mulrelin(s11, n, level):
    # N = 2^11, alpha = 1: the generic batch on both sides of n0 = 16 (x by-product), 2 n0 + n1 = 64 (fold, the cut of the batch) and at the maximum;
    # 17, 22 and 32 parties also as B = 2 inputs of mkhe_mul_relin_batch in lock step (one operation per tail launch: 51, 66 and 96 items)
    _mulrelin(s11, list(range(n)), list(range(n)), level, batch=level == 2 and n >= 17)


@pytest.mark.parametrize("level", [1, 5])
@pytest.mark.parametrize("n", [9, 17, 32])
def test_pn14_mulrelin_is_not_staged_beyond_eight_parties(pn14, n, level):
    # N = 2^14: the t_i are left after the cross stages only when step E is no item of the tail batch (mr_f2_hoist: e_free), and step E is one from
    # nine parties on -- whatever ext_fused_ok says of the shape (9 and 17 vectors at level 1 are within its 150 limbs), the full Decompose runs
    c = _mulrelin(pn14, list(range(n)), list(range(n)), level)
    assert _decomp(c) and not _staged(c), c


@pytest.mark.parametrize("n", [9, 17, 32])
def test_alpha2_mulrelin(a12, n):
    # alpha = 2 (CRT-reconstructed digits): decomp_spread over 18, 34 and 64 operand components (DEC_MAX_ITEMS = 64: one launch, full)
    _mulrelin(a12, list(range(n)), list(range(n)), a12.top)


# ---------------------------------------------------------------- 2. Rotate, RotateHoisted, Conjugate, rotate-and-add
def _rotate(w, n, level, fused=None, staged=None, and_add=False):
    """RotateNew (the engine hoists), RotateHoistedNew on the caller's hoisted form and ConjugateNew of an n-party ciphertext against the oracle,
    each twice; and_add: mkhe_rotate_multi with the input as post_add = ct + Rotate(ct)"""
    ids, rot = list(range(n)), 5
    w.need(ids, level)
    w.crs(rot)
    w.crs(-2)
    ks, ev = w.ks, w.ev
    h, ct = w.ct(ids, level)
    rks, cks = w.rotation_keys(ids, rot)
    rk_h, ck_h = [w.host(i, 0, level) for i in ids], [w.host(i, 1, level) for i in ids]
    ref = ks.rotate(level, pow(5, rot, 2 * w.N), ids, h, rk_h, w.host_crs(rot, level))
    res = {}
    c_rot = w.counts(lambda: res.update(rot=ev.RotateNew(ct, rot, rks)))
    assert (res["rot"].download() == ref).all()
    assert (ev.RotateNew(ct, rot, rks).download() == ref).all()
    hf = ev.HoistedForm(ct)
    assert (ev.RotateHoistedNew(ct, rot, hf, rks).download() == ref).all()
    assert (ev.RotateHoistedNew(ct, rot, hf, rks).download() == ref).all()
    cref = ks.conjugate(level, 2 * w.N - 1, ids, h, ck_h, w.host_crs(-2, level))
    c_conj = w.counts(lambda: res.update(conj=ev.ConjugateNew(ct, cks)))
    assert (res["conj"].download() == cref).all()
    assert (ev.ConjugateNew(ct, cks).download() == cref).all()
    assert (ct.download() == h).all()
    for c in (c_rot, c_conj):
        print("n=%d level=%d launches: %r" % (n, level, {k.split("  ")[0]: v for k, v in c.items() if v}))
        if fused is not None:
            assert _f2(c) == (1 if fused else 0) and (not _decomp(c)) == fused, c
        if staged is not None:
            assert _staged(c) == staged, c
    if and_add:
        rq = ks.ringQ
        sref = np.stack([np.stack([rq.add(l, h[s][l], ref[s][l]) for l in range(level + 1)]) for s in range(1 + n)])
        assert (ev.RotateAndAddNew(ct, rot, rks).download() == sref).all()
        assert (ev.RotateAndAddNew(ct, rot, rks).download() == sref).all()


@pytest.mark.parametrize("level", [1, 4])
@pytest.mark.parametrize("n", [9, 16, 17, 32])
def test_pn15_rotate_and_conjugate(pn15, n, level):
    # N = 2^15 without a hoisted form: ntt16_f2_kernel over n digit vectors where the planner takes the shape (n <= F2_MAX_P), the Decompose launch and
    # ext_inner over 2 n items otherwise; 32 parties = 64 items, the most a fused rotation takes (rotate: 2 n <= EXT_MAX_ITEMS)
    fused = n <= 16 and _f2_plan(n, level)[0] > 0
    assert fused == ((n, level) in ((9, 1), (9, 4), (16, 1), (16, 4)))
    _rotate(pn15, n, level, fused=fused)


@pytest.mark.parametrize("level", [0, 1, 5])
@pytest.mark.parametrize("n", [9, 16, 17, 32])
def test_pn14_rotate_and_conjugate(pn14, n, level):
    # N = 2^14: the staged digits while n * digits * limb slots <= 150 (ext_fused_ok) -- at level 0 up to EXTF_MAX_V = 32 vectors with two keys each
    # (32 x 1 x 3 = 96 limbs), at level 1 seventeen vectors (136 limbs) and not thirty-two (256) -- and the full Decompose at the top level
    nslots = level + 1 + len(pn14.p["P"])
    _rotate(pn14, n, level, staged=n * (level + 1) * nslots <= 150)


@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("n", [9, 16, 17, 32])
def test_small_ring_rotate_and_conjugate(s11, n, level):
    # N = 2^11: out_0 with n members in ceil(n / 4) virtual items of the merged ModDown; 16 and 32 parties also through mkhe_rotate_multi with post_add
    _rotate(s11, n, level, and_add=n in (16, 32))


@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("n", [9, 16, 17, 32])
def test_alpha2_rotate_and_conjugate(a12, n, level):
    # alpha = 2, four special primes: four members per virtual item is the most 16 / nP allows; a one-limb digit at level 0 and a last one at level 2
    _rotate(a12, n, level)


@pytest.mark.parametrize("n", [12, 32])
def test_pn16_head_rotate_and_conjugate(a16, n):
    # N = 2^16 at the first three Q primes of the PN16 chain (alpha = 2): the split NTT and decomp_spread's fused first stages over 12 and 32 vectors
    _rotate(a16, n, a16.top)


# ---------------------------------------------------------------- 3. MK-BFV: no x / y / E fusion beyond four parties, both gadgets through the generic batch
class BfvWorld:
    def __init__(self, pset):
        import harness_bfv as HB
        from mkhe_kklss_amd import mkbfv, mkrlwe
        from mkhe_kklss_amd._abi import handle_array, lib
        self.HB, self.mkb, self.mkr, self.lib, self.handle_array = HB, mkbfv, mkrlwe, lib(), handle_array
        self.pset, self.bfv = pset, HB.make_bfv(pset)
        self.params = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], pset["T"])
        self.ev = mkbfv.NewEvaluator(self.params)
        self.N, self.top = 1 << pset["logN"], len(pset["Q"]) - 1

    def material(self, parties, seed):
        """uniform operands, relinearisation keys and CRS of `parties` parties on both sides"""
        data = self.HB.uniform_bfv_inputs(self.pset, parties, seed)
        rlk = self.mkb.NewRelinearizationKeyKeySet(self.params)
        for i, n in enumerate(_names(range(parties))):
            rlk.AddRelinearizationKey(self.mkb.RelinearizationKey(self.params, n, *data["rlk"][i]))
        self.params.AddCRS(-1, data["u"])
        return data, rlk

    def ct(self, ids, host):
        return self.mkb.NewCiphertext(self.params, _names(ids)).upload(np.ascontiguousarray(host))


@pytest.fixture(scope="module")
def bfv():
    import harness_bfv as HB
    w = BfvWorld(HB.small_bfv(11, 3))             # T = 65537, as tests/test_gpu_bfv.py
    yield w
    w.params.close()


@pytest.mark.parametrize("n0,n1", [(5, 5), (8, 8), (9, 9), (16, 16), (17, 17), (32, 32), (16, 3)])
def test_bfv_mulrelin(bfv, n0, n1):
    # five parties: the first count without the fused x / y / E of the group kernel (csrc/engine_bfv.hip); 8 | 9 and 16 | 17: the steps the CKKS engine
    # changes at (nothing may change here); 32: 96 two-gadget items, the batch cut at EXT_MAX_ITEMS; (16, 3): unequal slot sets
    data, rlk = bfv.material(max(n0, n1), 0xBF00 + 64 * n0 + n1)
    ids0, ids1 = list(range(n0)), list(range(n1))
    h0, h1 = data["op0"][: 1 + n0], data["op1"][: 1 + n1]
    c0, c1 = bfv.ct(ids0, h0), bfv.ct(ids1, h1)
    oids, ref = bfv.bfv.mul_relin_new(ids0, h0, ids1, h1, data["rlk"], data["u"])
    out = bfv.ev.MulRelinNew(c0, c1, rlk)                    # the operands hoisted by the engine (DecomposeBFV + MulAndRelinBFVHoisted)
    assert out.ids == _names(oids) and (out.download() == ref).all()
    assert (bfv.ev.MulRelinNew(c0, c1, rlk).download() == ref).all()
    un = bfv.ev.mulRelin(c0, c1, rlk)                        # the non-hoisted twin, its own device path
    assert un.ids == out.ids and (un.download() == ref).all()
    assert (bfv.ev.mulRelin(c0, c1, rlk).download() == ref).all()
    assert (c0.download() == h0).all() and (c1.download() == h1).all()


@pytest.mark.parametrize("n", [9, 17])
def test_bfv_mulrelin_sum_of_two(bfv, n):
    # mkhe_bfv_mul_relin_sum, K = 2: the summed t_i of 9 and 17 parties under one Quantize and one tail (csrc/engine_bfv_sum.hip: no fused y / E here)
    import bfv_mulrelin_sum_model as BM
    data, rlk = bfv.material(n, 0xBF50 + n)
    rng = np.random.default_rng(n)
    ids = list(range(n))
    hosts0 = [data["op0"], H.uniform_ct(rng, bfv.bfv.ks, n, bfv.top + 1)]
    hosts1 = [data["op1"], H.uniform_ct(rng, bfv.bfv.ks, n, bfv.top + 1)]
    d0, d1 = [bfv.ct(ids, h) for h in hosts0], [bfv.ct(ids, h) for h in hosts1]
    out = bfv.mkb.NewCiphertext(bfv.params, _names(ids))
    ha = bfv.handle_array
    key = lambda i, g, j: rlk.GetRelinearizationKey(i).Value[g].Value[j].h
    names = _names(ids)
    rc = bfv.lib.mkhe_bfv_mul_relin_sum(bfv.params.ctx, 2, ha([c.h for c in d0]), ha([c.h for c in d1]),
                                        ha([key(i, 0, 0) for i in names]), ha([key(i, 1, 0) for i in names]),
                                        ha([key(i, 0, 1) for i in names]), ha([key(i, 1, 1) for i in names]), ha([key(i, 0, 2) for i in names]),
                                        bfv.params.CRS[-1].h, out.h)
    assert rc == 0, bfv.lib.mkhe_last_error().decode()
    oids, ref = BM.bfv_mul_relin_sum(bfv.bfv, ids, hosts0, ids, hosts1, data["rlk"], data["u"])
    assert oids == ids and (out.download() == ref).all()


@pytest.mark.parametrize("n", [9, 32])
def test_bfv_rotate(bfv, n):
    # mkbfv Rotate = the mkrlwe key switch on a BFV context (no staged digits, no fused F2 there: is_bfv), 9 and 32 parties
    rng = np.random.default_rng(0xBF70 + n)
    ks, ids, rot = bfv.bfv.ks, list(range(n)), 3
    h = H.uniform_ct(rng, ks, n, bfv.top + 1)
    c = bfv.ct(ids, h)
    rk_h, rk_d = [], bfv.mkr.RotationKeySet()
    for name in _names(ids):
        rk_h.append(H.uniform_swk(rng, ks))
        rk_d.AddRotationKey(bfv.mkr.RotationKey(bfv.params, rot, name, rk_h[-1]))
    crs_h = H.uniform_swk(rng, ks)
    bfv.params.AddCRS(rot, crs_h)
    ref = ks.rotate(bfv.top, pow(5, rot, 2 * bfv.N), ids, h, rk_h, crs_h)
    assert (bfv.ev.RotateNew(c, rot, rk_d).download() == ref).all()
    assert (bfv.ev.RotateNew(c, rot, rk_d).download() == ref).all()


# ---------------------------------------------------------------- 4. elementwise and protocol calls on 18 and 33 components
@pytest.fixture(scope="module")
def e10():
    yield from _world(H.small_ckks(10, 3), 0x10932)


def _slots(ids, h):
    return {i: h[1 + a] for a, i in enumerate(ids)}


@pytest.mark.parametrize("n", [17, 32])
def test_add_sub_sum(e10, n):
    # mkhe_ct_add / mkhe_ct_sub on overlapping id sets whose union has n parties (slots of op0 alone, of both and of op1 alone) and mkhe_ct_sum of
    # three n-party ciphertexts: 1 + n polynomials per operand, more than the 16 pointers a table holds inline
    w, rq, L = e10, e10.ks.ringQ, e10.top + 1
    ids0, ids1 = list(range(0, n - 4)), list(range(4, n))
    (h0, c0), (h1, c1) = w.ct(ids0, w.top), w.ct(ids1, w.top)
    add, sub = w.ev.AddNew(c0, c1), w.ev.SubNew(c0, c1)
    assert add.ids == sub.ids == _names(range(n))
    ga, gs = add.download(), sub.download()
    f = lambda fn, x, y: np.stack([getattr(rq, fn)(j, x[j], y[j]) for j in range(L)])
    neg = lambda x: np.stack([rq.neg(j, x[j]) for j in range(L)])
    assert (ga[0] == f("add", h0[0], h1[0])).all() and (gs[0] == f("sub", h0[0], h1[0])).all()
    s0, s1 = _slots(ids0, h0), _slots(ids1, h1)
    for i in range(n):
        if i in s0 and i in s1:
            assert (ga[1 + i] == f("add", s0[i], s1[i])).all() and (gs[1 + i] == f("sub", s0[i], s1[i])).all(), i
        elif i in s0:
            assert (ga[1 + i] == s0[i]).all() and (gs[1 + i] == s0[i]).all(), i
        else:
            assert (ga[1 + i] == s1[i]).all() and (gs[1 + i] == neg(s1[i])).all(), i
    ids = list(range(n))
    three = [w.ct(ids, w.top) for _ in range(3)]
    got = w.ev.SumNew([c for _, c in three]).download()
    ref = np.stack([f("add", f("add", three[0][0][s], three[1][0][s]), three[2][0][s]) for s in range(1 + n)])
    assert (got == ref).all()


@pytest.mark.parametrize("n", [17, 32])
def test_rescale(e10, n):
    # mkhe_rescale of 1 + n polynomials by one and by two moduli (DivRoundByLastModulusManyLvl)
    from mkhe_kklss_amd._abi import check, lib
    w = e10
    h, c = w.ct(list(range(n)), w.top)
    for nb in (1, 2):
        out = w.mkr.NewCiphertext(w.params, _names(range(n)), w.top - nb)
        check(lib().mkhe_rescale(w.params.ctx, c.h, nb, out.h))
        got = out.download()
        for s in range(1 + n):
            assert (got[s] == w.ks.ringQ.div_round_last_many(h[s], nb)[0]).all(), s
    assert (c.download() == h).all()


@pytest.mark.parametrize("n", [17, 32])
def test_lincomb(n):
    # mkhe_ct_lincomb of three n-party ciphertexts with complex weights and a constant, with and without the division by the last modulus, against the
    # integer model of tests/test_gpu_lincomb.py
    import test_gpu_lincomb as TL
    w = TL.World(H.small_ckks(10, nq=3))
    try:
        for nb in (0, 1):
            rng = np.random.default_rng([n, nb])
            hosts, add, weights = TL.draw(rng, w.Q, w.N, 3, 1 + n, 3, 3)
            TL.check(w, hosts, add, weights, 3, nb, _names(range(n)))
    finally:
        w.params.close()


@pytest.mark.parametrize("n", [17, 32])
def test_decrypt_and_noise_norm(e10, n):
    # mkhe_decrypt with the secret keys of n parties (the key and component pointer tables past ED_INLINE = 16) against the host restatement of
    # decryptor.go:48-66, and mkhe_noise_norm of that phase (the exact centred max norm) against tests/noise_model.py
    import noise_model as NM
    w = e10
    ids = list(range(n))
    names = _names(ids)
    kgen, dec, okg = w.mkr.NewKeyGenerator(w.params), w.mkr.NewDecryptor(w.params), w.O.KeyGen(w.ks)
    sks, sk_h = w.mkr.SecretKeySet(), {}
    for name in names:
        s = w.rng.choice(np.array([-1, 0, 0, 1], dtype=np.int32), w.N)
        sks.AddSecretKey(kgen.GenSecretKey(name, s))
        sk_h[name] = okg.gen_secret_key(s)[: w.top + 1]
    h, c = w.ct(ids, w.top)
    vals = {"0": h[0]}
    vals.update({name: h[1 + a] for a, name in enumerate(names)})
    want = H.KeyGen(w.ks).decrypt(vals, sk_h)
    assert (dec.Decrypt(c, sks).download()[0] == want).all()
    assert dec.NoiseNorm(c, sks) == NM.noise_norm_crt(0, want.tolist(), None, w.p["Q"])[0]
    ref = H.uniform_poly(w.rng, w.p["Q"], w.N)
    assert dec.NoiseNorm(c, sks, ref) == NM.noise_norm_crt(0, want.tolist(), ref.tolist(), w.p["Q"])[0]
