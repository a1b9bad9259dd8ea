"""Key switching with steered accumulators (-m gpu): the ModDown family and the alpha >= 2 digit lift at the values where they can be wrong.

Uniform ciphertexts and keys reach every launch shape and none of these values: a float64 correction index that sits on an integer (the last table
entry v = np included), a ModDown result of exactly 0 under a sign-flipping automorphism (stored as q, read back by the accumulate and the fused-add
branches), accumulators of q - 1 at every NTT point, a fused Rescale on its rounding boundary.  A compensated key (tests/steer_model.py)
puts a chosen polynomial in front of ModDown while digits and keys stay uniform; tests/test_steer_model.py proves on the CPU that the plant arrives
and which index the reference takes.  Every comparison here is bit for bit against the oracle over the whole output."""
import numpy as np
import pytest

import harness as H
import steer_model as S
from gpu_common import Pair

pytestmark = pytest.mark.gpu

LOGN = 11


def _pn16(nP):
    return dict(logN=LOGN, Q=H.PN16_Q[:4], P=H.PN16_P[:nP], scale=float(1 << 45))


SETS = {
    "ckks_np2": (H.small_ckks(LOGN, 4), 2),            # alpha 1, np 2
    "alpha2_np4": (H.small_alpha2(LOGN, 5), 2),        # alpha 2, np 4
    "pn16_np1_g1": (_pn16(1), 1),                      # v from a single term
    "pn16_np3_g3": (_pn16(3), 3),
    "pn16_np3_g1": (_pn16(3), 1),                      # alpha 3
}


@pytest.fixture(scope="module")
def pairs():
    made = {}

    def get(name):
        if name not in made:
            pset, gamma = SETS[name] if name in SETS else (H.PN14QP439, 2)
            made[name] = Pair(pset, seed=len(made) + 1, gamma=gamma)
        return made[name]
    yield get
    for p in made.values():
        p.params.close()


def _steered(build, seed):
    """build(rng) with the next seed whenever a digit 0 has a zero coefficient (steer_model.compensate): nothing is ever left out of a comparison"""
    while True:
        try:
            return build(np.random.default_rng(seed))
        except ValueError:
            seed += 1000


def _plan(pair, level, seed=0, **kw):
    return S.Plan(pair.Q, pair.P, pair.logN, level, seed=seed, **kw)


# ------------------------------------------------------------------ ExternalProduct, ExternalProductHoisted
@pytest.mark.parametrize("drop", [0, 1])
@pytest.mark.parametrize("name", list(SETS))
def test_external_product_on_planted_accumulators(pairs, name, drop):
    """moddown_kernel / moddown_batch_kernel behind one product: every planted pattern with x_q = 0, q - 1 and the zero result, every special-prime
    count of the merged kernel's instantiations"""
    pair = pairs(name)
    mk, ks, level = pair.mk, pair.ks, pair.maxlevel - drop
    plan = _plan(pair, level, seed=drop)

    def build(rng):
        a = H.uniform_ct(rng, ks, 1, pair.maxlevel + 1)
        return a, S.steer(ks, level, ks.decompose(level, a[1][: level + 1]), rng, plan.target(rng), H.uniform_swk)
    a, bg = _steered(build, 100 + drop)
    ref = ks.external_product(level, a[1][: level + 1], bg)
    assert all((ref[:, n] == 0).all() for n in plan.zero_positions())
    dev = mk.NewCiphertext(pair.params, ["u0"], pair.maxlevel).upload(a)
    bg_d = mk.SwitchingKey(pair.params, bg)
    out = mk.NewCiphertext(pair.params, ["u0"], level)
    pair.ksw.ExternalProduct(level, dev, "u0", bg_d, out, "0")
    assert (out.download()[0] == ref).all()
    ad = mk.NewSwitchingKey(pair.params)
    pair.ksw.Decompose(level, dev, "u0", ad)
    pair.ksw.ExternalProductHoisted(level, ad, bg_d, out, "u0")
    assert (out.download()[1] == ref).all()


# ------------------------------------------------------------------ Rotate, RotateHoisted, Conjugate
def _rotation_keys(pair, names, rot, keys, crs):
    pair.params.AddCRS(rot, crs)
    rkset = pair.mk.RotationKeySet()
    for i, k in zip(names, keys):
        rkset.AddRotationKey(pair.mk.RotationKey(pair.params, rot, i, k))
    return rkset


@pytest.mark.parametrize("parties", [1, 2, 4, 5])
def test_rotate_family_on_planted_accumulators(pairs, parties):
    """One target per party (the members of the merged destination out_0), the CRS steered for the last party.  At the planted coefficients every
    member's result and c_0 are 0 and rotations 1 and 5 flip the sign: out_0 and the last party's component hold q (asserted on the oracle's
    output); with five parties a second virtual item accumulates onto out_0 and reads that q back.  Conjugate: the same with the permutation first."""
    pair = pairs("ckks_np2")
    mk, ks, level = pair.mk, pair.ks, pair.maxlevel
    names = ["p%d" % i for i in range(parties)]
    plan = _plan(pair, level, seed=parties)
    ct, keys, crs = _steered(lambda rng: S.rotate_case(ks, plan, level, parties, rng, H), 200 + parties)
    d = mk.NewCiphertext(pair.params, names, level).upload(ct)
    hh = mk.NewHoistedCiphertext()
    for i in names:
        hh.Value[i] = mk.NewSwitchingKey(pair.params)
        pair.ksw.Decompose(level, d, i, hh.Value[i])
    for rot in (1, 5):
        gal = pow(5, rot, 2 * pair.N)
        ref = ks.rotate(level, gal, list(range(parties)), ct, keys, crs)
        for n in plan.zero_positions()[:-1]:
            dst = (n * gal) & (pair.N - 1)
            assert [int(x) for x in ref[0][:, dst]] == ks.Q[: level + 1] and [int(x) for x in ref[parties][:, dst]] == ks.Q[: level + 1]
        assert (ref[0][:, 0] == 0).all()
        rkset = _rotation_keys(pair, names, rot, keys, crs)
        out = mk.NewCiphertext(pair.params, names, level)
        pair.ksw.Rotate(d, rot, rkset, out)
        assert (out.download() == ref).all(), rot
        out = mk.NewCiphertext(pair.params, names, level)
        pair.ksw.RotateHoisted(d, rot, hh, rkset, out)
        assert (out.download() == ref).all(), rot
    gal = 2 * pair.N - 1
    ct, keys, crs = _steered(lambda rng: S.rotate_case(ks, plan, level, parties, rng, H, conj_gal=gal, shift=True), 300 + parties)
    d = mk.NewCiphertext(pair.params, names, level).upload(ct)
    pair.params.AddCRS(-2, crs)
    ckset = mk.ConjugationKeySet()
    for i, k in zip(names, keys):
        ckset.AddConjugationKey(mk.ConjugationKey(pair.params, i, k))
    out = mk.NewCiphertext(pair.params, names, level)
    pair.ksw.Conjugate(d, ckset, out)
    assert (out.download() == ks.conjugate(level, gal, list(range(parties)), ct, keys, crs)).all()


@pytest.mark.parametrize("parties", [2, 5])
def test_rotate_and_add_reads_a_stored_q_under_a_foreign_addend(pairs, parties):
    """RotateAndAddNew (the addend is the input) and mkhe_rotate_multi with a foreign addend whose coefficients under the flipped zeros hold 0 and
    q - 1: csub(post + q, q) must give 0 and q - 1 (the `post` path of the ModDown store), against the oracle's Rotate followed by ring.Add"""
    from mkhe_kklss_amd import mkckks
    pair = pairs("ckks_np2")
    ks, level, scale = pair.ks, pair.maxlevel, 2.0 ** 40
    names = ["p%d" % i for i in range(parties)]
    plan = _plan(pair, level, seed=10 + parties)
    ct, keys, crs = _steered(lambda rng: S.rotate_case(ks, plan, level, parties, rng, H), 400 + parties)
    rots = [1, 5]
    rtk = pair.mk.RotationKeySet()
    for rot in rots:
        pair.params.AddCRS(rot, crs)
        for i, k in zip(names, keys):
            rtk.AddRotationKey(pair.mk.RotationKey(pair.params, rot, i, k))
    ev = mkckks.Evaluator.__new__(mkckks.Evaluator)
    ev.params, ev.ksw, ev.fuse_rescale = pair.params, pair.ksw, True
    rng = np.random.default_rng(parties)
    add = [H.uniform_ct(rng, ks, parties, level + 1) for _ in rots]
    for b, rot in enumerate(rots):
        for k, n in enumerate(plan.zero_positions()):
            dst = (n * pow(5, rot, 2 * pair.N)) & (pair.N - 1)
            add[b][:, :, dst] = 0 if k % 2 == 0 else np.array(ks.Q[: level + 1], dtype=np.uint64)[None, :] - np.uint64(1)

    def ref(hadd, rot):
        o = ks.rotate(level, pow(5, rot, 2 * pair.N), list(range(parties)), ct, keys, crs)
        return np.stack([np.stack([ks.ringQ.add(j, hadd[s, j], o[s, j]) for j in range(level + 1)]) for s in range(1 + parties)])
    c = mkckks.NewCiphertext(pair.params, names, level, scale).upload(ct)
    for rot in rots:
        assert (ev.RotateAndAddNew(c, rot, rtk).download() == ref(ct, rot)).all(), rot
    bev = mkckks.BatchEvaluator(pair.params, len(rots), ev=ev)
    post = mkckks.BatchCiphertext([mkckks.NewCiphertext(pair.params, names, level, scale).upload(a) for a in add])
    got = bev._rotate_multi(c, rots, None, rtk, post)
    for b, rot in enumerate(rots):
        want = ref(add[b], rot)
        assert all((want[:, j] < np.uint64(q)).all() for j, q in enumerate(ks.Q[: level + 1]))
        assert (got.cts[b].download() == want).all(), rot


def test_small_ring_rotate_on_planted_accumulators(pairs):
    """PN14QP439, two parties at level 1, no hoisted form: ext_fused_lds_kernel in front of the same ModDown"""
    pair = pairs("pn14")
    mk, ks, level, names, rot = pair.mk, pair.ks, 1, ["p0", "p1"], 5
    plan = _plan(pair, level, seed=14)
    ct, keys, crs = _steered(lambda rng: S.rotate_case(ks, plan, level, 2, rng, H), 1400)
    d = mk.NewCiphertext(pair.params, names, level).upload(ct)
    rkset = _rotation_keys(pair, names, rot, keys, crs)
    out = mk.NewCiphertext(pair.params, names, level)
    pair.ksw.Rotate(d, rot, rkset, out)
    ref = ks.rotate(level, pow(5, rot, 2 * pair.N), [0, 1], ct, keys, crs)
    assert any((ref[0][j] == np.uint64(q)).any() for j, q in enumerate(ks.Q[: level + 1]))
    assert (out.download() == ref).all()


# ------------------------------------------------------------------ MulAndRelin, mkhe_mul_relin_rescale
@pytest.mark.parametrize("all_max", [False, True], ids=["planted", "all_q-1"])
@pytest.mark.parametrize("parties", [2, 4])
def test_mul_relin_on_planted_accumulators(pairs, parties, all_max):
    """Equal id sets, steered through the v_i: the v = np and boundary patterns in every member of out_0's merged ModDown at the same coefficient
    (planted), or NTT-domain accumulators of q_j - 1 at every point of every member (the largest load sum of the merged inverse NTT); the final
    out_0 at the free coefficients carries a dropped-limb residue on the rounding boundary of the fused Rescale (asserted on the oracle's output).
    mkhe_mul_relin_rescale against MulAndRelin followed by mkhe_rescale on the device, and both against the oracle's chain."""
    from mkhe_kklss_amd._abi import check, lib
    pair = pairs("ckks_np2")
    mk, ks, level = pair.mk, pair.ks, pair.maxlevel
    names = ["p%d" % i for i in range(parties)]
    plan = _plan(pair, level, seed=20 + parties)
    finals = S.rescale_finals(ks.Q[level])
    op0, op1, rlk, u, F = _steered(lambda rng: S.mulrelin_case(ks, plan, level, parties, rng, H, finals=finals, all_max=all_max), 500 + parties)
    ids = list(range(parties))
    _, ref = ks.mul_and_relin(level, ids, op0, ids, op1, rlk, u)
    for pos, Fv in F.items():
        assert [int(x) for x in ref[0][:, pos]] == Fv
    assert all_max or sorted(Fv[-1] for Fv in F.values()) == sorted(finals)
    d0 = mk.NewCiphertext(pair.params, names, level).upload(op0)
    d1 = mk.NewCiphertext(pair.params, names, level).upload(op1)
    rlk_d = mk.RelinearizationKeySet(pair.params)
    for i, n in enumerate(names):
        rlk_d.AddRelinearizationKey(mk.RelinearizationKey(pair.params, n, *rlk[i]))
    pair.params.AddCRS(-1, u)
    out = mk.NewCiphertext(pair.params, names, level)
    pair.ksw.MulAndRelin(d0, d1, rlk_d, out)
    assert (out.download() == ref).all()
    ref_r = np.stack([ks.ringQ.div_round_last_many(ref[s], 1)[0] for s in range(1 + parties)])
    fused = mk.NewCiphertext(pair.params, names, level - 1)
    pair.ksw.MulAndRelinHoisted(d0, d1, None, None, rlk_d, fused, rescaled=True)
    two = mk.NewCiphertext(pair.params, names, level - 1)
    check(lib().mkhe_rescale(pair.params.ctx, out.h, 1, two.h))
    assert (two.download() == ref_r).all()
    assert (fused.download() == ref_r).all()


# ------------------------------------------------------------------ Decompose with alpha >= 2
def _digit_plants(ks, level, rng):
    """a: uint64 [level + 1][N] uniform, with the limbs of every digit of two and more moduli planted at the first coefficients: (0, 0), (1, 1),
    (q - 1, q' - 1), (1, 0), (0, 1) and the boundary tuples of the digit's moduli (the float index of spread_prepare just below / above an integer)"""
    a = H.uniform_poly(rng, ks.Q[: level + 1], ks.N)
    for i in range(ks.beta(level)):
        lo, hi = i * ks.alpha, min((i + 1) * ks.alpha, level + 1)
        mods = ks.Q[lo:hi]
        if len(mods) < 2:
            continue
        limbs = [[0] * len(mods), [1] * len(mods), [q - 1 for q in mods], [1] + [0] * (len(mods) - 1), [0] * (len(mods) - 1) + [1]]
        for ts in S.boundary_tuples(mods, seed=i).values():
            limbs += [S.xp_of(t, mods) for t in ts]
        assert len(limbs) <= ks.N // 4
        for k, vals in enumerate(limbs):
            a[lo:hi, 4 * k + i] = vals
    return a


@pytest.mark.parametrize("is_ntt", [False, True])
@pytest.mark.parametrize("drop", [0, 1])
@pytest.mark.parametrize("name", ["alpha2_np4", "pn16_np3_g1"])
def test_decompose_digit_lift_on_planted_limbs(pairs, name, drop, is_ntt):
    """spread_prepare (the Decompose of alpha >= 2: the fifth restatement of the float index) on digits whose reconstruction sum sits on an integer"""
    pair = pairs(name)
    mk, ks, level = pair.mk, pair.ks, pair.maxlevel - drop
    a = _digit_plants(ks, level, np.random.default_rng(600 + drop))
    src = np.stack([ks.ringQ.ntt(j, a[j]) for j in range(level + 1)]) if is_ntt else a
    dev = mk.NewCiphertext(pair.params, [], level).upload(src[None])
    ad = mk.NewSwitchingKey(pair.params)
    pair.ksw.Decompose(level, dev, "0", ad, is_ntt=is_ntt)
    ref = ks.decompose(level, src, is_ntt=is_ntt)
    beta = ks.beta(level)
    act = list(range(level + 1)) + [len(pair.Q) + j for j in range(len(pair.P))]
    assert (ad.download()[:beta][:, act] == ref[:beta][:, act]).all()


# ------------------------------------------------------------------ mkhe_ct_automorphism on its own
def test_automorphism_writes_q_for_a_flipped_zero_and_add_takes_it(pairs):
    """zeros at flipping and at non-flipping coefficients: q and 0 on the output (keyswitch.go:290), and mkhe_ct_add of that output with a canonical
    ciphertext holding 0 and q - 1 there gives canonical sums"""
    from mkhe_kklss_amd._abi import check, lib
    pair = pairs("ckks_np2")
    mk, ks, level = pair.mk, pair.ks, pair.maxlevel
    rng = np.random.default_rng(700)
    h = H.uniform_ct(rng, ks, 2, level + 1)
    other = H.uniform_ct(rng, ks, 2, level + 1)
    qv = np.array(ks.Q[: level + 1], dtype=np.uint64)
    for gal in S.galois_elements(pair.logN):
        zeros = list(range(0, pair.N, 7))
        h[:, :, zeros] = 0
        flipped = [n for n in zeros if S.flips(n, gal, pair.logN)]
        assert len(flipped) > 8 and len(flipped) < len(zeros)
        for k, n in enumerate(zeros):
            other[:, :, (n * gal) & (pair.N - 1)] = 0 if k % 2 == 0 else qv[None, :] - np.uint64(1)
        d = mk.NewCiphertext(pair.params, ["a", "b"], level).upload(h)
        out = mk.NewCiphertext(pair.params, ["a", "b"], level)
        check(lib().mkhe_ct_automorphism(pair.params.ctx, gal, d.h, out.h))
        ref = np.stack([ks.ringQ.permute(gal, h[s]) for s in range(3)])
        for n in zeros:
            want = qv if n in flipped else 0 * qv
            assert (ref[:, :, (n * gal) & (pair.N - 1)] == want[None, :]).all()
        assert (out.download() == ref).all()
        o = mk.NewCiphertext(pair.params, ["a", "b"], level).upload(other)
        total = mk.NewCiphertext(pair.params, ["a", "b"], level)
        check(lib().mkhe_ct_add(pair.params.ctx, out.h, o.h, total.h))
        want = np.stack([np.stack([ks.ringQ.add(j, ref[s, j], other[s, j]) for j in range(level + 1)]) for s in range(3)])
        assert (want < qv[None, :, None]).all()
        assert (total.download() == want).all()
