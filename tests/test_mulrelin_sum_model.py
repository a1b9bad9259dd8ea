"""CPU: pins the yardstick of mkhe_mul_relin_sum (tests/mulrelin_sum_model.py) to the oracle: one pair is KeySwitcher.mul_and_relin bit for bit,
the order of the pairs is immaterial, and with valid keys three products under one relinearisation tail decrypt to their sum inside the reference's
MulRelin bound plus log2 K."""
import numpy as np
import pytest

import harness as H
import mulrelin_sum_model as M
from oracle import oracle as O
from scenario import Scenario

ID_SHAPES = [([1], [2]), ([1, 2], [1, 2]), ([1, 2], [2, 3]), ([1, 2, 3, 4], [1, 2, 3, 4])]
PSETS = {"ckks": H.small_ckks(10, 4), "alpha2": H.small_alpha2(10, 5)}


@pytest.fixture(scope="module", params=sorted(PSETS))
def mat(request):
    pset = PSETS[request.param]
    ks = O.KeySwitcher(pset["logN"], pset["Q"], pset["P"], 2)
    rng = np.random.default_rng(77)
    rlk = {i: tuple(H.uniform_swk(rng, ks) for _ in range(3)) for i in (1, 2, 3, 4)}
    return dict(ks=ks, rng=rng, rlk=rlk, u=H.uniform_swk(rng, ks), level=len(pset["Q"]) - 1)


@pytest.mark.parametrize("ids0,ids1", ID_SHAPES)
def test_one_pair_is_mul_and_relin(mat, ids0, ids1):
    ks, rng = mat["ks"], mat["rng"]
    for level, limbs in ((mat["level"], mat["level"] + 1), (1, 3)):
        op0, op1 = H.uniform_ct(rng, ks, len(ids0), limbs), H.uniform_ct(rng, ks, len(ids1), limbs)
        ido, ref = ks.mul_and_relin(level, ids0, op0, ids1, op1, mat["rlk"], mat["u"])
        idm, got = M.mul_relin_sum(ks, level, ids0, [op0], ids1, [op1], mat["rlk"], mat["u"])
        assert idm == ido and got.shape == ref.shape and (got == ref).all()


def test_order_of_the_pairs_is_immaterial(mat):
    ks, rng, level = mat["ks"], mat["rng"], mat["level"]
    ids0, ids1 = [1, 2], [2, 3]
    ops0 = [H.uniform_ct(rng, ks, 2, level + 1) for _ in range(3)]
    ops1 = [H.uniform_ct(rng, ks, 2, level + 1) for _ in range(3)]
    _, a = M.mul_relin_sum(ks, level, ids0, ops0, ids1, ops1, mat["rlk"], mat["u"])
    perm = [2, 0, 1]
    _, b = M.mul_relin_sum(ks, level, ids0, [ops0[k] for k in perm], ids1, [ops1[k] for k in perm], mat["rlk"], mat["u"])
    assert (a == b).all()
    # ... and it is NOT the sum of three relinearised products (three gadget noises instead of one): a different ciphertext of the same sum
    _, c = M.chain(ks, level, ids0, ops0, ids1, ops1, mat["rlk"], mat["u"])
    assert (a != c).any()


def _log2_err(a, b):
    d = np.abs(np.asarray(a) - np.asarray(b))
    return float(np.log2(max(d.real.max(), d.imag.max(), 1e-300)))


def test_three_products_decrypt_to_their_sum():
    """op0 under party 1, op1 under party 2, K = 3: log2 |delta| <= -log2(scale) + logSlots + 12 + log2 K (the reference's MulRelin bound,
    mkckks_test.go:357, once per summand)"""
    K = 3
    sc = Scenario(H.small_ckks(10, 4), parties=2, seed=11)
    ks, level = sc.ks, sc.level
    rl = {i: sc.rlk[n] for i, n in enumerate(sc.names)}
    zs = [sc.message(-1 - 1j, 1 + 1j) for _ in range(K)]
    ws = [sc.message(-1 - 1j, 1 + 1j) for _ in range(K)]
    ops0 = [np.stack(sc.encrypt(z, sc.names[0])) for z in zs]
    ops1 = [np.stack(sc.encrypt(w, sc.names[1])) for w in ws]
    want = sum(z * w for z, w in zip(zs, ws))
    nb, scale = ks.ckks_nb_rescales(level, sc.scale * sc.scale, sc.scale)
    bound = sc.precision_bound(12) + np.log2(K)
    errs = []
    for fn in (M.mul_relin_sum, M.chain):
        ids, out = fn(ks, level, [0], ops0, [1], ops1, rl, sc.kg.CRS[-1])
        assert ids == [0, 1]
        out = np.stack([ks.ringQ.div_round_last_many(out[s], nb)[0] for s in range(out.shape[0])])
        errs.append(_log2_err(sc.decrypt_decode(sc.names, out, scale), want))
    print("log2 |delta|: one tail %.1f, chain %.1f, bound %.1f" % (errs[0], errs[1], bound))
    assert errs[0] <= bound and errs[1] <= bound
