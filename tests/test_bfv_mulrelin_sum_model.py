"""CPU: pins the yardstick of mkhe_bfv_mul_relin_sum (tests/bfv_mulrelin_sum_model.py) to the oracle: one pair is BFV.mul_relin_new bit for bit, the
order of the pairs is immaterial, and with valid keys K = 2, 3 products under one Quantize and one relinearisation tail decrypt to exactly the sum
of the negacyclic products mod T."""
import numpy as np
import pytest

import bfv_mulrelin_sum_model as M
import harness as H
import harness_bfv as HB

PSETS = {"q3": HB.small_bfv(10, 3), "q2": HB.small_bfv(10, 2)}


@pytest.fixture(scope="module", params=sorted(PSETS))
def mat(request):
    bfv = HB.make_bfv(PSETS[request.param])
    rng = np.random.default_rng(78)
    rlk = {i: tuple(H.uniform_swk(rng, bfv.ks) for _ in range(5)) for i in (0, 1, 2)}
    return dict(bfv=bfv, rng=rng, rlk=rlk, u=H.uniform_swk(rng, bfv.ks))


def _cts(mat, n, K):
    return [H.uniform_ct(mat["rng"], mat["bfv"].ks, n, mat["bfv"].nq) for _ in range(K)]


@pytest.mark.parametrize("ids0,ids1", [([0, 1], [0, 1]), ([0, 1], [1, 2])])
def test_one_pair_is_mul_relin_new(mat, ids0, ids1):
    bfv = mat["bfv"]
    op0, op1 = _cts(mat, len(ids0), 1)[0], _cts(mat, len(ids1), 1)[0]
    ido, ref = bfv.mul_relin_new(ids0, op0, ids1, op1, mat["rlk"], mat["u"])
    idm, got = M.bfv_mul_relin_sum(bfv, ids0, [op0], ids1, [op1], mat["rlk"], mat["u"])
    assert idm == ido and got.shape == ref.shape and (got == ref).all()


def test_order_of_the_pairs_is_immaterial(mat):
    bfv, ids0, ids1 = mat["bfv"], [0, 1], [1, 2]
    ops0, ops1 = _cts(mat, 2, 3), _cts(mat, 2, 3)
    _, a = M.bfv_mul_relin_sum(bfv, ids0, ops0, ids1, ops1, mat["rlk"], mat["u"])
    perm = [2, 0, 1]
    _, b = M.bfv_mul_relin_sum(bfv, ids0, [ops0[k] for k in perm], ids1, [ops1[k] for k in perm], mat["rlk"], mat["u"])
    assert (a == b).all()
    # ... and it is NOT the sum of three relinearised products (one rounding and one gadget noise instead of three): another ciphertext of the same sum
    _, c = M.chain(bfv, ids0, ops0, ids1, ops1, mat["rlk"], mat["u"])
    assert (a != c).any()


@pytest.mark.parametrize("nq,parties", [(3, 2), (2, 3)])
@pytest.mark.parametrize("K", [2, 3])
def test_products_decrypt_to_their_sum_exactly(nq, parties, K):
    """op0[k] = the sum of fresh encryptions under every party, op1[k] one under the last party alone: both tensor shapes in one call"""
    sc = HB.BFVScenario(HB.small_bfv(10, nq), parties=parties, seed=30 + K)
    T = sc.bfv.T
    want = np.zeros(sc.N, dtype=np.int64)
    ops0, ops1 = [], []
    last = sc.ids[-1]
    for _ in range(K):
        ms = {i: sc.message(-3, 4) for i in sc.ids}
        b = sc.message(-3, 4)
        ops0.append(sc.sum_ct(ms))
        ops1.append(sc.fresh_ct(b, last))
        want += HB.negacyclic_mul_mod_t(sum(ms.values()), b, T)
    want %= T
    want = np.where(want > T // 2, want - T, want)
    for fn in (M.bfv_mul_relin_sum, M.chain):
        ids, out = fn(sc.bfv, sc.ids, ops0, [last], ops1, sc.rlk, sc.u)
        assert ids == sc.ids
        assert (sc.decrypt(ids, out) == want).all(), fn.__name__
