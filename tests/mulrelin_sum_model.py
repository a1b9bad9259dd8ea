"""The definition of mkhe_mul_relin_sum written with the oracle's own pieces (no reference counterpart: the reference relinearises every product).

K products under ONE relinearisation tail.  With ExtH = ExternalProductHoisted (inner product over the digits in QP, inverse NTT, ModDown by P)
and every + canonical mod q_l, for every pair k

    x^k, y^k   = mr_xy(mform=True)                                  (keyswitch_hoisted.go:78-117)
    out_0     += c0_0^k * c1_0^k                                    (negacyclic products mod q_l, :119-144)
    out_i     += c0_i^k * c1_0^k
    out_j     += c0_0^k * c1_j^k
    out_j     += ExtH(h(c1_j^k), x^k)                               (step E)
    t_i       += ExtH(h(c0_i^k), y^k)                               (step F1)

and then ONCE per party i of op0

    out_0     += ExtH(h(t_i), v_i)                                  (step F2)
    out_i     += ExtH(h(t_i), u)

The sums over k are sums of separately ModDown'd products, so K = 1 is KeySwitcher.mul_and_relin bit for bit and the order of the pairs is
immaterial.  ids are the oracle's dense party indices; every op0[k] is uint64[1 + |ids0|][limbs >= level + 1][N], of which the first level + 1
limbs are read."""
import numpy as np


def _add(R, dst, src):
    for l in range(dst.shape[0]):
        dst[l] = R.add(l, dst[l], src[l])


def _mul(R, a, b):
    """negacyclic product of two coefficient-domain polynomials, limb by limb"""
    return np.stack([R.intt(l, R.mul(l, R.mform(l, R.ntt(l, a[l])), R.ntt(l, b[l]))) for l in range(a.shape[0])])


def mul_relin_sum(ks, level, ids0, ops0, ids1, ops1, rlk, crs_u):
    """-> (ids_out, out[1 + nout][level + 1][N])"""
    assert len(ops0) == len(ops1) and len(ops0) >= 1
    R, L = ks.ringQ, level + 1
    ids_out = sorted(set(ids0) | set(ids1))
    slot = {i: 1 + s for s, i in enumerate(ids_out)}
    out = np.zeros((1 + len(ids_out), L, ks.N), dtype=np.uint64)
    t = {i: np.zeros((L, ks.N), dtype=np.uint64) for i in ids0}
    for op0, op1 in zip(ops0, ops1):
        op0 = np.ascontiguousarray(np.asarray(op0, dtype=np.uint64)[:, :L])
        op1 = np.ascontiguousarray(np.asarray(op1, dtype=np.uint64)[:, :L])
        x, y = ks.mr_xy(level, ids0, op0, ids1, op1, rlk, True)
        _add(R, out[0], _mul(R, op0[0], op1[0]))
        for a, i in enumerate(ids0):
            _add(R, out[slot[i]], _mul(R, op0[1 + a], op1[0]))
            _add(R, t[i], ks.external_product_hoisted(level, ks.decompose(level, op0[1 + a]), y))
        for a, j in enumerate(ids1):
            _add(R, out[slot[j]], _mul(R, op0[0], op1[1 + a]))
            _add(R, out[slot[j]], ks.external_product_hoisted(level, ks.decompose(level, op1[1 + a]), x))
    for i in ids0:
        ht = ks.decompose(level, t[i])
        _add(R, out[0], ks.external_product_hoisted(level, ht, rlk[i][2]))
        _add(R, out[slot[i]], ks.external_product_hoisted(level, ht, crs_u))
    return ids_out, out


def chain(ks, level, ids0, ops0, ids1, ops1, rlk, crs_u):
    """what the call replaces: K x mul_and_relin, summed"""
    R = ks.ringQ
    ids_out, acc = None, None
    for op0, op1 in zip(ops0, ops1):
        ids_out, o = ks.mul_and_relin(level, ids0, op0, ids1, op1, rlk, crs_u)
        if acc is None:
            acc = o
        else:
            for s in range(acc.shape[0]):
                _add(R, acc[s], o[s])
    return ids_out, acc
