"""The definition of mkhe_bfv_mul_relin_sum written with the oracle's own pieces (no reference counterpart: the reference relinearises every product).

K MK-BFV products under ONE Quantize and ONE relinearisation tail.  ExtB = ExternalProductBFVHoisted (both gadgets), ExtH = ExternalProductHoisted,
(h1, h2) = DecomposeBFV, every + canonical.  For every pair k

    r0, r1     = ModUpQtoR(op0[k]), Rescale(op1[k]) ;  f0, f1 = NTT_R(r0), NTT_R(r1)          (evaluator.go:118-140)
    z_0       += f0_0 * f1_0 ;  z_i += f1_0 * f0_i ;  z_j += f0_0 * f1_j                       (mod the primes of R = Q || QMul, NTT domain)
    x1, x2     = MForm(sum_i d1_i (.) h1(r0_i)), MForm(sum_i d2_i (.) h2(r0_i))               (keyswitch_hoisted.go:86-109)
    y1, y2     = the same with b1_j, b2_j over r1_j                                            (:111-134)
    e_j       += ExtB(h1(r1_j), h2(r1_j), x1, x2)                                              (step E, :176-183)
    t_i       += ExtB(h1(r0_i), h2(r0_i), y1, y2)                                              (step F1, :190-197)

and then ONCE

    out_o      = Quantize(z_o) ;  out_j += e_j
    out_0     += ExtH(h(t_i), v_i) ;  out_i += ExtH(h(t_i), u)                                 (step F2, :199-205)

K = 1 is BFV.mul_relin_new bit for bit; every sum is one of exact residues, so the order of the pairs is immaterial.  ids are the oracle's dense
party indices, every op0[k] is uint64[1 + |ids0|][nQ][N]; rlk[i] = (b1, b2, d1, d2, v)."""
import numpy as np


def _ring_r(bfv, l):
    return (bfv.ringQ, l) if l < bfv.nq else (bfv.ringQMul, l - bfv.nq)


def _ring_qp(bfv, l):
    return (bfv.ringQ, l) if l < bfv.nq else (bfv.ringP, l - bfv.nq)


def _add_q(bfv, dst, src):
    for l in range(bfv.nq):
        dst[l] = bfv.ringQ.add(l, dst[l], src[l])


def _mac_r(bfv, z, a, b):
    """z += a * b over R, NTT domain (MForm, MulCoeffsMontgomery, Add)"""
    for l in range(2 * bfv.nq):
        R, i = _ring_r(bfv, l)
        z[l] = R.add(i, z[l], R.mul(i, R.mform(i, a[l]), b[l]))


def _inner(bfv, keys, digits):
    """MForm(sum_i key_i (.) digits_i) over QP, digit by digit (MulCoeffsMontgomeryAndAdd onto zero, then MFormLvl)"""
    out = bfv.ks.new_swk()
    for d in range(out.shape[0]):
        for l in range(out.shape[1]):
            R, i = _ring_qp(bfv, l)
            acc = out[d, l]
            for key, dig in zip(keys, digits):
                acc = R.mul_add(i, key[d, l], dig[d, l], acc)
            out[d, l] = R.mform(i, acc)
    return out


def bfv_mul_relin_sum(bfv, ids0, ops0, ids1, ops1, rlk, crs_u):
    """-> (ids_out, out[1 + nout][nQ][N])"""
    assert len(ops0) == len(ops1) and len(ops0) >= 1
    nq, N, ks, level = bfv.nq, bfv.N, bfv.ks, bfv.nq - 1
    ids_out = sorted(set(ids0) | set(ids1))
    slot = {i: 1 + s for s, i in enumerate(ids_out)}
    z = np.zeros((1 + len(ids_out), 2 * nq, N), dtype=np.uint64)
    e = {j: np.zeros((nq, N), dtype=np.uint64) for j in ids1}
    t = {i: np.zeros((nq, N), dtype=np.uint64) for i in ids0}
    for op0, op1 in zip(ops0, ops1):
        op0, op1 = np.asarray(op0, dtype=np.uint64), np.asarray(op1, dtype=np.uint64)
        r0 = [bfv.modup_q_to_r(p) for p in op0]
        r1 = [bfv.rescale(p) for p in op1]
        f0, f1 = [bfv.ntt_r(p) for p in r0], [bfv.ntt_r(p) for p in r1]
        _mac_r(bfv, z[0], f0[0], f1[0])
        for a, i in enumerate(ids0):
            _mac_r(bfv, z[slot[i]], f1[0], f0[1 + a])
        for a, j in enumerate(ids1):
            _mac_r(bfv, z[slot[j]], f0[0], f1[1 + a])
        h0 = [bfv.decompose(r0[1 + a]) for a in range(len(ids0))]
        h1 = [bfv.decompose(r1[1 + a]) for a in range(len(ids1))]
        x1 = _inner(bfv, [rlk[i][2] for i in ids0], [h[0] for h in h0])
        x2 = _inner(bfv, [rlk[i][3] for i in ids0], [h[1] for h in h0])
        y1 = _inner(bfv, [rlk[j][0] for j in ids1], [h[0] for h in h1])
        y2 = _inner(bfv, [rlk[j][1] for j in ids1], [h[1] for h in h1])
        for a, j in enumerate(ids1):
            _add_q(bfv, e[j], bfv.external_product_hoisted(h1[a][0], h1[a][1], x1, x2))
        for a, i in enumerate(ids0):
            _add_q(bfv, t[i], bfv.external_product_hoisted(h0[a][0], h0[a][1], y1, y2))
    out = np.stack([bfv.quantize(p) for p in z])
    for j in ids1:
        _add_q(bfv, out[slot[j]], e[j])
    for i in ids0:
        ht = ks.decompose(level, t[i])
        _add_q(bfv, out[0], ks.external_product_hoisted(level, ht, rlk[i][4]))
        _add_q(bfv, out[slot[i]], ks.external_product_hoisted(level, ht, crs_u))
    return ids_out, out


def chain(bfv, ids0, ops0, ids1, ops1, rlk, crs_u):
    """what the call replaces: K x mul_relin_new, summed"""
    ids_out, acc = None, None
    for op0, op1 in zip(ops0, ops1):
        ids_out, o = bfv.mul_relin_new(ids0, op0, ids1, op1, rlk, crs_u)
        if acc is None:
            acc = o
        else:
            for s in range(acc.shape[0]):
                _add_q(bfv, acc[s], o[s])
    return ids_out, acc
