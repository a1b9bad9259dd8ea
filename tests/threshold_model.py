"""A model of the threshold secret keys (include/mkhe.h, "threshold secret keys") in Python integers on top of device_sampler_model and
sk_encrypt_model: kind 7 of the keystream (uniform mod m_j over all R rows; coefficient polynomial k, row j on the stream pair 2 ((k-1) R + j),
2 ((k-1) R + j) + 1), the Shamir shares of the stored words, the Lagrange coefficients at 0, the additive keys and the fold.  What
mkhe_threshold_gen_shares, mkhe_threshold_additive_key and mkhe_limbs_sum are compared with, bit for bit.  values = sk_encrypt_model.stream_values_np
gives the same keystream with numpy, for the rings on which the pure-Python one would take minutes."""
import numpy as np

import device_sampler_model as M
import sk_encrypt_model as SK


def kind7_streams(k, j, R):
    """(lo, hi) streams of coefficient polynomial k (1 .. t-1), row j < R"""
    assert k >= 1 and 0 <= j < R
    return 2 * ((k - 1) * R + j), 2 * ((k - 1) * R + j) + 1


def kind7_row(key, nonce, k, j, R, m, n, values=M.stream_values):
    """c_k[j][0 .. n): list of Python ints in [0, m)"""
    ls, hs = kind7_streams(k, j, R)
    lo, hi = values(key, nonce, ls, n), values(key, nonce, hs, n)
    return [SK.uniform_value(int(l), int(h), int(m)) for l, h in zip(lo, hi)]


def shares(S, t, points, key, nonce, moduli, values=M.stream_values, rows=None):
    """share_p[j][i] = (S[j][i] + sum_{k=1}^{t-1} c_k[j][i] x_p^k) mod m_j -> uint64 [len(points)][len(rows)][n].  S: [R][n] stored words (any
    integers below m_j), moduli = the R moduli of the rows; rows = the rows to compute (default: all), in the order given."""
    R = len(moduli)
    rows = list(range(R)) if rows is None else list(rows)
    n = len(S[0])
    out = np.zeros((len(points), len(rows), n), dtype=np.uint64)
    for r, j in enumerate(rows):
        m = int(moduli[j])
        c = [kind7_row(key, nonce, k, j, R, m, n, values) for k in range(1, t)]
        s = [int(v) for v in S[j]]
        for p, x in enumerate(points):
            x = int(x)
            acc = [0] * n
            for ck in reversed(c):                                  # Horner from k = t - 1 down to 1, then S
                acc = [(a * x + v) % m for a, v in zip(acc, ck)]
            out[p, r] = [(a * x + v) % m for a, v in zip(acc, s)]
    return out


def lagrange(point, active, m):
    """lambda_p = prod_{a in active, a != point} x_a (x_a - point)^-1 mod m (m prime, the points distinct and below m)"""
    assert list(active).count(point) == 1
    num = den = 1
    for a in active:
        if a != point:
            num = num * int(a) % m
            den = den * ((int(a) - int(point)) % m) % m
    return num * pow(den, m - 2, m) % m


def additive(share, point, active, moduli):
    """add_p[j][i] = share_p[j][i] lambda_p[j] mod m_j -> uint64 [R][n]"""
    out = np.zeros((len(moduli), len(share[0])), dtype=np.uint64)
    for j, m in enumerate(moduli):
        lam = lagrange(point, active, int(m))
        out[j] = [int(v) * lam % int(m) for v in share[j]]
    return out


def fold(bufs, moduli):
    """sum of buffers [..][limbs][n] mod m_j per row j (the second-to-last axis) -> uint64, the shape of one buffer"""
    bufs = [np.asarray(b, dtype=np.uint64) for b in bufs]
    acc = np.zeros(bufs[0].shape, dtype=object)
    for b in bufs:
        acc = acc + b.astype(object)
    limbs = bufs[0].shape[-2]
    assert limbs <= len(moduli)
    for j in range(limbs):
        acc[..., j, :] = acc[..., j, :] % int(moduli[j])
    return acc.astype(np.uint64)
