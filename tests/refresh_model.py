"""A model of the collective refresh (include/mkhe.h, "collective refresh") in Python integers on top of device_sampler_model and
decrypt_share_model: kind 3 of the keystream (a 128-bit value from two streams), the masked share, the plaintext -M, and the merge as CRT,
centred, reduced.  What mkhe_refresh_share and mkhe_refresh_merge are compared with, bit for bit."""
import numpy as np

import decrypt_share_model as D
import device_sampler_model as M


def wide_value(lo, hi, bits):
    """kind 3: uniform on [-2^(bits-1), 2^(bits-1)) from the top `bits` bits of r = hi 2^64 + lo; bits = 0: 0"""
    assert 0 <= bits <= 120 and 0 <= lo < 1 << 64 and 0 <= hi < 1 << 64
    return 0 if bits == 0 else (((hi << 64) | lo) >> (128 - bits)) - (1 << (bits - 1))


def mask_poly(key, nonce, b, n, bits):
    """the mask of item b of a call: lo from stream 2 b, hi from stream 2 b + 1; bits = 0 reads no stream"""
    if bits == 0:
        return [0] * n
    lo, hi = M.stream_values(key, nonce, 2 * b, n), M.stream_values(key, nonce, 2 * b + 1, n)
    return [wide_value(l, h, bits) for l, h in zip(lo, hi)]


def mask_limbs(m, moduli):
    """M mod q_j, canonical: uint64 [limbs][n]"""
    return D.flood_limbs(m, moduli)


def neg_mask_limbs(m, moduli):
    """the plaintext of the re-encryption: (-M) mod q_j, canonical"""
    return D.flood_limbs([-v for v in m], moduli)


def share(ks, c, sk, m):
    """c * s + M, canonical: uint64 [limbs][N] (decrypt_share_model.share with the mask in the place of the flood)"""
    return D.share(ks, c, sk, m)


def crt(residues, moduli):
    """the x in [0, Q) with the given residues: a list of Python ints (residues [limbs][n])"""
    Q = 1
    for q in moduli:
        Q *= int(q)
    x = [0] * len(residues[0])
    for r, q in zip(residues, moduli):
        q = int(q)
        c = (Q // q) * pow(Q // q, -1, q)
        x = [(a + int(v) * c) % Q for a, v in zip(x, r)]
    return x, Q


def centre(x, Q):
    """x in [0, Q), Q odd -> x if x <= (Q - 1) / 2, else x - Q"""
    return [v if v <= (Q - 1) // 2 else v - Q for v in x]


def merge(moduli, lin, lout, c0, shares, reenc):
    """mkhe_refresh_merge for one ciphertext: c0 uint64 [lin][N] (any representative), shares [k] of [lin][N], reenc [k] of [2][lout][N]
    -> uint64 [1 + k][lout][N]"""
    qin = [int(q) for q in moduli[:lin]]
    res = [[int(v) % q for v in row] for row, q in zip(c0, qin)]
    for s in shares:
        res = [[(a + int(v)) % q for a, v in zip(row, srow)] for row, srow, q in zip(res, s, qin)]
    x, Q = crt(res, qin)
    lifted = centre(x, Q)
    out = np.zeros((1 + len(shares), lout, len(lifted)), dtype=np.uint64)
    for j in range(lout):
        q = int(moduli[j])
        row = [v % q for v in lifted]
        for r in reenc:
            row = [(a + int(v)) % q for a, v in zip(row, r[0][j])]
        out[0, j] = np.array(row, dtype=np.uint64)
    for i, r in enumerate(reenc):
        out[1 + i] = np.asarray(r[1], dtype=np.uint64)[:lout]
    return out
