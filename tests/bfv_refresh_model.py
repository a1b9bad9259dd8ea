"""A model of the collective refresh of MK-BFV (include/mkhe.h, "collective refresh for MK-BFV") in Python integers on top of
device_sampler_model and decrypt_share_model: kinds 4 and 5 of the keystream with their stream layout, up and down, the share, the plaintext
of the re-encryption and the merge.  What mkhe_bfv_refresh_share and mkhe_bfv_refresh_merge are compared with, bit for bit."""
import numpy as np

import decrypt_share_model as D
import device_sampler_model as M


def words(flood_bits):
    """W: the 64-bit words of a flood"""
    assert 0 <= flood_bits <= 1024
    return (flood_bits + 63) // 64


def streams_per_item(flood_bits):
    """S = 2 + W: the streams item b owns, starting at b S"""
    return 2 + words(flood_bits)


def mask_value(lo, hi, T):
    """kind 4: A = ((hi 2^64 + lo) T) >> 128, in [0, T)"""
    assert 0 <= lo < 1 << 64 and 0 <= hi < 1 << 64
    return (((hi << 64) | lo) * T) >> 128


def flood_value(vs, flood_bits):
    """kind 5 from the 64-bit values vs[w] of the W streams: the top word masked to its low flood_bits - 64 (W - 1) bits, centred"""
    W = words(flood_bits)
    assert len(vs) == W
    if W == 0:
        return 0
    top = flood_bits - 64 * (W - 1)
    F = sum((int(v) & ((1 << top) - 1) if w == W - 1 else int(v)) << (64 * w) for w, v in enumerate(vs))
    return F - (1 << (flood_bits - 1))


def mask_poly(key, nonce, b, n, T, flood_bits, mask=1, values=M.stream_values):
    """A_b: lo from stream b S, hi from stream b S + 1; mask = 0 reads no stream"""
    if not mask:
        return [0] * n
    S = streams_per_item(flood_bits)
    return [mask_value(l, h, T) for l, h in zip(values(key, nonce, b * S, n), values(key, nonce, b * S + 1, n))]


def flood_poly(key, nonce, b, n, flood_bits, values=M.stream_values):
    """e_b: word w from stream b S + 2 + w; flood_bits = 0 reads no stream"""
    W, S = words(flood_bits), streams_per_item(flood_bits)
    if W == 0:
        return [0] * n
    cols = [values(key, nonce, b * S + 2 + w, n) for w in range(W)]
    return [flood_value([c[i] for c in cols], flood_bits) for i in range(n)]


def q_product(moduli):
    Q = 1
    for q in moduli:
        Q *= int(q)
    return Q


def up(x, moduli, T):
    """floor((Q x + h) / T) as an integer, x in [0, T)"""
    assert 0 <= x < T
    return (q_product(moduli) * x + T // 2) // T


def down(R, moduli, T):
    """floor((T R + floor(Q/2)) / Q) mod T, R in [0, Q)"""
    Q = q_product(moduli)
    assert 0 <= R < Q
    return ((T * R + Q // 2) // Q) % T


def up_limbs(xs, moduli, T):
    """up of every coefficient under every modulus: uint64 [limbs][n]"""
    big = [up(int(x), moduli, T) for x in xs]
    return np.array([[v % int(q) for v in big] for q in moduli], dtype=np.uint64)


def share_addend(A, e, moduli, T):
    """what the share adds to the product: (up(A) + e) mod q_j, canonical, uint64 [limbs][n]"""
    big = [up(int(a), moduli, T) + int(f) for a, f in zip(A, e)]
    return np.array([[v % int(q) for v in big] for q in moduli], dtype=np.uint64)


def reenc_plaintext(A, moduli, T):
    """pt = up((T - A) mod T)"""
    return up_limbs([(T - int(a)) % T for a in A], moduli, T)


def share(ks, c, sk, A, e, T):
    """c * s + up(A) + e, canonical: uint64 [limbs][N]"""
    q = np.array(ks.Q[: c.shape[0]], dtype=np.uint64)[:, None]
    return (D.product(ks, c, sk) + share_addend(A, e, ks.Q[: c.shape[0]], T)) % q


def crt(residues, moduli):
    """the x in [0, Q) with the given residues: a list of Python ints (residues [limbs][n])"""
    Q = q_product(moduli)
    x = [0] * len(residues[0])
    for r, q in zip(residues, moduli):
        q = int(q)
        c = (Q // q) * pow(Q // q, -1, q)
        x = [(a + int(v) * c) % Q for a, v in zip(x, r)]
    return x


def merge_w(moduli, T, c0, shares):
    """steps 1 and 2 of the merge: w = down(c_0 + sum of the shares), a list of ints in [0, T)"""
    qs = [int(q) for q in moduli]
    res = [[int(v) % q for v in row] for row, q in zip(c0, qs)]
    for s in shares:
        res = [[(a + int(v)) % q for a, v in zip(row, srow)] for row, srow, q in zip(res, s, qs)]
    return [down(R, moduli, T) for R in crt(res, qs)]


def merge(moduli, T, c0, shares, reenc):
    """mkhe_bfv_refresh_merge for one ciphertext: c0 uint64 [nQ][N] (any representative), shares [k] of [nQ][N], reenc [k] of [2][nQ][N]
    -> uint64 [1 + k][nQ][N]"""
    w = merge_w(moduli, T, c0, shares)
    out = np.zeros((1 + len(shares), len(moduli), len(w)), dtype=np.uint64)
    lifted = up_limbs(w, moduli, T)
    for j, q in enumerate(moduli):
        row = [int(v) for v in lifted[j]]
        for r in reenc:
            row = [(a + int(v)) % int(q) for a, v in zip(row, r[0][j])]
        out[0, j] = np.array(row, dtype=np.uint64)
    for i, r in enumerate(reenc):
        out[1 + i] = np.asarray(r[1], dtype=np.uint64)
    return out


def max_flood_bits(moduli, T, parties):
    """floor(log2(Q / (2 T parties))), capped at 1024: mkbfv.Refresher.MaxFloodBits"""
    return min(1024, (q_product(moduli) // (2 * int(T) * int(parties))).bit_length() - 1)
