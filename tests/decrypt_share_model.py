"""A model of distributed decryption (include/mkhe.h, "distributed decryption"): kind 2 of the keystream in Python integers on top of
device_sampler_model.stream_values, and share and merge from the oracle's ring pieces (the forward and inverse NTT and the Montgomery
product of harness.KeyGen.decrypt).  What mkhe_decrypt_share and mkhe_decrypt_merge are compared with, bit for bit."""
import numpy as np

import device_sampler_model as M


def flood_value(r, bits):
    """kind 2: uniform on [-2^(bits-1), 2^(bits-1)) from the top `bits` bits of r; bits = 0: 0"""
    assert 0 <= bits <= 62 and 0 <= r < 1 << 64
    return 0 if bits == 0 else (r >> (64 - bits)) - (1 << (bits - 1))


def flood_poly(key, nonce, stream, n, bits):
    """the flooding noise of one share: n Python ints; bits = 0 reads no stream"""
    if bits == 0:
        return [0] * n
    return [flood_value(r, bits) for r in M.stream_values(key, nonce, stream, n)]


def flood_limbs(e, moduli):
    """e mod q_j, canonical, for every limb: uint64 [limbs][n]"""
    return np.array([[v % int(q) for v in e] for q in moduli], dtype=np.uint64)


def product(ks, c, sk):
    """InvNTT(NTT(c) * sk): c uint64 [limbs][N] coefficient domain, sk the secret (NTT, Montgomery form; its first limbs are read)"""
    r = ks.ringQ
    return np.stack([r.intt(j, r.mul(j, r.ntt(j, c[j]), sk[j])) for j in range(c.shape[0])])


def share(ks, c, sk, e):
    """mu = c * s + e, canonical: uint64 [limbs][N]"""
    q = np.array(ks.Q[: c.shape[0]], dtype=np.uint64)[:, None]
    return (product(ks, c, sk) + flood_limbs(e, ks.Q[: c.shape[0]])) % q


def merge(ks, c0, shares):
    """c_0 + the sum of the shares, canonical"""
    q = np.array(ks.Q[: c0.shape[0]], dtype=np.uint64)[:, None]
    out = np.asarray(c0, dtype=np.uint64) % q
    for s in shares:
        out = (out + s) % q
    return out


def centred(x, q):
    """canonical residues -> the representatives in (-q/2, q/2] as Python ints"""
    return [int(v) - int(q) if int(v) > int(q) // 2 else int(v) for v in x]
