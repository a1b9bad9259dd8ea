"""A model of secret-key encryption with a seeded c1 (include/mkhe.h, "secret-key encryption") in Python integers on top of
device_sampler_model: kind 6 of the keystream (uniform mod q_j, rows (b, j) on the stream pairs 2 (b nQ + j), 2 (b nQ + j) + 1), the ciphertext
c1 = a, c0 = pt + e - a s with a schoolbook negacyclic product, and its decryption.  What mkhe_sample_uniform, mkhe_encrypt_sk,
mkhe_encrypt_sk_seeded and mkhe_ct_expand_seeded are compared with, bit for bit.  stream_values_np is the same keystream with numpy over the
blocks of a stream, for the rings on which the pure-Python one would take minutes; the model test pins it to device_sampler_model."""
import numpy as np

import device_sampler_model as M


def uniform_value(lo, hi, q):
    """kind 6: ((hi 2^64 + lo) q) >> 128, in [0, q)"""
    return (((hi << 64) | lo) * q) >> 128


def uniform_value_words(lo, hi, q):
    """the same from 64-bit pieces, the way the kernel forms it: (hi q + ((lo q) >> 64)) >> 64 with the carry of the low words"""
    M64 = (1 << 64) - 1
    p = hi * q
    ph, pl = p >> 64, p & M64
    s = pl + ((lo * q) >> 64)
    return ph + (1 if s > M64 else 0)


def row_streams(b, j, nq):
    """(lo, hi) streams of row (b, j): nq is the number of Q primes of the context, NOT the number of limbs expanded"""
    return 2 * (b * nq + j), 2 * (b * nq + j) + 1


def stream_values_np(key, nonce, stream, n):
    """device_sampler_model.stream_values as uint64 [n], vectorised over the blocks"""
    assert n % 8 == 0
    nb = n // 8
    state = [np.full(nb, c, dtype=np.uint32) for c in M.CONSTANTS] + [np.full(nb, int(k) & M.M32, dtype=np.uint32) for k in key]
    state += [np.arange(nb, dtype=np.uint32), np.full(nb, nonce & M.M32, dtype=np.uint32), np.full(nb, nonce >> 32, dtype=np.uint32),
              np.full(nb, stream, dtype=np.uint32)]
    x = [s.copy() for s in state]

    def rotl(v, r):
        return (v << np.uint32(r)) | (v >> np.uint32(32 - r))

    def quarter(a, b, c, d):
        x[a] = x[a] + x[b]; x[d] = rotl(x[d] ^ x[a], 16)
        x[c] = x[c] + x[d]; x[b] = rotl(x[b] ^ x[c], 12)
        x[a] = x[a] + x[b]; x[d] = rotl(x[d] ^ x[a], 8)
        x[c] = x[c] + x[d]; x[b] = rotl(x[b] ^ x[c], 7)

    for _ in range(10):
        quarter(0, 4, 8, 12); quarter(1, 5, 9, 13); quarter(2, 6, 10, 14); quarter(3, 7, 11, 15)
        quarter(0, 5, 10, 15); quarter(1, 6, 11, 12); quarter(2, 7, 8, 13); quarter(3, 4, 9, 14)
    w = [(a + b).astype(np.uint64) for a, b in zip(x, state)]
    return np.stack([w[2 * i] | (w[2 * i + 1] << np.uint64(32)) for i in range(8)], axis=1).reshape(n)


def uniform_row(key, nonce, b, j, nq, q, n, values=M.stream_values):
    """a[b][j][0 .. n): list of Python ints"""
    ls, hs = row_streams(b, j, nq)
    lo, hi = values(key, nonce, ls, n), values(key, nonce, hs, n)
    return [uniform_value(int(l), int(h), int(q)) for l, h in zip(lo, hi)]


def sample_uniform(key, nonce, count, limbs, moduli, n, values=M.stream_values):
    """what mkhe_sample_uniform writes: uint64 [count][limbs][n]; moduli = ALL the Q primes of the context (nQ = len(moduli))"""
    nq = len(moduli)
    return np.array([[uniform_row(key, nonce, b, j, nq, moduli[j], n, values) for j in range(limbs)] for b in range(count)], dtype=np.uint64)


def e_poly(key, nonce, b, n, cdt, values=M.stream_values):
    """e_b of mkhe_encrypt_sk_seeded: kind 1 on stream b of the SECRET (e_key, e_nonce)"""
    return [M.table(int(r), cdt) for r in values(key, nonce, b, n)]


def negacyclic(a, s, q):
    """a s mod (X^n + 1, q), schoolbook"""
    n = len(a)
    out = [0] * n
    for i in range(n):
        for k in range(n):
            t = a[i] * s[k]
            if i + k < n:
                out[i + k] += t
            else:
                out[i + k - n] -= t
    return [v % q for v in out]


def encrypt(a, s, pt, e, moduli):
    """(c0, c1) of one item: a, pt = [limbs][n] residues, s and e = [n] small integers -> two lists [limbs][n], canonical"""
    c0 = []
    for j, q in enumerate(moduli[: len(a)]):
        prod = negacyclic(a[j], s, q)
        c0.append([(pt[j][i] + e[i] - prod[i]) % q for i in range(len(s))])
    return c0, [list(r) for r in a]


def decrypt(c0, c1, s, moduli):
    """c0 + c1 s, canonical: [limbs][n]"""
    return [[(c0[j][i] + p) % q for i, p in enumerate(negacyclic(c1[j], s, q))] for j, q in enumerate(moduli[: len(c0)])]


def wire_bytes(limbs, n, seeded):
    """what a fresh ciphertext costs on the wire: c0 + 32 bytes of seed + 8 of nonce, or both polynomials"""
    return limbs * n * 8 + 40 if seeded else 2 * limbs * n * 8
