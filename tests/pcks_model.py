"""A model of the collective key switch to a recipient's public key (include/mkhe.h, "collective public-key switch") in Python integers on top
of device_sampler_model, decrypt_share_model and bfv_refresh_model.flood_value: the stream layout of a call, the share (h0, h1) and the merge,
from the oracle's ring pieces.  What mkhe_pcks_share and mkhe_pcks_merge are compared with, bit for bit."""
import numpy as np

import bfv_refresh_model as B
import decrypt_share_model as D
import device_sampler_model as M


def words(flood_bits):
    """W: the 64-bit words of a flood"""
    return B.words(flood_bits)


def streams(count, flood_bits):
    """the streams a call of `count` items reads: u, e1, and W words of flood per item"""
    return count * (2 + words(flood_bits))


def u_stream(count, b):
    return b


def e1_stream(count, b):
    return count + b


def flood_stream(count, b, flood_bits, w):
    return 2 * count + b * words(flood_bits) + w


def u_poly(key, nonce, count, b, n, values=M.stream_values):
    """u_b: kind 0 on stream b"""
    return [M.ternary(r) for r in values(key, nonce, u_stream(count, b), n)]


def e1_poly(key, nonce, count, b, n, cdt, values=M.stream_values):
    """e1_b: kind 1 on stream count + b"""
    return [M.table(r, cdt) for r in values(key, nonce, e1_stream(count, b), n)]


def flood_poly(key, nonce, count, b, n, flood_bits, values=M.stream_values):
    """E_b: kind 5, word w on stream 2 count + b W + w; flood_bits = 0 reads no stream"""
    W = words(flood_bits)
    if W == 0:
        return [0] * n
    cols = [values(key, nonce, flood_stream(count, b, flood_bits, w), n) for w in range(W)]
    return [B.flood_value([c[i] for c in cols], flood_bits) for i in range(n)]


def small_limbs(e, moduli):
    """e mod q_j, canonical, for every limb: uint64 [limbs][n]"""
    return D.flood_limbs(e, moduli)


def encrypt_zero(ks, pk, limbs, u, e0, e1):
    """harness.KeyGen.encrypt of the zero plaintext on GIVEN samples (encryptor.go:95-112) -> uint64 [2][limbs][N]"""
    r = ks.ringQ
    out = np.empty((2, limbs, ks.N), dtype=np.uint64)
    uq, e0q, e1q = (small_limbs(x, ks.Q[:limbs]) for x in (u, e0, e1))
    for j in range(limbs):
        un = r.mform(j, r.ntt(j, uq[j]))
        out[0, j] = r.add(j, r.intt(j, r.mul(j, un, pk[0][j])), e0q[j])
        out[1, j] = r.add(j, r.intt(j, r.mul(j, un, pk[1][j])), e1q[j])
    return out


def share(ks, c, sk, pk, u, e1, E):
    """(h0, h1) of one item: c uint64 [limbs][N] the party's polynomial (coefficient domain), sk its secret (NTT, Montgomery form), pk = (pk0, pk1)
    the recipient's public key as harness.KeyGen.gen_public_key gives it; u, e1, E lists of N Python ints -> uint64 [2][limbs][N], canonical.
    h0 = InvNTT(NTT(c) sk + NTT(u) pk0) + E: the two products are added in the NTT domain, the flood stands where e0 would."""
    r, limbs = ks.ringQ, c.shape[0]
    uq, e1q, Eq = (small_limbs(x, ks.Q[:limbs]) for x in (u, e1, E))
    out = np.empty((2, limbs, ks.N), dtype=np.uint64)
    for j in range(limbs):
        un = r.mform(j, r.ntt(j, uq[j]))
        w0 = r.add(j, r.mul(j, r.ntt(j, c[j]), sk[j]), r.mul(j, un, pk[0][j]))
        out[0, j] = r.add(j, r.intt(j, w0), Eq[j])
        out[1, j] = r.add(j, r.intt(j, r.mul(j, un, pk[1][j])), e1q[j])
    return out


def merge(moduli, c0, shares):
    """(c_0 + sum_i h0_i, sum_i h1_i), canonical: c0 uint64 [limbs][N] (any representative), shares [k] of [2][limbs][N] -> uint64 [2][limbs][N]"""
    q = np.array([int(m) for m in moduli[: c0.shape[0]]], dtype=np.uint64)[:, None]
    out = np.stack([np.asarray(c0, dtype=np.uint64) % q, np.zeros_like(np.asarray(c0, dtype=np.uint64))])
    for s in shares:
        out = (out + np.asarray(s, dtype=np.uint64)) % q
    return out


def noise_bound(parties, flood_bits, n, bound=19):
    """parties * (2^(flood_bits-1) + 2 n bound): mkrlwe.PublicKeySwitcher.NoiseBound"""
    return parties * ((1 << (flood_bits - 1) if flood_bits else 0) + 2 * n * bound)
