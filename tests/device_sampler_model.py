"""A model of the device sampler in Python integers only (include/mkhe.h, "device-side sampling"): the ChaCha20 block function of
RFC 8439 section 2.3, the mapping of (key, nonce, stream, coefficient) to a 64-bit value r, and the two kinds.  What
mkhe_sample_small and mkhe_encrypt_seeded are compared with, bit for bit; no numpy, no floats."""
from fractions import Fraction

M32 = 0xFFFFFFFF
CONSTANTS = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)


def _rotl(x, n):
    return ((x << n) & M32) | (x >> (32 - n))


def _quarter(x, a, b, c, d):
    x[a] = (x[a] + x[b]) & M32; x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] = (x[c] + x[d]) & M32; x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] = (x[a] + x[b]) & M32; x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] = (x[c] + x[d]) & M32; x[b] = _rotl(x[b] ^ x[c], 7)


def chacha20_block(key, w12, w13, w14, w15):
    """RFC 8439 section 2.3: key = 8 words, then the four words behind it (the RFC's counter and its three nonce words) -> 16 output words"""
    state = list(CONSTANTS) + [int(k) & M32 for k in key] + [w12 & M32, w13 & M32, w14 & M32, w15 & M32]
    assert len(state) == 16
    x = list(state)
    for _ in range(10):
        _quarter(x, 0, 4, 8, 12); _quarter(x, 1, 5, 9, 13); _quarter(x, 2, 6, 10, 14); _quarter(x, 3, 7, 11, 15)
        _quarter(x, 0, 5, 10, 15); _quarter(x, 1, 6, 11, 12); _quarter(x, 2, 7, 8, 13); _quarter(x, 3, 4, 9, 14)
    return [(a + b) & M32 for a, b in zip(x, state)]


def stream_values(key, nonce, stream, n):
    """r for the coefficients 0 .. n-1 of one stream (n a multiple of 8): block c = i // 8, words 2 (i % 8) (low) and 2 (i % 8) + 1 (high)"""
    assert n % 8 == 0 and 0 <= nonce < 1 << 64 and 0 <= stream < 1 << 32
    out = []
    for c in range(n // 8):
        w = chacha20_block(key, c, nonce & M32, nonce >> 32, stream)
        out += [w[2 * j] | (w[2 * j + 1] << 32) for j in range(8)]
    return out


def ternary(r):
    """kind 0: P(0) = 1/2, P(+1) = P(-1) = 1/4"""
    return 0 if r & 1 else (1 if r & 2 else -1)


def table(r, cdt):
    """kind 1: #{t : r >= cdt[t]} - ncdt/2"""
    return sum(1 for t in cdt if r >= t) - len(cdt) // 2


def sample_poly(kind, key, nonce, stream, n, cdt=None):
    rs = stream_values(key, nonce, stream, n)
    return [ternary(r) for r in rs] if kind == 0 else [table(r, cdt) for r in rs]


def sample_small(kind, count, key, nonce, first_stream, n, cdt=None):
    """what mkhe_sample_small writes: [count][n]"""
    return [sample_poly(kind, key, nonce, first_stream + p, n, cdt) for p in range(count)]


def encrypt_samples(count, key, nonce, n, cdt):
    """the samples of mkhe_encrypt_seeded, in the layout mkhe_encrypt takes: [count][3][n] = u (kind 0), e0, e1 (kind 1); stream 3 b + j"""
    return [[sample_poly(0 if j == 0 else 1, key, nonce, 3 * b + j, n, cdt) for j in range(3)] for b in range(count)]


def table_probabilities(cdt):
    """the exact distribution a table implies for a uniform r: {value: Fraction}"""
    edges = [0] + list(cdt) + [1 << 64]
    half = len(cdt) // 2
    return {k - half: Fraction(edges[k + 1] - edges[k], 1 << 64) for k in range(len(cdt) + 1)}


def moments(prob):
    """(mean, variance) of {value: probability}, exact"""
    mean = sum(v * p for v, p in prob.items())
    return mean, sum(v * v * p for v, p in prob.items()) - mean * mean
