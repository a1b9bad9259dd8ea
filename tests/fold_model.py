"""Big-integer model of the fold epilogues of the sharded paths (TEST INFRASTRUCTURE): mkhe_swk_fold, mkhe_ct_fold and
mkhe_swk_fold_pieces of include/mkhe.h restated with Python integers, so that it holds for any word value and any number of
summands -- where a uint64 sum (numpy, or the kernel before it reduced per summand) wraps 2^64.

    fold_words    word -> word mod q [times 2^64 mod q: MForm]                     (fold_kernel, csrc/poly_kernels.hip)
    fold_pieces   a limb range of a switching-key buffer <- fold_words(sum of the pieces); limb l is digit l // (nQ + nP) and
                  modulus l % (nQ + nP); limbs of inactive digits / moduli keep what dst held        (fold_pieces_kernel)
"""
import numpy as np

import harness as H

R = 1 << 64

# the two parameter sets of the fold tests, N = 2^11: 4 Q + 2 P moduli, gamma = 2 -> alpha = 1, four digits: 24 switching-key limbs
SETS = {
    "pn15": H.small_ckks(11, 4),                                                                    # 60-bit + 3 x 54-bit Q, 2 x 59-bit P
    "pn14": dict(logN=11, Q=H.PN14QP439["Q"][:4], P=H.PN14QP439["P"], scale=float(1 << 52)),      # 59-bit + 3 x 52-bit Q, 2 x 60-bit P
}


def fold_words(words, q, mform):
    """(w * (2^64 if mform else 1)) % q per word, as a uint64 array of the shape of `words` (any integers, any size)"""
    w = np.asarray(words, dtype=object)
    q = int(q)
    out = (w * R) % q if mform else w % q
    return np.asarray(out, dtype=np.uint64).reshape(np.shape(words))


def exact_sum(pieces):
    """sum over axis 0 of a uint64 array as Python integers (an object array).  The 32-bit halves are summed apart -- each sum is below
    npieces * 2^32, exact in uint64 for any npieces < 2^32 -- and put together as integers, so nothing ever wraps."""
    pieces = np.asarray(pieces, dtype=np.uint64)
    assert pieces.shape[0] < 1 << 32
    lo = (pieces & np.uint64(0xffffffff)).sum(axis=0, dtype=np.uint64)
    hi = (pieces >> np.uint64(32)).sum(axis=0, dtype=np.uint64)
    return hi.astype(object) * (1 << 32) + lo.astype(object)


def active_limb(l, level, nq, np_, ndigits):
    """-> the modulus index of limb l if the limb is active at `level` (digit < ndigits, modulus in {0..level} or a P modulus), else None"""
    digit, m = divmod(int(l), nq + np_)
    return m if digit < ndigits and (m <= level or m >= nq) else None


def fold_pieces(pieces, first_limb, nlimbs, level, mform, Q, P, beta, dst_before):
    """pieces: uint64[npieces][nlimbs][N] (summand p of limb first_limb + i at pieces[p][i]); beta: level -> number of active digits;
    dst_before: uint64[nlimbs][N], what the destination held.  -> uint64[nlimbs][N]"""
    pieces = np.asarray(pieces, dtype=np.uint64)
    out = np.array(dst_before, dtype=np.uint64, copy=True)
    assert pieces.ndim == 3 and pieces.shape[1] == nlimbs and out.shape == pieces.shape[1:]
    moduli = [int(q) for q in Q] + [int(p) for p in P]
    ndigits = beta(level)
    for i in range(nlimbs):
        m = active_limb(first_limb + i, level, len(Q), len(P), ndigits)
        if m is None:
            continue
        out[i] = fold_words(exact_sum(pieces[:, i, :]), moduli[m], mform)
    return out


def bound_table(q):
    """the words at which a fold can go wrong, all inside its documented domain (< 2^63): the ends of [0, q], the largest sum of 8 residues, the
    largest multiple of q below 2^63 with its two neighbours, and the top of the domain"""
    q = int(q)
    top = ((1 << 63) - 1) // q * q
    return [0, 1, q - 1, q, 8 * (q - 1), top - 1, top, top + 1, (1 << 63) - 1]
