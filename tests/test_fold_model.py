"""tests/fold_model.py (the big-integer reference of tests/test_gpu_fold.py) against the C oracle's reduce + MForm, against a table worked
out by hand, and the arithmetic facts the device cases rely on.  No GPU."""
import numpy as np
import pytest

import fold_model as FM
import harness as H
from oracle import oracle as O

SETS = FM.SETS
Q54, Q59, Q60 = H.PN15QP880["Q"][1], H.PN15QP880["P"][0], H.PN15QP880["Q"][0]
PRIMES60 = [H.PN15QP880["Q"][0]] + H.PN14QP439["P"]


def test_the_primes_are_what_the_cases_assume():
    assert [q.bit_length() for q in (Q54, Q59, Q60)] == [54, 59, 60]
    assert all(q.bit_length() == 60 for q in PRIMES60)
    assert Q60 in SETS["pn15"]["Q"] and Q59 in SETS["pn15"]["P"] and Q54 in SETS["pn15"]["Q"]
    assert all(p in SETS["pn14"]["P"] for p in H.PN14QP439["P"])
    for pset in SETS.values():
        assert len(pset["Q"]) == 4 and len(pset["P"]) == 2


def test_sums_of_8_residues_are_in_the_domain_and_17_wrap():
    for pset in SETS.values():
        for q in pset["Q"] + pset["P"]:
            assert 8 * (q - 1) < 2 ** 63
            assert all(w < 2 ** 63 for w in FM.bound_table(q))
    for q in PRIMES60:
        assert 16 * (q - 1) < 2 ** 64 <= 17 * (q - 1)           # the 17-piece case wraps a uint64 sum: an unreduced sum cannot pass it
    assert 32 * (Q59 - 1) < 2 ** 64 <= 33 * (Q59 - 1)


@pytest.mark.parametrize("q", [Q54, Q59, Q60])
@pytest.mark.parametrize("mform", [0, 1])
def test_fold_words_hand_table(q, mform):
    top = (2 ** 63 - 1) // q * q
    table = FM.bound_table(q)
    assert table == [0, 1, q - 1, q, 8 * q - 8, top - 1, top, top + 1, 2 ** 63 - 1]
    plain = [0, 1, q - 1, 0, q - 8, q - 1, 0, 1, 2 ** 63 - 1 - top]       # residues read off the table: 8q - 8 = 7q + (q - 8), top = 0 (mod q)
    assert 0 <= 2 ** 63 - 1 - top < q and top % q == 0 and top + q > 2 ** 63 - 1
    r1 = pow(2, 64, q)
    want = [p * r1 % q for p in plain] if mform else plain
    got = FM.fold_words(np.array(table, dtype=np.uint64), q, mform)
    assert got.dtype == np.uint64 and [int(v) for v in got] == want
    # any integers, not only uint64 words
    assert [int(v) for v in FM.fold_words([17 * (q - 1), 64 * (q - 1), 2 ** 70 + 3], q, 0)] == [q - 17, q - 64, (2 ** 70 + 3) % q]


@pytest.mark.parametrize("name", sorted(SETS))
def test_fold_words_agrees_with_the_oracle(oracle_lib, name):
    """ring.mform(k, ring.reduce(k, tot)) is what OracleShardBackend computes: two independent statements of the same operation"""
    pset = SETS[name]
    rng = np.random.default_rng(5)
    for ring in (O.Ring(pset["logN"], pset["Q"]), O.Ring(pset["logN"], pset["P"])):
        N = ring.N
        for k, q in enumerate(ring.moduli):
            for nsum in (1, 2, 8):
                tot = sum(rng.integers(0, q, N, dtype=np.uint64) for _ in range(nsum))
                tot[:9] = np.array(FM.bound_table(q), dtype=np.uint64)
                assert int(tot.max()) < 2 ** 63
                red = ring.reduce(k, tot)
                assert (FM.fold_words(tot, q, 0) == red).all()
                assert (FM.fold_words(tot, q, 1) == ring.mform(k, red)).all()


def test_fold_pieces_rule():
    """digit = l // (nQ + nP), modulus = l % (nQ + nP); active: digit < beta(level) and modulus in {0..level} or P"""
    pset = SETS["pn15"]
    Q, P = pset["Q"], pset["P"]
    beta = lambda level: level + 1                                  # alpha = 1
    assert [FM.active_limb(l, 3, 4, 2, 4) for l in range(24)] == [0, 1, 2, 3, 4, 5] * 4
    assert [FM.active_limb(l, 1, 4, 2, 2) for l in range(24)] == [0, 1, None, None, 4, 5] * 2 + [None] * 12
    assert [FM.active_limb(l, 0, 4, 2, 1) for l in range(24)] == [0, None, None, None, 4, 5] + [None] * 18
    rng = np.random.default_rng(11)
    N, first, n = 8, 4, 9                                           # limbs 4..12: moduli 4, 5 of digit 0, all of digit 1, modulus 0 of digit 2
    mods = (Q + P) * 4
    for npieces in (1, 3, 40):                                      # 40 pieces of q - 1 wrap a uint64 sum for every modulus of the set
        pieces = np.stack([np.stack([np.full(N, mods[first + i] - 1, dtype=np.uint64) for i in range(n)]) for _ in range(npieces)])
        pieces[:, :, 1:] = np.stack([np.stack([rng.integers(0, mods[first + i], N - 1, dtype=np.uint64) for i in range(n)]) for _ in range(npieces)])
        before = rng.integers(0, 2 ** 64, (n, N), dtype=np.uint64)
        for level in (3, 1, 0):
            for mform in (0, 1):
                got = FM.fold_pieces(pieces, first, n, level, mform, Q, P, beta, before)
                for i in range(n):
                    l = first + i
                    digit, m = divmod(l, 6)
                    if digit <= level and (m <= level or m >= 4):
                        q = mods[l]
                        want = [sum(int(pieces[p, i, c]) for p in range(npieces)) * (2 ** 64 if mform else 1) % q for c in range(N)]
                        assert [int(v) for v in got[i]] == want
                        assert int(got[i][0]) == (q - npieces) * (pow(2, 64, q) if mform else 1) % q
                    else:
                        assert (got[i] == before[i]).all()
    empty = FM.fold_pieces(np.zeros((2, 0, N), dtype=np.uint64), 7, 0, 3, 1, Q, P, beta, np.zeros((0, N), dtype=np.uint64))
    assert empty.shape == (0, N)
