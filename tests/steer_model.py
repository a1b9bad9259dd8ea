"""Compensated switching keys and the planted ModDown / digit-lift edges (TEST INFRASTRUCTURE; CPU: numpy and Python integers).

An external product accumulates acc_j = sum_i MRed(h_i,j , bg_i,j) in the NTT domain, h = Decompose(a), bg in storage form (NTT, Montgomery).  With a
and the digits bg_i, i >= 1, drawn uniformly, compensate() solves digit 0 of the key for a chosen accumulator A_j = NTT_j(T_j): every key and every
digit stays non-trivial, and T -- a coefficient-domain polynomial whose Q and P residues are free per coefficient -- is what ModDown reads.  Plan
lays the values at which the float64 correction index v = (u64) sum_i (double)y_i / (double)p_i (basis_extension.go:537-646) sits on an integer, and
the Q residues that make the ModDown result 0, at fixed coefficients of an otherwise uniform T.

moddown_literal() is the reference's ModDownQPtoQ for one coefficient on oracle/pymodel.py::modup_literal: it shares nothing with the C oracle.
moddown_with_index() restates the same arithmetic around a pluggable index (the mutants of tests/test_steer_model.py)."""
import functools
import random

import numpy as np

from oracle import pymodel as M

R = 1 << 64
MASK = R - 1

VARIANTS = ("xq0", "xqmax", "zero")          # x_q = 0, x_q = q - 1, the x_q of a ModDown result 0 in every limb


def prod(xs):
    out = 1
    for x in xs:
        out *= int(x)
    return out


# ------------------------------------------------------------------ ModDown of one coefficient
@functools.lru_cache(maxsize=None)
def _star_inv(P):
    Pp = prod(P)
    return tuple(pow(Pp // p, -1, p) for p in P)


def y_of(xp, P):
    """reconstructRNS: y_i = x_i * (P/p_i)^-1 mod p_i"""
    return [int(x) * s % p for x, s, p in zip(xp, _star_inv(tuple(P)), P)]


def xp_of(y, P):
    """the P residues whose reconstruction terms are y"""
    Pp = prod(P)
    return [int(v) * (Pp // p) % p for v, p in zip(y, P)]


def index_literal(y, P):
    vi = 0.0
    for v, p in zip(y, P):
        vi += float(v) / float(p)
    return int(vi)


@functools.lru_cache(maxsize=None)
def _cofactors(P):
    Pp = prod(P)
    return Pp, tuple(Pp // p for p in P)


def index_exact(y, P):
    """floor(sum_i y_i / p_i), over the common denominator prod(P)"""
    Pp, co = _cofactors(tuple(int(p) for p in P))
    return sum(int(v) * c for v, c in zip(y, co)) // Pp


def index_reciprocal(y, P):
    vi = 0.0
    for v, p in zip(y, P):
        vi += float(v) * (1.0 / float(p))
    return int(vi)


def index_reversed(y, P):
    vi = 0.0
    for v, p in zip(reversed(y), reversed(P)):
        vi += float(v) / float(p)
    return int(vi)


def lift_with_index(xp, Q, P, index=index_literal, clip=None):
    """multSum: the un-reduced lift of [x]_P into every q_j around the index function; clip: the largest table entry a mutant keeps"""
    Pp = prod(P)
    y = y_of(xp, P)
    v = index(y, P)
    vt_index = v if clip is None else min(v, clip)
    out = []
    for q in Q:
        acc = sum(yi * M.mform((Pp // p) % q, q) for yi, p in zip(y, P)) & ((1 << 128) - 1)
        rhi, rlo = acc >> 64, acc & MASK
        hhi = (((rlo * M.qinv64(q)) & MASK) * q) >> 64
        out.append((rhi - hhi + q + vt_index * (q - Pp % q) % q) & MASK)
    return out, v


def _down(lift, xq, Q, P):
    Pp = prod(P)
    return [M.mred((l + 2 * q - int(x)) & MASK, q - M.mform(pow(Pp, -1, q), q), q, M.qinv64(q)) for l, x, q in zip(lift, xq, Q)]


def moddown_literal(xq, xp, Q, P):
    """one coefficient of ModDownQPtoQ (basis_extension.go:192-232) with the float64 index: ([x_j'], v); xq lazy (< 2q), xp lazy (< 2p)"""
    lift, v = M.modup_literal([int(x) for x in xp], list(P), list(Q))
    return _down(lift, xq, Q, P), v


def moddown_with_index(xq, xp, Q, P, index=index_literal, clip=None):
    lift, v = lift_with_index(xp, Q, P, index, clip)
    return _down(lift, xq, Q, P), v


MUTANTS = {
    "exact floor": dict(index=index_exact),
    "y * (1.0/p)": dict(index=index_reciprocal),
    "table clipped at np-1": dict(clip=-1),              # (-1: resolved to len(P) - 1 by mutant())
    "reversed summation": dict(index=index_reversed),
}


def mutant(name, xq, xp, Q, P):
    kw = dict(MUTANTS[name])
    if kw.get("clip") == -1:
        kw["clip"] = len(P) - 1
    return moddown_with_index(xq, xp, Q, P, **kw)


def xq_for_result(r, xp, Q, P):
    """the Q residues for which the literal ModDown of (xq, xp) is r_j in limb j: x_j = r_j * P + lift_j mod q_j"""
    lift, _ = M.modup_literal([int(x) for x in xp], list(P), list(Q))
    Pp = prod(P)
    return [(int(rj) * Pp + l) % q for rj, l, q in zip(r, lift, Q)]


# ------------------------------------------------------------------ the planted reconstruction terms
def quotient_edge(p):
    """(the last y with (double)y / (double)p == 1.0, the first below it), searched downwards from p - 1"""
    y = p - 1
    while float(y) / float(p) == 1.0:
        y -= 1
    return y + 1, y


def boundary_tuples(mods, seed=0, count=16, wide=False, under=0, max_tries=None):
    """{"below": [...], "above": [...], "above_hi": [...]} of tuples y over mods (the special primes, or the moduli of a gadget digit):
    below   : exact sum just below an integer k in 1..n-1, float index k      (the float index is one above the true floor)
    above   : exact sum just above k - 1 for the same k, float index k - 1
    above_hi: exact sum just above k, float index k                            (half as many: where a rounded-down quotient would lose the step)
    rounding: see below
    under   : (only when under > 0) exact sum just above k, float index k - 1  (the float index is one BELOW the true floor: a sum of many terms
              whose roundings went down; two or four special primes do not have it)
    The y of an integer X under M = prod(mods) sum to exactly k +- e/M for X = M - e and X = e (CRT), so small e are the values next to an
    integer; every other draw takes e between M * 2^-55 and M * 2^-52, the scale of one float64 rounding of the sum, where the order and the form of
    the operations start to decide.
    wide: those draws reach further, up to M * n * ulp(n) -- n roundings of a sum near n, each as large as half an ulp of that sum -- with the
    exponent drawn uniformly, so that a sum of sixteen terms near 8 (ulp 2^-49) is still met inside its own rounding error.
    max_tries: None -- a family the search cannot fill is an error (today's callers: two and four special primes); a number -- each of the two
    searches stops there and every family holds what was found, possibly nothing: the caller decides what it requires.
    Searched, never tabulated: a candidate is kept only if its float index and its exact floor are the intended ones."""
    n = len(mods)
    rnd = random.Random(1000003 * seed + n)
    out = {"below": [], "above": [], "above_hi": []}
    if under:
        out["under"] = []
    if n < 2:
        return out
    Mp = prod(mods)
    per_k = -(-count // (n - 1))
    want = {"below": count, "above": count, "above_hi": count // 2}
    if under:
        want["under"] = under
    seen = {kind: {} for kind in out}
    top = (8 * n << (n.bit_length() - 1)).bit_length() if wide else 0       # e / (M 2^-55) below 2^top: 8 n ulp(n) / 2^-52

    def rounding_scale():
        if not wide:
            return max(1, (Mp >> 55) * rnd.randrange(1, 9) + rnd.randrange(0, 1 << 16))
        b = rnd.randrange(0, top)
        return max(1, (Mp >> 55) * rnd.randrange(1 << b, 2 << b) + rnd.randrange(0, 1 << 16))

    tries = 0
    while any(len(out[kind]) < want[kind] for kind in out):
        tries += 1
        if max_tries is not None and tries > max_tries:
            break
        assert tries < 200000, "the search for boundary tuples found too few under these moduli"
        e = rnd.randrange(1, 1 << 16) if tries & 1 else rounding_scale()
        for kind, X in (("below", Mp - e), ("above", e)):
            y = y_of([X % m for m in mods], mods)
            fl, lit = index_exact(y, mods), index_literal(y, mods)
            if kind == "below":
                k, ok = fl + 1, lit == fl + 1
            else:
                k, ok = fl + 1, lit == fl
                if under and lit == fl - 1 and len(out["under"]) < want["under"] and seen["under"].get(fl, 0) < per_k:
                    seen["under"][fl] = seen["under"].get(fl, 0) + 1
                    out["under"].append(y)
                    continue
                if ok and fl >= 1 and len(out["above_hi"]) < want["above_hi"] and seen["above_hi"].get(fl, 0) < per_k:
                    seen["above_hi"][fl] = seen["above_hi"].get(fl, 0) + 1
                    out["above_hi"].append(y)
                    continue
            if kind == "above" and seen[kind].get(1, 0) < per_k and len(out[kind]) < want[kind]:
                y = [rnd.randrange(0, 64) for _ in mods]                 # just above 0: only small y (an X = e sums to 1 + e/M or more)
                y[rnd.randrange(n)] += 1
                assert index_exact(y, mods) == 0 and index_literal(y, mods) == 0
                seen[kind][1] = seen[kind].get(1, 0) + 1
                out[kind].append(y)
                continue
            if ok and 1 <= k <= n - 1 and len(out[kind]) < want[kind] and seen[kind].get(k, 0) < per_k:
                seen[kind][k] = seen[kind].get(k, 0) + 1
                out[kind].append(y)
    # rounding: values at the rounding scale on which a float index of another FORM takes another table entry than the literal one -- count / 4
    # of them for y * (1.0 / p), as many (three moduli and more: a two-term float sum commutes) for the reversed order of the terms
    out["rounding"] = []
    got = {index_reciprocal: 0, index_reversed: 0 if n >= 3 else count // 4}
    tries = 0
    while min(got.values()) < count // 4:
        tries += 1
        if max_tries is not None and tries > max_tries:
            break
        assert tries < 400000, "the search for rounding-scale tuples found too few under these moduli"
        e = rounding_scale()
        for X in (Mp - e, e):
            y = y_of([X % m for m in mods], mods)
            lit = index_literal(y, mods)
            for other in got:
                if got[other] < count // 4 and other(y, mods) != lit and y not in out["rounding"]:
                    got[other] += 1
                    out["rounding"].append(y)
    return out


def patterns(P, seed=0, **search):
    """search: keywords of boundary_tuples (none: today's families and today's requirement that each be filled)"""
    return list(_patterns(tuple(int(p) for p in P), seed, tuple(sorted(search.items()))))


@functools.lru_cache(maxsize=None)
def _patterns(P, seed, search=()):
    """[(name, y tuple)]: the planted [T]_P of one parameter set, as reconstruction terms y"""
    n = len(P)
    pats = [("y=0", [0] * n), ("x_P=1", y_of([1] * n, P)), ("y=p-1 all", [p - 1 for p in P])]
    for i, p in enumerate(P):
        pats.append(("y_%d=p-1 alone" % i, [p - 1 if k == i else 0 for k in range(n)]))
    for i, p in enumerate(P):
        one, below = quotient_edge(p)
        pats.append(("y_%d last quotient 1.0" % i, [one if k == i else 0 for k in range(n)]))
        pats.append(("y_%d first quotient <1" % i, [below if k == i else 0 for k in range(n)]))
    for kind, ts in boundary_tuples(list(P), seed, **dict(search)).items():
        for t in ts:
            pats.append((kind, t))
    return pats


# ------------------------------------------------------------------ where the patterns sit
def flips(n, galEl, logN):
    return ((n * galEl) >> logN) & 1


def galois_elements(logN, rots=(1, 5)):
    N2 = 2 << logN
    return [pow(5, r, N2) for r in rots] + [N2 - 1]


class Plan:
    """The layout of one parameter set: pattern s, variant w sits at coefficient pos[s][w]; the "zero" variants sit where every Galois element of
    gals flips the sign, except the control (coefficient 0, which no automorphism flips) that carries "y=p-1 all" with a zero result; free[]: coefficients
    left to the caller (the final values of the fused Rescale)."""

    def __init__(self, Q, P, logN, level, seed=0, gals=None, nfree=8):
        self.Q, self.P, self.logN, self.N, self.level = [int(q) for q in Q], [int(p) for p in P], logN, 1 << logN, level
        self.Ql = self.Q[: level + 1]
        self.gals = galois_elements(logN) if gals is None else list(gals)
        self.pats = patterns(self.P, seed)
        rnd = random.Random(seed)
        flipping = [n for n in range(1, self.N) if all(flips(n, g, logN) for g in self.gals)]
        rest = [n for n in range(1, self.N) if not all(flips(n, g, logN) for g in self.gals)]
        rnd.shuffle(flipping)
        rnd.shuffle(rest)
        S = len(self.pats)
        assert len(flipping) >= S and len(rest) >= 2 * S + nfree, "ring too small for the planted set"
        self.pos = [(rest[2 * s], rest[2 * s + 1], flipping[s]) for s in range(S)]
        self.free = rest[2 * S: 2 * S + nfree]
        self.control = 0
        self.rng = np.random.default_rng(seed)

    def planted(self):
        """[(coefficient, pattern name, variant)] with the control last"""
        out = [(self.pos[s][w], self.pats[s][0], VARIANTS[w]) for s in range(len(self.pats)) for w in range(3)]
        return out + [(self.control, "y=p-1 all", "zero")]

    def zero_positions(self):
        return [p[2] for p in self.pos] + [self.control]

    def target(self, rng, results=None, shift=0):
        """T: uint64 [nQ + nP][N] (coefficient domain; rows of Q above the level are zero), uniform with the planted coefficients.
        results: {coefficient: [r_j]} -- Q residues chosen so that the ModDown result there is r (over whatever P residues the coefficient has)"""
        nq, mods = len(self.Q), self.Q + self.P
        T = np.zeros((len(mods), self.N), dtype=np.uint64)
        for j, q in enumerate(mods):
            if j <= self.level or j >= nq:
                T[j] = rng.integers(0, q, self.N, dtype=np.uint64)
        S = len(self.pats)
        def put(n, xq, xp):
            for j in range(self.level + 1):
                T[j, n] = xq[j]
            for i in range(len(self.P)):
                T[nq + i, n] = xp[i]
        for s in range(S):
            xp = xp_of(self.pats[(s + shift) % S][1], self.P)
            put(self.pos[s][0], [0] * len(self.Ql), xp)
            put(self.pos[s][1], [q - 1 for q in self.Ql], xp)
            put(self.pos[s][2], xq_for_result([0] * len(self.Ql), xp, self.Ql, self.P), xp)
        xp = xp_of([p - 1 for p in self.P], self.P)
        put(self.control, xq_for_result([0] * len(self.Ql), xp, self.Ql, self.P), xp)
        for n, r in (results or {}).items():
            xp = [int(T[nq + i, n]) for i in range(len(self.P))]
            put(n, xq_for_result(r, xp, self.Ql, self.P), xp)
        return T


def rescale_finals(qL):
    """dropped-limb residues t of a final value on the rounding boundary of DivRoundByLastModulus (h = (qL - 1) >> 1): t + h in {qL - 1, qL, qL + 1}
    (mod qL) and t in {0, h, h + 1, qL - 1}"""
    h = (qL - 1) >> 1
    return sorted({(qL - 1 - h) % qL, (qL - h) % qL, (qL + 1 - h) % qL, 0, h, h + 1, qL - 1})


# ------------------------------------------------------------------ the compensated key
def _obj(a):
    return np.asarray(a, dtype=np.uint64).astype(object)


def ntt_target(ks, level, T):
    """A_j = NTT_j(T_j) over Q[:level + 1] and P (rows of Q above the level stay zero)"""
    nq = len(ks.Q)
    A = np.zeros_like(T)
    for j in range(level + 1):
        A[j] = ks.ringQ.ntt(j, T[j])
    for i in range(len(ks.P)):
        A[nq + i] = ks.ringP.ntt(i, T[nq + i])
    return A


def compensate(ks, level, h, bg, target_ntt):
    """bg with digit 0 replaced so that sum_i MRed(h_i,j , bg_i,j) = target_ntt[j] on every active limb j (Q[:level + 1] and P):
    bg_0,j = MForm((A_j - sum_{i >= 1} h_i,j * invMForm(bg_i,j)) * h_0,j^-1 mod q_j).  Raises ValueError when h_0 has a zero (probability about
    N * limbs / 2^45: the caller takes the next seed; no coefficient is ever left out)."""
    nq, beta = len(ks.Q), ks.beta(level)
    out = np.array(bg, dtype=np.uint64, copy=True)
    mods = ks.Q + ks.P
    Rinv = {q: pow(R, -1, q) for q in mods}
    for j in list(range(level + 1)) + [nq + i for i in range(len(ks.P))]:
        q = mods[j]
        h0 = _obj(h[0][j])
        if (h0 == 0).any():
            raise ValueError("digit 0 has a zero in limb %d" % j)
        rest = np.zeros(ks.N, dtype=object)
        for i in range(1, beta):
            rest = (rest + _obj(h[i][j]) * _obj(bg[i][j]) * Rinv[q]) % q
        inv = np.array([pow(int(v), -1, q) for v in h0], dtype=object)
        out[0][j] = (((_obj(target_ntt[j]) - rest) * inv % q) * R % q).astype(np.uint64)
    return out


def steer(ks, level, h, rng, T, uniform_swk):
    """a uniform key compensated for the digits h so that ModDown reads T"""
    return compensate(ks, level, h, uniform_swk(rng, ks), ntt_target(ks, level, T))


# ------------------------------------------------------------------ whole operations with steered keys (oracle side)
def rotate_case(ks, plan, level, n, rng, H, chosen=None, conj_gal=None, shift=False):
    """(ct, keys, crs) of a Rotate (conj_gal None) or a Conjugate of an n-party ciphertext: party a's rk_a / ck_a steered to its own target, the CRS
    steered for the digits of party `chosen` (default: the last), c_0 zero where every member's ModDown result is zero -- so that every partial
    sum of out_0 is 0 there and the signed permutation of a Rotate stores q."""
    chosen = n - 1 if chosen is None else chosen
    ct = H.uniform_ct(rng, ks, n, level + 1)
    if conj_gal is None:
        ct[0][:, plan.zero_positions()] = 0
    src = ct if conj_gal is None else np.stack([ks.ringQ.permute(conj_gal, ct[s]) for s in range(1 + n)])
    hs = [ks.decompose(level, src[1 + a]) for a in range(n)]
    keys = [steer(ks, level, hs[a], rng, plan.target(rng, shift=a if shift else 0), H.uniform_swk) for a in range(n)]
    crs = steer(ks, level, hs[chosen], rng, plan.target(rng), H.uniform_swk)
    return ct, keys, crs


def mulrelin_case(ks, plan, level, n, rng, H, finals=None, all_max=False):
    """(op0, op1, rlk, u, F) of a MulAndRelin of two n-party ciphertexts with equal id sets 0..n-1: every v_i (rlk[i][2]) is steered for the digits
    h(t_i), t_i = <h(c0_i), y>_P, that the oracle's own steps A-C and F1 produce (oracle.mr_xy, external_product, decompose); the last member's Q
    residues at plan.free cancel the tensor term and the other members, so that out_0 there is finals[k] (F: {coefficient: [F_j]}).
    all_max: the NTT-domain accumulator of every member is q_j - 1 at every point instead."""
    ids = list(range(n))
    op0, op1 = H.uniform_ct(rng, ks, n, level + 1), H.uniform_ct(rng, ks, n, level + 1)
    rlk = {i: tuple(H.uniform_swk(rng, ks) for _ in range(3)) for i in ids}
    u = H.uniform_swk(rng, ks)
    _, y = ks.mr_xy(level, ids, op0, ids, op1, rlk, True)
    hs = [ks.decompose(level, ks.external_product(level, op0[1 + a], y)) for a in ids]
    nq, Ql = len(ks.Q), ks.Q[: level + 1]
    if all_max:
        A = np.zeros((ks.m, ks.N), dtype=np.uint64)
        for j, q in enumerate(ks.Q + ks.P):
            if j <= level or j >= nq:
                A[j] = q - 1
        for a in ids:
            rlk[a] = rlk[a][:2] + (compensate(ks, level, hs[a], rlk[a][2], A),)
        return op0, op1, rlk, u, {}
    # the tensor term of out_0: the oracle's out_0 under the uniform keys minus their own products
    _, base = ks.mul_and_relin(level, ids, op0, ids, op1, rlk, u)
    tensor = base[0]
    for a in ids:
        e = ks.external_product_hoisted(level, hs[a], rlk[a][2])
        tensor = np.stack([ks.ringQ.sub(j, tensor[j], e[j]) for j in range(level + 1)])
    others = np.zeros_like(tensor)
    for a in ids[:-1]:
        v = steer(ks, level, hs[a], rng, plan.target(rng), H.uniform_swk)
        rlk[a] = rlk[a][:2] + (v,)
        e = ks.external_product_hoisted(level, hs[a], v)
        others = np.stack([ks.ringQ.add(j, others[j], e[j]) for j in range(level + 1)])
    F = {}
    if finals is not None:
        for pos, t in zip(plan.free, finals):
            F[pos] = [int(rng.integers(0, q)) for q in Ql[:-1]] + [int(t)]
    results = {pos: [(f - int(tensor[j, pos]) - int(others[j, pos])) % Ql[j] for j, f in enumerate(Fv)] for pos, Fv in F.items()}
    last = ids[-1]
    rlk[last] = rlk[last][:2] + (steer(ks, level, hs[last], rng, plan.target(rng, results=results), H.uniform_swk),)
    return op0, op1, rlk, u, F
