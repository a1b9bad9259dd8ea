"""The MK-BFV basis conversions column by column, and the plants that steer them (TEST INFRASTRUCTURE; CPU: numpy and Python integers).

basis_conv_kernel (csrc/poly_kernels.hip) serves ModUpQtoR, both halves of Rescale and the Quantize tail (mkbfv/basis_extension.go:49-96 over
mkrlwe/basis_extension.go:337-357, 537-646).  It forms the 128-bit multSum of up to 16 products from 32-bit columns -- c0 = sum y0 t0,
c1 = sum (y0 t1 + y1 t0), c2 = sum y1 t1, the carry-outs of c0 and c1 counted in k0 and k1 -- and reads vtimesqmodp at the float64 index
v = (u64) sum_i (double)y_i / (double)q_i.  Conv restates that per coefficient and RETURNS the intermediate values, so that a test can assert what a
plant reached: k0, k1, c2 < 2^64, the index, the representative over the modulus.  It equals oracle/pymodel.py::modup_literal on every vector
(tests/test_bfv_conv_model.py) and shares nothing with the C oracle.

Plants: every entry point gets the input residues for chosen reconstruction terms y (plant_modup, plant_rescale_first, plant_rescale_second,
plant_quantize); families() lists the tuples y per source basis: steer_model.patterns(), y_i = q_i - 1 in exactly k limbs for every k = 0..ns (index
k: every table entry), the tuples whose float index is one BELOW the exact floor (sums of many terms only), and per target modulus the tuple with the
largest c1 (hence k1), the largest c0 (k0) and the largest representative a bounded seeded search finds.

The 60-bit set (bfv60): 16 + 16 primes of Q and QMul and 2 special primes below 2^60, = 1 mod 2^11, gamma = 2 (alpha = 1), drawn by a seeded shuffle of
the 82 largest such primes; the first seed is kept under which c1 passes 2^64 (k1 >= 1) on a target limb in BOTH directions.  Attained (seed 0,
asserted by tests/test_bfv_conv_model.py): c1 / 2^64 = 1.221 for Q -> QMul and 1.175 for QMul -> Q.  bfv60(nq) for nq in {1, 7, 8, 15} are prefixes:
launch_basis_conv deals 7 target limbs per blockIdx.y, so 7 | 8 and 14 | 15 change the grid."""
import functools
import random

import harness_bfv as HB
import steer_model as S
from oracle import pymodel as M

R = 1 << 64
MASK = R - 1
M32 = (1 << 32) - 1

SEARCH = dict(wide=True, under=8, max_tries=3000)          # boundary_tuples for the BFV bases: bounded, a family may come back short


# ------------------------------------------------------------------ one conversion, one coefficient
class Col:
    """the multSum of one coefficient under one target modulus, the kernel's way"""
    __slots__ = ("c0", "c1", "c2", "k0", "k1", "c1_sum", "rlo", "hhi")

    def rhi(self, k1="kept"):
        carry = 1 if self.rlo < self.c0 else 0
        hi = self.k0 + (self.c1 >> 32) + self.c2 + carry
        if k1 == "kept":
            hi += self.k1 << 32
        elif k1 == "weight 2^0":
            hi += self.k1
        else:
            assert k1 == "dropped"
        return hi & MASK


def index_floor(y, mods):
    return S.index_exact(y, mods)


class Conv:
    """modUpExact from the basis src to the basis dst: tables as NewFastBasisExtender builds them, one coefficient at a time"""

    def __init__(self, src, dst):
        self.S, self.T = [int(q) for q in src], [int(p) for p in dst]
        self.ns, self.nt = len(self.S), len(self.T)
        self.Sp = Sp = S.prod(self.S)
        self.star = [M.mform(pow(Sp // q, -1, q), q) for q in self.S]                    # qoverqiinvqi
        self.sinv = [M.qinv64(q) for q in self.S]
        self.tab = [[M.mform((Sp // q) % p, p) for q in self.S] for p in self.T]           # qoverqimodp[j][i]
        self.vt = [[v * (p - Sp % p) % p for v in range(self.ns + 1)] for p in self.T]      # vtimesqmodp[j][v]
        self.tinv = [M.qinv64(p) for p in self.T]

    def y_of(self, x):
        """reconstructRNS: y_i = MRed(x_i, qoverqiinvqi_i)"""
        return [M.mred(int(v), t, q, qi) for v, t, q, qi in zip(x, self.star, self.S, self.sinv)]

    def x_of(self, y):
        """the source residues whose reconstruction terms are y: x_i = y_i (S / s_i) mod s_i"""
        return S.xp_of(y, self.S)

    def columns(self, y):
        cols = []
        for j, p in enumerate(self.T):
            c0 = c1 = c2 = k0 = k1 = c1_sum = 0
            for yi, t in zip(y, self.tab[j]):
                y0, y1, t0, t1 = yi & M32, yi >> 32, t & M32, t >> 32
                c0 += y0 * t0
                k0 += c0 >> 64
                c0 &= MASK
                c1 += y0 * t1
                k1 += c1 >> 64
                c1 &= MASK
                c1 += y1 * t0
                k1 += c1 >> 64
                c1 &= MASK
                c1_sum += y0 * t1 + y1 * t0
                c2 += y1 * t1                                # NOT wrapped: the kernel assumes it stays below 2^64 (asserted by the tests)
            c = Col()
            c.c0, c.c1, c.c2, c.k0, c.k1, c.c1_sum = c0, c1, c2, k0, k1, c1_sum
            c.rlo = (c0 + (c1 << 32)) & MASK
            c.hhi = (((c.rlo * self.tinv[j]) & MASK) * p) >> 64
            cols.append(c)
        return cols

    def finish(self, y, cols, index=S.index_literal, clip=None, k1="kept"):
        """(lazy representatives, v): rhi - hhi + p + vtimesqmodp[v] in 64 bits; index / clip / k1: the mutants"""
        v = index(y, self.S)
        vi = v if clip is None else min(v, clip)
        return [(c.rhi(k1) - c.hhi + p + self.vt[j][vi]) & MASK for j, (c, p) in enumerate(zip(cols, self.T))], v

    def lift_y(self, y, **mutant):
        cols = self.columns(y)
        out, v = self.finish(y, cols, **mutant)
        return out, v, cols

    def lift(self, x, **mutant):
        return self.lift_y(self.y_of(x), **mutant)

    def mutant_kw(self, name):
        kw = dict(MUTANTS[name])
        if kw.get("clip") == -1:
            kw["clip"] = self.ns - 1
        return kw


MUTANTS = {
    "exact floor": dict(index=index_floor),
    "y * (1.0/p)": dict(index=S.index_reciprocal),
    "reversed summation": dict(index=S.index_reversed),
    "table clipped at ns-1": dict(clip=-1),
    "k1 dropped": dict(k1="dropped"),
    "k1 at weight 2^0": dict(k1="weight 2^0"),
}


# ------------------------------------------------------------------ the three conversions of mkbfv, one coefficient at a time
class Trace:
    """what one conversion read at one coefficient"""

    def __init__(self, y, v, cols, out, mods):
        self.y, self.v, self.cols, self.out, self.mods = y, v, cols, out, mods

    def ratio(self):
        return max(z / p for z, p in zip(self.out, self.mods))


class BfvConv:
    def __init__(self, pset):
        self.Q, self.QMul, self.T = [int(q) for q in pset["Q"]], [int(q) for q in pset["QMul"]], int(pset["T"])
        self.nq = len(self.Q)
        self.Qp, self.Mp = S.prod(self.Q), S.prod(self.QMul)
        self.q2m, self.m2q = Conv(self.Q, self.QMul), Conv(self.QMul, self.Q)
        self.m_in_q = [self.Mp % q for q in self.Q]
        self.minv_q = [pow(self.Mp, -1, q) for q in self.Q]
        self.qinv_m = [pow(self.Qp, -1, p) for p in self.QMul]
        self.tinv = [pow(self.T, -1, m) for m in self.Q + self.QMul]

    # ---- the entry points: residues of ONE coefficient in, residues out, and the trace of every conversion on the way
    def modup_q_to_r(self, x):
        lift, v, cols = self.q2m.lift(x)
        return [int(a) for a in x] + lift, [Trace(self.q2m.y_of(x), v, cols, lift, self.QMul)]

    def rescale(self, x):
        pq = [int(a) * m % q for a, m, q in zip(x, self.m_in_q, self.Q)]
        y1 = self.q2m.y_of(pq)
        lift, v1, cols1 = self.q2m.lift_y(y1)
        qm = [(0 - l) * i % p for l, i, p in zip(lift, self.qinv_m, self.QMul)]
        y2 = self.m2q.y_of(qm)
        back, v2, cols2 = self.m2q.lift_y(y2)
        return back + qm, [Trace(y1, v1, cols1, lift, self.QMul), Trace(y2, v2, cols2, back, self.Q)]

    def quantize(self, xr):
        """xr: the 2 nq residues of a COEFFICIENT-domain R polynomial (before the multiplication by T)"""
        nq = self.nq
        tq = [int(a) * self.T % q for a, q in zip(xr[:nq], self.Q)]
        tm = [int(a) * self.T % p for a, p in zip(xr[nq:], self.QMul)]
        y = self.m2q.y_of(tm)
        lift, v, cols = self.m2q.lift_y(y)
        return [(a - l) * i % q for a, l, i, q in zip(tq, lift, self.minv_q, self.Q)], [Trace(y, v, cols, lift, self.Q)]

    # ---- the plants: input residues for chosen reconstruction terms
    def plant_modup(self, y):
        """ModUpQtoR: x_i = y_i (Q / q_i) mod q_i"""
        return self.q2m.x_of(y)

    def plant_rescale_first(self, y):
        """Rescale, Q -> QMul: the same, times QMul^-1 mod q_i (the entry point multiplies by QMul first)"""
        return [a * i % q for a, i, q in zip(self.q2m.x_of(y), self.minv_q, self.Q)]

    def plant_rescale_second(self, y):
        """Rescale, QMul -> Q: the source of the second conversion is the output of the first, W = -(u - delta Q) / Q mod QMul with u = x QMul mod Q
        and delta = float index - exact floor of the first conversion.  For the W whose reconstruction terms are y: u = -(W + d) Q mod QMul, d in
        {0, +1, -1}, u < Q, x = u QMul^-1 mod Q; kept only when the model confirms it.  None: this target has no preimage."""
        y = [int(a) for a in y]
        W, _ = M.crt(self.m2q.x_of(y), self.QMul)
        for d in (0, 1, -1):
            u = (-(W + d) * self.Qp) % self.Mp
            while u < self.Qp:
                x = [(u % q) * i % q for q, i in zip(self.Q, self.minv_q)]
                if self.rescale(x)[1][1].y == y:
                    return x
                u += self.Mp
        return None

    def plant_quantize(self, y, result=None, xsub=None):
        """Quantize: the 2 nq residues of the coefficient-domain R polynomial whose QMul part, after the multiplication by T, has the reconstruction
        terms y, and whose Q part after it is xsub -- or, with result, the Q part for which the Quantize output is result_j in limb j (the analogue
        of steer_model.xq_for_result)"""
        tm = self.m2q.x_of(y)
        if xsub is None:
            lift, _, _ = self.m2q.lift_y([int(a) for a in y])
            xsub = [(int(r) * self.Mp + l) % q for r, l, q in zip(result, lift, self.Q)]
        t = [int(a) for a in xsub] + tm
        return [a * i % m for a, i, m in zip(t, self.tinv, self.Q + self.QMul)]


# ------------------------------------------------------------------ the tuples
def _best_split(q, t):
    """the y < q with the largest y0 t1 + y1 t0: increasing in both halves, so one of the two corners of y <= q - 1"""
    t0, t1 = t & M32, t >> 32
    a, b = q - 1, (((q - 1) >> 32) - 1) << 32 | M32
    f = lambda y: (y & M32) * t1 + (y >> 32) * t0
    return a if f(a) >= f(b) else b


def families(conv, seed=0):
    """[(name, y)] over the source basis of conv"""
    return list(_families(tuple(conv.S), tuple(conv.T), seed))


@functools.lru_cache(maxsize=None)
def _conv(src, dst):
    return Conv(src, dst)


@functools.lru_cache(maxsize=None)
def _families(src, dst, seed):
    conv = _conv(src, dst)
    ns, rnd = conv.ns, random.Random(7919 * seed + len(src))
    # (a prime of 53 bits or fewer has no y < q whose quotient is 1.0: quotient_edge then names q itself, which is no residue)
    out = [(name, list(y)) for name, y in S.patterns(src, seed, **SEARCH) if all(v < q for v, q in zip(y, src))]
    # index k for every k = 0..ns: q_i - 1 in k limbs -- every quotient is 1.0 from 54 bits on; below, (double)(q - 1) / (double)q is
    # 1 - 2^-53 and the sum of k of them may floor to k - 1, so the limbs (k of them or more) are searched for
    for k in range(ns + 1):
        for attempt in range(64 * (ns + 1)):
            on = set(rnd.sample(range(ns), min(ns, k + attempt // 64)))
            y = [q - 1 if i in on else 0 for i, q in enumerate(src)]
            if S.index_literal(y, src) == k:
                out.append(("index %d: q-1 in %d limbs" % (k, len(on)), y))
                break
    for j, p in enumerate(dst):
        tab = conv.tab[j]
        out.append(("max c1 -> limb %d" % j, [_best_split(q, t) for q, t in zip(src, tab)]))
        out.append(("max c0 -> limb %d" % j, [(((q - 1) >> 32) - 1) << 32 | M32 for q in src]))
        # largest representative: rhi - hhi is the Montgomery quotient of sum y_i t_i, largest with the y_i = q_i - 1 of the largest t_i; the
        # table entry v (p - S mod p) mod p is whatever it is -- so: for every v the v limbs of largest t_i at q_i - 1, then seeded draws around the best
        order = sorted(range(ns), key=lambda i: -tab[i])
        best, best_z = None, -1
        cands = [[src[i] - 1 if i in set(order[:v]) else 0 for i in range(ns)] for v in range(ns + 1)]
        for _ in range(64):
            y = list(cands[rnd.randrange(len(cands))])
            for i in rnd.sample(range(ns), rnd.randrange(1, ns + 1)):
                y[i] = rnd.choice((src[i] - 1, src[i] - 1 - rnd.randrange(1 << 20), rnd.randrange(src[i])))
            cands.append(y)
        for y in cands:
            z = conv.lift_y(y)[0][j]
            if z > best_z:
                best, best_z = y, z
        out.append(("max repr -> limb %d" % j, best))
    return out


# ------------------------------------------------------------------ parameter sets
@functools.lru_cache(maxsize=None)
def _pool60(count=82, step=1 << 11):
    out, c = [], ((1 << 60) - 1) // step * step + 1
    while len(out) < count:
        if c < (1 << 60) and M._is_prime(c):
            out.append(c)
        c -= step
    return out


def _max_c1(src, dst):
    """the largest c1 a tuple over src reaches under any modulus of dst"""
    conv = _conv(tuple(src), tuple(dst))
    best = 0
    for j in range(conv.nt):
        y = [_best_split(q, t) for q, t in zip(conv.S, conv.tab[j])]
        best = max(best, conv.columns(y)[j].c1_sum)
    return best


@functools.lru_cache(maxsize=None)
def _bfv60_full():
    pool = _pool60()
    P, rest = pool[:2], pool[2:]
    for seed in range(64):
        draw = list(rest)
        random.Random(6000 + seed).shuffle(draw)
        Q, QMul = draw[:16], draw[16:32]
        if _max_c1(Q, QMul) >= R and _max_c1(QMul, Q) >= R:
            return dict(Q=Q, QMul=QMul, P=P, T=65537, seed=seed)
    raise AssertionError("no seed gives k1 >= 1 in both directions")


def bfv60(nq=16, logN=10):
    full = _bfv60_full()
    return dict(logN=logN, Q=full["Q"][:nq], QMul=full["QMul"][:nq], P=full["P"], T=full["T"])


def sets():
    """{name: parameter set}: the ones tests/test_gpu_bfv_conv_edges.py runs on the device"""
    out = {
        "PN15QP880_N11": dict(HB.BFV_PN15QP880, logN=11),
        "PN14QP439_N10": dict(HB.BFV_PN14QP439, logN=10),
        "N12_q4big": HB.small_bfv(12, 4, big=True),
    }
    for nq in (1, 7, 8, 15, 16):
        out["60bit_q%d" % nq] = bfv60(nq)
    return out


def reachable_top(mods):
    """the largest float index any tuple over mods has: every quotient and every partial sum is monotone in y (rounding to nearest is monotone), so
    it is the index of y_i = q_i - 1 everywhere -- ns when every quotient rounds to 1.0, less under primes of 53 bits or fewer"""
    return S.index_literal([q - 1 for q in mods], mods)


# ------------------------------------------------------------------ the planted set of one parameter set
QUANTIZE_VARIANTS = ("result 0", "result q-1", "result random", "xsub 0", "xsub q-1")


class Plants:
    """every tuple of families() as the input of every entry point that can carry it:
    modup    [(name, y, x)]                         x: nq residues under Q
    rescale  [(name, which, y, x)]                  which: 0 the Q -> QMul conversion, 1 the QMul -> Q one behind it
    missing  [(name, y)]                            targets of the second conversion without a preimage
    quantize [(name, y, variant, xr)]               xr: 2 nq residues of the coefficient-domain R polynomial; two variants per tuple"""

    def __init__(self, pset, seed=0):
        self.pset, self.bc = pset, BfvConv(pset)
        bc, rnd = self.bc, random.Random(seed)
        self.fq, self.fm = families(bc.q2m, seed), families(bc.m2q, seed)
        self.modup = [(name, y, bc.plant_modup(y)) for name, y in self.fq]
        self.rescale = [(name, 0, y, bc.plant_rescale_first(y)) for name, y in self.fq]
        self.missing = []
        for name, y in self.fm:
            x = bc.plant_rescale_second(y)
            if x is None:
                self.missing.append((name, y))
            else:
                self.rescale.append((name, 1, y, x))
        self.quantize = []
        for s, (name, y) in enumerate(self.fm):
            for variant in (QUANTIZE_VARIANTS[s % 5], QUANTIZE_VARIANTS[(s + 2) % 5]):
                if variant.startswith("result"):
                    r = {"0": [0] * bc.nq, "q-1": [q - 1 for q in bc.Q], "random": [rnd.randrange(q) for q in bc.Q]}[variant.split()[1]]
                    xr = bc.plant_quantize(y, result=r)
                else:
                    xr = bc.plant_quantize(y, xsub=[0] * bc.nq if variant == "xsub 0" else [q - 1 for q in bc.Q])
                self.quantize.append((name, y, variant, xr))


@functools.lru_cache(maxsize=None)
def plants(name):
    return Plants(sets()[name])


def family_of(name):
    """the family a tuple's name belongs to (the names of steer_model.patterns() and of families() carry a limb number)"""
    for key in ("alone", "quotient 1.0", "quotient <1", "max c1", "max c0", "max repr"):
        if key in name:
            return key
    return "index k" if name.startswith("index ") else name


# ------------------------------------------------------------------ where the plants sit
class Layout:
    """plant s sits at (polynomial, coefficient) = at[s]: in turn in each polynomial of `polys` (the first and the last of a call, or every component
    of a ciphertext), the first plants at the last coefficients N - 1 and N - 2 (the tail of the grid), the rest at seeded places"""

    def __init__(self, N, count, polys=(0, 2), seed=0):
        rnd = random.Random(seed)
        places = [(c, n) for c in polys for n in range(N - 2)]
        assert len(places) >= count, "ring too small for the planted set"
        rnd.shuffle(places)
        self.at = ([(c, n) for n in (N - 1, N - 2) for c in polys] + places)[:count]

    def put(self, polys, rows):
        """polys[c][l][n] = rows[s][l] at (c, n) = at[s]"""
        for (c, n), row in zip(self.at, rows):
            for l, v in enumerate(row):
                polys[c][l][n] = v
        return polys
