"""Exact Python-integer models of the device arithmetic of csrc/modarith.h and csrc/h16_arith.h, the contracts their header comments state, the
twiddle packings of the Context constructor (csrc/engine.hip: sd_split, pack, pair_of) and the edge operands that tests/test_arith_model.py (CPU)
and tests/test_gpu_arith_probe.py (GPU, through lib/libmkhe_arith_probe.so) run them on.

Every model is written from the formula in the primitive's comment, in unbounded integers: it returns the SIGNED (or unsigned) representative the
device returns, not just the residue class, as long as no device accumulator wraps -- which is what the contracts promise.  pred and bflyF are
not modelled (their quotient comes out of a floating-point estimate): their reference is the contract itself, see check_pred / check_bflyF.
Every model takes an optional `mut` naming one deliberately wrong variant; the CPU tests show that the edge vectors alone tell each from the truth.
"""
import functools
import random
import struct

M32 = (1 << 32) - 1
M64 = (1 << 64) - 1
B63 = 1 << 63              # mont_mul_lazy: a < 2^63
B62 = 1 << 62              # mont_mul_sd, mm, mm30u: |a| < 2^62
B629 = int(2 ** 62.9)      # mm31, pred: |a| < 2^62.9
BLOCK = 256                # the probe's workgroup: the SW forms take one twiddle per BLOCK elements


def lo32(x):
    return x & M32


def hi32(x):
    return (x >> 32) & M32


def s32(x):
    x &= M32
    return x - (1 << 32) if x >> 31 else x


def s64(x):
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def sext(x, bits):
    """the low `bits` bits of x as a signed number (v_bfe_i32 x, 0, bits)"""
    x &= (1 << bits) - 1
    return x - (1 << bits) if x >> (bits - 1) else x


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def bits_f64(b):
    return struct.unpack("<d", struct.pack("<Q", b & M64))[0]


# ---------------------------------------------------------------- per-modulus constants (engine.hip, Context constructor)
class Mod:
    def __init__(self, q):
        assert q & 1
        self.q = q
        self.qinv = pow(q, -1, 1 << 64)
        self.ninv32 = (-self.qinv) & M32
        self.finv = f32_bits(4294967296.0 / float(q)) if q > (1 << 33) else 0    # float32 of 2^32 / q (struct rounds to nearest even, like the cast)
        self.qs = sd_split(q)
        self.r1 = (1 << 64) % q

    def words(self):
        """what the probe's `mod` argument takes"""
        return [self.q, self.qinv, self.ninv32, self.finv]

    def p(self, sh):
        """balanced radix-2^sh digits of q: q = p1 2^sh + p0, |p0| <= 2^(sh - 1)"""
        p0 = sext(self.q, sh)
        return p0, (self.q - p0) >> sh


def sd_split(v):
    """(hi, lo) with v = s32(hi) 2^32 + s32(lo): the high word absorbs the carry of reading the low word as signed"""
    return (v + ((lo32(v) >> 31) << 32)) & M64


def pack(x, balanced, sh, q):
    """engine.hip `pack`: radix-2^sh digits (d1, d0) of x mod q (balanced: of its representative in (-q/2, q/2], with a signed low digit)"""
    b = x - q if balanced and x > q // 2 else x
    d0 = b & ((1 << sh) - 1)
    if balanced and d0 >= 1 << (sh - 1):
        d0 -= 1 << sh
    d1 = (b - d0) >> sh
    return (d0 & M32) | ((d1 & M32) << 32)


@functools.lru_cache(maxsize=4096)
def pair_of(w, q, uc):
    """engine.hip `pair_of` for the plain twiddle w: (u, v) = packed (w 2^sh, w 2^(sh + 32)) mod q; sh = 30 and u unsigned in the U class"""
    sh = 30 if uc else 31
    wR = (w << 64) % q
    cinv = pow(pow(2, 64 - sh, q), -1, q)
    u = wR * cinv % q
    v = u * pow(2, 32, q) % q
    return pack(u, not uc, sh, q), pack(v, True, sh, q)


# ---------------------------------------------------------------- models: modarith.h
def mont_mul_lazy(a, w, md, mut=None):
    """a w 2^-64 mod q in [0, 2q) for a < 2^63, w < q: two rounds of radix 2^32"""
    q, ninv = md.q, md.ninv32
    a0, a1 = lo32(a), hi32(a)
    m = lo32(lo32(a0 * lo32(w)) * ninv)
    T = (a0 * w + m * q) >> 32
    if mut == "round1_reuses_m":
        m2 = m
    else:
        m2 = lo32(lo32(a1 * lo32(w) + T) * ninv)
    if mut == "carry_dropped":                     # the low words' carry into the high half is lost
        return ((a1 * w + m2 * q) >> 32) + (T >> 32)
    return (T + a1 * w + m2 * q) >> 32


def csub(a, q, mut=None):
    if mut == "gt":
        return a - q if a > q else a
    if mut == "never":
        return a
    return a - q if a >= q else a


def mont_mul(a, w, md, mut=None):
    if mut in ("gt", "never"):
        return csub(mont_mul_lazy(a, w, md), md.q, mut)
    return csub(mont_mul_lazy(a, w, md, mut), md.q)


def digits_sd(a, mut=None):
    """balanced 32-bit digits of the signed 64-bit a: a = a1 2^32 + a0, with the `+ (al >> 31)` carry"""
    al = lo32(a)
    a0 = s32(al)
    if mut == "digit_carry_dropped":
        return a0, s32(hi32(a))
    return a0, s32(hi32(a) + (al >> 31))


def mont_mul_sd(a, ws, md, mut=None):
    """a w 2^-64 mod q as the signed representative of modarith.h mont_mul_sd / h16_arith.h mm: a signed, ws and qs in signed-split form"""
    ninv = md.ninv32
    a0, a1 = digits_sd(a, mut)
    w0, w1, q0, q1 = s32(lo32(ws)), s32(hi32(ws)), s32(lo32(md.qs)), s32(hi32(md.qs))
    shr = (lambda x: (x & M64) >> 32) if mut == "logical_shift" else (lambda x: x >> 32)
    red = lo32 if mut == "unsigned_m" else s32
    P0 = a0 * w0
    m = red(lo32(P0) * ninv)
    S = m * q0 + P0
    Y = m * q1 + a0 * w1 + shr(S)
    U = a1 * w0 + Y
    m2 = red(lo32(U) * ninv)
    S2 = m2 * q0 + U
    return m2 * q1 + a1 * w1 + shr(S2)


def mont_mul_sdu(a, ws, md, mut=None):
    if mut == "bias_dropped":
        return mont_mul_sd(s64(a), ws, md)
    return mont_mul_sd(s64(a), ws, md, mut) + md.q


def mul64x64(a, b, mut=None):
    """(hi, lo) of the 128-bit product"""
    if mut == "cross_carry_dropped":               # the carry of the two cross products into the high word is lost
        a0, a1, b0, b1 = lo32(a), hi32(a), lo32(b), hi32(b)
        mid = lo32(a0 * b1) + lo32(a1 * b0) + hi32(a0 * b0)
        return (a1 * b1 + hi32(a0 * b1) + hi32(a1 * b0)) & M64, ((mid << 32) | lo32(a0 * b0)) & M64
    if mut == "signed_words":
        p = s64(a) * s64(b)
        return (p >> 64) & M64, p & M64
    p = a * b
    return p >> 64, p & M64


def mac128(a, b, hi, lo, mut=None):
    """(hi, lo) += a b, mod 2^128"""
    h, l = mul64x64(a, b)
    lo2 = (lo + l) & M64
    carry = 1 if lo2 < l else 0
    if mut == "carry_dropped":
        carry = 0
    if mut == "carry_always":
        carry = 1
    return (hi + h + carry) & M64, lo2


def redc128(hi, lo, md, mut=None):
    """(hi 2^64 + lo) 2^-64 mod q, canonical, for hi < 2q"""
    q = md.q
    mh = ((lo * md.qinv & M64) * q) >> 64
    lt = hi < mh
    if mut == "branch_inverted":
        lt = not lt
    if lt:
        return (hi + q - mh) & M64
    return csub((hi - mh) & M64, q, "never" if mut == "no_csub" else None)


# ---------------------------------------------------------------- models: h16_arith.h
def mm(a, ws, md, mut=None):
    """mm<SW>: the same product as mont_mul_sd, spelled as two asm blocks on the device"""
    return mont_mul_sd(a, ws, md, mut)


def mm31(a, us, vs, md, mut=None):
    """one Montgomery round of radix 2^31: T = (a0 u + a1 v + m q) / 2^31 = a w mod q, (u, v) = pair_of(w), balanced digits everywhere"""
    a0, a1 = digits_sd(a, mut)
    u0, u1, v0, v1 = s32(lo32(us)), s32(hi32(us)), s32(lo32(vs)), s32(hi32(vs))
    p0, p1 = md.p(31)
    C = a0 * u0 + a1 * v0
    m = lo32(lo32(C) * md.ninv32)
    m = m & 0x7fffffff if mut == "unbalanced_m" else sext(m, 31)
    X = C + m * p0
    X = (X & M64) >> 31 if mut == "logical_shift" else X >> 31
    return X + a0 * u1 + a1 * v1 + m * p1


def mm30u(a, us, vs, md, mut=None):
    """one round of radix 2^30 with an UNSIGNED low data digit: a = hi 2^32 + lo, u = w 2^30 in [0, q) with unsigned digits, v = w 2^62 balanced"""
    lo = s32(a) if mut == "lo_signed" else lo32(a)
    hi = s32(hi32(a))
    u0, u1, v0, v1 = lo32(us), hi32(us), s32(lo32(vs)), s32(hi32(vs))
    p0, p1 = md.p(30)
    C = lo * u0 + hi * v0
    m = lo32(lo32(C) * md.ninv32)
    m = m & 0x3fffffff if mut == "unbalanced_m" else sext(m, 30)
    X = C + m * p0
    X = (X & M64) >> 30 if mut == "logical_shift" else X >> 30
    return X + lo * u1 + hi * v1 + m * p1


def pred_exact(x, md, mut=None):
    """what an exact quotient would give: x - round(x / q) q.  NOT the device's value (its quotient is a float32 estimate): only a stand-in that
    the CPU tests run check_pred on, together with its mutants"""
    q = md.q
    n = (2 * x + q) // (2 * q)
    if mut == "quotient_off_by_one":
        n += 1
    if mut == "high_word_only":                    # the nt * q1 term alone: the low digit of q is forgotten
        return x - n * ((q >> 32) << 32)
    return x - n * q


# ---------------------------------------------------------------- contracts, as the comments state them (rational arithmetic, no floats)
def check_mont_mul_lazy(a, w, r, md):
    q = md.q
    if (r << 64) % q != a * w % q:
        return "not congruent"
    return None if 0 <= r < 2 * q else "outside [0, 2q)"


def check_mont_mul_sd(a, w, r, md):
    """|r| <= q/2 + q/2^33 + |a| w / 2^64 + 1 and r = a w 2^-64 mod q; w: the operand in [0, q) that the signed-split word ws stands for.
    (r 2^64 = a w + m q + m2 q 2^32 with m, m2 in [-2^31, 2^31): the first round's m contributes up to q / 2^33.  The comment used to say
    q/2 + |a| w / 2^64 + 1; these vectors showed the difference at m = m2 = -2^31.)"""
    q = md.q
    if ((r << 64) - a * w) % q:
        return "not congruent"
    return None if (abs(r) << 65) <= (q << 64) + (q << 32) + 2 * abs(a) * w + (1 << 65) else "|r| > q/2 + q/2^33 + |a| w / 2^64 + 1"


def check_mm31(a, w, r, md):
    q = md.q
    if (r - a * w) % q:
        return "not congruent"
    return None if (abs(r) << 64) <= (q << 64) + abs(a) * q else "|T| > q + |a| q / 2^64"


def check_mm30u(a, w, r, md):
    q = md.q
    if (r - a * w) % q:
        return "not congruent"
    return None if -q < r < 5 * q else "outside (-q, 5q)"


def check_pred(x, r, md):
    """r = x - n q with integer n and, as h16_arith.h states it, |r| <= q/2 + |x| 2^-22 + 2^33 for |x| < 2^62.9, |x| < 2^22 q; where that is
    below q 2^-19 (|x| + 2^55 <= 8 q) the bound |r| <= q/2 + q 2^-19 is asserted as such."""
    q = md.q
    if (x - r) % q:
        return "not congruent"
    if (abs(r) << 22) > (q << 21) + abs(x) + (1 << 55):
        return "|r| > q/2 + |x| 2^-22 + 2^33"
    if abs(x) + (1 << 55) <= 8 * q and (abs(r) << 20) > (q << 19) + 2 * q:
        return "|r| > q/2 + q 2^-19"
    return None


def check_bflyF(u, a, w, U2, V2, md):
    """U' = u + T, V' = u - T exactly, T = a w - n q with integer n, |T| <= 1.25 q (all integers; the caller has decoded the doubles)"""
    q = md.q
    T = U2 - u
    if V2 != u - T:
        return "V' != u - T"
    if (T - a * w) % q:
        return "not congruent"
    return None if 4 * abs(T) <= 5 * q else "|T| > 1.25 q"


def check_canonical(v, r, md):
    if (v - r) % md.q:
        return "not congruent"
    return None if 0 <= r < md.q else "outside [0, q)"


def double_int(bits):
    """the integer a double's bit pattern holds (None if it is not an integer)"""
    d = bits_f64(bits)
    return int(d) if d == int(d) else None


# ---------------------------------------------------------------- moduli on the class edges (they only need to be odd here)
Q_TOP = (1 << 60) - 1                              # the largest odd q below 2^60
Q_U_MAX = ((1 << 62) - 1) // 160                   # the largest q with 160 q < 2^62 ...
Q_U_MAX -= 1 - (Q_U_MAX & 1)                       # ... that is odd
Q_F_MAX = ((1 << 52) - 1) // 80
Q_F_MAX -= 1 - (Q_F_MAX & 1)                       # the largest odd q with 80 q < 2^52
Q_TINY = (1 << 20) + 1                             # for the h mod q estimate and csub only
MODULI = [Q_TOP, 0xfffffffff6a0001, (1 << 59) - 55, (1 << 57) + 0x2b0001, 0x3fffffffd60001, 0x80000000080001, Q_U_MAX, Q_U_MAX + 2,
          0x2000000a0001, 0x1fffffc20001, Q_F_MAX, Q_TINY]
MODULI_INT = [q for q in MODULI if q != Q_TINY]    # the Montgomery products, pred, redc128
MODULI_U = [q for q in MODULI_INT if 160 * q < 1 << 62]
MODULI_F = [q for q in MODULI_INT if 80 * q < 1 << 52]
assert Q_U_MAX in MODULI_U and Q_U_MAX + 2 not in MODULI_U and Q_F_MAX in MODULI_F and 160 * (Q_U_MAX + 2) > 1 << 62 and 80 * (Q_F_MAX + 2) > 1 << 52


# ---------------------------------------------------------------- edge operands
LOW_WORDS = [0, 1, 0x7fffffff, 0x80000000, 0xffffffff]


def uniq(xs):
    seen, out = set(), []
    for x in xs:
        if x not in seen:
            seen.add(x)
            out.append(x)
    return out


def signed_edges(bound, q):
    """|a| < bound: 0, +-1, every low word of LOW_WORDS under the high words {0, +-1, largest, smallest allowed}, +-(bound - 1), k q and k q +- 1 for
    small and maximal k"""
    top = (bound - 1) >> 32
    out = [0, 1, -1, bound - 1, -(bound - 1)]
    for lo in LOW_WORDS:
        for hi in (0, 1, -1, top, top - 1, -top, -top - 1):
            out.append((hi << 32) + lo)
    kmax = (bound - 1) // q
    for k in uniq([1, 2, 3, kmax - 1, kmax]):
        for d in (-1, 0, 1):
            out += [k * q + d, -(k * q + d)]
    return [a for a in uniq(out) if abs(a) < bound]


def unsigned_edges(bound, q):
    """0 <= a < bound (mont_mul_lazy: 2^63, where a1 = 2^31 - 1 is the largest high word)"""
    top = (bound - 1) >> 32
    out = [0, 1, bound - 1]
    for lo in LOW_WORDS:
        for hi in (0, 1, top, top - 1):
            out.append((hi << 32) + lo)
    kmax = (bound - 1) // q
    for k in uniq([1, 2, 3, kmax - 1, kmax]):
        out += [k * q - 1, k * q, k * q + 1]
    return [a for a in uniq(out) if 0 <= a < bound]


def twiddle_edges(q, form):
    """twiddles w in [0, q): 0, 1, q - 1, (q +- 1) / 2, and every w whose PACKED digits are extreme in `form`.  "lazy" and "sd": w is the operand
    of mont_mul_lazy / mont_mul_sd / mm itself (the Montgomery form of a plain twiddle; "sd": before sd_split), so the digits are w's own, and the
    Montgomery forms of the five plain values are included.  "31" and "30u": w is the PLAIN twiddle that pair_of packs for mm31 / mm30u, and each
    extreme one is target 2^-sh mod q for a target with the wanted digits."""
    out = [0, 1, q - 1, (q - 1) // 2, (q + 1) // 2]
    if form in ("lazy", "sd"):
        out += [(w << 64) % q for w in out]

    def back(target, sh):
        out.append(target % q * pow(pow(2, sh, q), -1, q) % q)

    if form == "lazy":
        top = (q - 1) >> 32
        for lo in LOW_WORDS + [0xfffffffe]:
            for hi in (0, top, top - 1):
                if (hi << 32) + lo < q:
                    out.append((hi << 32) + lo)
    elif form == "sd":
        top = (q - 1) >> 32
        for lo in LOW_WORDS + [0x7ffffffe, 0x80000001]:
            for hi in (0, 1, top, top - 1):
                if (hi << 32) + lo < q:
                    out.append((hi << 32) + lo)
    else:
        sh = 30 if form == "30u" else 31
        half = 1 << (sh - 1)
        # balanced targets (u and v of mm31, v of mm30u): low digit -2^(sh-1), 2^(sh-1) - 1, 0, +-1; high digit 0, +-1, largest, smallest
        d1max = (q // 2) >> sh
        bal = [(d1 << sh) + d0 for d0 in (-half, half - 1, 0, 1, -1) for d1 in (0, 1, -1, d1max, d1max - 1, -d1max, -d1max + 1)]
        bal = [t for t in bal if -(q // 2) <= t <= q // 2]
        # unsigned targets (u of mm30u): low digit 0, 1, 2^29, 2^30 - 1; high digit 0, largest
        d1top = (q - 1) >> sh
        uns = [(d1 << sh) + d0 for d0 in (0, 1, half, (1 << sh) - 1) for d1 in (0, d1top, d1top - 1)]
        uns = [t for t in uns if 0 <= t < q]
        for t in bal:
            back(t, sh + 32)                       # extreme digits in v
            if form == "31":
                back(t, sh)                        # ... and in u
        if form == "30u":
            for t in uns:
                back(t, sh)
    return uniq(out)


def pred_edges(q):
    """k q + (q +- 1) / 2 +- {0, 1, 2^40} for k across the quotient range, |x| < 2^62.9, plus the signed edge set"""
    out = list(signed_edges(B629, q))
    kmax = B629 // q
    ks = uniq([0, 1, 2, 3, 7, 8, 15, 16, 31, 32, kmax // 2, kmax - 2, kmax - 1, kmax] + [1 << j for j in range(6, 24) if (1 << j) < kmax])
    for k in ks:
        for sgn in (1, -1):
            for h in ((q - 1) // 2, (q + 1) // 2):
                for d in (0, 1, -1, 1 << 40, -(1 << 40)):
                    out.append(sgn * (k * q + h) + d)
    return [x for x in uniq(out) if abs(x) < B629]


def redc128_edges(q):
    """(hi, lo) with hi < 2q: sums of 1, 16 and 32 products (q - 1)^2, the largest hi with lo in {0, 2^64 - 1}, and small values"""
    out = []
    for k in (1, 16, 32):
        for d in (0, 1, q, -1):
            s = k * (q - 1) ** 2 + d
            out.append((s >> 64, s & M64))
    for hi in (0, 1, q - 1, q, q + 1, 2 * q - 2, 2 * q - 1):
        for lo in (0, 1, M64, 1 << 63, (1 << 63) - 1, q, M64 - q + 1):
            out.append((hi, lo))
    return [t for t in uniq(out) if t[0] < 2 * q]


def mul_edges():
    """operand words for mul64x64 / mac128: every combination of extreme 32-bit halves"""
    w = [0, 1, 0x7fffffff, 0x80000000, 0xffffffff]
    return [(h << 32) | l for h in w for l in w]


def bflyF_half_integer_pairs(q, rng, count):
    """(a, w) with a w mod q = (q +- 1) / 2, i.e. a w / q within 1 / (2q) <= 2^-20 of a half-integer: w random, a = (q +- 1)/2 w^-1 + j q, |a| < 40 q.
    rng: random.Random"""
    out = []
    while len(out) < count:
        w = rng.randrange(2, q)
        try:
            winv = pow(w, -1, q)
        except ValueError:
            continue
        for h in ((q - 1) // 2, (q + 1) // 2):
            a0 = h * winv % q
            j = rng.randrange(-40, 40)
            a = a0 + j * q
            if abs(a) < 40 * q:
                out.append((a, w))
    return out[:count]


def canon_edges(q):
    out = [0, 1, -1, (q - 1) // 2, -(q - 1) // 2, (q + 1) // 2, -(q + 1) // 2]
    for k in (1, 2, 3, 20, 38, 39):
        for d in (-1, 0, 1):
            out += [k * q + d, -(k * q + d)]
    return [v for v in uniq(out) if abs(v) < 40 * q]


def mod_by_estimate(h, q, mut=None):
    """h mod q as poly_kernels.h mod_by_estimate computes it: float64 quotient estimate (off by at most one), remainder fixed up"""
    k = int(float(h) / float(q))
    hr = (h - k * q) & M64
    if s64(hr) < 0 and mut != "no_add":
        hr = (hr + q) & M64
    if hr >= q and mut != "no_sub":
        hr -= q
    return hr


def mod_by_estimate_edges(moduli):
    """(h, q_i): h = (q_L - 1) / 2 for every ordered pair of the list, and multiples k q_i (+- 1) below 2^60, where the float64 quotient is off by one"""
    out = [((qL - 1) // 2, qi) for qL in moduli for qi in moduli if qL != qi]
    for qi in moduli:
        kmax = ((1 << 60) - 1) // qi
        for k in uniq([1, 2, kmax // 3, kmax // 2 + 1, kmax - 5, kmax - 4, kmax - 3, kmax - 2, kmax - 1, kmax]):
            for d in (-1, 0, 1):
                if 0 <= k * qi + d < 1 << 60:
                    out.append((k * qi + d, qi))
    return uniq(out)


def bflyF_exact(u, a, w, md, mut=None):
    """what an exact quotient would give (a stand-in for the CPU tests, like pred_exact): T = a w - round(a w / q) q, (u + T, u - T)"""
    q = md.q
    n = (2 * a * w + q) // (2 * q)
    if mut == "quotient_off_by_one":
        n -= 1
    T = a * w - n * q
    if mut == "v_plus":
        return u + T, u + T
    if mut == "low_part_dropped":                  # l = fma(a, w, -h) forgotten: T is off by the rounding error of the 53-bit product
        T -= (a * w) & 0xff
    return u + T, u - T


def canonF(v, md, mut=None):
    q = md.q
    n = (2 * v + q) // (2 * q)                     # rint up to ties, which no odd q has
    y = v - n * q
    if mut == "zero_to_q":
        return y + q if y <= 0 else y
    if mut == "no_add_q":
        return y & ((1 << 52) - 1)                 # d2u of a negative value: the low 52 bits of 2^52 + y
    return y + q if y < 0 else y


def u2d(v, mut=None):
    if mut == "no_subtract":
        return v | 0x4330000000000000
    if mut == "wrong_magic":
        return f64_bits(float(v) - 4503599627370496.0)
    return f64_bits(float(v))


def d2u(y, mut=None):
    if mut == "no_mask":
        return f64_bits(float(y) + 4503599627370496.0)
    if mut == "low_word_only":
        return int(y) & M32
    return int(y)


# ---------------------------------------------------------------- the registry both test modules walk
# per primitive: the moduli it is probed with, the probe's op code(s) (SW = false, SW = true), its mutants
PRIMS = {
    "mont_mul_lazy": dict(moduli=MODULI_INT, ops=(0,), muts=("round1_reuses_m", "carry_dropped")),
    "mont_mul": dict(moduli=MODULI_INT, ops=(1,), muts=("gt", "never", "carry_dropped")),
    "mont_mul_sd": dict(moduli=MODULI_INT, ops=(2,), muts=("digit_carry_dropped", "logical_shift", "unsigned_m")),
    "mont_mul_sdu": dict(moduli=MODULI_INT, ops=(3,), muts=("bias_dropped", "digit_carry_dropped")),
    "mul64x64": dict(moduli=[Q_TOP], ops=(4,), muts=("cross_carry_dropped", "signed_words")),
    "mac128": dict(moduli=[Q_TOP], ops=(5,), muts=("carry_dropped", "carry_always")),
    "redc128": dict(moduli=MODULI_INT, ops=(6,), muts=("branch_inverted", "no_csub")),
    "csub": dict(moduli=MODULI, ops=(7,), muts=("gt", "never")),
    "mm": dict(moduli=MODULI_INT, ops=(8, 9), muts=("digit_carry_dropped", "logical_shift", "unsigned_m")),
    "mm31": dict(moduli=MODULI_INT, ops=(10, 11), muts=("digit_carry_dropped", "unbalanced_m", "logical_shift")),
    "mm30u": dict(moduli=MODULI_U, ops=(12, 13), muts=("lo_signed", "unbalanced_m", "logical_shift")),
    "pred": dict(moduli=MODULI_INT, ops=(14,), muts=("quotient_off_by_one", "high_word_only")),
    "bflyF": dict(moduli=MODULI_F, ops=(15,), muts=("quotient_off_by_one", "v_plus", "low_part_dropped")),
    "u2d": dict(moduli=[Q_F_MAX], ops=(16,), muts=("no_subtract", "wrong_magic")),
    "d2u": dict(moduli=[Q_F_MAX], ops=(17,), muts=("no_mask", "low_word_only")),
    "canonF": dict(moduli=MODULI_F, ops=(18,), muts=("zero_to_q", "no_add_q")),
    "mod_by_estimate": dict(moduli=[Q_TOP], ops=(19,), muts=("no_add", "no_sub")),
}
SW_OPS = (9, 11, 13)


def blocked(as_, ws):
    """every a under every w, w-major, each w's run padded with zeros to whole BLOCKs: element i then uses the twiddle of block i // BLOCK"""
    pad = (-len(as_)) % BLOCK
    run = list(as_) + [0] * pad
    return [(a, w) for w in ws for a in run]


def edge_cases(prim, q):
    """the edge operands of one primitive and modulus, as tuples of Python integers (the LOGICAL operands: see device_inputs)"""
    if prim in ("mont_mul_lazy", "mont_mul"):
        return blocked(unsigned_edges(B63, q), twiddle_edges(q, "lazy"))
    if prim in ("mont_mul_sd", "mm"):
        return blocked(signed_edges(B62, q), twiddle_edges(q, "sd"))
    if prim == "mont_mul_sdu":
        return blocked(unsigned_edges(4 * q, q), twiddle_edges(q, "sd"))
    if prim == "mm31":
        return blocked(signed_edges(B629, q), twiddle_edges(q, "31"))
    if prim == "mm30u":
        return blocked(signed_edges(B62, q), twiddle_edges(q, "30u"))
    if prim == "mul64x64":
        return [(a, b) for a in mul_edges() for b in mul_edges()]
    if prim == "mac128":
        acc = [(0, 0), (0, M64), (M64, M64), (1, 1 << 63), (M64, 0), ((1 << 63) - 1, (1 << 63) + 1)]
        return [(a, b, h, l) for a in mul_edges()[::2] for b in mul_edges()[::3] for h, l in acc]
    if prim == "redc128":
        return redc128_edges(q)
    if prim == "csub":
        return [(a, q) for a in uniq([0, 1, q - 1, q, q + 1, 2 * q - 1, 2 * q, 2 * q + 1, M64, 1 << 63, (1 << 63) - 1]) if a <= M64]
    if prim == "pred":
        return [(x,) for x in pred_edges(q)]
    if prim == "bflyF":
        vals = canon_edges(q) + [40 * q - 1, -(40 * q - 1)]
        out = [(u, a, w) for w in (0, 1, q - 1, (q - 1) // 2, (q + 1) // 2) for a in vals for u in (0, 1, 40 * q - 1, -(40 * q - 1), (q - 1) // 2)]
        return out + [(u, a, w) for a, w in bflyF_half_integer_pairs(q, random.Random(q), 1024) for u in (0, -(40 * q - 1))]
    if prim in ("u2d", "d2u"):
        return [(v,) for v in uniq([0, 1, 2, (1 << 52) - 1, (1 << 52) - 2, 1 << 51, (1 << 51) - 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, q, 80 * q])]
    if prim == "canonF":
        return [(v,) for v in canon_edges(q)]
    if prim == "mod_by_estimate":
        return mod_by_estimate_edges(MODULI)
    raise KeyError(prim)


def random_cases(prim, q, rnd, count):
    """`count` operand tuples over the WHOLE accepted range; rnd: random.Random"""
    signed = lambda b: rnd.randrange(-b + 1, b)
    nw, na = max(1, count // BLOCK), BLOCK
    if prim in ("mont_mul_lazy", "mont_mul"):
        return blocked([rnd.randrange(B63) for _ in range(na)], [rnd.randrange(q) for _ in range(nw)])
    if prim in ("mont_mul_sd", "mm", "mm30u"):
        return blocked([signed(B62) for _ in range(na)], [rnd.randrange(q) for _ in range(nw)])
    if prim == "mont_mul_sdu":
        return blocked([rnd.randrange(4 * q) for _ in range(na)], [rnd.randrange(q) for _ in range(nw)])
    if prim == "mm31":
        return blocked([signed(B629) for _ in range(na)], [rnd.randrange(q) for _ in range(nw)])
    if prim == "mul64x64":
        return [(rnd.randrange(1 << 64), rnd.randrange(1 << 64)) for _ in range(count)]
    if prim == "mac128":
        return [tuple(rnd.randrange(1 << 64) for _ in range(4)) for _ in range(count)]
    if prim == "redc128":
        return [(rnd.randrange(2 * q), rnd.randrange(1 << 64)) for _ in range(count)]
    if prim == "csub":
        return [(rnd.randrange(2 * q), q) for _ in range(count)]
    if prim == "pred":
        return [(signed(B629),) for _ in range(count)]
    if prim == "bflyF":
        return [(signed(40 * q), signed(40 * q), rnd.randrange(q)) for _ in range(count)]
    if prim in ("u2d", "d2u"):
        return [(rnd.randrange(1 << 52),) for _ in range(count)]
    if prim == "canonF":
        return [(signed(40 * q),) for _ in range(count)]
    if prim == "mod_by_estimate":
        return [(rnd.randrange(1 << 60), rnd.choice(MODULI)) for _ in range(count)]
    raise KeyError(prim)


def device_inputs(prim, cases, md):
    """the probe's operand arrays (lists of 64-bit words, one list per operand) for a list of logical operand tuples"""
    q = md.q
    if prim in ("mont_mul_sd", "mm", "mont_mul_sdu"):
        return [[a & M64 for a, _ in cases], [sd_split(w) for _, w in cases]]
    if prim in ("mm31", "mm30u"):
        memo = {}
        for _, w in cases:
            if w not in memo:
                memo[w] = pair_of(w, q, prim == "mm30u")
        return [[a & M64 for a, _ in cases], [memo[w][0] for _, w in cases], [memo[w][1] for _, w in cases]]
    if prim == "bflyF":
        return [[f64_bits(float(u)) for u, _, _ in cases], [f64_bits(float(a)) for _, a, _ in cases], [f64_bits(float(w)) for _, _, w in cases]]
    if prim in ("d2u", "canonF"):
        return [[f64_bits(float(v)) for v, in cases]]
    return [[c[k] & M64 for c in cases] for k in range(len(cases[0]))]


def model(prim, c, md, mut=None):
    """the device's output words for one logical operand tuple (a tuple of unsigned 64-bit words), or None where the contract is the reference"""
    q = md.q
    if prim == "mont_mul_lazy":
        r = (mont_mul_lazy(c[0], c[1], md, mut),)
    elif prim == "mont_mul":
        r = (mont_mul(c[0], c[1], md, mut),)
    elif prim in ("mont_mul_sd", "mm"):
        r = (mont_mul_sd(c[0], sd_split(c[1]), md, mut),)
    elif prim == "mont_mul_sdu":
        r = (mont_mul_sdu(c[0], sd_split(c[1]), md, mut),)
    elif prim == "mm31":
        r = (mm31(c[0], *pair_of(c[1], q, False), md, mut),)
    elif prim == "mm30u":
        r = (mm30u(c[0], *pair_of(c[1], q, True), md, mut),)
    elif prim == "mul64x64":
        r = mul64x64(c[0], c[1], mut)
    elif prim == "mac128":
        r = mac128(c[0], c[1], c[2], c[3], mut)
    elif prim == "redc128":
        r = (redc128(c[0], c[1], md, mut),)
    elif prim == "csub":
        r = (csub(c[0], c[1], mut),)
    elif prim == "u2d":
        r = (u2d(c[0], mut),)
    elif prim == "d2u":
        r = (d2u(c[0], mut),)
    elif prim == "canonF":
        r = (canonF(c[0], md, mut),)
    elif prim == "mod_by_estimate":
        r = (mod_by_estimate(c[0], c[1], mut),)
    else:
        return None
    return tuple(x & M64 for x in r)


def contract(prim, c, out, md):
    """(error or None, |result| / q or None) of the device's output words `out` for the logical operands c, by the primitive's stated contract"""
    q = md.q
    if prim in ("mont_mul_lazy", "mont_mul"):
        r = out[0]
        err = check_mont_mul_lazy(c[0], c[1], r, md)
        if prim == "mont_mul" and not err and r >= q:
            err = "not canonical"
        return err, r / q
    if prim in ("mont_mul_sd", "mm"):
        r = s64(out[0])
        return check_mont_mul_sd(c[0], c[1], r, md), abs(r) / q
    if prim == "mont_mul_sdu":
        r = out[0]
        err = check_mont_mul_sd(c[0], c[1], r - q, md)
        return err or (None if 0 <= r < 2 * q else "outside [0, 2q)"), r / q
    if prim == "mm31":
        r = s64(out[0])
        return check_mm31(c[0], c[1], r, md), abs(r) / q
    if prim == "mm30u":
        r = s64(out[0])
        return check_mm30u(c[0], c[1], r, md), r / q
    if prim == "redc128":
        return check_canonical(((c[0] << 64) + c[1]) * pow(1 << 64, -1, q), out[0], md), out[0] / q
    if prim == "pred":
        r = s64(out[0])
        return check_pred(c[0], r, md), abs(r) / q
    if prim == "bflyF":
        U2, V2 = double_int(out[0]), double_int(out[1])
        if U2 is None or V2 is None:
            return "not an integer", None
        return check_bflyF(c[0], c[1], c[2], U2, V2, md), abs(U2 - c[0]) / q
    if prim == "canonF":
        return check_canonical(c[0], out[0], md), out[0] / q
    return None, None
