"""The definition of mkhe_noise_norm (include/mkhe.h, "noise measurement") in Python integers, the way the device computes it: residues ->
mixed-radix digits -> centred digits -> lexicographic maximum with ties to the smaller index.  TEST INFRASTRUCTURE: tests/test_noise_model.py pins
it against a plain CRT min(x, Q - x); the GPU tests compare the kernel with it."""


def product(qs):
    Q = 1
    for q in qs:
        Q *= int(q)
    return Q


def digits_of(x, qs):
    """the mixed-radix digits of 0 <= x < Q: x = d_0 + d_1 q_0 + d_2 q_0 q_1 + .."""
    d = []
    for q in qs:
        d.append(x % int(q))
        x //= int(q)
    return d


def value_of(d, qs):
    v, w = 0, 1
    for di, q in zip(d, qs):
        v, w = v + int(di) * w, w * int(q)
    return v


def garner(res, qs):
    """the digits of the x whose residue mod q_j is res[j] (Garner; modarith.h garner_digits without the Montgomery forms)"""
    d = []
    for j, q in enumerate(qs):
        q, t = int(q), int(res[j])
        for i in range(j):
            t = (t - d[i]) * pow(int(qs[i]), -1, q) % q
        d.append(t)
    return d


def is_negative(d, qs):
    """x > (Q - 1) / 2, decided on the digits, top digit first, against the digits of (Q - 1) / 2"""
    half = digits_of((product(qs) - 1) // 2, qs)
    return list(d)[::-1] > half[::-1]


def complement(d, qs):
    """the digits of Q - x for 0 < x < Q: q_i - 1 - d_i plus one with carry from digit 0"""
    out, carry = [], 1
    for di, q in zip(d, qs):
        t = int(q) - 1 - int(di) + carry
        carry = 1 if t == int(q) else 0
        out.append(0 if carry else t)
    return out


def centre(d, qs):
    """the digits of min(x, Q - x)"""
    return complement(d, qs) if is_negative(d, qs) else list(d)


def lex_max(cands):
    """cands: (digits, n) in any order -> the one with the lexicographically largest digits, top digit first; ties: the smallest n"""
    best = None
    for d, n in cands:
        if best is None or d[::-1] > best[0][::-1] or (d[::-1] == best[0][::-1] and n < best[1]):
            best = (list(d), n)
    return best


def residues(kind, phase, ref, qs, T=None):
    """x by its residues, [limbs][N] of Python integers: kind 0 phase - ref (ref None: phase), kind 1 T * phase"""
    out = []
    for j, q in enumerate(qs):
        q = int(q)
        if kind == 1:
            out.append([int(v) * (T % q) % q for v in phase[j]])
        elif ref is None:
            out.append([int(v) for v in phase[j]])
        else:
            out.append([(int(v) - int(w)) % q for v, w in zip(phase[j], ref[j])])
    return out


def noise_norm_digits(kind, phase, ref, qs, T=None):
    """one item: phase, ref [limbs][N] -> (digits, n) as the device writes them"""
    x = residues(kind, phase, ref, qs, T)
    N = len(x[0])
    return lex_max((centre(garner([x[j][n] for j in range(len(qs))], qs), qs), n) for n in range(N))


def noise_norm(kind, phase, ref, qs, T=None):
    """-> (r, n): the integer and the smallest index that attains it"""
    d, n = noise_norm_digits(kind, phase, ref, qs, T)
    return value_of(d, qs), n


def crt(res, qs):
    Q, x = product(qs), 0
    for r, q in zip(res, qs):
        m = Q // int(q)
        x += int(r) * m * pow(m, -1, int(q))
    return x % Q


def noise_norm_crt(kind, phase, ref, qs, T=None):
    """the same by plain integers: CRT, min(x, Q - x), the first maximum"""
    x, Q = residues(kind, phase, ref, qs, T), product(qs)
    best = (-1, -1)
    for n in range(len(x[0])):
        v = crt([x[j][n] for j in range(len(qs))], qs)
        v = min(v, Q - v)
        if v > best[0]:
            best = (v, n)
    return best


# ---- BFV: what the invariant value says about the noise
def scale_up(m, Q, T):
    """up(m) = floor((Q m + floor(T / 2)) / T), m in [0, T)"""
    return (Q * m + T // 2) // T


def bfv_noise_bound(r, T):
    """from r = |[T (up(m) + e)]_Q|: |e| <= this <= |e| + 2 as long as the noise has not wrapped"""
    return (r + T // 2) // T + 1


def noise_budget(r, Q):
    """bitlen(Q) - bitlen(r) - 1; never negative, because r <= (Q - 1) / 2"""
    return Q.bit_length() - r.bit_length() - 1
