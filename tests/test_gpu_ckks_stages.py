"""The device CKKS encoder stage by stage (-m gpu): mkhe_ckks_scale_up / scale_down / embed / project, the two fused calls, the Python
mirror against the host encoder, and the argument validation of the six calls (include/mkhe.h, csrc/ckks_kernels.h).

Bounds.  scale_up is exact (Python integers from the same doubles).  scale_down: relative error <= 4 limbs 2^-53 against exact
rationals (the issue's bound) -- the terms are non-negative and the largest one meets 3 L roundings (its digit's conversion; per lower
limb the conversion of q_i, the multiply and the add; the + 1 of a negative value; the division), (1 + u)^(3L) - 1 < 4 L u.  embed / project: at most 4 x the error of the host encoder against a long double direct sum: both are float64 transforms of
the error class u log n; the device adds a twist stage and another radix, and the maxima of two such error sets differ by a small
factor.  Each test prints the figures it asserts on."""
import ctypes as C
import types
from fractions import Fraction

import numpy as np
import pytest

import harness as H
from scenario import Scenario

pytestmark = pytest.mark.gpu

# csrc/ckks_kernels.h: CK_TILE_LOG_BIG = 13 -- one workgroup transforms up to n = N/2 = 2^13 points in LDS, so
LOGN_SINGLE_MAX = 14        # the largest logN on the single-workgroup FFT
LOGN_MULTI_MIN = 15         # the smallest logN on the two-launch FFT

PSETS = {"q60": H.small_ckks(10, 4), "q45": H.small_alpha2(10, 5)}


def pset_for(logN):
    return H.small_alpha2(16, 5) if logN == 16 else H.small_ckks(logN, 4)       # (the primes of small_ckks are 1 mod 2^16 only)


_worlds = {}


def world(key, pset):
    """one context per parameter set for the whole module"""
    if key not in _worlds:
        from mkhe_kklss_amd import mkckks
        params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], pset["scale"])
        _worlds[key] = types.SimpleNamespace(params=params, pset=pset, N=1 << pset["logN"], dev=mkckks.DeviceEncoder(params), host=mkckks.Encoder(params))
    return _worlds[key]


def dbuf(w, count, limbs, host=None):
    from mkhe_kklss_amd import mkrlwe
    d = mkrlwe.DeviceLimbs(w.params, count, limbs)
    if host is not None:
        d.upload(np.ascontiguousarray(host).view(np.uint64).reshape(count, limbs, w.N))
    return d


def call(name, w, *args):
    from mkhe_kklss_amd._abi import lib
    return getattr(lib(), name)(w.params.ctx, *args)


def ok(rc):
    from mkhe_kklss_amd._abi import check
    check(rc)


# ------------------------------------------------------------------------------------------------ 1. scale_up
def crafted_coefficients(rng, total):
    base = [0.0, 0.5, 1.5, 2.5, 2.0 ** 52 + 0.5, 2.0 ** 62, 2.0 ** 63, 1.5 * 2.0 ** 64, 2.0 ** 200 * (1 + 2.0 ** -52)]
    v = [s * b for b in base for s in (1.0, -1.0)]
    v += list(rng.standard_normal(1001) * 2.0 ** np.arange(1001))                   # k = 0 .. 1000
    v += list(rng.standard_normal(total - len(v)) * 2.0 ** rng.integers(0, 70, total - len(v)))
    return np.array(v, dtype=np.float64)


@pytest.mark.parametrize("key", ["q60", "q45"])
@pytest.mark.parametrize("scale", [1.0, 2.0 ** 54, 12345.678])
def test_scale_up_is_bit_exact(key, scale):
    w = world(key, PSETS[key])
    count, top = 3, len(w.pset["Q"]) - 1
    c = crafted_coefficients(np.random.default_rng(5), count * w.N).reshape(count, w.N)
    with np.errstate(over="ignore"):
        x = np.float64(c) * np.float64(scale)
    finite = np.isfinite(x)             # a product beyond float64 is the caller's error (output unspecified): only scale 2^54 with |c| >= 2^970
    assert finite.all() or scale == 2.0 ** 54
    assert (~finite).sum() <= 64 and finite[:, :18].all()
    r = [[int(v) if f else 0 for v, f in zip(np.rint(xr), fr)] for xr, fr in zip(x, finite)]
    src = dbuf(w, count, 1, c)
    for level in (0, top):
        pt = dbuf(w, count, level + 1)
        ok(call("mkhe_ckks_scale_up", w, level, count, src.devptr(), C.c_double(scale), pt.devptr()))
        got = pt.download()
        for l in range(level + 1):
            q = w.pset["Q"][l]
            want = np.array([[v % q for v in row] for row in r], dtype=np.uint64)
            bad = (got[:, l] != want) & finite
            assert not bad.any(), (level, l, c[bad][:4], got[:, l][bad][:4], want[bad][:4])
    print("scale_up exact: %s scale %g, %d coefficients, %d products beyond float64 not compared" % (key, scale, finite.sum(), (~finite).sum()))


# ------------------------------------------------------------------------------------------------ 2. scale_down
def crt_basis(Q):
    Qp = 1
    for q in Q:
        Qp *= q
    return Qp, [(Qp // q) * pow(Qp // q, -1, q) for q in Q]


@pytest.mark.parametrize("key,limbs", [("q60", 1), ("q60", 2), ("q60", 4), ("q45", 1), ("q45", 2), ("q45", 4), ("q45", 5)])
def test_scale_down_meets_the_derived_bound(key, limbs):
    w = world(key, PSETS[key])
    Q = w.pset["Q"][:limbs]
    rng = np.random.default_rng(11 + limbs)
    Qp, basis = crt_basis(Q)
    half = Qp // 2                                           # (Q-1)/2
    edges = [0, 1, Qp - 1, half, half + 1]                   # the last must come out negative, the one before positive
    count, cap = 2, min(1 << 70, half)
    small = [(-1) ** i * (int(rng.integers(0, 1 << 62)) * int(rng.integers(1, 1 << 8)) % cap) for i in range(w.N - len(edges))]      # |v| < 2^70
    res = np.empty((count, limbs, w.N), dtype=np.uint64)
    for l, q in enumerate(Q):
        res[0, l] = [v % q for v in edges + small]
        res[1, l] = rng.integers(0, q, w.N, dtype=np.uint64)
    lifted = [[sum(int(r) * c for r, c in zip(res[b, :, i], basis)) % Qp for i in range(w.N)] for b in range(count)]
    assert lifted[0][:5] == edges and lifted[0][5:] == [v % Qp for v in small]
    src, worst = dbuf(w, count, limbs, res), 0.0
    for scale in (2.0 ** 54, 3.7e9):
        dst = dbuf(w, count, 1)
        ok(call("mkhe_ckks_scale_down", w, limbs, count, src.devptr(), C.c_double(scale), dst.devptr()))
        got = dst.download().view(np.float64).reshape(count, w.N)
        for b in range(count):
            for i, x in enumerate(lifted[b]):
                exact = Fraction(x - Qp if x > half else x) / Fraction(scale)
                g = float(got[b, i])
                if exact == 0:
                    assert g == 0.0
                    continue
                assert np.isfinite(g) and (g < 0) == (exact < 0), (b, i, g, float(exact))
                worst = max(worst, float(abs(Fraction(g) - exact) / abs(exact)))
        assert got[0, 3] > 0 and got[0, 4] < 0 and got[0, 2] == -1.0 / scale and got[0, 1] == 1.0 / scale
    print("scale_down %s limbs %d: relative error %.3g, bound %.3g" % (key, limbs, worst, 4 * limbs * 2.0 ** -53))
    assert worst <= 4 * limbs * 2.0 ** -53


# ------------------------------------------------------------------------------------------------ 3. embed / project
PI = 4 * np.arctan(np.longdouble(1))


def truth_project(m, logN, js):
    """z_j = sum_k m_k zeta_j^k in long double, the angle k 5^j mod 2N reduced as an integer"""
    N = 1 << logN
    k, out = np.arange(N, dtype=np.int64), []
    for j in js:
        a = (k * pow(5, int(j), 2 * N)) % (2 * N)
        ang = PI * a.astype(np.longdouble) / np.longdouble(N)
        ml = m.astype(np.longdouble)
        out.append(complex(np.sum(ml * np.cos(ang)), np.sum(ml * np.sin(ang))))
    return np.array(out)


def truth_embed(z, logN, ks):
    """m_k = (2/N) Re sum_j z_j conj(zeta_j)^k"""
    N = 1 << logN
    five = np.array([pow(5, j, 2 * N) for j in range(N // 2)], dtype=np.int64)
    zr, zi, out = z.real.astype(np.longdouble), z.imag.astype(np.longdouble), []
    for k in ks:
        ang = PI * ((five * int(k)) % (2 * N)).astype(np.longdouble) / np.longdouble(N)
        out.append(float(np.sum(zr * np.cos(ang) + zi * np.sin(ang)) * 2 / N))
    return np.array(out)


@pytest.mark.parametrize("logN,count", [(10, 1), (10, 3), (LOGN_SINGLE_MAX, 1), (LOGN_MULTI_MIN, 1), (16, 1)])
def test_embed_and_project_are_as_accurate_as_the_host_encoder(logN, count):
    assert np.finfo(np.longdouble).eps < 1e-18
    w = world("n%d" % logN, pset_for(logN))
    N, n = w.N, w.N // 2
    rng = np.random.default_rng(100 + logN + count)
    z = rng.uniform(-1, 1, (count, n)) + 1j * rng.uniform(-1, 1, (count, n))
    m = rng.uniform(-1, 1, (count, N))
    m_dev, z_dev = w.dev.Embed(z if count > 1 else z[0]).reshape(count, N), w.dev.Project(m if count > 1 else m[0]).reshape(count, n)
    e = dict(embed_dev=0.0, embed_host=0.0, project_dev=0.0, project_host=0.0)
    for b in range(count):
        ks = np.arange(N) if logN == 10 else rng.choice(N, 64, replace=False)
        js = np.arange(n) if logN == 10 else rng.choice(n, 64, replace=False)
        tm, tz = truth_embed(z[b], logN, ks), truth_project(m[b], logN, js)
        e["embed_dev"] = max(e["embed_dev"], np.abs(m_dev[b][ks] - tm).max())
        e["embed_host"] = max(e["embed_host"], np.abs(w.host.Embed(z[b])[ks] - tm).max())
        e["project_dev"] = max(e["project_dev"], np.abs(z_dev[b][js] - tz).max())
        e["project_host"] = max(e["project_host"], np.abs(w.host.Project(m[b])[js] - tz).max())
    print("logN %d count %d: embed e_host %.3g e_dev %.3g; project e_host %.3g e_dev %.3g"
          % (logN, count, e["embed_host"], e["embed_dev"], e["project_host"], e["project_dev"]))
    assert e["embed_dev"] <= 4 * e["embed_host"]
    assert e["project_dev"] <= 4 * e["project_host"]


def test_two_launch_form_of_the_smaller_transforms_gives_the_same_bits():
    """where the runtime grants the large LDS, n = 2^12 and 2^13 are single-workgroup transforms; with the limit lowered to 2^11
    (mkhe_ctx_set_ckks_tile) they take the two-launch form with 2 and 4 rows -- what a runtime without the grant runs.  Both forms do the
    same butterflies with the same twiddles in the same order per element, so the results agree bit for bit."""
    for logN in (13, 14):
        w = world("n%d" % logN, pset_for(logN))
        N, n, count = w.N, w.N // 2, 2
        tile = call("mkhe_ctx_ckks_tile", w)
        print("logN %d: single-workgroup limit 2^%d" % (logN, tile))
        assert tile in (11, 13)
        rng = np.random.default_rng(40 + logN)
        z = rng.uniform(-1, 1, (count, n)) + 1j * rng.uniform(-1, 1, (count, n))
        m = rng.uniform(-1, 1, (count, N))
        a = (w.dev.Embed(z), w.dev.Project(m))
        ok(call("mkhe_ctx_set_ckks_tile", w, 11))
        try:
            assert call("mkhe_ctx_ckks_tile", w) == 11
            b = (w.dev.Embed(z), w.dev.Project(m))
        finally:
            ok(call("mkhe_ctx_set_ckks_tile", w, 0))
        assert call("mkhe_ctx_ckks_tile", w) == tile
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[0].any() and a[1].any()
        assert np.abs(w.dev.Project(a[0]) - z).max() < 1e-9            # (and the pair is a round trip)
    assert call("mkhe_ctx_set_ckks_tile", w, 12) != 0


# ------------------------------------------------------------------------------------------------ 4. fused == staged
@pytest.mark.parametrize("logN", [10, LOGN_MULTI_MIN])
def test_fused_calls_equal_the_stage_pairs_bit_for_bit(logN):
    w = world("n%d" % logN, pset_for(logN))
    N, n, count, L = w.N, w.N // 2, 3, len(w.pset["Q"])
    rng = np.random.default_rng(7 + logN)
    z = rng.uniform(-1, 1, (count, n)) + 1j * rng.uniform(-1, 1, (count, n))
    scale = C.c_double(w.pset["scale"])
    zs = dbuf(w, count, 1, z.view(np.float64))
    coeffs, pt_staged, pt_fused = dbuf(w, count, 1), dbuf(w, count, L), dbuf(w, count, L)
    ok(call("mkhe_ckks_embed", w, count, zs.devptr(), coeffs.devptr()))
    ok(call("mkhe_ckks_scale_up", w, L - 1, count, coeffs.devptr(), scale, pt_staged.devptr()))
    ok(call("mkhe_ckks_encode", w, L - 1, count, zs.devptr(), scale, pt_fused.devptr()))
    staged = pt_staged.download()
    assert (pt_fused.download() == staged).all() and staged.any()
    src = dbuf(w, count, L, H_uniform(rng, w.pset["Q"], count, N))
    back_c, back_staged, back_fused = dbuf(w, count, 1), dbuf(w, count, 1), dbuf(w, count, 1)
    ok(call("mkhe_ckks_scale_down", w, L, count, src.devptr(), scale, back_c.devptr()))
    ok(call("mkhe_ckks_project", w, count, back_c.devptr(), back_staged.devptr()))
    ok(call("mkhe_ckks_decode", w, L, count, src.devptr(), scale, back_fused.devptr()))
    st = back_staged.download()
    assert (back_fused.download() == st).all() and st.any()
    # and the pair is a round trip: decode(encode(z)) = z up to the rounding of the coefficients
    ok(call("mkhe_ckks_decode", w, L, count, pt_fused.devptr(), scale, back_fused.devptr()))
    rt = back_fused.download().view(np.float64).reshape(count, n, 2)
    assert np.abs(rt[..., 0] + 1j * rt[..., 1] - z).max() < N / w.pset["scale"]


def H_uniform(rng, Q, count, N):
    return np.stack([H.uniform_poly(rng, Q, N) for _ in range(count)])


# ------------------------------------------------------------------------------------------------ 5. against the host encoder
def test_cross_round_trips_with_the_host_encoder():
    from mkhe_kklss_amd import mkckks
    pset = H.small_ckks(11, 4)
    w = world("n11", pset)
    n, level, scale = w.N // 2, 3, 2.0 ** 54
    bound = Scenario.precision_bound(types.SimpleNamespace(scale=scale, logN=11), 8)
    rng = np.random.default_rng(3)
    z = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)

    def log2err(a):
        d = np.abs(a - z)
        return float(np.log2(max(d.real.max(), d.imag.max(), 1e-300)))
    a = log2err(w.host.Decode(w.dev.Encode(z, level, scale).download()[0], scale))
    b = log2err(w.dev.Decode(w.host.Encode(z, level, scale), scale))
    print("host(dev) 2^%.1f, dev(host) 2^%.1f, bound 2^%.1f" % (a, b, bound))
    assert a <= bound and b <= bound
    t = mkckks.slot_permutation(11)
    assert sorted(t) == list(range(n))
    assert (4 * t + 1 == w.host.rot).all()


# ------------------------------------------------------------------------------------------------ 6. validation
def test_every_validation_case_reports_and_leaves_the_context_usable():
    from mkhe_kklss_amd import mkckks, mkrlwe
    from mkhe_kklss_amd._abi import MkheError, lib
    pset = PSETS["q60"]
    params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], pset["scale"])
    w = types.SimpleNamespace(params=params, N=1 << pset["logN"])
    L, s = len(pset["Q"]), C.c_double(pset["scale"])
    a, pt = dbuf(w, 1, 1, np.zeros(w.N)), dbuf(w, 1, L)
    A, P = a.devptr(), pt.devptr()
    off = C.c_void_p(A.value + 8)

    def refused(name, *args):
        assert call(name, w, *args) != 0, (name, args)
        msg = lib().mkhe_last_error().decode()
        assert name in msg, msg
        return msg

    def every_call(bad_what):
        """the six calls with one argument replaced by bad_what(name, good arguments)"""
        good = {"mkhe_ckks_embed": [1, A, A], "mkhe_ckks_project": [1, A, A], "mkhe_ckks_scale_up": [L - 1, 1, A, s, P],
                "mkhe_ckks_scale_down": [L, 1, P, s, A], "mkhe_ckks_encode": [L - 1, 1, A, s, P], "mkhe_ckks_decode": [L, 1, P, s, A]}
        return [refused(name, *bad_what(name, list(args))) for name, args in good.items()]

    scaled = lambda name: "scale" in name or "code" in name
    ci = lambda name: 1 if scaled(name) else 0                                  # index of count
    for k in (-1, -2):                                                           # null pointers: last and first buffer
        def null(name, g, k=k):
            g[k if k == -1 else ci(name) + 1] = None
            return g
        assert all("null" in m for m in every_call(null))
    for bad in (0, -3):
        def cnt(name, g, bad=bad):
            g[ci(name)] = bad
            return g
        assert all("count" in m for m in every_call(cnt))
    for name, ups in (("mkhe_ckks_scale_up", True), ("mkhe_ckks_encode", True), ("mkhe_ckks_scale_down", False), ("mkhe_ckks_decode", False)):
        src, dst = (A, P) if ups else (P, A)
        for lv in ((-1, L) if ups else (0, L + 1)):
            assert "out of range" in refused(name, lv, 1, src, s, dst)
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            assert "scale" in refused(name, L - 1 if ups else L, 1, src, C.c_double(bad), dst)

    def misaligned(name, g):
        g[ci(name) + 1] = off
        return g
    assert all("aligned" in m for m in every_call(misaligned))
    # a context that owns a subset of the moduli
    own = (C.c_int * 2)(0, L)
    ok(lib().mkhe_ctx_set_owned(params.ctx, own, 2))
    assert all("subset of the moduli" in m for m in every_call(lambda name, g: g))
    ok(lib().mkhe_ctx_set_owned(params.ctx, own, 0))
    # inside a capture (where the runtime of this process can capture at all: tests/test_gpu_cnn.py)
    try:
        with params.Capture():
            msgs = every_call(lambda name, g: g)
        assert all("capture" in m for m in msgs)
        print("capture: the six calls were refused inside a capture")
    except MkheError as e:
        print("capture: mkhe_capture_begin refused in this process (%s): the refusals inside a capture did not run" % e)
        import gc
        gc.enable()                 # (Graph.__enter__ switched the collector off before the refusal)
        assert "cannot end a multi-stream capture" in str(e)
    # the context still works
    enc = mkckks.DeviceEncoder(params)
    z = np.random.default_rng(1).uniform(-1, 1, w.N // 2) + 0j
    d = np.abs(enc.Decode(enc.Encode(z, L - 1, pset["scale"]), pset["scale"]) - z).max()
    assert d < w.N / pset["scale"]
    assert (mkrlwe.DeviceLimbs(params, 1, 1).upload(np.ones((1, 1, w.N), dtype=np.uint64)).download() == 1).all()
    params.close()
