"""mkhe_noise_norm against tests/noise_model.py (-m gpu), N = 2^10 = four workgroups of the first launch: every assertion is an equality of
integers and indices.  H.small_ckks(10, nq=4) with limbs 1, 2, 4 and count 1, 3 for kind 0 -- uniform phases with and without a reference, with
strides limbs * N and 0, and planted phases ref + e that put the maximum where the selection can go wrong -- and HB.small_bfv(10, 3), T = 65537,
for kind 1.  The refusals that need a context follow, each with its exact message and a call that works behind it.
(The digit scratch and the candidates are wiped behind the second launch; like the scratch of the share calls, they lie in the context's pool,
which no entry point reads back, so no test here looks at them.)"""
import ctypes as C

import numpy as np
import pytest

import harness as H
import harness_bfv as HB
import noise_model as M

pytestmark = pytest.mark.gpu

LOGN, N = 10, 1 << 10
PSET, BSET = H.small_ckks(LOGN, nq=4), HB.small_bfv(LOGN, 3)
T = BSET["T"]


class World:
    def __init__(self):
        from mkhe_kklss_amd import mkbfv, mkrlwe
        from mkhe_kklss_amd._abi import lib
        self.mk, self.lib = mkrlwe, lib()
        self.ckks = mkrlwe.Parameters(PSET["logN"], PSET["Q"], PSET["P"])
        self.bfv = mkbfv.Parameters(BSET["logN"], BSET["Q"], BSET["QMul"], BSET["P"], T)

    def limbs(self, params, host):
        host = np.ascontiguousarray(host, dtype=np.uint64)
        return self.mk.DeviceLimbs(params, host.shape[0], host.shape[1]).upload(host)

    def rows(self, params, kind, phase, ref=None, stride=None):
        """one call -> uint64 [count][limbs + 1] as the device wrote it; stride None: limbs * N with one reference per item, else 0"""
        count, L, _ = phase.shape
        dp, dr = self.limbs(params, phase), None if ref is None else self.limbs(params, ref)
        if stride is None:
            stride = L * N if ref is not None and ref.shape[0] == count else 0
        words = count * (L + 1)
        out = self.mk.DeviceLimbs(params, -(-words // N), 1).upload(np.full((-(-words // N), 1, N), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64))
        rc = self.lib.mkhe_noise_norm(params.ctx, kind, L, count, dp.devptr(), None if dr is None else dr.devptr(), stride, out.devptr())
        assert rc == 0, self.lib.mkhe_last_error().decode()
        flat = out.download().reshape(-1)
        assert (flat[words:] == 0xA5A5A5A5A5A5A5A5).all()                       # nothing is written behind the count * (limbs + 1) words
        return flat[:words].reshape(count, L + 1)

    def close(self):
        self.ckks.close()
        self.bfv.close()


@pytest.fixture(scope="module")
def w():
    world = World()
    yield world
    world.close()


def uniform(rng, qs, count):
    return np.stack([H.uniform_poly(rng, qs, N) for _ in range(count)])


def expect(kind, phase, ref, qs, t=None):
    """the model, item by item -> [[d_0 .. d_(L-1), n]]; ref [count] or [1] (one for all) or None"""
    out = []
    for b in range(phase.shape[0]):
        r = None if ref is None else ref[b if ref.shape[0] > 1 else 0].tolist()
        d, n = M.noise_norm_digits(kind, phase[b].tolist(), r, qs, t)
        out.append(d + [n])
    return out


@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("limbs", [1, 2, 4])
@pytest.mark.parametrize("mode", ["no reference", "one reference per item", "one reference for all"])
def test_uniform_phases(w, limbs, count, mode):
    qs, rng = PSET["Q"][:limbs], np.random.default_rng(1000 + 10 * limbs + count)
    phase = uniform(rng, qs, count)
    ref = None if mode == "no reference" else uniform(rng, qs, count if mode == "one reference per item" else 1)
    got = w.rows(w.ckks, 0, phase, ref)
    assert got.tolist() == expect(0, phase, ref, qs)
    if count == 1 and ref is not None:                                           # with one item both strides name the same reference
        assert w.rows(w.ckks, 0, phase, ref, stride=0).tolist() == got.tolist() == w.rows(w.ckks, 0, phase, ref, stride=limbs * N).tolist()


def test_the_mirror_multiplies_the_digits_out(w):
    qs, rng = PSET["Q"], np.random.default_rng(5)
    phase, ref = uniform(rng, qs, 3), uniform(rng, qs, 1)
    dec = w.mk.NewDecryptor(w.ckks)
    got = dec.NoiseNormBatch(w.limbs(w.ckks, phase), w.limbs(w.ckks, ref))
    assert got == [M.noise_norm_crt(0, phase[b].tolist(), ref[0].tolist(), qs) for b in range(3)]
    assert all(isinstance(r, int) and isinstance(n, int) for r, n in got)
    assert dec.NoiseNormBatch(w.limbs(w.ckks, phase[:1, :2]))[0] == M.noise_norm_crt(0, phase[0, :2].tolist(), None, qs[:2])


def planted(qs, rng):
    """-> [(name, {n: e_n}, (r, n) expected)]: errors that are zero except at the chosen places; workgroup k holds n = 256 k .. 256 k + 255"""
    Q, L = M.product(qs), len(qs)
    big = int(rng.integers(1, 1 << 62)) * Q // (1 << 65) + 12345                 # some value below Q / 8
    low = [int(rng.integers(0, int(q))) for q in qs[:-1]] + [int(rng.integers(1, int(qs[-1]) // 4))]
    d0a, d0b = dict(enumerate(low)), dict(enumerate(low))
    d0a[0], d0b[0] = 5, 6
    ta, tb = list(low), list(low)
    ta[-1], tb[-1] = 7, 8
    v = lambda d: M.value_of([d[i] for i in range(L)] if isinstance(d, dict) else d, qs)
    return [
        ("all zero", {}, (0, 0)),
        ("a single -1", {300: -1}, (1, 300)),
        ("(Q-1)/2 before (Q+1)/2", {100: (Q - 1) // 2, 700: (Q + 1) // 2}, ((Q - 1) // 2, 100)),
        ("(Q+1)/2 before (Q-1)/2", {100: (Q + 1) // 2, 700: (Q - 1) // 2}, ((Q - 1) // 2, 100)),
        ("the maximum at n = 0", {0: 5, 511: 4, 512: -4}, (5, 0)),
        ("the maximum at n = N - 1", {N - 1: -7, 3: 6, 768: 6}, (7, N - 1)),
        ("the same maximum in two workgroups", {900: big, 200: -big, 201: big - 1}, (big, 200)),
        ("the same maximum twice in one workgroup", {276: -big, 257: big, 20: big - 1}, (big, 257)),
        ("two workgroups, candidates differ in digit 0 only", {100: v(d0a), 600: -v(d0b)}, (v(d0b), 600)),
        ("two workgroups, candidates differ in the top digit only", {800: -v(ta), 100: v(tb), 5: v(tb) - 1 if L > 1 else 1}, (v(tb), 100)),
    ]


@pytest.mark.parametrize("limbs", [1, 2, 4])
def test_planted_phases(w, limbs):
    qs, rng = PSET["Q"][:limbs], np.random.default_rng(2000 + limbs)
    ref = uniform(rng, qs, 1)
    cases = planted(qs, rng)
    phases = []
    for name, e, want in cases:
        p = [row[:] for row in ref[0].tolist()]
        for n, v in e.items():
            for j, q in enumerate(qs):
                p[j][n] = (p[j][n] + v) % int(q)
        phase = np.array(p, dtype=np.uint64)[None]
        assert M.noise_norm_crt(0, phase[0].tolist(), ref[0].tolist(), qs) == want, name         # the case says what it means to say
        phases.append(phase)
        row = w.rows(w.ckks, 0, phase, ref)[0].tolist()
        assert row == M.digits_of(want[0], qs) + [want[1]], name
    # the same items three to a call, against one reference for all and against one per item
    for k in range(0, len(cases) - 2, 3):
        batch = np.concatenate(phases[k:k + 3])
        want = [M.digits_of(c[2][0], qs) + [c[2][1]] for c in cases[k:k + 3]]
        assert w.rows(w.ckks, 0, batch, ref).tolist() == want
        assert w.rows(w.ckks, 0, batch, np.concatenate([ref] * 3)).tolist() == want


@pytest.mark.parametrize("count", [1, 3])
def test_bfv_invariant_on_uniform_phases(w, count):
    qs, rng = BSET["Q"], np.random.default_rng(3000 + count)
    phase = uniform(rng, qs, count)
    assert w.rows(w.bfv, 1, phase).tolist() == expect(1, phase, None, qs, T)


def test_bfv_invariant_on_planted_noise(w):
    """phase = up(m) + e: the invariant value is the model's, and the bound it gives brackets max |e|"""
    from mkhe_kklss_amd import mkbfv
    qs, rng = BSET["Q"], np.random.default_rng(3100)
    Q = M.product(qs)
    m = rng.integers(0, T, (3, N))
    room = Q // (4 * T)
    e = [[int(v) for v in rng.integers(-19, 20, N)] for _ in range(3)]
    e[1][1023], e[1][0] = room // 3, -(room // 3) + 1
    e[2][255], e[2][256] = -room, room
    phase = np.array([[[(M.scale_up(int(m[b][n]), Q, T) + e[b][n]) % int(q) for n in range(N)] for q in qs] for b in range(3)], dtype=np.uint64)
    got = w.rows(w.bfv, 1, phase)
    assert got.tolist() == expect(1, phase, None, qs, T)
    res = mkbfv.NewDecryptor(w.bfv).NoiseNormBatch(w.limbs(w.bfv, phase), kind=1)
    for b in range(3):
        r, n = res[b]
        assert (r, n) == (M.value_of(got[b][:3].tolist(), qs), int(got[b][3]))
        top = max(abs(v) for v in e[b])
        assert top <= M.bfv_noise_bound(r, T) <= top + 2
        assert M.noise_budget(r, Q) >= 0
    # against the plaintext of the message the residual is e itself
    up = np.array([[[M.scale_up(int(m[b][n]), Q, T) % int(q) for n in range(N)] for q in qs] for b in range(3)], dtype=np.uint64)
    exact = w.rows(w.bfv, 0, phase, up)
    for b in range(3):
        top = max(abs(v) for v in e[b])
        assert (M.value_of(exact[b][:3].tolist(), qs), int(exact[b][3])) == (top, [abs(v) for v in e[b]].index(top))


def test_refusals_with_a_context(w):
    L = len(PSET["Q"])
    buf = w.limbs(w.ckks, np.zeros((2, L, N), dtype=np.uint64))
    out = w.mk.DeviceLimbs(w.ckks, 1, 1)
    p, o, odd = buf.devptr(), out.devptr(), C.c_void_p(buf.devptr().value + 8)
    bbuf, bout = w.limbs(w.bfv, np.zeros((1, 3, N), dtype=np.uint64)), w.mk.DeviceLimbs(w.bfv, 1, 1)

    def call(params, *args):
        rc = w.lib.mkhe_noise_norm(params.ctx, *args)
        return rc, w.lib.mkhe_last_error().decode() if rc else ""

    def works():
        assert call(w.ckks, 0, L, 2, p, None, 0, o) == (0, "") and w.lib.mkhe_ctx_sync(w.ckks.ctx) == 0
        assert out.download().reshape(-1)[:2 * (L + 1)].tolist() == [0] * (2 * (L + 1))

    name = "mkhe_noise_norm: "
    rows = [
        ((w.ckks, 0, L + 1, 1, p, None, 0, o), "limbs out of range"),
        ((w.ckks, 0, L, 1, None, None, 0, o), "null argument"),
        ((w.ckks, 0, L, 1, p, None, 0, None), "null argument"),
        ((w.ckks, 0, L, 1, odd, None, 0, o), "device buffers must be 16-byte aligned"),
        ((w.ckks, 0, L, 1, p, odd, 0, o), "device buffers must be 16-byte aligned"),
        ((w.ckks, 0, L, 1, p, None, 0, odd), "device buffers must be 16-byte aligned"),
        ((w.ckks, 0, L, 2, p, p, N, o), "ref_stride_words must be 0 (one reference for all) or limbs * N"),
        ((w.ckks, 0, 2, 2, p, p, L * N, o), "ref_stride_words must be 0 (one reference for all) or limbs * N"),
        ((w.ckks, 0, L, 2, p, p, -1, o), "ref_stride_words must be 0 (one reference for all) or limbs * N"),
        ((w.ckks, 1, L, 1, p, None, 0, o), "kind 1 (BFV invariant) needs a BFV context"),
        ((w.bfv, 1, 2, 1, bbuf.devptr(), None, 0, bout.devptr()), "kind 1 takes the nQ limbs of the context"),
    ]
    for args, message in rows:
        assert call(*args) == (1, name + message), message
        works()
    own = (C.c_int * 2)(0, 2)
    assert w.lib.mkhe_ctx_set_owned(w.ckks.ctx, own, 2) == 0
    try:
        got = call(w.ckks, 0, L, 1, p, None, 0, o)
    finally:
        assert w.lib.mkhe_ctx_set_owned(w.ckks.ctx, own, 0) == 0
    assert got == (1, name + "not available on a context that owns a subset of the moduli")
    works()
    # (where the runtime of this process can capture at all: tests/test_gpu_decrypt_share.py)
    from mkhe_kklss_amd._abi import MkheError
    try:
        with w.ckks.Capture():
            got = call(w.ckks, 0, L, 1, p, None, 0, o)
        assert got == (1, name + "not available inside mkhe_capture_begin .. mkhe_capture_end (the call allocates and uploads)")
    except MkheError as e:
        import gc
        gc.enable()                 # (Graph.__enter__ switched the collector off before the refusal)
        assert "cannot end a multi-stream capture" in str(e)
    works()
    # kind 0 serves a BFV context too
    assert call(w.bfv, 0, 3, 1, bbuf.devptr(), bbuf.devptr(), 0, bout.devptr()) == (0, "")
    assert bout.download().reshape(-1)[:4].tolist() == [0, 0, 0, 0]
