"""Sparse CKKS packing on the device stage by stage (-m gpu): mkhe_ckks_embed_sparse / project_sparse / encode_sparse / decode_sparse
(include/mkhe.h, csrc/ckks_kernels.h), the Python mirror against the host encoder, and the argument validation of the four calls.

With n = 2^logSlots slots and the gap g = N / 2n the message sits on the coefficients k g, k < 2n, as the embedding m' of the ring of degree 2n,
and is exactly zero elsewhere.  Bounds.  embed / project: the device error against a long double direct sum over the ring of degree 2n is at
most max(4 x the error of the host encoder, floor), floor = 8 (logSlots + 3) 2^-53 times max|z| (embed) resp. sum_k |m_(k g)| (project): the
standard gamma_(c log n) bound of a radix-2 transform, which matters only where the host happens to be exact (n = 1, 2).  Everything else is bit for
bit.  Each test prints the figures it asserts on."""
import ctypes as C
import types

import numpy as np
import pytest

import harness as H
from scenario import Scenario
from test_gpu_ckks_stages import H_uniform, call, dbuf, ok, pset_for, truth_embed, truth_project, world

pytestmark = pytest.mark.gpu


def raw(w, a):
    """a float64 array in a device buffer of whole rows of N words"""
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    rows = -(-a.size // w.N)
    return dbuf(w, 1, rows, np.concatenate([a, np.zeros(rows * w.N - a.size)]))


def slots_of(buf, count, n):
    z = buf.download().view(np.float64).ravel()[: count * n * 2].reshape(count, n, 2)
    return z[..., 0] + 1j * z[..., 1]


def rand_slots(rng, count, n):
    return rng.uniform(-1, 1, (count, n)) + 1j * rng.uniform(-1, 1, (count, n))


def grid_mask(N, g):
    off = np.ones(N, dtype=bool)
    off[::g] = False
    return off


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and (a.view(np.uint64) == b.view(np.uint64)).all()


def coders(w, logSlots):
    from mkhe_kklss_amd import mkckks
    return mkckks.DeviceEncoder(w.params, logSlots=logSlots), mkckks.Encoder(w.params, logSlots=logSlots)


# ------------------------------------------------------------------------------------------------ 1. accuracy
# the direct sum (n < 16) and its upper edge; the tile transform with the register tail only (n = 16), with one and with two head passes; count > 1
# with messages 16 bytes apart; a large single-workgroup tile; the two-launch form
CASES = [(10, 0, 3), (10, 1, 3), (10, 3, 1), (10, 4, 3), (10, 5, 1), (10, 6, 1), (10, 8, 2), (13, 12, 1), (16, 14, 1)]


@pytest.mark.parametrize("logN,logSlots,count", CASES)
def test_embed_and_project_are_as_accurate_as_the_host_encoder(logN, logSlots, count):
    assert np.finfo(np.longdouble).eps < 1e-18
    w = world("n%d" % logN, pset_for(logN))
    dev, host = coders(w, logSlots)
    N, n = w.N, 1 << logSlots
    g = N // (2 * n)
    rng = np.random.default_rng(1000 * logN + 10 * logSlots + count)
    z, m = rand_slots(rng, count, n), rng.uniform(-1, 1, (count, N))
    m_dev = dev.Embed(z if count > 1 else z[0]).reshape(count, N)
    z_dev = dev.Project(m if count > 1 else m[0]).reshape(count, n)
    assert (m_dev[:, grid_mask(N, g)] == 0.0).all()
    e = dict(embed_dev=0.0, embed_host=0.0, project_dev=0.0, project_host=0.0, embed_floor=0.0, project_floor=0.0)
    for b in range(count):
        ks = np.arange(2 * n) if logSlots <= 9 else rng.choice(2 * n, 64, replace=False)
        js = np.arange(n) if logSlots <= 9 else rng.choice(n, 64, replace=False)
        tm, tz = truth_embed(z[b], logSlots + 1, ks), truth_project(m[b, ::g], logSlots + 1, js)
        e["embed_dev"] = max(e["embed_dev"], np.abs(m_dev[b, ::g][ks] - tm).max())
        e["embed_host"] = max(e["embed_host"], np.abs(host.Embed(z[b])[::g][ks] - tm).max())
        e["project_dev"] = max(e["project_dev"], np.abs(z_dev[b][js] - tz).max())
        e["project_host"] = max(e["project_host"], np.abs(host.Project(m[b])[js] - tz).max())
        e["embed_floor"] = max(e["embed_floor"], 8 * (logSlots + 3) * 2.0 ** -53 * np.abs(z[b]).max())
        e["project_floor"] = max(e["project_floor"], 8 * (logSlots + 3) * 2.0 ** -53 * np.abs(m[b, ::g]).sum())
    print("logN %d logSlots %d count %d: embed e_host %.3g e_dev %.3g floor %.3g; project e_host %.3g e_dev %.3g floor %.3g"
          % (logN, logSlots, count, e["embed_host"], e["embed_dev"], e["embed_floor"], e["project_host"], e["project_dev"], e["project_floor"]))
    assert e["embed_dev"] <= max(4 * e["embed_host"], e["embed_floor"])
    assert e["project_dev"] <= max(4 * e["project_host"], e["project_floor"])


@pytest.mark.parametrize("logSlots", [0, 4, 8])
def test_project_reads_the_grid_only(logSlots):
    w = world("n10", pset_for(10))
    dev, _ = coders(w, logSlots)
    g, count = w.N >> (logSlots + 1), 2
    m = np.random.default_rng(20 + logSlots).uniform(-1, 1, (count, w.N))
    off = grid_mask(w.N, g)
    zeros, nans = m.copy(), m.copy()
    zeros[:, off], nans[:, off] = 0.0, np.nan
    a, b = dev.Project(zeros), dev.Project(nans)
    assert np.isfinite(b).all() and same_bits(a, b) and a.any()
    assert same_bits(a, dev.Project(m))


# ------------------------------------------------------------------------------------------------ 2. full packing
def test_log_slots_of_full_packing_is_the_existing_calls_bit_for_bit():
    w = world("n10", pset_for(10))
    N, n, count, L, ls = w.N, w.N // 2, 2, len(w.pset["Q"]), 9
    rng = np.random.default_rng(31)
    scale = C.c_double(w.pset["scale"])
    zs, ms, pts = raw(w, rand_slots(rng, count, n).view(np.float64)), raw(w, rng.uniform(-1, 1, (count, N))), dbuf(w, count, L, H_uniform(rng, w.pset["Q"], count, N))
    pairs = [("mkhe_ckks_embed", (count, zs.devptr()), (ls, count, zs.devptr()), 1),
             ("mkhe_ckks_project", (count, ms.devptr()), (ls, count, ms.devptr()), 1),
             ("mkhe_ckks_encode", (L - 1, count, zs.devptr(), scale), (L - 1, ls, count, zs.devptr(), scale), L),
             ("mkhe_ckks_decode", (L, count, pts.devptr(), scale), (L, ls, count, pts.devptr(), scale), 1)]
    for name, args, sparse_args, limbs in pairs:
        a, b = dbuf(w, count, limbs), dbuf(w, count, limbs)
        ok(call(name, w, *args, a.devptr()))
        ok(call(name + "_sparse", w, *sparse_args, b.devptr()))
        x = a.download()
        assert (b.download() == x).all() and x.any(), name


# ------------------------------------------------------------------------------------------------ 3. fused == staged
@pytest.mark.parametrize("logSlots", [0, 4, 8])
def test_fused_calls_equal_the_stage_pairs_bit_for_bit(logSlots):
    w = world("n10", pset_for(10))
    N, n, count, L = w.N, 1 << logSlots, 3, len(w.pset["Q"])
    g = N // (2 * n)
    off = grid_mask(N, g)
    rng = np.random.default_rng(7 + logSlots)
    z = rand_slots(rng, count, n)
    scale = C.c_double(w.pset["scale"])
    zs = raw(w, z.view(np.float64))
    for limbs in (1, L):
        coeffs, pt_staged, pt_fused = dbuf(w, count, 1), dbuf(w, count, limbs), dbuf(w, count, limbs)
        pt_fused.upload(np.full((count, limbs, N), 7, dtype=np.uint64))                    # every word is written
        ok(call("mkhe_ckks_embed_sparse", w, logSlots, count, zs.devptr(), coeffs.devptr()))
        ok(call("mkhe_ckks_scale_up", w, limbs - 1, count, coeffs.devptr(), scale, pt_staged.devptr()))
        ok(call("mkhe_ckks_encode_sparse", w, limbs - 1, logSlots, count, zs.devptr(), scale, pt_fused.devptr()))
        staged, fused = pt_staged.download(), pt_fused.download()
        assert (fused == staged).all() and staged.any()
        assert not fused[:, :, off].any()
        src = dbuf(w, count, limbs, H_uniform(rng, w.pset["Q"][:limbs], count, N))        # uniform mod Q in every coefficient, off the grid too
        back_c, back_staged, back_fused = dbuf(w, count, 1), raw(w, np.zeros(2 * n * count)), raw(w, np.zeros(2 * n * count))
        ok(call("mkhe_ckks_scale_down", w, limbs, count, src.devptr(), scale, back_c.devptr()))
        ok(call("mkhe_ckks_project_sparse", w, logSlots, count, back_c.devptr(), back_staged.devptr()))
        ok(call("mkhe_ckks_decode_sparse", w, limbs, logSlots, count, src.devptr(), scale, back_fused.devptr()))
        st = slots_of(back_staged, count, n)
        assert same_bits(slots_of(back_fused, count, n), st) and st.any() and np.isfinite(st).all()
        # and the pair is a round trip: decode(encode(z)) = z up to the rounding of the coefficients
        ok(call("mkhe_ckks_decode_sparse", w, limbs, logSlots, count, pt_fused.devptr(), scale, back_fused.devptr()))
        err = np.abs(slots_of(back_fused, count, n) - z).max()
        print("logSlots %d limbs %d: |decode(encode(z)) - z| %.3g, bound %.3g" % (logSlots, limbs, err, N / w.pset["scale"]))
        assert err <= N / w.pset["scale"]


# ------------------------------------------------------------------------------------------------ 4. lowered tile
def test_two_launch_form_of_the_sparse_transforms_gives_the_same_bits():
    """as test_gpu_ckks_stages.py does for full packing: with the limit lowered to 2^11, n = 2^12 takes the two-launch form and n = 2^11 stays one
    workgroup; both forms do the same butterflies with the same twiddles in the same order per element"""
    w = world("n13", pset_for(13))
    N, count = w.N, 2
    tile = call("mkhe_ctx_ckks_tile", w)
    assert tile in (11, 13)
    for logSlots in (12, 11):
        dev, _ = coders(w, logSlots)
        n = 1 << logSlots
        rng = np.random.default_rng(40 + logSlots)
        z, m = rand_slots(rng, count, n), rng.uniform(-1, 1, (count, N))
        a = (dev.Embed(z), dev.Project(m))
        ok(call("mkhe_ctx_set_ckks_tile", w, 11))
        try:
            assert call("mkhe_ctx_ckks_tile", w) == 11
            b = (dev.Embed(z), dev.Project(m))
        finally:
            ok(call("mkhe_ctx_set_ckks_tile", w, 0))
        assert call("mkhe_ctx_ckks_tile", w) == tile
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and a[0].any() and a[1].any()
        assert np.abs(dev.Project(a[0]) - z).max() < 1e-9


# ------------------------------------------------------------------------------------------------ 5. against the host encoder
def test_cross_round_trips_with_the_host_encoder():
    from mkhe_kklss_amd._abi import MkheError
    w = world("n10", pset_for(10))
    dev, host = coders(w, 4)
    level, scale = 3, 2.0 ** 54
    bound = Scenario.precision_bound(types.SimpleNamespace(scale=scale, logN=10), 8)
    z = rand_slots(np.random.default_rng(3), 1, 16)[0]

    def log2err(a):
        d = np.abs(a - z)
        return float(np.log2(max(d.real.max(), d.imag.max(), 1e-300)))
    a = log2err(host.Decode(dev.Encode(z, level, scale).download()[0], scale))
    b = log2err(dev.Decode(host.Encode(z, level, scale), scale))
    print("host(dev) 2^%.1f, dev(host) 2^%.1f, bound 2^%.1f" % (a, b, bound))
    assert a <= bound and b <= bound
    assert dev.n == host.n == 16
    for wrong in (np.zeros(15), np.zeros(w.N // 2), np.zeros((2, 17))):
        with pytest.raises(MkheError, match="slots"):
            dev.EncodeBatch(wrong, level, scale)
    with pytest.raises(MkheError, match="slots"):
        host.Encode(np.zeros(w.N // 2), level, scale)
    with pytest.raises(MkheError, match="logSlots"):
        coders(w, 10)


# ------------------------------------------------------------------------------------------------ 6. validation
def test_every_validation_case_reports_and_leaves_the_context_usable():
    from mkhe_kklss_amd import mkckks, mkrlwe
    from mkhe_kklss_amd._abi import MkheError, lib
    pset = H.small_ckks(10, 4)
    params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], pset["scale"], logSlots=4)
    w = types.SimpleNamespace(params=params, N=1 << pset["logN"])
    L, s, ls = len(pset["Q"]), C.c_double(pset["scale"]), 4
    a, pt = dbuf(w, 1, 1, np.zeros(w.N)), dbuf(w, 1, L)
    A, P = a.devptr(), pt.devptr()
    off = C.c_void_p(A.value + 8)

    def refused(name, *args):
        assert call(name, w, *args) != 0, (name, args)
        msg = lib().mkhe_last_error().decode()
        assert name in msg, msg
        return msg

    def every_call(bad_what):
        """the four calls with one argument replaced by bad_what(name, good arguments)"""
        good = {"mkhe_ckks_embed_sparse": [ls, 1, A, A], "mkhe_ckks_project_sparse": [ls, 1, A, A],
                "mkhe_ckks_encode_sparse": [L - 1, ls, 1, A, s, P], "mkhe_ckks_decode_sparse": [L, ls, 1, P, s, A]}
        return [refused(name, *bad_what(name, list(args))) for name, args in good.items()]

    ci = lambda name: 2 if "code" in name else 1                                 # index of count; log_slots is the one before
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
    for bad in (-1, pset["logN"]):
        def slots(name, g, bad=bad):
            g[ci(name) - 1] = bad
            return g
        msgs = every_call(slots)
        assert all(m.endswith(": log_slots must be 0 .. 9") for m in msgs), msgs
    for name, ups in (("mkhe_ckks_encode_sparse", True), ("mkhe_ckks_decode_sparse", False)):
        src, dst = (A, P) if ups else (P, A)
        for lv in ((-1, L) if ups else (0, L + 1)):
            assert "out of range" in refused(name, lv, ls, 1, src, s, dst)
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            assert "scale" in refused(name, L - 1 if ups else L, ls, 1, src, C.c_double(bad), dst)

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
        print("capture: the four calls were refused inside a capture")
    except MkheError as e:
        print("capture: mkhe_capture_begin refused in this process (%s): the refusals inside a capture did not run" % e)
        import gc
        gc.enable()                 # (Graph.__enter__ switched the collector off before the refusal)
        assert "cannot end a multi-stream capture" in str(e)
    # the context still works: a sparse round trip with the encoder of the parameters' own slot count
    enc = mkckks.DeviceEncoder(params)
    assert enc.n == 16 and mkckks.NewMessage(params).Slots() == 16
    z = np.random.default_rng(1).uniform(-1, 1, 16) + 0j
    d = np.abs(enc.Decode(enc.Encode(z, L - 1, pset["scale"]), pset["scale"]) - z).max()
    assert d < w.N / pset["scale"]
    assert (mkrlwe.DeviceLimbs(params, 1, 1).upload(np.ones((1, 1, w.N), dtype=np.uint64)).download() == 1).all()
    params.close()
