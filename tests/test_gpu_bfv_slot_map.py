"""The BFV slot map on the device (-m gpu): mkhe_bfv_slot_map against its definition mkhe_bfv_coeffs_to_slots -> numpy gather and multiply mod T ->
mkhe_bfv_slots_to_coeffs, bit for bit (integer arithmetic throughout).  N = 2^10 in the single-workgroup form and N = 2^11 with the tile lowered to
2^10 in the two-launch form, each on small_bfv(logN, 3) with T = 65537 and on its big = True ring with the largest prime T = 1 mod 2N below 2^32
(2 T does not fit 32 bits); count = 1, 3 and 17; in place and out of place; inputs of any 64 bits.  Maps: the identity, a random permutation with
random multipliers, a constant index, multipliers 0 and T - 1.  mkhe_bfv_slot_map_prepare refuses an index >= N; a map of 0xFF bytes that it did
not write is read inside the message and gives values below T (the masked read: a bounds property, no fault is provoked)."""
import ctypes as C
import types

import numpy as np
import pytest

import harness_bfv as HB
from test_gpu_refresh import is_prime

pytestmark = pytest.mark.gpu

SENTINEL = 0x7B7B7B7B7B7B7B7B
FORMS = [(10, 0), (11, 10)]                                  # (logN, tile): 0 = the granted tile, one workgroup per message; 10 = two launches each way


def big_t(logN):
    """the largest prime = 1 mod 2N below 2^32"""
    step = 1 << (logN + 1)
    t = ((1 << 32) - 2) // step * step + 1
    while not is_prime(t):
        t -= step
    return t


_worlds = {}


def world(logN, big):
    if (logN, big) not in _worlds:
        from mkhe_kklss_amd import mkbfv, mkrlwe
        from mkhe_kklss_amd._abi import lib
        pset = HB.small_bfv(logN, 3, big=big)
        T = big_t(logN) if big else pset["T"]
        params = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], T)
        _worlds[(logN, big)] = types.SimpleNamespace(params=params, N=1 << logN, T=T, lib=lib(), mk=mkrlwe, dev=mkbfv.DeviceEncoder(params))
    return _worlds[(logN, big)]


@pytest.fixture(params=[(l, t, b) for l, t in FORMS for b in (False, True)], ids=lambda p: "N%d-tile%d-%s" % (p[0], p[1], "bigT" if p[2] else "T65537"))
def w(request):
    logN, tile, big = request.param
    x = world(logN, big)
    assert x.lib.mkhe_ctx_set_bfv_tile(x.params.ctx, tile) == 0, error()
    assert (x.lib.mkhe_ctx_bfv_tile(x.params.ctx) >= logN) == (tile == 0)
    return x


def error():
    from mkhe_kklss_amd._abi import lib
    return lib().mkhe_last_error().decode()


def buf(w, host):
    """host uint64 [count][N] -> device buffer with a sentinel row behind it"""
    host = np.ascontiguousarray(host, dtype=np.uint64)
    full = np.concatenate([host, np.full((1, w.N), SENTINEL, dtype=np.uint64)])
    return w.mk.DeviceLimbs(w.params, len(full), 1).upload(full.reshape(len(full), 1, w.N))


def prepare(w, index, mult=None):
    """mkhe_bfv_slot_map_prepare -> (rc, map buffer with a sentinel row behind it)"""
    idx = np.zeros(w.N // 2, dtype=np.uint64)
    idx[:] = np.asarray(index, dtype=np.uint32).view(np.uint64)
    di = w.mk.DeviceLimbs(w.params, 1, 1).upload(np.concatenate([idx, np.zeros(w.N // 2, dtype=np.uint64)]).reshape(1, 1, w.N))
    dm = None if mult is None else buf(w, np.asarray(mult, dtype=np.uint64)[None])
    out = buf(w, np.full((1, w.N), SENTINEL, dtype=np.uint64))
    rc = w.lib.mkhe_bfv_slot_map_prepare(w.params.ctx, di.devptr(), None if dm is None else dm.devptr(), out.devptr())
    assert (out.download()[1] == SENTINEL).all(), "mkhe_bfv_slot_map_prepare wrote behind uint64[N]"
    return rc, out


def slot_map(w, coeffs, dmap, in_place):
    """mkhe_bfv_slot_map -> uint64 [count][N]; the sentinel rows behind the input and the output are checked"""
    n = len(coeffs)
    src = buf(w, coeffs)
    dst = src if in_place else buf(w, np.full((n, w.N), SENTINEL, dtype=np.uint64))
    assert w.lib.mkhe_bfv_slot_map(w.params.ctx, n, src.devptr(), dmap.devptr(), dst.devptr()) == 0, error()
    got, after = dst.download()[:, 0], src.download()[:, 0]
    assert (got[n] == SENTINEL).all() and (after[n] == SENTINEL).all(), "mkhe_bfv_slot_map wrote behind uint64[count][N]"
    if not in_place:
        assert (after[:n] == coeffs).all()                     # the input is left alone
    return got[:n]


def definition(w, coeffs, index, mult):
    """slots_to_coeffs(mult * coeffs_to_slots(coeffs)[index] mod T) through the device encoder and numpy"""
    T = np.uint64(w.T)
    z = w.dev.CoeffsToSlots(coeffs).astype(np.int64)
    z = np.mod(z, w.T).astype(np.uint64)                       # residues in [0, T)
    m = np.ones(w.N, dtype=np.uint64) if mult is None else np.asarray(mult, dtype=np.uint64) % T
    out = (z[:, index] * m) % T                                # both below 2^32: the product fits 64 bits
    return w.dev.SlotsToCoeffs(out.astype(np.int64))


def inputs(w, rng, count):
    c = rng.integers(0, 1 << 64, (count, w.N), dtype=np.uint64)                 # any 64-bit value: taken mod T
    c[0, :6] = [0, 1, w.T - 1, w.T, w.T + 1, (1 << 64) - 1]
    c[-1, w.N // 2:] = rng.integers(0, w.T, w.N // 2, dtype=np.uint64)
    return c


def maps(w, rng):
    N, T = w.N, w.T
    edge = rng.integers(0, T, N, dtype=np.uint64)
    edge[::3], edge[1::3] = 0, T - 1
    return {
        "identity": (np.arange(N), None),
        "permutation": (rng.permutation(N), rng.integers(0, 1 << 64, N, dtype=np.uint64)),       # multipliers of any 64 bits: taken mod T
        "constant": (np.zeros(N, dtype=np.int64), None),
        "edge multipliers": (rng.integers(0, N, N), edge),
    }


@pytest.mark.parametrize("count", [1, 3, 17])
def test_slot_map_is_its_definition(w, count):
    rng = np.random.default_rng(100 * w.N + count + w.T % 7)
    coeffs = inputs(w, rng, count)
    reduced = coeffs % np.uint64(w.T)
    for name, (index, mult) in maps(w, rng).items():
        rc, dmap = prepare(w, index, mult)
        assert rc == 0, error()
        want = definition(w, coeffs, index, mult)
        for in_place in (False, True):
            got = slot_map(w, coeffs, dmap, in_place)
            assert (got < w.T).all() and (got == want).all(), (name, in_place)
        if name == "identity":
            assert (want == reduced).all()                     # output = input mod T
        if name == "constant":
            z = w.dev.CoeffsToSlots(want)
            assert (z == z[:, :1]).all() and (z[:, 0] == w.dev.CoeffsToSlots(coeffs)[:, 0]).all()       # every slot equals slot 0 of the input


def test_the_two_forms_give_the_same_bits():
    """N = 2^11 at the granted tile (one workgroup) and with the tile lowered to 2^10 (five launches)"""
    for big in (False, True):
        x = world(11, big)
        rng = np.random.default_rng(11)
        coeffs = inputs(x, rng, 3)
        index, mult = rng.integers(0, x.N, x.N), rng.integers(0, x.T, x.N, dtype=np.uint64)
        assert x.lib.mkhe_ctx_set_bfv_tile(x.params.ctx, 0) == 0, error()
        rc, dmap = prepare(x, index, mult)
        assert rc == 0, error()
        one = slot_map(x, coeffs, dmap, False)
        assert x.lib.mkhe_ctx_set_bfv_tile(x.params.ctx, 10) == 0, error()
        five = slot_map(x, coeffs, dmap, False)
        assert x.lib.mkhe_ctx_set_bfv_tile(x.params.ctx, 0) == 0, error()
        assert (one == five).all() and (one == definition(x, coeffs, index, mult)).all()


def test_a_map_that_prepare_did_not_write_is_read_inside_the_message(w):
    """every word 0xFF..FF: the gathered position is (word & (N - 1)) = N - 1, inside the message, and every value written is below T"""
    rng = np.random.default_rng(3)
    coeffs = inputs(w, rng, 3)
    dmap = buf(w, np.full((1, w.N), (1 << 64) - 1, dtype=np.uint64))
    for in_place in (False, True):
        got = slot_map(w, coeffs, dmap, in_place)               # (checks the sentinels behind input and output)
        assert (got < w.T).all()


def test_refusals(w):
    N = w.N
    rc, good = prepare(w, np.arange(N))
    assert rc == 0, error()
    coeffs = np.arange(N, dtype=np.uint64)[None] % np.uint64(w.T)

    def works():
        assert (slot_map(w, coeffs, good, False) == coeffs).all()

    for bad, at in ((N, 0), (N, N - 1), (0xFFFFFFFF, 5)):
        index = np.arange(N)
        index[at] = bad
        rc, out = prepare(w, index)
        assert rc != 0 and error().startswith("mkhe_bfv_slot_map_prepare: ") and "index[%d]" % at in error(), error()
        assert (out.download() == SENTINEL).all()              # a refused call writes nothing
        works()
    a, b, m = buf(w, coeffs), buf(w, coeffs), good
    off = lambda d: C.c_void_p(d.devptr().value + 8)
    ctx, L = w.params.ctx, w.lib
    for rc, text in ((L.mkhe_bfv_slot_map(ctx, 1, None, m.devptr(), b.devptr()), "null"), (L.mkhe_bfv_slot_map(ctx, 1, a.devptr(), None, b.devptr()), "null"),
                     (L.mkhe_bfv_slot_map(ctx, 1, a.devptr(), m.devptr(), None), "null"), (L.mkhe_bfv_slot_map(ctx, 1, off(a), m.devptr(), b.devptr()), "aligned"),
                     (L.mkhe_bfv_slot_map(ctx, 1, a.devptr(), off(m), b.devptr()), "aligned"), (L.mkhe_bfv_slot_map(ctx, 1, a.devptr(), m.devptr(), off(b)), "aligned"),
                     (L.mkhe_bfv_slot_map(ctx, 0, a.devptr(), m.devptr(), b.devptr()), "count"), (L.mkhe_bfv_slot_map(ctx, 65536, a.devptr(), m.devptr(), b.devptr()), "count")):
        assert rc != 0
    # (the messages, one call at a time)
    assert L.mkhe_bfv_slot_map(ctx, 1, a.devptr(), None, b.devptr()) != 0 and error() == "mkhe_bfv_slot_map: null argument"
    assert L.mkhe_bfv_slot_map(ctx, 1, a.devptr(), off(m), b.devptr()) != 0 and error().startswith("mkhe_bfv_slot_map: ") and "aligned" in error()
    assert L.mkhe_bfv_slot_map(ctx, 0, a.devptr(), m.devptr(), b.devptr()) != 0 and error().startswith("mkhe_bfv_slot_map: ") and "count" in error()
    assert L.mkhe_bfv_slot_map_prepare(ctx, None, None, b.devptr()) != 0 and error() == "mkhe_bfv_slot_map_prepare: null argument"
    assert L.mkhe_bfv_slot_map_prepare(ctx, a.devptr(), off(a), b.devptr()) != 0 and "aligned" in error()
    assert (b.download()[:, 0] == np.concatenate([coeffs, np.full((1, N), SENTINEL, dtype=np.uint64)])).all()
    works()


def test_refused_on_a_context_that_is_not_bfv_and_inside_a_capture():
    import test_gpu_refresh as TR
    from mkhe_kklss_amd._abi import MkheError
    r = TR.World()
    d = r.mk.DeviceLimbs(r.params, 1, 1)
    assert r.lib.mkhe_bfv_slot_map(r.params.ctx, 1, d.devptr(), d.devptr(), d.devptr()) != 0 and "needs a BFV context" in error()
    assert r.lib.mkhe_bfv_slot_map_prepare(r.params.ctx, d.devptr(), None, d.devptr()) != 0 and "needs a BFV context" in error()
    r.params.close()
    x = world(10, False)
    assert x.lib.mkhe_ctx_set_bfv_tile(x.params.ctx, 0) == 0, error()
    rc, good = prepare(x, np.arange(x.N))
    assert rc == 0, error()
    coeffs = np.arange(x.N, dtype=np.uint64)[None]
    a = buf(x, coeffs)
    try:
        with x.params.Capture():
            rc1 = x.lib.mkhe_bfv_slot_map(x.params.ctx, 1, a.devptr(), good.devptr(), a.devptr())
            msg1 = error()
            rc2 = x.lib.mkhe_bfv_slot_map_prepare(x.params.ctx, a.devptr(), None, a.devptr())
            msg2 = error()
        assert rc1 != 0 and msg1.startswith("mkhe_bfv_slot_map: ") and "capture" in msg1
        assert rc2 != 0 and msg2.startswith("mkhe_bfv_slot_map_prepare: ") and "capture" in msg2
    except MkheError as e:
        print("capture: mkhe_capture_begin refused in this process (%s): the refusals inside a capture did not run" % e)
        import gc
        gc.enable()
        assert "cannot end a multi-stream capture" in str(e)
    assert (slot_map(x, coeffs, good, False) == coeffs).all()
