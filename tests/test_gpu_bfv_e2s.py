"""Encryption to shares for MK-BFV on the device (-m gpu), the raw C call on the three rings of tests/test_gpu_bfv_refresh.py (N = 2^10, three
parties), bit for bit: mkhe_bfv_e2s_share's public share against mkhe_bfv_refresh_share(mask = 1), mkhe_bfv_scale_up of its secret against the
plaintext of tests/bfv_refresh_model.py (and the secret itself against (T - A) mod T); the identity w + sum_i secret_i = m (mod T) through
mkhe_decrypt_merge and mkhe_bfv_scale_down; a sentinel word behind every output buffer; every refusal followed by a call that works."""
import ctypes as C

import numpy as np
import pytest

import bfv_refresh_model as B
import test_gpu_bfv_refresh as TB
from test_gpu_bfv_refresh import BITS, KEY, NONCE_MASK, RINGS, SENTINEL, USERS, error, id_sets, key_arg, stream

pytestmark = pytest.mark.gpu

_worlds = {}


@pytest.fixture(scope="module", params=list(RINGS))
def w(request):
    if request.param not in _worlds:
        _worlds[request.param] = TB.World(RINGS[request.param])
    return _worlds[request.param]


@pytest.fixture(scope="module")
def w3():
    if "three" not in _worlds:
        _worlds["three"] = TB.World(RINGS["three"])
    return _worlds["three"]


def e2s_share(w, cts, who, bits, key=KEY, nonce=NONCE_MASK, count=None, slots=None, sk="default", out=None, sec=None, handles="default"):
    """mkhe_bfv_e2s_share into buffers of twice the size filled with a sentinel -> (rc, shares uint64 [count][nQ][N], secret uint64 [count][N]);
    a refused call leaves all of it untouched"""
    n = len(cts)
    buf = w.limbs(2 * n).upload(np.full((2 * n, w.L, w.N), SENTINEL, dtype=np.uint64))
    secret = w.mk.DeviceLimbs(w.params, 2 * n, 1).upload(np.full((2 * n, 1, w.N), SENTINEL, dtype=np.uint64))
    sl = [c.slot(who) for c in cts] if slots is None else slots
    rc = w.lib.mkhe_bfv_e2s_share(w.params.ctx, n if count is None else count, w.handles([c.h for c in cts]) if handles == "default" else handles,
                                  (C.c_int * n)(*sl), w.sk[who].Value.devptr() if sk == "default" else sk, key_arg(key), nonce, bits,
                                  buf.devptr() if out is None else out(buf), secret.devptr() if sec is None else sec(secret))
    got, s = buf.download(), secret.download()[:, 0]
    if rc == 0:
        assert (got[n:] == SENTINEL).all(), "mkhe_bfv_e2s_share wrote behind uint64[count][nQ][N]"
        assert (s[n:] == SENTINEL).all(), "mkhe_bfv_e2s_share wrote behind uint64[count][N]"
    else:
        assert (got == SENTINEL).all() and (s == SENTINEL).all(), "a refused mkhe_bfv_e2s_share wrote to its outputs"
    return rc, got[:n], s[:n]


def scale_up(w, coeffs):
    n = len(coeffs)
    src = w.mk.DeviceLimbs(w.params, n, 1).upload(np.ascontiguousarray(coeffs).reshape(n, 1, w.N))
    dst = w.limbs(n)
    assert w.lib.mkhe_bfv_scale_up(w.params.ctx, n, src.devptr(), dst.devptr()) == 0, error()
    return dst.download()


@pytest.mark.parametrize("count", [1, 3])
def test_share_is_the_share_of_the_refresh_and_up_of_the_secret_is_its_plaintext(w, count):
    who = "user1"
    sets = id_sets(who)
    cts = [w.ct(sets[b % 3])[0] for b in range(count)]          # different id sets and slots in one call
    assert count < 3 or len({c.slot(who) for c in cts}) > 1
    before = [c.download() for c in cts]
    widths = [f for f in BITS if f <= w.most] + [w.most]
    for bits in widths:
        rc, want, _ = w.share(cts, who, 1, bits)                # mkhe_bfv_refresh_share, mask = 1, the same key, nonce and width
        assert rc == 0, error()
        rc, got, secret = e2s_share(w, cts, who, bits)
        assert rc == 0, error()
        assert (got == want).all(), (bits, "share")
        A = [B.mask_poly(KEY, NONCE_MASK, b, w.N, w.T, bits, values=stream) for b in range(count)]
        assert (secret == np.array([[(w.T - a) % w.T for a in A[b]] for b in range(count)], dtype=np.uint64)).all(), (bits, "secret")
        pt = np.stack([B.reenc_plaintext(A[b], w.Q, w.T) for b in range(count)])
        assert (scale_up(w, secret) == pt).all(), (bits, "scale_up of the secret")
    assert all((c.download() == x).all() for c, x in zip(cts, before))       # the inputs are left alone


def test_seventeen_items_stage_the_pointer_tables(w3):
    w, who, count = w3, "user2", 17
    sets = id_sets(who)
    cts = [w.ct(sets[b % 3], which=b // 3 % 2)[0] for b in range(count)]
    rc, want, _ = w.share(cts, who, 1, 65)
    assert rc == 0, error()
    rc, got, secret = e2s_share(w, cts, who, 65)
    assert rc == 0, error()
    assert (got == want).all()
    up = scale_up(w, secret)
    for b in (0, 1, 16):
        A = B.mask_poly(KEY, NONCE_MASK, b, w.N, w.T, 65, values=stream)
        assert (up[b] == B.reenc_plaintext(A, w.Q, w.T)).all(), b


def test_public_share_plus_the_secret_shares_is_the_message_mod_t(w):
    """plaintexts up(m) with a small noise as c_0 + sum_i c_i s_i: built by SUBTRACTING the parties' unmasked products from up(m) + noise"""
    count = 3
    rng = np.random.default_rng(5)
    m = rng.integers(0, w.T, (count, w.N), dtype=np.uint64)
    items = [w.ct(USERS, which=b % 2) for b in range(count)]
    hosts = [h.copy() for _, h in items]
    cts0 = [c for c, _ in items]
    prod = sum(w.decrypt_share(cts0, u).astype(object) for u in USERS)      # sum_i c_i s_i per item, [count][L][N]
    up = scale_up(w, m)
    noise = rng.integers(-1000, 1001, (count, w.N))
    cts = []
    for b in range(count):
        c0 = np.stack([((up[b][j].astype(object) + noise[b].astype(object) - prod[b][j]) % int(q)).astype(np.uint64) for j, q in enumerate(w.Q)])
        hosts[b][0] = c0
        cts.append(w.bfv.Ciphertext(w.params, USERS).upload(hosts[b]))
    bits = min(65, w.bfv.NewRefresher(w.params).MaxFloodBits(3))
    shares, total = [], np.zeros((count, w.N), dtype=np.uint64)
    for i, u in enumerate(USERS):
        rc, sh, secret = e2s_share(w, cts, u, bits, nonce=NONCE_MASK + i)
        assert rc == 0, error()
        assert (secret < w.T).all()
        shares.append(sh)
        total = (total + secret) % np.uint64(w.T)
    bufs = [w.limbs(count).upload(s) for s in shares]
    pt, pub = w.limbs(count), w.mk.DeviceLimbs(w.params, count, 1)
    assert w.lib.mkhe_decrypt_merge(w.params.ctx, count, w.handles([c.h for c in cts]), 3, w.handles([x.devptr() for x in bufs]), pt.devptr()) == 0, error()
    assert w.lib.mkhe_bfv_scale_down(w.params.ctx, count, pt.devptr(), pub.devptr()) == 0, error()
    assert ((pub.download()[:, 0] + total) % np.uint64(w.T) == m).all()


def good_call(w):
    c, _ = w.ct(["user0"])
    rc, _, _ = e2s_share(w, [c], "user0", 20)
    assert rc == 0, error()


def test_refusals(w3):
    w = w3
    c3, c2 = w.ct(USERS)[0], w.ct(USERS[:2])[0]
    low = w.mk.Ciphertext(w.params, USERS, w.L - 2)

    def refused(text, cts=(c3,), who="user1", bits=50, **kw):
        rc, _, _ = e2s_share(w, list(cts), who, bits, **kw)
        assert rc != 0 and error().startswith("mkhe_bfv_e2s_share: ") and text in error() and not any("%08x" % x in error().lower() for x in KEY), error()
        good_call(w)

    refused("flood_bits", bits=-1)
    refused("flood_bits", bits=1025)
    refused("destroys the message", bits=w.most + 1)
    refused("null key", key=None)
    refused("slot out of range", slots=[0])
    refused("slot out of range", slots=[4])
    refused("slot out of range", cts=(c3, c2), slots=[3, 3])
    refused("nQ limbs", cts=(c3, low))
    refused("aligned", out=lambda buf: C.c_void_p(buf.devptr().value + 8))
    refused("aligned", sec=lambda buf: C.c_void_p(buf.devptr().value + 8))
    refused("aligned", sk=C.c_void_p(w.sk["user1"].Value.devptr().value + 8))
    refused("null", sk=None)
    refused("null", out=lambda buf: None)
    refused("null", sec=lambda buf: None)
    refused("null", handles=None)
    refused("count", count=0)
    refused("count", count=65536)
    assert w.lib.mkhe_bfv_e2s_share(None, 1, None, None, None, key_arg(), 0, 0, None, None) != 0 and error() == "mkhe_bfv_e2s_share: null context"


def test_refused_on_a_context_that_is_not_bfv():
    import test_gpu_refresh as TR
    r = TR.World()
    c, _ = r.ct(["user0"], TR.NQ - 1)
    buf = r.mk.DeviceLimbs(r.params, 1, TR.NQ).upload(np.full((1, TR.NQ, r.N), SENTINEL, dtype=np.uint64))
    sec = r.mk.DeviceLimbs(r.params, 1, 1).upload(np.full((1, 1, r.N), SENTINEL, dtype=np.uint64))
    rc = r.lib.mkhe_bfv_e2s_share(r.params.ctx, 1, r.handles([c.h]), (C.c_int * 1)(1), r.sk["user0"].Value.devptr(), key_arg(), 1, 10, buf.devptr(), sec.devptr())
    assert rc != 0 and error().startswith("mkhe_bfv_e2s_share: ") and "needs a BFV context" in error()
    assert (buf.download() == SENTINEL).all() and (sec.download() == SENTINEL).all()
    rc, sh, _ = r.refresh_share([c], "user0", 20, TR.NQ)       # the context is usable
    assert rc == 0, error()
    r.params.close()


def test_refused_inside_a_capture(w3):
    """(where the runtime of this process can capture at all: tests/test_gpu_cnn.py)"""
    from mkhe_kklss_amd._abi import MkheError
    w = w3
    c, _ = w.ct(["user0"])
    buf = w.limbs(1).upload(np.full((1, w.L, w.N), SENTINEL, dtype=np.uint64))
    sec = w.mk.DeviceLimbs(w.params, 1, 1).upload(np.full((1, 1, w.N), SENTINEL, dtype=np.uint64))
    try:
        with w.params.Capture():
            rc = w.lib.mkhe_bfv_e2s_share(w.params.ctx, 1, w.handles([c.h]), (C.c_int * 1)(1), w.sk["user0"].Value.devptr(), key_arg(), 1, 0, buf.devptr(),
                                          sec.devptr())
            msg = error()
        assert rc != 0 and msg.startswith("mkhe_bfv_e2s_share: ") and "capture" in msg
        print("capture: the call was refused inside a capture")
    except MkheError as e:
        print("capture: mkhe_capture_begin refused in this process (%s): the refusal inside a capture did not run" % e)
        import gc
        gc.enable()                 # (Graph.__enter__ switched the collector off before the refusal)
        assert "cannot end a multi-stream capture" in str(e)
    assert (buf.download() == SENTINEL).all() and (sec.download() == SENTINEL).all()
    good_call(w)
