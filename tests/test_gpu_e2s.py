"""Encryption to shares on the device (-m gpu), the raw C calls on the mkrlwe ring of tests/test_gpu_refresh.py (N = 2^10, the chain of three modulus
classes, three parties), bit for bit: mkhe_e2s_share's public share against mkhe_refresh_share's, its secret against (-M) mod q_j of
tests/refresh_model.py for secret_limbs below, at and above Lin; mkhe_e2s_merge against polynomial 0 of mkhe_refresh_merge with zero
re-encryptions for limbs_out below, at and above Lin; the identity (R~ + sum_i secret_i) mod q_j == mkhe_decrypt for j < Lin at every mask width;
a sentinel word behind every output buffer; every refusal followed by a call that works."""
import ctypes as C

import numpy as np
import pytest

import harness_bfv as HB
import refresh_model as R
import test_gpu_refresh as TR
from test_gpu_refresh import BITS, CHAIN, KEY, NONCE_MASK, NQ, SENTINEL, USERS, error, id_sets, key_arg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def w():
    return TR.World()


def e2s_share(w, cts, who, bits, secret_limbs, key=KEY, nonce=NONCE_MASK, count=None, slots=None, sk="default", out=None, sec=None, handles="default"):
    """mkhe_e2s_share into buffers of twice the size filled with a sentinel -> (rc, shares uint64 [count][Lin][N], secret uint64
    [count][secret_limbs][N]); a refused call leaves all of it untouched"""
    n, L, sl_alloc = len(cts), cts[0].Level() + 1, min(max(secret_limbs, 1), NQ)
    buf = w.mk.DeviceLimbs(w.params, 2 * n, L).upload(np.full((2 * n, L, w.N), SENTINEL, dtype=np.uint64))
    secret = w.mk.DeviceLimbs(w.params, 2 * n, sl_alloc).upload(np.full((2 * n, sl_alloc, w.N), SENTINEL, dtype=np.uint64))
    sl = [c.slot(who) for c in cts] if slots is None else slots
    rc = w.lib.mkhe_e2s_share(w.params.ctx, n if count is None else count, w.handles([c.h for c in cts]) if handles == "default" else handles,
                              (C.c_int * n)(*sl), w.sk[who].Value.devptr() if sk == "default" else sk, key_arg(key), nonce, bits,
                              buf.devptr() if out is None else out(buf), secret_limbs, secret.devptr() if sec is None else sec(secret))
    got, s = buf.download(), secret.download()
    if rc == 0:
        assert (got[n:] == SENTINEL).all(), "mkhe_e2s_share wrote behind uint64[count][Lin][N]"
        assert (s[n:] == SENTINEL).all(), "mkhe_e2s_share wrote behind uint64[count][secret_limbs][N]"
    else:
        assert (got == SENTINEL).all() and (s == SENTINEL).all(), "a refused mkhe_e2s_share wrote to its outputs"
    return rc, got[:n], s[:n]


def e2s_merge(w, cts, shares, limbs_out, nshares=None, count=None, handles="default", ptrs="default", out=None):
    """mkhe_e2s_merge of host share arrays [count][Lin][N] (one per party, slot order) into a sentinel-filled buffer of twice the size
    -> (rc, uint64 [count][limbs_out][N])"""
    n, L, lo = len(cts), cts[0].Level() + 1, min(max(limbs_out, 1), NQ)
    bufs = [w.mk.DeviceLimbs(w.params, n, L).upload(s) for s in shares]
    pt = w.mk.DeviceLimbs(w.params, 2 * n, lo).upload(np.full((2 * n, lo, w.N), SENTINEL, dtype=np.uint64))
    rc = w.lib.mkhe_e2s_merge(w.params.ctx, n if count is None else count, w.handles([c.h for c in cts]) if handles == "default" else handles,
                              len(bufs) if nshares is None else nshares, (w.handles([b.devptr() for b in bufs]) if bufs else None) if ptrs == "default" else ptrs(bufs),
                              limbs_out, pt.devptr() if out is None else out(pt))
    got = pt.download()
    if rc == 0:
        assert (got[n:] == SENTINEL).all(), "mkhe_e2s_merge wrote behind uint64[count][limbs_out][N]"
    else:
        assert (got == SENTINEL).all(), "a refused mkhe_e2s_merge wrote to its output"
    return rc, got[:n]


# ------------------------------------------------------------------ the share
@pytest.mark.parametrize("count", [1, 3, 17])                  # 17 > ED_INLINE: the staged pointer tables
@pytest.mark.parametrize("lin", [1, 2, 3])
def test_share_is_the_share_of_the_refresh_and_the_secret_is_minus_the_mask(w, lin, count):
    who, level = "user1", lin - 1
    sets = id_sets(who)
    cts = [w.ct(sets[b % 3], level, which=b // 3 % 2)[0] for b in range(count)]          # different id sets and slots in one call
    assert count < 3 or len({c.slot(who) for c in cts}) > 1
    before = [c.download() for c in cts]
    limbs = sorted({max(lin - 1, 1), lin, min(lin + 1, NQ), NQ})                          # below (where there is one), at and above Lin
    assert lin in limbs and (lin == 1 or min(limbs) < lin) and (lin == NQ or max(limbs) > lin)
    for bits in BITS:
        rc, want, _ = w.refresh_share(cts, who, bits, NQ)                                 # mkhe_refresh_share with the same key, nonce and width
        assert rc == 0, error()
        masks = {b: w.mask(b, bits) for b in (range(count) if count < 17 else (0, 1, 16))}    # (the model is Python integers: three items of the large batch)
        for sl in limbs:
            rc, got, secret = e2s_share(w, cts, who, bits, sl)
            assert rc == 0, error()
            assert (got == want).all(), (bits, sl, "share")
            for b, m in masks.items():
                assert (secret[b] == R.neg_mask_limbs(m, CHAIN[:sl])).all(), (bits, sl, b, "secret")
    assert all((c.download() == x).all() for c, x in zip(cts, before))                    # the inputs are left alone


def test_share_depends_on_the_nonce_and_the_key(w):
    cts = [w.ct(USERS, 1)[0]] * 2
    a, b, c, d = (e2s_share(w, cts, "user0", 100, NQ, nonce=n, key=k) for n, k in ((1, KEY), (1, KEY), (3, KEY), (1, KEY[::-1])))
    assert all(x[0] == 0 for x in (a, b, c, d)), error()
    assert (a[1] == b[1]).all() and (a[2] == b[2]).all()
    assert (a[1] != c[1]).mean() > 0.99 and (a[2] != c[2]).mean() > 0.99
    assert (a[1] != d[1]).mean() > 0.99 and (a[2] != d[2]).mean() > 0.99
    assert (a[2][0] != a[2][1]).mean() > 0.99                   # items 0 and 1 of one call
    rc, _, s = e2s_share(w, cts, "user0", 0, NQ, key=None)      # no mask: no stream is read, the key may be absent; the secret is zero
    assert rc == 0 and not s.any(), error()


# ------------------------------------------------------------------ the merge
@pytest.mark.parametrize("k", [0, 1, 3])
@pytest.mark.parametrize("lin,lout,count", [(1, NQ, 1), (2, NQ, 3), (3, NQ, 1), (1, 1, 1), (2, 2, 17), (2, 1, 1), (3, 2, 3)])
def test_merge_is_polynomial_0_of_the_refresh_merge_with_zero_reenc(w, lin, lout, count, k):
    ids = USERS[:k]
    items = [w.ct(ids, lin - 1, which=b % 2) for b in range(count)]
    cts = [c for c, _ in items]
    shares = [w.uniform((count,), lin) for _ in ids]
    rc, want = w.refresh_merge(cts, shares, [np.zeros((count, 2, lout, w.N), dtype=np.uint64)] * k, lout)
    assert rc == 0, error()
    rc, got = e2s_merge(w, cts, shares, lout)
    assert rc == 0, error()
    for b in range(count):
        assert (got[b] == want[b][0]).all(), b
    b = count - 1                                               # and the integer model on one item
    assert (got[b] == R.merge(CHAIN, lin, lout, items[b][1][0], [s[b] for s in shares], [])[0]).all()
    assert all((c.download() == h).all() for c, h in items[:2])


# ------------------------------------------------------------------ the identity
@pytest.mark.parametrize("lin", [1, 2, 3])
def test_public_share_plus_the_secret_shares_is_the_plaintext_of_decrypt(w, lin):
    """for j < Lin and ANY mask width, wrapped lift or not: the masks cancel modulo every prime"""
    count = 3
    items = [w.ct(USERS, lin - 1, which=b % 2) for b in range(count)]
    cts = [c for c, _ in items]
    plain = []
    for c in cts:
        pt = w.mk.DeviceLimbs(w.params, 1, lin)
        assert w.lib.mkhe_decrypt(w.params.ctx, c.h, w.handles([w.sk[u].Value.devptr() for u in USERS]), pt.devptr()) == 0, error()
        plain.append(pt.download()[0])
    q = w.q(lin)
    for bits in BITS:
        shares, total = [], np.zeros((count, lin, w.N), dtype=np.uint64)
        for i, u in enumerate(USERS):
            rc, sh, secret = e2s_share(w, cts, u, bits, NQ, nonce=NONCE_MASK + i)
            assert rc == 0, error()
            shares.append(sh)
            total = (total + secret[:, :lin]) % q
        rc, pub = e2s_merge(w, cts, shares, NQ)
        assert rc == 0, error()
        for b in range(count):
            assert ((pub[b][:lin] + total[b]) % q == plain[b]).all(), (bits, b)


# ------------------------------------------------------------------ refusals
def good_call(w):
    """the context works: a share and a merge of one party's ciphertext"""
    c, _ = w.ct(["user0"], 0)
    rc, sh, secret = e2s_share(w, [c], "user0", 20, NQ)
    assert rc == 0, error()
    rc, pub = e2s_merge(w, [c], [sh], NQ)
    assert rc == 0, error()


def test_e2s_share_refusals(w):
    c3, c2, low = w.ct(USERS, 1)[0], w.ct(USERS[:2], 1)[0], w.ct(USERS, 0)[0]

    def refused(text, cts=(c3,), who="user1", bits=100, sl=NQ, **kw):
        rc, _, _ = e2s_share(w, list(cts), who, bits, sl, **kw)
        assert rc != 0 and error().startswith("mkhe_e2s_share: ") and text in error() and not any("%08x" % x in error().lower() for x in KEY), error()
        good_call(w)

    refused("mask_bits", bits=-1)
    refused("mask_bits", bits=121)
    refused("null key", key=None)
    refused("slot out of range", slots=[0])
    refused("slot out of range", slots=[4])
    refused("slot out of range", cts=(c3, c2), slots=[3, 3])
    refused("same level", cts=(c3, low))
    refused("secret_limbs", sl=0)
    refused("secret_limbs", sl=NQ + 1)
    refused("aligned", out=lambda buf: C.c_void_p(buf.devptr().value + 8))
    refused("aligned", sec=lambda buf: C.c_void_p(buf.devptr().value + 8))
    refused("aligned", sk=C.c_void_p(w.sk["user1"].Value.devptr().value + 8))
    refused("null", sk=None)
    refused("null", out=lambda buf: None)
    refused("null", sec=lambda buf: None)
    refused("null", handles=None)
    refused("count", count=0)
    refused("count", count=65536)
    assert w.lib.mkhe_e2s_share(None, 1, None, None, None, None, 0, 0, None, 1, None) != 0 and error() == "mkhe_e2s_share: null context"


def test_e2s_merge_refusals(w):
    level = 1
    c3, other, low, c2 = w.ct(USERS, level)[0], w.ct(USERS, level, which=1)[0], w.ct(USERS, 0)[0], w.ct(USERS[:2], level)[0]
    one, two = np.zeros((1, level + 1, w.N), dtype=np.uint64), np.zeros((2, level + 1, w.N), dtype=np.uint64)

    def refused(text, cts=(c3,), shares=(one, one, one), lout=NQ, **kw):
        rc, _ = e2s_merge(w, list(cts), list(shares), lout, **kw)
        assert rc != 0 and error().startswith("mkhe_e2s_merge: ") and text in error(), error()
        good_call(w)

    refused("same level", cts=(c3, low), shares=(two, two, two))
    refused("same ids", cts=(c3, c2), shares=(two, two, two))
    refused("nshares", shares=(one, one))
    refused("nshares", nshares=-1)
    refused("limbs_out", lout=0)
    refused("limbs_out", lout=NQ + 1)
    refused("aligned", ptrs=lambda bufs: w.handles([bufs[0].devptr(), C.c_void_p(bufs[1].devptr().value + 8), bufs[2].devptr()]))
    refused("aligned", out=lambda pt: C.c_void_p(pt.devptr().value + 8))
    refused("null", ptrs=lambda bufs: w.handles([bufs[0].devptr(), None, bufs[2].devptr()]))
    refused("null", ptrs=lambda bufs: None)
    refused("null", out=lambda pt: None)
    refused("null", handles=None)
    refused("count", count=0)
    refused("count", count=65536)
    assert w.lib.mkhe_e2s_merge(None, 1, None, 0, None, 1, None) != 0 and error() == "mkhe_e2s_merge: null context"
    rc, _ = e2s_merge(w, [c3, other], [two, two, two], NQ)      # two ciphertexts over the same ids: accepted
    assert rc == 0, error()


def test_refused_on_a_bfv_context():
    from mkhe_kklss_amd import mkbfv, mkrlwe
    from mkhe_kklss_amd._abi import handle_array, lib
    p = HB.small_bfv(10, 3)
    params = mkbfv.Parameters(p["logN"], p["Q"], p["QMul"], p["P"], p["T"])
    params.AddCRS(0, seed=99)
    kgen = mkbfv.NewKeyGenerator(params, mkrlwe.HostSampler(np.random.default_rng(7), insecure_test_only=True))
    sk, _ = kgen.GenKeyPair("user0")
    N, L = 1 << p["logN"], len(p["Q"])
    ct = mkrlwe.Ciphertext(params, ["user0"], L - 1)
    buf = mkrlwe.DeviceLimbs(params, 1, L).upload(np.full((1, L, N), SENTINEL, dtype=np.uint64))
    sec = mkrlwe.DeviceLimbs(params, 1, L).upload(np.full((1, L, N), SENTINEL, dtype=np.uint64))
    rc = lib().mkhe_e2s_share(params.ctx, 1, handle_array([ct.h]), (C.c_int * 1)(1), sk.Value.devptr(), key_arg(), 1, 50, buf.devptr(), L, sec.devptr())
    assert rc != 0 and error().startswith("mkhe_e2s_share: ") and "BFV" in error()
    rc = lib().mkhe_e2s_merge(params.ctx, 1, handle_array([ct.h]), 1, handle_array([buf.devptr()]), L, sec.devptr())
    assert rc != 0 and error().startswith("mkhe_e2s_merge: ") and "BFV" in error()
    assert (buf.download() == SENTINEL).all() and (sec.download() == SENTINEL).all()
    sh = mkrlwe.NewDecryptor(params).ShareNew(ct, sk, 0, None)  # the context is usable
    assert not mkrlwe.NewDecryptor(params).MergeShares(ct, [sh]).download().any()
    params.close()


def test_refused_on_a_context_that_owns_a_subset_of_the_moduli(w):
    c, _ = w.ct(["user0"], 1)
    own = (C.c_int * 2)(0, 2)
    assert w.lib.mkhe_ctx_set_owned(w.params.ctx, own, 2) == 0, error()
    try:
        rc, _, _ = e2s_share(w, [c], "user0", 50, NQ)
        assert rc != 0 and error().startswith("mkhe_e2s_share: ") and "subset of the moduli" in error()
        rc, _ = e2s_merge(w, [c], [np.zeros((1, 2, w.N), dtype=np.uint64)], NQ)
        assert rc != 0 and error().startswith("mkhe_e2s_merge: ") and "subset of the moduli" in error()
    finally:
        assert w.lib.mkhe_ctx_set_owned(w.params.ctx, own, 0) == 0
    good_call(w)


def test_refused_inside_a_capture(w):
    """(where the runtime of this process can capture at all: tests/test_gpu_cnn.py)"""
    from mkhe_kklss_amd._abi import MkheError
    c, _ = w.ct(["user0"], 1)
    buf = w.mk.DeviceLimbs(w.params, 1, 2).upload(np.full((1, 2, w.N), SENTINEL, dtype=np.uint64))
    sec = w.mk.DeviceLimbs(w.params, 1, NQ).upload(np.full((1, NQ, w.N), SENTINEL, dtype=np.uint64))
    try:
        with w.params.Capture():
            rc1 = w.lib.mkhe_e2s_share(w.params.ctx, 1, w.handles([c.h]), (C.c_int * 1)(1), w.sk["user0"].Value.devptr(), key_arg(), 1, 0, buf.devptr(),
                                       NQ, sec.devptr())
            msg1 = error()
            rc2 = w.lib.mkhe_e2s_merge(w.params.ctx, 1, w.handles([c.h]), 1, w.handles([buf.devptr()]), NQ, sec.devptr())
            msg2 = error()
        assert rc1 != 0 and msg1.startswith("mkhe_e2s_share: ") and "capture" in msg1
        assert rc2 != 0 and msg2.startswith("mkhe_e2s_merge: ") and "capture" in msg2
        print("capture: both calls were refused inside a capture")
    except MkheError as e:
        print("capture: mkhe_capture_begin refused in this process (%s): the refusals inside a capture did not run" % e)
        import gc
        gc.enable()                 # (Graph.__enter__ switched the collector off before the refusal)
        assert "cannot end a multi-stream capture" in str(e)
    assert (buf.download() == SENTINEL).all() and (sec.download() == SENTINEL).all()
    good_call(w)
