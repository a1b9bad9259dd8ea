"""The collective refresh on the device (-m gpu), N = 2^10, bit for bit: mkhe_refresh_share against tests/refresh_model.py's mask added to what
mkhe_decrypt_share(flood_bits = 0) writes and against mkhe_encrypt of the model's plaintext and samples; mkhe_refresh_merge as a pure
function against the integer model (CRT, centred, reduced), on random and on crafted inputs around (Q - 1) / 2; every refusal followed by a
call that works.  The chain mixes the modulus classes: three primes = 1 mod 2^11, one below 2^31, one near 2^45, one just under 2^60, found by
search.  The end-to-end test on mkckks is tests/test_gpu_refresh_e2e.py."""
import ctypes as C

import numpy as np
import pytest

import device_sampler_model as M
import harness as H
import harness_bfv as HB
import refresh_model as R
from gpu_common import CHAIN, digits_neighbours, error, is_prime, prime_below  # noqa: F401

pytestmark = pytest.mark.gpu

KEY = [0x9E3779B9, 0x7F4A7C15, 0xF39CC060, 0x5CEDC834, 0x1082276B, 0xF3A27251, 0xF86C6A11, 0xD0C18E95]
NONCE_MASK, NONCE_ENC = 0xFEDCBA9876543210, 0x0123456789ABCDEF
SENTINEL = 0x7B7B7B7B7B7B7B7B
BITS = [0, 1, 62, 63, 64, 65, 120]
USERS = ["user0", "user1", "user2"]
LOGN = 10
NQ = len(CHAIN)


def key_arg(key=KEY):
    return None if key is None else (C.c_uint32 * 8)(*key)


_streams = {}


def stream(nonce, s, n):
    """the 64-bit values of one stream of KEY, computed once for the whole module"""
    if (nonce, s) not in _streams:
        _streams[(nonce, s)] = M.stream_values(KEY, nonce, s, n)
    return _streams[(nonce, s)]


class World:
    """a context over CHAIN, three parties with keys made on it, and the raw calls"""

    def __init__(self):
        from mkhe_kklss_amd import mkrlwe
        from mkhe_kklss_amd._abi import handle_array, lib
        assert [q % (1 << (LOGN + 1)) for q in CHAIN] == [1] * 3 and CHAIN[0] < 1 << 60 and CHAIN[1] < 1 << 45 and CHAIN[2] < 1 << 31
        self.mk, self.lib, self.handles, self.N = mkrlwe, lib(), handle_array, 1 << LOGN
        self.params = mkrlwe.Parameters(LOGN, CHAIN, H.PN15QP880["P"])
        self.params.AddCRS(0, seed=99)
        self.rng = np.random.default_rng(2027)
        kgen = mkrlwe.NewKeyGenerator(self.params, mkrlwe.HostSampler(np.random.default_rng(7), insecure_test_only=True))
        self.sk, self.pk = {}, {}
        for u in USERS:
            self.sk[u], self.pk[u] = kgen.GenKeyPair(u)
        self.cdt = mkrlwe.small_cdt(3.2)
        self._ct = {}

    def uniform(self, shape_head, limbs):
        return np.stack([self.rng.integers(0, q, tuple(shape_head) + (self.N,), dtype=np.uint64) for q in CHAIN[:limbs]], axis=len(shape_head))

    def ct(self, ids, level, which=0):
        """a uniform ciphertext over ids at level (made once per shape and number) -> (device ciphertext, host copy)"""
        k = (tuple(ids), level, which)
        if k not in self._ct:
            host = self.uniform((1 + len(ids),), level + 1)
            self._ct[k] = (self.mk.Ciphertext(self.params, list(ids), level).upload(host), host)
        return self._ct[k]

    def q(self, limbs):
        return np.array(CHAIN[:limbs], dtype=np.uint64)[:, None]

    # ---- the model's side
    def mask(self, b, bits):
        if bits == 0:
            return [0] * self.N
        return [R.wide_value(l, h, bits) for l, h in zip(stream(NONCE_MASK, 2 * b, self.N), stream(NONCE_MASK, 2 * b + 1, self.N))]

    def samples(self, count):
        """the model's u, e0, e1 of the encryption streams: int32 [count][3][N] (numpy restatement of device_sampler_model.encrypt_samples, checked
        against it on the first block)"""
        cdt, out = np.array(self.cdt, dtype=np.uint64), np.empty((count, 3, self.N), dtype=np.int32)
        for b in range(count):
            for j in range(3):
                r = np.array(stream(NONCE_ENC, 3 * b + j, self.N), dtype=np.uint64)
                out[b, j] = np.where(r & np.uint64(1), 0, np.where(r & np.uint64(2), 1, -1)) if j == 0 else np.searchsorted(cdt, r, side="right") - len(cdt) // 2
        assert out[0, :, :8].tolist() == [p[:8] for p in M.encrypt_samples(1, KEY, NONCE_ENC, 8, self.cdt)[0]]
        return out

    # ---- the raw calls
    def decrypt_share(self, cts, who):
        n, L = len(cts), cts[0].Level() + 1
        buf = self.mk.DeviceLimbs(self.params, n, L)
        assert self.lib.mkhe_decrypt_share(self.params.ctx, n, self.handles([c.h for c in cts]), (C.c_int * n)(*[c.slot(who) for c in cts]),
                                           self.sk[who].Value.devptr(), None, 0, 0, buf.devptr()) == 0, error()
        return buf.download()

    def encrypt(self, who, pt, samples):
        """mkhe_encrypt of host plaintexts [count][L][N] on host samples -> uint64 [count][2][L][N]"""
        n, L = pt.shape[0], pt.shape[1]
        d = self.mk.DeviceLimbs(self.params, n, L).upload(pt)
        outs = self.mk.batch_ciphertexts(self.mk.Ciphertext, self.params, [who], L - 1, n)
        smp = np.ascontiguousarray(samples, dtype=np.int32)
        assert self.lib.mkhe_encrypt(self.params.ctx, L - 1, n, self.pk[who].Value.devptr(), d.devptr(), 0, smp.ctypes.data_as(C.POINTER(C.c_int32)),
                                     self.handles([c.h for c in outs])) == 0, error()
        return np.stack([c.download() for c in outs])

    def refresh_share(self, cts, who, bits, lout, key=KEY, nonce_mask=NONCE_MASK, nonce_enc=NONCE_ENC, count=None, slots=None, sk="default",
                      pk="default", out=None, handles="default", reenc="default", cdt="default", ncdt=None):
        """mkhe_refresh_share into a share buffer of twice the size filled with a sentinel and sentinel-filled outputs
        -> (rc, shares uint64 [count][Lin][N], reenc uint64 [count][2][lout][N]); a refused call leaves all of it untouched"""
        n, L = len(cts), cts[0].Level() + 1
        buf = self.mk.DeviceLimbs(self.params, 2 * n, L).upload(np.full((2 * n, L, self.N), SENTINEL, dtype=np.uint64))
        sl = [c.slot(who) for c in cts] if slots is None else slots
        outs = [self.mk.Ciphertext(self.params, [c.ids[min(max(s, 1), len(c.ids)) - 1]], lout - 1).upload(np.full((2, lout, self.N), SENTINEL, dtype=np.uint64))
                for c, s in zip(cts, sl)]
        table = (C.c_uint64 * len(self.cdt))(*self.cdt) if cdt == "default" else cdt
        rc = self.lib.mkhe_refresh_share(self.params.ctx, n if count is None else count, self.handles([c.h for c in cts]) if handles == "default" else handles,
                                         (C.c_int * n)(*sl), self.sk[who].Value.devptr() if sk == "default" else sk,
                                         self.pk[who].Value.devptr() if pk == "default" else pk, key_arg(key), nonce_mask, nonce_enc, bits,
                                         table, len(self.cdt) if ncdt is None else ncdt, buf.devptr() if out is None else out(buf),
                                         self.handles([c.h for c in outs]) if reenc == "default" else reenc(outs))
        got, enc = buf.download(), np.stack([c.download() for c in outs])
        if rc == 0:
            assert (got[n:] == SENTINEL).all(), "mkhe_refresh_share wrote behind uint64[count][limbs][N]"
        else:
            assert (got == SENTINEL).all() and (enc == SENTINEL).all(), "a refused mkhe_refresh_share wrote to its outputs"
        return rc, got[:n], enc

    def refresh_merge(self, cts, shares, reenc, lout, nshares=None, count=None, handles="default", ptrs="default", re_ids=None, re_limbs=None,
                      re_list="default", outs=None):
        """mkhe_refresh_merge of host share arrays [count][Lin][N] and host re-encryptions [count][2][lout][N] (one of each per party, slot order)
        -> (rc, uint64 [count][1 + k][lout][N])"""
        n, L, ids = len(cts), cts[0].Level() + 1, cts[0].ids
        bufs = [self.mk.DeviceLimbs(self.params, n, L).upload(s) for s in shares]
        res = []
        for i, r in enumerate(reenc):
            for b in range(n):
                rid, rl = (ids[i] if re_ids is None else re_ids[i]), (lout if re_limbs is None else re_limbs)
                c = self.mk.Ciphertext(self.params, [rid], rl - 1)
                res.append(c.upload(r[b] if rl == lout else np.zeros((2, rl, self.N), dtype=np.uint64)))
        if outs is None:
            outs = [self.mk.Ciphertext(self.params, ids, lout - 1).upload(np.full((1 + len(ids), lout, self.N), SENTINEL, dtype=np.uint64)) for _ in range(n)]
        rc = self.lib.mkhe_refresh_merge(self.params.ctx, n if count is None else count, self.handles([c.h for c in cts]) if handles == "default" else handles,
                                         len(bufs) if nshares is None else nshares, self.handles([b.devptr() for b in bufs]) if ptrs == "default" else ptrs(bufs),
                                         (self.handles([c.h for c in res]) if res else None) if re_list == "default" else re_list(res),
                                         self.handles([c.h for c in outs]))
        return rc, [c.download() for c in outs]


@pytest.fixture(scope="module")
def w():
    return World()


def id_sets(who):
    """ciphertexts over 1, 2 and 3 parties that `who` belongs to (test_gpu_decrypt_share.py): its slot differs between them"""
    pair = ["user0", "user1"] if who != "user2" else ["user1", "user2"]
    return [[who], pair, USERS]


# ------------------------------------------------------------------ the share
@pytest.mark.parametrize("count", [1, 3, 17])                  # 17 > ED_INLINE: the staged pointer tables
@pytest.mark.parametrize("top", [False, True])                 # Lout = Lin, Lout = nQ
@pytest.mark.parametrize("lin", [1, 2, 3])
def test_share_is_the_unmasked_share_plus_the_mask_and_reenc_is_encrypt_of_minus_the_mask(w, lin, top, count):
    who, lout, level = "user1", NQ if top else lin, lin - 1
    sets = id_sets(who)
    cts = [w.ct(sets[b % 3], level, which=b // 3 % 2)[0] for b in range(count)]          # different id sets and slots in one call
    assert count < 3 or len({c.slot(who) for c in cts}) > 1
    before = [c.download() for c in cts]
    plain = w.decrypt_share(cts, who)                           # mkhe_decrypt_share, flood_bits = 0
    smp = w.samples(count)
    for bits in BITS:
        rc, got, enc = w.refresh_share(cts, who, bits, lout)
        assert rc == 0, error()
        masks = [w.mask(b, bits) for b in range(count)]
        want = np.stack([(plain[b] + R.mask_limbs(masks[b], CHAIN[:lin])) % w.q(lin) for b in range(count)])
        assert (got == want).all(), (bits, "share")
        pt = np.stack([R.neg_mask_limbs(masks[b], CHAIN[:lout]) for b in range(count)])
        assert (enc == w.encrypt(who, pt, smp)).all(), (bits, "reenc")       # mkhe_encrypt on the model's plaintext and samples
        if bits:
            assert all(-(1 << (bits - 1)) <= v < (1 << (bits - 1)) for v in masks[0]) and len(set(masks[0])) > (1 if bits > 1 else 0)
    assert all((c.download() == x).all() for c, x in zip(cts, before))       # the inputs are left alone


def test_share_depends_on_both_nonces_and_the_key(w):
    cts = [w.ct(USERS, 1)[0]] * 2
    a, b, c, d, e = (w.refresh_share(cts, "user0", 100, NQ, nonce_mask=nm, nonce_enc=ne, key=k)
                     for nm, ne, k in ((1, 2, KEY), (1, 2, KEY), (3, 2, KEY), (1, 4, KEY), (1, 2, KEY[::-1])))
    assert all(x[0] == 0 for x in (a, b, c, d, e)), error()
    assert (a[1] == b[1]).all() and (a[2] == b[2]).all()       # the same key and nonces: the same outputs
    assert (a[1] != c[1]).mean() > 0.99 and (a[2][:, 0] != c[2][:, 0]).mean() > 0.99     # another mask: share and c0 move, c1 (u * pk1 + e1) stays
    assert (a[2][:, 1] == c[2][:, 1]).all()
    assert (a[1] == d[1]).all() and (a[2] != d[2]).mean() > 0.99              # another encryption nonce: the share stays
    assert (a[1] != e[1]).mean() > 0.99 and (a[2] != e[2]).mean() > 0.99
    assert (a[1][0] != a[1][1]).mean() > 0.99                  # items 0 and 1 of one call


# ------------------------------------------------------------------ the merge as a pure function
@pytest.mark.parametrize("k", [0, 1, 3])
@pytest.mark.parametrize("lin,lout,count", [(1, NQ, 1), (2, NQ, 3), (3, NQ, 1), (1, 1, 1), (2, 2, 17), (2, 1, 1)])
def test_merge_is_the_integer_model(w, lin, lout, count, k):
    ids = USERS[:k]
    items = [w.ct(ids, lin - 1, which=b % 2) for b in range(count)]
    cts = [c for c, _ in items]
    shares = [w.uniform((count,), lin) for _ in ids]
    reenc = [w.uniform((count, 2), lout) for _ in ids]
    rc, got = w.refresh_merge(cts, shares, reenc, lout)
    assert rc == 0, error()
    for b in range(count if count < 17 else 3):                 # (the model is Python integers: three items of the large batch, the last among them)
        b = b if b < 2 else count - 1
        want = R.merge(CHAIN, lin, lout, items[b][1][0], [s[b] for s in shares], [r[b] for r in reenc])
        assert (got[b] == want).all(), b
    assert all((c.download() == h).all() for c, h in items[:2])


@pytest.mark.parametrize("k", [0, 1, 3])
@pytest.mark.parametrize("lin", [1, 2, 3])
def test_merge_lifts_exactly_around_half_q(w, lin, k):
    """all shares and re-encryptions zero, c_0 = the residues of crafted x: polynomial 0 of the output is the centred x under every modulus"""
    ids, lout = USERS[:k], NQ
    xs, Q = digits_neighbours(lin)
    host = w.uniform((1 + k,), lin)
    for j, q in enumerate(CHAIN[:lin]):
        host[0, j, : len(xs)] = [x % q for x in xs]
    ct = w.mk.Ciphertext(w.params, ids, lin - 1).upload(host)
    zero_s, zero_r = np.zeros((1, lin, w.N), dtype=np.uint64), np.zeros((1, 2, lout, w.N), dtype=np.uint64)
    rc, got = w.refresh_merge([ct], [zero_s] * k, [zero_r] * k, lout)
    assert rc == 0, error()
    for i, x in enumerate(xs):
        lifted = x if x <= (Q - 1) // 2 else x - Q
        assert [int(got[0][0, j, i]) for j in range(lout)] == [lifted % q for q in CHAIN[:lout]], (i, x)
    assert (got[0] == R.merge(CHAIN, lin, lout, host[0], [zero_s[0]] * k, [zero_r[0]] * k)).all()
    assert not got[0][1:].any()                                 # polynomial 1 of the zero re-encryptions


@pytest.mark.parametrize("k", [0, 1, 3])
@pytest.mark.parametrize("lin", [1, 2, 3])
def test_merge_with_zero_reenc_at_the_input_level_is_decrypt_merge(w, lin, k):
    ids = USERS[:k]
    items = [w.ct(ids, lin - 1, which=b) for b in range(2)]
    cts = [c for c, _ in items]
    shares = [w.uniform((2,), lin) for _ in ids]
    rc, got = w.refresh_merge(cts, shares, [np.zeros((2, 2, lin, w.N), dtype=np.uint64)] * k, lin)
    assert rc == 0, error()
    bufs = [w.mk.DeviceLimbs(w.params, 2, lin).upload(s) for s in shares]
    pt = w.mk.DeviceLimbs(w.params, 2, lin)
    assert w.lib.mkhe_decrypt_merge(w.params.ctx, 2, w.handles([c.h for c in cts]), k, w.handles([b.devptr() for b in bufs]), pt.devptr()) == 0, error()
    want = pt.download()
    for b in range(2):
        assert (got[b][0] == want[b]).all() and not got[b][1:].any()


# ------------------------------------------------------------------ refusals
def good_call(w):
    """the context works: a share and a merge of one party's ciphertext, whose result is over the same id at the top level"""
    c, _ = w.ct(["user0"], 0)
    rc, sh, enc = w.refresh_share([c], "user0", 20, NQ)
    assert rc == 0, error()
    rc, got = w.refresh_merge([c], [sh], [enc], NQ)
    assert rc == 0 and (got[0][1] == enc[0][1]).all(), error()


def test_refresh_share_refusals(w):
    level = 1
    c3, c2, low = w.ct(USERS, level)[0], w.ct(USERS[:2], level)[0], w.ct(USERS, 0)[0]
    solo = w.ct(["user1"], NQ - 1)[0]

    def refused(text, cts=(c3,), who="user1", bits=100, lout=NQ, **kw):
        rc, _, _ = w.refresh_share(list(cts), who, bits, lout, **kw)
        assert rc != 0 and error().startswith("mkhe_refresh_share: ") and text in error() and not any("%08x" % x in error().lower() for x in KEY), error()
        good_call(w)

    refused("mask_bits", bits=-1)
    refused("mask_bits", bits=121)
    refused("null key", key=None)
    refused("nonce_mask and nonce_enc must differ", nonce_mask=5, nonce_enc=5)
    refused("slot out of range", slots=[0])
    refused("slot out of range", slots=[4])
    refused("slot out of range", cts=(c3, c2), slots=[3, 3])
    refused("same level", cts=(c3, low))
    refused("aligned", out=lambda buf: C.c_void_p(buf.devptr().value + 8))
    refused("aligned", sk=C.c_void_p(w.sk["user1"].Value.devptr().value + 8))
    refused("aligned", pk=C.c_void_p(w.pk["user1"].Value.devptr().value + 8))
    refused("null", sk=None)
    refused("null", pk=None)
    refused("null", out=lambda buf: None)
    refused("null", handles=None)
    refused("null", reenc=lambda outs: None)
    refused("null table", cdt=None)
    refused("ncdt", ncdt=3)
    refused("count", count=0)
    refused("count", count=65536)
    pair, wrong, short = (w.mk.Ciphertext(w.params, ids, lvl) for ids, lvl in ((USERS[:2], NQ - 1), (["user0"], NQ - 1), (["user1"], 0)))
    refused("exactly the id", reenc=lambda outs: w.handles([pair.h]))
    refused("exactly the id", reenc=lambda outs: w.handles([wrong.h]))
    refused("same number of limbs", cts=(c3, c3), reenc=lambda outs: w.handles([outs[0].h, short.h]))
    assert not pair.download().any() and not wrong.download().any() and not short.download().any()
    refused("distinct", cts=(c3, c3), reenc=lambda outs: w.handles([outs[0].h, outs[0].h]))
    refused("aliases an input", cts=(solo,), reenc=lambda outs: w.handles([solo.h]))
    assert w.lib.mkhe_refresh_share(None, 1, None, None, None, None, None, 0, 1, 0, None, 0, None, None) != 0
    rc, _, _ = w.refresh_share([c3], "user1", 0, NQ, nonce_mask=5, nonce_enc=5)          # no mask stream: the nonces may coincide
    assert rc == 0, error()


def test_refresh_merge_refusals(w):
    level, lout = 1, NQ
    c3, other, low, c2 = w.ct(USERS, level)[0], w.ct(USERS, level, which=1)[0], w.ct(USERS, 0)[0], w.ct(USERS[:2], level)[0]
    top = w.ct(USERS, NQ - 1)[0]
    one, two = np.zeros((1, level + 1, w.N), dtype=np.uint64), np.zeros((2, level + 1, w.N), dtype=np.uint64)
    r1, r2 = np.zeros((1, 2, lout, w.N), dtype=np.uint64), np.zeros((2, 2, lout, w.N), dtype=np.uint64)

    def refused(text, cts=(c3,), shares=(one, one, one), reenc=(r1, r1, r1), lout=NQ, **kw):
        rc, _ = w.refresh_merge(list(cts), list(shares), list(reenc), lout, **kw)
        assert rc != 0 and error().startswith("mkhe_refresh_merge: ") and text in error(), error()
        good_call(w)

    refused("same level", cts=(c3, low), shares=(two, two, two), reenc=(r2, r2, r2))
    refused("same ids", cts=(c3, c2), shares=(two, two, two), reenc=(r2, r2, r2))
    refused("nshares", shares=(one, one), reenc=(r1, r1))
    refused("nshares", nshares=-1)
    refused("exactly the id", re_ids=["user0", "user2", "user2"])
    refused("limbs of out", re_limbs=2)
    refused("aligned", ptrs=lambda bufs: w.handles([bufs[0].devptr(), C.c_void_p(bufs[1].devptr().value + 8), bufs[2].devptr()]))
    refused("null", ptrs=lambda bufs: w.handles([bufs[0].devptr(), None, bufs[2].devptr()]))
    refused("null", ptrs=lambda bufs: None)
    refused("null", re_list=lambda res: None)
    refused("null", re_list=lambda res: w.handles([res[0].h, None, res[2].h]))
    refused("null", handles=None)
    refused("count", count=0)
    refused("count", count=65536)
    refused("ids of the inputs", outs=[w.mk.Ciphertext(w.params, USERS[:2], NQ - 1)])
    refused("distinct", cts=(c3, other), shares=(two, two, two), reenc=(r2, r2, r2), outs=[w.mk.Ciphertext(w.params, USERS, NQ - 1)] * 2)
    t1, t3 = np.zeros((1, NQ, w.N), dtype=np.uint64), np.zeros((1, 2, NQ, w.N), dtype=np.uint64)
    refused("aliases an input", cts=(top,), shares=(t1, t1, t1), reenc=(t3, t3, t3), outs=[top])
    assert w.lib.mkhe_refresh_merge(None, 1, None, 0, None, None, None) != 0 and error() == "mkhe_refresh_merge: null context"
    rc, _ = w.refresh_merge([c3, other], [two, two, two], [r2, r2, r2], NQ)               # two ciphertexts over the same ids: accepted
    assert rc == 0, error()


def test_merge_refuses_an_output_that_is_a_reenc(w):
    solo = w.ct(["user0"], 0)[0]
    rc, sh, enc = w.refresh_share([solo], "user0", 10, NQ)
    assert rc == 0, error()
    buf = w.mk.DeviceLimbs(w.params, 1, 1).upload(sh)
    re = w.mk.Ciphertext(w.params, ["user0"], NQ - 1).upload(enc[0])
    rc = w.lib.mkhe_refresh_merge(w.params.ctx, 1, w.handles([solo.h]), 1, w.handles([buf.devptr()]), w.handles([re.h]), w.handles([re.h]))
    assert rc != 0 and error().startswith("mkhe_refresh_merge: ") and "aliases an input" in error()
    assert (re.download() == enc[0]).all()
    good_call(w)


def test_refused_on_a_bfv_context():
    from mkhe_kklss_amd import mkbfv, mkrlwe
    from mkhe_kklss_amd._abi import handle_array, lib
    p = HB.small_bfv(10, 3)
    params = mkbfv.Parameters(p["logN"], p["Q"], p["QMul"], p["P"], p["T"])
    params.AddCRS(0, seed=99)
    kgen = mkbfv.NewKeyGenerator(params, mkrlwe.HostSampler(np.random.default_rng(7), insecure_test_only=True))
    sk, pk = kgen.GenKeyPair("user0")
    N, L = 1 << p["logN"], len(p["Q"])
    ct = mkrlwe.Ciphertext(params, ["user0"], L - 1)
    out, res = mkrlwe.Ciphertext(params, ["user0"], L - 1), mkrlwe.Ciphertext(params, ["user0"], L - 1)
    buf = mkrlwe.DeviceLimbs(params, 1, L).upload(np.zeros((1, L, N), dtype=np.uint64))
    cdt = mkrlwe.small_cdt(3.2)
    rc = lib().mkhe_refresh_share(params.ctx, 1, handle_array([ct.h]), (C.c_int * 1)(1), sk.Value.devptr(), pk.Value.devptr(), key_arg(), 1, 2, 50,
                                  (C.c_uint64 * len(cdt))(*cdt), len(cdt), buf.devptr(), handle_array([out.h]))
    assert rc != 0 and error().startswith("mkhe_refresh_share: ") and "BFV" in error()
    rc = lib().mkhe_refresh_merge(params.ctx, 1, handle_array([ct.h]), 1, handle_array([buf.devptr()]), handle_array([out.h]), handle_array([res.h]))
    assert rc != 0 and error().startswith("mkhe_refresh_merge: ") and "BFV" in error()
    assert not out.download().any() and not res.download().any()
    # the context is usable: a share and its merge (distributed decryption is defined on BFV contexts)
    sh = mkrlwe.NewDecryptor(params).ShareNew(ct, sk, 0, None)
    assert not mkrlwe.NewDecryptor(params).MergeShares(ct, [sh]).download().any()
    params.close()


def test_refused_on_a_context_that_owns_a_subset_of_the_moduli(w):
    c, _ = w.ct(["user0"], 1)
    own = (C.c_int * 2)(0, 2)
    assert w.lib.mkhe_ctx_set_owned(w.params.ctx, own, 2) == 0, error()
    try:
        rc, _, _ = w.refresh_share([c], "user0", 50, NQ)
        assert rc != 0 and error().startswith("mkhe_refresh_share: ") and "subset of the moduli" in error()
        rc, _ = w.refresh_merge([c], [np.zeros((1, 2, w.N), dtype=np.uint64)], [np.zeros((1, 2, NQ, w.N), dtype=np.uint64)], NQ)
        assert rc != 0 and error().startswith("mkhe_refresh_merge: ") and "subset of the moduli" in error()
    finally:
        assert w.lib.mkhe_ctx_set_owned(w.params.ctx, own, 0) == 0
    good_call(w)


def test_refused_inside_a_capture(w):
    """(where the runtime of this process can capture at all: tests/test_gpu_cnn.py)"""
    from mkhe_kklss_amd._abi import MkheError
    c, _ = w.ct(["user0"], 1)
    cdt = (C.c_uint64 * len(w.cdt))(*w.cdt)
    buf = w.mk.DeviceLimbs(w.params, 1, 2).upload(np.full((1, 2, w.N), SENTINEL, dtype=np.uint64))
    re = w.mk.Ciphertext(w.params, ["user0"], NQ - 1)
    out = w.mk.Ciphertext(w.params, ["user0"], NQ - 1)
    try:
        with w.params.Capture():
            rc1 = w.lib.mkhe_refresh_share(w.params.ctx, 1, w.handles([c.h]), (C.c_int * 1)(1), w.sk["user0"].Value.devptr(), w.pk["user0"].Value.devptr(),
                                           key_arg(), 1, 2, 0, cdt, len(w.cdt), buf.devptr(), w.handles([re.h]))
            msg1 = error()
            rc2 = w.lib.mkhe_refresh_merge(w.params.ctx, 1, w.handles([c.h]), 1, w.handles([buf.devptr()]), w.handles([re.h]), w.handles([out.h]))
            msg2 = error()
        assert rc1 != 0 and msg1.startswith("mkhe_refresh_share: ") and "capture" in msg1
        assert rc2 != 0 and msg2.startswith("mkhe_refresh_merge: ") and "capture" in msg2
        print("capture: both refresh calls were refused inside a capture")
    except MkheError as e:
        print("capture: mkhe_capture_begin refused in this process (%s): the refusals inside a capture did not run" % e)
        import gc
        gc.enable()                 # (Graph.__enter__ switched the collector off before the refusal)
        assert "cannot end a multi-stream capture" in str(e)
    assert (buf.download() == SENTINEL).all() and not re.download().any() and not out.download().any()
    good_call(w)
