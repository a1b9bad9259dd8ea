"""The collective refresh of MK-BFV on the device (-m gpu), N = 2^10, bit for bit: mkhe_bfv_refresh_share against what
mkhe_decrypt_share(flood_bits = 0) writes plus tests/bfv_refresh_model.py's up(A) and flood, and against mkhe_encrypt of the model's plaintext and
samples; mkhe_bfv_refresh_merge as a pure function against the integer model and against the composition mkhe_decrypt_merge ->
mkhe_bfv_scale_down -> mkhe_bfv_scale_up it replaces, on uniform and on crafted inputs at the rounding boundaries; every refusal followed by a
call that works.  Three rings: the three-prime chain with T = 65537, the chain with the 55-bit tail and the largest T below 2^32, and one limb
(one Garner digit).  The end-to-end test on mkbfv is tests/test_gpu_bfv_refresh_e2e.py."""
import ctypes as C

import numpy as np
import pytest

import bfv_refresh_model as B
import device_sampler_model as M
import harness as H
import harness_bfv as HB
from gpu_common import is_prime

pytestmark = pytest.mark.gpu

KEY = [0x9E3779B9, 0x7F4A7C15, 0xF39CC060, 0x5CEDC834, 0x1082276B, 0xF3A27251, 0xF86C6A11, 0xD0C18E95]
NONCE_MASK, NONCE_ENC = 0xFEDCBA9876543210, 0x0123456789ABCDEF
SENTINEL = 0x7B7B7B7B7B7B7B7B
BITS = [0, 1, 63, 64, 65, 128, 129]
USERS = ["user0", "user1", "user2"]
LOGN = 10


def big_t():
    """the largest prime = 1 mod 2^11 below 2^32"""
    step = 1 << (LOGN + 1)
    t = ((1 << 32) - 2) // step * step + 1
    while not is_prime(t):
        t -= step
    return t


RINGS = {"three": HB.small_bfv(LOGN, 3), "big": dict(HB.small_bfv(LOGN, 3, big=True), T=big_t()), "one": HB.small_bfv(LOGN, 1)}


def key_arg(key=KEY):
    return None if key is None else (C.c_uint32 * 8)(*key)


def error():
    from mkhe_kklss_amd._abi import lib
    return lib().mkhe_last_error().decode()


_streams = {}


def stream(key, nonce, s, n):
    """the 64-bit values of one stream of KEY, computed once for the whole module"""
    assert key == KEY
    if (nonce, s) not in _streams:
        _streams[(nonce, s)] = M.stream_values(KEY, nonce, s, n)
    return _streams[(nonce, s)]


class World:
    """a BFV context over one ring, three parties with keys made on it, and the raw calls"""

    def __init__(self, pset):
        from mkhe_kklss_amd import mkbfv, mkrlwe
        from mkhe_kklss_amd._abi import handle_array, lib
        self.mk, self.bfv, self.lib, self.handles, self.N = mkrlwe, mkbfv, lib(), handle_array, 1 << LOGN
        self.Q, self.T, self.L = pset["Q"], pset["T"], len(pset["Q"])
        self.params = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], pset["T"])
        self.params.AddCRS(0, seed=99)
        self.rng = np.random.default_rng(2028)
        kgen = mkbfv.NewKeyGenerator(self.params, mkrlwe.HostSampler(np.random.default_rng(7), insecure_test_only=True))
        self.sk, self.pk = {}, {}
        for u in USERS:
            self.sk[u], self.pk[u] = kgen.GenKeyPair(u)
        self.cdt = mkrlwe.small_cdt(3.2)
        self.Qprod = B.q_product(self.Q)
        self.most = (self.Qprod // (2 * self.T)).bit_length() - 1          # the widest flood the engine takes
        self._ct = {}

    def uniform(self, shape_head):
        return np.stack([self.rng.integers(0, q, tuple(shape_head) + (self.N,), dtype=np.uint64) for q in self.Q], axis=len(shape_head))

    def ct(self, ids, which=0):
        """a uniform ciphertext over ids (made once per id set and number) -> (device ciphertext, host copy)"""
        k = (tuple(ids), which)
        if k not in self._ct:
            host = self.uniform((1 + len(ids),))
            self._ct[k] = (self.bfv.Ciphertext(self.params, list(ids)).upload(host), host)
        return self._ct[k]

    def q(self):
        return np.array(self.Q, dtype=np.uint64)[:, None]

    def limbs(self, count):
        return self.mk.DeviceLimbs(self.params, count, self.L)

    def samples(self, count):
        """the model's u, e0, e1 of the encryption streams: int32 [count][3][N] (as tests/test_gpu_refresh.py)"""
        cdt, out = np.array(self.cdt, dtype=np.uint64), np.empty((count, 3, self.N), dtype=np.int32)
        for b in range(count):
            for j in range(3):
                r = np.array(stream(KEY, NONCE_ENC, 3 * b + j, self.N), dtype=np.uint64)
                out[b, j] = np.where(r & np.uint64(1), 0, np.where(r & np.uint64(2), 1, -1)) if j == 0 else np.searchsorted(cdt, r, side="right") - len(cdt) // 2
        assert out[0, :, :8].tolist() == [p[:8] for p in M.encrypt_samples(1, KEY, NONCE_ENC, 8, self.cdt)[0]]
        return out

    # ---- the raw calls
    def decrypt_share(self, cts, who):
        n = len(cts)
        buf = self.limbs(n)
        assert self.lib.mkhe_decrypt_share(self.params.ctx, n, self.handles([c.h for c in cts]), (C.c_int * n)(*[c.slot(who) for c in cts]),
                                           self.sk[who].Value.devptr(), None, 0, 0, buf.devptr()) == 0, error()
        return buf.download()

    def encrypt(self, who, pt, samples):
        """mkhe_encrypt of host plaintexts [count][L][N] on host samples -> uint64 [count][2][L][N]"""
        n = pt.shape[0]
        d = self.limbs(n).upload(pt)
        outs = self.mk.batch_ciphertexts(self.mk.Ciphertext, self.params, [who], self.L - 1, n)
        smp = np.ascontiguousarray(samples, dtype=np.int32)
        assert self.lib.mkhe_encrypt(self.params.ctx, self.L - 1, n, self.pk[who].Value.devptr(), d.devptr(), 0, smp.ctypes.data_as(C.POINTER(C.c_int32)),
                                     self.handles([c.h for c in outs])) == 0, error()
        return np.stack([c.download() for c in outs])

    def share(self, cts, who, mask, bits, key=KEY, nonce_mask=NONCE_MASK, nonce_enc=NONCE_ENC, count=None, slots=None, sk="default", pk="default",
              out=None, handles="default", reenc="default", cdt="default", ncdt=None):
        """mkhe_bfv_refresh_share into a share buffer of twice the size filled with a sentinel and sentinel-filled outputs
        -> (rc, shares uint64 [count][L][N], reenc uint64 [count][2][L][N]); a refused call leaves all of it untouched"""
        n, L = len(cts), self.L
        buf = self.limbs(2 * n).upload(np.full((2 * n, L, self.N), SENTINEL, dtype=np.uint64))
        sl = [c.slot(who) for c in cts] if slots is None else slots
        outs = [self.mk.Ciphertext(self.params, [c.ids[min(max(s, 1), len(c.ids)) - 1]], L - 1).upload(np.full((2, L, self.N), SENTINEL, dtype=np.uint64))
                for c, s in zip(cts, sl)]
        table = (C.c_uint64 * len(self.cdt))(*self.cdt) if cdt == "default" else cdt
        rc = self.lib.mkhe_bfv_refresh_share(self.params.ctx, n if count is None else count, self.handles([c.h for c in cts]) if handles == "default" else handles,
                                             (C.c_int * n)(*sl), self.sk[who].Value.devptr() if sk == "default" else sk,
                                             self.pk[who].Value.devptr() if pk == "default" else pk, key_arg(key), nonce_mask, nonce_enc, mask, bits,
                                             table, len(self.cdt) if ncdt is None else ncdt, buf.devptr() if out is None else out(buf),
                                             self.handles([c.h for c in outs]) if reenc == "default" else reenc(outs))
        got, enc = buf.download(), np.stack([c.download() for c in outs])
        if rc == 0:
            assert (got[n:] == SENTINEL).all(), "mkhe_bfv_refresh_share wrote behind uint64[count][nQ][N]"
        else:
            assert (got == SENTINEL).all() and (enc == SENTINEL).all(), "a refused mkhe_bfv_refresh_share wrote to its outputs"
        return rc, got[:n], enc

    def merge(self, cts, shares, reenc, nshares=None, count=None, handles="default", ptrs="default", re_ids=None, re_limbs=None, re_list="default", outs=None):
        """mkhe_bfv_refresh_merge of host share arrays [count][L][N] and host re-encryptions [count][2][L][N] (one of each per party, slot order)
        -> (rc, [count] of uint64 [1 + k][L][N])"""
        n, L, ids = len(cts), self.L, cts[0].ids
        bufs = [self.limbs(n).upload(s) for s in shares]
        res = []
        for i, r in enumerate(reenc):
            for b in range(n):
                rid, rl = (ids[i] if re_ids is None else re_ids[i]), (L if re_limbs is None else re_limbs)
                c = self.mk.Ciphertext(self.params, [rid], rl - 1)
                res.append(c.upload(r[b] if rl == L else np.zeros((2, rl, self.N), dtype=np.uint64)))
        if outs is None:
            outs = [self.mk.Ciphertext(self.params, ids, L - 1).upload(np.full((1 + len(ids), L, self.N), SENTINEL, dtype=np.uint64)) for _ in range(n)]
        rc = self.lib.mkhe_bfv_refresh_merge(self.params.ctx, n if count is None else count, self.handles([c.h for c in cts]) if handles == "default" else handles,
                                             len(bufs) if nshares is None else nshares, self.handles([b.devptr() for b in bufs]) if ptrs == "default" else ptrs(bufs),
                                             (self.handles([c.h for c in res]) if res else None) if re_list == "default" else re_list(res),
                                             self.handles([c.h for c in outs]))
        return rc, [c.download() for c in outs]

    def composition(self, cts, shares, reenc):
        """what the merge replaces: mkhe_decrypt_merge, mkhe_bfv_scale_down, mkhe_bfv_scale_up, and the re-encryptions' c0 added on the host
        -> uint64 [count][L][N], polynomial 0 of the outputs"""
        n = len(cts)
        bufs = [self.limbs(n).upload(s) for s in shares]
        pt, coeffs, up = self.limbs(n), self.mk.DeviceLimbs(self.params, n, 1), self.limbs(n)
        assert self.lib.mkhe_decrypt_merge(self.params.ctx, n, self.handles([c.h for c in cts]), len(bufs),
                                           self.handles([b.devptr() for b in bufs]) if bufs else None, pt.devptr()) == 0, error()
        assert self.lib.mkhe_bfv_scale_down(self.params.ctx, n, pt.devptr(), coeffs.devptr()) == 0, error()
        assert self.lib.mkhe_bfv_scale_up(self.params.ctx, n, coeffs.devptr(), up.devptr()) == 0, error()
        out = up.download()
        for r in reenc:
            out = (out + r[:, 0]) % self.q()
        return out


_worlds = {}


@pytest.fixture(scope="module", params=list(RINGS))
def w(request):
    if request.param not in _worlds:
        _worlds[request.param] = World(RINGS[request.param])
    return _worlds[request.param]


@pytest.fixture(scope="module")
def w3():
    if "three" not in _worlds:
        _worlds["three"] = World(RINGS["three"])
    return _worlds["three"]


def id_sets(who):
    """ciphertexts over 1, 2 and 3 parties that `who` belongs to (test_gpu_decrypt_share.py): its slot differs between them"""
    pair = ["user0", "user1"] if who != "user2" else ["user1", "user2"]
    return [[who], pair, USERS]


def test_the_second_ring_has_the_largest_t_below_2_32():
    t = RINGS["big"]["T"]
    assert t == 4294957057 and is_prime(t) and t % (1 << (LOGN + 1)) == 1 and t not in RINGS["big"]["Q"]
    assert max(RINGS["big"]["Q"]) >> 54 == 1 and len(RINGS["one"]["Q"]) == 1


# ------------------------------------------------------------------ the share
@pytest.mark.parametrize("count", [1, 3])
def test_share_is_the_plain_share_plus_up_of_the_mask_plus_the_flood_and_reenc_is_encrypt_of_up_of_minus_the_mask(w, count):
    who = "user1"
    sets = id_sets(who)
    cts = [w.ct(sets[b % 3])[0] for b in range(count)]          # different id sets and slots in one call
    assert count < 3 or len({c.slot(who) for c in cts}) > 1
    before = [c.download() for c in cts]
    plain = w.decrypt_share(cts, who)                           # mkhe_decrypt_share, flood_bits = 0
    smp = w.samples(count)
    widths = [f for f in BITS if f <= w.most] + [w.most]
    assert w.most == w.bfv.NewRefresher(w.params).MaxFloodBits(1) and len(widths) >= 2
    for mask in (0, 1):
        for bits in widths:
            rc, got, enc = w.share(cts, who, mask, bits)
            assert rc == 0, error()
            A = [B.mask_poly(KEY, NONCE_MASK, b, w.N, w.T, bits, mask, values=stream) for b in range(count)]
            e = [B.flood_poly(KEY, NONCE_MASK, b, w.N, bits, values=stream) for b in range(count)]
            want = np.stack([(plain[b] + B.share_addend(A[b], e[b], w.Q, w.T)) % w.q() for b in range(count)])
            assert (got == want).all(), (mask, bits, "share")
            pt = np.stack([B.reenc_plaintext(A[b], w.Q, w.T) for b in range(count)])
            assert (enc == w.encrypt(who, pt, smp)).all(), (mask, bits, "reenc")      # mkhe_encrypt on the model's plaintext and samples
            assert all(0 <= a < w.T for a in A[0]) and (len(set(A[0])) > 1) == bool(mask)
            if bits:
                assert all(-(1 << (bits - 1)) <= v < (1 << (bits - 1)) for v in e[0]) and len(set(e[0])) > 1
            if not mask:
                assert not pt.any()                             # the zero plaintext
                if not bits:
                    assert (got == plain).all()                 # PartialDecrypt's product: what mkhe_decrypt_share(flood_bits = 0) gives
    assert all((c.download() == x).all() for c, x in zip(cts, before))       # the inputs are left alone


def test_seventeen_items_stage_the_pointer_tables(w3):
    w, who, count = w3, "user2", 17
    sets = id_sets(who)
    cts = [w.ct(sets[b % 3], which=b // 3 % 2)[0] for b in range(count)]
    plain = w.decrypt_share(cts, who)
    rc, got, enc = w.share(cts, who, 1, 65)
    assert rc == 0, error()
    for b in (0, 1, 16):
        A, e = B.mask_poly(KEY, NONCE_MASK, b, w.N, w.T, 65, values=stream), B.flood_poly(KEY, NONCE_MASK, b, w.N, 65, values=stream)
        assert (got[b] == (plain[b] + B.share_addend(A, e, w.Q, w.T)) % w.q()).all(), b
    shares = [w.uniform((count,)) for _ in USERS]
    reenc = [w.uniform((count, 2)) for _ in USERS]
    all3 = [w.ct(USERS, which=b % 2) for b in range(count)]
    rc, out = w.merge([c for c, _ in all3], shares, reenc)
    assert rc == 0, error()
    for b in (0, 1, 16):
        assert (out[b] == B.merge(w.Q, w.T, all3[b][1][0], [s[b] for s in shares], [r[b] for r in reenc])).all(), b


def test_a_flood_of_twelve_words_on_the_full_chain():
    """the 14 primes of PN15QP880 at N = 2^10: Q has 760 bits and the widest flood 742 -- twelve streams, the top word of 38 bits; and a width
    that ends on a word boundary.  Share, re-encryption and one merge on that chain (14 Garner digits)."""
    w, who = World(HB.small_bfv(LOGN, 14)), "user0"
    assert w.L == 14 and w.most == 742 and B.words(w.most) == 12
    cts = [w.ct(USERS[:2])[0]]
    plain, smp = w.decrypt_share(cts, who), w.samples(1)
    for bits in (w.most, 704):
        rc, got, enc = w.share(cts, who, 1, bits)
        assert rc == 0, error()
        A, e = B.mask_poly(KEY, NONCE_MASK, 0, w.N, w.T, bits, values=stream), B.flood_poly(KEY, NONCE_MASK, 0, w.N, bits, values=stream)
        assert max(e).bit_length() >= bits - 8 and -min(e) >> (bits - 8)
        assert (got[0] == (plain[0] + B.share_addend(A, e, w.Q, w.T)) % w.q()).all(), bits
        assert (enc == w.encrypt(who, B.reenc_plaintext(A, w.Q, w.T)[None], smp)).all(), bits
    rc, _, _ = w.share(cts, who, 1, w.most + 1)
    assert rc != 0 and "destroys the message" in error()
    items = [w.ct(USERS[:2])]
    shares, reenc = [w.uniform((1,)) for _ in range(2)], [w.uniform((1, 2)) for _ in range(2)]
    rc, out = w.merge([items[0][0]], shares, reenc)
    assert rc == 0, error()
    assert (out[0] == B.merge(w.Q, w.T, items[0][1][0], [s[0] for s in shares], [r[0] for r in reenc])).all()
    assert (out[0][0] == w.composition([items[0][0]], shares, reenc)[0]).all()
    w.params.close()


def test_share_depends_on_both_nonces_and_the_key(w3):
    w = w3
    cts = [w.ct(USERS)[0]] * 2
    a, b, c, d, e = (w.share(cts, "user0", 1, 100, nonce_mask=nm, nonce_enc=ne, key=k)
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
@pytest.mark.parametrize("count", [1, 3])
def test_merge_is_the_integer_model_and_the_composition_it_replaces(w, count, k):
    ids = USERS[:k]
    items = [w.ct(ids, which=b % 2) for b in range(count)]
    cts = [c for c, _ in items]
    shares = [w.uniform((count,)) for _ in ids]
    reenc = [w.uniform((count, 2)) for _ in ids]
    rc, got = w.merge(cts, shares, reenc)
    assert rc == 0, error()
    comp = w.composition(cts, shares, reenc)
    for b in range(count):
        want = B.merge(w.Q, w.T, items[b][1][0], [s[b] for s in shares], [r[b] for r in reenc])
        assert (got[b] == want).all(), b
        assert (got[b][0] == comp[b]).all(), b
    assert all((c.download() == h).all() for c, h in items)


@pytest.mark.parametrize("k", [0, 2])
def test_merge_rounds_exactly_at_the_boundaries(w, k):
    """all shares and re-encryptions zero, c_0 = the residues of crafted R: 0, Q - 1, and for x in {0, 1, h, T - 1} the two integers on either
    side of (2x + 1) Q / (2T) -- polynomial 0 of the output is up(x) below the boundary and up(x + 1) above it"""
    ids, Q, T = USERS[:k], w.Qprod, w.T
    Rs, ws = [0, Q - 1], [0, 0]
    for x in (0, 1, T // 2, T - 1):
        edge = (2 * x + 1) * Q // (2 * T)
        Rs += [edge, edge + 1]
        ws += [x, (x + 1) % T]
    assert [B.down(R, w.Q, T) for R in Rs] == ws
    host = w.uniform((1 + k,))
    for j, q in enumerate(w.Q):
        host[0, j, : len(Rs)] = [R % q for R in Rs]
    ct = w.bfv.Ciphertext(w.params, ids).upload(host)
    zero_s, zero_r = np.zeros((1, w.L, w.N), dtype=np.uint64), np.zeros((1, 2, w.L, w.N), dtype=np.uint64)
    rc, got = w.merge([ct], [zero_s] * k, [zero_r] * k)
    assert rc == 0, error()
    for i, x in enumerate(ws):
        assert [int(got[0][0, j, i]) for j in range(w.L)] == [B.up(x, w.Q, T) % q for q in w.Q], (i, Rs[i])
    assert (got[0] == B.merge(w.Q, T, host[0], [zero_s[0]] * k, [zero_r[0]] * k)).all()
    assert (got[0][0] == w.composition([ct], [zero_s] * k, [zero_r] * k)[0]).all()
    assert not got[0][1:].any()                                 # polynomial 1 of the zero re-encryptions


# ------------------------------------------------------------------ refusals
def good_call(w):
    """the context works: a share and a merge of one party's ciphertext, whose result is over the same id"""
    c, _ = w.ct(["user0"])
    rc, sh, enc = w.share([c], "user0", 1, 20)
    assert rc == 0, error()
    rc, got = w.merge([c], [sh], [enc])
    assert rc == 0 and (got[0][1] == enc[0][1]).all(), error()


def test_refresh_share_refusals(w3):
    w = w3
    c3, c2 = w.ct(USERS)[0], w.ct(USERS[:2])[0]
    solo = w.ct(["user1"])[0]
    low = w.mk.Ciphertext(w.params, USERS, 0)

    def refused(text, cts=(c3,), who="user1", mask=1, bits=100, **kw):
        rc, _, _ = w.share(list(cts), who, mask, bits, **kw)
        assert rc != 0 and error().startswith("mkhe_bfv_refresh_share: ") and text in error() and not any("%08x" % x in error().lower() for x in KEY), error()
        good_call(w)

    refused("mask must be 0 or 1", mask=2)
    refused("mask must be 0 or 1", mask=-1)
    refused("flood_bits", bits=-1)
    refused("flood_bits", bits=1025)
    refused("destroys the message", bits=w.most + 1)
    refused("null key", key=None)
    refused("null key", key=None, mask=0, bits=0)
    refused("nonce_mask and nonce_enc must differ", nonce_mask=5, nonce_enc=5)
    refused("nonce_mask and nonce_enc must differ", nonce_mask=5, nonce_enc=5, mask=0, bits=1)
    refused("nonce_mask and nonce_enc must differ", nonce_mask=5, nonce_enc=5, mask=1, bits=0)
    refused("slot out of range", slots=[0])
    refused("slot out of range", slots=[4])
    refused("slot out of range", cts=(c3, c2), slots=[3, 3])
    refused("nQ limbs", cts=(c3, low))
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
    pair, wrong, short = (w.mk.Ciphertext(w.params, ids, lvl) for ids, lvl in ((USERS[:2], w.L - 1), (["user0"], w.L - 1), (["user1"], 0)))
    refused("exactly the id", reenc=lambda outs: w.handles([pair.h]))
    refused("exactly the id", reenc=lambda outs: w.handles([wrong.h]))
    refused("nQ limbs", cts=(c3, c3), reenc=lambda outs: w.handles([outs[0].h, short.h]))
    assert not pair.download().any() and not wrong.download().any() and not short.download().any()
    refused("distinct", cts=(c3, c3), reenc=lambda outs: w.handles([outs[0].h, outs[0].h]))
    refused("aliases an input", cts=(solo,), reenc=lambda outs: w.handles([solo.h]))
    assert w.lib.mkhe_bfv_refresh_share(None, 1, None, None, None, None, None, 0, 1, 1, 0, None, 0, None, None) != 0
    assert error() == "mkhe_bfv_refresh_share: null key"
    rc, _, _ = w.share([c3], "user1", 0, 0, nonce_mask=5, nonce_enc=5)       # no stream of nonce_mask is read: the nonces may coincide
    assert rc == 0, error()
    rc, _, _ = w.share([c3], "user1", 1, w.most)                              # the widest flood
    assert rc == 0, error()


def test_refresh_merge_refusals(w3):
    w = w3
    c3, other, c2 = w.ct(USERS)[0], w.ct(USERS, which=1)[0], w.ct(USERS[:2])[0]
    low = w.mk.Ciphertext(w.params, USERS, 0)
    one, two = np.zeros((1, w.L, w.N), dtype=np.uint64), np.zeros((2, w.L, w.N), dtype=np.uint64)
    r1, r2 = np.zeros((1, 2, w.L, w.N), dtype=np.uint64), np.zeros((2, 2, w.L, w.N), dtype=np.uint64)

    def refused(text, cts=(c3,), shares=(one, one, one), reenc=(r1, r1, r1), **kw):
        rc, _ = w.merge(list(cts), list(shares), list(reenc), **kw)
        assert rc != 0 and error().startswith("mkhe_bfv_refresh_merge: ") and text in error(), error()
        good_call(w)

    refused("nQ limbs", cts=(c3, low), shares=(two, two, two), reenc=(r2, r2, r2))
    refused("same ids", cts=(c3, c2), shares=(two, two, two), reenc=(r2, r2, r2))
    refused("nshares", shares=(one, one), reenc=(r1, r1))
    refused("nshares", nshares=-1)
    refused("exactly the id", re_ids=["user0", "user2", "user2"])
    refused("nQ limbs", re_limbs=2)
    refused("aligned", ptrs=lambda bufs: w.handles([bufs[0].devptr(), C.c_void_p(bufs[1].devptr().value + 8), bufs[2].devptr()]))
    refused("null", ptrs=lambda bufs: w.handles([bufs[0].devptr(), None, bufs[2].devptr()]))
    refused("null", ptrs=lambda bufs: None)
    refused("null", re_list=lambda res: None)
    refused("null", re_list=lambda res: w.handles([res[0].h, None, res[2].h]))
    refused("null", handles=None)
    refused("count", count=0)
    refused("count", count=65536)
    refused("ids of the inputs", outs=[w.mk.Ciphertext(w.params, USERS[:2], w.L - 1)])
    refused("nQ limbs", outs=[w.mk.Ciphertext(w.params, USERS, 1)])
    refused("distinct", cts=(c3, other), shares=(two, two, two), reenc=(r2, r2, r2), outs=[w.mk.Ciphertext(w.params, USERS, w.L - 1)] * 2)
    keep = c3.download()
    refused("aliases an input", outs=[c3])
    assert (c3.download() == keep).all()
    assert w.lib.mkhe_bfv_refresh_merge(None, 1, None, 0, None, None, None) != 0 and error() == "mkhe_bfv_refresh_merge: null context"
    rc, _ = w.merge([c3, other], [two, two, two], [r2, r2, r2])               # two ciphertexts over the same ids: accepted
    assert rc == 0, error()


def test_merge_refuses_an_output_that_is_a_reenc(w3):
    w = w3
    solo = w.ct(["user0"])[0]
    rc, sh, enc = w.share([solo], "user0", 1, 10)
    assert rc == 0, error()
    buf = w.limbs(1).upload(sh)
    re = w.mk.Ciphertext(w.params, ["user0"], w.L - 1).upload(enc[0])
    rc = w.lib.mkhe_bfv_refresh_merge(w.params.ctx, 1, w.handles([solo.h]), 1, w.handles([buf.devptr()]), w.handles([re.h]), w.handles([re.h]))
    assert rc != 0 and error().startswith("mkhe_bfv_refresh_merge: ") and "aliases an input" in error()
    assert (re.download() == enc[0]).all()
    good_call(w)


def raw_calls(mk, params, sk, pk, L, N):
    """both calls on one fresh ciphertext of a context -> ((rc, message) of the share, (rc, message) of the merge, the buffers they may have written)"""
    from mkhe_kklss_amd._abi import handle_array, lib
    ct, re, out = (mk.Ciphertext(params, ["user0"], L - 1) for _ in range(3))
    buf = mk.DeviceLimbs(params, 1, L).upload(np.zeros((1, L, N), dtype=np.uint64))
    cdt = mk.small_cdt(3.2)
    rc1 = lib().mkhe_bfv_refresh_share(params.ctx, 1, handle_array([ct.h]), (C.c_int * 1)(1), sk.Value.devptr(), pk.Value.devptr(), key_arg(), 1, 2, 1, 20,
                                       (C.c_uint64 * len(cdt))(*cdt), len(cdt), buf.devptr(), handle_array([re.h]))
    m1 = error()
    rc2 = lib().mkhe_bfv_refresh_merge(params.ctx, 1, handle_array([ct.h]), 1, handle_array([buf.devptr()]), handle_array([re.h]), handle_array([out.h]))
    return (rc1, m1), (rc2, error()), (ct, buf, re, out)


def test_refused_on_a_context_that_is_not_bfv():
    from mkhe_kklss_amd import mkrlwe
    params = mkrlwe.Parameters(LOGN, RINGS["three"]["Q"], H.PN15QP880["P"])
    params.AddCRS(0, seed=99)
    sk, pk = mkrlwe.NewKeyGenerator(params, mkrlwe.HostSampler(np.random.default_rng(7), insecure_test_only=True)).GenKeyPair("user0")
    (rc1, m1), (rc2, m2), (ct, buf, re, out) = raw_calls(mkrlwe, params, sk, pk, 3, 1 << LOGN)
    assert rc1 != 0 and m1.startswith("mkhe_bfv_refresh_share: ") and "BFV context" in m1
    assert rc2 != 0 and m2.startswith("mkhe_bfv_refresh_merge: ") and "BFV context" in m2
    assert not re.download().any() and not out.download().any() and not buf.download().any()
    # the context is usable: the refresh of its own kind
    sh = mkrlwe.NewRefresher(params).ShareNew(ct, sk, pk, 20, mkrlwe.DeviceSampler())
    assert mkrlwe.NewRefresher(params).MergeNew(ct, [sh]).Level() == 2
    params.close()


@pytest.mark.parametrize("t,text", [(257, "1 mod 2N"), (2049, "prime"), (4294967311, "below 2^32")])      # (as tests/test_gpu_bfv_encoder_stages.py)
def test_refused_for_a_plaintext_modulus_outside_the_preconditions_of_the_encoder(t, text):
    from mkhe_kklss_amd import mkbfv, mkrlwe
    p = RINGS["three"]
    params = mkbfv.Parameters(p["logN"], p["Q"], p["QMul"], p["P"], t)
    params.AddCRS(0, seed=99)
    sk, pk = mkbfv.NewKeyGenerator(params, mkrlwe.HostSampler(np.random.default_rng(7), insecure_test_only=True)).GenKeyPair("user0")
    (rc1, m1), (rc2, m2), (ct, buf, re, out) = raw_calls(mkrlwe, params, sk, pk, 3, 1 << LOGN)
    assert rc1 != 0 and m1.startswith("mkhe_bfv_refresh_share: ") and text in m1, m1
    assert rc2 != 0 and m2.startswith("mkhe_bfv_refresh_merge: ") and text in m2, m2
    assert not re.download().any() and not out.download().any() and not buf.download().any()
    # the context is usable: a share and its merge of distributed decryption
    sh = mkrlwe.NewDecryptor(params).ShareNew(ct, sk, 0, None)
    assert not mkrlwe.NewDecryptor(params).MergeShares(ct, [sh]).download().any()
    params.close()


def test_refused_on_a_context_that_owns_a_subset_of_the_moduli(w3):
    """Both calls refuse such a context (capi.hip: the step of the shared guard that holds the refusal), but no BFV context can become one:
    mkhe_ctx_set_owned itself refuses BFV contexts.  That refusal is what keeps the two calls off a subset of the moduli, so it is what is checked,
    with a call that works behind it; the source is read for the rest: the step holds the refusal, and both entry points reach it, through the
    functions they call, before they arm g_last_ctx."""
    w = w3
    own = (C.c_int * 2)(0, 2)
    assert w.lib.mkhe_ctx_set_owned(w.params.ctx, own, 2) != 0 and "limb sharding is wired for the mkckks path" in error()
    good_call(w)
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mkhe-kklss_amd", "csrc", "capi.hip")).read()
    refusal = 'if (c->masked()) throw Error(std::string(what) + ": not available on a context that owns a subset of the moduli");'
    # every function defined at the start of a line: name -> its text from the name to the closing brace in column 0
    bodies = {m.group(1): src[m.start():src.index("\n}\n", m.start())] for m in re.finditer(r"^[A-Za-z].*?\b(\w+)\([^;{}]*\) \{$", src, flags=re.M)}
    holders = [name for name, body in bodies.items() if "owns a subset of the moduli" in body]
    assert len(holders) == 1 and refusal in bodies[holders[0]], holders

    def arms(name):
        """the last value the function itself gives g_last_ctx is a context"""
        values = re.findall(r"g_last_ctx = (\w+)", bodies[name])
        return bool(values) and values[-1] != "nullptr"

    def reached(name, seen):
        """the functions of the file that `name` calls, and those call in turn, each up to the first place where it sets g_last_ctx or calls a
        function that arms it"""
        if name in seen:
            return seen
        seen.add(name)
        for m in re.finditer(r"g_last_ctx = |\b(\w+)\(", bodies[name].split("{", 1)[1]):
            if m.group(1) is None or (m.group(1) in bodies and arms(m.group(1))):
                break
            if m.group(1) in bodies:
                reached(m.group(1), seen)
        return seen

    for entry in ("mkhe_bfv_refresh_share", "mkhe_bfv_refresh_merge"):
        assert holders[0] in reached(entry, set()), entry


def test_refused_inside_a_capture(w3):
    """(where the runtime of this process can capture at all: tests/test_gpu_cnn.py)"""
    from mkhe_kklss_amd._abi import MkheError
    w = w3
    c, _ = w.ct(["user0"])
    cdt = (C.c_uint64 * len(w.cdt))(*w.cdt)
    buf = w.limbs(1).upload(np.full((1, w.L, w.N), SENTINEL, dtype=np.uint64))
    re = w.mk.Ciphertext(w.params, ["user0"], w.L - 1)
    out = w.mk.Ciphertext(w.params, ["user0"], w.L - 1)
    try:
        with w.params.Capture():
            rc1 = w.lib.mkhe_bfv_refresh_share(w.params.ctx, 1, w.handles([c.h]), (C.c_int * 1)(1), w.sk["user0"].Value.devptr(), w.pk["user0"].Value.devptr(),
                                               key_arg(), 1, 2, 1, 20, cdt, len(w.cdt), buf.devptr(), w.handles([re.h]))
            msg1 = error()
            rc2 = w.lib.mkhe_bfv_refresh_merge(w.params.ctx, 1, w.handles([c.h]), 1, w.handles([buf.devptr()]), w.handles([re.h]), w.handles([out.h]))
            msg2 = error()
        assert rc1 != 0 and msg1.startswith("mkhe_bfv_refresh_share: ") and "capture" in msg1
        assert rc2 != 0 and msg2.startswith("mkhe_bfv_refresh_merge: ") and "capture" in msg2
        print("capture: both calls were refused inside a capture")
    except MkheError as e:
        print("capture: mkhe_capture_begin refused in this process (%s): the refusals inside a capture did not run" % e)
        import gc
        gc.enable()                 # (Graph.__enter__ switched the collector off before the refusal)
        assert "cannot end a multi-stream capture" in str(e)
    assert (buf.download() == SENTINEL).all() and not re.download().any() and not out.download().any()
    good_call(w)
