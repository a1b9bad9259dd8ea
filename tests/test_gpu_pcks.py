"""The collective key switch to a recipient's public key on the device (-m gpu), N = 2^10, bit for bit: mkhe_pcks_share against the composition
of existing calls -- h0 = what mkhe_decrypt_share(flood_bits = 0) writes + c0 of mkhe_encrypt(pt = 0) on the model's samples (u, 0, e1) + the
model's flood, h1 = c1 of that mkhe_encrypt -- and mkhe_pcks_merge as a pure function against tests/pcks_model.py and against
mkhe_decrypt_merge; determinism and dependence on key and nonce; every refusal followed by a call that works.  Four rings: the three-prime BFV
chain, one limb, the 14 primes of PN15QP880 (a flood of twelve words), and an mkrlwe context whose inputs are BELOW the maximum level, where
row L + j of the public key is not pk1.  The end-to-end tests on mkckks and mkbfv are tests/test_gpu_pcks_e2e.py."""
import ctypes as C

import numpy as np
import pytest

import decrypt_share_model as D
import device_sampler_model as M
import harness as H
import harness_bfv as HB
import pcks_model as P

pytestmark = pytest.mark.gpu

KEY = [0x9E3779B9, 0x7F4A7C15, 0xF39CC060, 0x5CEDC834, 0x1082276B, 0xF3A27251, 0xF86C6A11, 0xD0C18E95]
NONCE = 0xFEDCBA9876543210
SENTINEL = 0x7B7B7B7B7B7B7B7B
BITS = [0, 1, 63, 64, 65, 128, 129]
USERS = ["user0", "user1", "user2"]
EVERYONE = USERS + ["carol"]                # carol holds no part of any ciphertext
LOGN = 10
RINGS = {"three": ("bfv", HB.small_bfv(LOGN, 3), 3), "one": ("bfv", HB.small_bfv(LOGN, 1), 1), "low": ("rlwe", H.small_ckks(LOGN, 4), 2)}


def key_arg(key=KEY):
    return None if key is None else (C.c_uint32 * 8)(*key)


def error():
    from mkhe_kklss_amd._abi import lib
    return lib().mkhe_last_error().decode()


_streams = {}


def stream(key, nonce, s, n):
    """the 64-bit values of one stream, computed once for the whole module"""
    k = (tuple(key), nonce, s)
    if k not in _streams:
        _streams[k] = M.stream_values(key, nonce, s, n)
    return _streams[k]


class World:
    """a context over one ring (BFV, or mkrlwe with the inputs at L limbs, below the maximum level), three parties and a recipient with keys
    made on it, and the raw calls"""

    def __init__(self, kind, pset, L):
        from mkhe_kklss_amd import mkbfv, mkrlwe
        from mkhe_kklss_amd._abi import handle_array, lib
        self.mk, self.lib, self.handles, self.N, self.L, self.kind = mkrlwe, lib(), handle_array, 1 << LOGN, L, kind
        if kind == "bfv":
            self.params = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], pset["T"])
            kgen, self.Tp = mkbfv.NewKeyGenerator(self.params, mkrlwe.HostSampler(np.random.default_rng(7), insecure_test_only=True)), pset["T"]
        else:
            self.params = mkrlwe.Parameters(pset["logN"], pset["Q"], pset["P"])
            kgen, self.Tp = mkrlwe.NewKeyGenerator(self.params, mkrlwe.HostSampler(np.random.default_rng(7), insecure_test_only=True)), 1
        assert L == len(pset["Q"]) if kind == "bfv" else L < len(pset["Q"])
        self.Q = pset["Q"][:L]
        self.params.AddCRS(0, seed=99)
        self.rng = np.random.default_rng(2029)
        self.sk, self.pk = {}, {}
        for u in EVERYONE:
            self.sk[u], self.pk[u] = kgen.GenKeyPair(u)
        self.cdt = mkrlwe.small_cdt(3.2)
        Qprod = 1
        for q in self.Q:
            Qprod *= q
        self.most = min(1024, (Qprod // (2 * self.Tp)).bit_length() - 1)    # the widest flood the engine takes
        self._ct = {}

    def uniform(self, shape_head):
        return np.stack([self.rng.integers(0, q, tuple(shape_head) + (self.N,), dtype=np.uint64) for q in self.Q], axis=len(shape_head))

    def ct(self, ids, which=0):
        """a uniform ciphertext over ids at L limbs (made once per id set and number) -> (device ciphertext, host copy)"""
        k = (tuple(ids), which)
        if k not in self._ct:
            host = self.uniform((1 + len(ids),))
            self._ct[k] = (self.mk.Ciphertext(self.params, list(ids), self.L - 1).upload(host), host)
        return self._ct[k]

    def q(self):
        return np.array(self.Q, dtype=np.uint64)[:, None]

    def limbs(self, count):
        return self.mk.DeviceLimbs(self.params, count, self.L)

    def samples(self, count, key=KEY, nonce=NONCE):
        """the model's samples of a call in the layout mkhe_encrypt takes: int32 [count][3][N] = (u_b, 0, e1_b); u_b from stream b, e1_b from stream
        count + b"""
        cdt, out = np.array(self.cdt, dtype=np.uint64), np.zeros((count, 3, self.N), dtype=np.int32)
        for b in range(count):
            r = np.array(stream(key, nonce, P.u_stream(count, b), self.N), dtype=np.uint64)
            out[b, 0] = np.where(r & np.uint64(1), 0, np.where(r & np.uint64(2), 1, -1))
            r = np.array(stream(key, nonce, P.e1_stream(count, b), self.N), dtype=np.uint64)
            out[b, 2] = np.searchsorted(cdt, r, side="right") - len(cdt) // 2
        assert out[0, 0, :8].tolist() == P.u_poly(key, nonce, count, 0, 8) and out[0, 2, :8].tolist() == P.e1_poly(key, nonce, count, 0, 8, self.cdt)
        return out

    def flood(self, count, bits, key=KEY, nonce=NONCE, items=None):
        """E_b mod q_j of the model for the items of a call: {b: uint64 [L][N]}"""
        return {b: D.flood_limbs(P.flood_poly(key, nonce, count, b, self.N, bits, values=stream), self.Q) for b in (range(count) if items is None else items)}

    # ---- the raw calls
    def decrypt_share(self, cts, who):
        n = len(cts)
        buf = self.limbs(n)
        assert self.lib.mkhe_decrypt_share(self.params.ctx, n, self.handles([c.h for c in cts]), (C.c_int * n)(*[c.slot(who) for c in cts]),
                                           self.sk[who].Value.devptr(), None, 0, 0, buf.devptr()) == 0, error()
        return buf.download()

    def encrypt_zero(self, recipient, samples):
        """mkhe_encrypt of `count` zero plaintexts under the recipient's key on host samples -> uint64 [count][2][L][N]"""
        n = samples.shape[0]
        d = self.limbs(n).upload(np.zeros((n, self.L, self.N), dtype=np.uint64))
        outs = self.mk.batch_ciphertexts(self.mk.Ciphertext, self.params, [recipient], self.L - 1, n)
        smp = np.ascontiguousarray(samples, dtype=np.int32)
        assert self.lib.mkhe_encrypt(self.params.ctx, self.L - 1, n, self.pk[recipient].Value.devptr(), d.devptr(), 0, smp.ctypes.data_as(C.POINTER(C.c_int32)),
                                     self.handles([c.h for c in outs])) == 0, error()
        return np.stack([c.download() for c in outs])

    def share(self, cts, who, recipient, bits, key=KEY, nonce=NONCE, count=None, slots=None, sk="default", pk="default", out=None, handles="default",
              cdt="default", ncdt=None):
        """mkhe_pcks_share into a buffer of twice the size filled with a sentinel -> (rc, shares uint64 [count][2][L][N]); a refused call leaves
        all of it untouched"""
        n, L = len(cts), self.L
        buf = self.limbs(4 * n).upload(np.full((4 * n, L, self.N), SENTINEL, dtype=np.uint64))
        sl = [c.slot(who) for c in cts] if slots is None else slots
        table = (C.c_uint64 * len(self.cdt))(*self.cdt) if cdt == "default" else cdt
        rc = self.lib.mkhe_pcks_share(self.params.ctx, n if count is None else count, self.handles([c.h for c in cts]) if handles == "default" else handles,
                                      (C.c_int * n)(*sl), self.sk[who].Value.devptr() if sk == "default" else sk,
                                      self.pk[recipient].Value.devptr() if pk == "default" else pk, key_arg(key), nonce, bits,
                                      table, len(self.cdt) if ncdt is None else ncdt, buf.devptr() if out is None else out(buf))
        got = buf.download()
        if rc == 0:
            assert (got[2 * n:] == SENTINEL).all(), "mkhe_pcks_share wrote behind uint64[count][2][L][N]"
        else:
            assert (got == SENTINEL).all(), "a refused mkhe_pcks_share wrote to its output"
        return rc, got[:2 * n].reshape(n, 2, L, self.N)

    def merge(self, cts, shares, recipient="carol", nshares=None, count=None, handles="default", ptrs="default", outs=None, out_list="default"):
        """mkhe_pcks_merge of host share arrays [count][2][L][N] (one per party, slot order) -> (rc, uint64 [count][2][L][N])"""
        n, L = len(cts), self.L
        bufs = [self.limbs(2 * n).upload(np.ascontiguousarray(s).reshape(2 * n, L, self.N)) for s in shares]
        fresh = outs is None
        if fresh:
            outs = [self.mk.Ciphertext(self.params, [recipient], L - 1).upload(np.full((2, L, self.N), SENTINEL, dtype=np.uint64)) for _ in range(n)]
        rc = self.lib.mkhe_pcks_merge(self.params.ctx, n if count is None else count, self.handles([c.h for c in cts]) if handles == "default" else handles,
                                      len(bufs) if nshares is None else nshares,
                                      (self.handles([b.devptr() for b in bufs]) if bufs else None) if ptrs == "default" else ptrs(bufs),
                                      self.handles([c.h for c in outs]) if out_list == "default" else out_list(outs))
        got = [c.download() for c in outs]
        if rc != 0 and fresh:
            assert all((g == SENTINEL).all() for g in got), "a refused mkhe_pcks_merge wrote to its outputs"
        return rc, got

    def decrypt_merge(self, cts, halves):
        """mkhe_decrypt_merge of host arrays [count][L][N] -> uint64 [count][L][N]"""
        n = len(cts)
        bufs = [self.limbs(n).upload(np.ascontiguousarray(s)) for s in halves]
        pt = self.limbs(n)
        assert self.lib.mkhe_decrypt_merge(self.params.ctx, n, self.handles([c.h for c in cts]), len(bufs),
                                           self.handles([b.devptr() for b in bufs]) if bufs else None, pt.devptr()) == 0, error()
        return pt.download()


_worlds = {}


def world(name):
    if name not in _worlds:
        _worlds[name] = World(*RINGS[name])
    return _worlds[name]


@pytest.fixture(scope="module", params=list(RINGS))
def w(request):
    return world(request.param)


@pytest.fixture(scope="module")
def w3():
    return world("three")


def id_sets(who):
    """ciphertexts over 1, 2 and 3 parties that `who` belongs to (test_gpu_decrypt_share.py): its slot differs between them"""
    pair = ["user0", "user1"] if who != "user2" else ["user1", "user2"]
    return [[who], pair, USERS]


def expected(w, plain, enc, flood, b):
    """(h0, h1) of item b from the composition of existing calls and the model's flood"""
    return (plain[b] + enc[b, 0] + flood[b]) % w.q(), enc[b, 1]


def test_the_rings():
    assert world("low").L == 2 and world("low").params.MaxLevel() == 3        # inputs two levels below the maximum: row L + j of pk is a row of pk0
    assert world("low").params.QCount() + world("low").params.PCount() != world("low").L
    assert world("one").L == 1 and world("three").Tp == 65537 and world("low").Tp == 1


# ------------------------------------------------------------------ the share
@pytest.mark.parametrize("recipient", ["carol", "user0"])      # outside the ciphertext's ids, and one of them
@pytest.mark.parametrize("count", [1, 3])
def test_share_is_the_plain_share_plus_an_encryption_of_zero_plus_the_flood(w, count, recipient):
    who = "user1"
    sets = id_sets(who)
    cts = [w.ct(sets[(b + 2) % 3])[0] for b in range(count)]   # different id sets and slots in one call
    assert count < 3 or len({c.slot(who) for c in cts}) > 1
    before = [c.download() for c in cts]
    plain = w.decrypt_share(cts, who)                           # mkhe_decrypt_share, flood_bits = 0
    enc = w.encrypt_zero(recipient, w.samples(count))           # mkhe_encrypt of zero on (u, 0, e1)
    widths = [f for f in BITS if f <= w.most] + [w.most]
    assert len(widths) >= 2
    for bits in widths:
        rc, got = w.share(cts, who, recipient, bits)
        assert rc == 0, error()
        flood = w.flood(count, bits)
        for b in range(count):
            h0, h1 = expected(w, plain, enc, flood, b)
            assert (got[b, 0] == h0).all(), (bits, b, "h0")
            assert (got[b, 1] == h1).all(), (bits, b, "h1")
        if bits:
            E = P.flood_poly(KEY, NONCE, count, 0, w.N, bits, values=stream)
            assert all(-(1 << (bits - 1)) <= v < (1 << (bits - 1)) for v in E) and len(set(E)) > 1
        else:
            assert not flood[0].any()
    assert all((c.download() == x).all() for c, x in zip(cts, before))       # the inputs are left alone


def test_seventeen_items(w3):
    """more items than a kernel-argument table holds: the share needs no table, the merge stages three"""
    w, who, count = w3, "user2", 17
    sets = id_sets(who)
    cts = [w.ct(sets[b % 3], which=b // 3 % 2)[0] for b in range(count)]
    plain = w.decrypt_share(cts, who)
    enc = w.encrypt_zero("carol", w.samples(count))
    rc, got = w.share(cts, who, "carol", 65)
    assert rc == 0, error()
    flood = w.flood(count, 65, items=(0, 1, 16))
    for b in (0, 1, 16):
        h0, h1 = expected(w, plain, enc, flood, b)
        assert (got[b, 0] == h0).all() and (got[b, 1] == h1).all(), b
    shares = [w.uniform((count, 2)) for _ in USERS]
    all3 = [w.ct(USERS, which=b % 2) for b in range(count)]
    rc, out = w.merge([c for c, _ in all3], shares)
    assert rc == 0, error()
    for b in (0, 1, 16):
        assert (out[b] == P.merge(w.Q, all3[b][1][0], [s[b] for s in shares])).all(), b


def test_a_flood_of_twelve_words_on_the_full_chain():
    """the 14 primes of PN15QP880 at N = 2^10: Q has 760 bits and the widest flood 742 -- twelve streams, the top word of 38 bits; and a width
    that ends on a word boundary"""
    w, who = World("bfv", HB.small_bfv(LOGN, 14), 14), "user0"
    assert w.L == 14 and w.most == 742 and P.words(w.most) == 12
    cts = [w.ct(USERS[:2])[0]]
    plain, enc = w.decrypt_share(cts, who), w.encrypt_zero("carol", w.samples(1))
    for bits in (w.most, 704):
        rc, got = w.share(cts, who, "carol", bits)
        assert rc == 0, error()
        E = P.flood_poly(KEY, NONCE, 1, 0, w.N, bits, values=stream)
        assert max(E).bit_length() >= bits - 8 and -min(E) >> (bits - 8)
        h0, h1 = expected(w, plain, enc, {0: D.flood_limbs(E, w.Q)}, 0)
        assert (got[0, 0] == h0).all() and (got[0, 1] == h1).all(), bits
    rc, _ = w.share(cts, who, "carol", w.most + 1)
    assert rc != 0 and "destroys the message" in error()
    shares = [w.uniform((1, 2)) for _ in range(2)]
    item = w.ct(USERS[:2])
    rc, out = w.merge([item[0]], shares)
    assert rc == 0 and (out[0] == P.merge(w.Q, item[1][0], [s[0] for s in shares])).all(), error()
    w.params.close()


def test_share_depends_on_the_nonce_and_the_key(w3):
    w = w3
    cts = [w.ct(USERS)[0]] * 2
    a, b, c, d = (w.share(cts, "user0", "carol", 100, nonce=n, key=k) for n, k in ((1, KEY), (1, KEY), (3, KEY), (1, KEY[::-1])))
    assert all(x[0] == 0 for x in (a, b, c, d)), error()
    assert (a[1] == b[1]).all()                                 # the same key and nonce: the same output
    for other in (c, d):                                        # another nonce, another key: both halves move
        assert (a[1][:, 0] != other[1][:, 0]).mean() > 0.99 and (a[1][:, 1] != other[1][:, 1]).mean() > 0.99
    assert (a[1][0, 0] != a[1][1, 0]).mean() > 0.99 and (a[1][0, 1] != a[1][1, 1]).mean() > 0.99      # items 0 and 1 of one call
    e, f = w.share(cts, "user0", "carol", 100, nonce=1), w.share(cts, "user0", "user1", 100, nonce=1)
    assert (e[1] == a[1]).all() and (f[1][:, 0] != a[1][:, 0]).mean() > 0.99   # and h0 on the recipient's key;
    assert (f[1][:, 1] == a[1][:, 1]).all()                     # h1 = u a + e1 does not: pk1 = a is the common reference string of every key


# ------------------------------------------------------------------ the merge as a pure function
@pytest.mark.parametrize("k", [0, 1, 3])
@pytest.mark.parametrize("count", [1, 3])
def test_merge_is_the_model_and_its_first_half_is_the_merge_of_distributed_decryption(w, count, k):
    ids = USERS[:k]
    items = [w.ct(ids, which=b % 2) for b in range(count)]
    cts = [c for c, _ in items]
    shares = [w.uniform((count, 2)) for _ in ids]
    rc, got = w.merge(cts, shares)
    assert rc == 0, error()
    for b in range(count):
        assert (got[b] == P.merge(w.Q, items[b][1][0], [s[b] for s in shares])).all(), b
    zeroed = [np.stack([s[:, 0], np.zeros_like(s[:, 1])], axis=1) for s in shares]           # h1 = 0
    rc, got = w.merge(cts, zeroed)
    assert rc == 0, error()
    pt = w.decrypt_merge(cts, [s[:, 0] for s in shares])
    for b in range(count):
        assert (got[b][0] == pt[b]).all() and not got[b][1].any(), b
    assert all((c.download() == h).all() for c, h in items)


# ------------------------------------------------------------------ refusals
def good_call(w):
    """the context works: a share and its merge of one party's ciphertext"""
    c, host = w.ct(["user0"])
    rc, sh = w.share([c], "user0", "carol", 20)
    assert rc == 0, error()
    rc, got = w.merge([c], [sh])
    assert rc == 0 and (got[0] == P.merge(w.Q, host[0], [sh[0]])).all(), error()


def test_share_refusals(w3):
    w = w3
    c3, c2 = w.ct(USERS)[0], w.ct(USERS[:2])[0]
    low = w.mk.Ciphertext(w.params, USERS, 0)

    def refused(text, cts=(c3,), who="user1", bits=100, **kw):
        rc, _ = w.share(list(cts), who, "carol", bits, **kw)
        assert rc != 0 and error().startswith("mkhe_pcks_share: ") and text in error() and not any("%08x" % x in error().lower() for x in KEY), error()
        good_call(w)

    refused("flood_bits", bits=-1)
    refused("flood_bits", bits=1025)
    refused("destroys the message", bits=w.most + 1)
    refused("null key", key=None)
    refused("null key", key=None, bits=0)
    refused("slot out of range", slots=[0])
    refused("slot out of range", slots=[4])
    refused("slot out of range", cts=(c3, c2), slots=[3, 3])
    refused("nQ limbs", cts=(c3, low))
    refused("aligned", out=lambda buf: C.c_void_p(buf.devptr().value + 8))
    refused("aligned", sk=C.c_void_p(w.sk["user1"].Value.devptr().value + 8))
    refused("aligned", pk=C.c_void_p(w.pk["carol"].Value.devptr().value + 8))
    refused("null", sk=None)
    refused("null", pk=None)
    refused("null", out=lambda buf: None)
    refused("null", handles=None)
    refused("null", handles=w.handles([None]))
    refused("null table", cdt=None)
    refused("ncdt", ncdt=3)
    refused("ncdt", ncdt=0)
    refused("ncdt", ncdt=66)
    refused("count", count=0)
    refused("count", count=65536)
    assert w.lib.mkhe_pcks_share(None, 1, None, None, None, None, key_arg(), 0, 1, None, 0, None) != 0 and error() == "mkhe_pcks_share: null context"
    rc, _ = w.share([c3], "user1", "carol", w.most)            # the widest flood
    assert rc == 0, error()


def test_share_refuses_inputs_at_different_levels_and_a_flood_wider_than_their_level():
    w = world("low")
    c, other = w.ct(USERS)[0], w.mk.Ciphertext(w.params, USERS, 0)
    rc, _ = w.share([c, other], "user1", "carol", 20)
    assert rc != 0 and error().startswith("mkhe_pcks_share: ") and "same level" in error()
    good_call(w)
    assert w.most < 128                                         # two of the four primes: the bound follows the level of the input, not the context
    rc, _ = w.share([c], "user1", "carol", w.most + 1)
    assert rc != 0 and "destroys the message" in error() and str(w.most) in error()
    good_call(w)


def test_merge_refusals(w3):
    w = w3
    c3, other, c2 = w.ct(USERS)[0], w.ct(USERS, which=1)[0], w.ct(USERS[:2])[0]
    low = w.mk.Ciphertext(w.params, USERS, 0)
    one, two = np.zeros((1, 2, w.L, w.N), dtype=np.uint64), np.zeros((2, 2, w.L, w.N), dtype=np.uint64)
    new = lambda ids, lvl: w.mk.Ciphertext(w.params, ids, lvl)

    def refused(text, cts=(c3,), shares=(one, one, one), **kw):
        rc, _ = w.merge(list(cts), list(shares), **kw)
        assert rc != 0 and error().startswith("mkhe_pcks_merge: ") and text in error(), error()
        good_call(w)

    refused("nQ limbs", cts=(c3, low), shares=(two, two, two))
    refused("same ids", cts=(c3, c2), shares=(two, two, two))
    refused("nshares", shares=(one, one))
    refused("nshares", nshares=-1)
    refused("aligned", ptrs=lambda bufs: w.handles([bufs[0].devptr(), C.c_void_p(bufs[1].devptr().value + 8), bufs[2].devptr()]))
    refused("null", ptrs=lambda bufs: w.handles([bufs[0].devptr(), None, bufs[2].devptr()]))
    refused("null", ptrs=lambda bufs: None)
    refused("null", handles=None)
    refused("null", out_list=lambda outs: None)
    refused("null", out_list=lambda outs: w.handles([None]))
    refused("count", count=0)
    refused("count", count=65536)
    refused("exactly one id", outs=[new(USERS[:2], w.L - 1)])
    refused("exactly one id", outs=[new([], w.L - 1)])
    refused("limbs of the inputs", outs=[new(["carol"], 1)])
    refused("distinct", cts=(c3, other), shares=(two, two, two), outs=[new(["carol"], w.L - 1)] * 2)
    solo = w.ct(["user0"])[0]
    keep = solo.download()
    refused("aliases an input", cts=(solo,), shares=(one,), outs=[solo])
    assert (solo.download() == keep).all()
    assert w.lib.mkhe_pcks_merge(None, 1, None, 0, None, None) != 0 and error() == "mkhe_pcks_merge: null context"
    rc, _ = w.merge([c3, other], [two, two, two])               # two ciphertexts over the same ids: accepted
    assert rc == 0, error()
    rc, got = w.merge([c3], [one, one, one], recipient="user1") # the recipient may be one of the parties
    assert rc == 0 and not got[0][1].any(), error()


def test_merge_refuses_inputs_at_different_levels():
    w = world("low")
    c, other = w.ct(USERS)[0], w.mk.Ciphertext(w.params, USERS, 0)
    two = np.zeros((2, 2, w.L, w.N), dtype=np.uint64)
    rc, _ = w.merge([c, other], [two, two, two])
    assert rc != 0 and error().startswith("mkhe_pcks_merge: ") and "same level" in error()
    rc, _ = w.merge([c], [two[:1]] * 3, outs=[w.mk.Ciphertext(w.params, ["carol"], w.params.MaxLevel())])
    assert rc != 0 and "limbs of the inputs" in error()
    good_call(w)


def test_refused_on_a_context_that_owns_a_subset_of_the_moduli():
    w = world("low")
    c, _ = w.ct(["user0"])
    own = (C.c_int * 2)(0, 2)
    assert w.lib.mkhe_ctx_set_owned(w.params.ctx, own, 2) == 0, error()
    try:
        rc, _ = w.share([c], "user0", "carol", 50)
        assert rc != 0 and error().startswith("mkhe_pcks_share: ") and "subset of the moduli" in error()
        rc, _ = w.merge([c], [np.zeros((1, 2, w.L, w.N), dtype=np.uint64)])
        assert rc != 0 and error().startswith("mkhe_pcks_merge: ") and "subset of the moduli" in error()
    finally:
        assert w.lib.mkhe_ctx_set_owned(w.params.ctx, own, 0) == 0
    good_call(w)


def test_share_refused_inside_a_capture(w3):
    """(where the runtime of this process can capture at all: tests/test_gpu_cnn.py)"""
    from mkhe_kklss_amd._abi import MkheError
    w = w3
    c, _ = w.ct(["user0"])
    cdt = (C.c_uint64 * len(w.cdt))(*w.cdt)
    buf = w.limbs(2).upload(np.full((2, w.L, w.N), SENTINEL, dtype=np.uint64))
    try:
        with w.params.Capture():
            rc = w.lib.mkhe_pcks_share(w.params.ctx, 1, w.handles([c.h]), (C.c_int * 1)(1), w.sk["user0"].Value.devptr(), w.pk["carol"].Value.devptr(),
                                       key_arg(), 1, 20, cdt, len(w.cdt), buf.devptr())
            msg = error()
        assert rc != 0 and msg.startswith("mkhe_pcks_share: ") and "capture" in msg
        print("capture: the share was refused inside a capture")
    except MkheError as e:
        print("capture: mkhe_capture_begin refused in this process (%s): the refusal inside a capture did not run" % e)
        import gc
        gc.enable()                 # (Graph.__enter__ switched the collector off before the refusal)
        assert "cannot end a multi-stream capture" in str(e)
    assert (buf.download() == SENTINEL).all()
    good_call(w)
