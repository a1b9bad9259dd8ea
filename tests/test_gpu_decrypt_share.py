"""Distributed decryption on the device (-m gpu): mkhe_decrypt_share and mkhe_decrypt_merge against tests/decrypt_share_model.py, bit for bit,
on H.small_ckks(logN, 3) and HB.small_bfv(10, 3); the two identities of include/mkhe.h (the merge of unflooded shares is mkhe_decrypt; a
flooded share differs from the unflooded one by e mod q_j of one integer e); every refusal followed by a call that works; and the mirrors
end to end.  The ciphertexts of the parity tests are uniform polynomials: both identities hold for any ciphertext."""
import ctypes as C
import types

import numpy as np
import pytest

import decrypt_share_model as D
import device_sampler_model as M
import harness as H
import harness_bfv as HB
from oracle import oracle as O
from scenario import Scenario

pytestmark = pytest.mark.gpu

KEY = [0x9E3779B9, 0x7F4A7C15, 0xF39CC060, 0x5CEDC834, 0x1082276B, 0xF3A27251, 0xF86C6A11, 0xD0C18E95]
NONCE = 0xFEDCBA9876543210
SENTINEL = 0x7B7B7B7B7B7B7B7B
BITS = [0, 1, 32, 33, 62]
USERS = ["user0", "user1", "user2"]
BFV = HB.small_bfv(10, 3)


def key_arg(key=KEY):
    return None if key is None else (C.c_uint32 * 8)(*key)


def error():
    from mkhe_kklss_amd._abi import lib
    return lib().mkhe_last_error().decode()


class World:
    """a context, three parties with keys made on it, their secrets on the host for the model, and the raw calls"""

    def __init__(self, params, Q, P, mod=None):
        from mkhe_kklss_amd import mkrlwe
        from mkhe_kklss_amd._abi import handle_array, lib
        self.mk, self.lib, self.handles, self.params, self.N, self.nq = mkrlwe, lib(), handle_array, params, params.N(), len(Q)
        self.ks = O.KeySwitcher(params.LogN(), Q, P, 2)
        self.rng = np.random.default_rng(self.N + self.nq)
        params.AddCRS(0, seed=99)
        kgen = (mod or mkrlwe).NewKeyGenerator(params, mkrlwe.HostSampler(np.random.default_rng(7), insecure_test_only=True))
        self.sk = {u: kgen.GenSecretKey(u) for u in USERS}
        self.sk_host = {u: self.sk[u].Value.download()[0] for u in USERS}
        self._r, self._ct = {}, {}

    def ct(self, ids, level, which=0):
        """a uniform ciphertext over ids at level (made once per shape and number) -> (device ciphertext, host copy)"""
        k = (tuple(ids), level, which)
        if k not in self._ct:
            host = H.uniform_ct(self.rng, self.ks, len(ids), level + 1)
            self._ct[k] = (self.mk.Ciphertext(self.params, list(ids), level).upload(host), host)
        return self._ct[k]

    def r(self, stream):
        """the 64-bit values of stream `stream` of (KEY, NONCE), computed once"""
        if stream not in self._r:
            self._r[stream] = np.array(M.stream_values(KEY, NONCE, stream, self.N), dtype=np.uint64)
        return self._r[stream]

    def e(self, stream, bits):
        """kind 2 as int64 [N] (numpy restatement of decrypt_share_model.flood_value, checked against it on the first block)"""
        if bits == 0:
            return np.zeros(self.N, dtype=np.int64)
        e = (self.r(stream) >> np.uint64(64 - bits)).astype(np.int64) - np.int64(1 << (bits - 1))
        assert [int(v) for v in e[:8]] == D.flood_poly(KEY, NONCE, stream, 8, bits)
        return e

    def e_mod(self, stream, bits, level):
        return np.stack([np.mod(self.e(stream, bits), np.int64(q)).astype(np.uint64) for q in self.ks.Q[: level + 1]])

    def q(self, level):
        return np.array(self.ks.Q[: level + 1], dtype=np.uint64)[:, None]

    def share(self, cts, who, bits, nonce=NONCE, key=KEY, count=None, slots=None, sk="default", out=None, handles="default"):
        """mkhe_decrypt_share into a buffer of twice the size filled with a sentinel -> (rc, uint64 [count][L][N]); what lies behind stays untouched"""
        n, L = len(cts), cts[0].Level() + 1
        buf = self.mk.DeviceLimbs(self.params, 2 * n, L).upload(np.full((2 * n, L, self.N), SENTINEL, dtype=np.uint64))
        sl = [c.slot(who) for c in cts] if slots is None else slots
        rc = self.lib.mkhe_decrypt_share(self.params.ctx, n if count is None else count, self.handles([c.h for c in cts]) if handles == "default" else handles,
                                         (C.c_int * n)(*sl), self.sk[who].Value.devptr() if sk == "default" else sk, key_arg(key), nonce, bits,
                                         buf.devptr() if out is None else out(buf))
        got = buf.download()
        if rc == 0:
            assert (got[n:] == SENTINEL).all(), "mkhe_decrypt_share wrote behind uint64[count][limbs][N]"
        else:
            assert (got == SENTINEL).all(), "a refused mkhe_decrypt_share wrote to its output"
        return rc, got[:n]

    def merge(self, cts, shares, nshares=None, count=None, out=None, handles="default", ptrs="default"):
        """mkhe_decrypt_merge of host share arrays [count][L][N] (one per party, slot order) -> (rc, uint64 [count][L][N])"""
        n, L = len(cts), cts[0].Level() + 1
        bufs = [self.mk.DeviceLimbs(self.params, n, L).upload(s) for s in shares]
        pt = self.mk.DeviceLimbs(self.params, 2 * n, L).upload(np.full((2 * n, L, self.N), SENTINEL, dtype=np.uint64))
        rc = self.lib.mkhe_decrypt_merge(self.params.ctx, n if count is None else count, self.handles([c.h for c in cts]) if handles == "default" else handles,
                                         len(bufs) if nshares is None else nshares, self.handles([b.devptr() for b in bufs]) if ptrs == "default" else ptrs(bufs),
                                         pt.devptr() if out is None else out(pt))
        got = pt.download()
        if rc == 0:
            assert (got[n:] == SENTINEL).all(), "mkhe_decrypt_merge wrote behind uint64[count][limbs][N]"
        else:
            assert (got == SENTINEL).all(), "a refused mkhe_decrypt_merge wrote to its output"
        return rc, got[:n]

    def decrypt(self, ct):
        pt = self.mk.DeviceLimbs(self.params, 1, ct.Level() + 1)
        assert self.lib.mkhe_decrypt(self.params.ctx, ct.h, self.handles([self.sk[u].Value.devptr() for u in ct.ids]), pt.devptr()) == 0, error()
        return pt.download()[0]

    def product(self, host, ct, who):
        """the model's unflooded share of `who` for one ciphertext"""
        return D.product(self.ks, host[ct.slot(who)], self.sk_host[who])


@pytest.fixture(scope="module")
def worlds():
    from mkhe_kklss_amd import mkrlwe
    w = {}

    def get(logN):
        if logN not in w:
            pset = H.small_ckks(logN, 3)
            w[logN] = World(mkrlwe.Parameters(pset["logN"], pset["Q"], pset["P"]), pset["Q"], pset["P"])
        return w[logN]
    return get


@pytest.fixture(scope="module")
def ck(worlds):
    return worlds(10)


@pytest.fixture(scope="module")
def bf():
    from mkhe_kklss_amd import mkbfv
    return World(mkbfv.Parameters(BFV["logN"], BFV["Q"], BFV["QMul"], BFV["P"], BFV["T"]), BFV["Q"], BFV["P"], mkbfv)


def id_sets(who):
    """ciphertexts over 1, 2 and 3 parties that `who` belongs to: its slot is the first (user0), the last of two and the middle of three
    (user1), the last (user2)"""
    pair = ["user0", "user1"] if who != "user2" else ["user1", "user2"]
    return [[who], pair, USERS]


def check_shares(w, level, who, items, bits_list=BITS):
    """items: (device ciphertext, host copy) per item of the batch; every width in bits_list against the model, and against the unflooded share"""
    cts = [c for c, _ in items]
    before = [c.download() for c in cts]
    plain = np.stack([w.product(h, c, who) for c, h in items])
    for bits in bits_list:
        rc, got = w.share(cts, who, bits, key=KEY if bits else None)        # bits = 0: the key may be NULL
        assert rc == 0, error()
        for b in range(len(cts)):
            em = w.e_mod(b, bits, level)
            assert (got[b] == (plain[b] + em) % w.q(level)).all(), (bits, b)
            diff = (got[b] + w.q(level) - plain[b]) % w.q(level)              # share - share|0 = e mod q_j
            assert (diff == em).all()
            if bits and all((1 << (bits - 1)) < q // 2 for q in w.ks.Q[: level + 1]):
                lifts = [D.centred(diff[j][:64], q) for j, q in enumerate(w.ks.Q[: level + 1])]
                assert all(l == [int(v) for v in w.e(b, bits)[:64]] for l in lifts)          # the same centred integer in every limb
    assert all((c.download() == x).all() for c, x in zip(cts, before))       # the inputs are left alone
    return plain


# ------------------------------------------------------------------ shares against the model
@pytest.mark.parametrize("who", USERS)
@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("logN", [10, 12])                     # N / 8 = 128 blocks: one workgroup; 512: four
def test_share_equals_the_model(worlds, logN, level, who):
    w = worlds(logN)
    check_shares(w, level, who, [w.ct(ids, level) for ids in id_sets(who)])


@pytest.mark.parametrize("count", [1, 17])                     # 17 > ED_INLINE: the staged pointer tables
@pytest.mark.parametrize("level", [0, 2])
def test_share_counts_and_separate_streams(ck, level, count):
    items = [ck.ct(USERS, level, which=b % 4) for b in range(count)]         # four ciphertexts, each at several items
    check_shares(ck, level, "user1", items, bits_list=[0, 33])
    if count > 4:
        rc, got = ck.share([c for c, _ in items], "user1", 33)
        assert rc == 0, error()
        q = ck.q(level)
        for b, b2 in ((0, 4), (1, 13), (4, 16)):                            # the same ciphertext at items b and b': the shares differ by e_b - e_b'
            want = (ck.e_mod(b, 33, level) + q - ck.e_mod(b2, 33, level)) % q
            assert ((got[b] + q - got[b2]) % q == want).all() and want.any()


def test_share_of_more_items_than_one_transform_launch(ck):
    """65 items: the gathering forward transform takes 64 per launch.  Unflooded, so that item b is what the call on its ciphertext alone gives"""
    level, count = 1, 65
    items = [ck.ct(USERS, level, which=b % 4) for b in range(count)]
    alone = []
    for b in range(4):
        rc, got = ck.share([items[b][0]], "user1", 0, key=None)
        assert rc == 0, error()
        alone.append(got[0])
        assert (got[0] == ck.product(items[b][1], items[b][0], "user1")).all()
    rc, got = ck.share([c for c, _ in items], "user1", 0, key=None)
    assert rc == 0, error()
    for b in range(count):
        assert (got[b] == alone[b % 4]).all(), b


@pytest.mark.parametrize("who", ["user0", "user2"])
def test_share_on_a_bfv_context(bf, who):
    level = bf.nq - 1
    check_shares(bf, level, who, [bf.ct(ids, level) for ids in id_sets(who)], bits_list=[0, 62])


def test_nonce_and_key_decide_the_flood(ck):
    level = 2
    cts = [ck.ct(USERS, level)[0]] * 2
    a, b, c, d = (ck.share(cts, "user0", 32, nonce=n, key=k) for n, k in ((NONCE, KEY), (NONCE, KEY), (NONCE + 1, KEY), (NONCE, KEY[::-1])))
    assert a[0] == 0 and b[0] == 0 and c[0] == 0 and d[0] == 0, error()
    assert (a[1] == b[1]).all()                                # the same (key, nonce): the same shares
    assert (a[1] != c[1]).mean() > 0.99 and (a[1] != d[1]).mean() > 0.99     # the next nonce, another key
    assert (a[1][0] != a[1][1]).mean() > 0.99                  # items 0 and 1 of one call


# ------------------------------------------------------------------ the merge
@pytest.mark.parametrize("count", [1, 3, 17])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_merge_of_unflooded_shares_is_decrypt(ck, k, count):
    level = 2 if count != 3 else 1
    ids = USERS[:k]
    items = [ck.ct(ids, level, which=b % 3) for b in range(count)]
    cts = [c for c, _ in items]
    shares = []
    for u in ids:
        rc, s = ck.share(cts, u, 0, key=None)
        assert rc == 0, error()
        shares.append(s)
    rc, got = ck.merge(cts, shares)
    assert rc == 0, error()
    want = [ck.decrypt(c) for c in cts[:3]]
    assert all((got[b] == want[b % 3]).all() for b in range(count))                         # mkhe_decrypt, bit for bit
    assert (got == np.stack([D.merge(ck.ks, h[0], [s[b] for s in shares]) for b, (_, h) in enumerate(items)])).all()
    rc, rev = ck.merge(cts, shares[::-1])
    assert rc == 0 and (rev == got).all()                       # shares commute
    assert all((c.download() == h).all() for c, h in items[:3])


@pytest.mark.parametrize("logN,level", [(10, 0), (12, 2)])
def test_merge_of_flooded_shares_adds_the_sum_of_the_floods(worlds, logN, level):
    w = worlds(logN)
    items = [w.ct(USERS, level, which=b) for b in range(2)]
    cts, q = [c for c, _ in items], w.q(level)
    shares, total = [], np.zeros((2, level + 1, w.N), dtype=np.uint64)
    for u, bits in zip(USERS, (62, 33, 1)):                     # (every party would use its own key: here one key, so that the model's streams serve)
        rc, s = w.share(cts, u, bits)
        assert rc == 0, error()
        shares.append(s)
        total = (total + np.stack([w.e_mod(b, bits, level) for b in range(2)])) % q
    rc, got = w.merge(cts, shares)
    assert rc == 0, error()
    for b, c in enumerate(cts):
        assert (got[b] == (w.decrypt(c) + total[b]) % q).all()


def test_merge_without_parties_reduces_c0(ck):
    level = 1
    c, host = ck.ct([], level)
    rc, got = ck.merge([c], [])
    assert rc == 0, error()
    assert (got[0] == host[0]).all() and (got[0] == ck.decrypt(c)).all()


def test_merge_on_a_bfv_context(bf):
    level = bf.nq - 1
    c, _ = bf.ct(USERS[:2], level)
    shares = [bf.share([c], u, 0, key=None)[1] for u in USERS[:2]]
    rc, got = bf.merge([c], shares)
    assert rc == 0 and (got[0] == bf.decrypt(c)).all(), error()


# ------------------------------------------------------------------ refusals
def good_call(w):
    """the context works: a share and a merge against mkhe_decrypt"""
    c, _ = w.ct(USERS[:2], 1)
    shares = [w.share([c], u, 0, key=None)[1] for u in USERS[:2]]
    rc, got = w.merge([c], shares)
    assert rc == 0 and (got[0] == w.decrypt(c)).all(), error()


def test_decrypt_share_refusals(ck):
    level = 2
    c3, c2, low = ck.ct(USERS, level)[0], ck.ct(USERS[:2], level)[0], ck.ct(USERS, 1)[0]

    def refused(text, cts=(c3,), who="user1", bits=30, **kw):
        rc, _ = ck.share(list(cts), who, bits, **kw)
        assert rc != 0 and error().startswith("mkhe_decrypt_share: ") and text in error() and not any("%08x" % x in error().lower() for x in KEY), error()
        good_call(ck)

    refused("flood_bits", bits=-1)
    refused("flood_bits", bits=63)
    refused("null key", key=None)
    refused("slot out of range", slots=[0])
    refused("slot out of range", slots=[4])
    refused("slot out of range", cts=(c3, c2), slots=[3, 3])
    refused("same level", cts=(c3, low))
    refused("aligned", out=lambda buf: C.c_void_p(buf.devptr().value + 8))
    refused("aligned", sk=C.c_void_p(ck.sk["user1"].Value.devptr().value + 8))
    refused("null", sk=None)
    refused("null", out=lambda buf: None)
    refused("null", handles=None)
    refused("count", count=0)
    refused("count", count=65536)
    assert ck.lib.mkhe_decrypt_share(None, 1, None, None, None, None, 0, 0, None) != 0 and error() == "mkhe_decrypt_share: null context"


def test_decrypt_merge_refusals(ck):
    level = 2
    c3, other, low = ck.ct(USERS, level)[0], ck.ct(USERS, level, which=1)[0], ck.ct(USERS, 1)[0]
    c2 = ck.ct(USERS[:2], level)[0]
    one = np.zeros((1, level + 1, ck.N), dtype=np.uint64)
    two = np.zeros((2, level + 1, ck.N), dtype=np.uint64)

    def refused(text, cts=(c3,), shares=(one, one, one), **kw):
        rc, _ = ck.merge(list(cts), list(shares), **kw)
        assert rc != 0 and error().startswith("mkhe_decrypt_merge: ") and text in error(), error()
        good_call(ck)

    refused("same level", cts=(c3, low), shares=(two, two, two))
    refused("same ids", cts=(c3, c2), shares=(two, two, two))
    refused("nshares", shares=(one, one))
    refused("nshares", shares=(one, one, one, one))
    refused("nshares", nshares=-1)
    refused("aligned", out=lambda pt: C.c_void_p(pt.devptr().value + 8))
    refused("aligned", ptrs=lambda bufs: ck.handles([bufs[0].devptr(), C.c_void_p(bufs[1].devptr().value + 8), bufs[2].devptr()]))
    refused("null", ptrs=lambda bufs: ck.handles([bufs[0].devptr(), None, bufs[2].devptr()]))
    refused("null", ptrs=lambda bufs: None)
    refused("null", out=lambda pt: None)
    refused("null", handles=None)
    refused("count", count=0)
    assert ck.lib.mkhe_decrypt_merge(None, 1, None, 0, None, None) != 0 and error() == "mkhe_decrypt_merge: null context"
    rc, got = ck.merge([c3, other], [two, two, two])           # two ciphertexts over the same ids: accepted
    assert rc == 0, error()


def test_refused_on_a_context_that_owns_a_subset_of_the_moduli(ck):
    pset = H.small_ckks(10, 3)
    c, _ = ck.ct(USERS[:2], 2)
    one = np.zeros((1, 3, ck.N), dtype=np.uint64)
    own = (C.c_int * 3)(0, 2, len(pset["Q"]) + len(pset["P"]) - 1)
    assert ck.lib.mkhe_ctx_set_owned(ck.params.ctx, own, 3) == 0, error()
    try:
        for bits, key in ((30, KEY), (0, None)):
            rc = ck.lib.mkhe_decrypt_share(ck.params.ctx, 1, ck.handles([c.h]), (C.c_int * 1)(1), ck.sk["user0"].Value.devptr(), key_arg(key), 0, bits,
                                           ck.mk.DeviceLimbs(ck.params, 1, 3).devptr())
            assert rc != 0 and error().startswith("mkhe_decrypt_share: ") and "subset of the moduli" in error()
        bufs = [ck.mk.DeviceLimbs(ck.params, 1, 3).upload(one) for _ in range(2)]
        rc = ck.lib.mkhe_decrypt_merge(ck.params.ctx, 1, ck.handles([c.h]), 2, ck.handles([b.devptr() for b in bufs]), ck.mk.DeviceLimbs(ck.params, 1, 3).devptr())
        assert rc != 0 and error().startswith("mkhe_decrypt_merge: ") and "subset of the moduli" in error()
    finally:
        assert ck.lib.mkhe_ctx_set_owned(ck.params.ctx, own, 0) == 0
    good_call(ck)


def test_flooded_share_refused_inside_a_capture(ck):
    """(where the runtime of this process can capture at all: tests/test_gpu_cnn.py)"""
    from mkhe_kklss_amd._abi import MkheError
    c, _ = ck.ct(USERS[:2], 2)
    out = ck.mk.DeviceLimbs(ck.params, 1, 3).upload(np.full((1, 3, ck.N), SENTINEL, dtype=np.uint64))
    try:
        with ck.params.Capture():
            rc = ck.lib.mkhe_decrypt_share(ck.params.ctx, 1, ck.handles([c.h]), (C.c_int * 1)(1), ck.sk["user0"].Value.devptr(), key_arg(), 0, 30, out.devptr())
            msg = error()
        assert rc != 0 and msg.startswith("mkhe_decrypt_share: ") and "capture" in msg
        print("capture: the flooded share was refused inside a capture")
    except MkheError as e:
        print("capture: mkhe_capture_begin refused in this process (%s): the refusal inside a capture did not run" % e)
        import gc
        gc.enable()                 # (Graph.__enter__ switched the collector off before the refusal)
        assert "cannot end a multi-stream capture" in str(e)
    assert (out.download() == SENTINEL).all()
    good_call(ck)


# ------------------------------------------------------------------ the mirrors, end to end
def _max_err(a, b):
    d = np.abs(np.asarray(a) - np.asarray(b))
    return float(max(d.real.max(), d.imag.max()))


@pytest.mark.parametrize("encoder", ["host", "device"])
@pytest.mark.parametrize("logN", [10, 11])
def test_mkckks_two_parties_end_to_end(logN, encoder):
    """every party shares under its own DeviceSampler; the shares travel as host arrays.  Tolerance, derived: Scenario.precision_bound with the 8
    extra bits of an encrypt / decrypt round trip (test_gpu_ckks_device_e2e.py) for each of the two summands, plus N k 2^(bits-1) / scale for the flood."""
    from mkhe_kklss_amd import mkckks, mkrlwe
    pset, bits = H.small_ckks(logN, 4), 30
    params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], pset["scale"])
    params.GenDefaultCRS(seed=4321)
    kgen = mkrlwe.NewKeyGenerator(params, mkrlwe.HostSampler(np.random.default_rng(2024), insecure_test_only=True))
    enc, dec, ev = mkckks.NewEncryptor(params, sampler=mkrlwe.DeviceSampler(), encoder=encoder), mkckks.NewDecryptor(params, encoder=encoder), mkckks.NewEvaluator(params)
    names, rng, n = ["user0", "user1"], np.random.default_rng(17), 1 << (logN - 1)
    sks, samplers, zs, ct = {}, {}, {}, None
    for p in names:
        sks[p], pk = kgen.GenKeyPair(p)
        samplers[p] = mkrlwe.DeviceSampler()
        zs[p] = np.full(n, complex(0.1 / 2, 1.0 / 2)) + rng.uniform(-0.05, 0.05, n)
        c = enc.EncryptMsgNew(mkckks.Message(zs[p]), pk)
        ct = c if ct is None else ev.AddNew(ct, c)
    wire = []
    for p in names:
        sh = dec.ShareNew(ct, sks[p], bits, samplers[p])
        assert samplers[p].counter == 1 and sh.ID == p and sh.Level() == ct.Level()
        wire.append((p, sh.Level(), sh.download()))
    shares = [mkrlwe.DecryptionShare(params, p, lvl, 1).upload(host) for p, lvl, host in reversed(wire)]
    got = dec.MergeSharesMsg(ct, shares).Value
    flood = dec.FloodSlotBound(2, bits, pset["scale"])
    assert flood == (1 << logN) * 2 * 2.0 ** (bits - 1) / pset["scale"]
    tol = 2 * 2.0 ** Scenario.precision_bound(types.SimpleNamespace(scale=pset["scale"], logN=logN), 8) + flood
    err = _max_err(got, zs["user0"] + zs["user1"])
    print("logN %d, %s encoder: error %.3g, tolerance %.3g (flood term %.3g)" % (logN, encoder, err, tol, flood))
    assert err <= tol
    skSet = mkrlwe.NewSecretKeySet()
    for p in names:
        skSet.AddSecretKey(sks[p])
    assert _max_err(got, dec.Decrypt(ct, skSet).Value) <= flood + 2.0 ** -40                # against Decrypt only the flood (and the decoder's rounding)
    params.close()


def test_mkbfv_two_parties_end_to_end_is_exact():
    from mkhe_kklss_amd import mkbfv, mkrlwe
    T, N, bits = BFV["T"], 1 << BFV["logN"], 62
    params = mkbfv.Parameters(BFV["logN"], BFV["Q"], BFV["QMul"], BFV["P"], T)
    params.GenDefaultCRS(seed=777)
    kgen = mkbfv.NewKeyGenerator(params, mkrlwe.HostSampler(np.random.default_rng(31), insecure_test_only=True))
    for encoder in ("host", "device"):
        enc, dec, ev = mkbfv.NewEncryptor(params, sampler=mkrlwe.DeviceSampler(), encoder=encoder), mkbfv.NewDecryptor(params, encoder=encoder), mkbfv.NewEvaluator(params)
        assert bits <= dec.MaxFloodBits(2)                      # 2 * 2^61 <= Q / (4 T): the message must come out exact
        rng, sks, ms, ct = np.random.default_rng(5), {}, {}, None
        for p in ("user0", "user1"):
            sks[p], pk = kgen.GenKeyPair(p)
            ms[p] = rng.integers(-(T // 4), T // 4, N).astype(np.int64)
            c = enc.EncryptMsgNew(mkbfv.Message(ms[p]), pk)
            ct = c if ct is None else ev.AddNew(ct, c)
        shares = [dec.ShareNew(ct, sks[p], bits, mkrlwe.DeviceSampler()) for p in ("user1", "user0")]
        moved = [mkrlwe.DecryptionShare(params, s.ID, s.Level(), 1).upload(s.download()) for s in shares]
        assert (dec.MergeSharesMsg(ct, moved).Value == ms["user0"] + ms["user1"]).all()
    params.close()
