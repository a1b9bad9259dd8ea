"""The threshold secret keys on the device (-m gpu), N = 2^10, bit for bit against tests/threshold_model.py: mkhe_threshold_gen_shares for seven
(t, n) that put n on, one above and twice-plus-one above every point-group size a kernel might have; mkhe_threshold_additive_key, also in place;
the Reconstruct identity for every t-subset; linearity through mkhe_decrypt_share and mkhe_decrypt_merge; mkhe_limbs_sum against numpy across the
inline / staged boundary of its pointer table; every refusal followed by a call that works.  Three rings: the three-prime BFV chain, one limb, and
the 4-prime mkrlwe context (inputs below the maximum level, so that limbs != nQ != R); once the 14 + 2 rows of PN15QP880 at N = 2^15, and once a
context with the modulus 65537, which a uint32 point can exceed.  The end-to-end tests on mkckks and mkbfv are tests/test_gpu_threshold_e2e.py."""
import ctypes as C
import itertools

import numpy as np
import pytest

import harness as H
import harness_bfv as HB
import sk_encrypt_model as SK
import threshold_model as T

pytestmark = pytest.mark.gpu

KEY = [0x9E3779B9, 0x7F4A7C15, 0xF39CC060, 0x5CEDC834, 0x1082276B, 0xF3A27251, 0xF86C6A11, 0xD0C18E95]
NONCE = 0xFEDCBA9876543210
SENTINEL = 0x7B7B7B7B7B7B7B7B               # above every modulus: no canonical word equals it
LOGN = 10
RINGS = {"three": ("bfv", HB.small_bfv(LOGN, 3), 3), "one": ("bfv", HB.small_bfv(LOGN, 1), 1), "low": ("rlwe", H.small_ckks(LOGN, 4), 2)}
# 1, 2^32 - 1 and non-consecutive values first; 32 pairwise distinct points in all
POINTS = [1, 4294967295, 7, 1000003, 2, 65537, 4294967294, 99] + [3 * i * i + 11 for i in range(1, 25)]
SHAPES = [(1, 1), (2, 3), (3, 4), (3, 5), (5, 5), (4, 9), (2, 32)]
assert len(set(POINTS)) == 32 and all(1 <= x < 1 << 32 for x in POINTS)


def key_arg(key=KEY):
    return None if key is None else (C.c_uint32 * 8)(*key)


def error():
    from mkhe_kklss_amd._abi import lib
    return lib().mkhe_last_error().decode()


_streams = {}


def stream(key, nonce, s, n):
    """the 64-bit values of one stream (numpy keystream, pinned to the integer model by tests/test_sk_encrypt_model.py), computed once per module"""
    k = (tuple(key), nonce, s, n)
    if k not in _streams:
        _streams[k] = SK.stream_values_np(key, nonce, s, n)
    return _streams[k]


class World:
    """a context over one ring, two parties with secret keys made on it, and the raw calls"""

    def __init__(self, kind, pset, L, keygen=True):
        from mkhe_kklss_amd import mkbfv, mkrlwe
        from mkhe_kklss_amd._abi import handle_array, lib
        self.mk, self.lib, self.handles, self.N, self.L, self.kind = mkrlwe, lib(), handle_array, 1 << pset["logN"], L, kind
        sampler = mkrlwe.HostSampler(np.random.default_rng(11), insecure_test_only=True)
        if kind == "bfv":
            self.params = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], pset["T"])
            kgen = mkbfv.NewKeyGenerator(self.params, sampler)
        else:
            self.params = mkrlwe.Parameters(pset["logN"], pset["Q"], pset["P"])
            kgen = mkrlwe.NewKeyGenerator(self.params, sampler)
        self.nq, self.moduli = len(pset["Q"]), list(pset["Q"]) + list(pset["P"])
        self.R = len(self.moduli)
        self.rng = np.random.default_rng(2031)
        if keygen:
            self.sk = {u: kgen.GenSecretKey(u) for u in ("user0", "user1")}
        else:                                                       # any canonical words serve as S: the sharing is linear in the stored words
            self.sk = {u: mkrlwe.SecretKey(self.params, u) for u in ("user0", "user1")}
            for u in self.sk:
                self.sk[u].Value.upload(self.uniform((1,), self.R))
        self.S = self.sk["user0"].Value.download()[0]              # the stored words [R][N]
        self._ct, self._model = {}, {}

    def uniform(self, head, limbs):
        """canonical uniform words [head..][limbs][N] under the first `limbs` moduli of the rows"""
        return np.stack([self.rng.integers(0, q, tuple(head) + (self.N,), dtype=np.uint64) for q in self.moduli[:limbs]], axis=len(head))

    def ct(self, ids):
        k = tuple(ids)
        if k not in self._ct:
            self._ct[k] = self.mk.Ciphertext(self.params, list(ids), self.L - 1).upload(self.uniform((1 + len(ids),), self.L))
        return self._ct[k]

    def rows(self, count=1, fill=SENTINEL):
        return self.mk.DeviceLimbs(self.params, count, self.R).upload(np.full((count, self.R, self.N), fill, dtype=np.uint64))

    def model(self, t, points, key=KEY, nonce=NONCE):
        k = (t, tuple(points), tuple(key), nonce)
        if k not in self._model:
            self._model[k] = T.shares(self.S, t, points, key, nonce, self.moduli, values=stream)
        return self._model[k]

    def canonical(self, a):
        return all((a[..., j, :] < m).all() for j, m in enumerate(self.moduli[:a.shape[-2]]))

    # ---- the raw calls
    def gen(self, t, points, key=KEY, nonce=NONCE, n=None, sk="default", pts="default", outs="default"):
        """mkhe_threshold_gen_shares into buffers of twice the size filled with a sentinel -> (rc, uint64 [n][R][N]); every word of every output is
        written, nothing behind it; a refused call leaves all of it untouched"""
        bufs = [self.rows(2) for _ in points]
        rc = self.lib.mkhe_threshold_gen_shares(self.params.ctx, self.sk["user0"].Value.devptr() if sk == "default" else sk, t,
                                                len(points) if n is None else n, (C.c_uint32 * len(points))(*points) if pts == "default" else pts,
                                                key_arg(key), nonce, self.handles([b.devptr() for b in bufs]) if outs == "default" else outs(bufs))
        got = np.stack([b.download() for b in bufs])
        if rc == 0:
            assert (got[:, 1] == SENTINEL).all(), "mkhe_threshold_gen_shares wrote behind uint64[R][N]"
            assert self.canonical(got[:, 0]), "a word of an output was not written, or is not canonical"
        else:
            assert (got == SENTINEL).all(), "a refused mkhe_threshold_gen_shares wrote to its outputs"
        return rc, got[:, 0]

    def additive(self, share, point, active, inplace=False, nactive=None, src="default", out="default", pts="default"):
        """mkhe_threshold_additive_key of a host share [R][N] -> (rc, uint64 [R][N])"""
        a = self.rows(2)
        a.upload(np.stack([share, np.full_like(share, SENTINEL)]))
        b = a if inplace else self.rows(2)
        rc = self.lib.mkhe_threshold_additive_key(self.params.ctx, a.devptr() if src == "default" else src(a), point, len(active) if nactive is None else nactive,
                                                  (C.c_uint32 * len(active))(*active) if pts == "default" else pts, b.devptr() if out == "default" else out(b))
        got = b.download()
        assert (got[1] == SENTINEL).all(), "mkhe_threshold_additive_key wrote behind uint64[R][N]"
        if rc != 0:
            assert (got[0] == (share if inplace else SENTINEL)).all(), "a refused mkhe_threshold_additive_key wrote to its output"
        if not inplace:
            assert (a.download()[0] == share).all()                 # the share is left alone
        return rc, got[0]

    def lsum(self, srcs, alias=None, count=None, limbs=None, nsrc=None, ptrs="default", dst="default"):
        """mkhe_limbs_sum of host arrays [count][limbs][N] -> (rc, uint64 [count][limbs][N]); alias = s: dst is the buffer of source s"""
        cnt, lim = srcs[0].shape[0], srcs[0].shape[1]
        bufs = [self.mk.DeviceLimbs(self.params, cnt, lim).upload(s) for s in srcs]
        out = self.mk.DeviceLimbs(self.params, 2 * cnt, lim).upload(np.full((2 * cnt, lim, self.N), SENTINEL, dtype=np.uint64))
        d = bufs[alias] if alias is not None else out
        rc = self.lib.mkhe_limbs_sum(self.params.ctx, cnt if count is None else count, lim if limbs is None else limbs, len(srcs) if nsrc is None else nsrc,
                                     self.handles([b.devptr() for b in bufs]) if ptrs == "default" else ptrs(bufs), d.devptr() if dst == "default" else dst(d))
        got = d.download()
        if alias is None:
            assert (got[cnt:] == SENTINEL).all(), "mkhe_limbs_sum wrote behind uint64[count][limbs][N]"
            if rc != 0:
                assert (got == SENTINEL).all(), "a refused mkhe_limbs_sum wrote to its output"
        for s, (b, h) in enumerate(zip(bufs, srcs)):
            if s != alias:
                assert (b.download() == h).all()                    # the sources are left alone
        return rc, got[:cnt]

    def expected_sum(self, srcs):
        acc = np.zeros_like(srcs[0])
        for s in srcs:
            for j in range(s.shape[1]):
                acc[:, j] = (acc[:, j] + s[:, j]) % np.uint64(self.moduli[j])       # below 2^61: no wrap
        return acc


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


def test_the_rings():
    assert (world("three").nq, world("three").R, world("one").nq, world("one").R, world("low").nq, world("low").R, world("low").L) == (3, 5, 1, 3, 4, 6, 2)
    assert all(m > 1 << 32 for name in RINGS for m in world(name).moduli)       # every uint32 point is below every modulus of these rings


# ------------------------------------------------------------------ the shares
@pytest.mark.parametrize("t,n", SHAPES)
def test_gen_shares_is_the_model(w, t, n):
    points = POINTS[:n] if n < 32 else POINTS
    rc, got = w.gen(t, points)
    assert rc == 0, error()
    want = w.model(t, points)
    for p in range(n):
        assert (got[p] == want[p]).all(), (t, n, p)
    if t == 1:
        assert all((got[p] == w.S).all() for p in range(n))        # t = 1 reads no stream and writes S
    else:
        assert all((got[p] != w.S).mean() > 0.99 for p in range(n))
    assert (w.sk["user0"].Value.download()[0] == w.S).all()        # the key is left alone


def test_shares_are_deterministic_and_depend_on_key_nonce_every_point_and_t(w3):
    w, points = w3, POINTS[:4]
    a, b, c, d = (w.gen(3, points, nonce=n, key=k) for n, k in ((NONCE, KEY), (NONCE, KEY), (NONCE + 1, KEY), (NONCE, KEY[::-1])))
    assert all(x[0] == 0 for x in (a, b, c, d)), error()
    assert (a[1] == b[1]).all()
    assert (a[1] != c[1]).mean() > 0.99 and (a[1] != d[1]).mean() > 0.99
    for p in range(4):                                              # another point for holder p: its share moves, the others do not
        moved = list(points)
        moved[p] = 123456789 + p
        rc, got = w.gen(3, moved)
        assert rc == 0, error()
        for o in range(4):
            assert ((got[o] != a[1][o]).mean() > 0.99) if o == p else (got[o] == a[1][o]).all(), (p, o)
    rc, two = w.gen(2, points)                                      # another threshold under the same key and nonce
    assert rc == 0 and (two != a[1]).mean() > 0.99, error()
    assert len({a[1][p].tobytes() for p in range(4)}) == 4          # no two holders have the same share


def test_additive_key_is_the_share_times_lambda_also_in_place(w):
    share = w.uniform((), w.R)
    for active in ([POINTS[1]], POINTS[:3], POINTS[1:6], POINTS):
        point = active[len(active) // 2]
        want = T.additive(share, point, active, w.moduli)
        for inplace in (False, True):
            rc, got = w.additive(share, point, active, inplace=inplace)
            assert rc == 0 and (got == want).all(), (len(active), inplace, error())
    assert (T.additive(share, POINTS[1], [POINTS[1]], w.moduli) == share).all()       # an active set of one: lambda = 1


def test_every_t_subset_and_a_superset_reconstruct_the_key(w):
    th, cb = w.mk.Thresholdizer(w.params), w.mk.Combiner(w.params)
    holders = {"h%d" % i: POINTS[i] for i in range(5)}
    shares = th.GenShares(w.sk["user0"], 3, holders, w.mk.DeviceSampler(key=KEY, insecure_test_only=True))
    assert sorted(shares) == sorted(holders) and all(s.ID == "user0" and s.Holder == h and s.Point == holders[h] and s.Threshold == 3 for h, s in shares.items())
    assert (np.stack([shares[h].download()[0] for h in holders]) == w.model(3, list(holders.values()), nonce=0)).all()      # the sampler's first nonce
    sets = list(itertools.combinations(holders, 3)) + [tuple(holders)[:4], tuple(holders)]
    assert len(sets) == 12
    for active in sets:
        pts = {h: holders[h] for h in active}
        keys = [cb.AdditiveKey(shares[h], pts) for h in active]
        assert all(k.ID == "user0" for k in keys)
        back = cb.Reconstruct(keys)
        assert back.ID == "user0" and (back.Value.download()[0] == w.S).all(), active
    two = [cb.AdditiveKey(shares[h], {h: holders[h] for h in ("h0", "h1")}) for h in ("h0", "h1")]
    assert (cb.Reconstruct(two).Value.download()[0] != w.S).mean() > 0.99         # t - 1 holders do not
    moved = w.mk.SecretKeyShare(w.params, "user0", "h2", holders["h2"], 3).upload(shares["h2"].download())        # the wire
    assert (cb.AdditiveKey(moved, list(holders.values())).Value.download() == cb.AdditiveKey(shares["h2"], holders).Value.download()).all()


def test_the_holders_shares_fold_to_the_share_of_the_key_and_merge_to_decrypt(w):
    """linearity through the real path: mkhe_decrypt_share(flood_bits = 0) on the additive keys, folded, is the call on the true key, bit for bit"""
    th, cb, dec = w.mk.Thresholdizer(w.params), w.mk.Combiner(w.params), w.mk.Decryptor(w.params)
    holders = {"h%d" % i: POINTS[i] for i in range(5)}
    shares = th.GenShares(w.sk["user0"], 3, holders, w.mk.DeviceSampler(key=KEY, insecure_test_only=True))
    ct = w.ct(["user0", "user1"])
    true = dec.ShareNew(ct, w.sk["user0"], 0, None)
    skSet = w.mk.NewSecretKeySet()
    for u in ("user0", "user1"):
        skSet.AddSecretKey(w.sk[u])
    whole = dec.Decrypt(ct, skSet).download()
    other = dec.ShareNew(ct, w.sk["user1"], 0, None)
    for active in (("h0", "h2", "h4"), ("h1", "h2", "h3", "h4")):
        pts = {h: holders[h] for h in active}
        parts = [dec.ShareNew(ct, cb.AdditiveKey(shares[h], pts), 0, None) for h in active]
        assert all(p.ID == "user0" and (p.download() != true.download()).mean() > 0.99 for p in parts)
        folded = dec.FoldShares(parts)
        assert folded.ID == "user0" and folded.Level() == w.L - 1 and folded.count == 1
        assert (folded.download() == true.download()).all(), active
        assert (dec.MergeShares(ct, [other, folded]).download() == whole).all(), active


def test_fold_shares_checks_ids_levels_and_counts_before_any_engine_call(w3):
    from mkhe_kklss_amd._abi import MkheError
    w, dec = w3, w3.mk.Decryptor(w3.params)
    a = w.mk.DecryptionShare(w.params, "user0", w.L - 1, 1)
    for bad, text in ((w.mk.DecryptionShare(w.params, "user1", w.L - 1, 1), "parties"), (w.mk.DecryptionShare(w.params, "user0", 0, 1), "levels"),
                      (w.mk.DecryptionShare(w.params, "user0", w.L - 1, 2), "ciphertexts")):
        with pytest.raises(MkheError, match=text):
            dec.FoldShares([a, bad])
    with pytest.raises(MkheError, match="no share"):
        dec.FoldShares([])


# ------------------------------------------------------------------ the fold
def test_limbs_sum_is_numpy(w):
    for limbs in sorted({1, w.nq, w.R}):
        for nsrc in (1, 2, 17, 32):                                 # 16 pointers travel in the kernel arguments; 17 and 32 stage the table
            for count in (1, 3):
                srcs = [w.uniform((count,), limbs) for _ in range(nsrc)]
                rc, got = w.lsum(srcs)
                assert rc == 0 and (got == w.expected_sum(srcs)).all(), (limbs, nsrc, count, error())
    srcs = [np.stack([np.full((w.N,), m - 1, dtype=np.uint64) for m in w.moduli])[None] for _ in range(32)]         # the largest canonical words
    rc, got = w.lsum(srcs)
    assert rc == 0 and (got == w.expected_sum(srcs)).all() and w.canonical(got), error()


def test_limbs_sum_with_dst_aliasing_a_source_and_on_a_pcks_shaped_buffer(w):
    for nsrc, alias in ((1, 0), (3, 1), (17, 16)):
        srcs = [w.uniform((2,), w.L) for _ in range(nsrc)]
        rc, got = w.lsum(srcs, alias=alias)
        assert rc == 0 and (got == w.expected_sum(srcs)).all(), (nsrc, alias, error())
    count = 3                                                       # mkhe_pcks_share buffers [count][2][L][N]: count * 2 items
    srcs = [w.uniform((count, 2), w.L) for _ in range(3)]
    rc, got = w.lsum([s.reshape(2 * count, w.L, w.N) for s in srcs])
    want = np.zeros_like(srcs[0])
    for s in srcs:
        want = (want + s) % np.array(w.moduli[:w.L], dtype=np.uint64)[:, None]
    assert rc == 0 and (got.reshape(count, 2, w.L, w.N) == want).all(), error()


# ------------------------------------------------------------------ the full chain, once
def test_pn15qp880_first_and_last_row_against_the_model_and_all_rows_through_reconstruct():
    w = World("rlwe", H.PN15QP880, 14)
    assert (w.N, w.nq, w.R) == (1 << 15, 14, 16)
    points = [1, 4294967295, 1000003]
    rc, got = w.gen(2, points)
    assert rc == 0, error()
    want = T.shares(w.S, 2, points, KEY, NONCE, w.moduli, values=stream, rows=[0, 15])      # the first Q row and the last P row
    assert (got[:, 0] == want[:, 0]).all() and (got[:, 15] == want[:, 1]).all()
    for active in ((0, 2), (0, 1, 2)):
        act = [points[p] for p in active]
        keys = []
        for p in active:
            rc, add = w.additive(got[p], points[p], act)
            assert rc == 0, error()
            keys.append(add[None])
        rc, back = w.lsum(keys)
        assert rc == 0 and (back[0] == w.S).all(), (active, error())
    w.params.close()


def test_a_point_must_be_below_every_modulus():
    """a context whose P holds 65537: the point 65536 is legal there and 65537 is not"""
    w = World("rlwe", dict(logN=LOGN, Q=[0x3fffffffd60001], P=[65537, 0xffffffffffc0001]), 1, keygen=False)
    assert w.moduli[1] == 65537 and (w.S[1] < 65537).all()
    rc, _ = w.gen(2, [1, 65537, 5])
    assert rc != 0 and error().startswith("mkhe_threshold_gen_shares: ") and "smaller than every modulus" in error(), error()
    share = w.uniform((), w.R)
    rc, _ = w.additive(share, 1, [1, 4294967295])
    assert rc != 0 and error().startswith("mkhe_threshold_additive_key: ") and "smaller than every modulus" in error(), error()
    points = [1, 65536, 5]
    rc, got = w.gen(2, points)
    assert rc == 0 and (got == w.model(2, points)).all(), error()
    keys = []
    for p in (1, 2):
        rc, add = w.additive(got[p], points[p], points[1:])
        assert rc == 0 and (add == T.additive(got[p], points[p], points[1:], w.moduli)).all(), error()
        keys.append(add[None])
    rc, back = w.lsum(keys)
    assert rc == 0 and (back[0] == w.S).all(), error()
    w.params.close()


# ------------------------------------------------------------------ refusals
def good_call(w):
    """the context works: a sharing, two additive keys and their fold"""
    points = POINTS[:3]
    rc, got = w.gen(2, points)
    assert rc == 0 and (got == w.model(2, points)).all(), error()
    keys = []
    for p in (0, 2):
        rc, add = w.additive(got[p], points[p], [points[0], points[2]])
        assert rc == 0, error()
        keys.append(add[None])
    rc, back = w.lsum(keys)
    assert rc == 0 and (back[0] == w.S).all(), error()


def check_refused(w, rc, name, text):
    msg = error()
    assert rc != 0 and msg.startswith(name + ": ") and text in msg, msg
    assert not any(("%08x" % x) in msg.lower() or str(x) in msg for x in KEY), msg
    good_call(w)


def test_gen_shares_refusals(w3):
    w, name = w3, "mkhe_threshold_gen_shares"

    def refused(text, t=2, points=POINTS[:3], **kw):
        rc, _ = w.gen(t, list(points), **kw)
        check_refused(w, rc, name, text)

    refused("threshold", t=0)
    refused("threshold", t=4)
    refused("threshold", t=-1)
    refused("nshares", n=0)
    refused("nshares", n=33)
    refused("null key", key=None)
    refused("null key", key=None, t=1)
    refused("null", sk=None)
    refused("null", outs=lambda bufs: None)
    refused("null output", outs=lambda bufs: w.handles([bufs[0].devptr(), None, bufs[2].devptr()]))
    refused("null points", pts=None)
    refused("aligned", sk=C.c_void_p(w.sk["user0"].Value.devptr().value + 8))
    refused("aligned", outs=lambda bufs: w.handles([bufs[0].devptr(), C.c_void_p(bufs[1].devptr().value + 8), bufs[2].devptr()]))
    refused("distinct", outs=lambda bufs: w.handles([bufs[0].devptr(), bufs[1].devptr(), bufs[0].devptr()]))
    keep = w.sk["user0"].Value.download()
    refused("secret key's buffer", outs=lambda bufs: w.handles([bufs[0].devptr(), w.sk["user0"].Value.devptr(), bufs[2].devptr()]))
    assert (w.sk["user0"].Value.download() == keep).all()
    refused("at least 1", points=[1, 0, 5])
    refused("pairwise distinct", points=[1, 5, 5])
    assert w.lib.mkhe_threshold_gen_shares(None, None, 1, 1, None, key_arg(), 0, None) != 0 and error() == name + ": null context"
    rc, got = w.gen(32, POINTS)                                     # the largest call: t = n = 32
    assert rc == 0 and (got[31] == w.model(32, POINTS[31:])[0]).all(), error()


def test_additive_key_refusals(w3):
    w, name = w3, "mkhe_threshold_additive_key"
    share = w.uniform((), w.R)

    def refused(text, point=7, active=(1, 7, 99), **kw):
        rc, _ = w.additive(share, point, list(active), **kw)
        check_refused(w, rc, name, text)

    refused("nactive", nactive=0)
    refused("nactive", nactive=33)
    refused("exactly once", point=8)
    refused("pairwise distinct", active=(1, 7, 7))
    refused("at least 1", active=(0, 7, 99))
    refused("null points", pts=None)
    refused("null", src=lambda a: None)
    refused("null", out=lambda b: None)
    refused("aligned", src=lambda a: C.c_void_p(a.devptr().value + 8))
    refused("aligned", out=lambda b: C.c_void_p(b.devptr().value + 8))
    assert w.lib.mkhe_threshold_additive_key(None, None, 1, 1, None, None) != 0 and error() == name + ": null context"


def test_limbs_sum_refusals(w3):
    w, name = w3, "mkhe_limbs_sum"
    one = [w.uniform((1,), w.L) for _ in range(2)]

    def refused(text, srcs=one, **kw):
        rc, _ = w.lsum(srcs, **kw)
        check_refused(w, rc, name, text)

    refused("limbs", limbs=0)
    refused("limbs", limbs=w.nq + 1)                                # 4 of nQ = 3, R = 5
    refused("limbs", limbs=w.R + 1)
    refused("nsrc", nsrc=0)
    refused("nsrc", nsrc=33)
    refused("count", count=0)
    refused("count", count=65536)
    refused("null", ptrs=lambda bufs: None)
    refused("null source", ptrs=lambda bufs: w.handles([bufs[0].devptr(), None]))
    refused("null", dst=lambda d: None)
    refused("aligned", ptrs=lambda bufs: w.handles([bufs[0].devptr(), C.c_void_p(bufs[1].devptr().value + 8)]))
    refused("aligned", dst=lambda d: C.c_void_p(d.devptr().value + 16 * 8 + 8))
    two = [w.uniform((2,), w.L) for _ in range(2)]
    refused("overlap", srcs=two, count=1, alias=0, dst=lambda d: C.c_void_p(d.devptr().value + 16))       # dst inside source 0, 16 bytes in
    assert w.lib.mkhe_limbs_sum(None, 1, 1, 1, None, None) != 0 and error() == name + ": null context"


def test_refused_on_a_context_that_owns_a_subset_of_the_moduli():
    w = world("low")
    share = w.uniform((), w.R)
    own = (C.c_int * 2)(0, 2)
    assert w.lib.mkhe_ctx_set_owned(w.params.ctx, own, 2) == 0, error()
    try:
        rc, _ = w.gen(2, POINTS[:3])
        assert rc != 0 and error().startswith("mkhe_threshold_gen_shares: ") and "subset of the moduli" in error()
        rc, _ = w.additive(share, 1, [1, 7])
        assert rc != 0 and error().startswith("mkhe_threshold_additive_key: ") and "subset of the moduli" in error()
        rc, _ = w.lsum([w.uniform((1,), 2)])
        assert rc != 0 and error().startswith("mkhe_limbs_sum: ") and "subset of the moduli" in error()
    finally:
        assert w.lib.mkhe_ctx_set_owned(w.params.ctx, own, 0) == 0
    good_call(w)


def test_inside_a_capture_the_sharing_and_a_staged_fold_are_refused_and_the_rest_is_recorded(w3):
    """(where the runtime of this process can capture at all: tests/test_gpu_cnn.py)"""
    from mkhe_kklss_amd._abi import MkheError
    w = w3
    share, srcs = w.uniform((), w.R), [w.uniform((1,), w.L) for _ in range(17)]
    a, b, outs = w.rows(1).upload(share[None]), w.rows(1), [w.rows(1) for _ in range(2)]
    bufs = [w.mk.DeviceLimbs(w.params, 1, w.L).upload(s) for s in srcs]
    dst = w.mk.DeviceLimbs(w.params, 1, w.L).upload(np.full((1, w.L, w.N), SENTINEL, dtype=np.uint64))
    active = (C.c_uint32 * 3)(1, 7, 99)
    try:
        with w.params.Capture() as g:
            rc1 = w.lib.mkhe_threshold_gen_shares(w.params.ctx, w.sk["user0"].Value.devptr(), 2, 2, (C.c_uint32 * 2)(1, 2), key_arg(), 1,
                                                  w.handles([o.devptr() for o in outs]))
            msg1 = error()
            rc2 = w.lib.mkhe_limbs_sum(w.params.ctx, 1, w.L, 17, w.handles([x.devptr() for x in bufs]), dst.devptr())
            msg2 = error()
            rc3 = w.lib.mkhe_threshold_additive_key(w.params.ctx, a.devptr(), 7, 3, active, b.devptr())
            rc4 = w.lib.mkhe_limbs_sum(w.params.ctx, 1, w.L, 16, w.handles([x.devptr() for x in bufs[:16]]), dst.devptr())
            msg4 = error()
        assert rc1 != 0 and msg1.startswith("mkhe_threshold_gen_shares: ") and "capture" in msg1
        assert rc2 != 0 and msg2.startswith("mkhe_limbs_sum: ") and "capture" in msg2
        assert rc3 == 0 and rc4 == 0, msg4
        assert (b.download() == SENTINEL).all() and (dst.download() == SENTINEL).all()     # recorded, not run
        g.launch()
        assert (b.download()[0] == T.additive(share, 7, [1, 7, 99], w.moduli)).all()
        assert (dst.download() == w.expected_sum(srcs[:16])).all()
        print("capture: the sharing and the staged fold were refused, the additive key and the inline fold replayed")
    except MkheError as e:
        print("capture: mkhe_capture_begin refused in this process (%s): the calls inside a capture did not run" % e)
        import gc
        gc.enable()                 # (Graph.__enter__ switched the collector off before the refusal)
        assert "cannot end a multi-stream capture" in str(e)
    assert all((o.download() == SENTINEL).all() for o in outs)
    good_call(w)
