"""Encrypt / PartialDecrypt / Decrypt on the device (-m gpu) through mkrlwe.Encryptor / Decryptor and their mkbfv wrappers
(mkhe_encrypt, mkhe_partial_decrypt, mkhe_decrypt) against the CPU restatement of mkrlwe/encryptor.go:95-112 and
mkrlwe/decryptor.go:26-66 in harness.py (KeyGen.encrypt / KeyGen.decrypt) on the same samples, bit-exact.  Keys are generated on
the device from explicit samples and mirrored on the host with the oracle's KeyGen, as in test_gpu_keygen.py."""
import numpy as np
import pytest

import harness as H
import harness_bfv as HB
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SETS = {
    "N10_q3": H.small_ckks(10, 3),
    "N12_a2_q5": H.small_alpha2(12, 5),
    "N13_q14": dict(H.PN15QP880, logN=13),
    "N16_a2_q3": H.small_alpha2(16, 3),
}
BFV_SETS = {
    "N10_q3": HB.small_bfv(10, 3),
    "N12_q4big": HB.small_bfv(12, 4, big=True),
    "N13_q2": HB.small_bfv(13, 2),
    "N11_q14": dict(HB.BFV_PN15QP880, logN=11),
}


def queued(base):
    """`base` (H.KeyGen or a subclass) whose ternary() / gaussian() hand back queued arrays: push(u, e0, e1) before every encrypt()"""
    class Queued(base):
        def push(self, samples):
            self.t = getattr(self, "t", []) + [np.asarray(samples[0], dtype=np.int64)]
            self.g = getattr(self, "g", []) + [np.asarray(samples[1], dtype=np.int64), np.asarray(samples[2], dtype=np.int64)]

        def ternary(self):
            return self.t.pop(0)

        def gaussian(self):
            return self.g.pop(0)
    return Queued


class Pair:
    """device context + host mirror over one parameter set, with as many parties as a test asks for"""

    def __init__(self, mod, params, ks, hkg, seed):
        from mkhe_kklss_amd import mkrlwe
        self.mk, self.mod, self.params, self.ks, self.hkg = mkrlwe, mod, params, ks, hkg
        self.okg = O.KeyGen(ks)
        self.rng = np.random.default_rng(seed)
        self.N, self.nq = ks.N, len(ks.Q)
        self.kgen = mod.NewKeyGenerator(params)
        self.enc, self.dec = mod.NewEncryptor(params), mod.NewDecryptor(params)
        self.crs_a = params.AddCRS(0).download()[0]
        self.names, self.sk, self.pk, self.sk_h, self.pk_h = [], {}, {}, {}, {}

    def ternary(self):
        return self.rng.choice(np.array([-1, 0, 0, 1], dtype=np.int32), self.N)

    def gauss(self, *count):
        return np.clip(np.rint(self.rng.normal(0, 3.2, count + (self.N,))), -19, 19).astype(np.int32)

    def samples(self, count=None):
        one = lambda: np.concatenate([self.ternary()[None], self.gauss(2)])
        return one() if count is None else np.stack([one() for _ in range(count)])

    def parties(self, k):
        while len(self.names) < k:
            n = "user%d" % len(self.names)
            s, e = self.ternary(), self.gauss(1)
            self.sk[n] = self.kgen.GenSecretKey(n, s)
            self.pk[n] = self.kgen.GenPublicKey(self.sk[n], e)
            self.sk_h[n] = self.okg.gen_secret_key(s)
            self.pk_h[n] = self.okg.gen_public_key(self.sk_h[n], e[0], self.crs_a)
            self.names.append(n)
        return self.names[:k]

    def plaintext(self, level):
        return H.uniform_poly(self.rng, self.ks.Q[: level + 1], self.N)

    def host_encrypt(self, pt, name, level, smp):
        self.hkg.push(smp)
        return np.stack(self.hkg.encrypt(pt, self.pk_h[name], level))

    def sum_ct(self, names, level):
        """the sum of single-party encryptions, as tests/scenario.py builds it: host array [1+k][level+1][N]"""
        ct = np.zeros((1 + len(names), level + 1, self.N), dtype=np.uint64)
        for a, n in enumerate(names):
            c = self.host_encrypt(self.plaintext(level), n, level, self.samples())
            for j in range(level + 1):
                ct[0][j] = self.ks.ringQ.add(j, ct[0][j], c[0][j])
            ct[1 + a] = c[1]
        return ct

    def host_decrypt(self, names, ct):
        vals = {"0": ct[0]}
        for a, n in enumerate(names):
            vals[n] = ct[1 + a]
        return self.hkg.decrypt(vals, {n: self.sk_h[n][: self.nq] for n in names})

    def sk_set(self, names):
        s = self.mk.SecretKeySet()
        for n in names:
            s.AddSecretKey(self.sk[n])
        return s


def make_pair(pset, seed):
    from mkhe_kklss_amd import mkrlwe
    params = mkrlwe.Parameters(pset["logN"], pset["Q"], pset["P"], pset.get("gamma", 2))
    ks = O.KeySwitcher(pset["logN"], pset["Q"], pset["P"], pset.get("gamma", 2))
    return Pair(mkrlwe, params, ks, queued(H.KeyGen)(ks, 0), seed)


@pytest.fixture(scope="module", params=list(SETS))
def pr(request):
    return make_pair(SETS[request.param], seed=sum(map(ord, request.param)))


@pytest.mark.parametrize("drop", [0, 1])
def test_encrypt(pr, drop):
    n, = pr.parties(1)
    level = pr.nq - 1 - drop
    pt, smp = pr.plaintext(level), pr.samples()
    want = pr.host_encrypt(pt, n, level, smp)
    ct = pr.enc.Encrypt(pt, pr.pk[n], pr.mk.Ciphertext(pr.params, [n], level, zero=False), smp)
    assert (ct.download() == want).all()
    pt_ntt = np.stack([pr.ks.ringQ.ntt(j, pt[j]) for j in range(level + 1)])
    ct = pr.enc.Encrypt(pt_ntt, pr.pk[n], pr.mk.Ciphertext(pr.params, [n], level, zero=False), smp, pt_is_ntt=True)
    assert (ct.download() == want).all()


@pytest.mark.parametrize("count", [1, 3, 8])
@pytest.mark.parametrize("ntt", [False, True])
def test_encrypt_batch_equals_one_at_a_time(pr, count, ntt):
    n, = pr.parties(1)
    level = pr.nq - 1
    pts, smp = np.stack([pr.plaintext(level) for _ in range(count)]), pr.samples(count)
    cts = pr.enc.EncryptBatch(pts, pr.pk[n], smp, pt_is_ntt=ntt)
    assert len(cts) == count
    for b in range(count):
        one = pr.enc.Encrypt(pts[b], pr.pk[n], pr.mk.Ciphertext(pr.params, [n], level, zero=False), smp[b], pt_is_ntt=ntt)
        assert cts[b].ids == [n] and cts[b].Level() == level
        assert (cts[b].download() == one.download()).all()


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_decrypt_and_partial_decrypt(pr, k):
    names = pr.parties(k)
    level = pr.nq - 1 - (k % 2 == 0)                  # both the top level and a dropped one are covered
    host = pr.sum_ct(names, level)
    want = pr.host_decrypt(names, host)
    ct = pr.mk.Ciphertext(pr.params, names, level, zero=False).upload(host)
    got = pr.dec.Decrypt(ct, pr.sk_set(pr.parties(max(k, 2)))).download()[0]         # a key too many is ignored (decryptor.go:55-59)
    assert (got == want).all()
    # the chain of PartialDecrypts in a random order, then a reduce, equals Decrypt; the first step against the host restatement
    order = [names[i] for i in pr.rng.permutation(k)]
    cur = ct
    for step, n in enumerate(order):
        nxt = pr.dec.PartialDecrypt(cur, pr.sk[n])
        assert nxt.ids == [i for i in cur.ids if i != n] and nxt.Level() == level
        if step == 0:
            h, a = nxt.download(), names.index(n)
            for j in range(level + 1):
                t = pr.ks.ringQ.intt(j, pr.ks.ringQ.mul(j, pr.ks.ringQ.ntt(j, host[1 + a][j]), pr.sk_h[n][j]))
                assert (h[0][j] == pr.ks.ringQ.add(j, host[0][j], t)).all()
            assert (h[1:] == np.delete(host, 1 + a, axis=0)[1:]).all()
        cur = nxt
    assert (ct.download() == host).all()              # PartialDecrypt leaves its input alone
    end = cur.download()
    assert end.shape == (1, level + 1, pr.N)
    assert (np.stack([pr.ks.ringQ.reduce(j, end[0][j]) for j in range(level + 1)]) == want).all()


def test_decrypt_with_a_missing_key_raises(pr):
    from mkhe_kklss_amd._abi import MkheError
    names = pr.parties(2)
    ct = pr.mk.Ciphertext(pr.params, names, pr.nq - 1)
    with pytest.raises(MkheError, match="Cannot Decrypt: there is a missing secretkey"):
        pr.dec.Decrypt(ct, pr.sk_set(names[:1]))


def test_argument_validation(pr):
    import ctypes as C
    from mkhe_kklss_amd._abi import MkheError, handle_array, lib, s32p
    n, m = pr.parties(2)
    level = pr.nq - 1
    pt, smp = pr.plaintext(level), pr.samples()
    out = pr.mk.Ciphertext(pr.params, [n], level)
    with pytest.raises(MkheError, match="expected samples of shape"):
        pr.enc.Encrypt(pt, pr.pk[n], out, smp[:2])
    with pytest.raises(MkheError, match="expected samples of shape"):
        pr.enc.EncryptBatch(np.stack([pt, pt]), pr.pk[n], smp[None])
    with pytest.raises(MkheError, match="out of range"):
        pr.enc.EncryptBatch(np.zeros((1, pr.nq + 1, pr.N), dtype=np.uint64), pr.pk[n], smp[None])
    two = pr.mk.Ciphertext(pr.params, [n, m], level)
    with pytest.raises(MkheError, match="over the id of pk alone"):
        pr.enc.Encrypt(pt, pr.pk[n], two, smp)
    # the same straight at the C ABI
    d = pr.mk.DeviceLimbs(pr.params, 1, level + 1).upload(pt[None])
    ptr = np.ascontiguousarray(smp[None]).ctypes.data_as(s32p)
    call = lambda lvl, cnt, o: lib().mkhe_encrypt(pr.params.ctx, lvl, cnt, pr.pk[n].Value.devptr(), d.devptr(), 0, ptr, handle_array([o.h]))
    for args, text in (((pr.nq, 1, out), "level out of range"), ((-1, 1, out), "level out of range"), ((level, 0, out), "count"),
                       ((level, 1, two), "exactly one party")):
        assert call(*args) != 0 and text in lib().mkhe_last_error().decode()          # the error text is read right behind its call
    assert lib().mkhe_encrypt(pr.params.ctx, level, 1, None, d.devptr(), 0, ptr, handle_array([out.h])) != 0
    assert (out.download() == 0).all()                # nothing was written
    for slot in (0, 3):
        assert lib().mkhe_partial_decrypt(pr.params.ctx, two.h, slot, pr.sk[n].Value.devptr(), out.h) != 0
        assert "slot out of range" in lib().mkhe_last_error().decode()
    assert lib().mkhe_partial_decrypt(pr.params.ctx, two.h, 1, pr.sk[n].Value.devptr(), two.h) != 0       # out over the wrong ids
    assert lib().mkhe_decrypt(pr.params.ctx, two.h, None, d.devptr()) != 0


def test_full_size_pn15qp880():
    pr = make_pair(H.PN15QP880, seed=880)
    names = pr.parties(4)
    level = pr.nq - 1
    pt, smp = pr.plaintext(level), pr.samples()
    ct = pr.enc.Encrypt(pt, pr.pk[names[0]], pr.mk.Ciphertext(pr.params, names[:1], level, zero=False), smp)
    assert (ct.download() == pr.host_encrypt(pt, names[0], level, smp)).all()
    host = pr.sum_ct(names, level)
    d = pr.mk.Ciphertext(pr.params, names, level, zero=False).upload(host)
    assert (pr.dec.Decrypt(d, pr.sk_set(names)).download()[0] == pr.host_decrypt(names, host)).all()


# ------------------------------------------------------------------ mkbfv
@pytest.fixture(scope="module", params=list(BFV_SETS))
def bp(request):
    from mkhe_kklss_amd import mkbfv
    pset = BFV_SETS[request.param]
    bfv = HB.make_bfv(pset)
    params = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], pset["T"])
    return Pair(mkbfv, params, bfv.ks, queued(HB.BFVKeyGen)(bfv, 0), seed=sum(map(ord, request.param)) + 1)


def test_bfv_encrypt_decrypt(bp):
    from mkhe_kklss_amd import mkbfv
    names = bp.parties(3)
    T, level = bp.params.T(), bp.nq - 1
    msgs = {n: bp.rng.integers(-(T // 2), T // 2 + 1, bp.N).astype(np.int64) for n in names}
    tot = None
    for n in names:
        pt = mkbfv.ScaleUp(msgs[n], bp.params)
        assert (pt == bp.hkg.encode(msgs[n])).all()
        smp = bp.samples()
        ct = bp.enc.EncryptPtxt(pt, bp.pk[n], smp)
        assert isinstance(ct, mkbfv.Ciphertext) and ct.ids == [n]
        assert (ct.download() == bp.host_encrypt(pt, n, level, smp)).all()
        # mkbfv_test.go:282-306: a fresh encryption decrypts exactly
        one = bp.sk_set([n])
        assert (mkbfv.ScaleDown(bp.dec.DecryptPtxt(ct, one), bp.params) == msgs[n]).all()
        tot = ct if tot is None else mkbfv.NewEvaluator(bp.params).AddNew(tot, ct)
    host = tot.download()
    want = bp.host_decrypt(names, host)
    got = bp.dec.DecryptPtxt(tot, bp.sk_set(names))
    assert (got == want).all()
    s = sum(msgs.values()) % T
    assert (mkbfv.ScaleDown(got, bp.params) == np.where(s > T // 2, s - T, s)).all()
    assert (mkbfv.ScaleDown(got, bp.params) == bp.hkg.decode(want)).all()
    part = bp.dec.PartialDecrypt(tot, bp.sk[names[1]])
    assert isinstance(part, mkbfv.Ciphertext) and part.ids == [names[0], names[2]]
    assert (bp.dec.DecryptPtxt(part, bp.sk_set(names)) == want).all()
