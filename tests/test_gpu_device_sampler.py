"""Encryption randomness drawn on the device (-m gpu): mkhe_sample_small against the Python-integer model of tests/device_sampler_model.py,
mkhe_encrypt_seeded against mkhe_encrypt fed the model's samples (that path is pinned by test_gpu_encdec.py), both bit for bit; determinism
and separation of (key, nonce, item); every refusal followed by a call that works; and the mirrors end to end with a DeviceSampler.
logN = 10 unless a case says otherwise."""
import ctypes as C
import types

import numpy as np
import pytest

import device_sampler_model as M
import harness as H
import harness_bfv as HB
from scenario import Scenario

pytestmark = pytest.mark.gpu

KEY = [0x9E3779B9, 0x7F4A7C15, 0xF39CC060, 0x5CEDC834, 0x1082276B, 0xF3A27251, 0xF86C6A11, 0xD0C18E95]
NONCE_HI = 0xFEDCBA9876543210
SENTINEL = 0x7B7B7B7B7B7B7B7B
CKKS = H.small_ckks(10, 3)
BFV = HB.small_bfv(10, 3)


def key_arg(key=KEY):
    return (C.c_uint32 * 8)(*key)


def table_arg(cdt):
    return None if cdt is None else (C.c_uint64 * len(cdt))(*cdt)


def error():
    from mkhe_kklss_amd._abi import lib
    return lib().mkhe_last_error().decode()


class Ring:
    """a context, one key pair made on it and what the calls below need"""

    def __init__(self, params, level_count, mod=None):
        from mkhe_kklss_amd import mkrlwe
        from mkhe_kklss_amd._abi import lib
        self.mk, self.lib, self.params, self.N, self.nq = mkrlwe, lib(), params, params.N(), level_count
        self.cdt = mkrlwe.small_cdt(3.2)
        self.rng = np.random.default_rng(self.N + level_count)
        params.AddCRS(0, seed=99)
        kgen = (mod or mkrlwe).NewKeyGenerator(params, mkrlwe.HostSampler(np.random.default_rng(7), insecure_test_only=True))
        self.sk, self.pk = kgen.GenKeyPair("user0")
        self._model = {}

    def sample(self, kind, count, nonce, first, cdt, key=KEY, out=None, limbs=1):
        """mkhe_sample_small into a buffer of twice the size filled with a sentinel -> (rc, int32 [count][N]); what lies behind stays untouched"""
        buf = self.mk.DeviceLimbs(self.params, max(count, 1), limbs).upload(np.full((max(count, 1), limbs, self.N), SENTINEL, dtype=np.uint64))
        rc = self.lib.mkhe_sample_small(self.params.ctx, kind, count, None if key is None else key_arg(key), nonce, first, table_arg(cdt),
                                        0 if cdt is None else len(cdt), buf.devptr() if out is None else out(buf))
        flat = buf.download().reshape(-1)
        n = max(count, 0) * self.N // 2
        if rc == 0:
            assert (flat[n:] == SENTINEL).all(), "mkhe_sample_small wrote behind int32[count][N]"
        else:
            assert (flat == SENTINEL).all(), "a refused mkhe_sample_small wrote to its output"
        return rc, flat[:n].view(np.int32).reshape(max(count, 0), self.N)

    def model_samples(self, nonce, count):
        """[count][3][N] of (KEY, nonce), computed once for the largest count asked for first (17) and cut"""
        if nonce not in self._model or len(self._model[nonce]) < count:
            self._model[nonce] = np.array(M.encrypt_samples(count, KEY, nonce, self.N, self.cdt), dtype=np.int32)
        return self._model[nonce][:count]

    def plaintexts(self, level, count, ntt):
        pts = np.stack([H.uniform_poly(self.rng, self.params.Q[: level + 1], self.N) for _ in range(count)])
        return self.mk.DeviceLimbs(self.params, count, level + 1).upload(pts)

    def outs(self, level, count):
        return [self.mk.Ciphertext(self.params, ["user0"], level) for _ in range(count)]

    def seeded(self, level, d, ntt, nonce, outs, key=KEY, cdt="default", ncdt=None, count=None, pk="default", handles="default"):
        from mkhe_kklss_amd._abi import handle_array
        cdt = self.cdt if cdt == "default" else cdt
        return self.lib.mkhe_encrypt_seeded(self.params.ctx, level, len(outs) if count is None else count,
                                            self.pk.Value.devptr() if pk == "default" else pk, d.devptr(), ntt,
                                            None if key is None else key_arg(key), nonce, table_arg(cdt),
                                            (0 if cdt is None else len(cdt)) if ncdt is None else ncdt,
                                            handle_array([c.h for c in outs]) if handles == "default" else handles)

    def host(self, level, d, ntt, samples, outs):
        from mkhe_kklss_amd._abi import handle_array, s32p
        s = np.ascontiguousarray(samples, dtype=np.int32)
        return self.lib.mkhe_encrypt(self.params.ctx, level, len(outs), self.pk.Value.devptr(), d.devptr(), ntt, s.ctypes.data_as(s32p),
                                     handle_array([c.h for c in outs]))


@pytest.fixture(scope="module")
def rings():
    from mkhe_kklss_amd import mkrlwe
    r = {}

    def get(logN):
        if logN not in r:
            pset = H.small_ckks(logN, 3)
            r[logN] = Ring(mkrlwe.Parameters(pset["logN"], pset["Q"], pset["P"]), 3)
        return r[logN]
    return get


@pytest.fixture(scope="module")
def ck(rings):
    return rings(10)


@pytest.fixture(scope="module")
def bf():
    from mkhe_kklss_amd import mkbfv
    return Ring(mkbfv.Parameters(BFV["logN"], BFV["Q"], BFV["QMul"], BFV["P"], BFV["T"]), len(BFV["Q"]), mkbfv)


# ------------------------------------------------------------------ mkhe_sample_small against the model
@pytest.mark.parametrize("count,first,nonce", [(1, 0, 0), (4, 0, NONCE_HI), (4, (1 << 32) - 4, 0), (1, 0, NONCE_HI), (4, (1 << 32) - 4, NONCE_HI), (4, 0, 0)])
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("logN", [10, 12])
def test_sample_small_equals_the_model(rings, logN, kind, count, first, nonce):
    r = rings(logN)
    cdt = r.cdt if kind == 1 else None
    rc, got = r.sample(kind, count, nonce, first, cdt)
    assert rc == 0, error()
    want = np.array(M.sample_small(kind, count, KEY, nonce, first, r.N, cdt), dtype=np.int32)
    assert got.shape == want.shape and (got == want).all()
    assert len(set(map(bytes, got))) == count                  # every stream is its own


def test_sample_small_ignores_the_table_for_kind_0(ck):
    a = ck.sample(0, 2, 5, 7, None)
    b = ck.sample(0, 2, 5, 7, [3, 2, 1])                       # not even looked at
    assert a[0] == 0 and b[0] == 0 and (a[1] == b[1]).all()


@pytest.mark.parametrize("name,cdt", [
    ("two", [1 << 62, 3 << 62]),
    ("sixty-four", [(t + 1) * ((1 << 64) // 65) for t in range(64)]),
    ("halves", [(1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 1]),          # a comparison on one half, or a signed one, counts these wrongly
    ("extremes", [0, (1 << 64) - 1]),
])
def test_sample_small_table_edge_cases(ck, name, cdt):
    rc, got = ck.sample(1, 2, 11, 3, cdt)
    assert rc == 0, error()
    want = np.array(M.sample_small(1, 2, KEY, 11, 3, ck.N, cdt), dtype=np.int32)
    assert (got == want).all()
    assert got.min() >= -len(cdt) // 2 and got.max() <= len(cdt) // 2 and len(np.unique(got)) >= (2 if name != "extremes" else 1)


# ------------------------------------------------------------------ mkhe_encrypt_seeded against mkhe_encrypt on the model's samples
def seeded_equals_host(r, level, count, ntt, nonce):
    d = r.plaintexts(level, count, ntt)
    a, b = r.outs(level, count), r.outs(level, count)
    assert r.seeded(level, d, ntt, nonce, a) == 0, error()
    assert r.host(level, d, ntt, r.model_samples(nonce, count), b) == 0, error()
    for x, y in zip(a, b):
        got = x.download()
        assert got.any() and (got == y.download()).all()


@pytest.mark.parametrize("count", [17, 3, 1])                  # 17 > ED_INLINE: the staged pointer table
@pytest.mark.parametrize("ntt", [0, 1])
@pytest.mark.parametrize("drop", [0, 2])                       # the top level and level 0
def test_encrypt_seeded_equals_encrypt_on_model_samples(ck, drop, ntt, count):
    seeded_equals_host(ck, ck.nq - 1 - drop, count, ntt, 21)


@pytest.mark.parametrize("ntt", [0, 1])
def test_encrypt_seeded_on_a_bfv_context(bf, ntt):
    seeded_equals_host(bf, bf.nq - 1, 3, ntt, NONCE_HI)


def test_determinism_and_separation(ck):
    level = ck.nq - 1
    one = H.uniform_poly(ck.rng, ck.params.Q[: level + 1], ck.N)
    d = ck.mk.DeviceLimbs(ck.params, 2, level + 1).upload(np.stack([one, one]))        # the same plaintext twice
    a, b, c = ck.outs(level, 2), ck.outs(level, 2), ck.outs(level, 2)
    assert ck.seeded(level, d, 0, 40, a) == 0 and ck.seeded(level, d, 0, 40, b) == 0 and ck.seeded(level, d, 0, 41, c) == 0, error()
    A, B, Cc = ([x.download() for x in v] for v in (a, b, c))
    assert all((x == y).all() for x, y in zip(A, B))           # the same (key, nonce): the same ciphertexts
    assert all((x != y).any() for x, y in zip(A, Cc))          # nonce n and n + 1
    assert (A[0][1] != A[1][1]).mean() > 0.99                  # items b and b + 1 carry different c1 (u, e1 differ; the plaintext is not in c1)
    assert (A[0][0] != A[1][0]).mean() > 0.99


# ------------------------------------------------------------------ refusals
def test_sample_small_refusals(ck):
    def refused(text, *args, **kw):
        rc, _ = ck.sample(*args, **kw)
        assert rc != 0 and error().startswith("mkhe_sample_small: ") and text in error() and not any("%08x" % w in error().lower() for w in KEY), error()
        rc, got = ck.sample(0, 1, 1, 0, None)                  # and the context works
        assert rc == 0 and set(np.unique(got)) == {-1, 0, 1}, error()

    refused("null key", 0, 1, 0, 0, None, key=None)
    refused("null output", 0, 1, 0, 0, None, out=lambda buf: None)
    refused("null table", 1, 1, 0, 0, None)
    rc = ck.lib.mkhe_sample_small(ck.params.ctx, 1, 1, key_arg(), 0, 0, table_arg(ck.cdt), 0, ck.mk.DeviceLimbs(ck.params, 1, 1).devptr())
    assert rc != 0 and error().startswith("mkhe_sample_small: ") and "ncdt" in error()
    refused("ncdt", 1, 1, 0, 0, ck.cdt[:37])
    refused("ncdt", 1, 1, 0, 0, list(range(1, 67)))
    refused("strictly increasing", 1, 1, 0, 0, [5, 9, 9, 12])
    refused("strictly increasing", 1, 1, 0, 0, [9, 5])
    refused("kind", 2, 1, 0, 0, ck.cdt)
    refused("kind", -1, 1, 0, 0, None)
    refused("count", 0, 0, 0, 0, None)
    refused("count", 0, -1, 0, 0, None)
    rc = ck.lib.mkhe_sample_small(ck.params.ctx, 0, 196606, key_arg(), 0, 0, None, 0, ck.mk.DeviceLimbs(ck.params, 1, 1).devptr())
    assert rc != 0 and error().startswith("mkhe_sample_small: ") and "count" in error()
    refused("2^32", 0, 4, 0, (1 << 32) - 3, None)
    refused("aligned", 0, 1, 0, 0, None, out=lambda buf: C.c_void_p(buf.devptr().value + 8))
    assert ck.lib.mkhe_sample_small(None, 0, 1, key_arg(), 0, 0, None, 0, None) != 0 and error() == "mkhe_sample_small: null context"


def test_encrypt_seeded_refusals(ck):
    level = ck.nq - 1
    d = ck.plaintexts(level, 1, 0)
    out = ck.outs(level, 1)

    def refused(text, **kw):
        outs = kw.pop("outs", out)
        before = [o.download() for o in outs]
        assert ck.seeded(kw.pop("level", level), d, 0, 3, outs, **kw) != 0
        assert error().startswith("mkhe_encrypt_seeded: ") and text in error() and not any("%08x" % w in error().lower() for w in KEY), error()
        assert all((o.download() == b).all() for o, b in zip(outs, before))            # nothing was written
        seeded_equals_host(ck, level, 1, 0, 3)                 # and the context works

    refused("null key", key=None)
    refused("null", handles=None)
    refused("null", pk=None)
    refused("null table", cdt=None)
    refused("ncdt", ncdt=0)
    refused("ncdt", cdt=ck.cdt[:37])
    refused("ncdt", cdt=list(range(1, 67)))
    refused("strictly increasing", cdt=[5, 9, 9, 12])
    refused("count", count=0)
    refused("count", count=65536)
    refused("level", level=ck.nq)
    refused("level+1 limbs", outs=ck.outs(level - 1, 1))
    two = [ck.mk.Ciphertext(ck.params, ["user0", "user1"], level)]
    refused("exactly one party", outs=two)


def test_refused_on_a_context_that_owns_a_subset_of_the_moduli(ck):
    level = ck.nq - 1
    d, out = ck.plaintexts(level, 1, 0), ck.outs(level, 1)
    mtot = len(CKKS["Q"]) + len(CKKS["P"])
    own = (C.c_int * 3)(0, 2, mtot - 1)
    assert ck.lib.mkhe_ctx_set_owned(ck.params.ctx, own, 3) == 0, error()
    try:
        assert ck.seeded(level, d, 0, 3, out) != 0 and error().startswith("mkhe_encrypt_seeded: ") and "subset of the moduli" in error()
        rc, _ = ck.sample(0, 1, 0, 0, None)
        assert rc != 0 and error().startswith("mkhe_sample_small: ") and "subset of the moduli" in error()
    finally:
        assert ck.lib.mkhe_ctx_set_owned(ck.params.ctx, own, 0) == 0
    assert (out[0].download() == 0).all()
    seeded_equals_host(ck, level, 1, 0, 3)
    assert ck.sample(0, 1, 0, 0, None)[0] == 0


def test_refused_inside_a_capture(ck):
    """(where the runtime of this process can capture at all: tests/test_gpu_cnn.py)"""
    from mkhe_kklss_amd._abi import MkheError
    level = ck.nq - 1
    d, out = ck.plaintexts(level, 1, 0), ck.outs(level, 1)
    buf = ck.mk.DeviceLimbs(ck.params, 1, 1)
    try:
        with ck.params.Capture():
            rc1 = ck.seeded(level, d, 0, 3, out)
            m1 = error()
            rc2 = ck.lib.mkhe_sample_small(ck.params.ctx, 0, 1, key_arg(), 0, 0, None, 0, buf.devptr())
            m2 = error()
        assert rc1 != 0 and m1.startswith("mkhe_encrypt_seeded: ") and "capture" in m1
        assert rc2 != 0 and m2.startswith("mkhe_sample_small: ") and "capture" in m2
        print("capture: both calls were refused inside a capture")
    except MkheError as e:
        print("capture: mkhe_capture_begin refused in this process (%s): the refusals inside a capture did not run" % e)
        import gc
        gc.enable()                 # (Graph.__enter__ switched the collector off before the refusal)
        assert "cannot end a multi-stream capture" in str(e)
    seeded_equals_host(ck, level, 1, 0, 3)
    assert ck.sample(0, 1, 0, 0, None)[0] == 0


# ------------------------------------------------------------------ the mirrors, end to end
def _max_log2_err(a, b):
    d = np.abs(np.asarray(a) - np.asarray(b))
    return float(np.log2(max(d.real.max(), d.imag.max(), 1e-300)))


def test_mkckks_end_to_end_with_a_device_sampler():
    """setting and bounds of test_gpu_ckks_device_e2e.py (Scenario.precision_bound, 8 extra bits for encrypt / decrypt, 12 for a product)"""
    from mkhe_kklss_amd import mkckks, mkrlwe
    pset = H.small_ckks(10, 4)
    bound = lambda extra: Scenario.precision_bound(types.SimpleNamespace(scale=pset["scale"], logN=pset["logN"]), extra)
    params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], pset["scale"])
    params.GenDefaultCRS(seed=4321)
    kgen = mkrlwe.NewKeyGenerator(params, mkrlwe.HostSampler(np.random.default_rng(2024), insecure_test_only=True))
    sampler = mkrlwe.DeviceSampler()
    enc, dec, ev = mkckks.NewEncryptor(params, sampler=sampler, encoder="device"), mkckks.NewDecryptor(params, encoder="device"), mkckks.NewEvaluator(params)
    skSet, pkSet, rlk = mkrlwe.NewSecretKeySet(), mkrlwe.NewPublicKeyKeySet(), mkrlwe.RelinearizationKeySet(params)
    names, rng, n = ["user0", "user1"], np.random.default_rng(17), 1 << (pset["logN"] - 1)
    for p in names:
        sk, pk = kgen.GenKeyPair(p)
        skSet.AddSecretKey(sk)
        pkSet.AddPublicKey(pk)
        rlk.AddRelinearizationKey(kgen.GenRelinearizationKey(sk, kgen.GenSecretKey(p)))
    zs = {p: np.full(n, complex(0.1 / 2, 1.0 / 2)) + rng.uniform(-0.05, 0.05, n) for p in names}           # mkckks_test.go:330-340
    ct = None
    for i, p in enumerate(names):
        c = enc.EncryptMsgNew(mkckks.Message(zs[p]), pkSet.GetPublicKey(p))
        assert sampler.counter == i + 1                        # one nonce per engine call
        assert _max_log2_err(dec.Decrypt(c, skSet).Value, zs[p]) <= bound(8)
        ct = c if ct is None else ev.AddNew(ct, c)
    got = dec.Decrypt(ev.MulRelinNew(ct, ct, rlk), skSet).Value
    print("product: 2^%.1f, bound 2^%.1f" % (_max_log2_err(got, sum(zs.values()) ** 2), bound(12)))
    assert _max_log2_err(got, sum(zs.values()) ** 2) <= bound(12)
    # two successive batches of the same messages: different ciphertexts, the same messages; explicit samples still go through mkhe_encrypt
    msgs = [mkckks.Message(zs["user0"]), mkckks.Message(zs["user1"]), mkckks.Message(zs["user0"])]
    b1, b2 = enc.EncryptMsgBatch(msgs, pkSet.GetPublicKey("user1")), enc.EncryptMsgBatch(msgs, pkSet.GetPublicKey("user1"))
    assert sampler.counter == 4
    for x, y, m in zip(b1, b2, msgs):
        assert (x.download() != y.download()).mean() > 0.99
        assert _max_log2_err(dec.Decrypt(x, skSet).Value, m.Value) <= bound(8) and _max_log2_err(dec.Decrypt(y, skSet).Value, m.Value) <= bound(8)
    assert (b1[0].download() != b1[2].download()).mean() > 0.99               # the same message twice in one batch
    smp = np.array(M.encrypt_samples(1, KEY, 0, params.N(), sampler.cdt), dtype=np.int32)[0]
    e1, e2 = enc.EncryptMsgNew(msgs[0], pkSet.GetPublicKey("user0"), smp), enc.EncryptMsgNew(msgs[0], pkSet.GetPublicKey("user0"), smp)
    assert sampler.counter == 4 and (e1.download() == e2.download()).all()
    params.close()


def test_mkbfv_end_to_end_with_a_device_sampler():
    from mkhe_kklss_amd import mkbfv, mkrlwe
    T, N = BFV["T"], 1 << BFV["logN"]
    centre = lambda v: np.where(np.mod(v, T) > T // 2, np.mod(v, T) - T, np.mod(v, T))
    params = mkbfv.Parameters(BFV["logN"], BFV["Q"], BFV["QMul"], BFV["P"], T)
    params.GenDefaultCRS(seed=777)
    kgen = mkbfv.NewKeyGenerator(params, mkrlwe.HostSampler(np.random.default_rng(31), insecure_test_only=True))
    sampler = mkrlwe.DeviceSampler()
    enc, dec, ev = mkbfv.NewEncryptor(params, sampler=sampler, encoder="device"), mkbfv.NewDecryptor(params, encoder="device"), mkbfv.NewEvaluator(params)
    skSet, pkSet, rlk = mkrlwe.NewSecretKeySet(), mkrlwe.NewPublicKeyKeySet(), mkbfv.RelinearizationKeySet(params)
    rng = np.random.default_rng(5)
    for p in ("user0", "user1"):
        sk, pk = kgen.GenKeyPair(p)
        skSet.AddSecretKey(sk)
        pkSet.AddPublicKey(pk)
        rlk.AddRelinearizationKey(kgen.GenRelinearizationKey(sk, kgen.GenSecretKey(p)))
    a, b = (rng.integers(-(T // 2), T // 2 + 1, N).astype(np.int64) for _ in range(2))
    ca, cb = enc.EncryptMsgNew(mkbfv.Message(a), pkSet.GetPublicKey("user0")), enc.EncryptMsgNew(mkbfv.Message(b), pkSet.GetPublicKey("user1"))
    assert sampler.counter == 2
    assert (dec.Decrypt(ca, skSet).Value == a).all() and (dec.Decrypt(cb, skSet).Value == b).all()          # exact round trip
    assert (dec.Decrypt(ev.MulRelinNew(ca, cb, rlk), skSet).Value == centre(a * b)).all()
    msgs = [mkbfv.Message(a), mkbfv.Message(b)]
    b1, b2 = enc.EncryptMsgBatch(msgs, pkSet.GetPublicKey("user0")), enc.EncryptMsgBatch(msgs, pkSet.GetPublicKey("user0"))
    assert sampler.counter == 4
    for x, y, m in zip(b1, b2, msgs):
        assert (x.download() != y.download()).mean() > 0.99
        assert (dec.Decrypt(x, skSet).Value == m.Value).all() and (dec.Decrypt(y, skSet).Value == m.Value).all()
    params.close()
