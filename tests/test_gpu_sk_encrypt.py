"""Secret-key encryption with a seeded c1 on the device (-m gpu), N = 2^10, bit for bit: mkhe_sample_uniform and polynomial 1 of mkhe_encrypt_sk
against tests/sk_encrypt_model.py (rows on the nQ-based stream pairs), polynomial 0 against (pt + e - D) mod q with D what
mkhe_decrypt_share(flood_bits = 0) writes for the ciphertext (0, c1), mkhe_encrypt_sk_seeded against mkhe_encrypt_sk on the model's kind-1
samples, mkhe_decrypt of the output minus pt against e, mkhe_ct_expand_seeded against polynomial 1 (at fewer limbs: the leading limbs);
determinism and dependence on both keys and both nonces; every refusal followed by a call that works.  The rings of tests/test_gpu_pcks.py --
the three-prime BFV chain, one limb, an mkrlwe 4-prime context used at level 1 (limbs != nQ) -- and the 14 primes of PN15QP880 at count 1.  The
end-to-end tests on mkckks and mkbfv are tests/test_gpu_sk_encrypt_e2e.py."""
import ctypes as C

import numpy as np
import pytest

import device_sampler_model as M
import harness as H
import harness_bfv as HB
import sk_encrypt_model as S

pytestmark = pytest.mark.gpu

A_KEY = [0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0, 0x082EFA98, 0xEC4E6C89]
E_KEY = [0x9E3779B9, 0x7F4A7C15, 0xF39CC060, 0x5CEDC834, 0x1082276B, 0xF3A27251, 0xF86C6A11, 0xD0C18E95]
A_NONCE, E_NONCE = 0x0123456789ABCDEF, 0xFEDCBA9876543210
SENTINEL = 0x7B7B7B7B7B7B7B7B
LOGN = 10
RINGS = {"three": ("bfv", HB.small_bfv(LOGN, 3), 3), "one": ("bfv", HB.small_bfv(LOGN, 1), 1), "low": ("rlwe", H.small_ckks(LOGN, 4), 2)}
ME = "user0"


def key_arg(key):
    return None if key is None else (C.c_uint32 * 8)(*key)


def error():
    from mkhe_kklss_amd._abi import lib
    return lib().mkhe_last_error().decode()


_streams = {}


def stream(key, nonce, s, n):
    """the 64-bit values of one stream as uint64 [n], computed once for the whole module (the numpy keystream: the model test pins it to the
    pure-Python one, and test_the_rings checks a block of it here)"""
    k = (tuple(key), nonce, s, n)
    if k not in _streams:
        _streams[k] = S.stream_values_np(key, nonce, s, n)
    return _streams[k]


class World:
    """a context over one ring (BFV, or mkrlwe used at L limbs), one party with a secret key made on it, and the raw calls"""

    def __init__(self, kind, pset, L):
        from mkhe_kklss_amd import mkbfv, mkrlwe
        from mkhe_kklss_amd._abi import handle_array, lib
        self.mk, self.lib, self.handles, self.N, self.L, self.kind = mkrlwe, lib(), handle_array, 1 << LOGN, L, kind
        smp = mkrlwe.HostSampler(np.random.default_rng(7), insecure_test_only=True)
        if kind == "bfv":
            self.params = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], pset["T"])
            kgen = mkbfv.NewKeyGenerator(self.params, smp)
        else:
            self.params = mkrlwe.Parameters(pset["logN"], pset["Q"], pset["P"])
            kgen = mkrlwe.NewKeyGenerator(self.params, smp)
        self.allQ, self.nQ, self.Q = list(pset["Q"]), len(pset["Q"]), pset["Q"][:L]
        self.rng = np.random.default_rng(2030)
        self.sk = kgen.GenSecretKey(ME)
        self.cdt = mkrlwe.small_cdt(3.2)
        self._pt = {}

    def q(self, limbs=None):
        return np.array(self.allQ[: self.L if limbs is None else limbs], dtype=np.uint64)[:, None]

    def limbs(self, count, L=None):
        return self.mk.DeviceLimbs(self.params, count, self.L if L is None else L)

    def rows(self, count, limbs, key=A_KEY, nonce=A_NONCE, items=None):
        """the model's a: uint64 [count][limbs][N], rows on the nQ-based stream pairs"""
        out = np.zeros((count, limbs, self.N), dtype=np.uint64)
        for b in (range(count) if items is None else items):
            for j in range(limbs):
                out[b, j] = S.uniform_row(key, nonce, b, j, self.nQ, self.allQ[j], self.N, values=stream)
        return out

    def e_model(self, count, key=E_KEY, nonce=E_NONCE):
        """the kind-1 samples of mkhe_encrypt_sk_seeded: int32 [count][N], e_b from stream b"""
        cdt = np.array(self.cdt, dtype=np.uint64)
        out = np.stack([np.searchsorted(cdt, stream(key, nonce, b, self.N), side="right") - len(cdt) // 2 for b in range(count)]).astype(np.int32)
        assert out[0, :8].tolist() == S.e_poly(key, nonce, 0, 8, self.cdt)
        return out

    def e_q(self, e, limbs=None):
        """e mod q_j, canonical: uint64 [count][limbs][N]"""
        q = self.q(limbs)[None]
        e = e.astype(np.int64)[:, None, :]
        return np.where(e < 0, q - np.abs(e).astype(np.uint64), e.astype(np.uint64)).astype(np.uint64)

    def plaintexts(self, count):
        """uniform plaintexts [count][L][N], made once per count: (host coefficient form, device coefficient form, device NTT form)"""
        if count not in self._pt:
            host = np.stack([self.rng.integers(0, q, (count, self.N), dtype=np.uint64) for q in self.Q], axis=1)
            dev, devn = self.limbs(count).upload(host), self.limbs(count)
            self.mk.ntt(self.params, dev, devn)
            self._pt[count] = (host, dev, devn)
        return self._pt[count]

    def outs(self, count, level=None, ids=(ME,)):
        lvl = self.L - 1 if level is None else level
        return [self.mk.Ciphertext(self.params, list(ids), lvl).upload(np.full((1 + len(ids), lvl + 1, self.N), SENTINEL, dtype=np.uint64)) for _ in range(count)]

    # ---- the raw calls
    def sample_uniform(self, count, limbs, key=A_KEY, nonce=A_NONCE, n=None, out=None):
        buf = self.limbs(2 * count, limbs).upload(np.full((2 * count, limbs, self.N), SENTINEL, dtype=np.uint64))
        rc = self.lib.mkhe_sample_uniform(self.params.ctx, limbs, count if n is None else n, key_arg(key), nonce, buf.devptr() if out is None else out(buf))
        got = buf.download()
        if rc == 0:
            assert (got[count:] == SENTINEL).all(), "mkhe_sample_uniform wrote behind uint64[count][limbs][N]"
        else:
            assert (got == SENTINEL).all(), "a refused mkhe_sample_uniform wrote to its output"
        return rc, got[:count]

    def encrypt(self, count, e=None, ntt=False, a_key=A_KEY, a_nonce=A_NONCE, e_key=E_KEY, e_nonce=E_NONCE, level=None, n=None, sk="default", pt="default",
                outs=None, out_list="default", cdt="default", ncdt=None):
        """mkhe_encrypt_sk on host samples e (int32 [count][N]), or mkhe_encrypt_sk_seeded when e is None, into sentinel-filled ciphertexts
        -> (rc, uint64 [count][2][L][N]); a refused call leaves all of them untouched"""
        host, dev, devn = self.plaintexts(count)
        fresh = outs is None
        if fresh:
            outs = self.outs(count)
        head = (self.params.ctx, self.L - 1 if level is None else level, count if n is None else n,
                self.sk.Value.devptr() if sk == "default" else sk, (devn if ntt else dev).devptr() if pt == "default" else pt, 1 if ntt else 0,
                key_arg(a_key), a_nonce)
        hs = self.handles([c.h for c in outs]) if out_list == "default" else out_list(outs)
        if e is None:
            table = (C.c_uint64 * len(self.cdt))(*self.cdt) if cdt == "default" else cdt
            rc = self.lib.mkhe_encrypt_sk_seeded(*head, key_arg(e_key), e_nonce, table, len(self.cdt) if ncdt is None else ncdt, hs)
        else:
            smp = None if isinstance(e, str) else np.ascontiguousarray(e, dtype=np.int32)
            rc = self.lib.mkhe_encrypt_sk(*head, None if smp is None else smp.ctypes.data_as(C.POINTER(C.c_int32)), hs)
        got = [c.download() for c in outs]
        if rc != 0 and fresh:
            assert all((g == SENTINEL).all() for g in got), "a refused encrypt call wrote to its outputs"
        return rc, (np.stack(got) if fresh and rc == 0 else got)

    def product(self, c1):
        """D = what mkhe_decrypt_share(flood_bits = 0) writes for the ciphertexts (0, c1[b]): uint64 [count][L][N]"""
        n = c1.shape[0]
        cts = [self.mk.Ciphertext(self.params, [ME], self.L - 1).upload(np.stack([np.zeros_like(c1[b]), c1[b]])) for b in range(n)]
        buf = self.limbs(n)
        assert self.lib.mkhe_decrypt_share(self.params.ctx, n, self.handles([c.h for c in cts]), (C.c_int * n)(*[1] * n), self.sk.Value.devptr(), None, 0, 0,
                                           buf.devptr()) == 0, error()
        return buf.download()

    def decrypt(self, host_ct):
        """mkhe_decrypt of one uploaded ciphertext [2][L][N] -> uint64 [L][N]"""
        ct = self.mk.Ciphertext(self.params, [ME], self.L - 1).upload(host_ct)
        buf = self.limbs(1)
        assert self.lib.mkhe_decrypt(self.params.ctx, ct.h, self.handles([self.sk.Value.devptr()]), buf.devptr()) == 0, error()
        return buf.download()[0]

    def expand(self, count, limbs, key=A_KEY, nonce=A_NONCE, n=None, outs=None, out_list="default"):
        fresh = outs is None
        if fresh:
            outs = self.outs(count, limbs - 1)
        rc = self.lib.mkhe_ct_expand_seeded(self.params.ctx, count if n is None else n, key_arg(key), nonce,
                                            self.handles([c.h for c in outs]) if out_list == "default" else out_list(outs))
        got = [c.download() for c in outs]
        if rc != 0:
            assert all((g == SENTINEL).all() for g in got), "a refused mkhe_ct_expand_seeded wrote to its outputs"
        return rc, got


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
    assert [world(n).L for n in RINGS] == [3, 1, 2] and [world(n).nQ for n in RINGS] == [3, 1, 4]
    assert [int(v) for v in stream(A_KEY, A_NONCE, 5, 1 << LOGN)[:16]] == M.stream_values(A_KEY, A_NONCE, 5, 16)     # the numpy keystream here


# ------------------------------------------------------------------ kind 6
@pytest.mark.parametrize("count", [1, 3])
def test_sample_uniform_is_the_model(w, count):
    rc, got = w.sample_uniform(count, w.L)
    assert rc == 0, error()
    want = w.rows(count, w.L)
    assert (got == want).all()
    assert (got < w.q()[None]).all() and len({got[b, j].tobytes() for b in range(count) for j in range(w.L)}) == count * w.L
    if w.L > 1:                                                 # fewer limbs: the leading rows (the stream index uses nQ)
        rc, fewer = w.sample_uniform(count, 1)
        assert rc == 0 and (fewer == want[:, :1]).all(), error()
    if w.nQ > w.L:                                              # ... and more, up to nQ
        rc, more = w.sample_uniform(count, w.nQ)
        assert rc == 0 and (more[:, : w.L] == want).all() and (more == w.rows(count, w.nQ)).all(), error()


def test_sample_uniform_seventeen_items_stage_the_pointer_table():
    w = world("one")
    rc, got = w.sample_uniform(17, 1)
    assert rc == 0, error()
    want = w.rows(17, 1, items=(0, 15, 16))
    for b in (0, 15, 16):
        assert (got[b] == want[b]).all(), b
    assert len({got[b].tobytes() for b in range(17)}) == 17


# ------------------------------------------------------------------ the ciphertext
@pytest.mark.parametrize("ntt", [False, True])
@pytest.mark.parametrize("count", [1, 3])
def test_encrypt_sk_is_the_model_row_and_pt_plus_e_minus_the_product(w, count, ntt):
    e = w.rng.integers(-19, 20, (count, w.N)).astype(np.int32)
    rc, got = w.encrypt(count, e=e, ntt=ntt)
    assert rc == 0, error()
    assert (got[:, 1] == w.rows(count, w.L)).all()              # c1 = a, rows on the nQ-based stream pairs (ring "low": limbs != nQ)
    pt, q = w.plaintexts(count)[0], w.q()[None]
    D = w.product(got[:, 1])
    want = (pt + w.e_q(e)) % q
    want = (want + q - D) % q
    assert (got[:, 0] == want).all()
    for b in range(count):                                      # the header's identity: Decrypt gives pt + e exactly
        dec = w.decrypt(got[b])
        assert ((dec + q[0] - pt[b]) % q[0] == w.e_q(e)[b]).all(), b


@pytest.mark.parametrize("ntt", [False, True])
@pytest.mark.parametrize("count", [1, 3])
def test_encrypt_sk_seeded_is_encrypt_sk_on_the_models_samples(w, count, ntt):
    e = w.e_model(count)
    assert np.abs(e).max() <= len(w.cdt) // 2 and e.any()
    rc, seeded = w.encrypt(count, ntt=ntt)
    assert rc == 0, error()
    rc, host = w.encrypt(count, e=e, ntt=ntt)
    assert rc == 0, error()
    assert (seeded == host).all()
    dec = w.decrypt(seeded[count - 1])
    pt, q = w.plaintexts(count)[0], w.q()
    assert ((dec + q - pt[count - 1]) % q == w.e_q(e)[count - 1]).all()


def test_seventeen_items_stage_the_pointer_table():
    w = world("one")
    e = w.e_model(17)
    rc, seeded = w.encrypt(17)
    assert rc == 0, error()
    rc, host = w.encrypt(17, e=e)
    assert rc == 0 and (seeded == host).all(), error()
    want = w.rows(17, 1, items=(0, 16))
    assert (seeded[0, 1] == want[0]).all() and (seeded[16, 1] == want[16]).all()
    pt, q = w.plaintexts(17)[0], w.q()
    assert ((w.decrypt(seeded[16]) + q - pt[16]) % q == w.e_q(e)[16]).all()


def test_the_fourteen_primes_of_pn15qp880():
    w = World("rlwe", H.small_ckks(LOGN, 14), 14)
    assert w.L == 14 and w.nQ == 14 and w.allQ == H.PN15QP880["Q"]
    e = w.e_model(1)
    for ntt in (False, True):
        rc, got = w.encrypt(1, ntt=ntt)
        assert rc == 0, error()
        assert (got[:, 1] == w.rows(1, 14)).all()
        pt, q = w.plaintexts(1)[0], w.q()
        D = w.product(got[:, 1])
        assert (got[0, 0] == ((pt[0] + w.e_q(e)[0]) % q + q - D[0]) % q).all()
        assert ((w.decrypt(got[0]) + q - pt[0]) % q == w.e_q(e)[0]).all()
    w.params.close()


# ------------------------------------------------------------------ the receiver
@pytest.mark.parametrize("count", [1, 3])
def test_expand_reproduces_polynomial_one_and_leaves_polynomial_zero(w, count):
    rc, enc = w.encrypt(count)
    assert rc == 0, error()
    rc, got = w.expand(count, w.L)
    assert rc == 0, error()
    for b in range(count):
        assert (got[b][1] == enc[b, 1]).all() and (got[b][0] == SENTINEL).all(), b
    for limbs in {1, w.L - 1, w.nQ} - {0, w.L}:                 # at fewer limbs the leading limbs; the rows do not depend on the level
        rc, other = w.expand(count, limbs)
        assert rc == 0, error()
        m = min(limbs, w.L)
        for b in range(count):
            assert (other[b][1][:m] == enc[b, 1][:m]).all() and (other[b][0] == SENTINEL).all(), (limbs, b)
        if limbs > w.L:
            assert (np.stack([o[1] for o in other]) == w.rows(count, limbs)).all()


def test_expand_seventeen_items():
    w = world("one")
    rc, got = w.expand(17, 1)
    assert rc == 0, error()
    want = w.rows(17, 1, items=(0, 16))
    assert (got[0][1] == want[0]).all() and (got[16][1] == want[16]).all() and all((g[0] == SENTINEL).all() for g in got)


# ------------------------------------------------------------------ determinism
def test_output_depends_on_both_keys_and_both_nonces(w3):
    w = w3
    base, again = w.encrypt(2), w.encrypt(2)
    assert base[0] == 0 and again[0] == 0 and (base[1] == again[1]).all(), error()
    a = base[1]
    assert (a[0, 1] != a[1, 1]).mean() > 0.99 and (a[0, 0] != a[1, 0]).mean() > 0.99       # items 0 and 1 of one call
    for kw in (dict(a_key=A_KEY[::-1]), dict(a_nonce=A_NONCE + 1)):                        # another a: both polynomials move
        rc, other = w.encrypt(2, **kw)
        assert rc == 0 and (other[:, 1] != a[:, 1]).mean() > 0.99 and (other[:, 0] != a[:, 0]).mean() > 0.99, error()
    for kw in (dict(e_key=E_KEY[::-1]), dict(e_nonce=E_NONCE + 1)):                        # another e: c1 stays, c0 moves by e - e'
        rc, other = w.encrypt(2, **kw)
        assert rc == 0 and (other[:, 1] == a[:, 1]).all(), error()
        diff = (other[:, 0] + w.q()[None] - a[:, 0]) % w.q()[None]
        assert (diff != 0).mean() > 0.5
        e0, e1 = w.e_model(2), w.e_model(2, key=kw.get("e_key", E_KEY), nonce=kw.get("e_nonce", E_NONCE))
        assert (diff == w.e_q(e1 - e0)).all()


# ------------------------------------------------------------------ refusals
def good_call(w):
    """the context works: a seeded encryption that decrypts to pt + e"""
    rc, got = w.encrypt(1)
    assert rc == 0, error()
    pt, q = w.plaintexts(1)[0], w.q()
    assert ((w.decrypt(got[0]) + q - pt[0]) % q == w.e_q(w.e_model(1))[0]).all()


@pytest.mark.parametrize("seeded", [True, False])
def test_encrypt_refusals(w3, seeded):
    w = w3
    name = "mkhe_encrypt_sk_seeded: " if seeded else "mkhe_encrypt_sk: "
    e = None if seeded else np.zeros((2, w.N), dtype=np.int32)
    new = lambda ids, lvl: w.outs(1, lvl, ids)[0]

    def refused(text, count=1, **kw):
        kw.setdefault("e", None if seeded else e[:count])
        rc, _ = w.encrypt(count, **kw)
        assert rc != 0 and error().startswith(name) and text in error() and not any("%08x" % x in error().lower() for x in E_KEY + A_KEY), error()
        good_call(w)

    refused("count", n=0)
    refused("count", n=65536)
    refused("level", level=-1)
    refused("level", level=3)
    refused("aligned", sk=C.c_void_p(w.sk.Value.devptr().value + 8))
    refused("aligned", pt=C.c_void_p(w.plaintexts(1)[1].devptr().value + 8))
    refused("null", sk=None)
    refused("null", pt=None)
    refused("null", a_key=None)
    refused("null", out_list=lambda outs: None)
    refused("null", out_list=lambda outs: w.handles([None]))
    refused("exactly one party", outs=[new([ME, "user1"], w.L - 1)])
    refused("exactly one party", outs=[new([], w.L - 1)])
    refused("level+1 limbs", outs=[new([ME], 1)])
    refused("distinct", count=2, outs=[new([ME], w.L - 1)] * 2)
    if seeded:
        refused("null key", e_key=None)
        refused("must differ from e_key", a_key=E_KEY)
        refused("null table", cdt=None)
        refused("ncdt", ncdt=3)
        refused("ncdt", ncdt=0)
        refused("ncdt", ncdt=66)
        assert w.lib.mkhe_encrypt_sk_seeded(None, 0, 1, None, None, 0, key_arg(A_KEY), 0, key_arg(E_KEY), 0, None, 0, None) != 0
    else:
        refused("null", e="null")
        assert w.lib.mkhe_encrypt_sk(None, 0, 1, None, None, 0, key_arg(A_KEY), 0, None, None) != 0
    assert error() == name + "null context"


def test_sampler_and_expand_refusals(w3):
    w = w3

    def refused(call, name, text):
        rc, _ = call()
        assert rc != 0 and error().startswith(name) and text in error(), error()
        good_call(w)

    su, ex = "mkhe_sample_uniform: ", "mkhe_ct_expand_seeded: "
    refused(lambda: w.sample_uniform(1, 3, n=0), su, "count")
    refused(lambda: w.sample_uniform(1, 3, n=65536), su, "count")
    refused(lambda: w.sample_uniform(1, 3, key=None), su, "null key")
    refused(lambda: w.sample_uniform(1, 3, out=lambda buf: None), su, "null")
    refused(lambda: w.sample_uniform(1, 3, out=lambda buf: C.c_void_p(buf.devptr().value + 8)), su, "aligned")
    for limbs in (0, 4):
        assert w.lib.mkhe_sample_uniform(w.params.ctx, limbs, 1, key_arg(A_KEY), 0, w.limbs(1).devptr()) != 0 and "limbs" in error()
    good_call(w)
    assert w.lib.mkhe_sample_uniform(None, 1, 1, key_arg(A_KEY), 0, None) != 0 and error() == su + "null context"
    refused(lambda: w.expand(1, 3, n=0), ex, "count")
    refused(lambda: w.expand(1, 3, key=None), ex, "null key")
    refused(lambda: w.expand(1, 3, out_list=lambda outs: None), ex, "null")
    refused(lambda: w.expand(1, 3, out_list=lambda outs: w.handles([None])), ex, "null")
    refused(lambda: w.expand(1, 3, outs=w.outs(1, 2, (ME, "user1"))), ex, "exactly one party")
    refused(lambda: w.expand(2, 3, outs=w.outs(1, 2) + w.outs(1, 1)), ex, "same level")
    refused(lambda: w.expand(2, 3, outs=w.outs(1, 2) * 2), ex, "distinct")
    assert w.lib.mkhe_ct_expand_seeded(None, 1, key_arg(A_KEY), 0, None) != 0 and error() == ex + "null context"


def test_refused_on_a_context_that_owns_a_subset_of_the_moduli():
    w = world("low")
    own = (C.c_int * 2)(0, 2)
    assert w.lib.mkhe_ctx_set_owned(w.params.ctx, own, 2) == 0, error()
    try:
        for e, name in ((None, "mkhe_encrypt_sk_seeded: "), (np.zeros((1, w.N), dtype=np.int32), "mkhe_encrypt_sk: ")):
            rc, _ = w.encrypt(1, e=e)
            assert rc != 0 and error().startswith(name) and "subset of the moduli" in error()
        rc, _ = w.sample_uniform(1, w.L)
        assert rc != 0 and error().startswith("mkhe_sample_uniform: ") and "subset of the moduli" in error()
        rc, _ = w.expand(1, w.L)
        assert rc != 0 and error().startswith("mkhe_ct_expand_seeded: ") and "subset of the moduli" in error()
    finally:
        assert w.lib.mkhe_ctx_set_owned(w.params.ctx, own, 0) == 0
    good_call(w)


def test_encrypt_refused_inside_a_capture(w3):
    """(where the runtime of this process can capture at all: tests/test_gpu_cnn.py)"""
    from mkhe_kklss_amd._abi import MkheError
    w = w3
    outs = w.outs(1)
    cdt = (C.c_uint64 * len(w.cdt))(*w.cdt)
    e = np.zeros((1, w.N), dtype=np.int32)
    head = (w.params.ctx, w.L - 1, 1, w.sk.Value.devptr(), w.plaintexts(1)[1].devptr(), 0, key_arg(A_KEY), 1)
    try:
        with w.params.Capture():
            rc0 = w.lib.mkhe_encrypt_sk_seeded(*head, key_arg(E_KEY), 1, cdt, len(w.cdt), w.handles([outs[0].h]))
            msg0 = error()
            rc1 = w.lib.mkhe_encrypt_sk(*head, e.ctypes.data_as(C.POINTER(C.c_int32)), w.handles([outs[0].h]))
            msg1 = error()
        assert rc0 != 0 and msg0.startswith("mkhe_encrypt_sk_seeded: ") and "capture" in msg0
        assert rc1 != 0 and msg1.startswith("mkhe_encrypt_sk: ") and "capture" in msg1
        print("capture: both encrypt calls were refused inside a capture")
    except MkheError as e:
        print("capture: mkhe_capture_begin refused in this process (%s): the refusal inside a capture did not run" % e)
        import gc
        gc.enable()                 # (Graph.__enter__ switched the collector off before the refusal)
        assert "cannot end a multi-stream capture" in str(e)
    assert (outs[0].download() == SENTINEL).all()
    good_call(w)
