"""The protocol merges past 16 parties on the device (-m gpu), N = 2^10, bit for bit: mkhe_decrypt_merge, mkhe_refresh_merge, mkhe_e2s_merge,
mkhe_bfv_refresh_merge and mkhe_pcks_merge over 16, 17 and 32 parties -- the last share table that travels in the kernel arguments, the first
one that is staged in the context's pointer scratch, and the ceiling of the C ABI -- and one call per merge with 17 items over 17 parties, in
which EVERY table of the call is staged, each at its own offset of the scratch.  The merges are pure arithmetic on their inputs and need no
keys: the ciphertexts, the shares and the re-encryptions are uniform host arrays, every one of them different, so that a table that reads
entry 0 twice, stops at entry 15 or starts at the wrong offset changes the result.  The references are the Python-integer models
(tests/refresh_model.py, tests/bfv_refresh_model.py, tests/pcks_model.py, and sum_model below for the plain sums).

On either side of the 16 / 17 boundary, per merge:
  mkhe_decrypt_merge       test_decrypt_merge_is_the_sum[16-1]                          test_decrypt_merge_is_the_sum[17-1]
  mkhe_refresh_merge       test_refresh_merge_is_the_integer_model[16-1-2-3]            test_refresh_merge_is_the_integer_model[17-1-2-3]
  mkhe_e2s_merge           test_e2s_merge_is_the_lift_of_the_refresh_merge[16-1]        test_e2s_merge_is_the_lift_of_the_refresh_merge[17-1]
  mkhe_bfv_refresh_merge   test_bfv_refresh_merge_is_the_integer_model[16-1]            test_bfv_refresh_merge_is_the_integer_model[17-1]
  mkhe_pcks_merge          test_pcks_merge_is_the_model_and_its_first_half_the_decrypt_merge[16-1]   ...[17-1]
and the all-staged call of each is the case [17-17] (refresh: [17-17-2-3], 289 re-encryptions behind 17 + 17 + 17 entries).

Further: every residue at q_j - 1 over 32 parties (an unreduced 64-bit sum wraps from the 17th addend on under the 60-bit prime); the sum R of
a refresh merge over 32 parties placed around (Q - 1) / 2 and on the rounding boundaries of down; the refusals at the ceiling; real shares
of 17 and 32 generated keys against mkhe_decrypt; the refresh of mkckks and of mkbfv with 17 parties; the capture rules of the calls that can
stage a table; floods of 961, 1023 and 1024 bits (sixteen keystream words) on mkhe_pcks_share over eighteen 60-bit primes, and the widest flood
a BFV context can take at all (942 bits on sixteen primes: the per-context bound, not the 1024 of the header, is what binds there); the sampler
rows of N = 2^12 (four workgroups a row), outside and inside a capture.

Every case takes a few seconds at the most, and nearly all of that is the Python-integer models (a CRT and a division per coefficient and
item, a sum per coefficient and party) and the pure-Python ChaCha20 blocks; the device side of a case is a handful of launches."""
import ctypes as C

import numpy as np
import pytest

import bfv_refresh_model as B
import decrypt_share_model as D
import device_sampler_model as M
import harness as H
import harness_bfv as HB
import pcks_model as P
import refresh_model as R
import sk_encrypt_model as S
from gpu_common import CHAIN, digits_neighbours, error, prime_below

pytestmark = pytest.mark.gpu

SENTINEL = 0x7B7B7B7B7B7B7B7B
LOGN, NQ = 10, len(CHAIN)
PARTIES = ["p%02d" % i for i in range(32)]       # (sorted as strings: slot 1 + i is party i)
RECIPIENT = "zed"
# the last inline share table, the first staged one, the ceiling; and every table of the call staged
CASES = [(k, count) for k in (16, 17, 32) for count in (1, 2)] + [(17, 17)]
MERGES = ["decrypt", "refresh", "e2s", "bfv_refresh", "pcks"]


def checked_items(count):
    """the model is Python integers: every item of a small batch, three of a large one, the first and the last among them"""
    return list(range(count)) if count <= 2 else [0, count // 2, count - 1]


def sum_model(c0, addends, moduli):
    """(c0 + the addends) mod q_j in Python integers (object arrays: nothing wraps): [limbs][N] each -> uint64 [limbs][N]"""
    q = np.array([int(m) for m in moduli[: c0.shape[0]]], dtype=object)[:, None]
    acc = np.asarray(c0).astype(object)
    for s in addends:
        acc = acc + np.asarray(s).astype(object)
    return (acc % q).astype(np.uint64)


class World:
    """a context (mkrlwe over CHAIN, or the three-prime BFV ring of tests/test_gpu_bfv_refresh.py) and the five merges as raw calls on host
    arrays.  Outputs are filled with a sentinel; raw output buffers are one item longer than the call may write."""

    def __init__(self, bfv):
        from mkhe_kklss_amd import mkbfv, mkrlwe
        from mkhe_kklss_amd._abi import handle_array, lib
        self.mk, self.lib, self.handles, self.N, self.bfv = mkrlwe, lib(), handle_array, 1 << LOGN, bfv
        if bfv:
            p = HB.small_bfv(LOGN, 3)
            self.params, self.Q, self.T = mkbfv.Parameters(p["logN"], p["Q"], p["QMul"], p["P"], p["T"]), list(p["Q"]), p["T"]
        else:
            self.params, self.Q, self.T = mkrlwe.Parameters(LOGN, CHAIN, H.PN15QP880["P"]), list(CHAIN), 1
        self.params.AddCRS(0, seed=99)
        self.rng = np.random.default_rng(2031)
        self._keys = {}

    def uniform(self, head, limbs):
        return np.stack([self.rng.integers(0, q, tuple(head) + (self.N,), dtype=np.uint64) for q in self.Q[:limbs]], axis=len(head))

    def q(self, limbs):
        return np.array(self.Q[:limbs], dtype=np.uint64)[:, None]

    def keys(self, who):
        """(sk, pk) of a party, generated once"""
        if who not in self._keys:
            kgen = self.mk.NewKeyGenerator(self.params, self.mk.HostSampler(np.random.default_rng(7 + len(self._keys)), insecure_test_only=True))
            self._keys[who] = kgen.GenKeyPair(who)
        return self._keys[who]

    def ct(self, ids, host):
        return self.mk.Ciphertext(self.params, list(ids), host.shape[1] - 1).upload(host)

    def sentinel_ct(self, ids, limbs):
        return self.ct(ids, np.full((1 + len(ids), limbs, self.N), SENTINEL, dtype=np.uint64))

    def limbs(self, host):
        return self.mk.DeviceLimbs(self.params, host.shape[0], host.shape[1]).upload(host)

    def out_buffer(self, count, limbs):
        return self.limbs(np.full((count + 1, limbs, self.N), SENTINEL, dtype=np.uint64))

    def read_buffer(self, buf, count, rc, name):
        got = buf.download()
        if rc == 0:
            assert (got[count:] == SENTINEL).all(), name + " wrote behind uint64[count][limbs][N]"
        else:
            assert (got == SENTINEL).all(), "a refused " + name + " wrote to its output"
        return got[:count]

    def read_cts(self, outs, rc, name):
        got = [c.download() for c in outs]
        if rc != 0:
            assert all((g == SENTINEL).all() for g in got), "a refused " + name + " wrote to its outputs"
        return got

    # ---- the raw calls: cts = device ciphertexts over the same ids, shares = one host array per share of the call (the call is given len(shares))
    def decrypt_merge(self, cts, shares):
        n, L = len(cts), cts[0].Level() + 1
        bufs, out = [self.limbs(s) for s in shares], self.out_buffer(n, L)
        rc = self.lib.mkhe_decrypt_merge(self.params.ctx, n, self.handles([c.h for c in cts]), len(bufs), self.handles([b.devptr() for b in bufs]), out.devptr())
        return rc, self.read_buffer(out, n, rc, "mkhe_decrypt_merge")

    def e2s_merge(self, cts, shares, lout):
        n = len(cts)
        bufs, out = [self.limbs(s) for s in shares], self.out_buffer(n, lout)
        rc = self.lib.mkhe_e2s_merge(self.params.ctx, n, self.handles([c.h for c in cts]), len(bufs), self.handles([b.devptr() for b in bufs]), lout, out.devptr())
        return rc, self.read_buffer(out, n, rc, "mkhe_e2s_merge")

    def refresh_merge(self, cts, shares, reenc, lout):
        """reenc: one host array [count][2][lout][N] per share, for the party at that slot (a share beyond the parties re-encrypts for the last)"""
        n, ids = len(cts), cts[0].ids
        bufs = [self.limbs(s) for s in shares]
        res = [self.ct([ids[min(i, len(ids) - 1)]], r[b]) for i, r in enumerate(reenc) for b in range(n)]
        outs = [self.sentinel_ct(ids, lout) for _ in range(n)]
        fn, name = (self.lib.mkhe_bfv_refresh_merge, "mkhe_bfv_refresh_merge") if self.bfv else (self.lib.mkhe_refresh_merge, "mkhe_refresh_merge")
        rc = fn(self.params.ctx, n, self.handles([c.h for c in cts]), len(bufs), self.handles([b.devptr() for b in bufs]), self.handles([c.h for c in res]),
                self.handles([c.h for c in outs]))
        return rc, self.read_cts(outs, rc, name)

    def pcks_merge(self, cts, shares):
        """shares: host arrays [count][2][L][N]"""
        n, L = len(cts), cts[0].Level() + 1
        bufs = [self.limbs(np.ascontiguousarray(s).reshape(2 * n, L, self.N)) for s in shares]
        outs = [self.sentinel_ct([RECIPIENT], L) for _ in range(n)]
        rc = self.lib.mkhe_pcks_merge(self.params.ctx, n, self.handles([c.h for c in cts]), len(bufs), self.handles([b.devptr() for b in bufs]),
                                      self.handles([c.h for c in outs]))
        return rc, self.read_cts(outs, rc, "mkhe_pcks_merge")


_worlds = {}


def world(bfv):
    if bfv not in _worlds:
        _worlds[bfv] = World(bfv)
    return _worlds[bfv]


@pytest.fixture(scope="module")
def ck():
    return world(False)


@pytest.fixture(scope="module")
def bf():
    return world(True)


def run_merge(name, k, count, nshares=None, lin=NQ, lout=NQ, top=False):
    """one call of a merge on uniform inputs over k parties (top: c_0 and every share at q_j - 1), given nshares shares (default k)
    -> (rc, the outputs per item, model(b) -> what item b must be)"""
    w = world(name == "bfv_refresh")
    ids, ns = PARTIES[:k], k if nshares is None else nshares
    host = w.uniform((count, 1 + k), lin)
    half = (2,) if name == "pcks" else ()
    shares = [w.uniform((count,) + half, lin) for _ in range(ns)]
    if top:
        host[:, 0] = w.q(lin) - np.uint64(1)
        shares = [np.broadcast_to(w.q(lin) - np.uint64(1), s.shape).copy() for s in shares]
    cts = [w.ct(ids, host[b]) for b in range(count)]
    if name == "decrypt":
        rc, got = w.decrypt_merge(cts, shares)
        return rc, got, lambda b: sum_model(host[b, 0], [s[b] for s in shares], w.Q)
    if name == "e2s":
        rc, got = w.e2s_merge(cts, shares, lout)
        return rc, got, lambda b: R.merge(w.Q, lin, lout, host[b, 0], [s[b] for s in shares], [])[0]
    if name == "pcks":
        rc, got = w.pcks_merge(cts, shares)
        return rc, got, lambda b: np.stack([sum_model(host[b, 0], [s[b, 0] for s in shares], w.Q),
                                            sum_model(np.zeros_like(host[b, 0]), [s[b, 1] for s in shares], w.Q)])
    reenc = [w.uniform((count, 2), lout) for _ in range(ns)]
    rc, got = w.refresh_merge(cts, shares, reenc, lout)
    if name == "refresh":
        return rc, got, lambda b: R.merge(w.Q, lin, lout, host[b, 0], [s[b] for s in shares], [r[b] for r in reenc])
    return rc, got, lambda b: B.merge(w.Q, w.T, host[b, 0], [s[b] for s in shares], [r[b] for r in reenc])


def assert_merge(name, k, count, **kw):
    rc, got, model = run_merge(name, k, count, **kw)
    assert rc == 0, error()
    for b in checked_items(count):
        assert (got[b] == model(b)).all(), (name, k, count, b)
    return got


def test_the_chain_and_the_wrap():
    assert [q % (1 << (LOGN + 1)) for q in CHAIN] == [1] * 3 and (1 << 59) < CHAIN[0] < (1 << 60) and CHAIN[1] < (1 << 45) and CHAIN[2] < (1 << 31)
    assert 16 * (CHAIN[0] - 1) < 1 << 64 <= 17 * (CHAIN[0] - 1)          # an unreduced 64-bit sum holds 16 addends and wraps at the 17th
    assert PARTIES == sorted(PARTIES)


# ------------------------------------------------------------------ the merges as pure functions
@pytest.mark.parametrize("k,count", CASES)
def test_decrypt_merge_is_the_sum(k, count):
    assert_merge("decrypt", k, count)


@pytest.mark.parametrize("k,count,lin,lout", [(k, c, lin, lout) for lin, lout in ((1, NQ), (2, NQ), (2, 2), (2, 1)) for k, c in CASES[:-1]] + [(17, 17, 2, NQ)])
def test_refresh_merge_is_the_integer_model(k, count, lin, lout):
    """polynomial 0 is the lift plus the sum of the c0 of the re-encryptions; polynomial 1 + i is the c1 of re-encryption i: a permuted table fails"""
    assert_merge("refresh", k, count, lin=lin, lout=lout)


@pytest.mark.parametrize("k,count", CASES)
def test_e2s_merge_is_the_lift_of_the_refresh_merge(ck, k, count):
    w, lin, lout = ck, 2, NQ
    got = assert_merge("e2s", k, count, lin=lin, lout=lout)
    assert got.shape == (count, lout, w.N)
    if k > 16 and count <= 2:                                   # polynomial 0 of mkhe_refresh_merge with zero re-encryptions, on the same inputs
        host, shares = w.uniform((count, 1 + k), lin), [w.uniform((count,), lin) for _ in range(k)]
        cts = [w.ct(PARTIES[:k], host[b]) for b in range(count)]
        rc, pt = w.e2s_merge(cts, shares, lout)
        assert rc == 0, error()
        rc, full = w.refresh_merge(cts, shares, [np.zeros((count, 2, lout, w.N), dtype=np.uint64)] * k, lout)
        assert rc == 0, error()
        for b in range(count):
            assert (full[b][0] == pt[b]).all() and not full[b][1:].any(), b


@pytest.mark.parametrize("k,count", CASES)
def test_bfv_refresh_merge_is_the_integer_model(k, count):
    """all 1 + k polynomials: up(down(c_0 + the shares)) + the c0 of the re-encryptions, and their c1 in slot order"""
    assert_merge("bfv_refresh", k, count)


@pytest.mark.parametrize("k,count", CASES)
def test_pcks_merge_is_the_model_and_its_first_half_the_decrypt_merge(ck, k, count):
    w = ck
    host, shares = w.uniform((count, 1 + k), NQ), [w.uniform((count, 2), NQ) for _ in range(k)]
    cts = [w.ct(PARTIES[:k], host[b]) for b in range(count)]
    rc, got = w.pcks_merge(cts, shares)
    assert rc == 0, error()
    for b in checked_items(count):
        assert (got[b] == P.merge(w.Q, host[b, 0], [s[b] for s in shares])).all(), b
        assert (got[b][0] == sum_model(host[b, 0], [s[b, 0] for s in shares], w.Q)).all(), b
    rc, pt = w.decrypt_merge(cts, [np.ascontiguousarray(s[:, 0]) for s in shares])
    assert rc == 0, error()
    assert all((got[b][0] == pt[b]).all() for b in range(count))


# ------------------------------------------------------------------ inputs made to fail
@pytest.mark.parametrize("name", MERGES)
def test_every_residue_at_the_top_of_its_modulus_over_32_parties(name):
    """c_0 and all 32 shares at q_j - 1: 33 (q - 1) = -33 mod q, and under the 60-bit prime a sum that is not reduced on the way wraps 2^64"""
    got = assert_merge(name, 32, 1, top=True)
    w = world(name == "bfv_refresh")
    if name in ("decrypt", "pcks"):
        first = got[0] if name == "decrypt" else got[0][0]
        assert (first == w.q(NQ) - np.uint64(33)).all()
    if name == "pcks":
        assert (got[0][1] == w.q(NQ) - np.uint64(32)).all()


def solve_share(w, host0, others, targets, limbs):
    """share 0 such that c_0 + share 0 + the others has the residues of targets[i] at coefficient i (uniform elsewhere)"""
    share = w.uniform((1,), limbs)
    rest = sum_model(host0, [s[0] for s in others], w.Q)
    for j, q in enumerate(w.Q[:limbs]):
        share[0, j, : len(targets)] = [(x - int(rest[j, i])) % q for i, x in enumerate(targets)]
    return share


@pytest.mark.parametrize("lin", [1, 2, 3])
def test_refresh_merge_over_32_parties_lifts_exactly_around_half_q(ck, lin):
    """the crafted R of test_merge_lifts_exactly_around_half_q as the sum of c_0 and 32 shares, 31 of them uniform; the re-encryptions uniform"""
    w, k, lout = ck, 32, NQ
    xs, Q = digits_neighbours(lin)
    host = w.uniform((1 + k,), lin)
    others = [w.uniform((1,), lin) for _ in range(k - 1)]
    shares = [solve_share(w, host[0], others, xs, lin)] + others
    reenc = [w.uniform((1, 2), lout) for _ in range(k)]
    rc, got = w.refresh_merge([w.ct(PARTIES[:k], host)], shares, reenc, lout)
    assert rc == 0, error()
    for i, x in enumerate(xs):
        lifted = x if x <= (Q - 1) // 2 else x - Q
        assert [int(got[0][0, j, i]) for j in range(lout)] == [(lifted + sum(int(r[0, 0, j, i]) for r in reenc)) % q for j, q in enumerate(w.Q[:lout])], (i, x)
    assert (got[0] == R.merge(w.Q, lin, lout, host[0], [s[0] for s in shares], [r[0] for r in reenc])).all()


def test_bfv_refresh_merge_over_32_parties_rounds_exactly_at_the_boundaries(bf):
    """the crafted R of test_merge_rounds_exactly_at_the_boundaries as the sum of c_0 and 32 shares, 31 of them uniform"""
    w, k = bf, 32
    Q, T, L = B.q_product(w.Q), w.T, len(w.Q)
    Rs, ws = [0, Q - 1], [0, 0]
    for x in (0, 1, T // 2, T - 1):
        edge = (2 * x + 1) * Q // (2 * T)
        Rs += [edge, edge + 1]
        ws += [x, (x + 1) % T]
    assert [B.down(r, w.Q, T) for r in Rs] == ws
    host = w.uniform((1 + k,), L)
    others = [w.uniform((1,), L) for _ in range(k - 1)]
    shares = [solve_share(w, host[0], others, Rs, L)] + others
    reenc = [w.uniform((1, 2), L) for _ in range(k)]
    rc, got = w.refresh_merge([w.ct(PARTIES[:k], host)], shares, reenc, L)
    assert rc == 0, error()
    for i, x in enumerate(ws):
        assert [int(got[0][0, j, i]) for j in range(L)] == [(B.up(x, w.Q, T) + sum(int(r[0, 0, j, i]) for r in reenc)) % q for j, q in enumerate(w.Q)], (i, Rs[i])
    assert (got[0] == B.merge(w.Q, T, host[0], [s[0] for s in shares], [r[0] for r in reenc])).all()


# ------------------------------------------------------------------ refusals at the ceiling
@pytest.mark.parametrize("name", MERGES)
def test_a_share_too_many_or_too_few_is_refused_and_nothing_is_written(name):
    fn = {"decrypt": "mkhe_decrypt_merge", "refresh": "mkhe_refresh_merge", "e2s": "mkhe_e2s_merge", "bfv_refresh": "mkhe_bfv_refresh_merge",
          "pcks": "mkhe_pcks_merge"}[name]
    for k, nshares in ((32, 33), (17, 16), (17, 18)):
        rc, _, _ = run_merge(name, k, 1, nshares=nshares)       # (the callers assert that a refused call left the sentinel everywhere)
        assert rc != 0 and error().startswith(fn + ": ") and "nshares must be the number of parties" in error(), (k, nshares, error())
        assert_merge(name, 17, 1)                               # the context works


# ------------------------------------------------------------------ real shares, past the boundary
@pytest.mark.parametrize("k", [17, 32])
def test_shares_of_generated_keys_merge_to_what_decrypt_gives_with_every_key(ck, k):
    """mkhe_decrypt_share(flood_bits = 0) of every party, merged, is mkhe_decrypt with all the keys (include/mkhe.h): through the Python mirror"""
    w = ck
    ids = PARTIES[:k]
    ct = w.ct(ids, w.uniform((1 + k,), NQ))
    dec, sks = w.mk.NewDecryptor(w.params), w.mk.NewSecretKeySet()
    for p in ids:
        sks.AddSecretKey(w.keys(p)[0])
    want = dec.Decrypt(ct, sks).download()
    shares = [dec.ShareNew(ct, w.keys(p)[0], 0, None) for p in reversed(ids)]
    assert len({s.download().tobytes() for s in shares}) == k
    got = dec.MergeShares(ct, shares).download()
    assert (got == want).all()
    assert (got[0] == sum_model(ct.download()[0], [s.download()[0] for s in shares], w.Q)).all()


def _max_err(a, b):
    d = np.abs(np.asarray(a) - np.asarray(b))
    return float(max(d.real.max(), d.imag.max()))


def test_seventeen_parties_refresh_an_mkckks_ciphertext():
    """tests/test_gpu_refresh_e2e.py with 17 parties: the refresh moves a slot by at most RefreshSlotBound(17, scale),
    and the message is still within the precision of a fresh encryption of it (Scenario.precision_bound) plus that term"""
    import types
    from mkhe_kklss_amd import mkckks, mkrlwe
    from scenario import Scenario
    k, pset = 17, H.small_ckks(LOGN, nq=4)
    scale, n, names = pset["scale"], 1 << (LOGN - 1), PARTIES[:17]
    params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], scale)
    params.GenDefaultCRS(seed=4321)
    kgen = mkrlwe.NewKeyGenerator(params, mkrlwe.HostSampler(np.random.default_rng(2026), insecure_test_only=True))
    enc, dec, ev, ref = mkckks.NewEncryptor(params, sampler=mkrlwe.DeviceSampler()), mkckks.NewDecryptor(params), mkckks.NewEvaluator(params), mkckks.NewRefresher(params)
    rng = np.random.default_rng(41)
    z = rng.uniform(0.5, 1.0, n) * np.exp(2j * np.pi * rng.uniform(0, 1, n))
    sks, pks, skSet, ct = {}, {}, mkrlwe.NewSecretKeySet(), None
    for p in names:
        sks[p], pks[p] = kgen.GenKeyPair(p)
        skSet.AddSecretKey(sks[p])
        c = enc.EncryptMsgNew(mkckks.Message(z / k), pks[p])
        ct = c if ct is None else ev.AddNew(ct, c)
    ct = ev.DropLevelNew(ct, 2)
    assert ct.Level() == 1 and ct.ids == names
    before = dec.Decrypt(ct, skSet).Value
    assert np.abs(before).max() <= 1.0 + 1e-6                   # (what MaxMaskBits is told: no slot above 1)
    bits = ref.MaxMaskBits(k, 1, ct.Scale)
    shares = [ref.ShareNew(ct, sks[p], pks[p], bits, mkrlwe.DeviceSampler()) for p in reversed(names)]
    res = ref.MergeNew(ct, shares)
    assert res.Level() == 3 and res.Scale == ct.Scale and res.ids == ct.ids
    after = dec.Decrypt(res, skSet).Value
    slot_bound, err = ref.RefreshSlotBound(k, ct.Scale), _max_err(after, before)
    tol = 2.0 ** Scenario.precision_bound(types.SimpleNamespace(scale=scale, logN=LOGN), np.log2(k)) + slot_bound      # k fresh encryptions, then the refresh
    print("17 parties, mask_bits %d: the refresh moved a slot by at most %.3g (bound %.3g); off the message by %.3g (bound %.3g)"
          % (bits, err, slot_bound, _max_err(after, z), tol))
    assert bits >= 1 and err <= slot_bound
    assert _max_err(after, z) <= tol
    params.close()


def test_seventeen_parties_refresh_an_mkbfv_ciphertext_exactly():
    from mkhe_kklss_amd import mkbfv, mkrlwe
    k, pset = 17, HB.small_bfv(LOGN, 3)
    N, T, names = 1 << LOGN, pset["T"], PARTIES[:17]
    params = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], T)
    params.GenDefaultCRS(seed=4322)
    kgen = mkbfv.NewKeyGenerator(params, mkrlwe.HostSampler(np.random.default_rng(2027), insecure_test_only=True))
    enc, dec, ev = mkbfv.NewEncryptor(params, sampler=mkrlwe.DeviceSampler(), encoder="device"), mkbfv.NewDecryptor(params, encoder="device"), mkbfv.NewEvaluator(params)
    ref, rng = mkbfv.NewRefresher(params), np.random.default_rng(43)
    sks, pks, skSet, ct, msg = {}, {}, mkrlwe.NewSecretKeySet(), None, np.zeros(N, dtype=np.int64)
    for p in names:
        sks[p], pks[p] = kgen.GenKeyPair(p)
        skSet.AddSecretKey(sks[p])
        m = rng.integers(-(T // 2), T // 2 + 1, N).astype(np.int64)
        c = enc.EncryptMsgNew(mkbfv.Message(m), pks[p])
        ct, msg = (c if ct is None else ev.AddNew(ct, c)), msg + m
    want = np.mod(msg, T)
    want = np.where(want > T // 2, want - T, want)
    assert ct.ids == names and (dec.Decrypt(ct, skSet).Value == want).all()
    # the widest flood that leaves half of the margin Q / (2 T) to the noise of the input, which here is that of 17 fresh encryptions
    bits = ref.MaxFloodBits(k)
    assert bits == B.max_flood_bits(pset["Q"], T, k) and k * (2 * N + 1) * 19 < B.q_product(pset["Q"]) // (4 * T)
    shares = [ref.ShareNew(ct, sks[p], pks[p], bits, mkrlwe.DeviceSampler()) for p in reversed(names)]
    fresh = ref.MergeNew(ct, shares)
    assert fresh.ids == ct.ids and (dec.Decrypt(fresh, skSet).Value == want).all()
    params.close()


# ------------------------------------------------------------------ the capture rules of the calls that can stage a table
def test_inside_a_capture_the_staged_merges_and_shares_are_refused_and_the_inline_ones_are_recorded(ck):
    """(where the runtime of this process can capture at all: tests/test_gpu_cnn.py)  Every shape has run once outside the capture, so that no
    scratch grows inside it (include/mkhe.h)."""
    from mkhe_kklss_amd._abi import MkheError
    w, L = ck, NQ
    sk = w.keys(PARTIES[0])[0]

    def merge_inputs(k, count, half=()):
        host, shares = w.uniform((count, 1 + k), L), [w.uniform((count,) + half, L) for _ in range(k)]
        cts = [w.ct(PARTIES[:k], host[b]) for b in range(count)]
        bufs = [w.limbs(np.ascontiguousarray(s).reshape(-1, L, w.N)) for s in shares]
        return host, shares, w.handles([c.h for c in cts]), w.handles([b.devptr() for b in bufs]), (cts, bufs)

    ctx, lib = w.params.ctx, w.lib
    a17, a2, a16 = merge_inputs(17, 1), merge_inputs(2, 17), merge_inputs(16, 16)
    p17, p16 = merge_inputs(17, 1, (2,)), merge_inputs(16, 2, (2,))
    o17, o2, o16, oshare, odec = w.out_buffer(1, L), w.out_buffer(17, L), w.out_buffer(16, L), w.out_buffer(17, L), w.out_buffer(1, L)
    q17, q16 = [w.sentinel_ct([RECIPIENT], L)], [w.sentinel_ct([RECIPIENT], L) for _ in range(2)]
    h17, h16 = w.handles([c.h for c in q17]), w.handles([c.h for c in q16])
    slots, sk17 = (C.c_int * 17)(*[1] * 17), w.handles([sk.Value.devptr()] * 17)
    # once outside the capture, into outputs of their own
    warm, wq = w.out_buffer(16, L), [w.sentinel_ct([RECIPIENT], L) for _ in range(2)]
    assert lib.mkhe_decrypt_merge(ctx, 16, a16[2], 16, a16[3], warm.devptr()) == 0, error()
    assert lib.mkhe_pcks_merge(ctx, 2, p16[2], 16, p16[3], w.handles([c.h for c in wq])) == 0, error()
    assert (warm.download()[0] == sum_model(a16[0][0, 0], [s[0] for s in a16[1]], w.Q)).all()
    try:
        with w.params.Capture() as g:
            rc, msg = [], []
            for call in (lambda: lib.mkhe_decrypt_merge(ctx, 1, a17[2], 17, a17[3], o17.devptr()),
                         lambda: lib.mkhe_decrypt_merge(ctx, 17, a2[2], 2, a2[3], o2.devptr()),
                         lambda: lib.mkhe_decrypt_share(ctx, 17, a2[2], slots, sk.Value.devptr(), None, 0, 0, oshare.devptr()),
                         lambda: lib.mkhe_decrypt(ctx, a17[4][0][0].h, sk17, odec.devptr()),
                         lambda: lib.mkhe_pcks_merge(ctx, 1, p17[2], 17, p17[3], h17),
                         lambda: lib.mkhe_decrypt_merge(ctx, 16, a16[2], 16, a16[3], o16.devptr()),
                         lambda: lib.mkhe_pcks_merge(ctx, 2, p16[2], 16, p16[3], h16)):
                rc.append(call())
                msg.append(error())
        for i, fn in enumerate(["mkhe_decrypt_merge", "mkhe_decrypt_merge", "mkhe_decrypt_share", "mkhe_decrypt", "mkhe_pcks_merge"]):
            assert rc[i] != 0 and msg[i].startswith(fn + ": ") and "capture" in msg[i] and "staged" in msg[i], (i, msg[i])
        assert rc[5] == 0 and rc[6] == 0, msg[5:]
        assert (o16.download() == SENTINEL).all() and all((c.download() == SENTINEL).all() for c in q16)     # recorded, not run
        g.launch()
        got = o16.download()
        assert (got[16:] == SENTINEL).all()
        for b in (0, 7, 15):
            assert (got[b] == sum_model(a16[0][b, 0], [s[b] for s in a16[1]], w.Q)).all(), b
        for b in range(2):
            assert (q16[b].download() == P.merge(w.Q, p16[0][b, 0], [s[b] for s in p16[1]])).all(), b
        print("capture: the staged merges, the staged share and the 17-party decrypt were refused, the inline merges replayed")
    except MkheError as e:
        print("capture: mkhe_capture_begin refused in this process (%s): the calls inside a capture did not run" % e)
        import gc
        gc.enable()                 # (Graph.__enter__ switched the collector off before the refusal)
        assert "cannot end a multi-stream capture" in str(e)
    assert all((o.download() == SENTINEL).all() for o in (o17, o2, oshare, odec)) and (q17[0].download() == SENTINEL).all()
    # outside the capture the refused shapes run, and the context is usable
    assert lib.mkhe_decrypt_merge(ctx, 1, a17[2], 17, a17[3], o17.devptr()) == 0, error()
    assert (o17.download()[0] == sum_model(a17[0][0, 0], [s[0] for s in a17[1]], w.Q)).all()
    assert_merge("pcks", 17, 1)


# ------------------------------------------------------------------ the widest flood
def wide_primes(n):
    """the n largest primes = 1 mod 2^11 below 2^60 that are not special primes of the reference's sets"""
    primes, q = [], 1 << 60
    while len(primes) < n:
        q = prime_below(q)
        if q not in HB.BFV_PN15QP880["P"] and q not in H.PN15QP880["P"]:
            primes.append(q)
    assert min(primes) > 1 << 59
    return primes


def wide_flood(e, bits):
    """a flood of `bits` bits fills its range"""
    return max(e).bit_length() >= bits - 8 and -min(e) >> (bits - 8) and all(-(1 << (bits - 1)) <= v < (1 << (bits - 1)) for v in e)


def test_the_widest_flood_of_a_bfv_context_on_the_refresh_and_e2s_shares():
    """A BFV context holds at most 16 primes of Q (the basis conversion), each below 2^60: bitlen(Q div 2T) - 1 is at most 960 - bitlen(2T) = 942, so the 1024
    bits the calls are documented to draw cannot be reached on one, and the per-context bound is the one that binds (include/mkhe.h says so).
    On the widest chain that can be created: a flood of fourteen full words, one bit more, and the widest -- fifteen words, the top one partial."""
    import test_gpu_bfv_e2s as TE
    import test_gpu_bfv_refresh as TB
    from mkhe_kklss_amd import mkbfv
    from mkhe_kklss_amd._abi import MkheError
    primes = wide_primes(34)
    with pytest.raises(MkheError, match="too many primes in Q"):
        mkbfv.Parameters(LOGN, primes[17:], primes[:17], HB.BFV_PN15QP880["P"], HB.BFV_PN15QP880["T"])
    pset = dict(logN=LOGN, Q=primes[16:32], QMul=primes[:16], P=HB.BFV_PN15QP880["P"], T=HB.BFV_PN15QP880["T"])
    most = B.max_flood_bits(pset["Q"], pset["T"], 1)
    assert 14 * 64 + 1 < most < 15 * 64 and B.words(most) == 15 and B.words(14 * 64) == 14
    w, who = TB.World(pset), "user0"
    assert w.L == 16 and w.most == most == w.bfv.NewRefresher(w.params).MaxFloodBits(1)       # the per-context bound is the model's
    cts = [w.ct(TB.USERS[:2])[0]]
    plain, smp = w.decrypt_share(cts, who), w.samples(1)
    for bits in (14 * 64, 14 * 64 + 1, most):
        rc, got, enc = w.share(cts, who, 1, bits)
        assert rc == 0, error()
        A, e = B.mask_poly(TB.KEY, TB.NONCE_MASK, 0, w.N, w.T, bits, values=TB.stream), B.flood_poly(TB.KEY, TB.NONCE_MASK, 0, w.N, bits, values=TB.stream)
        assert wide_flood(e, bits)
        want = (plain[0] + B.share_addend(A, e, w.Q, w.T)) % w.q()
        assert (got[0] == want).all(), bits
        assert (enc == w.encrypt(who, B.reenc_plaintext(A, w.Q, w.T)[None], smp)).all(), bits
        rc, pub, secret = TE.e2s_share(w, cts, who, bits)
        assert rc == 0, error()
        assert (pub[0] == want).all() and (secret[0] == np.array([(w.T - a) % w.T for a in A], dtype=np.uint64)).all(), bits
    for bits, text in ((most + 1, "destroys the message"), (1024, "destroys the message"), (1025, "flood_bits must be 0 .. 1024")):
        rc, _, _ = w.share(cts, who, 1, bits)
        assert rc != 0 and error().startswith("mkhe_bfv_refresh_share: ") and text in error(), (bits, error())
        rc, _, _ = TE.e2s_share(w, cts, who, bits)
        assert rc != 0 and error().startswith("mkhe_bfv_e2s_share: ") and text in error(), (bits, error())
    rc, _, _ = w.share(cts, who, 1, most)
    assert rc == 0, error()
    w.params.close()


def test_floods_of_sixteen_words_on_the_pcks_share():
    """eighteen primes just under 2^60 below the top of an mkrlwe chain of nineteen: bitlen(Q_l div 2) - 1 is above 1024, the cap of sixteen
    keystream words binds -- a partial top word, one bit short, and full"""
    import test_gpu_pcks as TP
    pset = dict(logN=LOGN, Q=wide_primes(19), P=H.PN15QP880["P"])
    room = (B.q_product(pset["Q"][:18]) // 2).bit_length() - 1
    assert room > 1024 and B.words(961) == B.words(1023) == B.words(1024) == 16
    w, who = TP.World("rlwe", pset, 18), "user0"
    assert w.L == 18 and w.most == 1024 == w.mk.PublicKeySwitcher(w.params).MaxFloodBits(17)  # the per-context bound is the model's
    cts = [w.ct(TP.USERS[:2])[0]]
    plain, enc = w.decrypt_share(cts, who), w.encrypt_zero("carol", w.samples(1))
    for bits in (961, 1023, 1024):
        rc, got = w.share(cts, who, "carol", bits)
        assert rc == 0, error()
        E = P.flood_poly(TP.KEY, TP.NONCE, 1, 0, w.N, bits, values=TP.stream)
        assert wide_flood(E, bits)
        h0, h1 = TP.expected(w, plain, enc, {0: D.flood_limbs(E, w.Q)}, 0)
        assert (got[0, 0] == h0).all() and (got[0, 1] == h1).all(), bits
    rc, _ = w.share(cts, who, "carol", 1025)
    assert rc != 0 and error().startswith("mkhe_pcks_share: ") and "flood_bits must be 0 .. 1024" in error()
    rc, _ = w.share(cts, who, "carol", 1024)
    assert rc == 0, error()
    w.params.close()


# ------------------------------------------------------------------ sampler rows longer than one workgroup
LOGN_ROWS = 12
BLOCKS_PER_WORKGROUP = 128                       # one thread a ChaCha20 block of 8 coefficients, 128 threads a workgroup: N = 2^12 is four workgroups a row

_rows_world = []


def rows_world():
    """tests/test_gpu_sk_encrypt.py's world on a ring of N = 2^12 with 3 limbs"""
    import test_gpu_sk_encrypt as TS
    if not _rows_world:
        w = TS.World("rlwe", H.small_ckks(LOGN_ROWS, 3), 3)
        w.N = 1 << LOGN_ROWS
        assert w.params.N() == w.N == 4 * 8 * BLOCKS_PER_WORKGROUP
        _rows_world.append(w)
    return TS, _rows_world[0]


def pin_stream(TS, key, nonce, s, n, whole):
    """the numpy keystream the expected rows are computed from against device_sampler_model's pure Python: the whole stream, or the first and
    the last block of every workgroup"""
    got = TS.stream(key, nonce, s, n)
    w13, w14 = nonce & M.M32, nonce >> 32
    blocks = range(n // 8) if whole else [c for g in range(n // 8 // BLOCKS_PER_WORKGROUP) for c in (g * BLOCKS_PER_WORKGROUP, (g + 1) * BLOCKS_PER_WORKGROUP - 1)]
    for c in blocks:
        o = M.chacha20_block(key, c, w13, w14, s)
        assert [int(v) for v in got[8 * c: 8 * c + 8]] == [o[2 * i] | (o[2 * i + 1] << 32) for i in range(8)], (s, c)


def model_rows(TS, w, count, limbs):
    """the rows of kind 6 for `count` items: uint64 [count][limbs][N]; the streams of the first and the last row pinned whole, the others at the
    edges of the workgroups"""
    for b in range(count):
        for j in range(limbs):
            for s in S.row_streams(b, j, w.nQ):
                pin_stream(TS, TS.A_KEY, TS.A_NONCE, s, w.N, whole=(b, j) in ((0, 0), (count - 1, limbs - 1)))
    return w.rows(count, limbs)


@pytest.mark.parametrize("count", [1, 17])
def test_sample_uniform_and_expand_on_rows_of_four_workgroups(count):
    TS, w = rows_world()
    assert M.stream_values(TS.A_KEY, TS.A_NONCE, 3, 16) == [int(v) for v in TS.stream(TS.A_KEY, TS.A_NONCE, 3, w.N)[:16]]
    want = model_rows(TS, w, count, 3)
    rc, got = w.sample_uniform(count, 3)
    assert rc == 0, error()
    assert (got == want).all() and (got < w.q()[None]).all()
    assert len({got[b, j, 1024 * g: 1024 * g + 1024].tobytes() for b in range(count) for j in range(3) for g in range(4)}) == count * 12
    rc, out = w.expand(count, 3)
    assert rc == 0, error()
    for b in range(count):
        assert (out[b][1] == want[b]).all() and (out[b][0] == SENTINEL).all(), b


@pytest.mark.parametrize("count", [1, 17])
def test_encrypt_sk_seeded_on_rows_of_four_workgroups(count):
    TS, w = rows_world()
    for b in (0, count - 1):
        pin_stream(TS, TS.E_KEY, TS.E_NONCE, b, w.N, whole=True)
    for b in range(1, count - 1):
        pin_stream(TS, TS.E_KEY, TS.E_NONCE, b, w.N, whole=False)
    e = w.e_model(count)
    for b in (0, count - 1):
        assert e[b].tolist() == [M.table(int(r), w.cdt) for r in TS.stream(TS.E_KEY, TS.E_NONCE, b, w.N)]
    rc, seeded = w.encrypt(count)
    assert rc == 0, error()
    rc, host = w.encrypt(count, e=e)
    assert rc == 0 and (seeded == host).all(), error()
    assert (seeded[:, 1] == model_rows(TS, w, count, 3)).all()  # c1 = a
    pt, q = w.plaintexts(count)[0], w.q()[None]
    prod = w.product(seeded[:, 1])
    assert (seeded[:, 0] == ((pt + w.e_q(e)) % q + q - prod) % q).all()
    for b in (0, count - 1):                                     # Decrypt gives pt + e exactly
        assert ((w.decrypt(seeded[b]) + q[0] - pt[b]) % q[0] == w.e_q(e)[b]).all(), b


def test_inside_a_capture_the_public_sampler_calls_are_recorded_and_their_staged_forms_refused():
    """mkhe_sample_uniform and mkhe_ct_expand_seeded read a PUBLIC stream and may be captured while they stage no table (include/mkhe.h); each
    shape has run once outside the capture (the tests above)"""
    from mkhe_kklss_amd._abi import MkheError
    TS, w = rows_world()
    want = model_rows(TS, w, 2, 3)
    rc, _ = w.sample_uniform(2, 3)
    assert rc == 0, error()
    rc, _ = w.expand(2, 3)
    assert rc == 0, error()
    buf, big = (w.limbs(n, 3).upload(np.full((n, 3, w.N), SENTINEL, dtype=np.uint64)) for n in (3, 17))
    outs, outs17 = w.outs(2), w.outs(17)
    h2, h17, key, ctx = w.handles([c.h for c in outs]), w.handles([c.h for c in outs17]), TS.key_arg(TS.A_KEY), w.params.ctx
    try:
        with w.params.Capture() as g:
            rc1 = w.lib.mkhe_sample_uniform(ctx, 3, 17, key, TS.A_NONCE, big.devptr())
            msg1 = error()
            rc2 = w.lib.mkhe_ct_expand_seeded(ctx, 17, key, TS.A_NONCE, h17)
            msg2 = error()
            rc3 = w.lib.mkhe_sample_uniform(ctx, 3, 2, key, TS.A_NONCE, buf.devptr())
            msg3 = error()
            rc4 = w.lib.mkhe_ct_expand_seeded(ctx, 2, key, TS.A_NONCE, h2)
            msg4 = error()
        assert rc1 != 0 and msg1.startswith("mkhe_sample_uniform: ") and "capture" in msg1 and "staged" in msg1
        assert rc2 != 0 and msg2.startswith("mkhe_ct_expand_seeded: ") and "capture" in msg2 and "staged" in msg2
        assert rc3 == 0 and rc4 == 0, (msg3, msg4)
        assert (buf.download() == SENTINEL).all() and all((c.download() == SENTINEL).all() for c in outs)     # recorded, not run
        g.launch()
        got = buf.download()
        assert (got[:2] == want).all() and (got[2] == SENTINEL).all()
        for b in range(2):
            assert (outs[b].download()[1] == want[b]).all() and (outs[b].download()[0] == SENTINEL).all(), b
        print("capture: the staged sampler and expansion were refused, the inline ones replayed")
    except MkheError as e:
        print("capture: mkhe_capture_begin refused in this process (%s): the calls inside a capture did not run" % e)
        import gc
        gc.enable()                 # (Graph.__enter__ switched the collector off before the refusal)
        assert "cannot end a multi-stream capture" in str(e)
    assert (big.download() == SENTINEL).all() and all((c.download() == SENTINEL).all() for c in outs17)
    rc, got = w.sample_uniform(2, 3)
    assert rc == 0 and (got == want).all(), error()
