"""Sparse CKKS packing on the host (no GPU): the numpy Encoder with 2^logSlots slots against the definition -- a sparse message is the
full-packing embedding of the tiled slots, exactly zero off the grid of stride N / 2n, and its projection reads the grid only, which is the
mean over the replicas of the full projection --, the slot count in the linear-transform plan, the range check of Parameters, and the
refusals of the sparse entry points that need no context."""
import ctypes as C

import numpy as np
import pytest

import harness as H

LOGN = 10
N = 1 << LOGN
LOG_SLOTS = [0, 1, 3, 4, 8, 9]


class StubParams:
    """the accessors the host encoder reads (a real Parameters object opens a device context)"""

    def __init__(self, logN, Q, logSlots=None):
        self.logN, self.Q, self.logSlots = logN, list(Q), logN - 1 if logSlots is None else logSlots

    def N(self): return 1 << self.logN
    def LogN(self): return self.logN
    def LogSlots(self): return self.logSlots


Q2 = H.PN15QP880["Q"][:2]


def encoders(logSlots):
    from mkhe_kklss_amd import mkckks
    p = StubParams(LOGN, Q2)
    return mkckks.Encoder(p, logSlots=logSlots), mkckks.Encoder(p)


def slots(rng, n):
    return rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)


@pytest.mark.parametrize("logSlots", LOG_SLOTS)
def test_embed_is_the_full_embedding_of_the_tiled_slots_and_zero_off_the_grid(logSlots):
    sparse, full = encoders(logSlots)
    n, g = 1 << logSlots, N >> (logSlots + 1)
    assert sparse.n == n
    z = slots(np.random.default_rng(logSlots), n)
    m, ref = sparse.Embed(z), full.Embed(np.tile(z, N // (2 * n)))
    off = np.ones(N, dtype=bool)
    off[::g] = False
    assert m.shape == (N,) and (m[off] == 0.0).all() and not np.signbit(m[off]).any()
    err = np.abs(m[::g] - ref[::g]).max()
    print("logSlots %d: |sparse - full(tile)| on the grid %.3g, bound %.3g; full off the grid %.3g" % (logSlots, err, 2.0 ** -45 * np.abs(z).max(),
                                                                                                     np.abs(ref[off]).max(initial=0.0)))
    assert err <= 2.0 ** -45 * np.abs(z).max()
    if logSlots == 0:
        assert (m[[0, N // 2]] == [z[0].real, z[0].imag]).all()              # m' = Re z + Y Im z


@pytest.mark.parametrize("logSlots", LOG_SLOTS)
def test_project_is_the_replica_mean_and_reads_the_grid_only(logSlots):
    sparse, full = encoders(logSlots)
    n, g = 1 << logSlots, N >> (logSlots + 1)
    m = np.random.default_rng(50 + logSlots).uniform(-1, 1, N)
    z = sparse.Project(m)
    mean = full.Project(m).reshape(N // (2 * n), n).mean(axis=0)
    err = np.abs(z - mean).max()
    print("logSlots %d: |project - replica mean| %.3g, bound %.3g" % (logSlots, err, 2.0 ** -40 * np.abs(m).max()))
    assert z.shape == (n,) and err <= 2.0 ** -40 * np.abs(m).max()
    poisoned = np.full(N, np.nan)
    poisoned[::g] = m[::g]
    zp = sparse.Project(poisoned)
    assert np.isfinite(zp).all() and (zp.view(np.float64) == z.view(np.float64)).all()


@pytest.mark.parametrize("logSlots", LOG_SLOTS)
def test_decode_inverts_encode(logSlots):
    sparse, _ = encoders(logSlots)
    n, g, scale = 1 << logSlots, N >> (logSlots + 1), 2.0 ** 40
    z = slots(np.random.default_rng(70 + logSlots), n)
    pt = sparse.Encode(z, 1, scale)
    off = np.ones(N, dtype=bool)
    off[::g] = False
    assert pt.shape == (2, N) and pt.dtype == np.uint64 and not pt[:, off].any()
    err = np.abs(sparse.Decode(pt, scale) - z).max()
    print("logSlots %d: |decode(encode(z)) - z| %.3g, bound %.3g" % (logSlots, err, N / scale))
    assert err <= N / scale
    # a noisy polynomial: only the grid is read
    rng = np.random.default_rng(90 + logSlots)
    noisy = np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in Q2])
    other = noisy.copy()
    other[:, off] = 1
    a, b = sparse.Decode(noisy, scale), sparse.Decode(other, scale)
    assert (a.view(np.float64) == b.view(np.float64)).all()
    with pytest.raises(Exception, match="slots"):
        sparse.Encode(np.zeros(n + 1), 1, scale)


def test_full_packing_keeps_its_bits():
    """logSlots = logN - 1, given or defaulted, computes what the encoder computed before sparse packing: one FFT of length 2N over all of N"""
    from mkhe_kklss_amd import mkckks
    sparse, full = encoders(LOGN - 1)
    rng = np.random.default_rng(4)
    z, m, scale = slots(rng, N // 2), rng.uniform(-1, 1, N), 2.0 ** 40
    rot, r = np.empty(N // 2, dtype=np.int64), 1
    for j in range(N // 2):
        rot[j], r = r, r * 5 % (2 * N)
    a = np.zeros(2 * N, dtype=np.complex128)
    a[rot] = z
    want_m = (2.0 / N) * np.real(np.fft.fft(a)[:N])
    a = np.zeros(2 * N, dtype=np.complex128)
    a[:N] = m
    want_z = (2 * N) * np.fft.ifft(a)[rot]
    for enc in (sparse, full):
        assert (enc.rot == rot).all()
        assert (enc.Embed(z) == want_m).all()
        assert (enc.Project(m).view(np.float64) == want_z.view(np.float64)).all()
    pt = full.Encode(z, 1, scale)
    assert (sparse.Encode(z, 1, scale) == pt).all()
    assert (sparse.Decode(pt, scale).view(np.float64) == full.Decode(pt, scale).view(np.float64)).all()
    for bad in (-1, LOGN, 2.5):
        with pytest.raises(mkckks.MkheError, match="logSlots"):
            mkckks.Encoder(StubParams(LOGN, Q2), logSlots=bad)
    assert mkckks.Encoder(StubParams(LOGN, Q2, logSlots=4)).n == 16          # the default is params.LogSlots()


def test_linear_transform_plan_and_diagonals_over_16_slots():
    from mkhe_kklss_amd import mkckks
    plan = mkckks.linear_transform_plan(range(16), 16)
    ks = sorted(b + g for g in plan.giants for b in plan.babies)
    assert ks == list(range(16)) and all(0 <= r < 16 for r in plan.babies + plan.giants)
    assert plan.n1 in (1, 2, 4, 8, 16) and set(plan.babies) == {k % plan.n1 for k in range(16)}
    assert mkckks.linear_transform_plan([17, -1, 16], 16).babies == mkckks.linear_transform_plan([1, 15, 0], 16).babies      # indices mod n
    rng = np.random.default_rng(6)
    M = rng.uniform(-1, 1, (16, 16)) + 1j * rng.uniform(-1, 1, (16, 16))
    d = mkckks.matrix_diagonals(M, 16)
    assert sorted(d) == list(range(16)) and all(v.shape == (16,) for v in d.values())
    z = slots(rng, 16)
    assert np.abs(sum(d[k] * np.roll(z, -k) for k in d) - M @ z).max() < 1e-12           # no replication at d = n


def test_parameters_refuse_a_slot_count_out_of_range_before_a_context_is_opened():
    from mkhe_kklss_amd import mkckks
    pset = H.small_ckks(10, 4)
    for bad in (-1, 10, 11):
        with pytest.raises(mkckks.MkheError, match="logSlots must lie between 0 and logN - 1 = 9"):
            mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], pset["scale"], logSlots=bad)


ANON = "mkhe: null context"
ROWS = [
    ("mkhe_ckks_encode_sparse", (0, 4, 1, None, 0.0, None), "mkhe_ckks_encode_sparse: scale must be finite and positive"),
    ("mkhe_ckks_encode_sparse", (0, 4, 1, None, 1.0, None), ANON),
    ("mkhe_ckks_decode_sparse", (1, 4, 1, None, float("nan"), None), "mkhe_ckks_decode_sparse: scale must be finite and positive"),
    ("mkhe_ckks_decode_sparse", (1, 4, 1, None, 1.0, None), ANON),
    ("mkhe_ckks_embed_sparse", (4, 1, None, None), ANON),
    ("mkhe_ckks_project_sparse", (4, 1, None, None), ANON),
]


@pytest.mark.parametrize("entry,args,message", ROWS, ids=["%s-%d" % (r[0], i) for i, r in enumerate(ROWS)])
def test_a_sparse_call_without_a_context_is_refused_with_exactly_this_message(entry, args, message):
    from mkhe_kklss_amd._abi import lib
    assert lib().mkhe_swk_fold(None, None, 0, 0) == 1 and lib().mkhe_last_error().decode() == "mkhe_swk_fold: null argument"
    assert getattr(lib(), entry)(None, *args) == 1
    assert lib().mkhe_last_error().decode() == message
