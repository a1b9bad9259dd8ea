"""The device BFV batch encoder stage by stage (-m gpu): mkhe_bfv_coeffs_to_slots / slots_to_coeffs / scale_up / scale_down, the two fused
calls, the two-launch form, the Python mirror against the host encoder, and the argument validation (include/mkhe.h, csrc/bfv_kernels.h).
Every stage is integer arithmetic, so every comparison is bit for bit; the specification is restated here in Python integers."""
import ctypes as C
import types

import numpy as np
import pytest

import harness as H
import harness_bfv as HB

pytestmark = pytest.mark.gpu

T_REF, T_MID, T_BIG = 65537, 786433, 4293918721          # 2^16 + 1; 3 * 2^18 + 1; 0xFFF00001 = 1 mod 2^20 with 2 T > 2^32
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


def pset_for(name, logN):
    if name == "q14":                                    # the full 14-prime chain of BFV_PN15QP880 (primes = 1 mod 2^16)
        return dict(HB.BFV_PN15QP880, logN=logN)
    if name == "pn16":                                   # logN = 16: the primes of harness.PN16_Q / PN16_P are 1 mod 2^17
        return dict(logN=16, Q=H.PN16_Q[:2], QMul=H.PN16_Q[2:4], P=H.PN16_P[:2], T=T_MID)
    if name == "big":
        return HB.small_bfv(logN, 3, big=True)
    return HB.small_bfv(logN, int(name[1:]))


_worlds = {}


def world(name, logN, T):
    """one context per (parameter set, T) for the whole module"""
    key = (name, logN, T)
    if key not in _worlds:
        from mkhe_kklss_amd import mkbfv
        pset = pset_for(name, logN)
        params = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], T)
        Qp = 1
        for q in pset["Q"]:
            Qp *= q
        _worlds[key] = types.SimpleNamespace(params=params, pset=pset, N=1 << pset["logN"], logN=pset["logN"], T=T, Q=pset["Q"], Qp=Qp, nq=len(pset["Q"]),
                                             dev=mkbfv.DeviceEncoder(params), mkbfv=mkbfv)
    return _worlds[key]


def host_encoder(w):
    if not hasattr(w, "host"):
        w.host = w.mkbfv.Encoder(w.params)
    return w.host


def centre(r, T):
    r = np.asarray(r, dtype=np.int64)
    return np.where(r > T // 2, r - T, r)


def residues(v, T):
    return np.array([int(x) % T for x in np.asarray(v).ravel()], dtype=np.uint64).reshape(np.shape(v))


def rns(xs, Q):
    """Python integers -> uint64 [nQ][len]"""
    return np.array([[x % q for x in xs] for q in Q], dtype=np.uint64)


def direct_slots(w, m):
    """slot j = m(psi^(e_j)) mod T with e_j = 5^j, -5^(j - N/2) mod 2N: a Vandermonde sum, no transform.  m: uint64 [N] < T"""
    N, T = w.N, w.T
    psi = w.params.slot_psi()
    assert pow(psi, N, T) == T - 1                                     # a primitive 2N-th root
    e, g = [], 1
    for _ in range(N // 2):
        e.append(g)
        g = g * 5 % (2 * N)
    e += [2 * N - x for x in e]
    x = np.array([pow(psi, k, T) for k in e], dtype=np.uint64)
    acc, p, Tu = np.zeros(N, dtype=np.uint64), np.ones(N, dtype=np.uint64), np.uint64(T)
    for k in range(N):                                                 # (T < 2^32: every product fits 64 bits)
        acc = (acc + p * m[k]) % Tu
        p = p * x % Tu
    return centre(acc, T)


def sample_values(rng, count, N, T):
    v = rng.integers(I64_MIN, I64_MAX, (count, N), dtype=np.int64, endpoint=True)
    v[0, :8] = [I64_MIN, I64_MAX, -1, 0, T, -T, T + 1, -(T // 2) - 1]
    v[-1, N // 2:] = rng.integers(-T, 2 * T, N - N // 2)
    return v


# ------------------------------------------------------------------------------------------------ 1. the slot definition
@pytest.mark.parametrize("T", [T_REF, T_MID, T_BIG])
def test_slots_are_the_evaluations_at_the_odd_powers_of_psi(T):
    w = world("n1", 10, T)
    assert w.params.slot_psi() == w.mkbfv.slot_psi(T, w.N)
    from mkhe_kklss_amd._abi import lib
    assert lib().mkhe_ctx_bfv_slot_psi(w.params.ctx) == w.params.slot_psi()
    rng, N = np.random.default_rng(T % 1000), w.N
    uni = rng.integers(0, T, (3, N), dtype=np.uint64)
    special = np.zeros((4, N), dtype=np.uint64)
    special[0, 0] = 1                                                   # 1
    special[1, 1] = 1                                                   # X
    special[2, N - 1] = 1                                               # X^(N-1)
    special[3, :] = T - 1                                               # T - 1 everywhere
    for m in (uni, special[:3], special[3:]):
        got = w.dev.CoeffsToSlots(m)
        for b in range(len(m)):
            assert (got[b] == direct_slots(w, m[b])).all(), (T, b)
    assert (w.dev.CoeffsToSlots(special[0]) == 1).all()
    # slots_to_coeffs is the inverse, for any int64
    v = sample_values(rng, 3, N, T)
    c = w.dev.SlotsToCoeffs(v)
    assert c.dtype == np.uint64 and (c < T).all()
    assert (w.dev.CoeffsToSlots(c) == centre(residues(v, T), T)).all()
    assert (w.dev.SlotsToCoeffs(w.dev.CoeffsToSlots(uni)) == uni).all()


# ------------------------------------------------------------------------------------------------ 2. scale_up
SCALE_SETS = [("n1", T_REF), ("n2", T_MID), ("n3", T_BIG), ("big", T_REF), ("big", T_BIG), ("q14", T_REF), ("q14", T_BIG)]


@pytest.mark.parametrize("name,T", SCALE_SETS)
def test_scale_up_is_mkbfv_scale_up(name, T):
    w = world(name, 10, T)
    rng = np.random.default_rng(3)
    m = rng.integers(0, T, (2, w.N), dtype=np.uint64)
    m[0, :5] = [0, 1, T // 2, T // 2 + 1, T - 1]
    got = w.dev.ScaleUp(m).download()
    for b in range(2):
        assert (got[b] == w.mkbfv.ScaleUp(m[b], w.params)).all(), (name, T, b)


# ------------------------------------------------------------------------------------------------ 3. scale_down
@pytest.mark.parametrize("name,T", SCALE_SETS)
def test_scale_down_is_exact_for_every_x(name, T):
    w = world(name, 10, T)
    Q, N = w.Qp, w.N
    rng = np.random.default_rng(7)
    big = lambda: int.from_bytes(rng.bytes(8 * w.nq + 8), "little")
    xs = [0, 1, Q - 1, Q // 2, Q // 2 + 1]
    ks = [0, 1, T // 2, T - 2, T - 1] + [int(k) for k in rng.integers(0, T, 200)]
    for k in ks:                                                        # the rounding boundaries
        edge = ((2 * k + 1) * Q) // (2 * T)
        xs += [edge - 1, edge, edge + 1]
    ms = [int(v) for v in rng.integers(0, T, 150)] + [0, 1, T // 2, T // 2 + 1, T - 1]
    noisy = []
    for i, m in enumerate(ms):                                          # ScaleUp(m) + e, |e| < Q / 4T
        e = [-(Q // (4 * T)) + 1, Q // (4 * T) - 1, big() % (Q // (4 * T))][i % 3] * (-1 if i % 2 else 1)
        assert abs(e) * 4 * T < Q
        noisy.append((Q * m + T // 2) // T + e)
    n_noisy = len(xs)
    xs += noisy
    xs = [x % Q for x in xs]
    assert len(xs) <= N
    xs += [big() % Q for _ in range(2 * N - len(xs))]                   # uniform x
    want = np.array([((T * x + Q // 2) // Q) % T for x in xs], dtype=np.uint64).reshape(2, N)
    assert (want.ravel()[n_noisy:n_noisy + len(ms)] == np.array(ms, dtype=np.uint64)).all()
    pt = np.stack([rns(xs[:N], w.Q), rns(xs[N:], w.Q)])
    got = w.dev.ScaleDown(pt)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (name, T, bad[:4], [xs[b * N + i] for b, i in bad[:4]])
    # the centred form is mkbfv.ScaleDown
    assert (centre(got[0], T) == w.mkbfv.ScaleDown(pt[0], w.params)).all()


# ------------------------------------------------------------------------------------------------ 4. fused = stage pairs
def stage_pairs(w, v):
    lib_ = w.dev
    c = lib_.SlotsToCoeffs(v)
    pt = lib_.ScaleUp(c)
    back = lib_.CoeffsToSlots(lib_.ScaleDown(pt))
    return c, pt.download(), back


@pytest.mark.parametrize("name,logN,T", [("n3", 10, T_REF), ("n2", 12, T_BIG), ("big", 10, T_MID)])
@pytest.mark.parametrize("count", [1, 5])
def test_fused_calls_equal_the_stage_pairs(name, logN, T, count):
    w = world(name, logN, T)
    v = sample_values(np.random.default_rng(count), count, w.N, T)
    c, pt, back = stage_pairs(w, v)
    enc = w.dev.EncodeBatch(v)
    assert (enc.download() == pt).all()
    # a noisy plaintext, as a decryption gives it
    noise = np.random.default_rng(5).integers(-1000, 1000, (count, w.N))         # one small integer per coefficient: |e| < Q / 4T
    noisy = np.stack([[(pt[b, l].astype(object) + noise[b]) % q for l, q in enumerate(w.Q)] for b in range(count)]).astype(np.uint64)
    dec = w.dev.Decode(noisy).reshape(count, w.N)
    assert (dec == w.dev.CoeffsToSlots(w.dev.ScaleDown(noisy)).reshape(count, w.N)).all()
    assert (dec == centre(residues(v, T), T)).all() and (np.reshape(back, (count, w.N)) == dec).all()


# ------------------------------------------------------------------------------------------------ 5. the two-launch form
def set_tile(w, log_points):
    from mkhe_kklss_amd._abi import check, lib
    check(lib().mkhe_ctx_set_bfv_tile(w.params.ctx, log_points))
    return lib().mkhe_ctx_bfv_tile(w.params.ctx)


@pytest.mark.parametrize("tile", [10, 11])
def test_two_launch_form_gives_the_same_bits(tile):
    w = world("n2", 12, T_BIG)
    granted = set_tile(w, 0)
    assert granted in (14, 15) and w.logN <= granted                   # logN = 12 is on the single-workgroup form by default
    rng = np.random.default_rng(tile)
    v = sample_values(rng, 3, w.N, w.T)
    m = rng.integers(0, w.T, (3, w.N), dtype=np.uint64)
    single = (w.dev.SlotsToCoeffs(v), w.dev.CoeffsToSlots(m), w.dev.EncodeBatch(v).download())
    noisy = single[2].copy()
    noisy[:, 0, :] = (noisy[:, 0, :] + np.uint64(3)) % np.uint64(w.Q[0])
    noisy[:, 1, :] = (noisy[:, 1, :] + np.uint64(3)) % np.uint64(w.Q[1])
    single += (w.dev.Decode(noisy),)
    try:
        assert set_tile(w, tile) == tile
        multi = (w.dev.SlotsToCoeffs(v), w.dev.CoeffsToSlots(m), w.dev.EncodeBatch(v).download(), w.dev.Decode(noisy))
    finally:
        assert set_tile(w, 0) == granted
    for a, b in zip(single, multi):
        assert (a == b).all()
    assert (multi[1][0] == direct_slots(w, m[0])).all()                 # item 1 on the two-launch form
    assert (multi[3] == centre(residues(v, w.T), w.T)).all()


def against_host(w, count, seed):
    host = host_encoder(w)
    v = sample_values(np.random.default_rng(seed), count, w.N, w.T)
    pt = w.dev.EncodeBatch(v).download()
    for b in range(count):
        assert (pt[b] == host.Encode(v[b])).all()
        assert (w.dev.SlotsToCoeffs(v[b]) == host.SlotsToCoeffs(v[b])).all()
    dec = w.dev.Decode(pt).reshape(count, w.N)
    assert (dec == centre(residues(v, w.T), w.T)).all()
    assert (host.Decode(pt[0]) == dec[0]).all()


def test_logn16_takes_the_two_launch_form_naturally():
    """A BFV context exists at logN = 16 within mkhe_ctx_create_bfv's constraints: Q, QMul and P from harness.PN16_Q / PN16_P (1 mod 2^17),
    T = 786433 = 3 * 2^18 + 1.  N = 2^16 words exceed the largest tile (2^15), so this is the two-launch form without forcing."""
    w = world("pn16", 16, T_MID)
    assert set_tile(w, 0) < w.logN
    against_host(w, 2, 16)


def test_logn15_reference_modulus_against_the_host_encoder():
    """logN = 15, T = 65537, nq = 3, count = 2: the single-workgroup form where the runtime grants 128 KiB of LDS, else the two-launch one"""
    w = world("n3", 15, T_REF)
    print("bfv tile: 2^%d words" % set_tile(w, 0))
    against_host(w, 2, 15)


# ------------------------------------------------------------------------------------------------ 6. host Encoder = DeviceEncoder
@pytest.mark.parametrize("name,logN,T", [("n3", 10, T_REF), ("n2", 12, T_BIG), ("q14", 10, T_BIG), ("big", 10, T_MID)])
def test_host_encoder_equals_device_encoder(name, logN, T):
    w = world(name, logN, T)
    host = host_encoder(w)
    rng = np.random.default_rng(logN)
    v = sample_values(rng, 1, w.N, T)[0]
    m = rng.integers(0, T, w.N, dtype=np.uint64)
    assert (host.SlotsToCoeffs(v) == w.dev.SlotsToCoeffs(v)).all()
    assert (host.CoeffsToSlots(m) == w.dev.CoeffsToSlots(m)).all()
    hp, dp = host.Encode(v), w.dev.Encode(v)
    assert dp.count == 1 and dp.limbs == w.nq and (dp.download()[0] == hp).all()
    want = centre(residues(v, T), T)
    assert (w.dev.Decode(hp) == want).all()                             # host encode -> device decode
    assert (host.Decode(dp.download()[0]) == want).all()                # device encode -> host decode


# ------------------------------------------------------------------------------------------------ 7. validation
CALLS = ["mkhe_bfv_slots_to_coeffs", "mkhe_bfv_coeffs_to_slots", "mkhe_bfv_scale_up", "mkhe_bfv_scale_down", "mkhe_bfv_encode", "mkhe_bfv_decode"]


def every_call(params, count, a, b):
    """the error text of each of the six calls (every one must be refused)"""
    from mkhe_kklss_amd._abi import lib
    out = []
    for name in CALLS:
        rc = getattr(lib(), name)(params.ctx, count, a, b)
        assert rc != 0, name
        out.append(lib().mkhe_last_error().decode())
        assert out[-1].startswith(name), out[-1]
    return out


def buffers(params, nq):
    from mkhe_kklss_amd import mkrlwe
    return mkrlwe.DeviceLimbs(params, 1, nq), mkrlwe.DeviceLimbs(params, 1, nq)


@pytest.mark.parametrize("logN,T,text", [(16, T_REF, "1 mod 2N"), (10, 257, "1 mod 2N"), (10, 4294967311, "below 2^32"), (10, 2049, "prime")])
def test_unsupported_plaintext_moduli_are_refused(logN, T, text):
    """65537 is not 1 mod 2^17; 257 is not 1 mod 2^11; 4294967311 >= 2^32; 2049 = 3 * 683 = 1 mod 2^11.  mkhe_ctx_create_bfv accepts them all."""
    from mkhe_kklss_amd import mkbfv, mkrlwe
    from mkhe_kklss_amd._abi import lib
    pset = pset_for("pn16", 16) if logN == 16 else HB.small_bfv(logN, 2)
    params = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], T)
    a, b = buffers(params, len(pset["Q"]))
    assert all(text in m for m in every_call(params, 1, a.devptr(), b.devptr()))
    assert lib().mkhe_ctx_bfv_tile(params.ctx) == -1 and lib().mkhe_ctx_bfv_slot_psi(params.ctx) == 0
    # the context still works
    N = 1 << logN
    assert (mkrlwe.DeviceLimbs(params, 1, 1).upload(np.ones((1, 1, N), dtype=np.uint64)).download() == 1).all()
    del a, b
    params.close()


def test_argument_validation():
    from mkhe_kklss_amd import mkckks, mkrlwe
    from mkhe_kklss_amd._abi import MkheError, lib
    w = world("n2", 10, T_MID)
    params = w.params
    a, b = buffers(params, w.nq)
    v = sample_values(np.random.default_rng(0), 1, w.N, w.T)[0]
    want = centre(residues(v, w.T), w.T)
    works = lambda: (w.dev.Decode(w.dev.Encode(v)) == want).all()
    assert works()
    for count in (0, 65536, -1):
        assert all("count" in m for m in every_call(params, count, a.devptr(), b.devptr()))
    assert works()
    assert all("null" in m for m in every_call(params, 1, None, b.devptr()))
    assert all("null" in m for m in every_call(params, 1, a.devptr(), None))
    assert all("aligned" in m for m in every_call(params, 1, C.c_void_p(a.devptr().value + 8), b.devptr()))
    assert works()
    assert lib().mkhe_ctx_set_bfv_tile(params.ctx, 9) != 0 and lib().mkhe_ctx_set_bfv_tile(params.ctx, 16) != 0
    assert works()
    # a non-BFV context
    ck = H.small_ckks(10, 2)
    cparams = mkckks.Parameters(ck["logN"], ck["Q"], ck["P"], ck["scale"])
    ca, cb = buffers(cparams, 2)
    assert all("BFV context" in m for m in every_call(cparams, 1, ca.devptr(), cb.devptr()))
    assert lib().mkhe_ctx_bfv_tile(cparams.ctx) == -1
    assert (mkrlwe.DeviceLimbs(cparams, 1, 1).upload(np.ones((1, 1, w.N), dtype=np.uint64)).download() == 1).all()
    del ca, cb
    cparams.close()
    # a context that owns a subset of the moduli: mkhe_ctx_set_owned does not make one of a BFV context, so the refusal of the encoder calls
    # on such a context (capi.hip, bfv_encode.hip) cannot be reached today; what can be checked is that the attempt leaves the encoder working
    own = (C.c_int * 2)(0, w.nq)
    assert lib().mkhe_ctx_set_owned(params.ctx, own, 2) != 0 and "mkckks path" in lib().mkhe_last_error().decode()
    assert works()
    # inside a capture (where the runtime of this process can capture at all: tests/test_gpu_cnn.py)
    try:
        with params.Capture():
            msgs = every_call(params, 1, a.devptr(), b.devptr())
        assert all("capture" in m for m in msgs)
        print("capture: the six calls were refused inside a capture")
    except MkheError as e:
        print("capture: mkhe_capture_begin refused in this process (%s): the refusals inside a capture did not run" % e)
        import gc
        gc.enable()                 # (Graph.__enter__ switched the collector off before the refusal)
        assert "cannot end a multi-stream capture" in str(e)
    assert works()
