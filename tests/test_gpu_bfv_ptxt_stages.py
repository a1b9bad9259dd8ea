"""The BFV plaintext operands on the device stage by stage (-m gpu): mkhe_bfv_lift, mkhe_bfv_encode_mul (single- and two-launch form),
mkhe_bfv_ct_mul_ptxt, mkhe_bfv_ct_add_ptxt and their argument validation (include/mkhe.h, "BFV plaintext operands").  Everything is integer
arithmetic, so every comparison is bit for bit.  Wherever an existing entry point computes the same value (mkhe_ntt, mkhe_ct_mul_ptxt,
mkhe_ct_add / mkhe_ct_sub) the new one is pinned to it; the definitions are restated in Python integers besides.

Encoder.EncodeMul (the host mirror) takes its forward NTT from the engine, so its check against a direct evaluation of the definition lives here
(test_encode_mul_is_the_ntt_of_the_lift), not in tests/test_bfv_ptxt_host.py."""
import ctypes as C

import numpy as np
import pytest

import harness as H
import test_gpu_bfv_encoder_stages as ES
from test_gpu_bfv_encoder_stages import T_BIG, T_MID, T_REF, sample_values, set_tile, world

pytestmark = pytest.mark.gpu


def centred(m, T):
    """Python integers: the centred representative of m mod T"""
    m = int(m) % T
    return m - T if m > T // 2 else m


def lift_ref(m, Q, T, mform=True):
    """uint64 [nQ][len(m)]: (c mod q_l), times 2^64 mod q_l with mform"""
    c = [centred(x, T) for x in m]
    return np.array([[((v % q) << 64) % q if mform else v % q for v in c] for q in Q], dtype=np.uint64)


def bitrev(x, bits):
    r = 0
    for _ in range(bits):
        r, x = (r << 1) | (x & 1), x >> 1
    return r


# ------------------------------------------------------------------------------------------------ 1. the lift
@pytest.mark.parametrize("name,T", [("n1", T_REF), ("n3", T_BIG), ("big", T_MID)])
def test_lift_is_the_centred_representative_in_montgomery_form(name, T):
    w = world(name, 10, T)
    rng = np.random.default_rng(T % 977)
    m = rng.integers(0, 2 ** 64, (2, w.N), dtype=np.uint64)
    m[0, :5] = [0, 1, T // 2, T // 2 + 1, T - 1]
    m[0, 5:11] = np.array([T, T + 1, 3 * T + T // 2, 3 * T + T // 2 + 1, 2 ** 63, 2 ** 64 - 1], dtype=np.uint64)         # the input is taken mod T
    m[1, :3] = np.array([2 ** 63 + T // 2, 2 ** 63 + 12345, (2 ** 64 - 1) // T * T], dtype=np.uint64)
    m[1, w.N // 2:] = rng.integers(0, T, w.N - w.N // 2)
    got = w.dev.Lift(m)
    assert got.count == 2 and got.limbs == w.nq
    got = got.download()
    for b in range(2):
        assert (got[b] == lift_ref(m[b], w.Q, T)).all(), (name, T, b)
        assert (got[b] == w.mkbfv.Lift(m[b], w.params)).all()
    # the planted values, spelt out for limb 0: 0, 1, floor(T/2) stay, floor(T/2) + 1 and T - 1 are negative
    q = w.Q[0]
    assert [int(x) for x in got[0, 0, :5]] == [0, (1 << 64) % q, ((T // 2) << 64) % q, ((q - T // 2) << 64) % q, ((q - 1) << 64) % q]


# ------------------------------------------------------------------------------------------------ 2. encode_mul = ntt(lift(slots_to_coeffs))
def staged(w, v):
    """the existing entry point mkhe_ntt applied to mkhe_bfv_lift(mkhe_bfv_slots_to_coeffs(v)) -> uint64 [count][nQ][N]"""
    from mkhe_kklss_amd import mkrlwe
    lift = w.dev.Lift(w.dev.SlotsToCoeffs(v).reshape(-1, w.N))
    out = mkrlwe.DeviceLimbs(w.params, lift.count, w.nq)
    mkrlwe.ntt(w.params, lift, out)
    return out.download()


@pytest.mark.parametrize("name,logN,T", [("n3", 10, T_REF), ("n2", 12, T_BIG)])
@pytest.mark.parametrize("count", [1, 5])
def test_encode_mul_equals_the_stages_and_the_host_encoder(name, logN, T, count):
    w = world(name, logN, T)
    v = sample_values(np.random.default_rng(100 + count), count, w.N, T)
    pm = w.dev.EncodeMulBatch(v)
    assert isinstance(pm, w.mkbfv.PlaintextMul) and pm.count == count and pm.Value.limbs == w.nq
    got = pm.download()
    assert (got == staged(w, v)).all()
    host = ES.host_encoder(w)
    for b in {0, count - 1}:
        assert (host.EncodeMul(v[b]) == got[b]).all(), b
    if count == 1:
        assert (w.dev.EncodeMul(v[0]).download() == got).all()


def test_encode_mul_is_the_ntt_of_the_lift():
    """position j of limb l is MForm(p(psi_l^(2 bitrev(j) + 1))) for p the centred lift of the coefficients: Horner in Python integers at a few j"""
    w = world("n3", 10, T_REF)
    v = sample_values(np.random.default_rng(9), 1, w.N, w.T)[0]
    got = w.dev.EncodeMul(v).download()[0]
    host = ES.host_encoder(w).EncodeMul(v)
    p = [centred(x, w.T) for x in w.dev.SlotsToCoeffs(v)]
    for l, q in enumerate(w.Q):
        psi = w.params.Psi(l)
        assert pow(psi, w.N, q) == q - 1
        for j in (0, 1, 2, w.N // 2 - 1, w.N // 2, w.N - 1):
            x, acc = pow(psi, 2 * bitrev(j, w.logN) + 1, q), 0
            for c in reversed(p):
                acc = (acc * x + c) % q
            assert int(got[l, j]) == (acc << 64) % q == int(host[l, j]), (l, j)


# ------------------------------------------------------------------------------------------------ 3. the two-launch form
@pytest.mark.parametrize("tile", [10, 11])
def test_two_launch_form_gives_the_same_bits(tile):
    w = world("n2", 12, T_BIG)
    granted = set_tile(w, 0)
    assert granted in (14, 15) and w.logN <= granted
    v = sample_values(np.random.default_rng(tile), 3, w.N, w.T)
    single = w.dev.EncodeMulBatch(v).download()
    try:
        assert set_tile(w, tile) == tile
        multi = w.dev.EncodeMulBatch(v).download()
    finally:
        assert set_tile(w, 0) == granted
    assert (single == multi).all()
    assert (multi == staged(w, v)).all()


def test_logn16_takes_the_two_launch_form_naturally():
    w = world("pn16", 16, T_MID)
    assert set_tile(w, 0) < w.logN
    v = sample_values(np.random.default_rng(16), 1, w.N, w.T)
    got = w.dev.EncodeMulBatch(v).download()
    assert (got == staged(w, v)).all()
    # the lift under it, at a few coefficients, in Python integers
    c = w.dev.SlotsToCoeffs(v[0])
    idx = [0, 1, w.N // 2, w.N - 1]
    assert (w.dev.Lift(c).download()[0][:, idx] == lift_ref(c[idx], w.Q, w.T)).all()


# ------------------------------------------------------------------------------------------------ 4. / 5. ciphertext operations
NAMES = ["user0", "user1", "user2"]


def uniform_cts(w, rng, k, B):
    """B ciphertexts over the first k parties with uniform residues -> (handles, host arrays)"""
    ids = NAMES[:k]
    host = [np.stack([H.uniform_poly(rng, w.Q, w.N) for _ in range(1 + k)]) for _ in range(B)]
    return [w.mkbfv.NewCiphertext(w.params, ids).upload(h) for h in host], host


def evaluator(w):
    if not hasattr(w, "ev"):
        w.ev = w.mkbfv.NewEvaluator(w.params)
    return w.ev


def negacyclic(a, b, q):
    """schoolbook (a * b mod X^N + 1) mod q in Python integers"""
    N = len(a)
    b = np.array([int(x) for x in b], dtype=object)
    acc = np.zeros(2 * N, dtype=object)
    for i, x in enumerate(a):
        acc[i:i + N] += int(x) * b
    return np.array([int(v) % q for v in acc[:N] - acc[N:]], dtype=np.uint64)


# (B = 65: the list transforms on both sides of the product take 64 ciphertexts per launch)
@pytest.mark.parametrize("B,k", [(1, 0), (3, 0), (1, 1), (3, 1), (1, 3), (3, 3), (65, 0)])
def test_ct_mul_ptxt(k, B):
    from mkhe_kklss_amd import mkrlwe
    from mkhe_kklss_amd._abi import check, lib
    w = world("n3", 10, T_REF)
    ev = evaluator(w)
    rng = np.random.default_rng(10 * k + B)
    cts, host = uniform_cts(w, rng, k, B)
    v = sample_values(rng, B, w.N, w.T)
    coeffs = w.dev.SlotsToCoeffs(v).reshape(B, w.N)
    per_item, shared = w.dev.EncodeMulBatch(v), w.dev.EncodeMul(v[0])
    # the reference: the existing mkhe_ct_mul_ptxt fed the host-computed lift as canonical residues, coefficient domain, no Montgomery form
    ref = []
    for b in range(B):
        row = []
        for pb in (b, 0):
            pt = mkrlwe.DeviceLimbs(w.params, 1, w.nq).upload(lift_ref(coeffs[pb], w.Q, w.T, mform=False)[None])
            out = w.mkbfv.NewCiphertext(w.params, NAMES[:k])
            check(lib().mkhe_ct_mul_ptxt(w.params.ctx, cts[b].h, pt.devptr(), out.h))
            row.append(out.download())
        ref.append(row)
    got = ev.MulPtxtBatch(cts, per_item)
    assert len(got) == B and all(g.ids == NAMES[:k] and g.Level() == w.params.MaxLevel() for g in got)
    for b in range(B):
        assert (got[b].download() == ref[b][0]).all(), ("per item", b)
    got = ev.MulPtxtBatch(cts, shared)
    for b in range(B):
        assert (got[b].download() == ref[b][1]).all(), ("shared", b)
    assert (ev.MulPtxtNew(cts[B - 1], shared).download() == ref[B - 1][1]).all()
    # one component, one limb: the schoolbook negacyclic product
    comp, l = k, w.nq - 1
    q = w.Q[l]
    assert (ref[0][0][comp, l] == negacyclic(host[0][comp, l], [centred(x, w.T) for x in coeffs[0]], q)).all()
    # in place
    hs = (C.c_void_p * B)(*[c.h for c in cts])
    check(lib().mkhe_bfv_ct_mul_ptxt(w.params.ctx, B, hs, per_item.Value.devptr(), w.nq * w.N if B > 1 else 0, hs))
    for b in range(B):
        assert (cts[b].download() == ref[b][0]).all(), ("in place", b)


@pytest.mark.parametrize("k", [0, 1, 3])
@pytest.mark.parametrize("B", [1, 3])
def test_ct_add_ptxt(k, B):
    """the reference is mkhe_ct_add / mkhe_ct_sub with a zero-party ciphertext that holds the plaintext (mkhe_ct_create accepts n = 0), and
    CRed(c_0 +- pt) in Python integers besides"""
    from mkhe_kklss_amd._abi import check, lib
    w = world("n3", 10, T_REF)
    ev = evaluator(w)
    rng = np.random.default_rng(50 + 10 * k + B)
    cts, host = uniform_cts(w, rng, k, B)
    pts = w.dev.EncodeBatch(sample_values(rng, B, w.N, w.T))
    pth = pts.download()
    for sub, fn in ((False, lib().mkhe_ct_add), (True, lib().mkhe_ct_sub)):
        ref = []
        for b in range(B):
            row = []
            for pb in (b, 0):
                pc = w.mkbfv.NewCiphertext(w.params, []).upload(pth[pb][None])
                out = w.mkbfv.NewCiphertext(w.params, NAMES[:k])
                check(fn(w.params.ctx, cts[b].h, pc.h, out.h))
                row.append(out.download())
                assert (row[-1][1:] == host[b][1:]).all()                     # components 1 .. k are unchanged
                for l, q in enumerate(w.Q):
                    x, y = host[b][0, l].astype(object), pth[pb][l].astype(object)
                    assert (row[-1][0, l].astype(object) == ((x - y) % q if sub else (x + y) % q)).all()
            ref.append(row)
        got = ev.AddPtxtBatch(cts, pts, sub=sub)
        assert all(g.ids == NAMES[:k] for g in got)
        for b in range(B):
            assert (got[b].download() == ref[b][0]).all(), (sub, "per item", b)
        got = ev.AddPtxtBatch(cts, pth[0], sub=sub)                           # a host plaintext, shared
        for b in range(B):
            assert (got[b].download() == ref[b][1]).all(), (sub, "shared", b)
        one = (ev.SubPtxtNew if sub else ev.AddPtxtNew)(cts[B - 1], pth[0])
        assert (one.download() == ref[B - 1][1]).all()
    # in place (sub): the other components are left alone
    hs = (C.c_void_p * B)(*[c.h for c in cts])
    check(lib().mkhe_bfv_ct_add_ptxt(w.params.ctx, 1, B, hs, pts.devptr(), w.nq * w.N if B > 1 else 0, hs))
    for b in range(B):
        assert (cts[b].download() == ref[b][0]).all(), ("in place", b)


# ------------------------------------------------------------------------------------------------ 6. validation
STAGE_CALLS = ["mkhe_bfv_lift", "mkhe_bfv_encode_mul"]


def stage_calls(params, count, a, b):
    from mkhe_kklss_amd._abi import lib
    out = []
    for name in STAGE_CALLS:
        assert getattr(lib(), name)(params.ctx, count, a, b) != 0, name
        out.append(lib().mkhe_last_error().decode())
        assert out[-1].startswith(name), out[-1]
    return out


def ct_calls(params, nbatch, ins, pt, stride, outs, op=0):
    """the error texts of mkhe_bfv_ct_mul_ptxt and mkhe_bfv_ct_add_ptxt (both must refuse)"""
    from mkhe_kklss_amd._abi import lib
    arr = lambda v: None if v is None else (C.c_void_p * max(len(v), 1))(*[getattr(c, "h", c) for c in v])
    out = []
    for name in ("mkhe_bfv_ct_mul_ptxt", "mkhe_bfv_ct_add_ptxt"):
        args = (params.ctx, nbatch, arr(ins), pt, stride, arr(outs))
        rc = lib().mkhe_bfv_ct_mul_ptxt(*args) if name.endswith("mul_ptxt") else lib().mkhe_bfv_ct_add_ptxt(args[0], op, *args[1:])
        assert rc != 0, name
        out.append(lib().mkhe_last_error().decode())
        assert out[-1].startswith(name), out[-1]
    return out


@pytest.mark.parametrize("logN,T,text", [(16, T_REF, "1 mod 2N"), (10, 257, "1 mod 2N"), (10, 4294967311, "below 2^32"), (10, 2049, "prime")])
def test_unsupported_plaintext_moduli_are_refused(logN, T, text):
    import harness_bfv as HB
    from mkhe_kklss_amd import mkbfv
    pset = ES.pset_for("pn16", 16) if logN == 16 else HB.small_bfv(logN, 2)
    params = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], T)
    nq = len(pset["Q"])
    a, b = ES.buffers(params, nq)
    assert all(text in m for m in stage_calls(params, 1, a.devptr(), b.devptr()))
    ct = mkbfv.NewCiphertext(params, ["user0"])
    assert all(text in m for m in ct_calls(params, 1, [ct], a.devptr(), 0, [ct]))
    host = np.ones(ct.shape(), dtype=np.uint64)
    assert (ct.upload(host).download() == host).all()                       # the context still works
    del a, b, ct
    params.close()


def test_argument_validation():
    from mkhe_kklss_amd import mkckks, mkrlwe
    from mkhe_kklss_amd._abi import MkheError, lib
    w = world("n2", 10, T_MID)
    params, ev = w.params, evaluator(w)
    a, b = ES.buffers(params, w.nq)
    rng = np.random.default_rng(0)
    v = sample_values(rng, 1, w.N, w.T)[0]
    cts, _ = uniform_cts(w, rng, 2, 3)
    other_ids = w.mkbfv.NewCiphertext(params, NAMES[1:3])
    low = mkrlwe.Ciphertext(params, NAMES[:2], params.MaxLevel() - 1)
    outs = [w.mkbfv.NewCiphertext(params, NAMES[:2]) for _ in range(3)]
    pm, pt = w.dev.EncodeMulBatch(np.stack([v] * 3)), w.dev.EncodeBatch(np.stack([v] * 3))
    want = [c.download() for c in ev.MulPtxtBatch(cts, pm)]

    def works():
        got = ev.MulPtxtBatch(cts, w.dev.EncodeMul(v))
        same = all((g.download() == x).all() for g, x in zip(got, want))
        back = ev.SubPtxtNew(ev.AddPtxtNew(cts[0], pt.download()[0]), pt.download()[0])
        return same and (back.download() == cts[0].download()).all()

    assert works()
    stride, P = w.nq * w.N, pm.Value.devptr()
    for count in (0, 65536, -1):
        assert all("count" in m for m in stage_calls(params, count, a.devptr(), b.devptr()))
        assert all("count" in m for m in ct_calls(params, count, cts, P, stride, outs))
    assert all("null" in m for m in stage_calls(params, 1, None, b.devptr()))
    assert all("null" in m for m in stage_calls(params, 1, a.devptr(), None))
    assert all("aligned" in m for m in stage_calls(params, 1, C.c_void_p(a.devptr().value + 8), b.devptr()))
    assert all("aligned" in m for m in stage_calls(params, 1, a.devptr(), C.c_void_p(b.devptr().value + 8)))
    assert works()
    assert all("null" in m for m in ct_calls(params, 3, cts, None, stride, outs))
    assert all("null" in m for m in ct_calls(params, 3, None, P, stride, outs))
    assert all("null" in m for m in ct_calls(params, 3, cts, P, stride, None))
    assert all("null" in m for m in ct_calls(params, 3, cts[:2] + [None], P, stride, outs))
    assert all("aligned" in m for m in ct_calls(params, 3, cts, C.c_void_p(P.value + 8), stride, outs))
    assert works()
    for bad in (1, w.N, stride - 1, 2 * stride, -stride):
        assert all("pt_stride_words" in m for m in ct_calls(params, 3, cts, P, bad, outs))
    assert all("share their ids" in m for m in ct_calls(params, 3, cts[:2] + [other_ids], P, stride, outs))
    assert all("ids of the inputs" in m for m in ct_calls(params, 3, cts, P, stride, outs[:2] + [other_ids]))
    assert all("maximum level" in m for m in ct_calls(params, 3, cts[:2] + [low], P, stride, outs))
    assert all("maximum level" in m for m in ct_calls(params, 3, cts, P, stride, outs[:2] + [low]))
    assert all("another item" in m for m in ct_calls(params, 3, cts, P, stride, [cts[1], outs[1], outs[2]]))
    assert all("distinct" in m for m in ct_calls(params, 3, cts, P, stride, [outs[0], outs[0], outs[2]]))
    rc = lib().mkhe_bfv_ct_add_ptxt(params.ctx, 2, 1, (C.c_void_p * 1)(cts[0].h), pt.devptr(), 0, (C.c_void_p * 1)(outs[0].h))
    assert rc != 0 and lib().mkhe_last_error().decode().startswith("mkhe_bfv_ct_add_ptxt: op")
    assert works()
    # the Python mirror refuses what it cannot pass on
    with pytest.raises(MkheError):
        ev.MulPtxtBatch(cts, w.dev.EncodeMulBatch(np.stack([v] * 2)))
    with pytest.raises(MkheError):
        ev.MulPtxtNew(cts[0], pt)
    # a non-BFV context
    ck = H.small_ckks(10, 2)
    cparams = mkckks.Parameters(ck["logN"], ck["Q"], ck["P"], ck["scale"])
    ca, cb = ES.buffers(cparams, 2)
    cct = mkrlwe.Ciphertext(cparams, ["user0"], 1)
    assert all("BFV context" in m for m in stage_calls(cparams, 1, ca.devptr(), cb.devptr()))
    assert all("BFV context" in m for m in ct_calls(cparams, 1, [cct], ca.devptr(), 0, [cct]))
    assert (mkrlwe.DeviceLimbs(cparams, 1, 1).upload(np.ones((1, 1, w.N), dtype=np.uint64)).download() == 1).all()
    del ca, cb, cct
    cparams.close()
    # a context that owns a subset of the moduli cannot be made of a BFV context today (tests/test_gpu_bfv_encoder_stages.py): the attempt
    # leaves the new calls working
    own = (C.c_int * 2)(0, w.nq)
    assert lib().mkhe_ctx_set_owned(params.ctx, own, 2) != 0
    assert works()
    # inside a capture (where the runtime of this process can capture at all)
    try:
        with params.Capture():
            msgs = stage_calls(params, 1, a.devptr(), b.devptr()) + ct_calls(params, 3, cts, P, stride, outs)
        assert all("capture" in m for m in msgs)
        print("capture: the four calls were refused inside a capture")
    except MkheError as e:
        print("capture: mkhe_capture_begin refused in this process (%s): the refusals inside a capture did not run" % e)
        import gc
        gc.enable()                 # (Graph.__enter__ switched the collector off before the refusal)
        assert "cannot end a multi-stream capture" in str(e)
    assert works()
