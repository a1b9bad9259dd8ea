"""Host-side parts of encryption / decryption (no GPU): the numpy CKKS encoder of the package against the matrix encoder of the
harness, the BFV scaling helpers against harness_bfv, the key sets, and the three new C-ABI symbols in the binding."""
import types

import numpy as np
import pytest

import harness as H
import harness_bfv as HB


class StubParams:
    """the accessors the host helpers read (a real Parameters object opens a device context)"""

    def __init__(self, logN, Q, T=None):
        self.logN, self.Q, self._T = logN, list(Q), T

    def N(self): return 1 << self.logN
    def LogN(self): return self.logN
    def LogSlots(self): return self.logN - 1
    def T(self): return self._T


def test_encoder_matches_matrix_encoder():
    from mkhe_kklss_amd import mkckks
    logN, Q = 8, H.PN15QP880["Q"][:2]
    rng = np.random.default_rng(0)
    z = rng.normal(size=1 << (logN - 1)) + 1j * rng.normal(size=1 << (logN - 1))
    slow, enc = H.CKKSEncoder(logN), mkckks.Encoder(StubParams(logN, Q))
    scale = float(1 << 40)
    p0, p1 = slow.encode(z, scale, Q), enc.Encode(z, 1, scale)
    assert p1.shape == p0.shape and p1.dtype == np.uint64
    for l, q in enumerate(Q):                            # coefficients agree to one unit: the rounding of a half may differ
        d = (p0[l].astype(object) - p1[l].astype(object)) % q
        assert all(min(int(v), q - int(v)) <= 1 for v in d)
    assert np.abs(enc.Decode(p1, scale) - z).max() < 1e-9
    assert np.abs(enc.Decode(p0, scale) - z).max() < 1e-9
    assert np.abs(slow.decode(p1, scale, Q) - z).max() < 1e-9
    assert enc.Encode(z, 0, scale).shape == (1, 1 << logN)


def test_encoder_is_exact_for_large_coefficients():
    """coefficients beyond 64 bits are reduced exactly (Python integers), and Decode inverts Encode at the precision of float64"""
    from mkhe_kklss_amd import mkckks
    logN, Q = 8, H.PN15QP880["Q"][:3]
    enc = mkckks.Encoder(StubParams(logN, Q))
    rng = np.random.default_rng(1)
    z = rng.normal(size=1 << (logN - 1)) + 1j * rng.normal(size=1 << (logN - 1))
    scale = 2.0 ** 100
    p = enc.Encode(z, 2, scale)
    x = enc.Embed(z) * scale
    for l, q in enumerate(Q):
        assert [int(v) for v in p[l]] == [int(round(float(v))) % q for v in x]
    assert np.abs(enc.Decode(p, scale) - z).max() < 1e-9
    with pytest.raises(Exception, match="slots"):
        enc.Encode(z[:5], 2, scale)


@pytest.mark.parametrize("name", ["N10_q3", "N12_q4big"])
def test_bfv_scale_up_down(name):
    from mkhe_kklss_amd import mkbfv
    pset = {"N10_q3": HB.small_bfv(10, 3), "N12_q4big": HB.small_bfv(12, 4, big=True)}[name]
    kg = HB.BFVKeyGen(HB.make_bfv(pset), 1)
    params = StubParams(pset["logN"], pset["Q"], pset["T"])
    rng = np.random.default_rng(2)
    T, N = pset["T"], 1 << pset["logN"]
    m = rng.integers(-(T // 2), T // 2 + 1, N).astype(np.int64)
    m[:4] = [0, T // 2, -(T // 2), 1]
    up = mkbfv.ScaleUp(m, params)
    assert up.dtype == np.uint64 and (up == kg.encode(m)).all()
    assert (mkbfv.ScaleDown(up, params) == m).all()
    noisy = H.uniform_poly(rng, pset["Q"], N)
    got = mkbfv.ScaleDown(noisy, params)
    assert got.dtype == np.int64 and (got == kg.decode(noisy)).all()


def test_key_sets():
    from mkhe_kklss_amd import mkrlwe
    from mkhe_kklss_amd._abi import MkheError
    for new, add, dele, get in ((mkrlwe.NewSecretKeySet, "AddSecretKey", "DelSecretKey", "GetSecretKey"),
                                (mkrlwe.NewPublicKeyKeySet, "AddPublicKey", "DelPublicKey", "GetPublicKey")):
        s = new()
        a, b, a2 = (types.SimpleNamespace(ID=i) for i in ("a", "b", "a"))
        getattr(s, add)(a)
        getattr(s, add)(b)
        assert getattr(s, get)("a") is a and getattr(s, get)("b") is b and set(s.Value) == {"a", "b"}
        getattr(s, add)(a2)                              # the same id replaces (keys.go:78,105)
        assert getattr(s, get)("a") is a2 and len(s.Value) == 2
        getattr(s, dele)("a")
        getattr(s, dele)("nobody")                       # deleting a missing id is a no-op, like Go's delete
        assert set(s.Value) == {"b"}
        with pytest.raises(MkheError, match="there is no public key with given id"):
            getattr(s, get)("a")


def test_new_symbols_are_bound():
    from mkhe_kklss_amd import _abi
    for name in ("mkhe_encrypt", "mkhe_partial_decrypt", "mkhe_decrypt"):
        assert name in _abi.SIGNATURES
        assert hasattr(_abi.lib(), name)


def test_mirror_names():
    from mkhe_kklss_amd import mkbfv, mkckks, mkrlwe
    for mod, names in ((mkrlwe, "SecretKeySet PublicKeySet Encryptor Decryptor NewEncryptor NewDecryptor"),
                       (mkckks, "Message NewMessage Encoder Encryptor Decryptor NewEncryptor NewDecryptor"),
                       (mkbfv, "Encryptor Decryptor NewEncryptor NewDecryptor ScaleUp ScaleDown")):
        for n in names.split():
            assert hasattr(mod, n), "%s.%s" % (mod.__name__, n)
    for n in "EncryptPtxt EncryptMsg EncryptMsgNew EncodeMsgNew EncryptBatch".split():
        assert hasattr(mkckks.Encryptor, n)
