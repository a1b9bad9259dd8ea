"""The guard that the sampler, protocol and encoder entry points share (-m gpu), N = 2^10: the exact message of each of its steps, one row per
entry -- the count range, the null input list, the scheme of the context and the context that owns a subset of the moduli.  One mkrlwe context,
one ciphertext over one party at the top level and one device buffer; in every row the key is present, the scalars are in range, the two nonces
differ and every pointer that the step under test does not look at is NULL.  Each refusal is followed by a call that works."""
import ctypes as C

import numpy as np
import pytest

import harness as H

pytestmark = pytest.mark.gpu

LOGN = 10
KEY = (C.c_uint32 * 8)(0x9E3779B9, 0x7F4A7C15, 0xF39CC060, 0x5CEDC834, 0x1082276B, 0xF3A27251, 0xF86C6A11, 0xD0C18E95)
KEY2 = (C.c_uint32 * 8)(*range(1, 9))
CDT = (C.c_uint64 * 2)(1, 2)
IN, OUT, SLOTS, COEFFS = "in", "out", "slots", "coeffs"        # stand for the ciphertext list, the buffer and its two halves

# entry -> its arguments behind the context, with the count and the places of the ciphertext list and of the output buffer left open
SHARE_MERGE = {
    "mkhe_decrypt_share": lambda n, i, o: (n, i, None, None, KEY, 7, 1, o),
    "mkhe_decrypt_merge": lambda n, i, o: (n, i, 1, None, o),
    "mkhe_refresh_share": lambda n, i, o: (n, i, None, None, None, KEY, 1, 2, 1, None, 0, o, None),
    "mkhe_refresh_merge": lambda n, i, o: (n, i, 1, None, None, None),
    "mkhe_bfv_refresh_share": lambda n, i, o: (n, i, None, None, None, KEY, 1, 2, 1, 1, None, 0, o, None),
    "mkhe_bfv_refresh_merge": lambda n, i, o: (n, i, 1, None, None, None),
    "mkhe_pcks_share": lambda n, i, o: (n, i, None, None, None, KEY, 7, 1, None, 0, o),
    "mkhe_pcks_merge": lambda n, i, o: (n, i, 1, None, None),
}
CKKS_SIDE = [e for e in SHARE_MERGE if "bfv" not in e]
COUNTED = dict(SHARE_MERGE, **{
    "mkhe_sample_uniform": lambda n, i, o: (1, n, KEY, 7, None),
    "mkhe_ct_expand_seeded": lambda n, i, o: (n, KEY, 7, None),
    "mkhe_ckks_embed": lambda n, i, o: (n, SLOTS, COEFFS),
})
MASKED = dict({e: SHARE_MERGE[e](1, IN, OUT) for e in CKKS_SIDE}, **{
    "mkhe_sample_small": (0, 1, KEY, 7, 0, None, 0, None),
    "mkhe_sample_uniform": (1, 1, KEY, 7, None),
    "mkhe_ct_expand_seeded": (1, KEY, 7, None),
    "mkhe_encrypt_seeded": (0, 1, None, None, 0, KEY, 7, CDT, 2, None),
    "mkhe_encrypt_sk": (0, 1, None, None, 0, KEY, 7, None, None),
    "mkhe_encrypt_sk_seeded": (0, 1, None, None, 0, KEY, 7, KEY2, 8, CDT, 2, None),
    "mkhe_ckks_embed": (1, SLOTS, COEFFS),
})
BFV_ONLY = ": needs a BFV context (mkhe_refresh_share / mkhe_refresh_merge serve the others)"


class World:
    def __init__(self):
        from mkhe_kklss_amd import mkrlwe
        from mkhe_kklss_amd._abi import handle_array, lib
        pset = H.small_ckks(LOGN, 4)
        self.lib, L, N = lib(), len(pset["Q"]), 1 << LOGN
        self.params = mkrlwe.Parameters(pset["logN"], pset["Q"], pset["P"])
        self.ct = mkrlwe.Ciphertext(self.params, ["user0"], L - 1)
        self.buf = mkrlwe.DeviceLimbs(self.params, 2, L).upload(np.zeros((2, L, N), dtype=np.uint64))
        self.places = {IN: handle_array([self.ct.h]), OUT: self.buf.devptr(), SLOTS: self.buf.devptr(),
                       COEFFS: C.c_void_p(self.buf.devptr().value + 8 * L * N)}
        assert self.buf.devptr().value % 16 == 0

    def call(self, entry, args):
        """-> (return code, message) of one call, with the names of the places filled in"""
        rc = getattr(self.lib, entry)(self.params.ctx, *[self.places[a] if isinstance(a, str) else a for a in args])
        return rc, self.lib.mkhe_last_error().decode()

    def works(self):
        assert self.call("mkhe_ckks_embed", (1, SLOTS, COEFFS))[0] == 0, self.lib.mkhe_last_error().decode()
        assert self.lib.mkhe_ctx_sync(self.params.ctx) == 0


@pytest.fixture(scope="module")
def w():
    world = World()
    yield world
    world.params.close()


@pytest.mark.parametrize("count", [0, 65536])
@pytest.mark.parametrize("entry", sorted(COUNTED))
def test_count_out_of_range(w, entry, count):
    assert w.call(entry, COUNTED[entry](count, None, None)) == (1, entry + ": count must be 1 .. 65535")
    w.works()


@pytest.mark.parametrize("entry", sorted(SHARE_MERGE))
def test_null_input_list(w, entry):
    assert w.call(entry, SHARE_MERGE[entry](1, None, None)) == (1, entry + ": null argument")
    w.works()


@pytest.mark.parametrize("entry,args,message", [
    ("mkhe_bfv_refresh_share", SHARE_MERGE["mkhe_bfv_refresh_share"](1, IN, None), "mkhe_bfv_refresh_share" + BFV_ONLY),
    ("mkhe_bfv_refresh_merge", SHARE_MERGE["mkhe_bfv_refresh_merge"](1, IN, None), "mkhe_bfv_refresh_merge" + BFV_ONLY),
    ("mkhe_bfv_encode", (1, SLOTS, COEFFS), "mkhe_bfv_encode: the BFV encoder needs a BFV context"),
], ids=["mkhe_bfv_refresh_share", "mkhe_bfv_refresh_merge", "mkhe_bfv_encode"])
def test_wrong_scheme(w, entry, args, message):
    assert w.call(entry, args) == (1, message)
    w.works()


@pytest.mark.parametrize("entry", sorted(MASKED))
def test_context_that_owns_a_subset_of_the_moduli(w, entry):
    own = (C.c_int * 2)(0, 2)
    assert w.lib.mkhe_ctx_set_owned(w.params.ctx, own, 2) == 0, w.lib.mkhe_last_error().decode()
    try:
        got = w.call(entry, MASKED[entry])
    finally:
        assert w.lib.mkhe_ctx_set_owned(w.params.ctx, own, 0) == 0
    assert got == (1, entry + ": not available on a context that owns a subset of the moduli")
    w.works()
