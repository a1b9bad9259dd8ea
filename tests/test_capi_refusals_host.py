"""The refusals of the sampler, protocol and encoder entry points that need no context (no GPU): every call passes a NULL context and is turned
away before any HIP call, so the exact mkhe_last_error() and the return code of each can be pinned here.  Scalar ranges, null keys and nonces are
checked before the context is looked at; the sampler and protocol families then report `<entry>: null context`, the two encoders and mkhe_encrypt
the `mkhe: null context` of every other entry point."""
import ctypes as C

import pytest

KEY = (C.c_uint32 * 8)(*range(1, 9))
KEY2 = (C.c_uint32 * 8)(*range(11, 19))
CDT = (C.c_uint64 * 2)(1, 2)
ANON = "mkhe: null context"


def named(entry):
    return entry + ": null context"


DIFFER = ": nonce_mask and nonce_enc must differ (the mask and the encryption would share streams)"

# (entry, arguments behind the context, return code, message)
ROWS = [
    ("mkhe_sample_small", (2, 1, KEY, 0, 0, None, 0, None), 1, "mkhe_sample_small: kind must be 0 (ternary) or 1 (table)"),
    ("mkhe_sample_small", (0, 1, KEY, 0, 0, None, 0, None), 1, named("mkhe_sample_small")),
    ("mkhe_encrypt_seeded", (0, 1, None, None, 0, KEY, 0, CDT, 2, None), 1, named("mkhe_encrypt_seeded")),
    ("mkhe_sample_uniform", (1, 1, KEY, 0, None), 1, named("mkhe_sample_uniform")),
    ("mkhe_ct_expand_seeded", (1, KEY, 0, None), 1, named("mkhe_ct_expand_seeded")),
    ("mkhe_encrypt_sk", (0, 1, None, None, 0, KEY, 0, None, None), 1, named("mkhe_encrypt_sk")),
    ("mkhe_encrypt_sk_seeded", (0, 1, None, None, 0, KEY, 0, KEY2, 1, CDT, 2, None), 1, named("mkhe_encrypt_sk_seeded")),
    ("mkhe_decrypt_merge", (1, None, 0, None, None), 1, named("mkhe_decrypt_merge")),
    ("mkhe_refresh_merge", (1, None, 0, None, None, None), 1, named("mkhe_refresh_merge")),
    ("mkhe_bfv_refresh_merge", (1, None, 0, None, None, None), 1, named("mkhe_bfv_refresh_merge")),
    ("mkhe_pcks_merge", (1, None, 0, None, None), 1, named("mkhe_pcks_merge")),
    ("mkhe_decrypt_share", (1, None, None, None, KEY, 0, 63, None), 1, "mkhe_decrypt_share: flood_bits must be 0 .. 62"),
    ("mkhe_decrypt_share", (1, None, None, None, None, 0, 1, None), 1, "mkhe_decrypt_share: null key"),
    ("mkhe_decrypt_share", (1, None, None, None, None, 0, 0, None), 1, named("mkhe_decrypt_share")),
    ("mkhe_refresh_share", (1, None, None, None, None, KEY, 1, 2, 121, CDT, 2, None, None), 1, "mkhe_refresh_share: mask_bits must be 0 .. 120"),
    ("mkhe_refresh_share", (1, None, None, None, None, None, 1, 2, 1, CDT, 2, None, None), 1, "mkhe_refresh_share: null key"),
    ("mkhe_refresh_share", (1, None, None, None, None, KEY, 5, 5, 1, CDT, 2, None, None), 1, "mkhe_refresh_share" + DIFFER),
    ("mkhe_refresh_share", (1, None, None, None, None, KEY, 5, 5, 0, CDT, 2, None, None), 1, named("mkhe_refresh_share")),
    ("mkhe_bfv_refresh_share", (1, None, None, None, None, KEY, 1, 2, 2, 0, CDT, 2, None, None), 1, "mkhe_bfv_refresh_share: mask must be 0 or 1"),
    ("mkhe_bfv_refresh_share", (1, None, None, None, None, KEY, 1, 2, 1, 1025, CDT, 2, None, None), 1,
     "mkhe_bfv_refresh_share: flood_bits must be 0 .. 1024"),
    ("mkhe_bfv_refresh_share", (1, None, None, None, None, None, 1, 2, 1, 0, CDT, 2, None, None), 1, "mkhe_bfv_refresh_share: null key"),
    ("mkhe_bfv_refresh_share", (1, None, None, None, None, KEY, 5, 5, 1, 0, CDT, 2, None, None), 1, "mkhe_bfv_refresh_share" + DIFFER),
    ("mkhe_bfv_refresh_share", (1, None, None, None, None, KEY, 5, 5, 0, 0, CDT, 2, None, None), 1, named("mkhe_bfv_refresh_share")),
    ("mkhe_pcks_share", (1, None, None, None, None, KEY, 0, 1025, CDT, 2, None), 1, "mkhe_pcks_share: flood_bits must be 0 .. 1024"),
    ("mkhe_pcks_share", (1, None, None, None, None, None, 0, 0, CDT, 2, None), 1, "mkhe_pcks_share: null key"),
    ("mkhe_pcks_share", (1, None, None, None, None, KEY, 0, 0, CDT, 2, None), 1, named("mkhe_pcks_share")),
    ("mkhe_ckks_encode", (0, 1, None, 0.0, None), 1, "mkhe_ckks_encode: scale must be finite and positive"),
    ("mkhe_ckks_encode", (0, 1, None, 1.0, None), 1, ANON),
    ("mkhe_ckks_embed", (1, None, None), 1, ANON),
    ("mkhe_ctx_set_ckks_tile", (10,), 1, ANON),
    ("mkhe_bfv_encode", (1, None, None), 1, ANON),
    ("mkhe_bfv_ct_add_ptxt", (7, 1, None, None, 0, None), 1, ANON),
    ("mkhe_encrypt", (0, 1, None, None, 0, None, None), 1, ANON),
    ("mkhe_ctx_ckks_tile", (), -1, ANON),
    ("mkhe_ctx_bfv_tile", (), -1, ANON),
]


@pytest.mark.parametrize("entry,args,rc,message", ROWS, ids=["%s-%d" % (r[0], i) for i, r in enumerate(ROWS)])
def test_a_call_without_a_context_is_refused_with_exactly_this_message(entry, args, rc, message):
    from mkhe_kklss_amd._abi import lib
    # a message of another call first, so that the one read back is this call's
    assert lib().mkhe_swk_fold(None, None, 0, 0) == 1 and lib().mkhe_last_error().decode() == "mkhe_swk_fold: null argument"
    assert getattr(lib(), entry)(None, *args) == rc
    assert lib().mkhe_last_error().decode() == message
