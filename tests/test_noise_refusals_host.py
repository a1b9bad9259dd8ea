"""The refusals of mkhe_noise_norm that need no context (no GPU), in the style of test_capi_refusals_host.py: the call passes a NULL context and is
turned away before any HIP call, so the exact mkhe_last_error() can be pinned here.  The scalar checks come first; then the call reports
`mkhe_noise_norm: null context`, as the protocol family does."""
import ctypes as C

import pytest

BUF = C.c_void_p(4096)          # never dereferenced: the call is refused before it looks at a buffer

# (arguments behind the context: kind, limbs, count, dev_phase, dev_ref, ref_stride_words, dev_out; message)
ROWS = [
    ((2, 1, 1, None, None, 0, None), "mkhe_noise_norm: kind must be 0 (residual) or 1 (BFV invariant)"),
    ((-1, 1, 1, None, None, 0, None), "mkhe_noise_norm: kind must be 0 (residual) or 1 (BFV invariant)"),
    ((0, 1, 0, None, None, 0, None), "mkhe_noise_norm: count must be 1 .. 65535"),
    ((0, 1, 65536, None, None, 0, None), "mkhe_noise_norm: count must be 1 .. 65535"),
    ((0, 0, 1, None, None, 0, None), "mkhe_noise_norm: limbs out of range"),
    ((1, -3, 1, None, None, 0, None), "mkhe_noise_norm: limbs out of range"),
    ((1, 3, 1, BUF, BUF, 0, BUF), "mkhe_noise_norm: kind 1 takes no reference (dev_ref must be NULL)"),
    ((0, 1, 1, None, None, 0, None), "mkhe_noise_norm: null context"),
    ((1, 3, 2, BUF, None, 0, BUF), "mkhe_noise_norm: null context"),
    ((0, 4, 65535, BUF, BUF, 7, BUF), "mkhe_noise_norm: null context"),
]


@pytest.mark.parametrize("args,message", ROWS, ids=[str(i) for i in range(len(ROWS))])
def test_a_call_without_a_context_is_refused_with_exactly_this_message(args, message):
    from mkhe_kklss_amd._abi import lib
    # a message of another call first, so that the one read back is this call's
    assert lib().mkhe_swk_fold(None, None, 0, 0) == 1 and lib().mkhe_last_error().decode() == "mkhe_swk_fold: null argument"
    assert lib().mkhe_noise_norm(None, *args) == 1
    assert lib().mkhe_last_error().decode() == message
