"""The refusals of mkhe_bfv_ct_ptxt_dot that need no device (no GPU), in the style of tests/test_capi_refusals_host.py: the counts are checked before
the context is looked at, then a NULL context is reported under the function's own name.  Nothing reaches a HIP call."""
import ctypes as C

import pytest

NAME = "mkhe_bfv_ct_ptxt_dot"
MASKS = (C.c_uint32 * 1)(1)

# (nbatch, nin, ngiant, message)
ROWS = [
    (0, 1, 1, NAME + ": nbatch must be 1 .. 16"),
    (17, 1, 1, NAME + ": nbatch must be 1 .. 16"),
    (-1, 1, 1, NAME + ": nbatch must be 1 .. 16"),
    (1, 0, 1, NAME + ": nin must be 1 .. 16"),
    (1, 17, 1, NAME + ": nin must be 1 .. 16"),
    (16, 16, 0, NAME + ": ngiant must be 1 .. 64"),
    (16, 16, 65, NAME + ": ngiant must be 1 .. 64"),
    (1, 1, 1, NAME + ": null context"),
    (16, 16, 64, NAME + ": null context"),
]


@pytest.mark.parametrize("nbatch,nin,ngiant,message", ROWS, ids=["%d-%d-%d" % r[:3] for r in ROWS])
def test_a_call_without_a_context_is_refused_with_exactly_this_message(nbatch, nin, ngiant, message):
    from mkhe_kklss_amd._abi import lib
    # a message of another call first, so that the one read back is this call's
    assert lib().mkhe_swk_fold(None, None, 0, 0) == 1 and lib().mkhe_last_error().decode() == "mkhe_swk_fold: null argument"
    assert lib().mkhe_bfv_ct_ptxt_dot(None, nbatch, nin, None, ngiant, MASKS, None, None) == 1
    assert lib().mkhe_last_error().decode() == message
