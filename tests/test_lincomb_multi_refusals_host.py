"""The refusals of mkhe_ct_lincomb_multi that need no device (no GPU), in the style of tests/test_bfv_lincomb_refusals_host.py: the counts and
nb_rescale are checked before the context is looked at, then a NULL context is reported under the function's own name.  Nothing reaches a HIP call."""
import pytest

NAME = "mkhe_ct_lincomb_multi"

# (nin, nout, nb_rescale, message)
ROWS = [
    (0, 1, 0, NAME + ": nin must be 1 .. 16"),
    (17, 1, 0, NAME + ": nin must be 1 .. 16"),
    (-1, 1, 1, NAME + ": nin must be 1 .. 16"),
    (16, 0, 0, NAME + ": nout must be 1 .. 16"),
    (16, 17, 1, NAME + ": nout must be 1 .. 16"),
    (1, 1, -1, NAME + ": nb_rescale must be 0 or 1"),
    (16, 16, 2, NAME + ": nb_rescale must be 0 or 1"),
    (1, 1, 0, NAME + ": null context"),
    (16, 16, 1, NAME + ": null context"),
]


@pytest.mark.parametrize("nin,nout,nb,message", ROWS, ids=["%d-%d-%d" % r[:3] for r in ROWS])
def test_a_call_without_a_context_is_refused_with_exactly_this_message(nin, nout, nb, message):
    from mkhe_kklss_amd._abi import lib
    # a message of another call first, so that the one read back is this call's
    assert lib().mkhe_swk_fold(None, None, 0, 0) == 1 and lib().mkhe_last_error().decode() == "mkhe_swk_fold: null argument"
    assert lib().mkhe_ct_lincomb_multi(None, nin, None, nout, None, nb, None) == 1
    assert lib().mkhe_last_error().decode() == message
