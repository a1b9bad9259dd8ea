"""The refusals of mkhe_ct_lincomb_batch and of the BatchEvaluator sums that need no device (no GPU).
Through the C ABI, in the style of tests/test_capi_refusals_host.py: the counts and nb_rescale are checked before the context is looked at, then a NULL
context is reported under the function's own name.  On the Python side: BatchEvaluator.LinCombNew / LinCombsNew raise MkheError on a wrong batch length,
more than 16 rows or mismatched ids before anything reaches the engine -- the operands here are stand-ins without handles, and every way into the
engine (the library, the constants upload, the output allocation) is replaced by a function that fails the test."""
import types

import pytest

import harness as H

NAME = "mkhe_ct_lincomb_batch"

# (nbatch, nin, nout, nb_rescale, message)
ROWS = [
    (0, 1, 1, 0, NAME + ": nbatch must be at least 1"),
    (-1, 16, 16, 1, NAME + ": nbatch must be at least 1"),
    (0, 0, 0, 2, NAME + ": nbatch must be at least 1"),
    (1, 0, 1, 0, NAME + ": nin must be 1 .. 16"),
    (2, 17, 1, 0, NAME + ": nin must be 1 .. 16"),
    (1, -1, 1, 1, NAME + ": nin must be 1 .. 16"),
    (1, 16, 0, 0, NAME + ": nout must be 1 .. 16"),
    (33, 16, 17, 1, NAME + ": nout must be 1 .. 16"),
    (1, 1, 1, -1, NAME + ": nb_rescale must be 0 or 1"),
    (5, 16, 16, 2, NAME + ": nb_rescale must be 0 or 1"),
    (1, 1, 1, 0, NAME + ": null context"),
    (1000000, 16, 16, 1, NAME + ": null context"),
]


@pytest.mark.parametrize("nbatch,nin,nout,nb,message", ROWS, ids=["%d-%d-%d-%d" % r[:4] for r in ROWS])
def test_a_call_without_a_context_is_refused_with_exactly_this_message(nbatch, nin, nout, nb, message):
    from mkhe_kklss_amd._abi import lib
    # a message of another call first, so that the one read back is this call's
    assert lib().mkhe_swk_fold(None, None, 0, 0) == 1 and lib().mkhe_last_error().decode() == "mkhe_swk_fold: null argument"
    assert lib().mkhe_ct_lincomb_batch(None, nbatch, nin, None, nout, None, nb, None) == 1
    assert lib().mkhe_last_error().decode() == message


class StandIn:
    """what the checks read of a ciphertext: ids, level, scale; no handle"""

    def __init__(self, ids, level=3, scale=2.0 ** 30):
        self.ids, self.Scale, self.h, self.params, self._level = list(ids), scale, None, None, level

    def Level(self): return self._level
    def IDSet(self): return set(self.ids)


@pytest.fixture
def bev(monkeypatch):
    from mkhe_kklss_amd import mkckks, mkrlwe

    def engine(*a, **k):
        raise AssertionError("the engine was reached")

    monkeypatch.setattr(mkckks, "lib", engine)
    monkeypatch.setattr(mkckks, "_upload_consts", engine)
    monkeypatch.setattr(mkrlwe, "batch_ciphertexts", engine)
    pset = H.small_ckks(10, nq=4)
    params = types.SimpleNamespace(Q=pset["Q"], Scale=lambda: 2.0 ** 30, ctx=None, N=lambda: 1 << 10)
    return mkckks.BatchEvaluator(params, 2, ev=object())


def batch(n, ids=("a", "b")):
    from mkhe_kklss_amd import mkckks
    return mkckks.BatchCiphertext([StandIn(ids) for _ in range(n)])


def test_a_batch_of_the_wrong_length_is_refused(bev):
    from mkhe_kklss_amd._abi import MkheError
    for cts in ([batch(3)], [batch(2), batch(1)], [StandIn(("a", "b")), batch(3)]):
        with pytest.raises(MkheError, match="a batch of [13] ciphertexts on an evaluator of 2 inputs"):
            bev.LinCombNew(cts, [1] * len(cts))
        with pytest.raises(MkheError, match="a batch of [13] ciphertexts on an evaluator of 2 inputs"):
            bev.LinCombsNew(cts, [[1] * len(cts)] * 2, [0, 0])
    with pytest.raises(MkheError, match="a batch of 3 ciphertexts"):
        bev.AddConstNew(batch(3), 1)


def test_more_than_16_rows_are_refused(bev):
    from mkhe_kklss_amd._abi import MkheError
    with pytest.raises(MkheError, match="LinCombsNew: 1 to 16 rows of weights per call, one constant per row"):
        bev.LinCombsNew([batch(2)], [[1]] * 17, [0] * 17)
    with pytest.raises(MkheError, match="LinCombsNew: 1 to 16 rows of weights per call, one constant per row"):
        bev.LinCombsNew([batch(2)], [], [])
    with pytest.raises(MkheError, match="LinCombNew: at most 16 non-zero weights per call"):
        bev.LinCombNew([batch(2)] * 17, [1] * 17)


def test_mismatched_ids_are_refused(bev):
    from mkhe_kklss_amd._abi import MkheError
    with pytest.raises(MkheError, match="LinCombNew: the ciphertexts must carry the same ids"):
        bev.LinCombNew([batch(2), batch(2, ("a", "c"))], [1, 1])
    with pytest.raises(MkheError, match="LinCombsNew: the ciphertexts must carry the same ids"):
        bev.LinCombsNew([batch(2), StandIn(("a",))], [[1, 1]], [0])


def test_setting_the_scale_of_a_batch_sets_every_member():
    b = batch(3)
    assert b.Scale == 2.0 ** 30
    b.Scale = 2.0 ** 31
    assert b.Scale == 2.0 ** 31 and all(c.Scale == 2.0 ** 31 for c in b.cts)
