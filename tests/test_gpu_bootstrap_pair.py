"""The two halves of a bootstrapping through EvalMod as ONE batch of two (-m gpu), in the world of tests/test_gpu_bootstrap_e2e.py (imported: logN = 10,
logSlots = 3, two parties of Hamming weight 32): Bootstrapper.EvalModNew on BatchCiphertext([lo, hi]) with a BatchEvaluator gives the two single
calls bit for bit, and BootstrapNew(pair=True) gives BootstrapNew(pair=False) bit for bit.  What the result decodes to is that file's subject."""
import pytest

import test_gpu_bootstrap_e2e as BE

pytestmark = pytest.mark.gpu


def _same(a, b):
    return a.Level() == b.Level() and a.Scale == b.Scale and a.ids == b.ids and (a.download() == b.download()).all()


def test_eval_mod_on_the_pair_equals_the_two_single_calls():
    w = BE.world(3, 2, 32)
    ct, _ = BE.encrypted_sum(w)
    lo, hi = w.boot.CoeffsToSlotsNew(ct, w.rks, w.cks)
    both = w.boot.EvalModNew(w.mkckks.BatchCiphertext([lo, hi]), w.rlk, BE.RATIO, w.mkckks.BatchEvaluator(w.params, 2, ev=w.ev))
    assert len(both) == 2 and both.Scale == both.cts[0].Scale == both.cts[1].Scale
    assert _same(both.cts[0], w.boot.EvalModNew(lo, w.rlk, BE.RATIO, w.ev)) and _same(both.cts[1], w.boot.EvalModNew(hi, w.rlk, BE.RATIO, w.ev))
    # a batch needs a batch evaluator of its length
    for ev in (w.ev, w.mkckks.BatchEvaluator(w.params, 3, ev=w.ev)):
        with pytest.raises(w.mkckks.MkheError):
            w.boot.EvalModNew(w.mkckks.BatchCiphertext([lo, hi]), w.rlk, BE.RATIO, ev)


def test_bootstrap_with_the_pair_equals_the_default():
    w = BE.world(3, 2, 32)
    ct15, _ = BE.encrypted_sum(w, radius=0.5)
    ct = w.ev.DropLevelNew(ct15, 15)
    one = w.boot.BootstrapNew(ct, w.rlk, w.rks, w.cks)
    assert _same(w.boot.BootstrapNew(ct, w.rlk, w.rks, w.cks, pair=True), one) and _same(w.boot.BootstrapNew(ct, w.rlk, w.rks, w.cks, pair=False), one)
    assert one.Level() == 15 - 12 and one.Scale == BE.SCALE
