"""cnn.Inference(sum_products=True) on the device (-m gpu): Convolution relinearises the sum of its four products and FC1Layer the sum of its eight
(mkhe_mul_relin_sum) instead of every summand -- a different ciphertext of the same logits.  The smallest setting of tests/test_gpu_cnn.py: two
parties, the synthetic model.

Bound on the difference of the logits: the sum of the two layers' bounds, each the reference's MulRelin bound -log2(scale) + logSlots + 12
(mkckks_test.go:357) plus log2 K of its K summands: 2^(-47 + 13 + 12 + 2) + 2^(-47 + 13 + 12 + 3) = 2^-20 + 2^-19."""
import math

import numpy as np
import pytest

import harness_cnn as HC

pytestmark = pytest.mark.gpu

TWO = dict(image="dataOwner", kernels="modelOwner", fc1="modelOwner", fc2="modelOwner")


def test_summed_products_give_the_same_logits():
    from mkhe_kklss_amd import cnn
    sc = HC.CnnScenario(TWO, seed=3)
    model = HC.synthetic_model(7)
    cts = sc.encrypt_model(model)
    pt, pt_scale = sc.mask_plaintext(sc.level - 4)
    args = (sc.eval, sc.rlkSet, sc.rtkSet, cts["ctImage"], cts["ctKernels"], cts["ctFC1"], cts["ctFC2"], cts["ctB1"], cts["ctB2"], pt, pt_scale)
    ref = cnn.Inference(*args)
    out = cnn.Inference(*args, sum_products=True)
    assert out.ids == ref.ids and out.Level() == ref.Level() == 0 and out.Scale == ref.Scale
    a, b = sc.decrypt(out)[:HC.NCLS].real, sc.decrypt(ref)[:HC.NCLS].real
    layer = lambda K: 2.0 ** (-math.log2(sc.scale) + (HC.PN14QP433["logN"] - 1) + 12 + math.log2(K))
    bound = layer(4) + layer(8)
    print("logits", np.round(b, 4), "max |difference| 2^%.1f, bound 2^%.1f" % (math.log2(max(np.abs(a - b).max(), 1e-300)), math.log2(bound)))
    assert int(np.argmax(a)) == int(np.argmax(b)) == int(np.argmax(HC.plain_forward(model)))
    assert np.abs(a - b).max() <= bound
    assert (out.download() != ref.download()).any()          # (one gadget noise per layer instead of one per summand: not the same ciphertext)


def test_sum_products_is_for_the_plain_evaluator_on_one_context():
    """forks and evaluators without MulRelinSumNew (a BatchEvaluator) are refused before anything is computed"""
    from mkhe_kklss_amd import cnn
    from mkhe_kklss_amd._abi import MkheError
    with pytest.raises(MkheError, match="sum_products"):
        cnn.Convolution(object(), None, None, None, None, [], [], sum_products=True)
    with pytest.raises(MkheError, match="sum_products"):
        cnn.FC1Layer(type("E", (), {"MulRelinSumNew": None})(), None, None, None, None, [], [], None, forks=[object()], sum_products=True)
