"""mkhe_ct_lincomb_batch (-m gpu): nbatch independent items, each the nout sums of its own nin inputs, all with ONE constant block.  Every item is compared,
bit for bit, with the Python-integer model of tests/test_gpu_lincomb_multi.py (imported: the formulas of include/mkhe.h and the rounding rule of
DivRoundByLastModulus) and with mkhe_ct_lincomb_multi called on that item with the same block.  Weights and constants are independent uniform residues
per limb, as there.

One launch holds 384 / (nin + nout) items (CTLB_MAX_PTRS of csrc/poly_kernels.h): 12 at 16 x 16 and 128 at 2 x 1, so 33 items at 16 x 16 are three launches
and 129 items at 2 x 1 two, the second with a single item."""
import os
import subprocess
import sys

import numpy as np
import pytest

import harness as H
import harness_bfv as HB
import test_gpu_lincomb_multi as T

pytestmark = pytest.mark.gpu

NAME = "mkhe_ct_lincomb_batch: "


@pytest.fixture(scope="module")
def worlds():
    return {logN: T.World(H.small_ckks(logN, nq=6)) for logN in (10, 12)}


def batch(w, items, consts, nb, outs):
    """items[b] = the nin inputs of item b, outs[b] = its nout outputs"""
    return w.lib.mkhe_ct_lincomb_batch(w.params.ctx, len(items), len(items[0]), w.handle_array([c.h for it in items for c in it]), len(outs[0]),
                                       consts.devptr(), nb, w.handle_array([c.h for o in outs for c in o]))


def check(w, hosts, table, Lc, nb, ids, items=None):
    """hosts[b] = the host inputs of item b (items[b]: their ciphertexts, when some are shared).  The call against the model and against
    mkhe_ct_lincomb_multi, item by item"""
    items = [[w.ct(x, ids) for x in hs] for hs in hosts] if items is None else items
    outs = [[w.new(ids, Lc - nb) for _ in table] for _ in hosts]
    consts = w.consts(table, Lc)
    assert batch(w, items, consts, nb, outs) == 0, w.error()
    one = [w.new(ids, Lc - nb) for _ in table]
    got = []
    for b, hs in enumerate(hosts):
        got.append([o.download() for o in outs[b]])
        ref = T.model(w.Q, hs, table, Lc, nb)
        assert w.multi(items[b], consts, nb, one) == 0, w.error()
        for g in range(len(table)):
            assert got[b][g].shape == ref[g].shape and (got[b][g] == ref[g]).all(), "item %d, row %d differs from the model" % (b, g)
            assert (one[g].download() == got[b][g]).all(), "item %d, row %d differs from mkhe_ct_lincomb_multi" % (b, g)
    return got


def draw(rng, w, nbatch, nin, nout, polys, limbs, Lc):
    """nbatch independent sets of inputs and one table"""
    hosts, table = T.draw(rng, w.Q, w.N, nin, nout, polys, limbs, Lc)
    return [hosts] + [T.draw(rng, w.Q, w.N, nin, 1, polys, limbs, Lc)[0] for _ in range(nbatch - 1)], table


@pytest.mark.parametrize("nbatch", [1, 2, 5])
@pytest.mark.parametrize("Lc,nb", [(1, 0), (2, 1), (4, 0), (4, 1)])
@pytest.mark.parametrize("nin,nout", [(1, 1), (5, 2), (9, 7), (16, 16), (16, 1)])          # every NI and NO of the kernel
@pytest.mark.parametrize("parties", [1, 3])
@pytest.mark.parametrize("logN", [10, 12])          # N/2 pairs = 2 and 8 workgroups of 256 per row and item
def test_basic_shapes(worlds, logN, parties, nin, nout, Lc, nb, nbatch):
    w = worlds[logN]
    rng = np.random.default_rng([logN, parties, nin, nout, Lc, nb, nbatch])
    hosts, table = draw(rng, w, nbatch, nin, nout, 1 + parties, Lc, Lc)
    check(w, hosts, table, Lc, nb, ["p%d" % i for i in range(parties)])


@pytest.mark.parametrize("nbatch,nin,nout", [(33, 16, 16), (65, 2, 1), (129, 2, 1)], ids=["33x16x16", "65x2x1", "129x2x1"])
def test_more_items_than_one_launch_holds(worlds, nbatch, nin, nout):
    """33 * 32 = 1056 base addresses are over any kernel-argument block; 129 items at 2 x 1 are one more than this launcher's 128 per launch"""
    w, Lc = worlds[10], 2
    rng = np.random.default_rng([nbatch, nin, nout])
    hosts, table = draw(rng, w, nbatch, nin, nout, 2, Lc, Lc)
    check(w, hosts, table, Lc, 1, ["p0"])


@pytest.mark.parametrize("nb", [0, 1])
def test_inputs_with_more_limbs_than_the_sums(worlds, nb):
    w, Lc = worlds[10], 3
    rng = np.random.default_rng(177 + nb)
    hosts, table = draw(rng, w, 3, 3, 5, 3, Lc + 2, Lc)
    check(w, hosts, table, Lc, nb, ["p0", "p1"])
    # input k deeper than input k': input 1 at Lc limbs, input 2 at Lc + 1, input 0 at Lc + 2, in every item
    hosts = [[hs[0], hs[1][:, :Lc], hs[2][:, : Lc + 1]] for hs in hosts]
    check(w, hosts, table, Lc, nb, ["p0", "p1"])


@pytest.mark.parametrize("nb", [0, 1])
def test_a_broadcast_input(worlds, nb):
    """input 1 is ONE ciphertext, shared by all items (the model operand of a batched circuit)"""
    w, Lc, ids = worlds[10], 3, ["p0", "p1"]
    rng = np.random.default_rng(277 + nb)
    hosts, table = draw(rng, w, 4, 3, 2, 3, Lc, Lc)
    hosts = [[hs[0], hosts[0][1], hs[2]] for hs in hosts]
    shared = w.ct(hosts[0][1], ids)
    items = [[w.ct(hs[0], ids), shared, w.ct(hs[2], ids)] for hs in hosts]
    check(w, hosts, table, Lc, nb, ids, items)


@pytest.mark.parametrize("nb", [0, 1])
def test_a_row_of_zero_weights(worlds, nb):
    w, Lc, ids = worlds[10], 3, ["p0", "p1"]
    rng = np.random.default_rng(377 + nb)
    zero = [0] * Lc
    hosts, table = draw(rng, w, 3, 5, 4, 3, Lc, Lc)
    table[1] = (table[1][0], [(zero, zero)] * 5)
    got = check(w, hosts, table, Lc, nb, ids)
    if not nb:
        want = np.zeros_like(got[0][1])
        want[0, :, 0], want[0, :, w.N // 2] = table[1][0][0], table[1][0][1]
        assert all((g[1] == want).all() for g in got)


@pytest.mark.parametrize("nb", [0, 1])
def test_worst_case_accumulation(nb):
    """16 x 16, every residue, weight and constant q - 1 over a 60-bit and a 54-bit prime: 32 products of (q - 1)^2 per accumulator, in every item"""
    pset = H.small_ckks(10, nq=2)
    assert pset["Q"][0].bit_length() == 60 and pset["Q"][1].bit_length() == 54
    w, Lc = T.World(pset), 2
    host = np.stack([np.stack([np.full(w.N, q - 1, dtype=np.uint64) for q in w.Q]) for _ in range(3)])
    top = [q - 1 for q in w.Q]
    check(w, [[host] * T.CAP_IN] * 2, [((top, top), [(top, top)] * T.CAP_IN)] * T.CAP_OUT, Lc, nb, ["p0", "p1"])


def test_refusals_on_a_live_context(worlds):
    from mkhe_kklss_amd import mkbfv
    w, Lc, ids = worlds[10], 2, ["p0", "p1"]
    rng = np.random.default_rng(1606)
    hosts, table = draw(rng, w, 2, 2, 2, 3, Lc, Lc)
    items, consts = [[w.ct(x, ids) for x in hs] for hs in hosts], w.consts(table, Lc)
    outs = [[w.new(ids, Lc), w.new(ids, Lc)] for _ in range(2)]
    sentinel = np.stack([H.uniform_poly(rng, w.Q[:Lc], w.N) for _ in range(3)])
    for o in outs[0] + outs[1]:
        o.upload(sentinel)
    ctx = w.params.ctx
    hin, hout = w.handle_array([c.h for it in items for c in it]), w.handle_array([c.h for o in outs for c in o])

    def refused(rc, text):
        assert rc != 0, "accepted"
        assert w.error() == NAME + text, w.error()

    call = w.lib.mkhe_ct_lincomb_batch
    # bad counts
    refused(call(ctx, 0, 2, hin, 2, consts.devptr(), 0, hout), "nbatch must be at least 1")
    refused(call(ctx, -3, 2, hin, 2, consts.devptr(), 0, hout), "nbatch must be at least 1")
    refused(call(ctx, 2, 0, hin, 2, consts.devptr(), 0, hout), "nin must be 1 .. 16")
    refused(call(ctx, 2, 17, hin, 2, consts.devptr(), 0, hout), "nin must be 1 .. 16")
    refused(call(ctx, 2, 2, hin, 0, consts.devptr(), 0, hout), "nout must be 1 .. 16")
    refused(call(ctx, 2, 2, hin, 17, consts.devptr(), 0, hout), "nout must be 1 .. 16")
    refused(call(ctx, 2, 2, hin, 2, consts.devptr(), 2, hout), "nb_rescale must be 0 or 1")
    refused(call(ctx, 2, 2, None, 2, consts.devptr(), 0, hout), "null argument")
    refused(call(ctx, 2, 2, hin, 2, None, 0, hout), "null argument")
    refused(call(ctx, 2, 2, hin, 2, consts.devptr(), 0, None), "null argument")
    # an output of item 1 that is an input of item 0; an output that is an input of its own item
    refused(batch(w, [[items[0][0], outs[1][1]], items[1]], consts, 0, outs), "an output must not alias an input")
    refused(batch(w, [items[0], [outs[1][0], items[1][1]]], consts, 0, outs), "an output must not alias an input")
    # a repeated output, within an item and across the items
    refused(batch(w, items, consts, 0, [outs[0], [outs[1][0], outs[1][0]]]), "the outputs must be distinct")
    refused(batch(w, items, consts, 0, [outs[0], [outs[1][0], outs[0][1]]]), "the outputs must be distinct")
    # mismatched ids, of an input and of an output
    refused(batch(w, [items[0], [items[1][0], w.ct(hosts[1][1], ["p0", "p2"])]], consts, 0, outs), "every input and output must carry the same ids")
    refused(batch(w, items, consts, 0, [outs[0], [outs[1][0], w.new(["p0"], Lc)]]), "every input and output must carry the same ids")
    # unequal output limbs; an input below Lc, directly and through the rescale
    refused(batch(w, items, consts, 0, [outs[0], [outs[1][0], w.new(ids, Lc - 1)]]), "the outputs must have the same number of limbs")
    deep = [[w.new(ids, Lc + 1), w.new(ids, Lc + 1)] for _ in range(2)]
    refused(batch(w, items, consts, 0, deep), "an input has fewer limbs than the sums (limbs(out) + nb_rescale)")
    refused(batch(w, items, consts, 1, outs), "an input has fewer limbs than the sums (limbs(out) + nb_rescale)")
    # input 1 has Lc limbs in item 0 and Lc + 1 in item 1
    longer = w.ct(np.stack([H.uniform_poly(rng, w.Q[: Lc + 1], w.N) for _ in range(3)]), ids)
    refused(batch(w, [items[0], [items[1][0], longer]], consts, 0, outs), "input k must have the same number of limbs in every item")
    # a BFV context: the call of that scheme is mkhe_bfv_ct_lincomb
    pset = HB.small_bfv(10, 3)
    bfv = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], pset["T"])
    bins, bouts = [mkbfv.NewCiphertext(bfv, ids) for _ in range(2)], [mkbfv.NewCiphertext(bfv, ids) for _ in range(2)]
    block = w.mk.DeviceLimbs(bfv, 1, 1)
    assert call(bfv.ctx, 1, 2, w.handle_array([c.h for c in bins]), 2, block.devptr(), 0, w.handle_array([c.h for c in bouts])) != 0
    assert w.error() == "mkhe_ct_lincomb_batch: needs a CKKS or mkrlwe context (mkhe_bfv_ct_lincomb is the BFV call)"
    # nothing was launched: the outputs still hold what was uploaded; and the context still works
    for o in outs[0] + outs[1]:
        assert (o.download() == sentinel).all()
    assert batch(w, items, consts, 0, outs) == 0, w.error()
    for b in range(2):
        for o, ref in zip(outs[b], T.model(w.Q, hosts[b], table, Lc, 0)):
            assert (o.download() == ref).all()


def test_inside_a_captured_graph():
    """mkhe_capture_begin / mkhe_ct_lincomb_batch / mkhe_capture_end / mkhe_graph_launch against the direct call, in a fresh interpreter (a process that
    has imported torch is bound to a HIP runtime in which mkhe_capture_begin refuses to capture, tests/test_gpu_cnn.py)"""
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, os.path.join(here, "lincomb_batch_graph_check.py")], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and "graph replay ok" in out.stdout
