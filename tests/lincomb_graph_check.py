"""Run by tests/test_gpu_lincomb.py in a fresh interpreter (no torch: the ROCm >= 7.2 runtime, which can capture): mkhe_ct_lincomb with its fused
rescale recorded into a HIP graph; the replay gives the eager result bit for bit, also after the input handles and the constant block have
received new contents (the constants are read when the graph runs, not when it is recorded)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import test_gpu_lincomb as T  # noqa: E402
import harness as H  # noqa: E402


def main():
    w, Lc, ids, n = T.World(H.small_ckks(11, nq=4)), 4, ["p0", "p1"], 5
    rng = np.random.default_rng(808)
    hosts, add, weights = T.draw(rng, w.Q, w.N, n, 3, Lc, Lc)
    ins, consts = [w.ct(x, ids) for x in hosts], w.consts(add, weights, Lc)
    eager, out = w.new(ids, Lc - 1), w.new(ids, Lc - 1)
    assert w.lincomb(ins, consts, 1, eager) == 0, w.error()
    ref = eager.download()
    assert (ref == T.model(w.Q, hosts, add, weights, Lc, 1)).all()
    with w.params.Capture() as graph:
        assert w.lincomb(ins, consts, 1, out) == 0, w.error()
    graph.launch()
    assert (out.download() == ref).all()
    hosts2, add2, weights2 = T.draw(rng, w.Q, w.N, n, 3, Lc, Lc)
    for c, x in zip(ins, hosts2):
        c.upload(x)
    consts.upload(w.consts(add2, weights2, Lc).download())
    graph.launch()
    assert (out.download() == T.model(w.Q, hosts2, add2, weights2, Lc, 1)).all()
    print("graph replay ok")


if __name__ == "__main__":
    main()
