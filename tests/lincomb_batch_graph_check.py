"""Run by tests/test_gpu_lincomb_batch.py in a fresh interpreter (no torch: the ROCm >= 7.2 runtime, which can capture), in the manner of
tests/lincomb_multi_graph_check.py: mkhe_ct_lincomb_batch with its fused rescale recorded into a HIP graph through params.Capture().  36 items at 5 x 6
are two launches (34 + 2), a chain of two kernel nodes on one stream.  The replay gives the direct call's result bit for bit, twice, each time after the
input handles and the constant block have received new contents: base addresses are recorded, contents are read when the graph runs."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import test_gpu_lincomb_batch as B  # noqa: E402
import test_gpu_lincomb_multi as T  # noqa: E402
import harness as H  # noqa: E402


def main():
    w, Lc, ids, nbatch, nin, nout = T.World(H.small_ckks(11, nq=4)), 4, ["p0", "p1"], 36, 5, 6
    rng = np.random.default_rng(1808)
    hosts, table = B.draw(rng, w, nbatch, nin, nout, 3, Lc, Lc)
    items, consts = [[w.ct(x, ids) for x in hs] for hs in hosts], w.consts(table, Lc)
    direct, outs = ([[w.new(ids, Lc - 1) for _ in range(nout)] for _ in range(nbatch)] for _ in range(2))

    def direct_call():
        assert B.batch(w, items, consts, 1, direct) == 0, w.error()
        return [[o.download() for o in row] for row in direct]

    def same(ref):
        return all((o.download() == r).all() for row, rrow in zip(outs, ref) for o, r in zip(row, rrow))

    ref = direct_call()
    for b in (0, nbatch - 1):                               # (an item of each launch against the model; the rest is tests/test_gpu_lincomb_batch.py)
        assert all((a == m).all() for a, m in zip(ref[b], T.model(w.Q, hosts[b], table, Lc, 1)))
    with w.params.Capture() as graph:
        assert B.batch(w, items, consts, 1, outs) == 0, w.error()
    graph.launch()
    assert same(ref)
    for _ in range(2):
        hosts, table = B.draw(rng, w, nbatch, nin, nout, 3, Lc, Lc)
        for it, hs in zip(items, hosts):
            for c, x in zip(it, hs):
                c.upload(x)
        consts.upload(w.consts(table, Lc).download())
        graph.launch()
        got = [[o.download() for o in row] for row in outs]
        ref = direct_call()
        assert all((a == r).all() for grow, rrow in zip(got, ref) for a, r in zip(grow, rrow))
        assert all((a == m).all() for a, m in zip(got[nbatch - 1], T.model(w.Q, hosts[nbatch - 1], table, Lc, 1)))
    print("graph replay ok")


if __name__ == "__main__":
    main()
