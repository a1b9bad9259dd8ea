"""Run by tests/test_gpu_lincomb_multi.py in a fresh interpreter (no torch: the ROCm >= 7.2 runtime, which can capture): mkhe_ct_lincomb_multi with its
fused rescale recorded into a HIP graph through params.Capture() -- one kernel node, a single-branch graph; the replay gives the eager result bit
for bit, also after the input handles and the constant block have received new contents (the constants are read when the graph runs, not when it
is recorded)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import test_gpu_lincomb_multi as T  # noqa: E402
import harness as H  # noqa: E402


def main():
    w, Lc, ids, nin, nout = T.World(H.small_ckks(11, nq=4)), 4, ["p0", "p1"], 5, 6
    rng = np.random.default_rng(808)
    hosts, table = T.draw(rng, w.Q, w.N, nin, nout, 3, Lc, Lc)
    ins, consts = [w.ct(x, ids) for x in hosts], w.consts(table, Lc)
    eager, outs = [w.new(ids, Lc - 1) for _ in range(nout)], [w.new(ids, Lc - 1) for _ in range(nout)]
    assert w.multi(ins, consts, 1, eager) == 0, w.error()
    ref = [o.download() for o in eager]
    assert all((a == b).all() for a, b in zip(ref, T.model(w.Q, hosts, table, Lc, 1)))
    with w.params.Capture() as graph:
        assert w.multi(ins, consts, 1, outs) == 0, w.error()
    graph.launch()
    assert all((o.download() == r).all() for o, r in zip(outs, ref))
    hosts2, table2 = T.draw(rng, w.Q, w.N, nin, nout, 3, Lc, Lc)
    for c, x in zip(ins, hosts2):
        c.upload(x)
    consts.upload(w.consts(table2, Lc).download())
    graph.launch()
    assert all((o.download() == r).all() for o, r in zip(outs, T.model(w.Q, hosts2, table2, Lc, 1)))
    print("graph replay ok")


if __name__ == "__main__":
    main()
