"""Run by tests/test_gpu_ptxt_dot.py in a fresh interpreter (no torch: the ROCm >= 7.2 runtime, which can capture): mkhe_ct_ptxt_dot recorded into a HIP
graph after one warm-up call of the shape (which leaves the temporaries in the context's pool); the replay gives the eager result bit for bit, also
after the input handles have received new contents.  The masks are part of the recording: they are kernel arguments."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import test_gpu_ptxt_dot as T  # noqa: E402
import harness as H  # noqa: E402


def main():
    w, L, ids, nin, masks = T.World(H.small_ckks(11, nq=4)), 3, ["p0", "p1"], 5, [0b10011, 0b01100, 0b11111]
    rng = np.random.default_rng(808)
    draw = lambda: [H.uniform_ct(rng, w, 2, L) for _ in range(nin)]
    hosts = draw()
    pt_host = np.stack([H.uniform_poly(rng, w.Q[:L], w.N) for _ in range(sum(T.popcount(m) for m in masks))])
    ins, pt, ptntt = [w.ct(x, ids) for x in hosts], w.limbs(pt_host), w.limbs(pt_host)
    assert w.prepare(ptntt) == 0, w.error()
    eager, outs = [w.new(ids, L) for _ in masks], [w.new(ids, L) for _ in masks]
    assert w.dot(ins, masks, ptntt, L, eager) == 0, w.error()                     # warm-up, and the reference of the first replay
    ref = [o.download() for o in eager]
    for a, b in zip(ref, T.chain(w, ins, masks, pt, L, ids)):
        assert (a == b).all()
    with w.params.Capture() as graph:
        assert w.dot(ins, masks, ptntt, L, outs) == 0, w.error()
    graph.launch()
    for o, a in zip(outs, ref):
        assert (o.download() == a).all()
    for c, x in zip(ins, draw()):
        c.upload(x)
    graph.launch()
    got = [o.download() for o in outs]
    assert w.dot(ins, masks, ptntt, L, eager) == 0, w.error()
    for a, o in zip(got, eager):
        assert (a == o.download()).all()
    assert any((a != b).any() for a, b in zip(got, ref))                          # (the second replay did compute something new)
    print("graph replay ok")


if __name__ == "__main__":
    main()
