"""Plain transforms (mkhe_ntt) on both sides of every launch-size boundary of the NTT routes (csrc/ntt_route.h), N = 2^13 .. 2^16.

One modulus per launch, so that the limb count of the launch is the polynomial count: forward and inverse, out of place and in place,
bit for bit against the oracle's ring transform; and the last polynomial of every batch transformed alone (count = 1: the smallest
route of its ring) gives the bits it gave inside the batch.  The counts are the thresholds of tests/test_ntt_route_host.py that a plain
transform reaches; both modulus classes of each ring run (modulus 0 and modulus 1 of the set)."""
import numpy as np
import pytest

import harness as H

pytestmark = pytest.mark.gpu

PSETS = {13: H.small_ckks(13, 2), 14: H.small_ckks(14, 2), 15: H.small_ckks(15, 2), 16: H.small_alpha2(16, 2)}
COUNTS = {13: [128, 129], 14: [63, 64, 127, 128, 129], 15: [127, 128, 511, 512, 513], 16: [63, 64]}
CASES = [(logN, c) for logN in sorted(COUNTS) for c in COUNTS[logN]]


class _Ring:
    """One ring on both sides; the inputs and the oracle's transforms of max(COUNTS) polynomials per modulus, computed once."""

    def __init__(self, logN):
        from oracle import oracle as O
        from mkhe_kklss_amd import mkckks
        p = PSETS[logN]
        self.N = 1 << logN
        self.params = mkckks.Parameters(p["logN"], p["Q"], p["P"], p["scale"], device=0)
        ring = O.KeySwitcher(p["logN"], p["Q"], p["P"], 2).ringQ
        rng = np.random.default_rng(0x9077E + logN)
        cnt = max(COUNTS[logN])
        self.a, self.fwd, self.inv = [], [], []
        for m in (0, 1):
            a = rng.integers(0, p["Q"][m], (cnt, self.N), dtype=np.uint64)
            self.a.append(a)
            self.fwd.append(np.stack([ring.ntt(m, x) for x in a]))
            self.inv.append(np.stack([ring.intt(m, x) for x in a]))
        for v in self.a + self.fwd + self.inv:
            v.setflags(write=False)


_rings = {}


@pytest.fixture
def ring(request):
    logN = request.param
    if logN not in _rings:
        _rings.clear()              # one ring's buffers at a time
        _rings[logN] = _Ring(logN)
    return _rings[logN]


@pytest.mark.parametrize("ring,count", CASES, indirect=["ring"], ids=["N%d-%d" % c for c in CASES])
def test_plain_ntt_on_both_sides_of_the_route_thresholds(ring, count):
    from mkhe_kklss_amd import mkrlwe
    params = ring.params
    for m in (0, 1):
        a = ring.a[m][:count, None, :]
        for inverse, ref in ((False, ring.fwd[m][:count]), (True, ring.inv[m][:count])):
            src = mkrlwe.DeviceLimbs(params, count, 1).upload(a)
            dst = mkrlwe.DeviceLimbs(params, count, 1)
            mkrlwe.ntt(params, src, dst, mod_base=m, inverse=inverse)
            got = dst.download()[:, 0]
            assert (got == ref).all(), (m, inverse, "out of place")
            mkrlwe.ntt(params, src, src, mod_base=m, inverse=inverse)
            assert (src.download()[:, 0] == ref).all(), (m, inverse, "in place")
            one = mkrlwe.DeviceLimbs(params, 1, 1).upload(a[count - 1:])
            out = mkrlwe.DeviceLimbs(params, 1, 1)
            mkrlwe.ntt(params, one, out, mod_base=m, inverse=inverse)
            assert (out.download()[0, 0] == got[count - 1]).all(), (m, inverse, "alone")
