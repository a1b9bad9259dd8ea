"""mkhe_ptxt_prepare and mkhe_ct_ptxt_dot (-m gpu), bit for bit: the prepared plaintext against mkhe_ntt followed by x * 2^64 mod q in Python integers;
the dot product against the chain it replaces -- mkhe_ct_mul_ptxt per present diagonal on the coefficient-domain plaintexts, mkhe_ct_sum per giant --
and, for single coefficients and the worst case of the accumulator, against the negacyclic product in Python integers.  Ciphertexts and plaintexts are
independent uniform residues: no encoding and no key is involved at this level."""
import os
import subprocess
import sys

import numpy as np
import pytest

import harness as H

pytestmark = pytest.mark.gpu

CAP_IN, CAP_GIANT = 16, 64                      # CTDOT_MAX_IN, CTDOT_MAX_GIANT of csrc/poly_kernels.h
R = 1 << 64


class World:
    def __init__(self, pset, params=None):
        import ctypes as C
        from mkhe_kklss_amd import mkrlwe
        from mkhe_kklss_amd._abi import handle_array, lib
        self.C, self.mk, self.lib, self.handle_array = C, mkrlwe, lib(), handle_array
        self.Q, self.N = pset["Q"], 1 << pset["logN"]            # (H.uniform_ct reads .Q and .N)
        self.params = mkrlwe.Parameters(pset["logN"], pset["Q"], pset["P"], 2) if params is None else params

    def ct(self, host, ids):
        return self.mk.NewCiphertext(self.params, ids, host.shape[1] - 1).upload(host)

    def new(self, ids, limbs):
        return self.mk.NewCiphertext(self.params, ids, limbs - 1)

    def limbs(self, host):
        return self.mk.DeviceLimbs(self.params, host.shape[0], host.shape[1]).upload(host)

    def prepare(self, pt, dst=None):
        dst = pt if dst is None else dst
        return self.lib.mkhe_ptxt_prepare(self.params.ctx, pt.limbs, pt.count, pt.devptr(), dst.devptr())

    def dot(self, ins, masks, ptntt, pt_limbs, outs, nin=None, ngiant=None):
        arr = (self.C.c_uint32 * max(1, len(masks)))(*masks)
        return self.lib.mkhe_ct_ptxt_dot(self.params.ctx, len(ins) if nin is None else nin, self.handle_array([c.h for c in ins]),
                                         len(outs) if ngiant is None else ngiant, arr, ptntt.devptr(), pt_limbs, self.handle_array([c.h for c in outs]))

    def error(self):
        return self.lib.mkhe_last_error().decode()


@pytest.fixture(scope="module")
def worlds():
    return {logN: World(H.small_ckks(logN, nq=4)) for logN in (10, 11)}


def popcount(m):
    return bin(m).count("1")


def chain(w, ins, masks, pt, L, ids):
    """the reference: mkhe_ct_mul_ptxt of every (input dropped to L limbs, coefficient-domain plaintext) pair of a set mask bit, mkhe_ct_sum per giant.
    pt: DeviceLimbs [nnz][pt_limbs][N].  -> list of uint64 [polys][L][N]"""
    from mkhe_kklss_amd import _abi
    ctx, words = w.params.ctx, pt.limbs * w.N
    one = np.array([R % q for q in w.Q[:L]], dtype=np.uint64)
    low = []
    for c in ins:                                                # DropLevel: the product entry point wants input and output at one level
        low.append(w.new(ids, L))
        assert w.lib.mkhe_ct_mul_const(ctx, c.h, one.ctypes.data_as(_abi.u64p), one.ctypes.data_as(_abi.u64p), low[-1].h) == 0, w.error()
    res, index = [], 0
    for m in masks:
        prods = []
        for b in range(len(ins)):
            if m >> b & 1:
                src = pt
                if pt.limbs != L:                                # mkhe_ct_mul_ptxt reads a plaintext of exactly L limbs: the first L of this one
                    src = w.limbs(pt.download()[index: index + 1, :L])
                    ptr = src.devptr()
                else:
                    ptr = w.C.c_void_p(pt.devptr().value + 8 * words * index)
                prods.append((w.new(ids, L), src))
                assert w.lib.mkhe_ct_mul_ptxt(ctx, low[b].h, ptr, prods[-1][0].h) == 0, w.error()
                index += 1
        out = w.new(ids, L)
        assert w.lib.mkhe_ct_sum(ctx, len(prods), w.handle_array([p.h for p, _ in prods]), out.h) == 0, w.error()
        res.append(out.download())
    return res


def run_case(w, seed, parties, nin, masks, in_limbs, L, pt_limbs):
    rng = np.random.default_rng(seed)
    ids = ["p%d" % i for i in range(parties)]
    hosts = [H.uniform_ct(rng, w, parties, in_limbs) for _ in range(nin)]
    nnz = sum(popcount(m) for m in masks)
    pt_host = np.stack([H.uniform_poly(rng, w.Q[:pt_limbs], w.N) for _ in range(nnz)])
    ins, pt, ptntt = [w.ct(x, ids) for x in hosts], w.limbs(pt_host), w.limbs(pt_host)
    assert w.prepare(ptntt) == 0, w.error()
    outs = [w.new(ids, L) for _ in masks]
    assert w.dot(ins, masks, ptntt, pt_limbs, outs) == 0, w.error()
    got, ref = [o.download() for o in outs], chain(w, ins, masks, pt, L, ids)
    for g, (a, b) in enumerate(zip(got, ref)):
        assert a.shape == b.shape == (1 + parties, L, w.N) and (a == b).all(), "giant %d" % g
    for c, x in zip(ins, hosts):
        assert (c.download() == x).all()                        # the inputs are left as they were
    return hosts, pt_host, got


@pytest.mark.parametrize("inplace", [True, False])
def test_prepare_is_ntt_then_mform(worlds, inplace):
    w, count, limbs = worlds[10], 3, 3
    rng = np.random.default_rng(31 + inplace)
    host = np.stack([H.uniform_poly(rng, w.Q[:limbs], w.N) for _ in range(count)])
    src, via = w.limbs(host), w.limbs(host)
    dst = src if inplace else w.limbs(np.zeros_like(host))
    assert w.prepare(src, dst) == 0, w.error()
    ntt = w.limbs(np.zeros_like(host))
    w.mk.ntt(w.params, via, ntt)
    want = np.stack([np.stack([(x[l].astype(object) * R % w.Q[l]).astype(np.uint64) for l in range(limbs)]) for x in ntt.download()])
    assert (dst.download() == want).all()
    if not inplace:
        assert (src.download() == host).all()


CASES = {
    "one-of-everything": dict(logN=10, parties=1, nin=1, masks=[1], in_limbs=2, L=2, pt_limbs=2),
    "full-width": dict(logN=10, parties=2, nin=16, masks=[0xFFFF, 0x8000, 0x5555], in_limbs=3, L=3, pt_limbs=3),
    "inputs-above-the-outputs": dict(logN=10, parties=2, nin=5, masks=[0b10110, 0b01001], in_limbs=4, L=2, pt_limbs=4),
    "four-parties": dict(logN=11, parties=4, nin=3, masks=[0b101, 0b111], in_limbs=4, L=4, pt_limbs=4),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_equals_the_chain_of_mul_ptxt_and_sum(worlds, name):
    c = dict(CASES[name])
    w = worlds[c.pop("logN")]
    hosts, pt_host, got = run_case(w, sorted(CASES).index(name) + 100, **c)
    if name != "full-width":
        return
    # eight coefficients of one output polynomial against the O(N) negacyclic sum in Python integers: giant 2 (mask 0x5555), polynomial 1, limb 2
    g, p, l, N = 2, 1, 2, w.N
    q, first = w.Q[l], popcount(0xFFFF) + popcount(0x8000)
    bits = [b for b in range(16) if 0x5555 >> b & 1]
    for j in (0, 1, 2, N // 2 - 1, N // 2, N - 3, N - 2, N - 1):
        acc = 0
        for i, b in enumerate(bits):
            x, y = hosts[b][p, l].astype(object), pt_host[first + i, l].astype(object)
            k = np.arange(N)
            acc += int((x[k[: j + 1]] * y[j - k[: j + 1]]).sum()) - int((x[k[j + 1:]] * y[N + j - k[j + 1:]]).sum())
        assert int(got[g][p, l, j]) == acc % q, j


def test_inputs_at_different_levels(worlds):
    """the forward transform is launched once per run of inputs with one limb count"""
    w, ids, L = worlds[10], ["p0", "p1"], 2
    rng = np.random.default_rng(909)
    limbs = [4, 4, 2, 3]
    hosts = [H.uniform_ct(rng, w, 2, k) for k in limbs]
    masks = [0b1111, 0b0100]
    pt_host = np.stack([H.uniform_poly(rng, w.Q[:L], w.N) for _ in range(5)])
    ins, pt, ptntt = [w.ct(x, ids) for x in hosts], w.limbs(pt_host), w.limbs(pt_host)
    assert w.prepare(ptntt) == 0, w.error()
    outs = [w.new(ids, L) for _ in masks]
    assert w.dot(ins, masks, ptntt, L, outs) == 0, w.error()
    for a, b in zip([o.download() for o in outs], chain(w, ins, masks, pt, L, ids)):
        assert (a == b).all()


def test_worst_case_accumulation():
    """nin = 16, first limb the 60-bit prime, against Python integers.
    (a) Every input word and every plaintext residue q_l - 1: both are the polynomial -(1 + X + .. + X^(N-1)), whose negacyclic square has the
        coefficients (j + 1) - (N - 1 - j) = 2 j + 2 - N; sixteen of them per output.
    (b) The accumulator at its largest: the prepared block written down directly, every word q_l - 1 (the Montgomery form of -2^-64), and inputs whose
        TRANSFORM is q_l - 1 in every word, the constant polynomial -1: sixteen products (q - 1)^2 in every sum, 16 (q - 1)^2 2^-64 = 16 * 2^-64 mod q in
        every word of the transform, i.e. the constant polynomial 16 * 2^-64 mod q."""
    pset = H.small_ckks(10, nq=2)
    assert pset["Q"][0].bit_length() == 60
    w, L, ids = World(pset), 2, ["p0", "p1"]
    top = np.stack([np.full(w.N, q - 1, dtype=np.uint64) for q in w.Q])
    host = np.stack([top] * 3)
    ins, ptntt, outs = [w.ct(host, ids) for _ in range(CAP_IN)], w.limbs(np.stack([top] * CAP_IN)), [w.new(ids, L)]
    assert w.prepare(ptntt) == 0, w.error()
    assert w.dot(ins, [0xFFFF], ptntt, L, outs) == 0, w.error()
    got = outs[0].download()
    for l, q in enumerate(w.Q):
        want = np.array([CAP_IN * (2 * j + 2 - w.N) % q for j in range(w.N)], dtype=np.uint64)
        assert (got[:, l, :] == want).all()
    const = np.zeros_like(host)
    for l, q in enumerate(w.Q):
        const[:, l, 0] = q - 1
    ins = [w.ct(const, ids) for _ in range(CAP_IN)]
    assert w.dot(ins, [0xFFFF], w.limbs(np.stack([top] * CAP_IN)), L, outs) == 0, w.error()
    got = outs[0].download()
    for l, q in enumerate(w.Q):
        assert (got[:, l, 0] == np.uint64(CAP_IN * pow(R, -1, q) % q)).all() and not got[:, l, 1:].any()


def test_errors(worlds):
    w, L, ids = worlds[10], 2, ["p0", "p1"]
    rng = np.random.default_rng(606)
    hosts = [H.uniform_ct(rng, w, 2, L) for _ in range(2)]
    pt_host = np.stack([H.uniform_poly(rng, w.Q[:L], w.N) for _ in range(3)])
    ins, pt, ptntt = [w.ct(x, ids) for x in hosts], w.limbs(pt_host), w.limbs(pt_host)
    assert w.prepare(ptntt) == 0, w.error()
    sentinel = H.uniform_ct(rng, w, 2, L)
    outs = [w.new(ids, L).upload(sentinel) for _ in range(2)]
    masks = [0b11, 0b10]

    def refused(rc, name="mkhe_ct_ptxt_dot"):
        assert rc != 0, "accepted"
        assert w.error().startswith(name), w.error()
        return w.error()

    refused(w.dot(ins, masks, ptntt, L, outs, nin=0))                                              # nin 0 and 17
    refused(w.dot([ins[0]] * (CAP_IN + 1), masks, ptntt, L, outs))
    refused(w.dot(ins, masks, ptntt, L, outs, ngiant=0))                                           # ngiant 0 and 65
    many = [w.new(ids, L) for _ in range(CAP_GIANT + 1)]
    refused(w.dot(ins, [1] * (CAP_GIANT + 1), ptntt, L, many))
    refused(w.dot(ins, [0b11, 0], ptntt, L, outs))                                                 # a zero mask
    refused(w.dot(ins, [0b11, 0b100], ptntt, L, outs))                                             # a mask bit >= nin
    refused(w.dot(ins, masks, ptntt, L - 1, outs))                                                 # pt_limbs < L
    refused(w.dot([ins[0], w.ct(hosts[1], ["p0", "p2"])], masks, ptntt, L, outs))                  # ids that differ: among the inputs,
    refused(w.dot(ins, masks, ptntt, L, [outs[0], w.new(["p0"], L)]))                              # among the outputs,
    refused(w.dot(ins, masks, ptntt, L, [w.new(["p0", "p2"], L), w.new(["p0", "p2"], L)]))         # between the two
    refused(w.dot(ins, masks, ptntt, L, [outs[0], w.new(ids, L + 1)]))                             # outputs of two levels
    refused(w.dot([w.ct(hosts[0][:, :1], ids), ins[1]], masks, ptntt, L, outs))                    # an input below the outputs
    refused(w.dot([ins[0], outs[1]], masks, ptntt, L, outs))                                       # an output aliasing an input
    refused(w.dot(ins, masks, ptntt, L, [outs[0], outs[0]]))                                       # two equal outputs
    ctx, harr, oarr = w.params.ctx, w.handle_array([c.h for c in ins]), w.handle_array([c.h for c in outs])
    marr = (w.C.c_uint32 * 2)(*masks)
    refused(w.lib.mkhe_ct_ptxt_dot(None, 2, harr, 2, marr, ptntt.devptr(), L, oarr))               # null pointers
    refused(w.lib.mkhe_ct_ptxt_dot(ctx, 2, None, 2, marr, ptntt.devptr(), L, oarr))
    refused(w.lib.mkhe_ct_ptxt_dot(ctx, 2, harr, 2, None, ptntt.devptr(), L, oarr))
    refused(w.lib.mkhe_ct_ptxt_dot(ctx, 2, harr, 2, marr, None, L, oarr))
    refused(w.lib.mkhe_ct_ptxt_dot(ctx, 2, harr, 2, marr, ptntt.devptr(), L, None))
    refused(w.lib.mkhe_ct_ptxt_dot(ctx, 2, w.handle_array([ins[0].h, None]), 2, marr, ptntt.devptr(), L, oarr))
    refused(w.lib.mkhe_ct_ptxt_dot(ctx, 2, harr, 2, marr, ptntt.devptr(), L, w.handle_array([outs[0].h, None])))
    for bad in (dict(limbs=0), dict(limbs=len(w.Q) + 1), dict(count=0)):                           # and the prepare call
        kw = dict(limbs=L, count=3)
        kw.update(bad)
        refused(w.lib.mkhe_ptxt_prepare(ctx, kw["limbs"], kw["count"], pt.devptr(), ptntt.devptr()), "mkhe_ptxt_prepare")
    refused(w.lib.mkhe_ptxt_prepare(None, L, 3, pt.devptr(), ptntt.devptr()), "mkhe_ptxt_prepare")
    refused(w.lib.mkhe_ptxt_prepare(ctx, L, 3, None, ptntt.devptr()), "mkhe_ptxt_prepare")
    refused(w.lib.mkhe_ptxt_prepare(ctx, L, 3, pt.devptr(), None), "mkhe_ptxt_prepare")
    # nothing was launched: the outputs still hold what was uploaded; and the context still works
    for o in outs:
        assert (o.download() == sentinel).all()
    assert w.dot(ins, masks, ptntt, L, outs) == 0, w.error()
    for a, b in zip([o.download() for o in outs], chain(w, ins, masks, pt, L, ids)):
        assert (a == b).all()


def test_a_bfv_context_is_refused():
    import harness_bfv as HB
    from mkhe_kklss_amd import mkbfv
    pset = HB.small_bfv(10, 2)
    w = World(pset, mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], pset["T"]))
    rng = np.random.default_rng(5)
    L, ids = len(w.Q), ["p0"]
    x, sentinel = H.uniform_ct(rng, w, 1, L), H.uniform_ct(rng, w, 1, L)
    cin, out = w.ct(x, ids), w.new(ids, L).upload(sentinel)
    pt_host = np.stack([H.uniform_poly(rng, w.Q, w.N)])
    pt, dst = w.limbs(pt_host), w.limbs(np.zeros_like(pt_host))
    assert w.prepare(pt, dst) != 0 and w.error().startswith("mkhe_ptxt_prepare"), w.error()
    assert w.dot([cin], [1], pt, L, [out]) != 0 and w.error().startswith("mkhe_ct_ptxt_dot"), w.error()
    assert (out.download() == sentinel).all() and not dst.download().any() and (pt.download() == pt_host).all()


def test_inside_a_captured_graph():
    """mkhe_capture_begin / mkhe_ct_ptxt_dot / mkhe_capture_end / mkhe_graph_launch against the eager call, in a fresh interpreter: a process that has
    imported torch is bound to a HIP runtime in which mkhe_capture_begin refuses to capture (tests/test_gpu_cnn.py)"""
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, os.path.join(here, "ptxt_dot_graph_check.py")], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and "graph replay ok" in out.stdout


def test_more_limbs_than_limb_groups():
    """N = 2^15 with four polynomials is the smallest shape at which the launch makes fewer limb groups than limbs, so that one thread walks several
    limbs with its inputs reloaded: the loop that every smaller shape runs exactly once"""
    w = World(H.small_ckks(15, nq=6))
    run_case(w, 1500, parties=3, nin=2, masks=[0b11, 0b01], in_limbs=6, L=6, pt_limbs=6)
