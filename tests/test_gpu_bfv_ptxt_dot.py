"""mkhe_bfv_ct_ptxt_dot (-m gpu), bit for bit against the chain it replaces: mkhe_bfv_ct_mul_ptxt per set mask bit, mkhe_ct_sum per output.
Ciphertexts and prepared plaintexts are independent uniform residues: no encoding and no key is involved at this level.  small_bfv(10, 3) and
small_bfv(11, 3), T = 65537.  nin = 1, 4, 5, 8, 9, 16 are the boundaries of the kernel's three register layouts."""
import ctypes as C

import numpy as np
import pytest

import harness as H
import harness_bfv as HB

pytestmark = pytest.mark.gpu

NAMES = ["user0", "user1"]
NAME = "mkhe_bfv_ct_ptxt_dot"
SPARSE = 0b1010010010010101


class World:
    def __init__(self, logN):
        from mkhe_kklss_amd import mkbfv, mkrlwe
        from mkhe_kklss_amd._abi import handle_array, lib
        pset = HB.small_bfv(logN, 3)
        self.mkbfv, self.mk, self.lib, self.handle_array = mkbfv, mkrlwe, lib(), handle_array
        self.Q, self.N, self.nq = pset["Q"], 1 << logN, len(pset["Q"])
        self.params = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], pset["T"])

    def ct(self, host, ids):
        return self.mkbfv.NewCiphertext(self.params, ids).upload(host)

    def new(self, ids):
        return self.mkbfv.NewCiphertext(self.params, ids)

    def limbs(self, host):
        return self.mk.DeviceLimbs(self.params, host.shape[0], host.shape[1]).upload(host)

    def dot(self, nbatch, nin, ins, masks, pt, outs, ctx=None):
        arr = None if masks is None else (C.c_uint32 * max(1, len(masks)))(*masks)
        h = lambda v: None if v is None else (C.c_void_p * max(1, len(v)))(*[getattr(c, "h", c) for c in v])
        ptr = pt.devptr() if hasattr(pt, "devptr") else pt
        return self.lib.mkhe_bfv_ct_ptxt_dot(self.params.ctx if ctx is None else ctx, nbatch, nin, h(ins), len(masks) if masks is not None else 1,
                                             arr, ptr, h(outs))

    def error(self):
        return self.lib.mkhe_last_error().decode()


@pytest.fixture(scope="module")
def worlds():
    return {logN: World(logN) for logN in (10, 11)}


def popcount(m):
    return bin(m).count("1")


def chain(w, ins, nbatch, nin, masks, pt, ids):
    """the reference: mkhe_bfv_ct_mul_ptxt(in[b][i], P(g, i)) for every set mask bit, mkhe_ct_sum per (b, g) -> uint64 [polys][nQ][N] in (b, g) order"""
    ctx, words = w.params.ctx, w.nq * w.N
    res = []
    for b in range(nbatch):
        index = 0
        for m in masks:
            prods = []
            for i in range(nin):
                if m >> i & 1:
                    prods.append(w.new(ids))
                    one_in, one_out = (C.c_void_p * 1)(ins[b * nin + i].h), (C.c_void_p * 1)(prods[-1].h)
                    ptr = C.c_void_p(pt.devptr().value + 8 * words * index)
                    assert w.lib.mkhe_bfv_ct_mul_ptxt(ctx, 1, one_in, ptr, 0, one_out) == 0, w.error()
                    index += 1
            out = w.new(ids)
            assert w.lib.mkhe_ct_sum(ctx, len(prods), w.handle_array([p.h for p in prods]), out.h) == 0, w.error()
            res.append(out.download())
    return res


def run_case(w, seed, parties, nbatch, nin, masks):
    rng = np.random.default_rng(seed)
    ids = NAMES[:parties]
    hosts = [H.uniform_ct(rng, w, parties, w.nq) for _ in range(nbatch * nin)]
    nnz = sum(popcount(m) for m in masks)
    pt = w.limbs(np.stack([H.uniform_poly(rng, w.Q, w.N) for _ in range(nnz)]))
    ins = [w.ct(x, ids) for x in hosts]
    outs = [w.new(ids) for _ in range(nbatch * len(masks))]
    assert w.dot(nbatch, nin, ins, masks, pt, outs) == 0, w.error()
    got, ref = [o.download() for o in outs], chain(w, ins, nbatch, nin, masks, pt, ids)
    assert len(got) == len(ref) == nbatch * len(masks)
    for k, (a, b) in enumerate(zip(got, ref)):
        assert a.shape == b.shape == (1 + parties, w.nq, w.N) and (a == b).all(), "item %d, giant %d" % divmod(k, len(masks))
    for c, x in zip(ins, hosts):
        assert (c.download() == x).all()                        # the inputs are left as they were
    return got


@pytest.mark.parametrize("parties", [1, 2])
@pytest.mark.parametrize("nbatch", [1, 3])
@pytest.mark.parametrize("nin", [1, 4, 5, 8, 9, 16])
def test_three_giants_full_single_bit_and_sparse_masks(worlds, nin, nbatch, parties):
    full = (1 << nin) - 1
    run_case(worlds[10], 1000 + 100 * nin + 10 * nbatch + parties, parties, nbatch, nin, [full, 1 << (nin - 1), (SPARSE & full) or 1])


@pytest.mark.parametrize("kind", ["full", "bit0", "top"])
@pytest.mark.parametrize("nin", [1, 4, 5, 8, 9, 16])
def test_one_giant(worlds, nin, kind):
    mask = {"full": (1 << nin) - 1, "bit0": 1, "top": 1 << (nin - 1)}[kind]
    nbatch, parties = (3, 1) if nin in (4, 8, 16) else (1, 2)
    run_case(worlds[11], 2000 + 10 * nin + len(kind), parties, nbatch, nin, [mask])


@pytest.mark.parametrize("nin,nbatch,parties", [(5, 1, 2), (5, 3, 1), (16, 1, 1), (16, 3, 2)])
def test_sixty_four_giants(worlds, nin, nbatch, parties):
    rng = np.random.default_rng(64 + nin + nbatch)
    masks = [int(m) or 1 for m in rng.integers(0, 1 << nin, 64)]
    masks[0], masks[1], masks[63] = (1 << nin) - 1, 1, 1 << (nin - 1)
    run_case(worlds[10], 3000 + nin + nbatch, parties, nbatch, nin, masks)


def test_one_item_of_a_batch_equals_the_call_alone(worlds):
    """the batch dimension only adds rows to the grid: item 1 of three, computed alone, has the same bits"""
    w, ids, nin, masks = worlds[10], NAMES, 5, [0b10110, 0b01001]
    rng = np.random.default_rng(77)
    hosts = [H.uniform_ct(rng, w, 2, w.nq) for _ in range(3 * nin)]
    pt = w.limbs(np.stack([H.uniform_poly(rng, w.Q, w.N) for _ in range(5)]))
    ins = [w.ct(x, ids) for x in hosts]
    outs, alone = [w.new(ids) for _ in range(6)], [w.new(ids) for _ in range(2)]
    assert w.dot(3, nin, ins, masks, pt, outs) == 0, w.error()
    assert w.dot(1, nin, ins[nin: 2 * nin], masks, pt, alone) == 0, w.error()
    for g in range(2):
        assert (outs[2 + g].download() == alone[g].download()).all()


def test_sixty_five_inputs_cross_the_transform_launch(worlds):
    """nbatch * nin = 5 * 13 = 65 input ciphertexts: the forward transform takes 64 per launch.  Every item against its call alone"""
    w, ids, nbatch, nin = worlds[10], NAMES[:1], 5, 13
    masks = [(1 << nin) - 1]
    rng = np.random.default_rng(65)
    ins = [w.ct(H.uniform_ct(rng, w, 1, w.nq), ids) for _ in range(nbatch * nin)]
    pt = w.limbs(np.stack([H.uniform_poly(rng, w.Q, w.N) for _ in range(nin)]))
    outs, alone = [w.new(ids) for _ in range(nbatch)], w.new(ids)
    assert w.dot(nbatch, nin, ins, masks, pt, outs) == 0, w.error()
    for b in range(nbatch):
        assert w.dot(1, nin, ins[b * nin: (b + 1) * nin], masks, pt, [alone]) == 0, w.error()
        assert (outs[b].download() == alone.download()).all(), b


def test_refusals(worlds):
    from mkhe_kklss_amd import mkckks, mkrlwe
    from mkhe_kklss_amd._abi import MkheError
    w, ids = worlds[10], NAMES
    rng = np.random.default_rng(606)
    nbatch, nin, masks = 2, 2, [0b11, 0b10]
    hosts = [H.uniform_ct(rng, w, 2, w.nq) for _ in range(nbatch * nin)]
    pt = w.limbs(np.stack([H.uniform_poly(rng, w.Q, w.N) for _ in range(3)]))
    ins = [w.ct(x, ids) for x in hosts]
    sentinel = H.uniform_ct(rng, w, 2, w.nq)
    outs = [w.new(ids).upload(sentinel) for _ in range(nbatch * len(masks))]
    want = None

    def refused(rc, text):
        assert rc != 0
        assert w.error().startswith(NAME + ": ") and text in w.error(), w.error()
        for o in outs:
            assert (o.download() == sentinel).all()              # nothing was enqueued
        for c, x in zip(ins, hosts):
            assert (c.download() == x).all()

    def works():
        fresh = [w.new(ids) for _ in outs]
        assert w.dot(nbatch, nin, ins, masks, pt, fresh) == 0, w.error()
        return [f.download() for f in fresh]

    want = works()
    for bad, text in (((0, nin), "nbatch"), ((17, nin), "nbatch"), ((nbatch, 0), "nin"), ((nbatch, 17), "nin")):
        refused(w.dot(bad[0], bad[1], ins, masks, pt, outs), text)
    refused(w.lib.mkhe_bfv_ct_ptxt_dot(w.params.ctx, nbatch, nin, w.handle_array([c.h for c in ins]), 0, (C.c_uint32 * 1)(1), pt.devptr(),
                                       w.handle_array([o.h for o in outs])), "ngiant")
    refused(w.lib.mkhe_bfv_ct_ptxt_dot(w.params.ctx, nbatch, nin, w.handle_array([c.h for c in ins]), 65, (C.c_uint32 * 65)(*[1] * 65), pt.devptr(),
                                       w.handle_array([o.h for o in outs])), "ngiant")
    refused(w.dot(nbatch, nin, ins, [0b11, 0], pt, outs), "a mask is zero")
    refused(w.dot(nbatch, nin, ins, [0b11, 0b100], pt, outs), "at or above nin")
    refused(w.dot(nbatch, nin, ins, masks, None, outs), "null")
    refused(w.dot(nbatch, nin, None, masks, pt, outs), "null")
    refused(w.dot(nbatch, nin, ins, None, pt, outs), "null")
    refused(w.dot(nbatch, nin, ins, masks, pt, None), "null")
    refused(w.dot(nbatch, nin, ins[:3] + [None], masks, pt, outs), "null")
    refused(w.dot(nbatch, nin, ins, masks, pt, outs[:3] + [None]), "null")
    refused(w.dot(nbatch, nin, ins, masks, C.c_void_p(pt.devptr().value + 8), outs), "aligned")
    assert [x.tolist() for x in works()] == [x.tolist() for x in want]
    other = w.ct(H.uniform_ct(rng, w, 1, w.nq), NAMES[1:])
    low = mkrlwe.Ciphertext(w.params, ids, w.params.MaxLevel() - 1)
    refused(w.dot(nbatch, nin, ins[:3] + [other], masks, pt, outs), "share their ids")
    refused(w.dot(nbatch, nin, ins, masks, pt, outs[:3] + [other]), "ids of the inputs")
    refused(w.dot(nbatch, nin, ins[:3] + [low], masks, pt, outs), "maximum level")
    refused(w.dot(nbatch, nin, ins, masks, pt, outs[:3] + [low]), "maximum level")
    refused(w.dot(nbatch, nin, ins, masks, pt, [outs[0], outs[0], outs[2], outs[3]]), "distinct")
    assert w.dot(nbatch, nin, ins, masks, pt, [ins[1], outs[1], outs[2], outs[3]]) != 0           # (an input as an output: the inputs stay)
    assert w.error().startswith(NAME + ": ") and "alias" in w.error()
    for c, x in zip(ins, hosts):
        assert (c.download() == x).all()
    assert w.dot(nbatch, nin, ins, masks, pt, outs, ctx=C.c_void_p(None)) != 0 and w.error() == NAME + ": null context"
    assert [x.tolist() for x in works()] == [x.tolist() for x in want]
    # a CKKS context is refused, and the CKKS calls keep refusing a BFV context
    ck = H.small_ckks(10, 3)
    cparams = mkckks.Parameters(ck["logN"], ck["Q"], ck["P"], ck["scale"])
    cin, cout = mkrlwe.Ciphertext(cparams, ["user0"], 2), mkrlwe.Ciphertext(cparams, ["user0"], 2)
    cpt = mkrlwe.DeviceLimbs(cparams, 1, 3)
    assert w.dot(1, 1, [cin], [1], cpt, [cout], ctx=cparams.ctx) != 0
    assert w.error().startswith(NAME + ": ") and "BFV context" in w.error()
    del cin, cout, cpt
    cparams.close()
    arr = (C.c_uint32 * 2)(*masks)
    assert w.lib.mkhe_ct_ptxt_dot(w.params.ctx, nin, w.handle_array([c.h for c in ins[:2]]), 2, arr, pt.devptr(), w.nq,
                                  w.handle_array([o.h for o in outs[:2]])) != 0
    assert w.error() == "mkhe_ct_ptxt_dot: needs a CKKS context"
    assert w.lib.mkhe_ptxt_prepare(w.params.ctx, w.nq, 1, pt.devptr(), pt.devptr()) != 0 and w.error() == "mkhe_ptxt_prepare: needs a CKKS context"
    # inside a capture (where the runtime of this process can capture at all)
    try:
        with w.params.Capture():
            rc = w.dot(nbatch, nin, ins, masks, pt, outs)
            msg = w.error()
        assert rc != 0 and msg.startswith(NAME + ": ") and "capture" in msg
        print("capture: the call was refused inside a capture")
    except MkheError as e:
        print("capture: mkhe_capture_begin refused in this process (%s): the refusal inside a capture did not run" % e)
        import gc
        gc.enable()                 # (Graph.__enter__ switched the collector off before the refusal)
        assert "cannot end a multi-stream capture" in str(e)
    assert [x.tolist() for x in works()] == [x.tolist() for x in want]


def test_ckks_dot_still_equals_its_own_chain():
    """the kernel is shared with mkhe_ct_ptxt_dot (one item): nine inputs, two parties, inputs above the outputs' level"""
    import test_gpu_ptxt_dot as PD
    w = PD.World(H.small_ckks(10, nq=4))
    PD.run_case(w, 4242, parties=2, nin=9, masks=[0x1FF, 0x100, 0x0A5], in_limbs=4, L=3, pt_limbs=4)
    PD.run_case(w, 4243, parties=1, nin=16, masks=[0xFFFF, 0x8001], in_limbs=2, L=2, pt_limbs=2)
