"""-m gpu: the reduction epilogues of the sharded paths -- mkhe_swk_fold, mkhe_ct_fold, mkhe_swk_fold_pieces (include/mkhe.h; fold_kernel and
fold_pieces_kernel of csrc/poly_kernels.hip) -- against the big-integer model of tests/fold_model.py, bit for bit, at the edges of their domain:
every limb range / level / stride / piece count the mesh exchange of mkhe_kklss_amd.dist can produce, extreme residues, words up to 2^63 - 1,
piece counts at which a plain uint64 sum wraps 2^64, and the argument checks of the entry.

Buffers of the fold_pieces cases: `dst` is a whole switching-key buffer (24 limbs) between two guard limbs, all of it a sentinel pattern of words
>= 2^63 (no residue); the call gets the address of limb first_limb, as dist.py passes it.  The pieces lie `stride` words apart in a buffer whose
every other word carries a second sentinel pattern.  After the call: active limbs of the range = model, every other word of dst = sentinel, the
pieces buffer unchanged.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import fold_model as FM

pytestmark = pytest.mark.gpu

N = 1 << 11
NQ, NP, MTOT, DIGITS, LIMBS = 4, 2, 6, 4, 24
TOP = NQ - 1
SENT_DST, SENT_SRC = 0xA5C3F00D5EED0000, 0xC3A5BADC0FFE0000


def beta(level):
    return level + 1                                   # alpha = 1: one digit per active Q modulus


def sentinel(nwords, base):
    return np.uint64(base) + np.arange(nwords, dtype=np.uint64)


def limb_moduli(name):
    return (FM.SETS[name]["Q"] + FM.SETS[name]["P"]) * DIGITS


def active_mask(level):
    return np.array([FM.active_limb(l, level, NQ, NP, beta(level)) is not None for l in range(LIMBS)])


@pytest.fixture(scope="module")
def ctx_of():
    """one engine context per parameter set, shared by the cases of this file"""
    import torch
    torch.cuda.init()                                  # torch opens the device before the engine does, as in every torch test of tests/test_dist_sharded.py
    from mkhe_kklss_amd import mkrlwe
    made = {}

    def get(name):
        if name not in made:
            pset = FM.SETS[name]
            made[name] = mkrlwe.Parameters(pset["logN"], pset["Q"], pset["P"], 2)
            assert made[name].SwkShape() == (DIGITS, MTOT, N)
        return made[name]
    yield get
    for p in made.values():
        p.close()


def model_full(name, pieces, level, mform):
    """the model over the whole key; inactive limbs come back as zeros and are masked by the caller"""
    pset = FM.SETS[name]
    return FM.fold_pieces(pieces, 0, LIMBS, level, mform, pset["Q"], pset["P"], beta, np.zeros((LIMBS, N), dtype=np.uint64))


@functools.lru_cache(maxsize=8)
def uniform_case(name, npieces, level):
    """summands for the whole key, shared by the cases that follow each other and never changed: uniform canonical residues on the limbs active at `level`, arbitrary 64-bit words
    (half of them >= 2^63) on the others; and the model for both mform values"""
    rng = np.random.default_rng([npieces, level, sorted(FM.SETS).index(name), 20])
    mods, act = limb_moduli(name), active_mask(level)
    pieces = rng.integers(0, 1 << 64, (npieces, LIMBS, N), dtype=np.uint64)
    for l in range(LIMBS):
        if act[l]:
            pieces[:, l, :] = rng.integers(0, mods[l], (npieces, N), dtype=np.uint64)
    pieces.setflags(write=False)
    return pieces, {mform: model_full(name, pieces, level, mform) for mform in (0, 1)}


def constant_case(name, columns, mform):
    """every coefficient of limb l carries the column columns(q_l) (one word per piece): the model is evaluated on one coefficient and repeated"""
    mods = limb_moduli(name)
    col = np.array([[int(w) for w in columns(q)] for q in mods], dtype=np.uint64).T[:, :, None]         # [npieces][24][1]
    pset = FM.SETS[name]
    want = FM.fold_pieces(col, 0, LIMBS, TOP, mform, pset["Q"], pset["P"], beta, np.zeros((LIMBS, 1), dtype=np.uint64))
    return np.ascontiguousarray(np.broadcast_to(col, (col.shape[0], LIMBS, N))), np.ascontiguousarray(np.broadcast_to(want, (LIMBS, N)))


def to_device(host_u64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(host_u64).view(np.int64)).cuda()


def to_host(t):
    return t.cpu().numpy().view(np.uint64)


class FoldPiecesCall:
    """lays the buffers out, calls mkhe_swk_fold_pieces once and keeps what came back"""

    def __init__(self, params, pieces_full, first, nlimbs, level, mform, stride):
        import torch
        from mkhe_kklss_amd._abi import lib
        npieces = pieces_full.shape[0]
        assert 0 <= first and 0 <= nlimbs and first + nlimbs <= LIMBS and stride >= nlimbs * N          # the call stays inside the buffers below
        self.first, self.nlimbs, self.level = first, nlimbs, level
        self.src_before = sentinel(npieces * stride + N, SENT_SRC)
        for p in range(npieces):
            self.src_before[p * stride: p * stride + nlimbs * N] = pieces_full[p, first:first + nlimbs].reshape(-1)
        self.dst_before = sentinel((LIMBS + 2) * N, SENT_DST)
        src, dst = to_device(self.src_before), to_device(self.dst_before)
        torch.cuda.synchronize()
        self.rc = lib().mkhe_swk_fold_pieces(params.ctx, C.c_void_p(src.data_ptr()), npieces, stride, first, nlimbs, level, mform,
                                             C.c_void_p(dst.data_ptr() + 8 * (1 + first) * N))
        params.sync()
        self.src_after, self.dst_after = to_host(src), to_host(dst).reshape(LIMBS + 2, N)

    def check(self, want_full):
        """want_full: the model over the whole key (rows of inactive limbs are ignored)"""
        from mkhe_kklss_amd._abi import lib
        assert self.rc == 0, lib().mkhe_last_error().decode()
        written = np.zeros(LIMBS + 2, dtype=bool)
        written[1 + self.first: 1 + self.first + self.nlimbs] = active_mask(self.level)[self.first:self.first + self.nlimbs]
        before = self.dst_before.reshape(LIMBS + 2, N)
        got, want = self.dst_after[1:-1], np.asarray(want_full)
        bad = [l for l in range(LIMBS) if written[1 + l] and not (got[l] == want[l]).all()]
        assert not bad, "active limbs differ from the model: %r (first word of limb %d: got %#x, want %#x)" % (
            bad, bad[0], int(got[bad[0]][0]), int(want[bad[0]][0]))
        touched = [l - 1 for l in range(LIMBS + 2) if not written[l] and not (self.dst_after[l] == before[l]).all()]
        assert not touched, "limbs that must keep the sentinel were written (-1 / %d: the guards): %r" % (LIMBS, touched)
        assert (self.src_after == self.src_before).all(), "the pieces buffer changed"


# ---------------------------------------------------------------- 2a: ranges and shapes
RANGES = [(0, 24), (5, 1), (4, 9), (23, 1), (7, 0)]     # whole key; one limb inside a digit; mid-digit start across two digit boundaries; last limb; empty


@pytest.mark.parametrize("level", [3, 1, 0])
@pytest.mark.parametrize("first,nlimbs", RANGES)
@pytest.mark.parametrize("npieces", [1, 2, 3, 8])
@pytest.mark.parametrize("mform", [0, 1])
@pytest.mark.parametrize("name", sorted(FM.SETS))
def test_fold_pieces_ranges(ctx_of, name, mform, npieces, first, nlimbs, level):
    """levels 1 and 0 leave moduli 2, 3 (resp. 1, 2, 3) and digits 2, 3 (resp. 1, 2, 3) inactive inside the ranges: their limbs -- whose summands are
    arbitrary words -- must keep the sentinel, as must everything outside the range"""
    pieces, want = uniform_case(name, npieces, level)
    for stride in (nlimbs * N, nlimbs * N + 3 * N):
        FoldPiecesCall(ctx_of(name), pieces, first, nlimbs, level, mform, stride).check(want[mform])


# ---------------------------------------------------------------- 2b: extreme residues, 8 pieces
EXTREMES = {
    "all_q_minus_1": lambda q: [q - 1] * 8,                         # 8q - 8: the largest sum of 8 residues
    "all_zero": lambda q: [0] * 8,
    "sum_is_q": lambda q: [q - 1, 1, 0, 0, 0, 0, 0, 0],             # folds to 0
    "sum_is_7q": lambda q: [q - 1] * 7 + [7],
    "sum_is_4q": lambda q: [q - 1, 1] * 4,
    "alternating": lambda q: [q - 1, 0] * 4,                        # 4q - 4
}


@pytest.mark.parametrize("pattern", sorted(EXTREMES))
@pytest.mark.parametrize("mform", [0, 1])
@pytest.mark.parametrize("name", sorted(FM.SETS))
def test_fold_pieces_extreme_residues(ctx_of, name, mform, pattern):
    pieces, want = constant_case(name, EXTREMES[pattern], mform)
    mods = limb_moduli(name)
    if pattern.startswith("sum_is") or pattern == "all_zero":
        assert not want.any()                                        # multiples of q fold to 0 in either form
    if pattern == "all_q_minus_1":
        assert [int(want[l][0]) for l in range(LIMBS)] == [(q - 8) * (pow(2, 64, q) if mform else 1) % q for q in mods]
    FoldPiecesCall(ctx_of(name), pieces, 0, LIMBS, TOP, mform, LIMBS * N).check(want)


# ---------------------------------------------------------------- 2c: mkhe_swk_fold / mkhe_ct_fold at the bound of their domain
def table_words(rng, q, n):
    """n words drawn from the table of the host test (all < 2^63), every entry of the table at least once"""
    tab = np.array(FM.bound_table(q), dtype=np.uint64)
    words = tab[rng.integers(0, len(tab), n)]
    words[:len(tab)] = tab
    return rng.permutation(words)


@pytest.mark.parametrize("level", [3, 1])
@pytest.mark.parametrize("mform", [0, 1])
@pytest.mark.parametrize("name", sorted(FM.SETS))
def test_swk_fold_at_the_bound(ctx_of, name, mform, level):
    from mkhe_kklss_amd import mkrlwe
    from mkhe_kklss_amd._abi import check, lib
    params, mods, act = ctx_of(name), limb_moduli(name), active_mask(level)
    rng = np.random.default_rng([mform, level, 31])
    host = rng.integers(0, 1 << 64, (LIMBS, N), dtype=np.uint64)            # inactive limbs: arbitrary words
    want = host.copy()
    for l in range(LIMBS):
        if act[l]:
            host[l] = table_words(rng, mods[l], N)
            want[l] = FM.fold_words(host[l], mods[l], mform)
    assert act.sum() == (24 if level == 3 else 8) and int(host[act].max()) == 2 ** 63 - 1
    swk = mkrlwe.SwitchingKey(params, host.reshape(DIGITS, MTOT, N))
    check(lib().mkhe_swk_fold(params.ctx, swk.h, level, mform))
    got = swk.download().reshape(LIMBS, N)
    assert (got[act] == want[act]).all()
    assert (got[~act] == host[~act]).all()                                  # inactive digits and moduli are not touched


@pytest.mark.parametrize("limbs", [4, 2])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("name", sorted(FM.SETS))
def test_ct_fold_at_the_bound(ctx_of, name, k, limbs):
    from mkhe_kklss_amd import mkrlwe
    from mkhe_kklss_amd._abi import check, lib
    params, Q = ctx_of(name), FM.SETS[name]["Q"]
    rng = np.random.default_rng([k, limbs, 37])
    host = np.stack([np.stack([table_words(rng, Q[j], N) for j in range(limbs)]) for _ in range(1 + k)])
    want = np.stack([np.stack([FM.fold_words(host[s][j], Q[j], 0) for j in range(limbs)]) for s in range(1 + k)])
    ct = mkrlwe.NewCiphertext(params, ["p%d" % i for i in range(k)], limbs - 1).upload(host)
    check(lib().mkhe_ct_fold(params.ctx, ct.h))
    assert (ct.download() == want).all()


@pytest.mark.parametrize("name", sorted(FM.SETS))
def test_fold_pieces_equals_host_sum_and_swk_fold(ctx_of, name):
    """what mkhe.h claims: the mesh form gives the integers of the all-reduce form (8 pieces: the host's uint64 sum is exact)"""
    from mkhe_kklss_amd import mkrlwe
    from mkhe_kklss_amd._abi import check, lib
    params = ctx_of(name)
    pieces, want = uniform_case(name, 8, TOP)
    call = FoldPiecesCall(params, pieces, 0, LIMBS, TOP, 1, LIMBS * N)
    call.check(want[1])
    total = pieces.sum(axis=0, dtype=np.uint64)
    assert (total.astype(object) == FM.exact_sum(pieces)).all()
    swk = mkrlwe.SwitchingKey(params, total.reshape(DIGITS, MTOT, N))
    check(lib().mkhe_swk_fold(params.ctx, swk.h, TOP, 1))
    assert (swk.download().reshape(LIMBS, N) == call.dst_after[1:-1]).all()


# ---------------------------------------------------------------- 2e: past 16 pieces, and the argument checks
@pytest.mark.parametrize("fill", ["q_minus_1", "uniform"])
@pytest.mark.parametrize("npieces", [9, 16, 17, 33, 64])
@pytest.mark.parametrize("name", sorted(FM.SETS))
def test_fold_pieces_many_pieces(ctx_of, name, npieces, fill):
    """17 summands q - 1 of a 60-bit prime (33 of a 59-bit one) pass 2^64: the sum must be reduced on the way, not after.
    A kernel that adds the pieces in a plain uint64 returns wrong limbs with return code 0 (measured on an MI355X): in the q - 1 cases at 17 pieces on
    the limbs of the 60-bit primes (0, 6, 12, 18 of pn15; 4, 5, 10, 11, 16, 17, 22, 23 of pn14), at 33 and 64 pieces on those of the 59-bit primes too;
    in the uniform cases at 33 and 64 pieces.  It passes 9 and 16 pieces, and 17 uniform pieces, whose sums stay below 2^64."""
    if fill == "uniform":
        pieces, want = uniform_case(name, npieces, TOP)
        want = want[1]
    else:
        pieces, want = constant_case(name, lambda q: [q - 1] * npieces, 1)
        assert [int(want[l][0]) for l in range(LIMBS)] == [(q - npieces) * pow(2, 64, q) % q for q in limb_moduli(name)]
    FoldPiecesCall(ctx_of(name), pieces, 0, LIMBS, TOP, 1, LIMBS * N).check(want)


@pytest.mark.parametrize("name", sorted(FM.SETS))
def test_fold_pieces_argument_checks(ctx_of, name):
    """every bad call is refused on the host (non-zero, mkhe_last_error names fold_pieces, dst untouched); a good one on the same context then passes.
    The buffers are sized so that none of the calls, were it accepted, would leave them: `src` holds 65 limbs before and after the address passed."""
    import torch
    from mkhe_kklss_amd._abi import lib
    params = ctx_of(name)
    L = lib()
    src_before, dst_before = sentinel(130 * N, SENT_SRC), sentinel((LIMBS + 2) * N, SENT_DST)
    src, dst = to_device(src_before), to_device(dst_before)
    torch.cuda.synchronize()
    mid, key = src.data_ptr() + 8 * 65 * N, dst.data_ptr() + 8 * N            # key: limb 0 of the switching-key buffer

    def call(pieces=mid, npieces=2, stride=N, first=5, nlimbs=1, level=TOP, dst_ptr=None):
        at = key + 8 * first * N if dst_ptr is None else dst_ptr
        return L.mkhe_swk_fold_pieces(params.ctx, C.c_void_p(pieces), npieces, stride, first, nlimbs, level, 1, C.c_void_p(at))

    bad = {
        "npieces 0": dict(npieces=0), "npieces 65": dict(npieces=65),
        "null pieces": dict(pieces=None), "null dst": dict(dst_ptr=0),
        "first_limb < 0": dict(first=-1), "nlimbs < 0": dict(nlimbs=-1), "past the key": dict(first=23, nlimbs=2, stride=2 * N),
        "level -1": dict(level=-1), "level 4": dict(level=NQ),
        "stride < nlimbs * N": dict(nlimbs=2, stride=N), "stride 0": dict(stride=0), "stride one word short": dict(nlimbs=2, stride=2 * N - 1),
        "negative stride": dict(stride=-N), "negative stride, one piece": dict(npieces=1, stride=-1),
    }
    for what, kw in bad.items():
        rc = call(**kw)
        err = L.mkhe_last_error().decode()
        assert rc != 0, what + ": accepted"
        assert "fold_pieces" in err, "%s: %r" % (what, err)
        params.sync()
        assert (to_host(dst) == dst_before).all(), what + ": dst written"
    assert (to_host(src) == src_before).all()
    # the context still works: one piece with stride 0 (the stride is not used), then a 3-piece call
    pieces, want = uniform_case(name, 3, TOP)
    src1 = to_device(pieces[0, 5].copy())
    torch.cuda.synchronize()
    assert L.mkhe_swk_fold_pieces(params.ctx, C.c_void_p(src1.data_ptr()), 1, 0, 5, 1, TOP, 1, C.c_void_p(key + 8 * 5 * N)) == 0
    params.sync()
    got = to_host(dst).reshape(LIMBS + 2, N)
    assert (got[1 + 5] == FM.fold_words(pieces[0, 5], limb_moduli(name)[5], 1)).all()
    rest = np.ones(LIMBS + 2, dtype=bool)
    rest[1 + 5] = False
    assert (got[rest] == dst_before.reshape(LIMBS + 2, N)[rest]).all()
    FoldPiecesCall(params, pieces, 0, LIMBS, TOP, 1, LIMBS * N).check(want[1])
