"""Host-side mirror of the reference package `mkrlwe` for the accelerated path.

Same names, argument meaning and error behaviour as the Go types (reference file:line cited per
item); all polynomial data lives in HBM behind C-ABI handles (include/mkhe.h).  The Go reference
panics on misuse; here the same conditions raise `MkheError`/`KeyError` with the reference's text.
"""
import ctypes as C
import math

import numpy as np

from . import _abi
from ._abi import MkheError, check, handle_array, lib

GALOIS_GEN = 5  # lattigo rlwe.GaloisGen


class Parameters:
    """mkrlwe.Parameters (mkrlwe/params.go:8-12): ring parameters + CRS map + gamma, plus the
    engine context (= NewKeySwitcher state, keyswitch.go:33-47)."""

    def __init__(self, logN, Q, P, gamma=2, psiQ=None, psiP=None, device=0):
        self.logN, self._N = int(logN), 1 << int(logN)
        self.Q, self.P, self.gamma = [int(q) for q in Q], [int(p) for p in P], int(gamma)
        self.device = int(device)
        self._psi = (psiQ, psiP)
        self.ctx = self._create_context(psiQ, psiP)
        self.CRS = {}                      # idx -> SwitchingKey   (params.go:37-46)
        self._ids = {}                     # party id string -> dense int for the C ABI

    def _create_context(self, psiQ, psiP):
        q = np.asarray(self.Q, dtype=np.uint64)
        p = np.asarray(self.P, dtype=np.uint64)
        pq = np.asarray(psiQ, dtype=np.uint64) if psiQ is not None else None
        pp = np.asarray(psiP, dtype=np.uint64) if psiP is not None else None
        h = C.c_void_p()
        check(lib().mkhe_ctx_create(C.byref(h), self.logN, q.ctypes.data_as(_abi.u64p), len(self.Q),
                                    p.ctypes.data_as(_abi.u64p), len(self.P), self.gamma,
                                    pq.ctypes.data_as(_abi.u64p) if pq is not None else None,
                                    pp.ctypes.data_as(_abi.u64p) if pp is not None else None, self.device))
        return h

    def close(self):
        """destroys the engine context.  The CRS handles point back at this object (a reference cycle whose finalizers run in
        arbitrary order), so they are released here first; handles that outlive the context are freed by their own
        finalizer through the context-less path of mkhe_*_destroy (plain hipFree)."""
        if getattr(self, "ctx", None):
            if getattr(self, "_parent", None) is None:          # a fork shares its parent's CRS dictionary
                for key in list(getattr(self, "CRS", {}).values()):
                    key.__del__()
                self.CRS.clear()
            lib().mkhe_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # rlwe.Parameters accessors used by the reference
    def N(self): return self._N
    def LogN(self): return self.logN
    def QCount(self): return len(self.Q)
    def PCount(self): return len(self.P)
    def MaxLevel(self): return len(self.Q) - 1
    def Gamma(self): return self.gamma
    def Alpha(self): return self.PCount() // self.gamma                              # params.go:63-65
    def Beta(self, levelQ): return int(math.ceil((levelQ + 1) / self.Alpha()))       # params.go:67-71
    def SwkShape(self): return (self.Beta(self.MaxLevel()), self.QCount() + self.PCount(), self._N)

    def GaloisElementForColumnRotationBy(self, k):
        return pow(GALOIS_GEN, k % (2 * self._N), 2 * self._N)

    def GaloisElementForRowRotation(self):
        return 2 * self._N - 1

    def Psi(self, i):
        return int(lib().mkhe_ctx_psi(self.ctx, i))

    CRS_SEED = 0x4D4B4845          # default public seed of the device-side CRS expansion

    def AddCRS(self, idx, host_swk=None, seed=None):
        """params.AddCRS / NewParameters CRS slots (params.go:37-61,77-99).  With host_swk the uniform polys are
        sampled by the caller (NTT + Montgomery form) and uploaded once; without, CRS[idx] is expanded on the
        device from the public `seed` (mkhe_crs_expand: Philox4x32-10 + mask-and-reject, then MForm) -- every party
        that uses the same seed holds the same CRS and nothing is transferred."""
        if host_swk is not None:
            self.CRS[idx] = SwitchingKey(self, host_swk)
        else:
            self.CRS[idx] = SwitchingKey(self)
            check(lib().mkhe_crs_expand(self.ctx, self.CRS_SEED if seed is None else int(seed), int(idx), self.CRS[idx].h))
        return self.CRS[idx]

    def GenDefaultCRS(self, seed=None):
        """the CRS list NewParameters creates (params.go:37-46): 0, -1 (relin), -2 (conj), -3, -4 (BFV relin) and the
        power-of-two rotations"""
        for idx in [0, -1, -2, -3, -4] + [1 << i for i in range(self.logN - 1)]:
            self.AddCRS(idx, seed=seed)

    def party_index(self, pid):
        if pid == "0":
            raise MkheError("Cannot IDSet Add : 0 cannot be used")              # idset.go:12-16
        if pid not in self._ids:
            self._ids[pid] = len(self._ids)
        return self._ids[pid]

    def sync(self):
        check(lib().mkhe_ctx_sync(self.ctx))

    def Fork(self):
        """A second engine context over the same ring (own stream and scratch pools) that shares this object's CRS map,
        party ids and every key / ciphertext handle.  Operations issued through different forks run concurrently on
        the GPU; order them with wait_for.  (No reference counterpart: the Go evaluator is single-threaded.)"""
        import copy
        f = copy.copy(self)                 # same Q / P lists, same CRS and id dictionaries (shared objects)
        f.ctx = self._create_context(*self._psi)
        f._parent = self                    # the CRS handles belong to the parent's context: keep it alive
        return f

    def Capture(self):
        """context manager recording every engine call issued through this context (and through forks ordered after it and
        joined back) into a HIP graph: `with params.Capture() as g: ...calls...`, then g.launch() replays them with one
        submission.  Objects created inside the block are kept alive by the graph (their buffers are its temporaries)."""
        return Graph(self)

    def wait_for(self, other):
        """work issued through this context from now on starts after everything issued through `other` so far"""
        check(lib().mkhe_ctx_wait_for(self.ctx, other.ctx))

    def stream(self):
        return lib().mkhe_ctx_stream(self.ctx)


class Graph:
    """mkhe_capture_* / mkhe_graph_launch (include/mkhe.h): a captured sequence of engine calls."""

    def __init__(self, params):
        self.params, self.h, self.keep = params, None, []

    def __enter__(self):
        import gc
        # no destructor of an unrelated device object may run inside the capture window (hipFree / stream destruction are
        # device-wide operations): collect pending cyclic garbage now and keep the collector off until the capture ends
        gc.collect()
        self._gc = gc.isenabled()
        gc.disable()
        check(lib().mkhe_capture_begin(self.params.ctx))
        _live_graphs.append(self)
        return self

    def __exit__(self, et, ev, tb):
        import gc
        _live_graphs.remove(self)
        h = C.c_void_p()
        rc = lib().mkhe_capture_end(self.params.ctx, C.byref(h))
        if self._gc:
            gc.enable()
        if et is None:
            check(rc)
            self.h = h
        return False

    def launch(self):
        check(lib().mkhe_graph_launch(self.params.ctx, self.h))

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.params.sync()
                lib().mkhe_graph_destroy(self.h)
                self.h = None
        except Exception:
            pass


_live_graphs = []      # captures in progress: device objects created meanwhile are pinned to them (never freed before the graph)


def _pin(obj):
    for g in _live_graphs:
        g.keep.append(obj)


class SwitchingKey:
    """mkrlwe.SwitchingKey (keys.go:23-25): []rlwe.PolyQP of Beta(maxLevel) digits, resident in HBM.
    Host layout uint64[beta][nQ+nP][N]."""

    def __init__(self, params, host=None, zero=True):
        """zero=False: no zero fill (the key is about to be written by an engine call or an upload)"""
        self.params = params
        h = C.c_void_p()
        create = lib().mkhe_swk_create if (zero and host is None) else lib().mkhe_swk_create_uninit
        check(create(params.ctx, C.byref(h)))
        self.h = h
        _pin(self)
        if host is not None:
            self.upload(host)

    def upload(self, host):
        host = np.ascontiguousarray(host, dtype=np.uint64)
        if host.shape != self.params.SwkShape():
            raise MkheError("SwitchingKey: expected shape %r, got %r" % (self.params.SwkShape(), host.shape))
        check(lib().mkhe_swk_upload(self.params.ctx, self.h, host.ctypes.data_as(_abi.u64p)))

    def download(self):
        out = np.empty(self.params.SwkShape(), dtype=np.uint64)
        check(lib().mkhe_swk_download(self.params.ctx, self.h, out.ctypes.data_as(_abi.u64p)))
        return out

    def devptr(self):
        return lib().mkhe_swk_devptr(self.h)

    def __del__(self):
        try:
            if getattr(self, "h", None) and getattr(self, "_block", None) is None:
                lib().mkhe_swk_destroy(self.params.ctx, self.h)          # ctx None (context already closed): plain hipFree
                self.h = None
        except Exception:
            pass


def NewSwitchingKey(params):
    """keys.go:245-255"""
    return SwitchingKey(params)


class RelinearizationKey:
    """keys.go:34-37: Value = (b, d, v)."""

    def __init__(self, params, id, b=None, d=None, v=None):
        self.ID = id
        self.Value = [SwitchingKey(params, b), SwitchingKey(params, d), SwitchingKey(params, v)]


class RelinearizationKeySet:
    """keys.go:53-57,165-198"""

    def __init__(self, params):
        self.params = params
        self.Value = {}

    def AddRelinearizationKey(self, rlk):
        self.Value[rlk.ID] = rlk

    def DelRelinearizationKey(self, id):
        self.Value.pop(id, None)

    def GetRelinearizationKey(self, id):
        if id not in self.Value:
            raise MkheError("cannot GetRelinearizationKey: there is no relinearization key with given id")
        return self.Value[id]


class RotationKey:
    """keys.go:40-44"""

    def __init__(self, params, rotidx, id, value=None):
        self.ID, self.RotIdx = id, int(rotidx)
        self.Value = SwitchingKey(params, value)


class RotationKeySet:
    """keys.go:60-62,128-162"""

    def __init__(self):
        self.Value = {}

    def AddRotationKey(self, rk):
        self.Value.setdefault(rk.ID, {})[rk.RotIdx] = rk

    def GetRotationKey(self, id, rotidx):
        if id not in self.Value or rotidx not in self.Value[id]:
            raise MkheError("cannot GetRotationKeys: there is no rotation key with given id")
        return self.Value[id][rotidx]


class ConjugationKey:
    """keys.go:47-50"""

    def __init__(self, params, id, value=None):
        self.ID = id
        self.Value = SwitchingKey(params, value)


class ConjugationKeySet:
    """keys.go:65-67,200-228"""

    def __init__(self):
        self.Value = {}

    def AddConjugationKey(self, ck):
        self.Value[ck.ID] = ck

    def GetConjugationKey(self, id):
        if id not in self.Value:
            raise MkheError("cannot GetConjugationKey: there is no conjugation key with given id")
        return self.Value[id]


class HoistedCiphertext:
    """elements.go:5-15: map id -> SwitchingKey holding h(c_id)."""

    def __init__(self):
        self.Value = {}


def NewHoistedCiphertext():
    return HoistedCiphertext()


class Ciphertext:
    """mkrlwe.Ciphertext (elements.go:17-33): Value["0"] plus one poly per party id, all at the same
    level, coefficient domain.  Device layout uint64[1+n][level+1][N]; `ids` fixes the slot order."""

    def __init__(self, params, idset, level, zero=True):
        """zero=False: no zero fill (the ciphertext is about to be the ctOut of an engine call, which writes all of it)"""
        self.params = params
        self.ids = sorted(idset)
        for i in self.ids:
            params.party_index(i)
        self._level = int(level)
        arr = np.asarray([params.party_index(i) for i in self.ids], dtype=np.int32)
        h = C.c_void_p()
        create = lib().mkhe_ct_create if zero else lib().mkhe_ct_create_uninit
        check(create(params.ctx, len(self.ids), arr.ctypes.data_as(_abi.i32p), level + 1, C.byref(h)))
        self.h = h
        _pin(self)

    def IDSet(self):
        return set(self.ids)

    def Level(self):
        return self._level

    def slot(self, id):
        return 0 if id == "0" else 1 + self.ids.index(id)

    def shape(self):
        return (1 + len(self.ids), self._level + 1, self.params.N())

    def upload(self, host):
        host = np.ascontiguousarray(host, dtype=np.uint64)
        if host.shape != self.shape():
            raise MkheError("Ciphertext: expected shape %r, got %r" % (self.shape(), host.shape))
        check(lib().mkhe_ct_upload(self.params.ctx, self.h, host.ctypes.data_as(_abi.u64p)))
        return self

    def download(self):
        out = np.empty(self.shape(), dtype=np.uint64)
        check(lib().mkhe_ct_download(self.params.ctx, self.h, out.ctypes.data_as(_abi.u64p)))
        return out

    def set_values(self, value):
        """value: {"0": poly, id: poly} with polys uint64[level+1][N] (Go: ct.Value[id].Coeffs)."""
        host = np.zeros(self.shape(), dtype=np.uint64)
        for k, v in value.items():
            host[self.slot(k)] = np.asarray(v, dtype=np.uint64)[: self._level + 1]
        return self.upload(host)

    def values(self):
        host = self.download()
        out = {"0": host[0]}
        for a, i in enumerate(self.ids):
            out[i] = host[1 + a]
        return out

    def devptr(self):
        return lib().mkhe_ct_devptr(self.h)

    def __del__(self):
        try:
            if getattr(self, "h", None) and getattr(self, "_block", None) is None:
                lib().mkhe_ct_destroy(self.params.ctx, self.h)           # ctx None (context already closed): plain hipFree
                self.h = None
        except Exception:
            pass


def NewCiphertext(params, idset, level):
    """elements.go:22-33"""
    return Ciphertext(params, idset, level)


class _HandleBlock:
    """the handles of one mkhe_ct_create_batch / mkhe_swk_create_batch call: views of one pooled block, destroyed by ONE call when the last Python
    view is gone (every view keeps a reference to this object)"""

    def __init__(self, params, arr, count, destroy):
        self.params, self.arr, self.count, self.destroy = params, arr, count, destroy

    def __del__(self):
        try:
            if self.arr is not None:
                self.destroy(self.params.ctx, self.count, self.arr)
                self.arr = None
        except Exception:
            pass


def batch_ciphertexts(cls, params, idset, level, B, **attrs):
    """B uninitialised ciphertexts of one shape as views of one block (mkhe_ct_create_batch); cls: Ciphertext or a subclass, attrs: extra attributes"""
    ids = sorted(idset)
    arr_ids = np.asarray([params.party_index(i) for i in ids], dtype=np.int32)
    hs = (C.c_void_p * B)()
    check(lib().mkhe_ct_create_batch(params.ctx, B, len(ids), arr_ids.ctypes.data_as(_abi.i32p), level + 1, hs))
    block = _HandleBlock(params, hs, B, lib().mkhe_ct_destroy_batch)
    _pin(block)
    out = []
    for k in range(B):
        c = object.__new__(cls)
        c.params, c.ids, c._level, c.h, c._block = params, ids, int(level), C.c_void_p(hs[k]), block
        for a, v in attrs.items():
            setattr(c, a, v)
        out.append(c)
    return out


def batch_switching_keys(params, count):
    """count uninitialised switching keys / hoisted-digit vectors as views of one block (mkhe_swk_create_batch)"""
    hs = (C.c_void_p * count)()
    check(lib().mkhe_swk_create_batch(params.ctx, count, hs))
    block = _HandleBlock(params, hs, count, lib().mkhe_swk_destroy_batch)
    _pin(block)
    out = []
    for k in range(count):
        s = object.__new__(SwitchingKey)
        s.params, s.h, s._block = params, C.c_void_p(hs[k]), block
        out.append(s)
    return out


# ---- what the plaintext linear transforms of mkckks and mkbfv share (no reference counterpart)
def rotation_keys(params, rkSet, ids, rotations, prefix):
    """{r: the rotation-key handle of every id} for the rotation indices a transform needs; prefix opens the refusal of an index without a CRS"""
    keys = {}
    for r in rotations:
        if r not in params.CRS:
            raise MkheError("%s: no CRS for rotation index %d" % (prefix, r))
        keys[r] = [rkSet.GetRotationKey(i, r).Value.h for i in ids]              # (MkheError when a party has none)
    return keys


def rotate_lanes(params, keys, ids, srcs, rots, hoists, outs):
    """outs[i] = srcs[i] rotated by rots[i] != 0, as lanes of one mkhe_rotate_multi; keys: rotation_keys(..); hoists: one hoisted form per lane, or None"""
    gal = (C.c_uint64 * len(rots))(*[params.GaloisElementForColumnRotationBy(r) for r in rots])
    hs = handle_array([h.Value[i].h for h in hoists for i in ids]) if hoists is not None else None
    check(lib().mkhe_rotate_multi(params.ctx, len(rots), gal, handle_array([c.h for c in srcs]), hs, handle_array([h for r in rots for h in keys[r]]),
                                  handle_array([params.CRS[r].h for r in rots]), None, handle_array([o.h for o in outs])))
    return outs


def sum_in_groups(ctx, terms, new, group=16):
    """the sum of terms (ciphertexts of one shape): mkhe_ct_sum over groups of `group` into new() until one is left.  Sums of canonical residues: the
    grouping does not change a bit"""
    while len(terms) > 1:
        groups = [terms[i: i + group] for i in range(0, len(terms), group)]
        terms = []
        for grp in groups:
            terms.append(new())
            check(lib().mkhe_ct_sum(ctx, len(grp), handle_array([c.h for c in grp]), terms[-1].h))
    return terms[0]


class KeySwitcher:
    """mkrlwe.KeySwitcher (keyswitch.go:8-47).  The scratch pools of the reference (ks.Pool,
    swkPool1-3, polyQPool) are engine-internal device buffers owned by the context."""

    def __init__(self, params):
        self.Parameters = params
        self.ctx = params.ctx

    # -- Decompose (keyswitch.go:49-73)
    def Decompose(self, levelQ, ct, id, ad, is_ntt=False):
        check(lib().mkhe_decompose(self.ctx, levelQ, 1 if is_ntt else 0, ct.h, ct.slot(id), ad.h))

    # -- ExternalProduct (keyswitch.go:79-118): c <- ModDown(<h(a), bg>), a = ct.Value[id]
    def ExternalProduct(self, levelQ, ct, id, bg, out, out_id, is_ntt=False):
        check(lib().mkhe_external_product(self.ctx, levelQ, 1 if is_ntt else 0, ct.h, ct.slot(id), bg.h,
                                          out.h, out.slot(out_id)))

    # -- ExternalProductHoisted (keyswitch_hoisted.go:10-40)
    def ExternalProductHoisted(self, levelQ, aHoisted, bg, out, out_id):
        check(lib().mkhe_external_product_hoisted(self.ctx, levelQ, aHoisted.h, bg.h, out.h, out.slot(out_id)))

    # -- MulAndRelin (keyswitch.go:122-230)
    def MulAndRelin(self, op0, op1, rlkSet, ctOut):
        self.MulAndRelinHoisted(op0, op1, None, None, rlkSet, ctOut)

    # -- MulAndRelinHoisted (keyswitch_hoisted.go:44-179)
    def MulAndRelinHoisted(self, op0, op1, op0Hoisted, op1Hoisted, rlkSet, ctOut, rescaled=False):
        """rescaled=True (no reference counterpart at this level; mkckks.Evaluator.mulRelinHoisted, evaluator.go:558-581, is the caller):
        ctOut is one level below the product and receives Rescale(MulAndRelin(..)) in one engine call (mkhe_mul_relin_rescale)"""
        level = ctOut.Level() + (1 if rescaled else 0)
        if op0.Level() < level:
            raise MkheError("Cannot MulAndRelin: op0 and op1 have different levels")        # :48-50
        if op1.Level() < level:
            raise MkheError("Cannot MulAndRelin: op0 and op1 have different levels")
        params = self.Parameters
        if -1 not in params.CRS:
            raise MkheError("mkhe: CRS[-1] (u) has not been uploaded")
        d0 = [rlkSet.GetRelinearizationKey(i).Value[1].h for i in op0.ids]
        v0 = [rlkSet.GetRelinearizationKey(i).Value[2].h for i in op0.ids]
        b1 = [rlkSet.GetRelinearizationKey(i).Value[0].h for i in op1.ids]
        h0 = [op0Hoisted.Value[i].h for i in op0.ids] if op0Hoisted is not None else None
        if op1Hoisted is op0Hoisted and op1 is op0:
            h1 = h0
        else:
            h1 = [op1Hoisted.Value[i].h for i in op1.ids] if op1Hoisted is not None else None
        a_h0 = handle_array(h0)
        a_h1 = a_h0 if h1 is h0 else handle_array(h1)
        fn = lib().mkhe_mul_relin_rescale if rescaled else lib().mkhe_mul_and_relin
        check(fn(self.ctx, op0.h, op1.h, a_h0, a_h1, handle_array(b1), handle_array(d0),
                 handle_array(v0), params.CRS[-1].h, ctOut.h))

    # -- K products under one relinearisation tail (no reference counterpart; mkhe_mul_relin_sum, include/mkhe.h)
    def MulRelinSum(self, ops0, ops1, hoisted0, hoisted1, rlkSet, ctOut, rescaled=False):
        """ctOut = [Rescale] sum_k ops0[k] * ops1[k]; every ops0[k] carries the ids of ops0[0], every ops1[k] those of ops1[0];
        hoisted0 / hoisted1: one HoistedCiphertext per pair, or None (the engine hoists that side)"""
        if len(ops0) != len(ops1) or not ops0:
            raise MkheError("MulRelinSum: as many first operands as second ones, at least one pair")
        params = self.Parameters
        if -1 not in params.CRS:
            raise MkheError("mkhe: CRS[-1] (u) has not been uploaded")
        for side, hs in ((ops0, hoisted0), (ops1, hoisted1)):
            if hs is not None and len(hs) != len(side):
                raise MkheError("MulRelinSum: one hoisted form per pair")
        ids0, ids1 = ops0[0].ids, ops1[0].ids
        d0 = [rlkSet.GetRelinearizationKey(i).Value[1].h for i in ids0]
        v0 = [rlkSet.GetRelinearizationKey(i).Value[2].h for i in ids0]
        b1 = [rlkSet.GetRelinearizationKey(i).Value[0].h for i in ids1]
        h0 = [h.Value[i].h for h in hoisted0 for i in ids0] if hoisted0 is not None else None
        h1 = [h.Value[i].h for h in hoisted1 for i in ids1] if hoisted1 is not None else None
        check(lib().mkhe_mul_relin_sum(self.ctx, len(ops0), handle_array([c.h for c in ops0]), handle_array([c.h for c in ops1]),
                                       handle_array(h0), handle_array(h1), handle_array(b1), handle_array(d0), handle_array(v0),
                                       params.CRS[-1].h, 1 if rescaled else 0, ctOut.h))

    def _rotidx(self, rotidx):
        n2 = self.Parameters.N() // 2
        while rotidx < 0:
            rotidx += n2                                                                     # keyswitch.go:246-249
        return rotidx

    # -- Rotate (keyswitch.go:234-298)
    def Rotate(self, ctIn, rotidx, rkSet, ctOut):
        self.RotateHoisted(ctIn, rotidx, None, rkSet, ctOut)

    # -- RotateHoisted (keyswitch_hoisted.go:183-247)
    def RotateHoisted(self, ctIn, rotidx, ctInHoisted, rkSet, ctOut):
        params = self.Parameters
        if ctIn.Level() < ctOut.Level():
            raise MkheError("Cannot Rotate: ctIn and ctOut have different levels")
        rotidx = self._rotidx(rotidx)
        if rotidx not in params.CRS:
            raise MkheError("mkhe: no CRS for rotation index %d" % rotidx)
        rk = [rkSet.GetRotationKey(i, rotidx).Value.h for i in ctIn.ids]
        hs = [ctInHoisted.Value[i].h for i in ctIn.ids] if ctInHoisted is not None else None
        galEl = params.GaloisElementForColumnRotationBy(rotidx)
        check(lib().mkhe_rotate(self.ctx, galEl, ctIn.h, handle_array(hs), handle_array(rk), params.CRS[rotidx].h, ctOut.h))

    # -- Conjugate (keyswitch.go:302-332)
    def Conjugate(self, ctIn, ckSet, ctOut):
        params = self.Parameters
        if ctIn.Level() < ctOut.Level():
            raise MkheError("Cannot Conjugate: ctIn and ctOut have different levels")
        ck = [ckSet.GetConjugationKey(i).Value.h for i in ctIn.ids]
        check(lib().mkhe_conjugate(self.ctx, params.GaloisElementForRowRotation(), ctIn.h, handle_array(ck),
                                   params.CRS[-2].h, ctOut.h))


def NewKeySwitcher(params):
    return KeySwitcher(params)


# ---- key generation
class SecretKey:
    """mkrlwe.SecretKey (keys.go:9-12): Value = PolyQP (NTT, Montgomery form) resident on the device."""

    def __init__(self, params, id):
        self.ID = id
        self.Value = DeviceLimbs(params, 1, params.QCount() + params.PCount())


class PublicKey:
    """mkrlwe.PublicKey (keys.go:15-18): Value = [2]PolyQP, (-a*s + e, a)."""

    def __init__(self, params, id):
        self.ID = id
        self.Value = DeviceLimbs(params, 2, params.QCount() + params.PCount())


class HostSampler:
    """The small-norm samples of lattigo's ring.TernarySampler / ring.GaussianSampler, drawn on the HOST: secret
    randomness never comes from the GPU.

    Default (no argument): every draw is fed by os.urandom -- the kernel CSPRNG, the counterpart of lattigo's keyed
    blake2b XOF (utils.NewPRNG, keygen.go:26).  Uniform 64-bit words become 53-bit uniforms; ternary values come from
    one uniform each, Gaussians from Box-Muller pairs, rounded, and redrawn while |.| > 6 sigma like lattigo's sampler.

    `rng` (a numpy Generator) replaces the entropy source for REPRODUCIBLE TESTS AND BENCHMARKS ONLY and must be
    acknowledged with insecure_test_only=True: numpy's generators are not cryptographic."""

    def __init__(self, rng=None, sigma=3.2, insecure_test_only=False):
        if rng is not None and not insecure_test_only:
            raise MkheError("HostSampler: a numpy Generator is not a cryptographic source -- pass insecure_test_only=True "
                            "(tests / benchmarks), or no rng at all for os.urandom")
        self.rng = rng
        self.sigma, self.bound = float(sigma), int(6 * float(sigma))        # rlwe.DefaultSigma, keygen.go:36

    def _uniform(self, n):
        """n uniforms in [0, 1) with 53 random bits each"""
        if self.rng is not None:
            return self.rng.random(n)
        import os
        w = np.frombuffer(os.urandom(8 * n), dtype=np.uint64)
        return (w >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))

    def _normal(self, n):
        if self.rng is not None:
            return self.rng.normal(0.0, self.sigma, n)
        m = (n + 1) // 2
        u1, u2 = 1.0 - self._uniform(m), self._uniform(m)                   # u1 in (0, 1]
        r = np.sqrt(-2.0 * np.log(u1)) * self.sigma
        return np.concatenate([r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2)])[:n]

    def ternary(self, N, p=0.5):
        """0 with probability p, +-1 with (1-p)/2 each (GenSecretKeyWithDistrib keygen.go:69-76)"""
        u = self._uniform(N)
        return np.where(u < p, 0, np.where(u < p + (1 - p) / 2, 1, -1)).astype(np.int32)

    def ternary_hw(self, N, h):
        """exactly h non-zero coefficients, their positions a uniform h-subset of the N (the h smallest of N uniforms) and their signs uniform: the
        sparse secret of a bootstrapping, whose raised phase carries an integer part of standard deviation about sqrt((1 + h) / 12) per key"""
        N, h = int(N), int(h)
        if not 0 <= h <= N:
            raise MkheError("HostSampler.ternary_hw: the Hamming weight must lie between 0 and N = %d, got %d" % (N, h))
        s = np.zeros(N, dtype=np.int32)
        pos = np.argsort(self._uniform(N), kind="stable")[:h]
        s[pos] = np.where(self._uniform(h) < 0.5, 1, -1)
        return s

    def gaussian(self, count, N):
        """round(N(0, sigma)), resampled while |.| > bound"""
        e = np.rint(self._normal(count * N)).reshape(count, N)
        bad = np.abs(e) > self.bound
        while bad.any():
            e[bad] = np.rint(self._normal(int(bad.sum())))
            bad = np.abs(e) > self.bound
        return e.astype(np.int32)


def small_cdt(sigma, bound=None):
    """The table of mkhe_sample_small / mkhe_encrypt_seeded (kind 1) for the rounded Gaussian of HostSampler.gaussian: round(N(0, sigma))
    truncated at +-B, B = int(6 sigma) by default.  With Phi(x) = erfc(-x / (sigma sqrt 2)) / 2, lo = Phi(-B - 1/2), hi = Phi(B + 1/2):
    T_k = min(2^64 - 1, floor((Phi(k + 1/2) - lo) / (hi - lo) * 2^64)) for k = -B .. B - 1, so that #{k : r >= T_k} - B has the
    probabilities of the truncated rounded Gaussian to float64 precision.  A pure function -> list of 2B Python ints."""
    sigma = float(sigma)
    if not (sigma > 0.0 and math.isfinite(sigma)):
        raise MkheError("small_cdt: sigma must be finite and positive")
    B = int(6 * sigma) if bound is None else int(bound)
    if B < 1 or 2 * B > 64:
        raise MkheError("small_cdt: the table has 2 * bound entries and holds 2 .. 64 (bound = %d)" % B)
    phi = lambda x: math.erfc(-x / (sigma * math.sqrt(2.0))) / 2.0
    lo, hi = phi(-B - 0.5), phi(B + 0.5)
    # (p * 2^64 as an exact integer: a float64 in [0, 1] times 2^64 is an integer or has an exact floor)
    table = [min((1 << 64) - 1, int(math.floor((phi(k + 0.5) - lo) / (hi - lo) * 18446744073709551616.0))) for k in range(-B, B)]
    if any(b <= a for a, b in zip(table, table[1:])):
        raise MkheError("small_cdt: the table is not strictly increasing (sigma too small for this bound)")
    return table


def _key_words(key, who):
    """32 bytes or 8 words of 32 bits -> (uint32 * 8)"""
    if isinstance(key, (bytes, bytearray)):
        if len(key) != 32:
            raise MkheError("%s: the key is 32 bytes" % who)
        words = [int.from_bytes(key[4 * i: 4 * i + 4], "little") for i in range(8)]
    else:
        words = [int(w) for w in key]
        if len(words) != 8 or any(not 0 <= w < (1 << 32) for w in words):
            raise MkheError("%s: the key is 8 words of 32 bits" % who)
    return (C.c_uint32 * 8)(*words)


class DeviceSampler:
    """Encryption randomness drawn ON THE DEVICE: u, e0, e1 are expanded by the engine from a ChaCha20 key (include/mkhe.h, "device-side
    sampling"), so that an Encrypt moves 32 + 8 bytes of key and nonce instead of 12 N bytes of samples.  For Encryptor only: keys are
    long-term and one-off, KeyGenerator keeps its host sampler.

    key=None (default): 32 bytes from os.urandom.  A given key (32 bytes, or 8 uint32 words) makes every draw reproducible and must be
    acknowledged with insecure_test_only=True -- the policy of HostSampler(rng=...).  Every engine call consumes one nonce of a 64-bit
    counter (advanced under a lock): a (key, nonce) pair never serves two calls.  The Gaussian is the table small_cdt(sigma)."""

    def __init__(self, key=None, sigma=3.2, insecure_test_only=False):
        import os
        import threading
        if key is not None and not insecure_test_only:
            raise MkheError("DeviceSampler: a given key makes the samples reproducible -- pass insecure_test_only=True "
                            "(tests / benchmarks), or no key at all for os.urandom")
        if key is None:
            key = os.urandom(32)
        self._key = _key_words(key, "DeviceSampler")
        self.sigma = float(sigma)
        self.cdt = small_cdt(self.sigma)
        self._cdt = (C.c_uint64 * len(self.cdt))(*self.cdt)
        self._lock = threading.Lock()
        self._counter = 0

    @property
    def counter(self):
        """the nonce the next engine call will use"""
        return self._counter

    def _next_nonce(self):
        with self._lock:
            if self._counter >= (1 << 64) - 1:
                raise MkheError("DeviceSampler: the 64-bit call counter is exhausted -- use a fresh key")
            n = self._counter
            self._counter += 1
            return n

    def encrypt_args(self):
        """(key, nonce, cdt, ncdt) for ONE mkhe_encrypt_seeded call"""
        return self._key, self._next_nonce(), self._cdt, len(self.cdt)

    def share_args(self):
        """(key, nonce) for ONE mkhe_decrypt_share call: the same counter as encrypt_args, so that no nonce serves two calls of either kind"""
        return self._key, self._next_nonce()

    def switch_args(self):
        """(key, nonce, cdt, ncdt) for ONE mkhe_pcks_share call: the same counter as the other calls"""
        return self._key, self._next_nonce(), self._cdt, len(self.cdt)

    def sk_encrypt_args(self):
        """(e_key, e_nonce, cdt, ncdt) for ONE mkhe_encrypt_sk_seeded call: the same counter as the other calls"""
        return self._key, self._next_nonce(), self._cdt, len(self.cdt)

    def threshold_args(self):
        """(key, nonce) for ONE mkhe_threshold_gen_shares call: the same counter as the other calls"""
        return self._key, self._next_nonce()

    def e2s_args(self):
        """(key, nonce_mask) for ONE mkhe_e2s_share / mkhe_bfv_e2s_share call: one value of the same counter, taken under the lock"""
        return self._key, self._next_nonce()

    def refresh_args(self):
        """(key, nonce_mask, nonce_enc) for ONE mkhe_refresh_share call: two values of the same counter, taken under the lock"""
        with self._lock:
            if self._counter >= (1 << 64) - 2:
                raise MkheError("DeviceSampler: the 64-bit call counter is exhausted -- use a fresh key")
            n = self._counter
            self._counter += 2
        return self._key, n, n + 1


def _s32(a, shape):
    a = np.ascontiguousarray(a, dtype=np.int32)
    if a.shape != tuple(shape):
        raise MkheError("keygen: expected samples of shape %r, got %r" % (tuple(shape), a.shape))
    return a, a.ctypes.data_as(_abi.s32p)


class KeyGenerator:
    """mkrlwe.KeyGenerator (keygen.go:13-40) on the device.  Every Gen* method takes the samples it would draw as an
    optional argument (`s` / `e`, int32) -- given, the result is a deterministic function of them (parity tests);
    omitted, they come from `sampler`."""

    def __init__(self, params, sampler=None):
        if isinstance(sampler, DeviceSampler):
            raise MkheError("KeyGenerator: keys are long-term and one-off, their samples stay host-drawn -- a DeviceSampler serves Encryptor only")
        self.params = params
        self.sampler = sampler if sampler is not None else HostSampler()

    def _beta(self):
        return self.params.Beta(self.params.MaxLevel())

    def _errors(self, e, count):
        N = self.params.N()
        if e is None:
            e = self.sampler.gaussian(int(np.prod(count)), N)
        return _s32(np.asarray(e).reshape(tuple(np.atleast_1d(count)) + (N,)), tuple(np.atleast_1d(count)) + (N,))

    def GenSecretKey(self, id, s=None):
        """keygen.go:58-60 (ternary, P(0) = 1/2) -> genSecretKeyFromSampler :44-55"""
        return self.GenSecretKeyWithDistrib(0.5, id, s)

    def GenSecretKeyWithDistrib(self, p, id, s=None):
        """keygen.go:69-76"""
        if s is None:
            s = self.sampler.ternary(self.params.N(), p)
        a, ptr = _s32(s, (self.params.N(),))
        sk = SecretKey(self.params, id)
        check(lib().mkhe_keygen_secret(self.params.ctx, ptr, sk.Value.devptr()))
        return sk

    def GenSecretKeySparse(self, id, h):
        """a ternary key of Hamming weight exactly h, signs uniform (HostSampler.ternary_hw; no reference counterpart): what mkckks.Bootstrapper asks of
        every party"""
        return self.GenSecretKeyWithDistrib(0.0, id, self.sampler.ternary_hw(self.params.N(), h))

    def GenSecretKeyGaussian(self, id, s=None):
        """keygen.go:63-65"""
        if s is None:
            s = self.sampler.gaussian(1, self.params.N())[0]
        return self.GenSecretKeyWithDistrib(0.0, id, s)

    def GenPublicKey(self, sk, e=None):
        """keygen.go:88-109"""
        if 0 not in self.params.CRS:
            raise MkheError("cannot GenPublicKey: CRS[0] is not generated")
        a, ptr = self._errors(e, 1)
        pk = PublicKey(self.params, sk.ID)
        check(lib().mkhe_keygen_public_key(self.params.ctx, sk.Value.devptr(), ptr, self.params.CRS[0].h, pk.Value.devptr()))
        return pk

    def GenKeyPair(self, id):
        """keygen.go:112-115"""
        sk = self.GenSecretKey(id)
        return sk, self.GenPublicKey(sk)

    def GenSwitchingKey(self, skIn, swk, e=None):
        """keygen.go:270-327: swk <- g*skIn + e in MForm"""
        a, ptr = self._errors(e, self._beta())
        check(lib().mkhe_keygen_switching_key(self.params.ctx, skIn.Value.devptr(), ptr, swk.h))

    def GenRelinearizationKey(self, sk, r, e=None):
        """keygen.go:137-187; e: [3][beta][N] for b, d, v"""
        params = self.params
        if params.PCount() == 0:
            raise MkheError("modulus P is empty")
        a, ptr = self._errors(e, (3, self._beta()))
        rlk = RelinearizationKey(params, sk.ID)
        check(lib().mkhe_keygen_relin_key(params.ctx, sk.Value.devptr(), r.Value.devptr(), ptr, params.CRS[0].h, params.CRS[-1].h,
                                          rlk.Value[0].h, rlk.Value[1].h, rlk.Value[2].h))
        return rlk

    def GenRotationKey(self, rotidx, sk, e=None):
        """keygen.go:190-229"""
        params = self.params
        if rotidx not in params.CRS:
            raise MkheError("Cannot GenRotationKey: CRS for given rot idx is not generated")
        crs = params.CRS[rotidx]
        while rotidx < 0:
            rotidx += params.N() // 2
        a, ptr = self._errors(e, self._beta())
        rk = RotationKey(params, rotidx, sk.ID)
        check(lib().mkhe_keygen_rotation_key(params.ctx, params.GaloisElementForColumnRotationBy(rotidx), sk.Value.devptr(), ptr,
                                             crs.h, rk.Value.h))
        return rk

    def GenDefaultRotationKeys(self, sk, rtkSet):
        """keygen.go:232-237"""
        rotidx = 1
        while rotidx < self.params.N() // 2:
            rtkSet.AddRotationKey(self.GenRotationKey(rotidx, sk))
            rotidx *= 2

    def GenConjugationKey(self, sk, e=None):
        """keygen.go:240-268"""
        params = self.params
        a, ptr = self._errors(e, self._beta())
        ck = ConjugationKey(params, sk.ID)
        check(lib().mkhe_keygen_conjugation_key(params.ctx, sk.Value.devptr(), ptr, params.CRS[-2].h, ck.Value.h))
        return ck


def NewKeyGenerator(params, sampler=None):
    return KeyGenerator(params, sampler)


# ---- raw device buffers for ring-level calls (tests / bench of the NTT kernel)
class DeviceLimbs:
    """uint64[count][limbs][N] raw device buffer (mkhe_buf_*)."""

    def __init__(self, params, count, limbs):
        self.params, self.count, self.limbs = params, count, limbs
        self.words = count * limbs * params.N()
        d = C.c_void_p()
        check(lib().mkhe_buf_alloc(params.ctx, self.words, C.byref(d)))
        self.d = d
        _pin(self)

    def upload(self, host):
        host = np.ascontiguousarray(host, dtype=np.uint64)
        assert host.shape == (self.count, self.limbs, self.params.N())
        check(lib().mkhe_buf_upload(self.params.ctx, self.d, host.ctypes.data_as(_abi.u64p), self.words))
        return self

    def download(self):
        out = np.empty((self.count, self.limbs, self.params.N()), dtype=np.uint64)
        check(lib().mkhe_buf_download(self.params.ctx, self.d, out.ctypes.data_as(_abi.u64p), self.words))
        return out

    def devptr(self):
        return self.d

    def __del__(self):
        try:
            if getattr(self, "d", None) and self.params.ctx:
                lib().mkhe_buf_free(self.params.ctx, self.d)
                self.d = None
        except Exception:
            pass


def ntt(params, src, dst, mod_base=0, inverse=False, lazy=False):
    """ring.NTTLvl / InvNTTLvl / InvNTTLazyLvl on DeviceLimbs buffers (limb l under modulus mod_base+l)."""
    assert src.count == dst.count and src.limbs == dst.limbs
    check(lib().mkhe_ntt(params.ctx, src.devptr(), dst.devptr(), src.count, src.limbs, mod_base,
                         1 if inverse else 0, 1 if lazy else 0))


# ---- public-key encryption and decryption (mkrlwe/encryptor.go, mkrlwe/decryptor.go, keys.go:70-121)
class SecretKeySet:
    """keys.go:70-94"""

    def __init__(self):
        self.Value = {}

    def AddSecretKey(self, sk):
        self.Value[sk.ID] = sk

    def DelSecretKey(self, id):
        self.Value.pop(id, None)

    def GetSecretKey(self, id):
        if id not in self.Value:
            raise MkheError("cannot GetPublicKey: there is no public key with given id")       # keys.go:91 (the reference's own text)
        return self.Value[id]


def NewSecretKeySet():
    return SecretKeySet()


class PublicKeySet:
    """keys.go:96-122"""

    def __init__(self):
        self.Value = {}

    def AddPublicKey(self, pk):
        self.Value[pk.ID] = pk

    def DelPublicKey(self, id):
        self.Value.pop(id, None)

    def GetPublicKey(self, id):
        if id not in self.Value:
            raise MkheError("cannot GetPublicKey: there is no public key with given id")
        return self.Value[id]


def NewPublicKeyKeySet():
    return PublicKeySet()


def _device_plaintexts(params, pts):
    """plaintexts for the engine: DeviceLimbs [B][limbs][N] as they are; a host array [B][limbs][N] / a list of [limbs][N] is uploaded"""
    if isinstance(pts, DeviceLimbs):
        return pts
    host = np.ascontiguousarray(np.stack([np.asarray(p, dtype=np.uint64) for p in pts]) if isinstance(pts, (list, tuple)) else pts, dtype=np.uint64)
    if host.ndim != 3 or host.shape[0] < 1 or host.shape[2] != params.N():
        raise MkheError("Cannot Encrypt: expected plaintexts of shape [count][limbs][%d], got %r" % (params.N(), host.shape))
    return DeviceLimbs(params, host.shape[0], host.shape[1]).upload(host)


class Encryptor:
    """mkrlwe.Encryptor (encryptor.go:8-52) on the device.  u (ternary, P(0) = 1/2) and e0, e1 (Gaussian: the sampler's sigma and bound)
    are drawn on the HOST from `sampler`, like the secrets and errors of KeyGenerator; given as `samples` (int32 [3][N]: u, e0, e1) the
    result is a deterministic function of them (parity tests).  With a DeviceSampler (and no explicit `samples`) they are drawn on the
    DEVICE instead: mkhe_encrypt_seeded, one nonce of the sampler's counter per call, nothing but key and nonce crossing the bus.
    Plaintexts are RNS polynomials: DeviceLimbs or host uint64 arrays."""

    def __init__(self, params, sampler=None):
        self.params = params
        self.sampler = sampler if sampler is not None else HostSampler()

    def _samples(self, samples, count):
        N = self.params.N()
        if samples is None:
            samples = np.stack([np.concatenate([self.sampler.ternary(N, 0.5)[None], self.sampler.gaussian(2, N)]) for _ in range(count)])
        return _s32(samples, (count, 3, N))

    def _check_level(self, level):
        if not 0 <= level <= self.params.MaxLevel():
            raise MkheError("Cannot Encrypt: level %d out of range" % level)

    def _new_batch(self, id, level, count, like=None):
        return batch_ciphertexts(Ciphertext, self.params, [id], level, count)

    def _draw(self, samples, count):
        """the host samples of one engine call as (array, pointer); None where the engine draws them itself (a DeviceSampler and no `samples`)"""
        if samples is None and isinstance(self.sampler, DeviceSampler):
            return None
        return self._samples(samples, count)

    def _engine_encrypt(self, level, pk, d, pt_is_ntt, smp, outs):
        """one engine call over the plaintexts d: mkhe_encrypt on host samples, mkhe_encrypt_seeded (one nonce of the sampler) without"""
        args = (self.params.ctx, level, d.count, pk.Value.devptr(), d.devptr(), 1 if pt_is_ntt else 0)
        if smp is None:
            check(lib().mkhe_encrypt_seeded(*args, *self.sampler.encrypt_args(), handle_array([c.h for c in outs])))
        else:
            check(lib().mkhe_encrypt(*args, smp[1], handle_array([c.h for c in outs])))

    def Encrypt(self, pt, pk, ctOut, samples=None, pt_is_ntt=False):
        """encryptor.go:55-118.  pt: one plaintext [limbs][N] (or DeviceLimbs of count 1) with at least ctOut.Level() + 1 limbs; the Go
        version shortens ctOut to a lower plaintext level, a device ciphertext keeps its shape, so that case raises."""
        if ctOut.ids != [pk.ID]:
            raise MkheError("Cannot Encrypt: ctOut must be a ciphertext over the id of pk alone")
        d = pt if isinstance(pt, DeviceLimbs) else _device_plaintexts(self.params, np.asarray(pt, dtype=np.uint64)[None])
        if d.count != 1:
            raise MkheError("Cannot Encrypt: one plaintext expected (EncryptBatch takes several)")
        level = ctOut.Level()
        self._check_level(level)
        if d.limbs < level + 1:
            raise MkheError("Cannot Encrypt: the plaintext is below the level of ctOut")
        self._engine_encrypt(level, pk, d, pt_is_ntt, self._draw(None if samples is None else np.asarray(samples)[None], 1), [ctOut])
        return ctOut

    def EncryptBatch(self, pts, pk, samples=None, pt_is_ntt=False):
        """B plaintexts ([B][level+1][N]) under one public key as ONE engine call (mkhe_encrypt: five launches whatever B is);
        samples: int32 [B][3][N].  Returns the list of B ciphertexts over {pk.ID} (views of one device block)."""
        d = _device_plaintexts(self.params, pts)
        level = d.limbs - 1
        self._check_level(level)
        smp = self._draw(samples, d.count)
        outs = self._new_batch(pk.ID, level, d.count)
        self._engine_encrypt(level, pk, d, pt_is_ntt, smp, outs)
        return outs


def NewEncryptor(params, sampler=None):
    return Encryptor(params, sampler)


# ---- secret-key encryption with a seeded c1 (include/mkhe.h, "secret-key encryption"; no reference counterpart)
class SeededCiphertext:
    """`count` fresh ciphertexts of party `id` at `level` in their half-size form: the c0 polynomials plus the PUBLIC (Key, Nonce) that c1 is
    expanded from (kind 6 of the keystream).  c0 lives in polynomial 0 of `count` device ciphertexts whose polynomial 1 is not yet written.
    download() -> (c0 uint64 [count][level+1][N], key 32 bytes, nonce) is what travels; the receiver builds
    SeededCiphertext(params, id, level, count).upload(c0, key, nonce) and calls Expand().  Only fresh ciphertexts have a seed."""

    def __init__(self, params, id, level, count=1, cls=Ciphertext, **attrs):
        if not 0 <= int(level) <= params.MaxLevel():
            raise MkheError("SeededCiphertext: level %d out of range" % level)
        if not 1 <= int(count) <= 65535:
            raise MkheError("SeededCiphertext: count must be 1 .. 65535")
        self.params, self.ID, self._level, self.count = params, id, int(level), int(count)
        self._cls, self._attrs = cls, dict(attrs)
        self._cts = batch_ciphertexts(cls, params, [id], self._level, self.count, **attrs)
        self.Key, self.Nonce = None, None
        self._expanded = False

    def Level(self):
        return self._level

    def _set_seed(self, key, nonce):
        self._key = _key_words(key, "SeededCiphertext")
        self.Key = b"".join(int(w).to_bytes(4, "little") for w in self._key)
        self.Nonce = int(nonce)
        if not 0 <= self.Nonce < (1 << 64):
            raise MkheError("SeededCiphertext: the nonce is 64 bits")
        return self

    def _limb_ptrs(self, rows):
        return (C.c_void_p * len(rows))(*[r.ctypes.data for r in rows])

    def download(self):
        if self.Key is None:
            raise MkheError("SeededCiphertext: nothing to download (no seed yet)")
        N = self.params.N()
        c0 = np.empty((self.count, self._level + 1, N), dtype=np.uint64)
        for b, ct in enumerate(self._cts):
            check(lib().mkhe_ct_download_poly_limbs(self.params.ctx, ct.h, 0, self._limb_ptrs(list(c0[b]))))
        return c0, self.Key, self.Nonce

    def upload(self, c0, key, nonce):
        c0 = np.ascontiguousarray(c0, dtype=np.uint64)
        if c0.shape != (self.count, self._level + 1, self.params.N()):
            raise MkheError("SeededCiphertext: expected c0 of shape %r, got %r" % ((self.count, self._level + 1, self.params.N()), c0.shape))
        if self._expanded:
            raise MkheError("SeededCiphertext: already expanded")
        self._set_seed(key, nonce)
        for b, ct in enumerate(self._cts):
            check(lib().mkhe_ct_upload_poly_limbs(self.params.ctx, ct.h, 0, self._limb_ptrs(list(c0[b]))))
        return self

    def Expand(self, level=None):
        """-> `count` ordinary ciphertexts over {ID}: mkhe_ct_expand_seeded writes polynomial 1.  level=None (or the level of c0): the
        ciphertexts that hold c0 themselves, no copy.  A lower level: new ciphertexts with the first level + 1 limbs of c0 (through the host)
        and the same rows of a -- they do not depend on the level they are expanded at."""
        if self.Key is None:
            raise MkheError("SeededCiphertext: nothing to expand (no seed yet)")
        level = self._level if level is None else int(level)
        if not 0 <= level <= self._level:
            raise MkheError("SeededCiphertext: cannot expand at level %d (c0 is at level %d)" % (level, self._level))
        if level == self._level:
            outs = self._cts
            if self._expanded:
                return outs
        else:
            c0 = self.download()[0]
            outs = batch_ciphertexts(self._cls, self.params, [self.ID], level, self.count, **self._attrs)
            for b, ct in enumerate(outs):
                check(lib().mkhe_ct_upload_poly_limbs(self.params.ctx, ct.h, 0, self._limb_ptrs(list(c0[b][: level + 1]))))
        check(lib().mkhe_ct_expand_seeded(self.params.ctx, self.count, self._key, self.Nonce, handle_array([c.h for c in outs])))
        if level == self._level:
            self._expanded = True
        return outs


class SecretKeyEncryptor:
    """Encryption under the party's OWN secret key with c1 expanded from a public seed: c1 = a, c0 = pt + e - a s (include/mkhe.h,
    "secret-key encryption").  The phase error is e alone, and a fresh ciphertext travels as c0 plus 40 bytes (EncryptSeededBatch).

    sampler: a HostSampler (default; e is drawn on the host, mkhe_encrypt_sk) or a DeviceSampler (mkhe_encrypt_sk_seeded: e is formed in
    registers from one nonce of the sampler's counter).  seed: 32 PUBLIC bytes (default os.urandom(32)); every engine call takes one value
    of the encryptor's own locked 64-bit counter as the nonce of a -- an (a_key, a_nonce) pair serves one call.  A given seed makes a
    reproducible and must be acknowledged with insecure_test_only=True, the policy of DeviceSampler."""

    def __init__(self, params, sk, sampler=None, seed=None, insecure_test_only=False):
        import os
        import threading
        if seed is not None and not insecure_test_only:
            raise MkheError("SecretKeyEncryptor: a given seed makes c1 reproducible -- pass insecure_test_only=True "
                            "(tests / benchmarks), or no seed at all for os.urandom")
        self.params, self.sk = params, sk
        self.sampler = sampler if sampler is not None else HostSampler()
        self._seed = _key_words(os.urandom(32) if seed is None else seed, "SecretKeyEncryptor")
        self._lock = threading.Lock()
        self._counter = 0

    @property
    def counter(self):
        """the nonce of a the next engine call will use"""
        return self._counter

    def _next_nonce(self):
        with self._lock:
            if self._counter >= (1 << 64) - 1:
                raise MkheError("SecretKeyEncryptor: the 64-bit call counter is exhausted -- use a fresh seed")
            n = self._counter
            self._counter += 1
            return n

    def _check_level(self, level):
        if not 0 <= level <= self.params.MaxLevel():
            raise MkheError("Cannot Encrypt: level %d out of range" % level)

    def _engine_encrypt(self, level, d, pt_is_ntt, e, outs):
        """one engine call over the plaintexts d into outs; returns the nonce of a it used"""
        nonce = self._next_nonce()
        args = (self.params.ctx, level, d.count, self.sk.Value.devptr(), d.devptr(), 1 if pt_is_ntt else 0, self._seed, nonce)
        hs = handle_array([c.h for c in outs])
        if e is None and isinstance(self.sampler, DeviceSampler):
            check(lib().mkhe_encrypt_sk_seeded(*args, *self.sampler.sk_encrypt_args(), hs))
        else:
            N = self.params.N()
            smp = _s32(self.sampler.gaussian(d.count, N) if e is None else e, (d.count, N))
            check(lib().mkhe_encrypt_sk(*args, smp[1], hs))
        return nonce

    def _new_batch(self, level, count):
        return batch_ciphertexts(Ciphertext, self.params, [self.sk.ID], level, count)

    def _new_seeded(self, level, count):
        return SeededCiphertext(self.params, self.sk.ID, level, count)

    def Encrypt(self, pt, ctOut, e=None, pt_is_ntt=False):
        """pt: one plaintext [limbs][N] (or DeviceLimbs of count 1) with at least ctOut.Level() + 1 limbs; e: int32 [N] (parity tests)"""
        if ctOut.ids != [self.sk.ID]:
            raise MkheError("Cannot Encrypt: ctOut must be a ciphertext over the id of sk alone")
        d = pt if isinstance(pt, DeviceLimbs) else _device_plaintexts(self.params, np.asarray(pt, dtype=np.uint64)[None])
        if d.count != 1:
            raise MkheError("Cannot Encrypt: one plaintext expected (EncryptBatch takes several)")
        level = ctOut.Level()
        self._check_level(level)
        if d.limbs != level + 1:
            raise MkheError("Cannot Encrypt: the plaintext must have the limbs of ctOut")
        self._engine_encrypt(level, d, pt_is_ntt, None if e is None else np.asarray(e)[None], [ctOut])
        return ctOut

    def EncryptBatch(self, pts, e=None, pt_is_ntt=False):
        """B plaintexts ([B][level+1][N]) as ONE engine call; e: int32 [B][N].  Returns the list of B ciphertexts over {sk.ID}."""
        d = _device_plaintexts(self.params, pts)
        level = d.limbs - 1
        self._check_level(level)
        outs = self._new_batch(level, d.count)
        self._engine_encrypt(level, d, pt_is_ntt, e, outs)
        return outs

    def EncryptSeededBatch(self, pts, e=None, pt_is_ntt=False):
        """the same call, returned in the half-size form: a SeededCiphertext (c0 on the device, the seed and the nonce of this call)"""
        d = _device_plaintexts(self.params, pts)
        level = d.limbs - 1
        self._check_level(level)
        sc = self._new_seeded(level, d.count)
        nonce = self._engine_encrypt(level, d, pt_is_ntt, e, sc._cts)
        sc._set_seed(self._seed, nonce)
        sc._expanded = True                                 # (the engine has written polynomial 1 as well: Expand() has nothing left to do)
        return sc


def NewSecretKeyEncryptor(params, sk, sampler=None, seed=None, insecure_test_only=False):
    return SecretKeyEncryptor(params, sk, sampler, seed, insecure_test_only)


class DecryptionShare:
    """What one party publishes in distributed decryption (include/mkhe.h, "distributed decryption"): mu = c_id * s_id + e for `count`
    ciphertexts at `level`, uint64 [count][level+1][N] on the device.  Shares travel between parties: download() gives the host array,
    upload() takes it on the receiving side (DecryptionShare(params, id, level, count).upload(host))."""

    def __init__(self, params, id, level, count=1):
        self.ID, self._level, self.count = id, int(level), int(count)
        self.Value = DeviceLimbs(params, self.count, self._level + 1)

    def Level(self):
        return self._level

    def download(self):
        return self.Value.download()

    def upload(self, host):
        self.Value.upload(host)
        return self


def order_shares(ids, level, count, shares):
    """the shares of a merge in the slot order of a ciphertext over `ids`; raises on a missing or duplicate share, on one of a party the
    ciphertext does not have, at another level or for another batch size.  Pure: no engine call."""
    by_id = {}
    for sh in shares:
        if sh.ID in by_id:
            raise MkheError("Cannot MergeShares: two shares of party %r" % (sh.ID,))
        if sh.ID not in ids:
            raise MkheError("Cannot MergeShares: a share of party %r, which the ciphertext does not have" % (sh.ID,))
        if sh.Level() != level:
            raise MkheError("Cannot MergeShares: the share of party %r is at level %d, the ciphertext at level %d" % (sh.ID, sh.Level(), level))
        if sh.count != count:
            raise MkheError("Cannot MergeShares: the share of party %r is for %d ciphertexts, the merge for %d" % (sh.ID, sh.count, count))
        by_id[sh.ID] = sh
    for i in ids:
        if i not in by_id:
            raise MkheError("Cannot MergeShares: the share of party %r is missing" % (i,))
    return [by_id[i] for i in ids]


class Decryptor:
    """mkrlwe.Decryptor (decryptor.go:8-23) on the device; secret keys never leave it.  Between parties, decryption is ShareNew (each party, on
    its own key) and MergeShares (anyone): Decrypt needs every key in one place, and the output of PartialDecrypt gives the key away."""

    def __init__(self, params):
        self.params = params

    def _like(self, ct, ids):
        return Ciphertext(self.params, ids, ct.Level(), zero=False)

    @staticmethod
    def FloodBound(parties, flood_bits):
        """what a merge of `parties` shares with flood_bits bits adds to a coefficient, at most: parties * 2^(flood_bits - 1) (exact integer; 0 bits: 0)"""
        return 0 if flood_bits == 0 else int(parties) << (int(flood_bits) - 1)

    def ShareBatch(self, cts, sk, flood_bits, sampler):
        """The decryption shares of the party of `sk` for B ciphertexts at one level (their id sets may differ) as ONE engine call
        (mkhe_decrypt_share) -> one DecryptionShare of count B.  flood_bits = 1 .. 62: the width of the flooding noise, uniform on
        [-2^(bits-1), 2^(bits-1)), drawn on the device under one nonce of `sampler` (a DeviceSampler); it must exceed the noise of the ciphertext
        by the statistical security parameter, which the engine cannot know -- so there is no default (NoiseNorm / NoiseBits of the scheme's
        Decryptor measure that noise).  flood_bits = 0 (no noise, sampler
        unused) is for TESTS ONLY: such a share is PartialDecrypt's product and reveals sk."""
        cts = list(cts)
        if not cts:
            raise MkheError("Cannot ShareBatch: no ciphertext")
        level = cts[0].Level()
        for ct in cts:
            if sk.ID not in ct.ids:
                raise MkheError("Cannot Share: the ciphertext has no component for the id of sk")
            if ct.Level() != level:
                raise MkheError("Cannot Share: the ciphertexts of one call must be at the same level")
        if not isinstance(flood_bits, int) or not 0 <= flood_bits <= 62:
            raise MkheError("Cannot Share: flood_bits must be an integer 0 .. 62")
        key, nonce = None, 0
        if flood_bits > 0:
            if not isinstance(sampler, DeviceSampler):
                raise MkheError("Cannot Share: the flooding noise is drawn on the device -- pass a DeviceSampler")
            key, nonce = sampler.share_args()
        out = DecryptionShare(self.params, sk.ID, level, len(cts))
        slots = (C.c_int * len(cts))(*[ct.slot(sk.ID) for ct in cts])
        check(lib().mkhe_decrypt_share(self.params.ctx, len(cts), handle_array([ct.h for ct in cts]), slots, sk.Value.devptr(), key, nonce,
                                       flood_bits, out.Value.devptr()))
        return out

    def ShareNew(self, ct, sk, flood_bits, sampler):
        """ShareBatch of one ciphertext"""
        return self.ShareBatch([ct], sk, flood_bits, sampler)

    def MergeSharesBatch(self, cts, shares):
        """c_0 + the shares of ALL parties, for B ciphertexts over the same ids at one level -> DeviceLimbs [B][level+1][N], canonical,
        coefficient domain (what Decrypt gives, plus the sum of the flooding noises).  shares: one DecryptionShare of count B per party,
        in any order."""
        cts = list(cts)
        if not cts:
            raise MkheError("Cannot MergeShares: no ciphertext")
        for ct in cts:
            if ct.ids != cts[0].ids or ct.Level() != cts[0].Level():
                raise MkheError("Cannot MergeShares: the ciphertexts of one call must be over the same ids and at the same level")
        ordered = order_shares(cts[0].ids, cts[0].Level(), len(cts), shares)
        pt = DeviceLimbs(self.params, len(cts), cts[0].Level() + 1)
        check(lib().mkhe_decrypt_merge(self.params.ctx, len(cts), handle_array([ct.h for ct in cts]), len(ordered),
                                       handle_array([sh.Value.devptr() for sh in ordered]), pt.devptr()))
        return pt

    def MergeShares(self, ct, shares):
        """MergeSharesBatch of one ciphertext -> DeviceLimbs [1][level+1][N]"""
        return self.MergeSharesBatch([ct], shares)

    def FoldShares(self, shares):
        """The DecryptionShares that the t holders of ONE absent party's key made with their additive keys (Combiner.AdditiveKey; same id, level
        and count) -> one DecryptionShare of that id, their sum (mkhe_limbs_sum): what the party itself would have published, with t floods in
        the place of one.  MergeShares* then works unchanged.  A party covered by t holders contributes t floods: call FloodBound /
        FloodSlotBound with k - 1 + t in the place of k."""
        shares = list(shares)
        if not shares:
            raise MkheError("Cannot FoldShares: no share")
        first = shares[0]
        for sh in shares:
            if sh.ID != first.ID:
                raise MkheError("Cannot FoldShares: shares of the parties %r and %r (a fold is over the holders of ONE party's key)" % (first.ID, sh.ID))
            if sh.Level() != first.Level():
                raise MkheError("Cannot FoldShares: shares at the levels %d and %d" % (first.Level(), sh.Level()))
            if sh.count != first.count:
                raise MkheError("Cannot FoldShares: shares for %d and %d ciphertexts" % (first.count, sh.count))
        out = DecryptionShare(self.params, first.ID, first.Level(), first.count)
        check(lib().mkhe_limbs_sum(self.params.ctx, first.count, first.Level() + 1, len(shares),
                                   handle_array([sh.Value.devptr() for sh in shares]), out.Value.devptr()))
        return out

    def PartialDecrypt(self, ct, sk):
        """decryptor.go:26-43.  The Go version works in place and deletes ct.Value[sk.ID]; a device ciphertext keeps its shape, so the
        result is a NEW ciphertext over the remaining ids and `ct` is left as it was (the deviation Rescale already makes).
        WARNING: the result REVEALS sk to anyone who sees it (c_0 and c_id are public and c_id is invertible with overwhelming probability):
        it is for a process that holds every key, as in the reference's tests.  Between parties use ShareNew / MergeShares."""
        if sk.ID not in ct.ids:
            raise MkheError("Cannot PartialDecrypt: the ciphertext has no component for the id of sk")
        out = self._like(ct, [i for i in ct.ids if i != sk.ID])
        check(lib().mkhe_partial_decrypt(self.params.ctx, ct.h, ct.slot(sk.ID), sk.Value.devptr(), out.h))
        return out

    def Decrypt(self, ct, skSet):
        """decryptor.go:48-66 -> DeviceLimbs [1][level+1][N]: canonical residues, coefficient domain"""
        for i in ct.ids:
            if i not in skSet.Value:
                raise MkheError("Cannot Decrypt: there is a missing secretkey")               # decryptor.go:61-63
        pt = DeviceLimbs(self.params, 1, ct.Level() + 1)
        sks = [skSet.Value[i].Value.devptr() for i in ct.ids]
        check(lib().mkhe_decrypt(self.params.ctx, ct.h, handle_array(sks), pt.devptr()))
        return pt

    def NoiseNormBatch(self, phases, refs=None, kind=0):
        """The exact centred max norm of B phases as ONE engine call (mkhe_noise_norm; include/mkhe.h, "noise measurement") ->
        [(r, n)] per item: r = max_n min(x_n, Q - x_n) as a Python integer, Q the product of the first `limbs` moduli, and the smallest n that
        attains it.  phases: DeviceLimbs [B][limbs][N], canonical, coefficient domain -- what Decrypt gives, or MergeSharesBatch, so parties
        that hold only their own key can measure too (with flood_bits = 0 shares; otherwise the flood is measured with the noise).
        kind 0: x = phases - refs (refs: DeviceLimbs [B][limbs][N], or [1][limbs][N] for one reference for all; None: x = phases).
        kind 1 (BFV contexts, limbs = nQ, no refs): x = T * phases, the invariant noise.  Only the digits and n come down; the host
        multiplies the mixed-radix digits out."""
        if not isinstance(phases, DeviceLimbs):
            raise MkheError("Cannot NoiseNorm: the phases must be DeviceLimbs [count][limbs][N]")
        count, limbs, N = phases.count, phases.limbs, self.params.N()
        ref, stride = None, 0
        if refs is not None:
            if not isinstance(refs, DeviceLimbs) or refs.limbs != limbs or refs.count not in (1, count):
                raise MkheError("Cannot NoiseNorm: the references must be DeviceLimbs [count][limbs][N] or [1][limbs][N] with the limbs of the phases")
            ref, stride = refs.devptr(), (0 if refs.count == 1 else limbs * N)
        words = count * (limbs + 1)
        out = DeviceLimbs(self.params, -(-words // N), 1)
        check(lib().mkhe_noise_norm(self.params.ctx, int(kind), limbs, count, phases.devptr(), ref, stride, out.devptr()))
        rows = out.download().reshape(-1)[:words].reshape(count, limbs + 1)
        res = []
        for row in rows:
            r, w = 0, 1
            for d, q in zip(row[:limbs], self.params.Q):
                r, w = r + int(d) * w, w * int(q)
            res.append((r, int(row[limbs])))
        return res

    def NoiseNorm(self, ct, skSet, ref=None):
        """Decrypt, then NoiseNormBatch against `ref` (DeviceLimbs [1][level+1][N], or a host polynomial [level+1][N]: the plaintext the
        ciphertext is expected to hold) -> the largest coefficient of the residual, centred, as a Python integer: the noise of ct when ref is
        its plaintext.  Its bit_length() is the size that the flood_bits of ShareNew must exceed."""
        if ref is not None and not isinstance(ref, DeviceLimbs):
            ref = _device_plaintexts(self.params, np.asarray(ref, dtype=np.uint64)[None])
        return self.NoiseNormBatch(Decryptor.Decrypt(self, ct, skSet), ref)[0][0]


def NewDecryptor(params):
    return Decryptor(params)


# ---- collective refresh (include/mkhe.h, "collective refresh")
class RefreshShare:
    """What one party publishes in a collective refresh of `count` ciphertexts: .Share, a DecryptionShare at level_in that carries the MASKED
    products c_id * s_id + M, and .Reenc, `count` ciphertexts over the party's id alone at level_out that encrypt -M.  Both travel:
    download() gives (share array, [reenc arrays]), upload() takes them on the receiving side."""

    def __init__(self, params, id, level_in, level_out, count=1):
        self.ID, self.count, self._level_out = id, int(count), int(level_out)
        self.Share = DecryptionShare(params, id, level_in, count)
        self.Reenc = batch_ciphertexts(Ciphertext, params, [id], level_out, self.count)

    def Level(self):
        """the level of the ciphertexts the share was made for"""
        return self.Share.Level()

    def LevelOut(self):
        return self._level_out

    def download(self):
        return self.Share.download(), [c.download() for c in self.Reenc]

    def upload(self, host):
        share, reenc = host
        if len(reenc) != self.count:
            raise MkheError("RefreshShare: expected %d re-encryptions, got %d" % (self.count, len(reenc)))
        self.Share.upload(share)
        for c, h in zip(self.Reenc, reenc):
            c.upload(h)
        return self


class Refresher:
    """The collective refresh between parties: ShareNew (each party, on its own keys and its own DeviceSampler) and MergeNew (anyone) give a
    ciphertext of the same message over the same parties at level_out (default: the maximum level).  The caller chooses mask_bits
    (MaxMaskBits): mask_bits minus the bit size of the message is the statistical hiding it gets."""

    def __init__(self, params):
        self.params = params

    def _out(self, like, count, level_out):
        """the `count` outputs of a merge over the ids of `like`"""
        return batch_ciphertexts(Ciphertext, self.params, like.ids, level_out, count)

    @staticmethod
    def MaxMaskBits(q_product, parties, msg_bits):
        """the largest bits <= 120 with parties * 2^(bits-1) + 2^msg_bits <= (Q - 1) / 2: the lift of a merge cannot wrap.  Pure; raises when
        not even one bit fits."""
        q_product, parties, msg_bits = int(q_product), int(parties), int(msg_bits)
        if parties < 1 or msg_bits < 0:
            raise MkheError("MaxMaskBits: parties must be positive and msg_bits non-negative")
        room = (q_product - 1) // 2 - (1 << msg_bits)
        bits = 0
        while bits < 120 and (parties << bits) <= room:         # bits + 1 fits: parties * 2^((bits+1)-1) <= room
            bits += 1
        if bits == 0:
            raise MkheError("MaxMaskBits: no mask fits: %d parties and a message of %d bits leave no room below Q / 2" % (parties, msg_bits))
        return bits

    def ShareBatch(self, cts, sk, pk, mask_bits, sampler, level_out=None):
        """The refresh shares of the party of (sk, pk) for B ciphertexts at one level (their id sets may differ) as ONE engine call
        (mkhe_refresh_share) -> one RefreshShare of count B.  mask_bits = 1 .. 120; 0 (no mask) is for TESTS ONLY: such a share reveals sk.
        Two nonces of `sampler` (a DeviceSampler) serve the call: one for the mask, one for the encryption."""
        cts = list(cts)
        if not cts:
            raise MkheError("Cannot RefreshShare: no ciphertext")
        if sk.ID != pk.ID:
            raise MkheError("Cannot RefreshShare: sk and pk belong to different parties")
        level = cts[0].Level()
        level_out = self.params.MaxLevel() if level_out is None else int(level_out)
        if not 0 <= level_out <= self.params.MaxLevel():
            raise MkheError("Cannot RefreshShare: level_out %d out of range" % level_out)
        for ct in cts:
            if sk.ID not in ct.ids:
                raise MkheError("Cannot RefreshShare: the ciphertext has no component for the id of sk")
            if ct.Level() != level:
                raise MkheError("Cannot RefreshShare: the ciphertexts of one call must be at the same level")
        if not isinstance(mask_bits, int) or not 0 <= mask_bits <= 120:
            raise MkheError("Cannot RefreshShare: mask_bits must be an integer 0 .. 120")
        if not isinstance(sampler, DeviceSampler):
            raise MkheError("Cannot RefreshShare: mask and encryption samples are drawn on the device -- pass a DeviceSampler")
        key, nonce_mask, nonce_enc = sampler.refresh_args()
        out = RefreshShare(self.params, sk.ID, level, level_out, len(cts))
        slots = (C.c_int * len(cts))(*[ct.slot(sk.ID) for ct in cts])
        check(lib().mkhe_refresh_share(self.params.ctx, len(cts), handle_array([ct.h for ct in cts]), slots, sk.Value.devptr(), pk.Value.devptr(),
                                       key, nonce_mask, nonce_enc, mask_bits, sampler._cdt, len(sampler.cdt), out.Share.Value.devptr(),
                                       handle_array([c.h for c in out.Reenc])))
        return out

    def ShareNew(self, ct, sk, pk, mask_bits, sampler, level_out=None):
        """ShareBatch of one ciphertext"""
        return self.ShareBatch([ct], sk, pk, mask_bits, sampler, level_out)

    def MergeBatch(self, cts, shares):
        """The refreshed ciphertexts of B ciphertexts over the same ids at one level: one RefreshShare of count B per party, in any order
        (ordering and errors: order_shares) -> B ciphertexts over the same ids at the shares' level_out.  ONE engine call (mkhe_refresh_merge)."""
        cts = list(cts)
        if not cts:
            raise MkheError("Cannot RefreshMerge: no ciphertext")
        for ct in cts:
            if ct.ids != cts[0].ids or ct.Level() != cts[0].Level():
                raise MkheError("Cannot RefreshMerge: the ciphertexts of one call must be over the same ids and at the same level")
        ordered = order_shares(cts[0].ids, cts[0].Level(), len(cts), shares)
        levels = {sh.LevelOut() for sh in ordered}
        if len(levels) > 1:
            raise MkheError("Cannot RefreshMerge: the shares are for different output levels %r" % sorted(levels))
        level_out = levels.pop() if levels else self.params.MaxLevel()
        outs = self._out(cts[0], len(cts), level_out)
        reenc = [c.h for sh in ordered for c in sh.Reenc]
        check(lib().mkhe_refresh_merge(self.params.ctx, len(cts), handle_array([ct.h for ct in cts]), len(ordered),
                                       handle_array([sh.Share.Value.devptr() for sh in ordered]), handle_array(reenc) if reenc else None,
                                       handle_array([c.h for c in outs])))
        return outs

    def MergeNew(self, ct, shares):
        """MergeBatch of one ciphertext -> the refreshed ciphertext"""
        return self.MergeBatch([ct], shares)[0]


def NewRefresher(params):
    return Refresher(params)


# ---- encryption to shares and back (include/mkhe.h, "encryption to shares")
class SecretShare:
    """An ADDITIVE share of the plaintexts of `count` ciphertexts: a device buffer uint64 [count][limbs][N] plus the id of the party that holds
    it (None: the public share, which anyone can compute), the level (None where the share is over Z_T: mkbfv) and the count.  A party's share
    is as secret as its mask: it travels to nobody.  download() / upload() move it between the device and its owner's host; wipe() overwrites
    the device buffer with zeros and then frees it."""

    def __init__(self, params, id, level, count=1, limbs=None):
        self.params, self.ID, self.count = params, id, int(count)
        self._level = None if level is None else int(level)
        self.Value = DeviceLimbs(params, self.count, int(limbs) if limbs is not None else self._level + 1)

    def Level(self):
        return self._level

    def download(self):
        return self.Value.download()

    def upload(self, host):
        self.Value.upload(host)
        return self

    def wipe(self):
        v = self.Value
        if v is not None and v.d:
            v.upload(np.zeros((v.count, v.limbs, self.params.N()), dtype=np.uint64))
            lib().mkhe_buf_free(self.params.ctx, v.d)
            v.d = None
        self.Value = None


class ShareConverter:
    """HE <-> additive secret sharing between parties, exact over R_Q in the coefficient domain.  E2S: every party runs E2SShareBatch on its own
    key and DeviceSampler, publishes the DecryptionShare and KEEPS the SecretShare; anyone runs E2SMergeBatch on the published shares, which
    gives the public share.  public + the sum of the secret shares is the plaintext of Decrypt modulo every prime of the input level, whatever
    mask_bits is; nobody has seen it.  S2E: the party that holds the public share folds it into its own (FoldPublic: mkhe_limbs_sum) BEFORE it
    encrypts -- a plaintext cannot be added behind the merge without an operation the ring has none of here; every party encrypts its share
    under its own public key (S2EShareBatch), and S2EMergeNew is the AddNew chain over the parties' ciphertexts.  With the nonces of a
    Refresher.ShareNew (e2s_args then encrypt_args take the two counter values refresh_args takes) the result is Refresher.MergeNew's, bit for bit."""

    def __init__(self, params):
        self.params = params

    MaxMaskBits = staticmethod(Refresher.MaxMaskBits)

    def _new(self, ids, level, count, like=None):
        """`count` output ciphertexts over ids at level"""
        return batch_ciphertexts(Ciphertext, self.params, ids, level, count)

    def _level_out(self, level_out, who):
        level_out = self.params.MaxLevel() if level_out is None else int(level_out)
        if not 0 <= level_out <= self.params.MaxLevel():
            raise MkheError("Cannot %s: level_out %d out of range" % (who, level_out))
        return level_out

    def E2SShareBatch(self, cts, sk, mask_bits, sampler, level_out=None):
        """The party of sk, for B ciphertexts at one level (their id sets may differ), as ONE engine call (mkhe_e2s_share) -> (DecryptionShare
        to publish: Refresher.ShareBatch's, bit for bit; SecretShare to keep: -M under the level_out + 1 first moduli, default the maximum
        level).  mask_bits = 1 .. 120 (MaxMaskBits); 0 (no mask) is for TESTS ONLY: such a share reveals sk.  One nonce of `sampler`."""
        cts = list(cts)
        if not cts:
            raise MkheError("Cannot E2SShare: no ciphertext")
        level = cts[0].Level()
        level_out = self._level_out(level_out, "E2SShare")
        for ct in cts:
            if sk.ID not in ct.ids:
                raise MkheError("Cannot E2SShare: the ciphertext has no component for the id of sk")
            if ct.Level() != level:
                raise MkheError("Cannot E2SShare: the ciphertexts of one call must be at the same level")
        if not isinstance(mask_bits, int) or not 0 <= mask_bits <= 120:
            raise MkheError("Cannot E2SShare: mask_bits must be an integer 0 .. 120")
        if not isinstance(sampler, DeviceSampler):
            raise MkheError("Cannot E2SShare: the mask is drawn on the device -- pass a DeviceSampler")
        key, nonce = sampler.e2s_args()
        pub = DecryptionShare(self.params, sk.ID, level, len(cts))
        sec = SecretShare(self.params, sk.ID, level_out, len(cts))
        slots = (C.c_int * len(cts))(*[ct.slot(sk.ID) for ct in cts])
        check(lib().mkhe_e2s_share(self.params.ctx, len(cts), handle_array([ct.h for ct in cts]), slots, sk.Value.devptr(), key, nonce, mask_bits,
                                   pub.Value.devptr(), level_out + 1, sec.Value.devptr()))
        return pub, sec

    def E2SMergeBatch(self, cts, shares, level_out=None):
        """Anyone, for B ciphertexts over the same ids at one level and one DecryptionShare of count B per party, in any order -> the public
        additive share, a SecretShare with id None at level_out: the exact centred lift of c_0 + the shares.  ONE engine call (mkhe_e2s_merge)."""
        cts = list(cts)
        if not cts:
            raise MkheError("Cannot E2SMerge: no ciphertext")
        for ct in cts:
            if ct.ids != cts[0].ids or ct.Level() != cts[0].Level():
                raise MkheError("Cannot E2SMerge: the ciphertexts of one call must be over the same ids and at the same level")
        level_out = self._level_out(level_out, "E2SMerge")
        ordered = order_shares(cts[0].ids, cts[0].Level(), len(cts), shares)
        out = SecretShare(self.params, None, level_out, len(cts))
        check(lib().mkhe_e2s_merge(self.params.ctx, len(cts), handle_array([ct.h for ct in cts]), len(ordered),
                                   handle_array([sh.Value.devptr() for sh in ordered]), level_out + 1, out.Value.devptr()))
        return out

    def FoldPublic(self, secret, public):
        """the share of the party that holds the public share, with the public share added in (mkhe_limbs_sum) -> a new SecretShare of that party"""
        if secret.count != public.count or secret.Value.limbs != public.Value.limbs:
            raise MkheError("Cannot FoldPublic: the shares differ in count or level")
        out = SecretShare(self.params, secret.ID, secret.Level(), secret.count, secret.Value.limbs)
        check(lib().mkhe_limbs_sum(self.params.ctx, secret.count, secret.Value.limbs, 2,
                                   handle_array([secret.Value.devptr(), public.Value.devptr()]), out.Value.devptr()))
        return out

    def S2EShareBatch(self, secret, pk, sampler):
        """The party of pk encrypts its SecretShare as a plaintext under its own public key -> `count` ciphertexts over the party's id at the
        share's level.  mkhe_encrypt_seeded with a DeviceSampler (one nonce), mkhe_encrypt with a host sampler: nothing new in the engine."""
        if secret.ID is not None and secret.ID != pk.ID:
            raise MkheError("Cannot S2EShare: the share and pk belong to different parties")
        enc = Encryptor(self.params, sampler)
        level = secret.Value.limbs - 1
        outs = self._new([pk.ID], level, secret.count, like=secret)
        enc._engine_encrypt(level, pk, secret.Value, False, enc._draw(None, secret.count), outs)
        return outs

    def S2EMergeNew(self, cts_by_party, public=None):
        """The AddNew chain over the parties' ciphertexts (one each, from S2EShareBatch) -> one ciphertext over all their ids.  public must be
        None: the public share is not an argument of the merge -- its holder folds it into its own share (FoldPublic) before S2EShareBatch."""
        if public is not None:
            raise MkheError("Cannot S2EMerge: the public share is folded into its holder's share (FoldPublic) before that party encrypts")
        cts = list(cts_by_party)
        if not cts:
            raise MkheError("Cannot S2EMerge: no ciphertext")
        acc = cts[0]
        for ct in cts[1:]:
            if ct.Level() != acc.Level():
                raise MkheError("Cannot S2EMerge: the ciphertexts must be at the same level")
            out = self._new(sorted(set(acc.ids) | set(ct.ids)), acc.Level(), 1, like=acc)[0]
            check(lib().mkhe_ct_add(self.params.ctx, acc.h, ct.h, out.h))
            acc = out
        return acc


def NewShareConverter(params):
    return ShareConverter(params)


# ---- collective public-key switch (include/mkhe.h, "collective public-key switch")
class PublicKeySwitchShare:
    """What one party publishes in a collective key switch of `count` ciphertexts at `level` to a recipient's public key: the pairs (h0, h1),
    uint64 [count][2][level+1][N] on the device.  Shares travel between parties: download() gives the host array, upload() takes it on the
    receiving side (PublicKeySwitchShare(params, id, level, count).upload(host))."""

    def __init__(self, params, id, level, count=1):
        self.ID, self._level, self.count = id, int(level), int(count)
        self.Value = DeviceLimbs(params, 2 * self.count, self._level + 1)

    def Level(self):
        return self._level

    def download(self):
        h = self.Value.download()
        return h.reshape(self.count, 2, h.shape[1], h.shape[2])

    def upload(self, host):
        host = np.ascontiguousarray(host, dtype=np.uint64)
        if host.ndim != 4 or host.shape[:2] != (self.count, 2):
            raise MkheError("PublicKeySwitchShare: expected an array of shape [%d][2][limbs][N], got %r" % (self.count, host.shape))
        self.Value.upload(host.reshape(2 * self.count, host.shape[2], host.shape[3]))
        return self


class PublicKeySwitcher:
    """The collective key switch to a recipient's public key between parties: ShareNew (each party, on its own secret key, the RECIPIENT's public
    key and its own DeviceSampler) and MergeNew (anyone) give an ordinary ciphertext of the same message over the recipient's id alone, which the
    recipient decrypts with Decrypt on its own key or goes on computing with.  Nobody else learns the message; the recipient need not be online
    and need not be one of the parties.  The caller chooses flood_bits (at most MaxFloodBits): flood_bits minus the bit size of the ciphertext's
    noise is the statistical hiding of that noise.  The engine cannot check whose key pk_recipient is."""

    def __init__(self, params):
        self.params = params

    def _t(self):
        """T' of the flood bound: the plaintext modulus of a BFV ring, 1 otherwise"""
        return 1

    def _out(self, like, count, recipient_id):
        """the `count` outputs of a merge: ciphertexts over [recipient_id] at the level of `like`"""
        return batch_ciphertexts(Ciphertext, self.params, [recipient_id], like.Level(), count)

    @staticmethod
    def NoiseBound(parties, flood_bits, N, bound=19):
        """what a switch adds to a coefficient of the phase, at most: parties * (2^(flood_bits - 1) + 2 N bound) (exact integer).  Under the
        recipient's secret the result decrypts to the phase of the input plus sum_i (u_i e_R + E_i + e1_i s_R): u_i and s_R ternary, e_R and
        e1_i truncated at `bound` (floor(6 sigma): 19 at sigma 3.2), E_i in [-2^(flood_bits-1), 2^(flood_bits-1))."""
        flood = 0 if int(flood_bits) == 0 else 1 << (int(flood_bits) - 1)
        return int(parties) * (flood + 2 * int(N) * int(bound))

    def MaxFloodBits(self, level=None):
        """the widest flood the engine takes for ciphertexts at `level` (default: the maximum): bitlen(Q_l div 2T') - 1, capped at the 1024
        bits the engine draws; T' = T on a BFV ring, 1 otherwise.  Such a flood alone would still leave the message standing; what the noise of
        the ciphertext (NoiseNorm / NoiseBits of the scheme's Decryptor) and the number of parties leave of it is the caller's budget (NoiseBound)."""
        return self._most(self.params.MaxLevel() if level is None else int(level))

    def _most(self, level):
        q = 1
        for m in self.params.Q[: level + 1]:
            q *= int(m)
        return min(1024, (q // (2 * self._t())).bit_length() - 1)

    def ShareBatch(self, cts, sk, pk_recipient, flood_bits, sampler):
        """The key-switch shares of the party of `sk` for B ciphertexts at one level (their id sets may differ) as ONE engine call
        (mkhe_pcks_share) -> one PublicKeySwitchShare of count B whose .ID is sk.ID.  One nonce of `sampler` (a DeviceSampler) serves the call.
        flood_bits = 0 (no flood) is for TESTS ONLY: such a share gives sk away."""
        cts = list(cts)
        if not cts:
            raise MkheError("Cannot SwitchShare: no ciphertext")
        level = cts[0].Level()
        for ct in cts:
            if sk.ID not in ct.ids:
                raise MkheError("Cannot SwitchShare: the ciphertext has no component for the id of sk")
            if ct.Level() != level:
                raise MkheError("Cannot SwitchShare: the ciphertexts of one call must be at the same level")
        if not isinstance(flood_bits, int) or not 0 <= flood_bits <= self._most(level):
            raise MkheError("Cannot SwitchShare: flood_bits must be an integer 0 .. %d" % self._most(level))
        if not isinstance(sampler, DeviceSampler):
            raise MkheError("Cannot SwitchShare: u, e1 and the flood are drawn on the device -- pass a DeviceSampler")
        key, nonce, cdt, ncdt = sampler.switch_args()
        out = PublicKeySwitchShare(self.params, sk.ID, level, len(cts))
        slots = (C.c_int * len(cts))(*[ct.slot(sk.ID) for ct in cts])
        check(lib().mkhe_pcks_share(self.params.ctx, len(cts), handle_array([ct.h for ct in cts]), slots, sk.Value.devptr(), pk_recipient.Value.devptr(),
                                    key, nonce, flood_bits, cdt, ncdt, out.Value.devptr()))
        return out

    def ShareNew(self, ct, sk, pk_recipient, flood_bits, sampler):
        """ShareBatch of one ciphertext"""
        return self.ShareBatch([ct], sk, pk_recipient, flood_bits, sampler)

    def MergeBatch(self, cts, shares, recipient_id):
        """The switched ciphertexts of B ciphertexts over the same ids at one level: one PublicKeySwitchShare of count B per party, in any order
        (ordering and errors: order_shares) -> B ciphertexts over [recipient_id] at the same level.  ONE engine call (mkhe_pcks_merge)."""
        cts = list(cts)
        if not cts:
            raise MkheError("Cannot SwitchMerge: no ciphertext")
        for ct in cts:
            if ct.ids != cts[0].ids or ct.Level() != cts[0].Level():
                raise MkheError("Cannot SwitchMerge: the ciphertexts of one call must be over the same ids and at the same level")
        ordered = order_shares(cts[0].ids, cts[0].Level(), len(cts), shares)
        outs = self._out(cts[0], len(cts), recipient_id)
        check(lib().mkhe_pcks_merge(self.params.ctx, len(cts), handle_array([ct.h for ct in cts]), len(ordered),
                                    handle_array([sh.Value.devptr() for sh in ordered]) if ordered else None, handle_array([c.h for c in outs])))
        return outs

    def MergeNew(self, ct, shares, recipient_id):
        """MergeBatch of one ciphertext -> the ciphertext over [recipient_id]"""
        return self.MergeBatch([ct], shares, recipient_id)[0]


def NewPublicKeySwitcher(params):
    return PublicKeySwitcher(params)


# ---- threshold secret keys (include/mkhe.h, "threshold secret keys")
def _points(points, who):
    """holder points -> (uint32 * n); the engine checks them against the moduli"""
    xs = [int(x) for x in points]
    if not 1 <= len(xs) <= 32 or any(not 1 <= x < (1 << 32) for x in xs) or len(set(xs)) != len(xs):
        raise MkheError("%s: 1 .. 32 pairwise distinct points, each 1 .. 2^32 - 1" % who)
    return (C.c_uint32 * len(xs))(*xs)


class SecretKeyShare:
    """The Shamir share of the secret key of party `id` that `holder` keeps, at the public point `point`, under a t-of-n sharing with t =
    `threshold`: Value = uint64 [1][nQ+nP][N] on the device, in the representation of SecretKey.Value.  Fewer than t shares say nothing about the
    key, but the t shares of an active set together ARE the key: a share is key material and travels only to its holder, over a private channel
    (download() gives the host array, SecretKeyShare(params, id, holder, point, threshold).upload(host) takes it on the receiving side)."""

    def __init__(self, params, id, holder, point, threshold):
        self.ID, self.Holder, self.Point, self.Threshold = id, holder, int(point), int(threshold)
        self.Value = DeviceLimbs(params, 1, params.QCount() + params.PCount())

    def download(self):
        return self.Value.download()

    def upload(self, host):
        self.Value.upload(host)
        return self


class Thresholdizer:
    """The party side of t-out-of-n thresholdisation (lattigo's drlwe.Thresholdizer): Shamir-shares a secret key among n holders."""

    def __init__(self, params):
        self.params = params

    def GenShares(self, sk, threshold, points, sampler):
        """{holder: SecretKeyShare} for points = {holder: x}, 1 <= threshold <= len(points) <= 32, as ONE engine call
        (mkhe_threshold_gen_shares).  The coefficient polynomials are drawn on the device under one nonce of `sampler` (a DeviceSampler) and
        exist in registers only.  threshold = 1 hands every holder the key itself (TESTS ONLY)."""
        if not isinstance(sampler, DeviceSampler):
            raise MkheError("Cannot GenShares: the coefficient polynomials are drawn on the device -- pass a DeviceSampler")
        holders = list(points)
        xs = _points([points[h] for h in holders], "Cannot GenShares")
        if not isinstance(threshold, int) or not 1 <= threshold <= len(holders):
            raise MkheError("Cannot GenShares: threshold must be an integer 1 .. %d" % len(holders))
        out = {h: SecretKeyShare(self.params, sk.ID, h, points[h], threshold) for h in holders}
        key, nonce = sampler.threshold_args()
        check(lib().mkhe_threshold_gen_shares(self.params.ctx, sk.Value.devptr(), threshold, len(holders), xs, key, nonce,
                                              handle_array([out[h].Value.devptr() for h in holders])))
        return out


class Combiner:
    """The holder side (lattigo's drlwe.Combiner): from a Shamir share to the additive key for one active set."""

    def __init__(self, params):
        self.params = params

    def AdditiveKey(self, share, active_points):
        """share (a SecretKeyShare) times its Lagrange coefficient for the active set `active_points` (the points of at least t holders, share.Point
        among them; a dict {holder: x} or a list) -> a SecretKey with ID = share.ID, as ONE engine call (mkhe_threshold_additive_key).  The additive
        keys of the active set sum to the key of party share.ID, so Decryptor.ShareBatch, Refresher.ShareBatch and PublicKeySwitcher.ShareBatch take
        it unchanged and the holders' outputs add up to that party's share (Decryptor.FoldShares).  It is key material of the same rank as a key,
        and a share made from it must be FLOODED exactly like one made from a key."""
        xs = list(active_points.values()) if isinstance(active_points, dict) else list(active_points)
        arr = _points(xs, "Cannot AdditiveKey")
        if [int(x) for x in xs].count(share.Point) != 1:
            raise MkheError("Cannot AdditiveKey: the point of the share must be one of the active points")
        out = SecretKey(self.params, share.ID)
        check(lib().mkhe_threshold_additive_key(self.params.ctx, share.Value.devptr(), share.Point, len(xs), arr, out.Value.devptr()))
        return out

    def Reconstruct(self, keys):
        """the sum of the additive keys of ONE active set (mkhe_limbs_sum over the nQ+nP rows) -> the SecretKey of their party.  For tests and key
        recovery: in the protocols the additive keys never meet."""
        keys = list(keys)
        if not keys:
            raise MkheError("Cannot Reconstruct: no key")
        if any(k.ID != keys[0].ID for k in keys):
            raise MkheError("Cannot Reconstruct: additive keys of different parties")
        out = SecretKey(self.params, keys[0].ID)
        check(lib().mkhe_limbs_sum(self.params.ctx, 1, self.params.QCount() + self.params.PCount(), len(keys),
                                   handle_array([k.Value.devptr() for k in keys]), out.Value.devptr()))
        return out


def NewThresholdizer(params):
    return Thresholdizer(params)


def NewCombiner(params):
    return Combiner(params)
