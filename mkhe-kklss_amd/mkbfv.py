"""Host-side mirror of the reference package `mkbfv` (Evaluator hot methods).

Same names and argument meaning as mkbfv/{params,keys,elements,evaluator,basis_extension}.go; all
polynomial work runs on the device through the C ABI (include/mkhe.h, mkhe_bfv_* and mkhe_ct_*).
BFV ciphertexts live at the maximum level in the coefficient domain (elements.go:9-11).
"""
import collections
import ctypes as C
import functools
import math

import numpy as np

from . import _abi, mkrlwe
from ._abi import MkheError, check, handle_array, lib
from .mkckks import PTXT_DOT_MAX_GIANT, linear_transform_plan, poly_eval_plan


class Parameters(mkrlwe.Parameters):
    """mkbfv.Parameters (params.go:21-76): mkrlwe parameters over (Q, P) with gamma = 2, plus ring QMul,
    ring R = Q || QMul and the plaintext modulus T."""

    def __init__(self, logN, Q, QMul, P, T, device=0):
        if len(Q) != len(QMul):
            raise MkheError("cannot NewParametersFromLiteral: length of Q & QMul is not equal")     # params.go:30-32
        self.QMul = [int(q) for q in QMul]
        self._T = int(T)
        super().__init__(logN, Q, P, gamma=2, device=device)

    def _create_context(self, psiQ, psiP):
        q = np.asarray(self.Q, dtype=np.uint64)
        qm = np.asarray(self.QMul, dtype=np.uint64)
        p = np.asarray(self.P, dtype=np.uint64)
        h = C.c_void_p()
        check(lib().mkhe_ctx_create_bfv(C.byref(h), self.logN, q.ctypes.data_as(_abi.u64p), qm.ctypes.data_as(_abi.u64p),
                                        len(self.Q), p.ctypes.data_as(_abi.u64p), len(self.P), self.gamma,
                                        self._T, self.device))
        return h

    def T(self): return self._T
    def RCount(self): return 2 * len(self.Q)

    def slot_psi(self):
        """the primitive 2N-th root of unity mod T of the slot definition (include/mkhe.h, "BFV batch encoder"): slot i is m(psi^(5^i)),
        slot N/2 + i is m(psi^(-5^i))"""
        return slot_psi(self._T, self.N())


class Ciphertext(mkrlwe.Ciphertext):
    """mkbfv.Ciphertext (elements.go:5-11): always at params.MaxLevel()."""

    def __init__(self, params, idset, zero=True):
        super().__init__(params, idset, params.MaxLevel(), zero)


def NewCiphertext(params, idset, zero=True):
    return Ciphertext(params, idset, zero)


class RelinearizationKey:
    """mkbfv.RelinearizationKey (keys.go:6-9,23-31): Value[0], Value[1] = two mkrlwe relinearization keys
    (b1, d1, v) and (b2, d2, -) for the Q resp. QMul gadget (keygen.go:41-83)."""

    def __init__(self, params, id, b1=None, b2=None, d1=None, d2=None, v=None):
        self.ID = id
        self.Value = [mkrlwe.RelinearizationKey(params, id, b1, d1, v), mkrlwe.RelinearizationKey(params, id, b2, d2, None)]


class RelinearizationKeySet:
    """keys.go:11-21,33-82.  PolyRPool / HoistPool of the reference are engine-internal device buffers."""

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


def NewRelinearizationKeyKeySet(params):
    return RelinearizationKeySet(params)


class KeyGenerator(mkrlwe.KeyGenerator):
    """mkbfv.KeyGenerator (mkbfv/keygen.go:9-21): the mkrlwe generator plus the BFV relinearization key."""

    def gadget(self, which):
        """residues [beta][nQ+nP] of the big-integer gadget scalars Gi of GenBFVSwitchingKey (keygen.go:104-116 for the
        Q digits, which = 0; :137-149 for the QMul digits, which = 1)"""
        params = self.params
        Q, QMul, P = math.prod(params.Q), math.prod(params.QMul), math.prod(params.P)
        moduli = params.Q if which == 0 else params.QMul
        alpha, beta = params.Alpha(), params.Beta(params.MaxLevel())
        g = np.zeros((beta, params.QCount() + params.PCount()), dtype=np.uint64)
        for i in range(beta):
            Qi = math.prod(moduli[i * alpha:(i + 1) * alpha])
            Gi = (Q * QMul) // Qi
            Ti = pow(Gi % Qi, -1, Qi)
            Gi = (Gi * params.T() * Ti * P) // QMul
            g[i] = [Gi % m for m in params.Q + params.P]
        return g

    def GenBFVSwitchingKey(self, sk, swk1, swk2, e=None):
        """keygen.go:91-162; e: [2][beta][N]"""
        a, ptr = self._errors(e, (2, self._beta()))
        for which, swk in enumerate((swk1, swk2)):
            g = self.gadget(which)
            check(lib().mkhe_bfv_keygen_switching_key(self.params.ctx, sk.Value.devptr(), g.ctypes.data_as(_abi.u64p),
                                                      a[which].ctypes.data_as(_abi.s32p), swk.h))

    def GenRelinearizationKey(self, sk, r, e=None):
        """mkbfv/keygen.go:24-88; e: [5][beta][N] for b1, b2, d1, d2, v"""
        params = self.params
        a, ptr = self._errors(e, (5, self._beta()))
        rlk = RelinearizationKey(params, sk.ID)
        g1, g2 = self.gadget(0), self.gadget(1)
        V = rlk.Value
        check(lib().mkhe_bfv_keygen_relin_key(params.ctx, sk.Value.devptr(), r.Value.devptr(), g1.ctypes.data_as(_abi.u64p),
                                              g2.ctypes.data_as(_abi.u64p), ptr, params.CRS[0].h, params.CRS[-3].h, params.CRS[-1].h,
                                              V[0].Value[0].h, V[1].Value[0].h, V[0].Value[1].h, V[1].Value[1].h, V[0].Value[2].h))
        return rlk


def NewKeyGenerator(params, sampler=None):
    return KeyGenerator(params, sampler)


class PolyR(mkrlwe.DeviceLimbs):
    """`count` polynomials over ring R (uint64[count][2nQ][N]) resident on the device."""

    def __init__(self, params, count=1):
        super().__init__(params, count, params.RCount())


class FastBasisExtender:
    """mkbfv.FastBasisExtender (basis_extension.go:7-47) on device buffers."""

    def __init__(self, params):
        self.params = params

    def ModUpQtoR(self, polyQ, polyR):
        """basis_extension.go:49-64; polyQ: DeviceLimbs [count][nQ][N], polyR: PolyR"""
        check(lib().mkhe_bfv_modup_q_to_r(self.params.ctx, polyQ.devptr(), polyR.devptr(), polyQ.count))

    def Rescale(self, polyQ, polyR):
        """basis_extension.go:82-96"""
        check(lib().mkhe_bfv_rescale(self.params.ctx, polyQ.devptr(), polyR.devptr(), polyQ.count))

    def Quantize(self, polyR, polyQ, t=None):
        """basis_extension.go:66-80; polyR in the NTT domain; t must be params.T()"""
        if t is not None and int(t) != self.params.T():
            raise MkheError("mkhe: Quantize scalar must be the context's plaintext modulus")
        check(lib().mkhe_bfv_quantize(self.params.ctx, polyR.devptr(), polyQ.devptr(), polyR.count))


class KeySwitcher(mkrlwe.KeySwitcher):
    """mkbfv.KeySwitcher (keyswitch.go:7-65): the mkrlwe key switcher over (Q, P) plus the BFV gadget calls."""

    def DecomposeBFV(self, polyR, ad1, ad2, index=0):
        """keyswitch.go:67-90: polynomial `index` of a PolyR buffer -> (ad1, ad2)"""
        off = index * polyR.limbs * self.Parameters.N() * 8
        check(lib().mkhe_bfv_decompose(self.ctx, C.c_void_p(polyR.devptr().value + off), ad1.h, ad2.h))

    def ExternalProductBFV(self, polyR, bg1, bg2, c, index=0):
        """keyswitch.go:83-113 (non-hoisted: the decomposition happens inside); polynomial `index` of a PolyR buffer;
        c: DeviceLimbs [1][nQ][N]"""
        off = index * polyR.limbs * self.Parameters.N() * 8
        check(lib().mkhe_bfv_external_product(self.ctx, C.c_void_p(polyR.devptr().value + off), bg1.h, bg2.h, c.devptr()))

    def ExternalProductBFVHoisted(self, aHoisted1, aHoisted2, bg1, bg2, c):
        """keyswitch_hoisted.go:6-34; c: DeviceLimbs [1][nQ][N]"""
        check(lib().mkhe_bfv_external_product_hoisted(self.ctx, aHoisted1.h, aHoisted2.h, bg1.h, bg2.h, c.devptr()))


def NewKeySwitcher(params):
    return KeySwitcher(params)


class Evaluator:
    """mkbfv.Evaluator (evaluator.go:7-20)."""

    def __init__(self, params):
        self.params = params
        self.ksw = KeySwitcher(params)
        self.conv = FastBasisExtender(params)

    def newCiphertextBinary(self, op0, op1):
        """evaluator.go:22-25"""
        return NewCiphertext(self.params, op0.IDSet() | op1.IDSet())

    def AddNew(self, op0, op1):
        """evaluator.go:44-52"""
        ctOut = self.newCiphertextBinary(op0, op1)
        check(lib().mkhe_ct_add(self.params.ctx, op0.h, op1.h, ctOut.h))
        return ctOut

    def SubNew(self, op0, op1):
        """evaluator.go:54-76"""
        ctOut = self.newCiphertextBinary(op0, op1)
        check(lib().mkhe_ct_sub(self.params.ctx, op0.h, op1.h, ctOut.h))
        return ctOut

    def mulRelin(self, op0, op1, rlkSet):
        """evaluator.go:95-113 -> KeySwitcher.MulAndRelinBFV (keyswitch.go:115-251): the non-hoisted twin of mulRelinHoisted, on its
        own device path (mkhe_bfv_mul_relin_unhoisted: the reference's order and pool discipline, every party component decomposed
        twice into one pair of pool vectors); the same ciphertext bit for bit."""
        return self.MulRelinNew(op0, op1, rlkSet, hoisted=False)

    def MulRelinNew(self, op0, op1, rlkSet, hoisted=True):
        """evaluator.go:78-82 -> mulRelinHoisted (:118-140)"""
        params = self.params
        if -1 not in params.CRS:
            raise MkheError("mkhe: CRS[-1] (u) has not been uploaded")
        ctOut = NewCiphertext(params, op0.IDSet() | op1.IDSet(), zero=False)        # every limb is written by the engine
        k0 = [rlkSet.GetRelinearizationKey(i) for i in op0.ids]
        k1 = [rlkSet.GetRelinearizationKey(i) for i in op1.ids]
        b1 = [k.Value[0].Value[0].h for k in k1]
        b2 = [k.Value[1].Value[0].h for k in k1]
        d1 = [k.Value[0].Value[1].h for k in k0]
        d2 = [k.Value[1].Value[1].h for k in k0]
        v = [k.Value[0].Value[2].h for k in k0]
        fn = lib().mkhe_bfv_mul_relin if hoisted else lib().mkhe_bfv_mul_relin_unhoisted
        check(fn(params.ctx, op0.h, op1.h, handle_array(b1), handle_array(b2), handle_array(d1),
                 handle_array(d2), handle_array(v), params.CRS[-1].h, ctOut.h))
        return ctOut

    def MulRelinSumNew(self, ops0, ops1, rlkSet):
        """sum_k MulRelin(ops0[k], ops1[k]) under ONE Quantize and ONE relinearisation tail (no reference counterpart; mkhe_bfv_mul_relin_sum,
        DESIGN.md 4.5j): an encrypted inner product mod T.  Every ops0[k] carries the ids of ops0[0], every ops1[k] those of ops1[0]; 1 to 16
        pairs.  Another ciphertext of the same sum than the chain of MulRelinNew and AddNew: one rounding and one gadget noise of step F2."""
        ops0, ops1 = list(ops0), list(ops1)
        if len(ops0) != len(ops1) or not ops0:
            raise MkheError("MulRelinSumNew: as many first operands as second ones, at least one pair")
        if len(ops0) > MULRELIN_SUM_MAX:
            raise MkheError("MulRelinSumNew: at most %d pairs per call" % MULRELIN_SUM_MAX)
        params = self.params
        if -1 not in params.CRS:
            raise MkheError("mkhe: CRS[-1] (u) has not been uploaded")
        ctOut = NewCiphertext(params, ops0[0].IDSet() | ops1[0].IDSet(), zero=False)      # every limb is written by the engine
        k0 = [rlkSet.GetRelinearizationKey(i) for i in ops0[0].ids]
        k1 = [rlkSet.GetRelinearizationKey(i) for i in ops1[0].ids]
        b1 = [k.Value[0].Value[0].h for k in k1]
        b2 = [k.Value[1].Value[0].h for k in k1]
        d1 = [k.Value[0].Value[1].h for k in k0]
        d2 = [k.Value[1].Value[1].h for k in k0]
        v = [k.Value[0].Value[2].h for k in k0]
        check(lib().mkhe_bfv_mul_relin_sum(params.ctx, len(ops0), handle_array([c.h for c in ops0]), handle_array([c.h for c in ops1]),
                                           handle_array(b1), handle_array(b2), handle_array(d1), handle_array(d2), handle_array(v),
                                           params.CRS[-1].h, ctOut.h))
        return ctOut

    def RotateNew(self, ct0, rotidx, rkSet):
        """evaluator.go:142-180"""
        n2 = self.params.N() // 2
        rotidx %= n2
        ctOut = NewCiphertext(self.params, ct0.IDSet())
        if rotidx == 0:
            check(lib().mkhe_ct_copy(self.params.ctx, ct0.h, ctOut.h))
            return ctOut
        if rotidx in self.params.CRS:
            self.ksw.Rotate(ct0, rotidx, rkSet, ctOut)
            return ctOut
        ctTmp, k = ct0, 1
        while rotidx > 0:
            if rotidx % 2:
                nxt = NewCiphertext(self.params, ct0.IDSet())
                self.ksw.Rotate(ctTmp, k, rkSet, nxt)
                ctTmp = nxt
            rotidx //= 2
            k *= 2
        return ctTmp

    def ConjugateNew(self, ct0, ckSet):
        """evaluator.go:182-192"""
        ctOut = NewCiphertext(self.params, ct0.IDSet())
        self.ksw.Conjugate(ct0, ckSet, ctOut)
        return ctOut

    # ---- hoisted rotations (the mirror of mkckks.Evaluator.HoistedForm / RotateHoistedNew: every mkrlwe-level call works on a BFV context)
    def HoistedForm(self, ct):
        h = mkrlwe.NewHoistedCiphertext()
        for id in ct.ids:
            h.Value[id] = mkrlwe.SwitchingKey(self.params, zero=False)          # every digit is written below
        check(lib().mkhe_hoisted_form(self.params.ctx, ct.Level(), ct.h, handle_array([h.Value[id].h for id in ct.ids])))
        return h

    def RotateHoistedNew(self, ct0, rotidx, ct0Hoisted, rkSet):
        """RotateNew from the hoisted form of ct0 (HoistedForm), shared by every rotation of ct0: the same ciphertext bit for bit"""
        rotidx %= self.params.N() // 2
        ctOut = NewCiphertext(self.params, ct0.IDSet(), zero=False)
        if rotidx == 0:
            check(lib().mkhe_ct_copy(self.params.ctx, ct0.h, ctOut.h))
            return ctOut
        if rotidx not in self.params.CRS:
            raise MkheError("Hoisted rotation only works for precomputed rotation keys")
        self.ksw.RotateHoisted(ct0, rotidx, ct0Hoisted, rkSet, ctOut)
        return ctOut

    # ---- plaintext linear transform (no reference counterpart: include/mkhe.h, "BFV plaintext linear transform")
    def LinearTransformBatch(self, cts, lt, rkSet, ckSet=None, fused=True):
        """M z for every ciphertext of `cts` (one id set, at most 16) and the cleartext diagonals of `lt` (LinearTransform), by baby steps and giant
        steps: LT_d(z) + swap(LT_e~(z)), the baby rotations shared by both parts and ONE mkhe_bfv_ct_ptxt_dot for the whole batch.  Keys for
        lt.Rotations(), and ckSet where lt.NeedsConjugation().  MkheError before any engine call when a CRS, a rotation key or a conjugation key is
        missing, the id sets differ or lt was built for other parameters.  fused=False runs the same schedule through the single-operation entry
        points and gives the same ciphertexts bit for bit."""
        return linear_transform_batch(self, cts, lt, rkSet, ckSet, fused)

    def LinearTransformNew(self, ct, lt, rkSet, ckSet=None, fused=True):
        """LinearTransformBatch of one ciphertext"""
        return self.LinearTransformBatch([ct], lt, rkSet, ckSet, fused)[0]

    # ---- plaintext operands (no reference counterpart: include/mkhe.h, "BFV plaintext operands").  The result carries the ids of the input: no
    # party is added and no key is used.
    def _encoder(self):
        if getattr(self, "_enc", None) is None:
            self._enc = DeviceEncoder(self.params)
        return self._enc

    def _ptmul(self, pt, B):
        """-> (PlaintextMul, stride in words) for B ciphertexts: one plaintext for all, or one per item"""
        if isinstance(pt, Message):
            pt = self._encoder().EncodeMul(pt.Value)
        elif isinstance(pt, (list, tuple)) and all(isinstance(m, Message) for m in pt):
            pt = self._encoder().EncodeMulBatch(np.stack([m.Value for m in pt]))
        if not isinstance(pt, PlaintextMul):
            raise MkheError("mkbfv.Evaluator: MulPtxt takes a PlaintextMul (Encoder.EncodeMul / DeviceEncoder.EncodeMul) or a Message")
        return pt, self._stride(pt.Value, B)

    def _ptadd(self, pt, B):
        if isinstance(pt, Message):
            pt = self._encoder().Encode(pt.Value)
        elif isinstance(pt, (list, tuple)) and all(isinstance(m, Message) for m in pt):
            pt = self._encoder().EncodeBatch(np.stack([m.Value for m in pt]))
        pt = self._encoder()._plaintexts(pt)
        return pt, self._stride(pt, B)

    def _stride(self, limbs, B):
        if limbs.limbs != self.params.QCount() or limbs.count not in (1, B):
            raise MkheError("mkbfv.Evaluator: %d ciphertexts need 1 or %d plaintexts of %d limbs, got %d of %d"
                            % (B, B, self.params.QCount(), limbs.count, limbs.limbs))
        return 0 if limbs.count == 1 and B > 1 else self.params.QCount() * self.params.N()

    def _outputs(self, cts):
        if len(cts) == 1:
            return [NewCiphertext(self.params, cts[0].IDSet(), zero=False)]
        return mkrlwe.batch_ciphertexts(Ciphertext, self.params, cts[0].IDSet(), self.params.MaxLevel(), len(cts))

    def MulPtxtBatch(self, cts, pts):
        """ct * plaintext for a list of ciphertexts of one id set as ONE engine call (mkhe_bfv_ct_mul_ptxt).  pts: a PlaintextMul holding one
        plaintext (shared) or one per ciphertext, or a Message / a list of Messages, which the device encoder prepares first."""
        pt, stride = self._ptmul(pts, len(cts))
        outs = self._outputs(cts)
        check(lib().mkhe_bfv_ct_mul_ptxt(self.params.ctx, len(cts), handle_array([c.h for c in cts]), pt.Value.devptr(), stride,
                                         handle_array([c.h for c in outs])))
        return outs

    def AddPtxtBatch(self, cts, pts, sub=False):
        """ct + plaintext (sub: ct - plaintext) for a list of ciphertexts of one id set as ONE engine call (mkhe_bfv_ct_add_ptxt).  pts: the
        DeviceLimbs of DeviceEncoder.Encode / EncodeBatch (one plaintext, or one per ciphertext), a host uint64 [nQ][N] / [B][nQ][N], a Message or a
        list of Messages."""
        pt, stride = self._ptadd(pts, len(cts))
        outs = self._outputs(cts)
        check(lib().mkhe_bfv_ct_add_ptxt(self.params.ctx, 1 if sub else 0, len(cts), handle_array([c.h for c in cts]), pt.devptr(), stride,
                                         handle_array([c.h for c in outs])))
        return outs

    def MulPtxtNew(self, ct, pt):
        """ct * pt slot by slot: pt a PlaintextMul, or a Message (encoded with the device encoder).  Three NTT launches and one elementwise kernel."""
        return self.MulPtxtBatch([ct], pt)[0]

    def AddPtxtNew(self, ct, pt):
        """ct + pt: pt the DeviceLimbs of DeviceEncoder.Encode, a host uint64 [nQ][N] (Encoder.Encode), or a Message"""
        return self.AddPtxtBatch([ct], pt)[0]

    def SubPtxtNew(self, ct, pt):
        """ct - pt, pt as for AddPtxtNew"""
        return self.AddPtxtBatch([ct], pt, sub=True)[0]

    # ---- weighted sums, additive constants and polynomials over Z_T (no reference counterpart: include/mkhe.h, "BFV weighted sums").  No key is
    # used and no party is added by the sums; the constants are encoded and uploaded per call: not inside a graph capture.
    def _consts_buffer(self, arr):
        n = self.params.N()
        buf = mkrlwe.DeviceLimbs(self.params, 1, -(-arr.size // n))
        return buf.upload(np.concatenate([arr.ravel(), np.zeros(buf.words - arr.size, dtype=np.uint64)]).reshape(1, buf.limbs, n))

    def LinCombsNew(self, cts, weight_rows, consts):
        """[sum_b weight_rows[g][b] * cts[b] + consts[g] for every g] slot by slot mod T as ONE engine call (mkhe_bfv_ct_lincomb): 1 to 16 ciphertexts
        of one id set, 1 to 64 rows of integer weights (any int, taken mod T) with one integer constant each.  The results are views of one pooled
        block."""
        cts, rows, consts = list(cts), [list(r) for r in weight_rows], list(consts)
        if not cts or len(cts) > LINCOMB_MAX_IN:
            raise MkheError("LinCombsNew: 1 to %d ciphertexts per call" % LINCOMB_MAX_IN)
        if not rows or len(rows) > LINCOMB_MAX_OUT or len(rows) != len(consts):
            raise MkheError("LinCombsNew: 1 to %d rows of weights per call, one constant per row" % LINCOMB_MAX_OUT)
        if any(len(r) != len(cts) for r in rows):
            raise MkheError("LinCombsNew: one weight per ciphertext in every row")
        if any(c.ids != cts[0].ids for c in cts):
            raise MkheError("LinCombsNew: the ciphertexts must carry the same ids")
        params = self.params
        buf = self._consts_buffer(bfv_lincomb_consts(params.Q, params.T(), rows, consts))
        outs = self._outputs([cts[0]] * len(rows))
        check(lib().mkhe_bfv_ct_lincomb(params.ctx, len(cts), handle_array([c.h for c in cts]), len(rows), buf.devptr(),
                                        handle_array([c.h for c in outs])))
        return outs

    def LinCombNew(self, cts, weights, const=0, fused=True):
        """sum_b weights[b] * cts[b] + const: the one-row form of LinCombsNew.  fused=False: the same sum through mkhe_ct_lincomb (real weights, no
        division), the same ciphertext bit for bit."""
        if fused:
            return self.LinCombsNew(cts, [weights], [const])[0]
        cts, weights = list(cts), list(weights)
        if not cts or len(cts) > LINCOMB_MAX_IN or len(cts) != len(weights):
            raise MkheError("LinCombNew: 1 to %d ciphertexts per call, one weight each" % LINCOMB_MAX_IN)
        if any(c.ids != cts[0].ids for c in cts):
            raise MkheError("LinCombNew: the ciphertexts must carry the same ids")
        params = self.params
        row = bfv_lincomb_consts(params.Q, params.T(), [weights], [const])[0]            # [nin + 1][nQ]
        buf = self._consts_buffer(np.stack([row, np.zeros_like(row)], axis=1))               # [nin + 1][2][nQ]: no imaginary part
        out = NewCiphertext(params, cts[0].IDSet(), zero=False)
        check(lib().mkhe_ct_lincomb(params.ctx, len(cts), handle_array([c.h for c in cts]), buf.devptr(), 0, out.h))
        return out

    def AddConstNew(self, ct, c):
        """ct + c in every slot: the weight 1, so only coefficient 0 of component 0 changes, limb by limb"""
        return self.LinCombNew([ct], [1], c)

    def MulConstNew(self, ct, w):
        """w * ct in every slot for an integer w (taken mod T, centred): a scalar per limb, no NTT"""
        return self.LinCombNew([ct], [w], 0)

    def EvaluatePolysNew(self, ct, polys, rlkSet, fused=True):
        """[sum_k coeffs[k] * ct^k mod T for every coeffs of polys] slot by slot (monomial basis, integer coefficients taken mod T, degree 1 .. 255)
        by baby steps and giant steps (mkckks.poly_eval_plan for the largest degree): the polynomials share the powers of ct and ONE LinCombsNew that
        writes every inner sum of every polynomial, then one MulRelinSumNew and one AddNew each.  MkheError before any engine call for a degree out of
        range, a zero polynomial, more than 64 inner sums in all or a missing CRS[-1].  fused=False runs the same schedule through one mkhe_ct_lincomb
        per inner sum and one MulRelinNew per giant product: the same decryption, another ciphertext."""
        return evaluate_polys(self, ct, polys, rlkSet, fused)

    def EvaluatePolyNew(self, ct, coeffs, rlkSet, fused=True):
        """EvaluatePolysNew of one polynomial"""
        return self.EvaluatePolysNew(ct, [coeffs], rlkSet, fused)[0]


MULRELIN_SUM_MAX = 16     # pairs per mkhe_bfv_mul_relin_sum call (csrc/poly_kernels.h, TSUM_MAX_K)
LINCOMB_MAX_IN, LINCOMB_MAX_OUT = 16, 64      # ciphertexts and rows per mkhe_bfv_ct_lincomb call (csrc/poly_kernels.h, BLIN_MAX_IN / BLIN_MAX_OUT)
POLY_MAX_DEGREE = 255


def bfv_lincomb_consts(Q, T, weight_rows, consts):
    """The constant block of mkhe_bfv_ct_lincomb, uint64 [nout][nin + 1][nQ], a pure function (Python integers).  Entry [g][0][l]: consts[g] taken to
    [0, T), then scale_up of include/mkhe.h: floor((Q c + floor(T/2)) / T) mod q_l.  Entry [g][1 + b][l]: weight_rows[g][b] taken mod T, then the lift of
    mkhe_bfv_lift: the centred representative w in (-T/2, T/2] as MForm(w mod q_l) = (w mod q_l) 2^64 mod q_l."""
    Q, T = [int(q) for q in Q], int(T)
    rows, consts = [list(r) for r in weight_rows], list(consts)
    if not rows or len(rows) != len(consts) or any(len(r) != len(rows[0]) for r in rows) or not rows[0]:
        raise MkheError("bfv_lincomb_consts: rows of one length, at least one weight, one constant per row")
    prod = 1
    for q in Q:
        prod *= q
    out = np.zeros((len(rows), len(rows[0]) + 1, len(Q)), dtype=np.uint64)
    for g, (row, c) in enumerate(zip(rows, consts)):
        up = ((int(c) % T) * prod + T // 2) // T
        for l, q in enumerate(Q):
            out[g, 0, l] = up % q
        for b, w in enumerate(row):
            w = int(w) % T
            w = w - T if w > T // 2 else w
            for l, q in enumerate(Q):
                out[g, 1 + b, l] = ((w % q) << 64) % q
    return out


def interpolate(xs, ys, T):
    """The coefficients mod T (monomial basis, constant first) of the polynomial of degree < len(xs) through the points (xs[i], ys[i]) over Z_T, T
    prime (Lagrange, Python integers).  MkheError when two abscissae agree mod T."""
    T = int(T)
    xs, ys = [int(x) % T for x in xs], [int(y) % T for y in ys]
    n = len(xs)
    if n < 1 or n != len(ys):
        raise MkheError("interpolate: as many values as abscissae, at least one")
    if len(set(xs)) != n:
        raise MkheError("interpolate: two abscissae agree mod T")
    master = [1]                                            # prod_i (X - x_i), constant first
    for x in xs:
        master = [(a - x * b) % T for a, b in zip([0] + master, master + [0])]
    out = [0] * n
    for x, y in zip(xs, ys):
        quot, carry = [0] * n, 0                            # master / (X - x) by synthetic division
        for k in range(n, 0, -1):
            carry = (master[k] + x * carry) % T
            quot[k - 1] = carry
        denom = 1
        for z in xs:
            if z != x:
                denom = denom * (x - z) % T
        s = y * pow(denom, -1, T) % T
        out = [(o + s * a) % T for o, a in zip(out, quot)]
    return out


def evaluate_polys(ev, ct, polys, rlkSet, fused=True):
    """Evaluator.EvaluatePolysNew on any evaluator with params, MulRelinNew, LinCombsNew, MulRelinSumNew and AddNew (fused=False: LinCombNew instead of
    the two fused calls).  With m, g of poly_eval_plan(largest degree): p(X) = sum_i inner_i(X) X^(m i), inner_i = sum_j coeffs[i m + j] X^j.  Stages:
    the baby powers X^2 .. X^(m-1) and giant powers X^(m i) that some polynomial uses (MulRelinNew); ONE LinCombsNew whose rows are the non-zero inner_i
    of every polynomial (an inner_i that is only a constant is a row of zero weights); per polynomial ONE MulRelinSumNew of its pairs (inner_i, X^(m i)),
    i >= 1; ONE AddNew with inner_0.  There is no scale to manage: every sum and product is exact mod T while the noise lasts."""
    params = ev.params
    T = int(params.T())
    polys = [[int(c) % T for c in p] for p in polys]
    if not polys:
        raise MkheError("EvaluatePolysNew: at least one polynomial")
    for p in polys:
        if len(p) - 1 < 1 or len(p) - 1 > POLY_MAX_DEGREE:
            raise MkheError("EvaluatePolysNew: the degree must be between 1 and %d" % POLY_MAX_DEGREE)
        if not any(p):
            raise MkheError("EvaluatePolysNew: the zero polynomial")
    plan = poly_eval_plan(max(len(p) - 1 for p in polys))
    m = plan.m
    inner = [[p[i: i + m] for i in range(0, len(p), m)] for p in polys]
    rows = [(k, i) for k, blocks in enumerate(inner) for i, c in enumerate(blocks) if any(c)]
    if len(rows) > LINCOMB_MAX_OUT:
        raise MkheError("EvaluatePolysNew: %d inner sums, at most %d per call" % (len(rows), LINCOMB_MAX_OUT))
    babies = sorted({j for k, i in rows for j, c in enumerate(inner[k][i]) if j and c}) or [1]
    giants = sorted({m * i for k, i in rows if i})
    if (giants or babies != [1]) and -1 not in params.CRS:
        raise MkheError("mkhe: CRS[-1] (u) has not been uploaded")
    needed = set(babies) | set(giants)
    for k, a, b in reversed(plan.products):                 # a power nobody uses is not computed
        if k in needed:
            needed |= {a, b}
    power = {1: ct}
    for k, a, b in plan.products:
        if k in needed:
            power[k] = ev.MulRelinNew(power[a], power[b], rlkSet)
    ins = [power[j] for j in babies]
    weights = [[(inner[k][i][j] if j < len(inner[k][i]) else 0) for j in babies] for k, i in rows]
    consts = [inner[k][i][0] for k, i in rows]
    if fused:
        sums = ev.LinCombsNew(ins, weights, consts)
    else:
        sums = [ev.LinCombNew(ins, w, c, fused=False) for w, c in zip(weights, consts)]
    sums = dict(zip(rows, sums))
    out = []
    for k in range(len(polys)):
        pairs = [(sums[(k, i)], power[m * i]) for kk, i in rows if kk == k and i]
        res = None
        if pairs and fused:
            res = ev.MulRelinSumNew([a for a, _ in pairs], [b for _, b in pairs], rlkSet)
        elif pairs:
            for a, b in pairs:
                prod = ev.MulRelinNew(a, b, rlkSet)
                res = prod if res is None else ev.AddNew(res, prod)
        if (k, 0) in sums:
            res = sums[(k, 0)] if res is None else ev.AddNew(res, sums[(k, 0)])
        out.append(res)
    return out


def NewEvaluator(params):
    return Evaluator(params)


# ---- plaintext linear transforms over Z_T (no reference counterpart; include/mkhe.h, "BFV plaintext linear transform").  A message is two rows of
# n = N/2 slots, z[r][j]; (M z)[r][j] = sum_k d_k[r][j] z[r][(j+k) mod n] + sum_k e_k[r][j] z[1-r][(j+k) mod n] = LT_d(z) + swap(LT_e~(z)) with
# e~_k[r] = e_k[1-r].  The construction below is pure (numpy only), so that it can be checked against the defining sum without a context.
PTXT_DOT_MAX_BATCH = 16                                   # csrc/poly_kernels.h, CTDOT_MAX_BATCH
CT_SUM_MAX = 16                                           # ciphertexts per mkhe_ct_sum call the transform issues
LinTransLayout = collections.namedtuple("LinTransLayout", "plan giants_d giants_e order masks rows")


def diagonal_rows(diagonals, n, what="diagonals"):
    """{k: int64 [2][n] or [n]} -> {k mod n: int64 [2][n]}: a [n] array is the same diagonal in both rows"""
    out = {}
    for k, d in dict(diagonals or {}).items():
        d = np.asarray(d)
        if d.dtype.kind not in "iu":
            raise MkheError("mkbfv.LinearTransform: %s[%d] must be integers (they are taken mod T)" % (what, k))
        d = d.astype(np.int64)
        if d.shape == (n,):
            d = np.stack([d, d])
        if d.shape != (2, n):
            raise MkheError("mkbfv.LinearTransform: %s[%d] must have shape (2, %d) or (%d,), got %r" % (what, k, n, n, d.shape))
        if int(k) % n in out:
            raise MkheError("mkbfv.LinearTransform: %s[%d] is given twice (indices are taken mod %d)" % (what, k, n))
        out[int(k) % n] = d
    return out


def linear_transform_layout(n, diagonals, swapped=None, n1=None):
    """The plan, the masks and the pre-rotated diagonals of a transform, a pure function.  The plan (mkckks.linear_transform_plan) is taken over the
    union of both index sets, so that both parts share n1 and the babies.  -> LinTransLayout: giants_d / giants_e the giants of each part, order =
    [(part, g, b)] and rows = [int64 [2][n]] in the order of the plaintext block (part 0 = d, part 1 = e~; roll(d_(g+b), g) along the slots of each
    row), masks for [giants of d] + [giants of e~] over the babies of the plan."""
    d, e = diagonal_rows(diagonals, n), diagonal_rows(swapped, n, "swapped")
    if not d and not e:
        raise MkheError("mkbfv.LinearTransform: no diagonal")
    plan = linear_transform_plan(set(d) | set(e), n, n1)
    parts = [d, {k: v[::-1] for k, v in e.items()}]                                  # e~_k[r] = e_k[1 - r]
    giants = [sorted({k - k % plan.n1 for k in p}) for p in parts]
    if len(giants[0]) + len(giants[1]) > PTXT_DOT_MAX_GIANT:
        raise MkheError("mkbfv.LinearTransform: more than %d giant steps over the two parts" % PTXT_DOT_MAX_GIANT)
    order, masks, rows = [], [], []
    for part, p in enumerate(parts):
        for g in giants[part]:
            masks.append(sum(1 << i for i, b in enumerate(plan.babies) if (g + b) in p))
            for b in plan.babies:
                if (g + b) in p:
                    order.append((part, g, b))
                    rows.append(np.roll(p[g + b], g, axis=1))
    return LinTransLayout(plan, giants[0], giants[1], order, masks, rows)


def matrix_layout(M, n, blocks=False):
    """(diagonals, swapped) of an integer matrix for n slots per row, the all-zero diagonals left out.  blocks=False: M is d x d and acts on each
    row, d_k[r][j] = M[j mod d][(j + k) mod d].  blocks=True: M = [[A, B], [C, D]] is 2d x 2d; A and D act within rows 0 and 1, B takes row 1 into
    row 0 and C row 0 into row 1 (the swapped diagonals).  d a power of two <= n."""
    M = np.asarray(M)
    if M.dtype.kind not in "iu":
        raise MkheError("mkbfv.LinearTransform.FromMatrix: the matrix must hold integers")
    M = M.astype(np.int64)
    d = M.shape[0] // 2 if blocks else M.shape[0]
    if M.ndim != 2 or M.shape[0] != M.shape[1] or (blocks and M.shape[0] != 2 * d) or d < 1 or d & (d - 1) or d > n:
        raise MkheError("mkbfv.LinearTransform.FromMatrix: the matrix must be d x d (blocks: 2d x 2d) with d a power of two, at most %d" % n)
    j = np.arange(n)
    diag = lambda A, k: A[j % d, (j + k) % d]
    if blocks:
        A, B, Cm, D = M[:d, :d], M[:d, d:], M[d:, :d], M[d:, d:]
    else:
        A, B, Cm, D = M, None, None, M
    diags = {k: np.stack([diag(A, k), diag(D, k)]) for k in range(d)}
    swapped = {k: np.stack([diag(B, k), diag(Cm, k)]) for k in range(d)} if blocks else {}
    diags = {k: v for k, v in diags.items() if v.any()}
    swapped = {k: v for k, v in swapped.items() if v.any()}
    if not diags and not swapped:
        raise MkheError("mkbfv.LinearTransform.FromMatrix: the zero matrix")
    return diags, swapped


class _PlaintextInBlock(mkrlwe.DeviceLimbs):
    """plaintext `index` of a block of prepared plaintexts, where it lies: what MulPtxtNew takes as a PlaintextMul.  Holds the block, owns nothing."""

    def __init__(self, block, index):
        self.params, self.count, self.limbs = block.params, 1, block.limbs
        self.words = block.limbs * block.params.N()
        self._block = block
        self.d = C.c_void_p(block.devptr().value + 8 * self.words * index)

    def __del__(self):
        pass


class LinearTransform:
    """The diagonals of a Z_T-linear map on the two slot rows, encoded once for Evaluator.LinearTransformNew / LinearTransformBatch.  diagonals
    {k: d_k} keep the rows, swapped {k: e_k} exchange them: (M z)[r][j] = sum_k d_k[r][j] z[r][(j+k) mod n] + sum_k e_k[r][j] z[1-r][(j+k) mod n] --
    the convention of RotateNew(ct, k), which moves slot j + k to slot j in each row, and of ConjugateNew, which swaps the rows.  Each d_k / e_k is
    an int64 [2][n] array, or [n] for the same diagonal in both rows.  All pre-rotated diagonals of both parts are encoded in ONE
    DeviceEncoder.EncodeMulBatch into the compact block of mkhe_bfv_ct_ptxt_dot.  keep_single is accepted for symmetry with mkckks (keep_coeff):
    the single calls of fused=False address a plaintext inside the block (Plaintext(i)), so nothing more is kept."""

    def __init__(self, params, diagonals, swapped=None, n1=None, keep_single=False):
        self.params, self.n = params, params.N() // 2
        lay = linear_transform_layout(self.n, diagonals, swapped, n1)
        self.plan, self.giants_d, self.giants_e, self.order, self.masks = lay.plan, lay.giants_d, lay.giants_e, lay.order, lay.masks
        self.keep_single = bool(keep_single)
        self.pt = DeviceEncoder(params).EncodeMulBatch(np.stack([r.reshape(-1) for r in lay.rows]))

    @classmethod
    def FromMatrix(cls, params, M, blocks=False, **kw):
        """blocks=False: the d x d integer matrix M applied to each slot row, as its d-periodic diagonals: on rows whose d entries are replicated
        n / d times it gives M @ v mod T, replicated.  blocks=True: the 2d x 2d matrix [[A, B], [C, D]] on the pair of rows (matrix_layout)."""
        diags, swapped = matrix_layout(M, params.N() // 2, blocks)
        return cls(params, diags, swapped, **kw)

    def Rotations(self):
        """the sorted non-zero baby and giant indices: what AddCRS / GenRotationKey must have provided"""
        return sorted({r for r in self.plan.babies + self.giants_d + self.giants_e if r})

    def NeedsConjugation(self):
        """whether the transform has a row-swapping part: a conjugation key per party and CRS[-2]"""
        return bool(self.giants_e)

    def Plaintext(self, index):
        """prepared plaintext `index` of the block (the order of self.order) as a PlaintextMul, read where it lies"""
        return PlaintextMul(self.params, _PlaintextInBlock(self.pt.Value, index))


def linear_transform_batch(ev, cts, lt, rkSet, ckSet=None, fused=True):
    """Evaluator.LinearTransformBatch.  Launch sets of the fused form for B items: HoistedForm of each item; the non-zero baby rotations of all items
    as lanes of mkhe_rotate_multi; ONE mkhe_bfv_ct_ptxt_dot; the non-zero giant rotations as lanes of mkhe_rotate_multi; mkhe_ct_sum per part in groups
    of 16; mkhe_conjugate of the swapped sum; mkhe_ct_add."""
    params, cts = ev.params, list(cts)
    if lt.params is not params:
        raise MkheError("LinearTransform: the transform was encoded for other parameters")
    if not cts or len(cts) > PTXT_DOT_MAX_BATCH:
        raise MkheError("LinearTransformBatch: takes 1 to %d ciphertexts" % PTXT_DOT_MAX_BATCH)
    ids = cts[0].ids
    for ct in cts:
        if ct.ids != ids:
            raise MkheError("LinearTransformBatch: the ciphertexts of one call must be over the same ids")
    keys = mkrlwe.rotation_keys(params, rkSet, ids, lt.Rotations(), "LinearTransform")
    if lt.NeedsConjugation():
        if ckSet is None:
            raise MkheError("LinearTransform: the transform swaps the slot rows: pass the conjugation keys (ckSet)")
        if -2 not in params.CRS:
            raise MkheError("LinearTransform: no CRS for the conjugation (CRS[-2])")
        for i in ids:
            ckSet.GetConjugationKey(i)
    L, ctx, B = lib(), params.ctx, len(cts)
    babies, giants = lt.plan.babies, lt.giants_d + lt.giants_e
    nd = len(lt.giants_d)
    new = lambda: NewCiphertext(params, ids, zero=False)
    hoisted = [ev.HoistedForm(ct) if any(babies) else None for ct in cts]

    summed = lambda terms: mkrlwe.sum_in_groups(ctx, terms, new, CT_SUM_MAX)

    def finish(part_d, part_e, add_all):
        """LT_d + swap(LT_e~) from the rotated inner sums of each part"""
        total = add_all(part_d) if part_d else None
        if part_e:
            sw = ev.ConjugateNew(add_all(part_e), ckSet)
            total = sw if total is None else ev.AddNew(total, sw)
        return total

    if not fused:
        outs = []
        for ct, h in zip(cts, hoisted):
            rot = {b: ev.RotateHoistedNew(ct, b, h, rkSet) if b else ct for b in babies}
            terms, index = [], 0
            for g, mask in zip(giants, lt.masks):
                part = None
                for i, b in enumerate(babies):
                    if mask >> i & 1:
                        prod = ev.MulPtxtNew(rot[b], lt.Plaintext(index))
                        part = prod if part is None else ev.AddNew(part, prod)
                        index += 1
                terms.append(ev.RotateNew(part, g, rkSet) if g else part)
            outs.append(finish(terms[:nd], terms[nd:], lambda t: functools.reduce(ev.AddNew, t)))
        return outs

    def rotate_lanes(srcs, rots, hoists):
        outs = mkrlwe.batch_ciphertexts(Ciphertext, params, ids, params.MaxLevel(), len(srcs)) if len(srcs) > 1 else [new()]
        return mkrlwe.rotate_lanes(params, keys, ids, srcs, rots, hoists, outs)

    nzb = [b for b in babies if b]
    rot = [{0: ct} for ct in cts]
    if nzb:
        lanes = rotate_lanes([ct for ct in cts for _ in nzb], nzb * B, [h for h in hoisted for _ in nzb])
        for k in range(B):
            rot[k].update(zip(nzb, lanes[k * len(nzb): (k + 1) * len(nzb)]))
    inner = mkrlwe.batch_ciphertexts(Ciphertext, params, ids, params.MaxLevel(), B * len(giants)) if B * len(giants) > 1 else [new()]
    masks = (C.c_uint32 * len(giants))(*lt.masks)
    check(L.mkhe_bfv_ct_ptxt_dot(ctx, B, len(babies), handle_array([rot[k][b].h for k in range(B) for b in babies]), len(giants), masks,
                                 lt.pt.Value.devptr(), handle_array([c.h for c in inner])))
    nz = [(k, j) for k in range(B) for j, g in enumerate(giants) if g]
    if nz:
        lanes = rotate_lanes([inner[k * len(giants) + j] for k, j in nz], [giants[j] for _, j in nz], None)
        for (k, j), c in zip(nz, lanes):
            inner[k * len(giants) + j] = c
    outs = []
    for k in range(B):
        terms = inner[k * len(giants): (k + 1) * len(giants)]
        outs.append(finish(terms[:nd], terms[nd:], summed))
    return outs


# ---- encoder, encryptor, decryptor (mkbfv/encryptor.go, mkbfv/decryptor.go, elements.go:26-28); plaintexts are RNS polynomials over Q.
# lattigo's bfv.Encoder, which EncodeInt / DecodeInt of those files reach, is not in the reference tree: Encoder / DeviceEncoder restate the
# mathematics of slot batching over Z_T (include/mkhe.h, "BFV batch encoder"), not lattigo's code path.  ScaleUp / ScaleDown are the
# coefficient-wise halves of EncodeInt / DecodeInt.
def _q_product(params):
    Q = 1
    for q in params.Q:
        Q *= q
    return Q


def ScaleUp(m, params):
    """coefficients over Z_T -> RNS polynomial uint64 [nQ][N]: round(Q/T * (m mod T)), exact in Python integers"""
    Q, T = _q_product(params), params.T()
    c = ((np.asarray(m).astype(object) % T) * Q + T // 2) // T
    return np.stack([np.array([int(v) for v in c % q], dtype=np.uint64) for q in params.Q])


def ScaleDown(poly, params):
    """RNS polynomial [nQ][N] -> round(T/Q * x) mod T with x the centred CRT lift, centred in (-T/2, T/2], int64"""
    Q, T = _q_product(params), params.T()
    poly = np.asarray(poly, dtype=np.uint64)
    x = np.zeros(poly.shape[1], dtype=object)
    for l, q in enumerate(params.Q):
        Mi = Q // q
        x = x + poly[l].astype(object) * (Mi * pow(Mi, -1, q))
    x = x % Q
    out = []
    for v in x:
        v = v - Q if v > Q // 2 else v
        r = ((v * T * 2 + Q) // (2 * Q)) % T
        out.append(r - T if r > T // 2 else r)
    return np.array(out, dtype=np.int64)


def Lift(m, params):
    """coefficients over Z_T -> uint64 [nQ][N]: MForm(c mod q_l) = (c mod q_l) 2^64 mod q_l for the centred representative c of m mod T (c = m for
    m <= floor(T/2), else m - T), exact in Python integers.  The multiplication plaintext in the coefficient domain (mkhe_bfv_lift)."""
    T = params.T()
    c = [int(v) % T for v in np.asarray(m).astype(object)]
    c = [v - T if v > T // 2 else v for v in c]
    return np.stack([np.array([((v % q) << 64) % q for v in c], dtype=np.uint64) for q in params.Q])


class PlaintextMul:
    """`count` prepared multiplication plaintexts: Value = mkrlwe.DeviceLimbs [count][nQ][N], the forward NTT over Q of Lift, in Montgomery form
    (the operand of Evaluator.MulPtxtNew / MulPtxtBatch).  value: such a DeviceLimbs, or the host array of Encoder.EncodeMul ([nQ][N] or
    [count][nQ][N]), which is uploaded."""

    def __init__(self, params, value):
        if not isinstance(value, mkrlwe.DeviceLimbs):
            value = np.ascontiguousarray(value, dtype=np.uint64)
            value = value[None] if value.ndim == 2 else value
            value = mkrlwe.DeviceLimbs(params, value.shape[0], value.shape[1]).upload(value)
        if value.limbs != params.QCount():
            raise MkheError("mkbfv.PlaintextMul: a BFV plaintext has %d limbs, got %d" % (params.QCount(), value.limbs))
        self.params, self.Value = params, value

    @property
    def count(self):
        return self.Value.count

    def download(self):
        return self.Value.download()


def _is_prime(n):
    if n < 2:
        return False
    small = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for p in small:
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in small:                                  # deterministic below 2^64
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def slot_psi(T, N):
    """the engine's choice of a primitive 2N-th root of unity (csrc/engine.hip default_psi) for the plaintext modulus: g the smallest
    generator >= 3 of Z_T*, psi = g^((T-1)/2N).  Raises where the encoder calls of the C ABI do."""
    T, N = int(T), int(N)
    if T >= 1 << 32:
        raise MkheError("mkbfv encoder: the plaintext modulus must be below 2^32")
    if not _is_prime(T):
        raise MkheError("mkbfv encoder: the plaintext modulus must be prime")
    if (T - 1) % (2 * N):
        raise MkheError("mkbfv encoder: the plaintext modulus must be 1 mod 2N")
    f, n, p = [], T - 1, 2
    while p * p <= n:
        if n % p == 0:
            f.append(p)
            while n % p == 0:
                n //= p
        p += 1 if p == 2 else 2
    if n > 1:
        f.append(n)
    g = 3
    while any(pow(g, (T - 1) // q, T) == 1 for q in f):
        g += 1
    return pow(g, (T - 1) // (2 * N), T)


def slot_exponents(logN):
    """e with slot j = m(psi^e[j]): e[i] = 5^i mod 2N, e[N/2 + i] = 2N - e[i] (two rows of N/2: lattigo's index matrix)"""
    N = 1 << logN
    e, g = np.empty(N, dtype=np.int64), 1
    for i in range(N // 2):
        e[i], e[N // 2 + i], g = g, 2 * N - g, g * mkrlwe.GALOIS_GEN % (2 * N)
    return e


class Message:
    """mkbfv.Message (elements.go:26-28): Value []int64, one value per slot"""

    def __init__(self, value):
        self.Value = np.asarray(value, dtype=np.int64)

    def Slots(self):
        return len(self.Value)


def NewMessage(params):
    return Message(np.zeros(params.N(), dtype=np.int64))


class Encoder:
    """Exact host model of the batch encoder (numpy, uint64 arithmetic mod T < 2^32): slots <-> coefficients by a negacyclic number-theoretic
    transform mod T, then ScaleUp / ScaleDown.  `params` needs N(), LogN(), T() and Q only."""

    def __init__(self, params):
        self.params = params
        self.N, self.logN, self.T = params.N(), params.LogN(), int(params.T())
        N, T = self.N, self.T
        self.psi = slot_psi(T, N)
        k = np.arange(N, dtype=object)
        pw = lambda b: np.array([pow(b, int(i), T) for i in k], dtype=np.uint64)      # (N modular powers, once per encoder)
        psi_inv = pow(self.psi, -1, T)
        self._twist, self._itwist = pw(self.psi), pw(psi_inv) * np.uint64(pow(N, -1, T)) % np.uint64(T)
        self._w, self._winv = pw(self.psi * self.psi % T)[: N // 2], pw(psi_inv * psi_inv % T)[: N // 2]
        self._t = (slot_exponents(self.logN) - 1) // 2                                # slot j is bin t[j] of the cyclic transform

    def _dft(self, a, w):
        """X[k] = sum_j a_j w^(jk) mod T, natural order in and out: radix-2 decimation in time on a bit-reversed copy"""
        N, T = self.N, np.uint64(self.T)
        rev = np.zeros(N, dtype=np.int64)
        for b in range(self.logN):
            rev |= ((np.arange(N) >> b) & 1) << (self.logN - 1 - b)
        a = a[rev].copy()
        h = 1
        while h < N:
            a = a.reshape(-1, 2, h)
            tw = w[:: N // (2 * h)][:h]
            x = a[:, 1, :] * tw % T
            a = np.stack([(a[:, 0, :] + x) % T, (a[:, 0, :] + T - x) % T], axis=1).reshape(-1)
            h *= 2
        return a

    def residues(self, values):
        """int64 message values -> residues in [0, T) as uint64"""
        v = np.asarray(values, dtype=np.int64)
        if v.shape != (self.N,):
            raise MkheError("mkbfv.Encoder: expected %d slots, got %r" % (self.N, v.shape))
        return np.mod(v, np.int64(self.T)).astype(np.uint64)

    def SlotsToCoeffs(self, values):
        """slots int64 [N] -> coefficients uint64 [N] in [0, T)"""
        z = np.zeros(self.N, dtype=np.uint64)
        z[self._t] = self.residues(values)
        return self._dft(z, self._winv) * self._itwist % np.uint64(self.T)

    def CoeffsToSlots(self, coeffs):
        """coefficients mod T [N] -> slots int64 [N], centred in (-T/2, T/2]"""
        T = np.uint64(self.T)
        m = np.asarray(coeffs, dtype=np.uint64) % T
        z = self._dft(m * self._twist % T, self._w)[self._t].astype(np.int64)
        return np.where(z > self.T // 2, z - self.T, z)

    def Encode(self, values):
        """slots int64 [N] -> RNS plaintext uint64 [nQ][N] (EncodeInt of encryptor.go:38-41)"""
        return ScaleUp(self.SlotsToCoeffs(values), self.params)

    def Decode(self, poly):
        """RNS plaintext [nQ][N] (canonical residues) -> slots int64 [N], centred (DecodeInt of decryptor.go:52-54)"""
        return self.CoeffsToSlots(np.mod(ScaleDown(poly, self.params), np.int64(self.T)).astype(np.uint64))

    def EncodeMul(self, values):
        """slots int64 [N] -> the prepared multiplication plaintext uint64 [nQ][N]: the same bits as DeviceEncoder.EncodeMul.  The slot transform and
        the lift (Lift) run here in numpy / Python integers; the forward NTT over Q is NOT restated: it is the engine's own (mkhe_ntt on the uploaded
        lift), so `params` must be device parameters (mkbfv.Parameters) for this call."""
        params = self.params
        lift = mkrlwe.DeviceLimbs(params, 1, params.QCount()).upload(Lift(self.SlotsToCoeffs(values), params)[None])
        out = mkrlwe.DeviceLimbs(params, 1, params.QCount())
        mkrlwe.ntt(params, lift, out)
        return out.download()[0]


class DeviceEncoder:
    """The interface of Encoder on the DEVICE (mkhe_bfv_*: csrc/bfv_kernels.hip), plus batch forms.  Messages go up and come down as N int64
    slots; plaintexts stay resident as mkrlwe.DeviceLimbs [count][nQ][N].  Integer arithmetic throughout: the same bits as Encoder."""

    def __init__(self, params):
        self.params = params
        self.N = params.N()

    def _rows(self, a, dtype, what):
        """-> (array [count][N] of dtype, whether the caller passed one row)"""
        a = np.asarray(a, dtype=dtype)
        one = a.ndim == 1
        a = a[None] if one else a
        if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] != self.N:
            raise MkheError("mkbfv.DeviceEncoder: expected %d %s per message, got %r" % (self.N, what, a.shape))
        return np.ascontiguousarray(a), one

    def _up(self, a):
        return mkrlwe.DeviceLimbs(self.params, len(a), 1).upload(a.view(np.uint64).reshape(len(a), 1, self.N))

    def _stage(self, fn, src, limbs_out, dtype, one):
        dst = mkrlwe.DeviceLimbs(self.params, src.count, limbs_out)
        check(fn(self.params.ctx, src.count, src.devptr(), dst.devptr()))
        if dtype is None:                                # a plaintext: stays on the device
            return dst
        out = dst.download().view(dtype).reshape(src.count, self.N)
        return out[0] if one else out

    def SlotsToCoeffs(self, values):
        """slots int64 [N] (or [count][N]) -> coefficients uint64 in [0, T)"""
        z, one = self._rows(values, np.int64, "slots")
        return self._stage(lib().mkhe_bfv_slots_to_coeffs, self._up(z), 1, np.uint64, one)

    def CoeffsToSlots(self, coeffs):
        """coefficients uint64 [N] (or [count][N]) -> slots int64, centred"""
        m, one = self._rows(coeffs, np.uint64, "coefficients")
        return self._stage(lib().mkhe_bfv_coeffs_to_slots, self._up(m), 1, np.int64, one)

    def ScaleUp(self, coeffs):
        """coefficients uint64 [N] (or [count][N]) -> device plaintexts [count][nQ][N]"""
        m, _ = self._rows(coeffs, np.uint64, "coefficients")
        return self._stage(lib().mkhe_bfv_scale_up, self._up(m), self.params.QCount(), None, False)

    def _plaintexts(self, poly):
        if not isinstance(poly, mkrlwe.DeviceLimbs):
            poly = np.ascontiguousarray(poly, dtype=np.uint64)
            poly = poly[None] if poly.ndim == 2 else poly
            poly = mkrlwe.DeviceLimbs(self.params, poly.shape[0], poly.shape[1]).upload(poly)
        if poly.limbs != self.params.QCount():
            raise MkheError("mkbfv.DeviceEncoder: a BFV plaintext has %d limbs, got %d" % (self.params.QCount(), poly.limbs))
        return poly

    def ScaleDown(self, poly):
        """device plaintext(s) [count][nQ][N] (or a host polynomial) -> coefficients uint64 in [0, T) (not centred)"""
        poly = self._plaintexts(poly)
        return self._stage(lib().mkhe_bfv_scale_down, poly, 1, np.uint64, poly.count == 1)

    def EncodeBatch(self, values):
        """count messages -> device plaintexts [count][nQ][N] (coefficient domain, canonical) as one launch set"""
        z, _ = self._rows(values, np.int64, "slots")
        return self._stage(lib().mkhe_bfv_encode, self._up(z), self.params.QCount(), None, False)

    def Encode(self, values):
        """-> device plaintext [1][nQ][N]: what mkrlwe.Encryptor.Encrypt takes as it is"""
        z, one = self._rows(values, np.int64, "slots")
        if not one:
            raise MkheError("mkbfv.DeviceEncoder: Encode takes one message (EncodeBatch takes several)")
        return self.EncodeBatch(z)

    def Decode(self, poly):
        """device plaintext(s) [count][nQ][N] (or a host polynomial [nQ][N]) -> slots int64 [N] ([count][N] for count > 1), centred"""
        poly = self._plaintexts(poly)
        return self._stage(lib().mkhe_bfv_decode, poly, 1, np.int64, poly.count == 1)

    def Lift(self, coeffs):
        """coefficients uint64 [N] (or [count][N]) -> device buffer [count][nQ][N]: MForm of the centred lift, coefficient domain (mkhe_bfv_lift)"""
        m, _ = self._rows(coeffs, np.uint64, "coefficients")
        return self._stage(lib().mkhe_bfv_lift, self._up(m), self.params.QCount(), None, False)

    def EncodeMulBatch(self, values):
        """count messages -> PlaintextMul of count prepared plaintexts as one launch set (mkhe_bfv_encode_mul)"""
        z, _ = self._rows(values, np.int64, "slots")
        return PlaintextMul(self.params, self._stage(lib().mkhe_bfv_encode_mul, self._up(z), self.params.QCount(), None, False))

    def EncodeMul(self, values):
        """one message -> PlaintextMul: what Evaluator.MulPtxtNew takes as it is"""
        z, one = self._rows(values, np.int64, "slots")
        if not one:
            raise MkheError("mkbfv.DeviceEncoder: EncodeMul takes one message (EncodeMulBatch takes several)")
        return self.EncodeMulBatch(z)


def _encoder(params, which):
    if which not in ("host", "device"):
        raise MkheError("mkbfv: encoder must be \"host\" or \"device\"")
    return Encoder(params) if which == "host" else DeviceEncoder(params)


class Encryptor(mkrlwe.Encryptor):
    """mkbfv.Encryptor (encryptor.go:7-25): mkrlwe.Encryptor + the encoder.  encoder="host" (default): the numpy Encoder, whose plaintext
    is uploaded; "device": DeviceEncoder, whose plaintext goes to mkhe_encrypt without touching the host.  The encoder is built at its
    first use, so that EncryptPtxt works for every plaintext modulus the context accepts."""

    def __init__(self, params, sampler=None, encoder="host"):
        super().__init__(params, sampler)
        if encoder not in ("host", "device"):
            raise MkheError("mkbfv: encoder must be \"host\" or \"device\"")
        self._which, self._encoder = encoder, None

    @property
    def encoder(self):
        if self._encoder is None:
            self._encoder = _encoder(self.params, self._which)
        return self._encoder

    def _new_batch(self, id, level, count, like=None):
        return mkrlwe.batch_ciphertexts(Ciphertext, self.params, [id], level, count)

    def EncryptPtxt(self, pt_rns, pk, samples=None):
        """encryptor.go:30-32 on a fresh ciphertext over {pk.ID} (EncryptMsgNew :47-51 without the encoder)"""
        return self.Encrypt(pt_rns, pk, NewCiphertext(self.params, [pk.ID], zero=False), samples)

    def EncryptMsg(self, msg, pk, ctOut, samples=None):
        """encryptor.go:38-41: EncodeInt, then Encrypt"""
        return self.Encrypt(self.encoder.Encode(msg.Value), pk, ctOut, samples)

    def EncryptMsgNew(self, msg, pk, samples=None):
        """encryptor.go:47-51"""
        return self.EncryptMsg(msg, pk, NewCiphertext(self.params, [pk.ID], zero=False), samples)

    def EncryptMsgBatch(self, msgs, pk, samples=None):
        """EncryptMsgNew for several messages under one public key: one encode (one launch set with the device encoder) and one
        mkhe_encrypt call"""
        if isinstance(self.encoder, DeviceEncoder):
            pts = self.encoder.EncodeBatch(np.stack([m.Value for m in msgs]))
        else:
            pts = np.stack([self.encoder.Encode(m.Value) for m in msgs])
        return self.EncryptBatch(pts, pk, samples)


def NewEncryptor(params, sampler=None, encoder="host"):
    return Encryptor(params, sampler, encoder)


class SeededCiphertext(mkrlwe.SeededCiphertext):
    """mkrlwe.SeededCiphertext at the maximum level whose Expand() returns mkbfv Ciphertexts"""

    def __init__(self, params, id, count=1):
        super().__init__(params, id, params.MaxLevel(), count, cls=Ciphertext)

    def Expand(self, level=None):
        if level is not None and level != self._level:
            raise MkheError("mkbfv.SeededCiphertext: a BFV ciphertext is always at the maximum level")
        return super().Expand()


class SecretKeyEncryptor(mkrlwe.SecretKeyEncryptor):
    """mkrlwe.SecretKeyEncryptor + the encoder (no reference counterpart): a party encrypts its own slots under its secret key.
    EncryptMsgSeeded returns the half-size form that travels; its Expand() gives what EncryptMsgBatch gives.  The encoder as for Encryptor."""

    def __init__(self, params, sk, sampler=None, encoder="host", seed=None, insecure_test_only=False):
        super().__init__(params, sk, sampler, seed, insecure_test_only)
        if encoder not in ("host", "device"):
            raise MkheError("mkbfv: encoder must be \"host\" or \"device\"")
        self._which, self._encoder = encoder, None

    @property
    def encoder(self):
        if self._encoder is None:
            self._encoder = _encoder(self.params, self._which)
        return self._encoder

    def _new_batch(self, level, count):
        return mkrlwe.batch_ciphertexts(Ciphertext, self.params, [self.sk.ID], level, count)

    def _new_seeded(self, level, count):
        return SeededCiphertext(self.params, self.sk.ID, count)

    def _encode(self, msgs):
        if isinstance(self.encoder, DeviceEncoder):
            return self.encoder.EncodeBatch(np.stack([m.Value for m in msgs]))
        return np.stack([self.encoder.Encode(m.Value) for m in msgs])

    def EncryptMsgBatch(self, msgs, e=None):
        """one encode (one launch set with the device encoder) and one mkhe_encrypt_sk / mkhe_encrypt_sk_seeded call"""
        return self.EncryptBatch(self._encode(msgs), e)

    def EncryptMsgNew(self, msg, e=None):
        return self.EncryptMsgBatch([msg], None if e is None else np.asarray(e)[None])[0]

    def EncryptMsgSeeded(self, msgs, e=None):
        return self.EncryptSeededBatch(self._encode(msgs), e)


def NewSecretKeyEncryptor(params, sk, sampler=None, encoder="host", seed=None, insecure_test_only=False):
    return SecretKeyEncryptor(params, sk, sampler, encoder, seed, insecure_test_only)


class Decryptor(mkrlwe.Decryptor):
    """mkbfv.Decryptor (decryptor.go:6-24); the encoder as for Encryptor"""

    def __init__(self, params, encoder="host"):
        super().__init__(params)
        if encoder not in ("host", "device"):
            raise MkheError("mkbfv: encoder must be \"host\" or \"device\"")
        self._which, self._encoder = encoder, None

    @property
    def encoder(self):
        if self._encoder is None:
            self._encoder = _encoder(self.params, self._which)
        return self._encoder

    def _like(self, ct, ids):
        return NewCiphertext(self.params, ids, zero=False)

    def DecryptPtxt(self, ct, skSet):
        """decryptor.go:34-53 up to the decoder -> RNS polynomial uint64 [nQ][N], canonical"""
        return mkrlwe.Decryptor.Decrypt(self, ct, skSet).download()[0]

    def Decrypt(self, ct, skSet):
        """decryptor.go:31-56 -> Message.  With the device encoder the output buffer of mkhe_decrypt goes straight to mkhe_bfv_decode: only
        the slots come down."""
        if isinstance(self.encoder, DeviceEncoder):
            return Message(self.encoder.Decode(mkrlwe.Decryptor.Decrypt(self, ct, skSet)))
        return Message(self.encoder.Decode(self.DecryptPtxt(ct, skSet)))

    def MaxFloodBits(self, parties):
        """floor(log2(Q / (2 T parties))): with flood_bits up to this, parties * 2^(flood_bits - 1) <= Q / (4 T), which leaves the other half of
        the decryption margin Q / (2 T) to the noise of the ciphertext (the message is exact while the two together stay below Q / (2 T))"""
        Q = 1
        for q in self.params.Q:
            Q *= int(q)
        return (Q // (2 * int(self.params.T()) * int(parties))).bit_length() - 1

    def InvariantNoise(self, ct, skSet):
        """r = max_n |[T * phase(ct)]_Q| as a Python integer, measured on the device (mkhe_noise_norm, kind 1): with phase = up(m) + e it is
        T |e| up to the rounding of up, and needs no message.  r <= (Q - 1) / 2."""
        return self.NoiseNormBatch(mkrlwe.Decryptor.Decrypt(self, ct, skSet), kind=1)[0][0]

    def NoiseBudget(self, ct, skSet):
        """bitlen(Q) - bitlen(InvariantNoise) - 1, in bits: never negative, and 0 where the noise has reached Q / (2 T) and decryption fails"""
        return int(_q_product(self.params)).bit_length() - self.InvariantNoise(ct, skSet).bit_length() - 1

    def NoiseNorm(self, ct, skSet, msg=None):
        """The noise of ct, max_n |e_n| with phase(ct) = up(m) + e, as a Python integer.  With msg (a Message): exactly, as the residual
        against the DEVICE encoder's plaintext of msg (mkhe_bfv_encode), whichever encoder this Decryptor decodes with.  Without: the bound
        (r + T // 2) // T + 1 from r = InvariantNoise, which lies in [|e|, |e| + 2] as long as the noise has not wrapped (NoiseBudget > 0)."""
        if msg is not None:
            return mkrlwe.Decryptor.NoiseNorm(self, ct, skSet, DeviceEncoder(self.params).Encode(msg.Value))
        T = int(self.params.T())
        return (self.InvariantNoise(ct, skSet) + T // 2) // T + 1

    def NoiseBits(self, ct, skSet, msg=None):
        """NoiseNorm(ct, skSet, msg).bit_length(): what the flood_bits of ShareNew (Decryptor, Refresher, PublicKeySwitcher) must exceed,
        by the statistical security parameter"""
        return self.NoiseNorm(ct, skSet, msg).bit_length()

    def MergeSharesMsg(self, ct, shares):
        """the merge of the shares of all parties -> Message.  With the device encoder the merged buffer goes straight to mkhe_bfv_decode."""
        pt = self.MergeShares(ct, shares)
        if isinstance(self.encoder, DeviceEncoder):
            return Message(self.encoder.Decode(pt))
        return Message(self.encoder.Decode(pt.download()[0]))


def NewDecryptor(params, encoder="host"):
    return Decryptor(params, encoder)


# ---- collective refresh (include/mkhe.h, "collective refresh for MK-BFV")
class Refresher:
    """The collective refresh of MK-BFV between parties: ShareNew (each party, on its own keys and its own DeviceSampler) and MergeNew (anyone)
    give a ciphertext of the same message over the same parties whose noise is that of a fresh encryption (RefreshNoiseBound); nobody sees the
    message.  A share is c_id * s_id + up(A) + e with A uniform mod T and e a flood of flood_bits bits, and comes with Encrypt(up(-A)); the
    merge rounds c_0 + the shares to Z_T, scales up again and adds the re-encryptions.  The caller chooses flood_bits (at most MaxFloodBits):
    flood_bits minus the bit size of the ciphertext's noise (Decryptor.NoiseBits) is the statistical hiding of that noise, which depends on the keys."""

    def __init__(self, params):
        self.params = params

    def _q(self):
        return _q_product(self.params)

    def MaxFloodBits(self, parties):
        """floor(log2(Q / (2 T parties))), capped at the 1024 bits the engine draws: the formula of Decryptor.MaxFloodBits.  With flood_bits up
        to this, parties * 2^(flood_bits - 1) <= Q / (4 T), which leaves the other half of the margin Q / (2 T) to the noise of the input"""
        return min(1024, (self._q() // (2 * int(self.params.T()) * int(parties))).bit_length() - 1)

    def RefreshNoiseBound(self, parties, sigma=3.2):
        """the noise of a refreshed ciphertext, at most: parties * (2N + 1) * floor(6 sigma) + (parties + 1) / 2 per coefficient.  Each party's
        fresh encryption adds |u e_pk + e0 + e1 s| <= (2N + 1) floor(6 sigma) (u and s ternary, the table truncated at floor(6 sigma)); the
        roundings of up add (parties + 1) / 2"""
        N, k = self.params.N(), int(parties)
        return k * (2 * N + 1) * int(6 * float(sigma)) + (k + 1) / 2

    def ShareBatch(self, cts, sk, pk, flood_bits, sampler):
        """The refresh shares of the party of (sk, pk) for B ciphertexts (their id sets may differ) as ONE engine call (mkhe_bfv_refresh_share,
        mask = 1) -> one mkrlwe.RefreshShare of count B.  Two nonces of `sampler` (a DeviceSampler) serve the call: one for mask and flood,
        one for the encryption."""
        cts = list(cts)
        if not cts:
            raise MkheError("Cannot RefreshShare: no ciphertext")
        if sk.ID != pk.ID:
            raise MkheError("Cannot RefreshShare: sk and pk belong to different parties")
        for ct in cts:
            if sk.ID not in ct.ids:
                raise MkheError("Cannot RefreshShare: the ciphertext has no component for the id of sk")
        if not isinstance(flood_bits, int) or not 0 <= flood_bits <= self.MaxFloodBits(1):
            raise MkheError("Cannot RefreshShare: flood_bits must be an integer 0 .. %d" % self.MaxFloodBits(1))
        if not isinstance(sampler, mkrlwe.DeviceSampler):
            raise MkheError("Cannot RefreshShare: mask, flood and encryption samples are drawn on the device -- pass a DeviceSampler")
        level = self.params.MaxLevel()
        key, nonce_mask, nonce_enc = sampler.refresh_args()
        out = mkrlwe.RefreshShare(self.params, sk.ID, level, level, len(cts))
        slots = (C.c_int * len(cts))(*[ct.slot(sk.ID) for ct in cts])
        check(lib().mkhe_bfv_refresh_share(self.params.ctx, len(cts), handle_array([ct.h for ct in cts]), slots, sk.Value.devptr(), pk.Value.devptr(),
                                           key, nonce_mask, nonce_enc, 1, flood_bits, sampler._cdt, len(sampler.cdt), out.Share.Value.devptr(),
                                           handle_array([c.h for c in out.Reenc])))
        return out

    def ShareNew(self, ct, sk, pk, flood_bits, sampler):
        """ShareBatch of one ciphertext"""
        return self.ShareBatch([ct], sk, pk, flood_bits, sampler)

    def MergeBatch(self, cts, shares):
        """The refreshed ciphertexts of B ciphertexts over the same ids: one RefreshShare of count B per party, in any order (ordering and
        errors: mkrlwe.order_shares) -> B ciphertexts over the same ids.  ONE engine call (mkhe_bfv_refresh_merge)."""
        cts = list(cts)
        if not cts:
            raise MkheError("Cannot RefreshMerge: no ciphertext")
        for ct in cts:
            if ct.ids != cts[0].ids:
                raise MkheError("Cannot RefreshMerge: the ciphertexts of one call must be over the same ids")
        ordered = mkrlwe.order_shares(cts[0].ids, self.params.MaxLevel(), len(cts), shares)
        outs = mkrlwe.batch_ciphertexts(Ciphertext, self.params, cts[0].ids, self.params.MaxLevel(), len(cts))
        reenc = [c.h for sh in ordered for c in sh.Reenc]
        check(lib().mkhe_bfv_refresh_merge(self.params.ctx, len(cts), handle_array([ct.h for ct in cts]), len(ordered),
                                           handle_array([sh.Share.Value.devptr() for sh in ordered]), handle_array(reenc) if reenc else None,
                                           handle_array([c.h for c in outs])))
        return outs

    def MergeNew(self, ct, shares):
        """MergeBatch of one ciphertext -> the refreshed ciphertext"""
        return self.MergeBatch([ct], shares)[0]

    # -- the refresh that applies a slot map: the message comes out as slot_map.apply(message), with no rotation key and no key switch.  The map is
    # Z_T-linear, so it commutes with the masks: every party maps its own -A before it encrypts, anyone maps the masked plaintext in the clear.
    def ShareMapBatch(self, cts, sk, pk, flood_bits, sampler, slot_map):
        """ShareBatch with slot_map (a SlotMap) applied to the mask that is re-encrypted: mkhe_bfv_e2s_share -> mkhe_bfv_slot_map ->
        mkhe_bfv_scale_up -> mkhe_encrypt_seeded, on the two nonces ShareBatch takes (nonce_mask = n, nonce_enc = n + 1) -> one
        mkrlwe.RefreshShare of count B.  With the identity map it is ShareBatch's, bit for bit.  The intermediate secret buffers are zeroed
        behind their last use."""
        cts = list(cts)
        if not cts:
            raise MkheError("Cannot RefreshShare: no ciphertext")
        if sk.ID != pk.ID:
            raise MkheError("Cannot RefreshShare: sk and pk belong to different parties")
        for ct in cts:
            if sk.ID not in ct.ids:
                raise MkheError("Cannot RefreshShare: the ciphertext has no component for the id of sk")
        if not isinstance(flood_bits, int) or not 0 <= flood_bits <= self.MaxFloodBits(1):
            raise MkheError("Cannot RefreshShare: flood_bits must be an integer 0 .. %d" % self.MaxFloodBits(1))
        if not isinstance(sampler, mkrlwe.DeviceSampler):
            raise MkheError("Cannot RefreshShare: mask, flood and encryption samples are drawn on the device -- pass a DeviceSampler")
        if not isinstance(slot_map, SlotMap):
            raise MkheError("Cannot RefreshShare: slot_map must be a mkbfv.SlotMap")
        B, level, ctx = len(cts), self.params.MaxLevel(), self.params.ctx
        key, nonce_mask, nonce_enc = sampler.refresh_args()
        out = mkrlwe.RefreshShare(self.params, sk.ID, level, level, B)
        sec, pt = SecretShare(self.params, sk.ID, B), mkrlwe.SecretShare(self.params, sk.ID, level, B)
        slots = (C.c_int * B)(*[ct.slot(sk.ID) for ct in cts])
        try:
            check(lib().mkhe_bfv_e2s_share(ctx, B, handle_array([ct.h for ct in cts]), slots, sk.Value.devptr(), key, nonce_mask, flood_bits,
                                           out.Share.Value.devptr(), sec.Value.devptr()))
            check(lib().mkhe_bfv_slot_map(ctx, B, sec.Value.devptr(), slot_map.devptr(), sec.Value.devptr()))
            check(lib().mkhe_bfv_scale_up(ctx, B, sec.Value.devptr(), pt.Value.devptr()))
            check(lib().mkhe_encrypt_seeded(ctx, level, B, pk.Value.devptr(), pt.Value.devptr(), 0, key, nonce_enc, sampler._cdt, len(sampler.cdt),
                                            handle_array([c.h for c in out.Reenc])))
        finally:
            sec.wipe()
            pt.wipe()
        return out

    def ShareMapNew(self, ct, sk, pk, flood_bits, sampler, slot_map):
        """ShareMapBatch of one ciphertext"""
        return self.ShareMapBatch([ct], sk, pk, flood_bits, sampler, slot_map)

    def MergeMapBatch(self, cts, shares, slot_map):
        """MergeBatch for shares made by ShareMapBatch with the same slot_map: ShareConverter.E2SMergeBatch (w = (m + sum A_i) mod T) ->
        mkhe_bfv_slot_map -> mkhe_bfv_scale_up, added (mkhe_bfv_ct_add_ptxt) into c_0 of the sum of the re-encryptions (mkhe_ct_add over the
        unions) -> B ciphertexts over the same ids that encrypt slot_map.apply(message).  With the identity map it is MergeBatch's, bit for bit."""
        if not isinstance(slot_map, SlotMap):
            raise MkheError("Cannot RefreshMerge: slot_map must be a mkbfv.SlotMap")
        cts = list(cts)
        if not cts:
            raise MkheError("Cannot RefreshMerge: no ciphertext")
        for ct in cts:
            if ct.ids != cts[0].ids:
                raise MkheError("Cannot RefreshMerge: the ciphertexts of one call must be over the same ids")
        B, level, nq, ctx = len(cts), self.params.MaxLevel(), self.params.QCount(), self.params.ctx
        ordered = mkrlwe.order_shares(cts[0].ids, level, B, shares)
        if not ordered:
            raise MkheError("Cannot RefreshMerge: ciphertexts without parties have nothing to refresh")
        w = ShareConverter(self.params).E2SMergeBatch(cts, [sh.Share for sh in ordered])
        pt = mkrlwe.DeviceLimbs(self.params, B, nq)
        check(lib().mkhe_bfv_slot_map(ctx, B, w.Value.devptr(), slot_map.devptr(), w.Value.devptr()))
        check(lib().mkhe_bfv_scale_up(ctx, B, w.Value.devptr(), pt.devptr()))
        acc, ids = list(ordered[0].Reenc), [ordered[0].ID]
        for sh in ordered[1:]:
            ids = sorted(set(ids) | {sh.ID})
            nxt = mkrlwe.batch_ciphertexts(Ciphertext, self.params, ids, level, B)
            check(lib().mkhe_ct_binary_batch(ctx, 0, B, handle_array([c.h for c in acc]), handle_array([c.h for c in sh.Reenc]),
                                             handle_array([c.h for c in nxt])))
            acc = nxt
        outs = mkrlwe.batch_ciphertexts(Ciphertext, self.params, cts[0].ids, level, B)
        check(lib().mkhe_bfv_ct_add_ptxt(ctx, 0, B, handle_array([c.h for c in acc]), pt.devptr(), nq * self.params.N(), handle_array([c.h for c in outs])))
        return outs

    def MergeMapNew(self, ct, shares, slot_map):
        """MergeMapBatch of one ciphertext -> the refreshed, mapped ciphertext"""
        return self.MergeMapBatch([ct], shares, slot_map)[0]


def NewRefresher(params):
    return Refresher(params)


# ---- encryption to shares and back; slot maps (include/mkhe.h, "encryption to shares", "BFV slot map")
class SecretShare(mkrlwe.SecretShare):
    """mkrlwe.SecretShare over Z_T: coefficients uint64 [count][1][N], each below T, in the format mkhe_bfv_scale_down writes; no level.
    Slots() is the share of the SLOTS (additive mod T slot by slot, as the transform is Z_T-linear)."""

    def __init__(self, params, id, count=1):
        super().__init__(params, id, None, count, limbs=1)

    def Slots(self):
        """-> int64 [count][N], centred, through mkhe_bfv_coeffs_to_slots"""
        dst = mkrlwe.DeviceLimbs(self.params, self.count, 1)
        check(lib().mkhe_bfv_coeffs_to_slots(self.params.ctx, self.count, self.Value.devptr(), dst.devptr()))
        return dst.download().view(np.int64).reshape(self.count, self.params.N())

    @classmethod
    def FromSlots(cls, params, values, id=None):
        """the inverse of Slots: int64 [count][N] (or [N]) -> SecretShare, through mkhe_bfv_slots_to_coeffs"""
        z = np.asarray(values, dtype=np.int64)
        z = z[None] if z.ndim == 1 else z
        if z.ndim != 2 or z.shape[0] < 1 or z.shape[1] != params.N():
            raise MkheError("mkbfv.SecretShare: expected %d slots per item, got %r" % (params.N(), z.shape))
        src = mkrlwe.DeviceLimbs(params, len(z), 1).upload(np.ascontiguousarray(z).view(np.uint64).reshape(len(z), 1, params.N()))
        out = cls(params, id, len(z))
        check(lib().mkhe_bfv_slots_to_coeffs(params.ctx, len(z), src.devptr(), out.Value.devptr()))
        return out


class ShareConverter:
    """HE <-> additive secret sharing over Z_T for MK-BFV, exact slot by slot.  E2S: every party runs E2SShareBatch on its own key and
    DeviceSampler, publishes the DecryptionShare and KEEPS the SecretShare (T - A); anyone runs E2SMergeBatch, which gives the public share
    w = (m + sum A_i) mod T.  (public + the sum of the secret shares) mod T is the message, coefficient by coefficient and -- after Slots() --
    slot by slot, as long as the noise of the ciphertext and the floods stay below Q / (2 T) (Refresher.MaxFloodBits).  S2E: every party
    encrypts its share (S2EShareBatch: mkhe_bfv_scale_up, then mkhe_encrypt / mkhe_encrypt_seeded), S2EMergeNew is the AddNew chain over the
    parties' ciphertexts, and the public share, scaled up, is added to the result as a plaintext (mkhe_bfv_ct_add_ptxt)."""

    def __init__(self, params):
        self.params = params

    def MaxFloodBits(self, parties):
        return Refresher(self.params).MaxFloodBits(parties)

    def E2SShareBatch(self, cts, sk, flood_bits, sampler):
        """The party of sk, for B ciphertexts (their id sets may differ), as ONE engine call (mkhe_bfv_e2s_share) -> (DecryptionShare to
        publish: Refresher.ShareBatch's, bit for bit; SecretShare to keep).  One nonce of `sampler` (a DeviceSampler)."""
        cts = list(cts)
        if not cts:
            raise MkheError("Cannot E2SShare: no ciphertext")
        for ct in cts:
            if sk.ID not in ct.ids:
                raise MkheError("Cannot E2SShare: the ciphertext has no component for the id of sk")
        if not isinstance(flood_bits, int) or not 0 <= flood_bits <= self.MaxFloodBits(1):
            raise MkheError("Cannot E2SShare: flood_bits must be an integer 0 .. %d" % self.MaxFloodBits(1))
        if not isinstance(sampler, mkrlwe.DeviceSampler):
            raise MkheError("Cannot E2SShare: mask and flood are drawn on the device -- pass a DeviceSampler")
        key, nonce = sampler.e2s_args()
        pub = mkrlwe.DecryptionShare(self.params, sk.ID, self.params.MaxLevel(), len(cts))
        sec = SecretShare(self.params, sk.ID, len(cts))
        slots = (C.c_int * len(cts))(*[ct.slot(sk.ID) for ct in cts])
        check(lib().mkhe_bfv_e2s_share(self.params.ctx, len(cts), handle_array([ct.h for ct in cts]), slots, sk.Value.devptr(), key, nonce,
                                       flood_bits, pub.Value.devptr(), sec.Value.devptr()))
        return pub, sec

    def E2SMergeBatch(self, cts, shares):
        """Anyone, for B ciphertexts over the same ids and one DecryptionShare of count B per party, in any order -> the public share, a
        SecretShare with id None: mkhe_decrypt_merge followed by mkhe_bfv_scale_down."""
        cts = list(cts)
        if not cts:
            raise MkheError("Cannot E2SMerge: no ciphertext")
        for ct in cts:
            if ct.ids != cts[0].ids:
                raise MkheError("Cannot E2SMerge: the ciphertexts of one call must be over the same ids")
        ordered = mkrlwe.order_shares(cts[0].ids, self.params.MaxLevel(), len(cts), shares)
        pt = mkrlwe.DeviceLimbs(self.params, len(cts), self.params.QCount())
        check(lib().mkhe_decrypt_merge(self.params.ctx, len(cts), handle_array([ct.h for ct in cts]), len(ordered),
                                       handle_array([sh.Value.devptr() for sh in ordered]), pt.devptr()))
        out = SecretShare(self.params, None, len(cts))
        check(lib().mkhe_bfv_scale_down(self.params.ctx, len(cts), pt.devptr(), out.Value.devptr()))
        return out

    def _scale_up(self, share):
        pt = mkrlwe.DeviceLimbs(self.params, share.count, self.params.QCount())
        check(lib().mkhe_bfv_scale_up(self.params.ctx, share.count, share.Value.devptr(), pt.devptr()))
        return pt

    def S2EShareBatch(self, secret, pk, sampler):
        """The party of pk encrypts its SecretShare under its own public key -> `count` ciphertexts over the party's id"""
        if secret.ID is not None and secret.ID != pk.ID:
            raise MkheError("Cannot S2EShare: the share and pk belong to different parties")
        enc = mkrlwe.Encryptor(self.params, sampler)
        level = self.params.MaxLevel()
        outs = mkrlwe.batch_ciphertexts(Ciphertext, self.params, [pk.ID], level, secret.count)
        enc._engine_encrypt(level, pk, self._scale_up(secret), False, enc._draw(None, secret.count), outs)
        return outs

    def S2EMergeNew(self, cts_by_party, public=None):
        """The AddNew chain over the parties' ciphertexts (one each) -> one ciphertext over all their ids; public (a SecretShare of count 1):
        scaled up and added to the result as a plaintext"""
        cts = list(cts_by_party)
        if not cts:
            raise MkheError("Cannot S2EMerge: no ciphertext")
        ev = Evaluator(self.params)
        acc = cts[0]
        for ct in cts[1:]:
            acc = ev.AddNew(acc, ct)
        if public is not None:
            if public.count != 1:
                raise MkheError("Cannot S2EMerge: the public share of one ciphertext expected")
            acc = ev.AddPtxtNew(acc, self._scale_up(public))
        return acc


def NewShareConverter(params):
    return ShareConverter(params)


class SlotMap:
    """out_slot[i] = mult[i] * in_slot[index[i]] mod T for 0 <= i < N, slots numbered as the batch encoder numbers them (two rows of N/2): any
    permutation, replication or slot-wise scaling.  index: N integers in 0 .. N-1, any function; mult: N integers taken mod T, default all
    ones.  The constructor checks on the host and touches no device; the device form (mkhe_bfv_slot_map_prepare) is prepared once, at the
    first use."""

    def __init__(self, params, index, mult=None):
        N, T = params.N(), int(params.T())
        idx = np.asarray(index)
        if idx.shape != (N,) or idx.dtype.kind not in "iu":
            raise MkheError("mkbfv.SlotMap: index must be %d integers, got %r of %s" % (N, idx.shape, idx.dtype))
        if len(idx) and (int(idx.min()) < 0 or int(idx.max()) >= N):
            raise MkheError("mkbfv.SlotMap: every index must be a slot 0 .. %d" % (N - 1))
        if mult is None:
            m = np.ones(N, dtype=np.uint64)
        else:
            m = mult if isinstance(mult, np.ndarray) else np.asarray(mult, dtype=object)      # (Python integers of any size)
            if m.shape != (N,) or m.dtype.kind not in "iuO" or not all(isinstance(x, (int, np.integer)) for x in m.tolist()):
                raise MkheError("mkbfv.SlotMap: mult must be %d integers, got %r of %s" % (N, m.shape, m.dtype))
            m = np.asarray([int(x) % T for x in m.tolist()], dtype=np.uint64)
        self.params, self.N, self.T = params, N, T
        self.index, self.mult = idx.astype(np.int64), m
        self._map = None

    @classmethod
    def Permutation(cls, params, perm, mult=None):
        """out_slot[i] = in_slot[perm[i]] for a permutation perm of 0 .. N-1"""
        p = np.asarray(perm)
        if p.shape != (params.N(),) or p.dtype.kind not in "iu" or not np.array_equal(np.sort(p), np.arange(params.N())):
            raise MkheError("mkbfv.SlotMap: Permutation takes a permutation of 0 .. %d" % (params.N() - 1))
        return cls(params, p, mult)

    @classmethod
    def Rotation(cls, params, k, swap_rows=False):
        """what RotateNew(ct, k) does to the slots: slot i + k moves to slot i within each row of N/2; swap_rows: and the rows change places
        (ConjugateNew)"""
        half = params.N() // 2
        i = np.arange(params.N())
        row = (i // half) ^ (1 if swap_rows else 0)
        return cls(params, row * half + (i % half + int(k)) % half)

    def apply(self, values):
        """the host definition: (mult * values[index]) mod T, centred, int64 [N] (or [count][N])"""
        v = np.asarray(values, dtype=np.int64)
        if v.shape[-1] != self.N:
            raise MkheError("mkbfv.SlotMap: expected %d slots, got %r" % (self.N, v.shape))
        r = (np.mod(v, self.T).astype(np.uint64)[..., self.index] * self.mult) % np.uint64(self.T)        # both below 2^32: the product fits
        r = r.astype(np.int64)
        return np.where(r > self.T // 2, r - self.T, r)

    def devptr(self):
        if self._map is None:
            N = self.N
            words = mkrlwe.DeviceLimbs(self.params, 2, 1)                     # row 0: the index as uint32 [N] (half a row), row 1: mult
            host = np.zeros((2, 1, N), dtype=np.uint64)
            host[0, 0, : N // 2] = self.index.astype(np.uint32).view(np.uint64)
            host[1, 0] = self.mult
            words.upload(host)
            m = mkrlwe.DeviceLimbs(self.params, 1, 1)
            check(lib().mkhe_bfv_slot_map_prepare(self.params.ctx, words.devptr(), C.c_void_p(words.devptr().value + 8 * N), m.devptr()))
            self._map = m
        return self._map.devptr()

    def MapCoeffs(self, secret_share):
        """the map applied to a SecretShare (coefficients over Z_T) -> a new SecretShare of the same party: ONE engine call (mkhe_bfv_slot_map)"""
        out = SecretShare(self.params, secret_share.ID, secret_share.count)
        check(lib().mkhe_bfv_slot_map(self.params.ctx, secret_share.count, secret_share.Value.devptr(), self.devptr(), out.Value.devptr()))
        return out


class PublicKeySwitcher(mkrlwe.PublicKeySwitcher):
    """The collective key switch of mkrlwe.PublicKeySwitcher on mkbfv ciphertexts: the result is a mkbfv.Ciphertext over the recipient's id.  The
    message stays exact as long as NoiseBound plus the noise of the input is below Q / (2 T)."""

    def _t(self):
        return int(self.params.T())

    def _out(self, like, count, recipient_id):
        return mkrlwe.batch_ciphertexts(Ciphertext, self.params, [recipient_id], self.params.MaxLevel(), count)

    def MaxFloodBits(self, parties=1):
        """floor(log2(Q / (2 T parties))), capped at the 1024 bits the engine draws: the formula of Refresher.MaxFloodBits.  With flood_bits up
        to this, parties * 2^(flood_bits - 1) <= Q / (4 T), which leaves the other half of the margin Q / (2 T) to the noise of the input
        (parties = 1: the widest flood the engine takes)"""
        return min(1024, (_q_product(self.params) // (2 * int(self.params.T()) * int(parties))).bit_length() - 1)


def NewPublicKeySwitcher(params):
    return PublicKeySwitcher(params)


# ---- threshold secret keys (include/mkhe.h, "threshold secret keys"): keys are the ring's, so the classes are mkrlwe's
SecretKeyShare = mkrlwe.SecretKeyShare
Thresholdizer = mkrlwe.Thresholdizer
Combiner = mkrlwe.Combiner
NewThresholdizer = mkrlwe.NewThresholdizer
NewCombiner = mkrlwe.NewCombiner
