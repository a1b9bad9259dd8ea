"""Host-side mirror of the reference package `mkckks` (Evaluator hot methods).

Orchestration and float64 scale bookkeeping stay on the host exactly as in
mkckks/evaluator.go:359-443,543-617; all polynomial work runs on the device via mkrlwe.KeySwitcher.
"""
import collections
import ctypes as C
import math

import numpy as np

from . import _abi, mkrlwe
from ._abi import MkheError, check, handle_array, lib


def scaleUpExact(value, n, q):
    """mkckks/utils.go:59-86: round(|value| * n) mod q through a 53-bit big.Float (= float64 arithmetic), negated
    for value < 0 (q - 0 = q is kept, like the reference)."""
    x = float(-n * value) if value < 0 else float(n * value)
    res = int(x + 0.5) % q
    return q - res if value < 0 else res


def _check_log_slots(who, logSlots, logN):
    if isinstance(logSlots, bool) or int(logSlots) != logSlots or not 0 <= logSlots <= logN - 1:
        raise MkheError("%s: logSlots must lie between 0 and logN - 1 = %d, got %r" % (who, logN - 1, logSlots))


class Parameters(mkrlwe.Parameters):
    """mkckks.Parameters (mkckks/params.go:11-24): mkrlwe parameters with gamma = 2 + default scale.  logSlots (default logN - 1, full packing):
    messages have 2^logSlots slots (sparse packing below logN - 1: Encoder)."""

    def __init__(self, logN, Q, P, scale, logSlots=None, psiQ=None, psiP=None, device=0):
        logSlots = logN - 1 if logSlots is None else logSlots
        _check_log_slots("mkckks.Parameters", logSlots, logN)          # (before the context is opened)
        super().__init__(logN, Q, P, gamma=2, psiQ=psiQ, psiP=psiP, device=device)
        self._scale = float(scale)
        self.logSlots = int(logSlots)

    def Scale(self): return self._scale
    def LogSlots(self): return self.logSlots


class Ciphertext(mkrlwe.Ciphertext):
    """mkckks.Ciphertext (mkckks/elements.go:5-17): mkrlwe.Ciphertext + Scale."""

    def __init__(self, params, idset, level, scale, zero=True):
        super().__init__(params, idset, level, zero)
        self.Scale = float(scale)

    def ScalingFactor(self):
        return self.Scale


def NewCiphertext(params, idset, level, scale, zero=True):
    return Ciphertext(params, idset, level, scale, zero)


class Evaluator:
    """mkckks.Evaluator (mkckks/evaluator.go:13-39)."""

    def __init__(self, params):
        self.params = params
        self.ksw = mkrlwe.NewKeySwitcher(params)
        self.fuse_rescale = True          # MulRelin[Hoisted]New: the single Rescale inside the engine call (False: two calls, for A/B tests)

    def Fork(self):
        """an evaluator on a forked context (mkrlwe.Parameters.Fork): same keys and ciphertexts, its own stream"""
        return Evaluator(self.params.Fork())

    def newCiphertextBinary(self, op0, op1):
        """evaluator.go:306-313"""
        return NewCiphertext(self.params, op0.IDSet() | op1.IDSet(), min(op0.Level(), op1.Level()),
                             max(op0.ScalingFactor(), op1.ScalingFactor()), zero=False)      # every limb is written by the engine call that follows

    # ---- AddNew / SubNew (evaluator.go:316-357 -> evaluateInPlace :200-304)
    def _binary(self, op0, op1, fn):
        s0, s1 = op0.ScalingFactor(), op1.ScalingFactor()
        # scale matching (evaluateInPlace :270-292, the branch for a fresh ctOut): the operand with the smaller scale is
        # first multiplied by floor(ratio) when that is > 1 -- MultByConst with an integer-valued float64, i.e. constant scale 1
        # -- into a pool element; the result carries max(s0, s1) like the reference's (the residual factor is not tracked)
        if s1 > s0 and math.floor(s1 / s0) > 1:
            tmp = NewCiphertext(self.params, op0.ids, op0.Level(), s0, zero=False)
            self.MultByConst(op0, float(math.floor(s1 / s0)), tmp)
            op0 = tmp
        elif s0 > s1 and math.floor(s0 / s1) > 1:
            tmp = NewCiphertext(self.params, op1.ids, op1.Level(), s1, zero=False)
            self.MultByConst(op1, float(math.floor(s0 / s1)), tmp)
            op1 = tmp
        ctOut = self.newCiphertextBinary(op0, op1)
        ctOut.Scale = max(s0, s1)
        check(fn(self.params.ctx, op0.h, op1.h, ctOut.h))
        return ctOut

    def AddNew(self, op0, op1):
        return self._binary(op0, op1, lib().mkhe_ct_add)

    def SubNew(self, op0, op1):
        return self._binary(op0, op1, lib().mkhe_ct_sub)

    # ---- getConstAndScale (evaluator.go:40-94)
    def getConstAndScale(self, level, constant):
        scale = 1.0
        if isinstance(constant, complex):
            cReal, cImag = constant.real, constant.imag
            for c in (cReal, cImag):
                if c != 0 and c - float(int(c)) != 0:
                    scale = float(self.params.Q[level])
        elif isinstance(constant, float):
            cReal, cImag = constant, 0.0
            if cReal != 0 and cReal - float(int(cReal)) != 0:
                scale = float(self.params.Q[level])
        else:
            cReal, cImag = float(int(constant)), 0.0
        return cReal, cImag, scale

    # ---- MultByConst (evaluator.go:117-199): constants per limb on the host, the products on the device
    def MultByConst(self, ct0, constant, ctOut):
        params = self.params
        level = min(ct0.Level(), ctOut.Level())
        cReal, cImag, scale = self.getConstAndScale(level, constant)
        first = np.zeros(ctOut.Level() + 1, dtype=np.uint64)
        second = np.zeros(ctOut.Level() + 1, dtype=np.uint64)
        R = 1 << 64
        for i in range(level + 1):
            qi = params.Q[i]
            sReal = scaleUpExact(cReal, scale, qi) if cReal != 0 else 0
            sConst, sImag = sReal, 0
            if cImag != 0:
                # MRed(scaleUpExact(cImag), NttPsi[i][1]): NttPsi[i][1] = psi^(N/2) * R, so the product is plain
                sImag = (scaleUpExact(cImag, scale, qi) * pow(params.Psi(i), params.N() // 2, qi)) % qi
                sConst = (sConst + sImag) % qi if sConst + sImag >= qi else sConst + sImag            # CRed
            first[i] = (sConst % qi) * R % qi                                                       # MForm
            c2 = sConst
            if cImag != 0:
                c2 = sReal + (qi - sImag)
                c2 = c2 - qi if c2 >= qi else c2                                                     # CRed
            second[i] = (c2 % qi) * R % qi
        check(lib().mkhe_ct_mul_const(params.ctx, ct0.h, first.ctypes.data_as(_abi.u64p), second.ctypes.data_as(_abi.u64p), ctOut.h))
        ctOut.Scale = ct0.Scale * scale

    # ---- DropLevelNew (evaluator.go:96-114): keep the first level+1-levels limbs of every component
    def DropLevelNew(self, ct0, levels):
        out = NewCiphertext(self.params, ct0.IDSet(), ct0.Level() - levels, ct0.Scale, zero=False)
        one = np.array([(1 << 64) % q for q in self.params.Q[: out.Level() + 1]], dtype=np.uint64)      # MForm(1): x * 1
        check(lib().mkhe_ct_mul_const(self.params.ctx, ct0.h, one.ctypes.data_as(_abi.u64p), one.ctypes.data_as(_abi.u64p), out.h))
        return out

    # ---- MulPtxtNew (evaluator.go:465-481); pt: host polynomial uint64[level+1][N] (coefficient domain) + its scale
    def MulPtxtNew(self, ct, pt_value, pt_scale):
        params = self.params
        level = ct.Level()
        ctOut = NewCiphertext(params, ct.IDSet(), level, ct.Scale * float(pt_scale), zero=False)
        if isinstance(pt_value, mkrlwe.DeviceLimbs):          # already resident (uploaded once by the caller, or DeviceEncoder.Encode's; required inside a graph capture)
            pt = pt_value
            if pt.limbs != level + 1:
                raise MkheError("MulPtxtNew: the resident plaintext must have level + 1 limbs")
        else:
            pt = mkrlwe.DeviceLimbs(params, 1, level + 1).upload(np.ascontiguousarray(pt_value, dtype=np.uint64)[None, : level + 1])
        check(lib().mkhe_ct_mul_ptxt(params.ctx, ct.h, pt.devptr(), ctOut.h))
        if ctOut.Level() == 0:                 # eval.Rescale returns an error there; MulPtxtNew ignores it (:480)
            return ctOut
        nb, scale = self.nbRescales(ctOut, params.Scale())
        if nb == 0:
            return ctOut
        res = NewCiphertext(params, ctOut.IDSet(), level - nb, scale, zero=False)
        check(lib().mkhe_rescale(params.ctx, ctOut.h, nb, res.h))
        return res

    # ---- Rescale (evaluator.go:359-398)
    def nbRescales(self, ctIn, minScale):
        return self._nb_rescales(ctIn.Level(), ctIn.Scale, minScale)

    def _nb_rescales(self, level, scale, minScale):
        Q = self.params.Q
        nb = 0
        while level - nb >= 0 and scale / float(Q[level - nb]) >= minScale / 2:
            scale /= float(Q[level - nb])
            nb += 1
        return nb, scale

    def RescaleNew(self, ct0, threshold):
        if threshold <= 0:
            raise MkheError("cannot Rescale: minScale is 0")
        if ct0.Scale == 0:
            raise MkheError("cannot Rescale: ciphertext scale is 0")
        if ct0.Level() == 0:
            raise MkheError("cannot Rescale: input Ciphertext already at level 0")
        nb, scale = self.nbRescales(ct0, threshold)
        out = NewCiphertext(self.params, ct0.IDSet(), ct0.Level() - nb, scale, zero=False)
        check(lib().mkhe_rescale(self.params.ctx, ct0.h, nb, out.h))
        return out

    # ---- HoistedForm (evaluator.go:543-553)
    def HoistedForm(self, ct):
        h = mkrlwe.NewHoistedCiphertext()
        for id in ct.ids:
            h.Value[id] = mkrlwe.SwitchingKey(self.params, zero=False)          # every digit the level uses is written below
        check(lib().mkhe_hoisted_form(self.params.ctx, ct.Level(), ct.h, handle_array([h.Value[id].h for id in ct.ids])))   # one batched launch
        return h

    # ---- MulRelinNew (evaluator.go:416-443): hoisting of both operands happens inside the engine
    def MulRelinNew(self, op0, op1, rlkSet):
        return self.MulRelinHoistedNew(op0, op1, None, None, rlkSet)

    # ---- MulRelinHoistedNew / mulRelinHoisted (evaluator.go:558-581)
    def MulRelinHoistedNew(self, op0, op1, op0Hoisted, op1Hoisted, rlkSet):
        level, prod_scale = min(op0.Level(), op1.Level()), op0.ScalingFactor() * op1.ScalingFactor()
        # the number of rescales depends on scales and moduli only (evaluator.go:359-398): the usual single one is folded into the
        # engine call (mkhe_mul_relin_rescale: the DivRoundByLastModulus rides on the last ModDown's store), bit-identical to the two calls
        nb1, scale1 = self._nb_rescales(level, prod_scale, self.params.Scale())
        if nb1 == 1 and level >= 1 and self.fuse_rescale:
            res = NewCiphertext(self.params, op0.IDSet() | op1.IDSet(), level - 1, scale1, zero=False)
            self.ksw.MulAndRelinHoisted(op0, op1, op0Hoisted, op1Hoisted, rlkSet, res, rescaled=True)
            return res
        ctOut = NewCiphertext(self.params, op0.IDSet() | op1.IDSet(), level, prod_scale, zero=False)      # newCiphertextBinary, :306-313
        self.ksw.MulAndRelinHoisted(op0, op1, op0Hoisted, op1Hoisted, rlkSet, ctOut)
        nb, scale = self.nbRescales(ctOut, self.params.Scale())
        if nb == 0 or ctOut.Level() == 0:
            return ctOut
        res = NewCiphertext(self.params, ctOut.IDSet(), ctOut.Level() - nb, scale, zero=False)
        check(lib().mkhe_rescale(self.params.ctx, ctOut.h, nb, res.h))
        return res

    # ---- sum_k MulRelin(ops0[k], ops1[k]) under ONE relinearisation tail (no reference counterpart: cnn.Convolution / FC1Layer, cnn/cnn.go:16-31,51-61,
    # relinearise every summand; mkhe_mul_relin_sum).  A different ciphertext of the same sum: one gadget noise of step F2 instead of K
    def MulRelinSumNew(self, ops0, ops1, rlkSet, hoisted0=None, hoisted1=None):
        ops0, ops1 = list(ops0), list(ops1)
        if len(ops0) != len(ops1) or not ops0:
            raise MkheError("MulRelinSumNew: as many first operands as second ones, at least one pair")
        if len(ops0) > MULRELIN_SUM_MAX:
            raise MkheError("MulRelinSumNew: at most %d pairs per call" % MULRELIN_SUM_MAX)
        prod_scale = ops0[0].ScalingFactor() * ops1[0].ScalingFactor()
        for a, b in zip(ops0, ops1):
            if a.ScalingFactor() * b.ScalingFactor() != prod_scale:
                raise MkheError("MulRelinSumNew: all products must have one scale")
        level = min(min(c.Level() for c in ops0), min(c.Level() for c in ops1))
        ids = ops0[0].IDSet() | ops1[0].IDSet()
        nb1, scale1 = self._nb_rescales(level, prod_scale, self.params.Scale())          # as MulRelinHoistedNew, fuse_rescale included
        if nb1 == 1 and level >= 1 and self.fuse_rescale:
            res = NewCiphertext(self.params, ids, level - 1, scale1, zero=False)
            self.ksw.MulRelinSum(ops0, ops1, hoisted0, hoisted1, rlkSet, res, rescaled=True)
            return res
        ctOut = NewCiphertext(self.params, ids, level, prod_scale, zero=False)
        self.ksw.MulRelinSum(ops0, ops1, hoisted0, hoisted1, rlkSet, ctOut)
        nb, scale = self.nbRescales(ctOut, self.params.Scale())
        if nb == 0 or ctOut.Level() == 0:
            return ctOut
        res = NewCiphertext(self.params, ctOut.IDSet(), ctOut.Level() - nb, scale, zero=False)
        check(lib().mkhe_rescale(self.params.ctx, ctOut.h, nb, res.h))
        return res

    def _norm_rot(self, rotidx):
        n2 = self.params.N() // 2
        return rotidx % n2

    # ---- RotateNew (evaluator.go:485-525)
    def RotateNew(self, ct0, rotidx, rkSet):
        rotidx = self._norm_rot(rotidx)
        ctOut = NewCiphertext(self.params, ct0.IDSet(), ct0.Level(), ct0.Scale, zero=False)
        if rotidx == 0:
            check(lib().mkhe_ct_copy(self.params.ctx, ct0.h, ctOut.h))
            return ctOut
        if rotidx in self.params.CRS:
            self.ksw.Rotate(ct0, rotidx, rkSet, ctOut)
            return ctOut
        ctTmp, k = ct0, 1
        while rotidx > 0:                                   # power-of-two decomposition, :516-523
            if rotidx % 2:
                nxt = NewCiphertext(self.params, ct0.IDSet(), ct0.Level(), ct0.Scale, zero=False)
                self.ksw.Rotate(ctTmp, k, rkSet, nxt)
                ctTmp = nxt
            rotidx //= 2
            k *= 2
        return ctTmp

    # ---- RotateHoistedNew (evaluator.go:585-617)
    def RotateHoistedNew(self, ct0, rotidx, ct0Hoisted, rkSet):
        rotidx = self._norm_rot(rotidx)
        ctOut = NewCiphertext(self.params, ct0.IDSet(), ct0.Level(), ct0.Scale, zero=False)
        if rotidx == 0:
            check(lib().mkhe_ct_copy(self.params.ctx, ct0.h, ctOut.h))
            return ctOut
        if rotidx not in self.params.CRS:
            raise MkheError("Hoisted rotation only works for precomputed rotation keys")
        self.ksw.RotateHoisted(ct0, rotidx, ct0Hoisted, rkSet, ctOut)
        return ctOut

    # ---- ConjugateNew (evaluator.go:527-541)
    def ConjugateNew(self, ct0, ckSet):
        ctOut = NewCiphertext(self.params, ct0.IDSet(), ct0.Level(), ct0.Scale, zero=False)
        self.ksw.Conjugate(ct0, ckSet, ctOut)
        return ctOut

    # ---- AddNew(ct0, RotateNew(ct0, rotidx, rkSet)): the step every log-sum of cnn/cnn.go repeats (:33-37,64-67,83-86,90-93) as ONE engine call --
    # the ring.Add rides on the store of the rotation's ModDown (mkhe_rotate_multi with post_add).  Same integers as the two calls.
    def RotateAndAddNew(self, ct0, rotidx, rkSet):
        rotidx = self._norm_rot(rotidx)
        if rotidx == 0:
            return self.AddNew(ct0, self.RotateNew(ct0, 0, rkSet))
        ctTmp, k, steps = ct0, 1, []
        if rotidx in self.params.CRS:
            steps = [rotidx]
        else:
            r = rotidx
            while r > 0:                                    # power-of-two decomposition, :516-523: the addition joins the LAST rotation
                if r % 2:
                    steps.append(k)
                r //= 2
                k *= 2
        for s in steps[:-1]:
            nxt = NewCiphertext(self.params, ct0.IDSet(), ct0.Level(), ct0.Scale, zero=False)
            self.ksw.Rotate(ctTmp, s, rkSet, nxt)
            ctTmp = nxt
        last = steps[-1]
        if last not in self.params.CRS:
            raise MkheError("mkhe: no CRS for rotation index %d" % last)
        ctOut = NewCiphertext(self.params, ct0.IDSet(), ct0.Level(), ct0.Scale, zero=False)
        rk = [rkSet.GetRotationKey(i, last).Value.h for i in ct0.ids]
        gal = (C.c_uint64 * 1)(self.params.GaloisElementForColumnRotationBy(last))
        check(lib().mkhe_rotate_multi(self.params.ctx, 1, gal, handle_array([ctTmp.h]), None, handle_array(rk), handle_array([self.params.CRS[last].h]),
                                      handle_array([ct0.h]), handle_array([ctOut.h])))
        return ctOut

    # ---- out = cts[0]; for c in cts[1:]: out = AddNew(out, c) -- the sum over the products of a layer (cnn/cnn.go:19-30,58-62) -- as ONE launch
    # when the summands have one shape and one scale (then every AddNew is a plain ring.Add per component); the chain itself otherwise.
    def SumNew(self, cts):
        cts = list(cts)
        c0 = cts[0]
        if len(cts) == 1 or any(c.ids != c0.ids or c.Level() != c0.Level() or c.Scale != c0.Scale for c in cts):
            out = c0
            for c in cts[1:]:
                out = self.AddNew(out, c)
            return out
        out = NewCiphertext(self.params, c0.IDSet(), c0.Level(), c0.Scale, zero=False)
        check(lib().mkhe_ct_sum(self.params.ctx, len(cts), handle_array([c.h for c in cts]), out.h))
        return out

    def Lanes(self, n):
        """n independent operations of one shape on THIS context as one launch set (a BatchEvaluator over the same stream): how the device runs the
        independent chains of cnn.Convolution / FC1Layer -- small kernels do not overlap each other on this chip, lanes make them one kernel"""
        hit = self.__dict__.setdefault("_lanes", {}).get(n)
        if hit is None:
            hit = self._lanes[n] = BatchEvaluator(self.params, n, ev=self)
        return hit

    # ---- weighted sums, additive constants and polynomials (no reference counterpart: its evaluator multiplies by a constant and squares, nothing else).
    # Everything goes through mkhe_ct_lincomb, where i is the monomial X^(N/2) of the coefficient domain -- NOT MultByConst's half-split.
    def LinCombNew(self, cts, weights, const=0, scale=None, rescale=True, level=None):
        """sum_k weights[k] * cts[k] + const (complex weights and constant) as ONE engine call, with an EXACT declared scale: weight k is encoded at
        S_mid / cts[k].Scale, whatever scales the summands carry, so the sum is at S_mid.  rescale=True: S_mid = scale * Q[l] and the result, one level
        below the work level l, has Scale == scale; rescale=False: S_mid = scale, the result stays at level l.  l = the lowest level among cts (or the
        lower `level`: the summands' higher limbs are not read); scale defaults to params.Scale().  A weight that is exactly zero drops its ciphertext.
        The constants are encoded and uploaded here, once per call: not inside a graph capture."""
        params = self.params
        terms, l, scale, block = _lincomb_plan(params, cts, weights, const, scale, rescale, level)
        buf = _upload_consts(params, block)
        out = NewCiphertext(params, terms[0].IDSet(), l - (1 if rescale else 0), scale, zero=False)
        check(lib().mkhe_ct_lincomb(params.ctx, len(terms), handle_array([c.h for c in terms]), buf.devptr(), 1 if rescale else 0, out.h))
        return out

    def LinCombsNew(self, cts, weight_rows, consts, scales=None, rescale=True, level=None):
        """[sum_b weight_rows[g][b] * cts[b] + consts[g] for every g] as ONE engine call (mkhe_ct_lincomb_multi) with ONE constants upload: 1 to 16 rows
        of complex weights over the same ciphertexts, one complex constant each.  Row g follows the rules of LinCombNew -- weight b encoded at S_mid_g /
        cts[b].Scale, the result at Scale == scales[g] exactly (one float for all rows, or one per row; default params.Scale()) -- and equals
        LinCombNew(cts, weight_rows[g], consts[g], scale=scales[g], rescale=rescale, level=level) bit for bit.  All rows share the work level and
        `rescale`.  A ciphertext whose weight is zero in every row is dropped (at most 16 may remain); zeros inside the table stay, the kernel skips
        them.  MkheError before any engine call on a shape error.  Not inside a graph capture (the constants are uploaded here)."""
        params = self.params
        terms, l, scales, block = _lincombs_plan(params, cts, weight_rows, consts, scales, rescale, level)
        buf = _upload_consts(params, block)
        outs = [NewCiphertext(params, terms[0].IDSet(), l - (1 if rescale else 0), s, zero=False) for s in scales]
        check(lib().mkhe_ct_lincomb_multi(params.ctx, len(terms), handle_array([c.h for c in terms]), len(scales), buf.devptr(), 1 if rescale else 0,
                                          handle_array([o.h for o in outs])))
        return outs

    def AddConstNew(self, ct, c):
        """ct + c for a complex constant c: the weight 1 at ratio 1 is the integer 1, so the ciphertext part is unchanged bit for bit"""
        return self.LinCombNew([ct], [1], c, scale=ct.Scale, rescale=False)

    def MulRelinOnceNew(self, op0, op1, rlkSet, scale=None):
        """MulRelinNew where its Rescale count is the usual one; where the scales would make it another number, the product with exactly ONE Rescale all
        the same (a node of a polynomial evaluation fixes the level).  scale: the declared scale of the result when the caller knows it exactly."""
        level, prod = min(op0.Level(), op1.Level()), op0.ScalingFactor() * op1.ScalingFactor()
        if level < 1:
            raise MkheError("cannot Rescale: input Ciphertext already at level 0")
        if self._nb_rescales(level, prod, self.params.Scale())[0] == 1:
            res = self.MulRelinNew(op0, op1, rlkSet)
        else:
            res = NewCiphertext(self.params, op0.IDSet() | op1.IDSet(), level - 1, prod / float(self.params.Q[level]), zero=False)
            self.ksw.MulAndRelinHoisted(op0, op1, None, None, rlkSet, res, rescaled=True)
        if scale is not None:
            res.Scale = float(scale)
        return res

    def MulRelinRawNew(self, op0, op1, rlkSet):
        """the relinearised product at level min(levels) with Scale = the product of the scales and NO Rescale (a node of a Chebyshev recurrence folds
        the division into the LinCombNew that follows it)"""
        level = min(op0.Level(), op1.Level())
        res = NewCiphertext(self.params, op0.IDSet() | op1.IDSet(), level, op0.ScalingFactor() * op1.ScalingFactor(), zero=False)
        self.ksw.MulAndRelinHoisted(op0, op1, None, None, rlkSet, res, rescaled=False)
        return res

    def EvaluatePolyNew(self, ct, coeffs, rlkSet, scale=None, fused=False):
        """sum_k coeffs[k] * ct^k (monomial basis, real or complex coefficients, degree 1 .. 63) by baby steps and giant steps (poly_eval_plan): the result
        has Scale == scale (default params.Scale()) exactly and level ct.Level() - (ceil(log2(degree + 1)) + 1); MkheError before any engine call when
        that is below 0.  fused=True: the inner sums of the giant products come from ONE LinCombsNew instead of one LinCombNew each -- the same
        ciphertext bit for bit."""
        return evaluate_poly(self, ct, coeffs, rlkSet, scale, fused)

    def EvaluateChebyshevNew(self, ct, coeffs, interval, rlkSet, scale=None, fused=True):
        """sum_k coeffs[k] * T_k((2 x - a - b) / (b - a)) for the slots x of ct in the real interval (a, b) = interval (Chebyshev basis, degree 1 .. 255;
        chebyshev_approx gives the coefficients of a function): the change of variable (one LinCombNew and one level, skipped for (-1, 1)), the powers
        T_k by T_(a'+b') = 2 T_a' T_b' - T_|a'-b'| on the schedule of poly_eval_plan, the inner sums of chebyshev_blocks, the giant products.  The
        result has Scale == scale (default params.Scale()) exactly and level ct.Level() - (change of variable: 0 or 1) - (ceil(log2(degree + 1)) + 1);
        MkheError before any engine call when that is below 0, on the zero polynomial or when a >= b.  fused=True: the inner sums of the giant products
        are ONE LinCombsNew; fused=False: one LinCombNew each, the same ciphertext bit for bit."""
        return evaluate_chebyshev(self, ct, coeffs, interval, rlkSet, scale, fused)

    def LinearTransformNew(self, ct, lt, rkSet, fused=True):
        """M z for the cleartext diagonals of `lt` (LinearTransform): sum_g rot_g(sum_b d'_(g,b) (.) rot_b ct) with one Rescale, the result at level
        lt.level - 1 and at Scale lt.out_scale exactly when ct.Scale == lt.in_scale (ct.Scale * lt.pt_scale / Q[lt.level] otherwise).  MkheError before any
        engine call when ct lies below lt.level, lt.level < 1 or a CRS / rotation key of lt.Rotations() is missing.  fused=False runs the same schedule
        through the single-operation entry points (it needs LinearTransform(.., keep_coeff=True)) and gives the same ciphertext bit for bit."""
        return linear_transform(self, ct, lt, rkSet, fused)

    def FactoredTransformNew(self, ct, ft, rkSet, fused=True):
        """F_f .. F_1 z for the factors of `ft` (FactoredTransform): LinearTransformNew on each factor in turn, ft.Depth() levels; the result is at level
        ft.level - ft.Depth() and at Scale ft.out_scale exactly when ct.Scale == ft.in_scale.  MkheError before any engine call when a CRS / rotation key
        of ft.Rotations() is missing; fused as in LinearTransformNew."""
        return factored_transform(self, ct, ft, rkSet, fused)

    # ---- the two ciphertext steps that open a bootstrapping (no reference counterpart; Bootstrapper below composes the rest)
    def ModRaiseNew(self, ct, level=None):
        """the level-0 ciphertext ct, read as its centred representatives mod Q[0], at `level` (default: the top) as ONE engine call (mkhe_ct_mod_raise).
        Its phase there is m + e + Q[0] I for a small integer polynomial I; the Scale is unchanged."""
        level = self.params.MaxLevel() if level is None else int(level)
        if ct.Level() != 0:
            raise MkheError("ModRaiseNew: the ciphertext must be at level 0, it is at level %d" % ct.Level())
        if not 1 <= level <= self.params.MaxLevel():
            raise MkheError("ModRaiseNew: the target level must lie between 1 and %d" % self.params.MaxLevel())
        out = NewCiphertext(self.params, ct.IDSet(), level, ct.Scale, zero=False)
        check(lib().mkhe_ct_mod_raise(self.params.ctx, ct.h, out.h))
        return out

    def SubSumNew(self, ct, rkSet):
        """the trace onto the sub-ring of X^gap, gap = N / 2n, n = 2^params.LogSlots(): log2(gap) calls of RotateAndAddNew, by n, 2n, 4n, .. (X -> X^(5^n)
        generates the automorphisms that fix X^gap).  A coefficient on the grid is multiplied by gap, every other one cancels; the declared Scale is
        ct.Scale * gap (exact: gap is a power of two), so the slots read the same.  Full packing: ct itself."""
        n, half = 1 << self.params.LogSlots(), self.params.N() // 2
        if n == half:
            return ct
        out, r = ct, n
        while r < half:
            out = self.RotateAndAddNew(out, r, rkSet)
            r *= 2
        out.Scale = ct.Scale * (half // n)
        return out


MULRELIN_SUM_MAX = 16     # pairs per mkhe_mul_relin_sum call (csrc/poly_kernels.h, TSUM_MAX_K)
LINCOMB_MAX = 16          # ciphertexts per mkhe_ct_lincomb call (csrc/poly_kernels.h, CTLIN_MAX)
LINCOMBS_MAX_OUT = 16     # rows per mkhe_ct_lincomb_multi call (csrc/poly_kernels.h, CTLM_MAX_OUT)
CHEBYSHEV_MAX_DEGREE = 255
PolyEvalPlan = collections.namedtuple("PolyEvalPlan", "degree m g products depth")


def lincomb_consts(Q, s_mid, const, scales, weights):
    """One constant block of mkhe_ct_lincomb, uint64 [n + 1][2][len(Q)], a pure function: row 0 = the complex constant at s_mid as plain residues, row
    1 + k = weights[k] at s_mid / scales[k] in Montgomery form (scaleUpExact, the rounding of the reference's constants)."""
    const = complex(const)
    out = np.zeros((len(weights) + 1, 2, len(Q)), dtype=np.uint64)
    for i, q in enumerate(Q):
        out[0, 0, i], out[0, 1, i] = scaleUpExact(const.real, s_mid, q) % q, scaleUpExact(const.imag, s_mid, q) % q
        for k, (s, w) in enumerate(zip(scales, weights)):
            w, ratio = complex(w), s_mid / s
            out[k + 1, 0, i] = ((scaleUpExact(w.real, ratio, q) % q) << 64) % q              # MForm
            out[k + 1, 1, i] = ((scaleUpExact(w.imag, ratio, q) % q) << 64) % q
    return out


def _lincomb_plan(params, cts, weights, const, scale, rescale, level):
    """the checks of LinCombNew and its constant block, before any engine call, on ciphertexts or batches of them (anything with ids, Level() and Scale)
    -> (the summands whose weight is not zero, the work level, the declared scale, the block)"""
    cts, weights, const = list(cts), [complex(w) for w in weights], complex(const)
    if not cts or len(cts) != len(weights):
        raise MkheError("LinCombNew: one weight per ciphertext, at least one ciphertext")
    if any(c.ids != cts[0].ids for c in cts):
        raise MkheError("LinCombNew: the ciphertexts must carry the same ids")
    lmin = min(c.Level() for c in cts)
    l = lmin if level is None else int(level)
    if l > lmin or l < 0:
        raise MkheError("LinCombNew: the work level must lie between 0 and the lowest level of the ciphertexts")
    if rescale and l < 1:
        raise MkheError("cannot Rescale: input Ciphertext already at level 0")
    scale = params.Scale() if scale is None else float(scale)
    terms = [(c, w) for c, w in zip(cts, weights) if w != 0] or [(cts[0], 0j)]
    if len(terms) > LINCOMB_MAX:
        raise MkheError("LinCombNew: at most %d non-zero weights per call" % LINCOMB_MAX)
    s_mid = scale * float(params.Q[l]) if rescale else scale
    return [c for c, _ in terms], l, scale, lincomb_consts(params.Q[: l + 1], s_mid, const, [c.Scale for c, _ in terms], [w for _, w in terms])


def _lincombs_plan(params, cts, weight_rows, consts, scales, rescale, level):
    """the same for LinCombsNew -> (the summands with a non-zero weight in some row, the work level, one declared scale per row, the block of all rows)"""
    cts, rows, consts = list(cts), [[complex(w) for w in r] for r in weight_rows], [complex(c) for c in consts]
    if not cts:
        raise MkheError("LinCombsNew: at least one ciphertext")
    if not rows or len(rows) > LINCOMBS_MAX_OUT or len(rows) != len(consts):
        raise MkheError("LinCombsNew: 1 to %d rows of weights per call, one constant per row" % LINCOMBS_MAX_OUT)
    if any(len(r) != len(cts) for r in rows):
        raise MkheError("LinCombsNew: one weight per ciphertext in every row")
    if any(c.ids != cts[0].ids for c in cts):
        raise MkheError("LinCombsNew: the ciphertexts must carry the same ids")
    lmin = min(c.Level() for c in cts)
    l = lmin if level is None else int(level)
    if l > lmin or l < 0:
        raise MkheError("LinCombsNew: the work level must lie between 0 and the lowest level of the ciphertexts")
    if rescale and l < 1:
        raise MkheError("cannot Rescale: input Ciphertext already at level 0")
    if scales is None or np.ndim(scales) == 0:
        scales = [params.Scale() if scales is None else float(scales)] * len(rows)
    scales = [float(s) for s in scales]
    if len(scales) != len(rows):
        raise MkheError("LinCombsNew: one scale for all rows, or one per row")
    keep = [b for b in range(len(cts)) if any(r[b] != 0 for r in rows)] or [0]
    if len(keep) > LINCOMB_MAX:
        raise MkheError("LinCombsNew: at most %d ciphertexts with a non-zero weight per call" % LINCOMB_MAX)
    Q = params.Q[: l + 1]
    block = np.stack([lincomb_consts(Q, s * float(params.Q[l]) if rescale else s, c, [cts[b].Scale for b in keep], [r[b] for b in keep])
                      for r, c, s in zip(rows, consts, scales)])
    return [cts[b] for b in keep], l, scales, block


def _upload_consts(params, block):
    n = params.N()
    buf = mkrlwe.DeviceLimbs(params, 1, -(-block.size // n))
    return buf.upload(np.concatenate([block.ravel(), np.zeros(buf.words - block.size, dtype=np.uint64)]).reshape(1, buf.limbs, n))


def poly_eval_plan(degree):
    """The baby-step / giant-step schedule of a degree-`degree` polynomial, a pure function: m = 2^ceil(log2(degree + 1) / 2) baby powers X^1 .. X^(m-1),
    giant powers X^(m i) for 1 <= i < g = ceil((degree + 1) / m).  products = [(k, a, b)]: X^k = X^a * X^b, in an order in which a and b exist already
    (a = the largest power of two below k, or k / 2, so that depth[k] = ceil(log2 k) multiplications lie under X^k)."""
    degree = int(degree)
    if degree < 1:
        raise MkheError("poly_eval_plan: degree must be at least 1")
    m = 1 << ((degree.bit_length() + 1) // 2)              # bit_length(d) = ceil(log2(d + 1))
    g = -(-(degree + 1) // m)
    products, depth = [], {1: 0}
    for k in list(range(2, m)) + [m * i for i in range(1, g)]:
        a = 1 << ((k - 1).bit_length() - 1)                 # 2^(ceil(log2 k) - 1): k / 2 for a power of two
        products.append((k, a, k - a))
        depth[k] = depth[a] + 1
    return PolyEvalPlan(degree, m, g, products, depth)


def _giant_parts(ev, babies, rows, consts, taus, level, fused):
    """the inner sums that meet a giant power: row i = sum_j rows[i][j] * babies[j] + consts[i], rescaled from `level` onto (level - 1, taus[i]).  fused: ONE
    LinCombsNew over the babies that some row uses; otherwise one LinCombNew per row over the babies that row uses -- the same ciphertexts bit for bit"""
    if not rows:
        return []
    if fused:
        cols = [j for j in range(len(babies)) if any(r[j] != 0 for r in rows)] or [0]
        return ev.LinCombsNew([babies[j] for j in cols], [[r[j] for j in cols] for r in rows], consts, scales=taus, rescale=True, level=level)
    parts = []
    for r, c, tau in zip(rows, consts, taus):
        cols = [j for j in range(len(babies)) if r[j] != 0]
        parts.append(ev.LinCombNew([babies[j] for j in cols] or babies[:1], [r[j] for j in cols] or [0], c, scale=tau, rescale=True, level=level))
    return parts


def evaluate_poly(ev, ct, coeffs, rlkSet, scale=None, fused=False):
    """Evaluator.EvaluatePolyNew on any evaluator with params, MulRelinOnceNew, LinCombNew and SumNew (fused=True: LinCombsNew as well, for the inner sums
    i >= 1 in one call).  p(X) = sum_i inner_i(X) * X^(m i), inner_i = sum_j
    coeffs[i m + j] X^j one LinCombNew each.  Scale bookkeeping, with S the target and l_out the level of the result: inner_0 is summed at S * Q[l_out + 1]
    and rescaled onto (l_out, S); inner_i, i >= 1, is summed at tau_i * Q[l_out + 2] and rescaled to (l_out + 1, tau_i) with tau_i = S * Q[l_out + 1] /
    scale(X^(m i)), so that its product with the giant power lands on S after that product's single Rescale.  Equal scales, one mkhe_ct_sum."""
    params = ev.params
    coeffs = [complex(c) for c in coeffs]
    d = len(coeffs) - 1
    if d < 1 or d > 63:
        raise MkheError("EvaluatePolyNew: the degree must be between 1 and 63")
    l_out = ct.Level() - (d.bit_length() + 1)
    if l_out < 0:
        raise MkheError("EvaluatePolyNew: degree %d needs level %d, the ciphertext is at level %d" % (d, d.bit_length() + 1, ct.Level()))
    if not any(coeffs):
        raise MkheError("EvaluatePolyNew: the zero polynomial")
    S = params.Scale() if scale is None else float(scale)
    plan = poly_eval_plan(d)
    m, inner = plan.m, [coeffs[i: i + plan.m] for i in range(0, d + 1, plan.m)]
    needed = {j for c in inner for j in range(1, len(c)) if c[j] != 0} | {m * i for i in range(1, plan.g) if any(inner[i])}
    for k, a, b in reversed(plan.products):                 # a power nobody uses is not computed
        if k in needed:
            needed |= {a, b}
    power = {1: ct}
    for k, a, b in plan.products:
        if k in needed:
            power[k] = ev.MulRelinOnceNew(power[a], power[b], rlkSet)
    babies = lambda c: [power[j] for j in range(1, len(c)) if c[j] != 0] or [ct]
    weights = lambda c: [w for w in c[1:] if w != 0] or [0]
    terms = []
    if any(inner[0]):
        terms.append(ev.LinCombNew(babies(inner[0]), weights(inner[0]), inner[0][0], scale=S, rescale=True, level=l_out + 1))
    if fused:
        used = [i for i in range(1, plan.g) if any(inner[i])]
        taus = [S * float(params.Q[l_out + 1]) / power[m * i].Scale for i in used]
        rows = [(inner[i][1:] + [0j] * m)[: m - 1] for i in used]
        parts = _giant_parts(ev, [power.get(j) for j in range(1, m)], rows, [inner[i][0] for i in used], taus, l_out + 2, True)
        return ev.SumNew(terms + [ev.MulRelinOnceNew(part, power[m * i], rlkSet, scale=S) for part, i in zip(parts, used)])
    for i in range(1, plan.g):
        if any(inner[i]):
            giant = power[m * i]
            tau = S * float(params.Q[l_out + 1]) / giant.Scale
            part = ev.LinCombNew(babies(inner[i]), weights(inner[i]), inner[i][0], scale=tau, rescale=True, level=l_out + 2)
            terms.append(ev.MulRelinOnceNew(part, giant, rlkSet, scale=S))
    return ev.SumNew(terms)


def chebyshev_approx(f, a, b, degree):
    """float64 Chebyshev coefficients c_0 .. c_degree of the interpolant of f at the degree + 1 Chebyshev nodes of [a, b]: f(x) ~ sum_k c_k T_k((2 x - a -
    b) / (b - a)).  f takes a numpy array.  Pure numpy, host only."""
    a, b, degree = float(a), float(b), int(degree)
    if not a < b or degree < 0:
        raise MkheError("chebyshev_approx: needs a < b and a degree of at least 0")
    return np.polynomial.chebyshev.chebinterpolate(lambda y: np.asarray(f(0.5 * (b - a) * y + 0.5 * (b + a)), dtype=np.float64), degree)


def chebyshev_blocks(coeffs, m):
    """sum_k c_k T_k = sum_i inner_i * T_(m i) with inner_i = sum_(j < m) B[i][j] T_j: the blocks B [ceil(len / m)][m] of a baby-step / giant-step evaluation
    in the Chebyshev basis, a pure function.  From T_(m i + j) = 2 T_j T_(m i) - T_(m i - j), top block down on running coefficients c': B[i][0] = c'[m i];
    B[i][j] = 2 c'[m i + j] and c'[m i - j] -= c'[m i + j] for 1 <= j < m; B[0] = c'[0 : m].  |B| stays below 14 for |c_k| <= 1 up to degree 255."""
    m = int(m)
    c = np.asarray(coeffs)
    c = c.astype(np.complex128 if np.iscomplexobj(c) else np.float64)
    if m < 1 or c.ndim != 1 or c.size < 1:
        raise MkheError("chebyshev_blocks: a list of coefficients and a block length of at least 1")
    g = -(-c.size // m)
    c = np.concatenate([c, np.zeros(g * m - c.size, dtype=c.dtype)])
    B = np.zeros((g, m), dtype=c.dtype)
    for i in range(g - 1, 0, -1):
        B[i, 0] = c[m * i]
        for j in range(1, m):
            B[i, j] = 2 * c[m * i + j]
            c[m * i - j] -= c[m * i + j]
    B[0] = c[:m]
    return B


def evaluate_chebyshev(ev, ct, coeffs, interval, rlkSet, scale=None, fused=True):
    """Evaluator.EvaluateChebyshevNew on any evaluator with params, LinCombNew, LinCombsNew, MulRelinRawNew, MulRelinOnceNew and SumNew.
    Change of variable: y = (2 x - a - b) / (b - a), one LinCombNew at the scale of ct, one level; none for (a, b) = (-1, 1).
    Powers, on poly_eval_plan(degree) as it is: for (k, a', b'), T_k = 2 T_a' T_b' - T_c with c = a' - b' (an earlier power, or 0: T_0 = 1).  With prod =
    MulRelinRawNew(T_a', T_b') at level l, T_k = LinCombNew([prod, T_c], [2, -1], 0, scale=prod.Scale / Q[l], level=l) -- the division of the product
    rides on the sum, the weight of prod is the integer 2 and T_c is re-weighted onto prod.Scale by an integer, so no scale mismatch is tolerated
    anywhere.  T_c lies no deeper than T_a' (c <= a'), so it has level l at least; depth[k] = ceil(log2 k) as in the monomial basis.
    Inner sums and giant products: the bookkeeping of evaluate_poly (S, tau_i, l_out) on the blocks of chebyshev_blocks: inner_0 is summed at S * Q[l_out
    + 1] onto (l_out, S); inner_i, i >= 1, at tau_i * Q[l_out + 2] onto (l_out + 1, tau_i), tau_i = S * Q[l_out + 1] / scale(T_(m i)), all in ONE
    LinCombsNew (fused) or one LinCombNew each; MulRelinOnceNew(inner_i, T_(m i)) lands on (l_out, S); one SumNew."""
    params = ev.params
    coeffs = [complex(c) for c in coeffs]
    d = len(coeffs) - 1
    if d < 1 or d > CHEBYSHEV_MAX_DEGREE:
        raise MkheError("EvaluateChebyshevNew: the degree must be between 1 and %d" % CHEBYSHEV_MAX_DEGREE)
    a, b = (float(v) for v in interval)
    if not a < b:
        raise MkheError("EvaluateChebyshevNew: the interval (a, b) needs a < b")
    change = (a, b) != (-1.0, 1.0)
    need = (1 if change else 0) + d.bit_length() + 1
    l_out = ct.Level() - need
    if l_out < 0:
        raise MkheError("EvaluateChebyshevNew: degree %d on this interval needs level %d, the ciphertext is at level %d" % (d, need, ct.Level()))
    if not any(coeffs):
        raise MkheError("EvaluateChebyshevNew: the zero polynomial")
    S = params.Scale() if scale is None else float(scale)
    plan = poly_eval_plan(d)
    m, B = plan.m, [list(r) for r in chebyshev_blocks(coeffs, plan.m)]
    needed = {j for r in B for j in range(1, m) if r[j] != 0} | {m * i for i in range(1, plan.g) if any(B[i])}
    for k, p, q in reversed(plan.products):                 # a power nobody uses is not computed; T_(p - q) is used by T_k
        if k in needed:
            needed |= {p, q, p - q} - {0}
    y = ev.LinCombNew([ct], [2 / (b - a)], -(a + b) / (b - a), scale=ct.Scale, rescale=True) if change else ct
    power = {1: y}
    for k, p, q in plan.products:
        if k in needed:
            prod = ev.MulRelinRawNew(power[p], power[q], rlkSet)
            l = prod.Level()
            rest, w, const = ([power[p - q]], [-1], 0) if p != q else ([], [], -1)
            power[k] = ev.LinCombNew([prod] + rest, [2] + w, const, scale=prod.Scale / float(params.Q[l]), rescale=True, level=l)
    babies = [power.get(j) for j in range(1, m)]
    terms = []
    if any(B[0]):
        cols = [j for j in range(1, m) if B[0][j] != 0]
        terms.append(ev.LinCombNew([power[j] for j in cols] or [y], [B[0][j] for j in cols] or [0], B[0][0], scale=S, rescale=True, level=l_out + 1))
    used = [i for i in range(1, plan.g) if any(B[i])]
    taus = [S * float(params.Q[l_out + 1]) / power[m * i].Scale for i in used]
    parts = _giant_parts(ev, babies, [B[i][1:] for i in used], [B[i][0] for i in used], taus, l_out + 2, fused)
    terms += [ev.MulRelinOnceNew(part, power[m * i], rlkSet, scale=S) for part, i in zip(parts, used)]
    return ev.SumNew(terms)


# ---- plaintext linear transforms M z = sum_k d_k (.) rot_k(z) (no reference counterpart: the reference has MulPtxtNew and RotateNew, one at a time)
PTXT_DOT_MAX_IN, PTXT_DOT_MAX_GIANT = 16, 64          # csrc/poly_kernels.h, CTDOT_MAX_IN / CTDOT_MAX_GIANT
LinTransPlan = collections.namedtuple("LinTransPlan", "n1 babies giants")


def linear_transform_plan(indices, n, n1=None, stride=1):
    """Baby steps and giant steps for the diagonal indices `indices` (taken mod n, the number of slots), a pure function: k = b + g with b = k mod n1 and g = k - b.
    -> (n1, sorted babies, sorted giants).  n1 is a power of two <= 16; the default minimises the number of rotations (non-zero babies + non-zero
    giants), ties to the smaller n1.  MkheError when the diagonals need more than 64 giants.
    stride = s > 1 is for diagonals that all lie at multiples of s (a factor of a factored transform): with k = s u, b = s (u mod n1) and g = k - b, so
    the babies are s, 2 s, .. instead of all collapsing onto baby 0.  The stride is declared, never guessed from the indices; an index that is no
    multiple of it is refused."""
    n, s = int(n), int(stride)
    idx = sorted({int(k) % n for k in indices})
    if not idx:
        raise MkheError("linear_transform_plan: no diagonal")
    if n1 is not None and (int(n1) != n1 or n1 < 1 or n1 > PTXT_DOT_MAX_IN or n1 & (n1 - 1)):
        raise MkheError("linear_transform_plan: n1 must be a power of two, at most %d" % PTXT_DOT_MAX_IN)
    if s != stride or s < 1:
        raise MkheError("linear_transform_plan: the stride must be a positive integer")
    off = [k for k in idx if k % s]
    if off:
        raise MkheError("linear_transform_plan: diagonal %d is no multiple of the stride %d" % (off[0], s))
    best = None
    for m in ([int(n1)] if n1 is not None else [1, 2, 4, 8, 16]):
        babies, giants = sorted({k % (s * m) for k in idx}), sorted({k - k % (s * m) for k in idx})
        cost = sum(1 for b in babies if b) + sum(1 for g in giants if g)
        if len(giants) <= PTXT_DOT_MAX_GIANT and (best is None or cost < best[0]):
            best = (cost, LinTransPlan(m, babies, giants))
    if best is None:
        raise MkheError("linear_transform_plan: more than %d giant steps" % PTXT_DOT_MAX_GIANT)
    return best[1]


class LinearTransform:
    """The diagonals {k: d_k} of (M z)[j] = sum_k d_k[j] z[(j + k) mod n], n = 2^params.LogSlots() slots -- the convention of RotateNew(ct, k), which moves slot j + k to
    slot j -- encoded once for Evaluator.LinearTransformNew.  Diagonal k = g + b (linear_transform_plan) is stored pre-rotated, np.roll(d_k, g), so that
    M z = sum_g rot_g(sum_b d'_(g,b) (.) rot_b z).  All of them are encoded on the device in ONE EncodeBatch at `level` and at the scale
    pt_scale = out_scale * Q[level] / in_scale (both default to params.Scale()), then prepared in ONE mkhe_ptxt_prepare into a compact block in (g, b)
    order: no plaintext transform is left for the evaluation.  keep_coeff=True also keeps the coefficient-domain plaintexts (LinearTransformNew(..,
    fused=False)).  stride: the declared common divisor of the indices (linear_transform_plan)."""

    def __init__(self, params, diagonals, level, in_scale=None, out_scale=None, n1=None, keep_coeff=False, stride=1):
        n = 1 << params.LogSlots()
        level = int(level)
        if level < 0 or level > params.MaxLevel():
            raise MkheError("LinearTransform: the level must lie between 0 and %d" % params.MaxLevel())
        diag = {}
        for k, d in dict(diagonals).items():
            d = np.asarray(d, dtype=np.complex128)
            if d.shape != (n,):
                raise MkheError("LinearTransform: diagonal %d must have %d slots, got %r" % (k, n, d.shape))
            if int(k) % n in diag:
                raise MkheError("LinearTransform: diagonal %d is given twice (indices are taken mod %d)" % (k, n))
            diag[int(k) % n] = d
        self.params, self.level, self.n = params, level, n
        self.plan = linear_transform_plan(diag, n, n1, stride)
        self.in_scale = params.Scale() if in_scale is None else float(in_scale)
        self.out_scale = params.Scale() if out_scale is None else float(out_scale)
        self.pt_scale = self.out_scale * float(params.Q[level]) / self.in_scale
        babies, giants = self.plan.babies, self.plan.giants
        self.order = [(g, b) for g in giants for b in babies if (g + b) in diag]          # (g + b < n: g <= k and b = k - g)
        self.masks = [sum(1 << i for i, b in enumerate(babies) if (g + b) in diag) for g in giants]
        self.pt_coeff = DeviceEncoder(params).EncodeBatch(np.stack([np.roll(diag[g + b], g) for g, b in self.order]), level, self.pt_scale)
        self.pt = mkrlwe.DeviceLimbs(params, len(self.order), level + 1) if keep_coeff else self.pt_coeff
        check(lib().mkhe_ptxt_prepare(params.ctx, level + 1, len(self.order), self.pt_coeff.devptr(), self.pt.devptr()))
        if not keep_coeff:
            self.pt_coeff = None

    @classmethod
    def FromMatrix(cls, params, M, level, **kw):
        """the d x d matrix M, d a power of two <= n, as the d diagonals of the d-periodic operator d_k[j] = M[j mod d][(j + k) mod d]: on a vector whose
        d entries are replicated n / d times it gives M @ v, replicated (d = n = 2^params.LogSlots(): M @ v itself).  Diagonals that are zero
        throughout are left out."""
        M = np.asarray(M, dtype=np.complex128)
        n, d = 1 << params.LogSlots(), M.shape[0]
        if M.ndim != 2 or M.shape != (d, d) or d < 1 or d & (d - 1) or d > n:
            raise MkheError("LinearTransform.FromMatrix: the matrix must be d x d with d a power of two, at most %d" % n)
        diags = matrix_diagonals(M, n)
        if not diags:
            raise MkheError("LinearTransform.FromMatrix: the zero matrix")
        return cls(params, diags, level, **kw)

    def Rotations(self):
        """the sorted non-zero baby and giant indices: what AddCRS / GenRotationKey must have provided"""
        return sorted({r for r in self.plan.babies + self.plan.giants if r})


def matrix_diagonals(M, n):
    """{k: d_k} with d_k[j] = M[j mod d][(j + k) mod d] over n slots, the all-zero diagonals left out (LinearTransform.FromMatrix)"""
    M = np.asarray(M, dtype=np.complex128)
    d, j = M.shape[0], np.arange(n)
    out = {k: M[j % d, (j + k) % d] for k in range(d)}
    return {k: v for k, v in out.items() if v.any()}


def linear_transform(ev, ct, lt, rkSet, fused=True):
    """Evaluator.LinearTransformNew.  Launch sets of the fused form: HoistedForm(ct) once; the non-zero baby rotations as lanes of ONE mkhe_rotate_multi that
    share that hoisted form; ONE mkhe_ct_ptxt_dot; the non-zero giant rotations of the inner sums as lanes of ONE mkhe_rotate_multi; ONE mkhe_ct_lincomb
    with weights 1 that carries the Rescale (more than 16 summands: first reduced in groups by mkhe_ct_sum).  A ciphertext above lt.level is first
    dropped to it (DropLevelNew), in both forms: a hoisted form belongs to the level it was made at."""
    params, level = ev.params, lt.level
    if lt.params is not params:
        raise MkheError("LinearTransformNew: the transform was encoded for other parameters")
    if level < 1:
        raise MkheError("cannot Rescale: the linear transform is encoded at level 0")
    if ct.Level() < level:
        raise MkheError("LinearTransformNew: the ciphertext is at level %d, the transform was encoded at level %d" % (ct.Level(), level))
    if not fused and lt.pt_coeff is None:
        raise MkheError("LinearTransformNew: fused=False needs LinearTransform(.., keep_coeff=True)")
    babies, giants = lt.plan.babies, lt.plan.giants
    keys = mkrlwe.rotation_keys(params, rkSet, ct.ids, lt.Rotations(), "LinearTransformNew")
    L, ctx = lib(), params.ctx
    if ct.Level() > level:
        ct = ev.DropLevelNew(ct, ct.Level() - level)
    mid_scale = ct.Scale * lt.pt_scale
    new = lambda scale, lv=level: NewCiphertext(params, ct.IDSet(), lv, scale, zero=False)
    hoisted = ev.HoistedForm(ct) if any(babies) else None

    def rotate_lanes(srcs, rots, hoists):
        return mkrlwe.rotate_lanes(params, keys, ct.ids, srcs, rots, hoists, [new(c.Scale) for c in srcs])

    words = (level + 1) * params.N()
    if fused:
        nzb = [b for b in babies if b]
        rot = dict(zip(nzb, rotate_lanes([ct] * len(nzb), nzb, [hoisted] * len(nzb)))) if nzb else {}
        rot[0] = ct
        inner = [new(mid_scale) for _ in giants]
        masks = (C.c_uint32 * len(giants))(*lt.masks)
        check(L.mkhe_ct_ptxt_dot(ctx, len(babies), handle_array([rot[b].h for b in babies]), len(giants), masks, lt.pt.devptr(), level + 1,
                                 handle_array([c.h for c in inner])))
        nzg = [(g, c) for g, c in zip(giants, inner) if g]
        terms = [c for g, c in zip(giants, inner) if not g]
        if nzg:
            terms += rotate_lanes([c for _, c in nzg], [g for g, _ in nzg], None)
        while len(terms) > LINCOMB_MAX:
            terms = [mkrlwe.sum_in_groups(ctx, terms[i: i + LINCOMB_MAX], lambda: new(mid_scale)) for i in range(0, len(terms), LINCOMB_MAX)]
        consts = np.zeros((len(terms) + 1, 2, level + 1), dtype=np.uint64)
        consts[1:, 0, :] = np.array([(1 << 64) % q for q in params.Q[: level + 1]], dtype=np.uint64)              # MForm(1)
        n = params.N()
        buf = mkrlwe.DeviceLimbs(params, 1, -(-consts.size // n))
        buf.upload(np.concatenate([consts.ravel(), np.zeros(buf.words - consts.size, dtype=np.uint64)]).reshape(1, buf.limbs, n))
        out = new(0.0, level - 1)
        check(L.mkhe_ct_lincomb(ctx, len(terms), handle_array([c.h for c in terms]), buf.devptr(), 1, out.h))
    else:
        rot = {b: ev.RotateHoistedNew(ct, b, hoisted, rkSet) if b else ct for b in babies}

        summed = lambda cts: mkrlwe.sum_in_groups(ctx, cts, lambda: new(mid_scale))
        terms, index = [], 0
        for g, mask in zip(giants, lt.masks):
            prods = []
            for i, b in enumerate(babies):
                if mask >> i & 1:
                    prods.append(new(mid_scale))
                    check(L.mkhe_ct_mul_ptxt(ctx, rot[b].h, C.c_void_p(lt.pt_coeff.devptr().value + 8 * words * index), prods[-1].h))
                    index += 1
            part = summed(prods)
            terms.append(ev.RotateNew(part, g, rkSet) if g else part)
        total = summed(terms)
        out = new(0.0, level - 1)
        check(L.mkhe_rescale(ctx, total.h, 1, out.h))
    out.Scale = lt.out_scale if ct.Scale == lt.in_scale else mid_scale / float(params.Q[level])
    return out


class FactoredTransform:
    """A product of sparse factors, M = F_f .. F_2 F_1 with `factors` = [F_1, .. F_f] in the order they are applied, each a dict of diagonals in the
    convention of LinearTransform: one LinearTransform per factor at the levels level, level - 1, .., each with its own stride (`strides`, default 1
    throughout).  The class knows nothing about what the factors are; dft_factors gives those of the slot matrix C0.
    Scales.  Factor t (t = 0 .. f - 1) takes its input at s_t and leaves it at s_(t+1), with s_0 = in_scale, s_f = out_scale (both default to
    params.Scale()) and s_t = in_scale (out_scale / in_scale)^(t / f) in between: every factor's plaintexts are then encoded at Q[level - t] times the
    same ratio (out_scale / in_scale)^(1 / f), and a ciphertext that enters at in_scale leaves at out_scale exactly.  A pure power of two common to a
    factor's entries (the 2^-g of an inverse butterfly) is better put into a declared scale by the caller than into these plaintexts."""

    def __init__(self, params, factors, level, in_scale=None, out_scale=None, strides=None, keep_coeff=False):
        factors = [dict(F) for F in factors]
        f, level = len(factors), int(level)
        if not f:
            raise MkheError("FactoredTransform: no factor")
        strides = [1] * f if strides is None else [int(s) for s in strides]
        if len(strides) != f:
            raise MkheError("FactoredTransform: %d strides for %d factors" % (len(strides), f))
        if level - (f - 1) < 0 or level > params.MaxLevel():
            raise MkheError("FactoredTransform: %d factors from level %d need the levels %d .. %d of 0 .. %d" % (f, level, level, level - f + 1, params.MaxLevel()))
        self.params, self.level = params, level
        self.in_scale = params.Scale() if in_scale is None else float(in_scale)
        self.out_scale = params.Scale() if out_scale is None else float(out_scale)
        self.scales = [self.in_scale] + [self.in_scale * (self.out_scale / self.in_scale) ** (t / f) for t in range(1, f)] + [self.out_scale]
        self.transforms = [LinearTransform(params, F, level - t, in_scale=self.scales[t], out_scale=self.scales[t + 1], stride=s, keep_coeff=keep_coeff)
                           for t, (F, s) in enumerate(zip(factors, strides))]

    def Rotations(self):
        """the union of the factors' Rotations()"""
        return sorted({r for lt in self.transforms for r in lt.Rotations()})

    def Depth(self):
        """one level per factor"""
        return len(self.transforms)


def factored_transform(ev, ct, ft, rkSet, fused=True):
    """Evaluator.FactoredTransformNew: linear_transform on each factor in turn; every key of ft.Rotations() is looked up before the first engine call"""
    if ft.params is not ev.params:
        raise MkheError("FactoredTransformNew: the transform was encoded for other parameters")
    mkrlwe.rotation_keys(ev.params, rkSet, ct.ids, ft.Rotations(), "FactoredTransformNew")
    for lt in ft.transforms:
        ct = linear_transform(ev, ct, lt, rkSet, fused)
    return ct


def _dft_stage(n, l, inverse):
    """the diagonals {k mod n: d_k} of the radix-2 stage S_l over n slots (dft_factors), or of its inverse"""
    h, p = l // 2, np.arange(n) % l
    low = p < h
    e, acc = [], 1
    for _ in range(h):
        e.append(acc)
        acc = acc * 5 % (4 * l)
    om = np.exp(2j * np.pi * np.array(e)[p % h] / (4 * l))
    if inverse:
        parts = [(0, np.where(low, 0.5, -0.5 / om)), (h, np.where(low, 0.5, 0)), (-h, np.where(low, 0, 0.5 / om))]
    else:
        parts = [(0, np.where(low, 1, -om)), (h, np.where(low, om, 0)), (-h, np.where(low, 0, 1))]
    out = {}
    for k, d in parts:
        out[k % n] = out.get(k % n, 0) + d.astype(np.complex128)
    return out


def _diag_product(A, B, n):
    """the diagonals of A B: (A B z)[j] = sum_a A_a[j] sum_b B_b[j + a] z[j + a + b]"""
    out = {}
    for a, da in A.items():
        for b, db in B.items():
            k = (a + b) % n
            out[k] = out.get(k, 0) + da * np.roll(db, -a)
    return out


def dft_groups(logSlots, groups, who="dft_factors"):
    """(strides, index sets) of the factors of dft_factors(logSlots, groups), without their entries: stride_t = 2^(g_1 + .. + g_(t-1)), the indices of F_t are
    the multiples u stride_t with |u| < 2^g_t, taken mod n.  MkheError for a group below 1 or a sum other than logSlots."""
    groups = [int(g) for g in groups]
    if int(logSlots) < 1 or not groups or min(groups) < 1 or sum(groups) != int(logSlots):
        raise MkheError("%s: the groups %r must be positive and sum to logSlots = %d >= 1" % (who, tuple(groups), logSlots))
    n, strides = 1 << int(logSlots), [1 << sum(groups[:t]) for t in range(len(groups))]
    return strides, [sorted({u * s % n for u in range(-(1 << g) + 1, 1 << g)}) for g, s in zip(groups, strides)]


def dft_factors(logSlots, groups, inverse=False):
    """The slot matrix C0 of bootstrap_matrices as a product of sparse factors, pure numpy.  n = 2^logSlots.  The radix-2 stage S_l, l = 2, 4, .. n, acts on
    every block of l entries: out[i + j] = in[i + j] + w in[i + j + l/2], out[i + j + l/2] = in[i + j] - w in[i + j + l/2] for j < l / 2 with
    w = exp(2 pi i (5^j mod 4l) / 4l); C0 = S_n .. S_4 S_2 R with (R a)[i] = a[bitrev(i)].  groups = (g_1, .. g_f), positive, summing to logSlots: F_t is
    the product of the next g_t stages in ascending l (F_1 holds S_2), so C0 = F_f .. F_1 R.
    -> (factors, strides): factors[t] = {k: d_k} of F_(t+1) in the convention of LinearTransform, indices in [0, n), all-zero diagonals left out;
    strides[t] = 2^(g_1 + .. + g_t) divides every index of it.  A factor has 2^(g+1) - 1 diagonals (the last 2^g: +k and -k meet mod n) with entries of
    modulus 1 or 0.  inverse=True: the F_t^-1 in the same list order, on the negated indices, entries of modulus 2^-g_t or 0."""
    strides, _ = dft_groups(logSlots, groups)
    n, factors, l = 1 << int(logSlots), [], 2
    for g in groups:
        acc = None
        for _ in range(int(g)):
            S = _dft_stage(n, l, inverse)
            acc = S if acc is None else (_diag_product(acc, S, n) if inverse else _diag_product(S, acc, n))
            l *= 2
        factors.append({k: d for k, d in sorted(acc.items()) if d.any()})
    return factors, strides


def bit_reverse(n):
    """the permutation i -> bitrev(i) over log2(n) bits, as an index array: a[bit_reverse(n)] is R a"""
    bits = int(n).bit_length() - 1
    return np.array([int(format(i, "0%db" % bits)[::-1], 2) if bits else 0 for i in range(n)], dtype=np.int64)


# ---- bootstrapping (no reference counterpart; DESIGN.md, "Bootstrapping"): ModRaise, SubSum, CoeffsToSlots, EvalMod, SlotsToCoeffs; dense transforms for
# 2^logSlots <= 1024 slots, factored ones (dft_factors above) for any number
BOOTSTRAP_MAX_LOG_SLOTS = 10      # without `factors`: one LinearTransform holds 16 x 64 diagonals (PTXT_DOT_MAX_IN x PTXT_DOT_MAX_GIANT)
BOOTSTRAP_MIN_RATIO = 2.0 ** 8    # Q[0] / scale: below it the sine's cubic term, (2 pi / ratio)^2 / 6, costs more than 2^-11.6


def bootstrap_matrices(params):
    """(M1, M2, C0, C1), n x n complex, n = 2^params.LogSlots(), in the convention of Encoder: for the 2n real grid coefficients a of the plaintext
    whose slots are z, w = M1 z + M2 conj(z) has w[t] = a[t] + i a[t + n], and z = C0 a[:n] + C1 a[n:].  With zeta_j = exp(i pi 5^j / 2n), z_j = sum_k
    a_k zeta_j^k: C0[j][k] = zeta_j^k, C1[j][k] = zeta_j^(k + n).  zeta_j^n = i^(5^j) = i for every j, so C1 = i C0 and z = C0 w: the map is complex-linear,
    M2 is identically zero, and M1 = C0^-1 = C0^H / n (the zeta_j conj(zeta_j') are distinct n-th roots of unity).  Pure numpy, no device."""
    enc = Encoder(params)
    n, k = enc.n, np.arange(enc.n, dtype=np.int64)
    root = lambda e: np.exp(1j * np.pi * ((enc.rot[:, None] * e[None, :]) % (2 * enc.M)) / enc.M)          # zeta_j^e
    C0, C1 = root(k), root(k + n)
    return np.conj(C0).T / n, np.zeros((n, n), dtype=np.complex128), C0, C1


def eval_mod_coeffs(K=16, double_angle=3, degree=31):
    """Chebyshev coefficients c_0 .. c_degree of cos(2 pi (K y - 1/4) / 2^double_angle) on (-1, 1): after double_angle steps of 2 v^2 - 1 it is
    cos(2 pi (K y - 1/4)) = sin(2 pi K y)"""
    return chebyshev_approx(lambda y: np.cos(2 * np.pi * (K * y - 0.25) / 2.0 ** double_angle), -1, 1, degree)


def eval_mod_model(t, K, double_angle, coeffs, ratio):
    """the cleartext pipeline of EvalModNew on t = m / ratio + I: the series at t / K, double_angle steps of 2 v^2 - 1, times ratio / (2 pi) -- m, up to the
    series' error and the sine's cubic term m (2 pi m / ratio)^2 / 6.  t may be complex (the pipeline is a polynomial: a slot with a small imaginary
    part comes out with it times the derivative)."""
    t = np.asarray(t)
    v = np.polynomial.chebyshev.chebval(t.astype(np.complex128 if np.iscomplexobj(t) else np.float64) / K, coeffs)
    for _ in range(int(double_angle)):
        v = 2 * v * v - 1
    return v * (float(ratio) / (2 * np.pi))


class Bootstrapper:
    """A refresh of a level-0 MK-CKKS ciphertext that uses PUBLIC evaluation keys only (Refresher needs every party online with its secret key).

    Contract.  The slots of the ciphertext are bounded by 1 in modulus.  Every party's secret key is SPARSE (KeyGenerator.GenSecretKeySparse): the
    raised phase is m + e + Q[0] I, and the integer part I has a standard deviation of about sqrt((1 + total Hamming weight) / 12) per coefficient;
    EvalMod removes it only while |I| <= K - 1, so K is chosen against the TOTAL weight over the parties (K = 16 against a total weight of 64 fails with
    probability below 1e-9 per bootstrapping).  ratio = Q[0] / ct.Scale >= 2^8; the result differs from the message by the series' error plus the
    sine's cubic term, at most (2 pi / ratio)^2 / 6 per coefficient over the scale, plus the evaluation noise ("Bootstrapping").

    Steps of BootstrapNew and their levels, from `level` (default: the top) down: ModRaise; SubSum; CoeffsToSlots (1: one transform, M2 being zero) and
    the split into real and imaginary part onto params.Scale() (1); EvaluateChebyshevNew on (-1, 1) (ceil(log2(degree + 1)) + 1); double_angle
    steps of 2 v^2 - 1 (1 each); SlotsToCoeffs (1).  The constants cost no level: 1 / gap and 1 / (K ratio) are the declared scale Q[0] K gap of the
    ciphertext that enters CoeffsToSlots, ratio / (2 pi) is the declared scale of the one that leaves EvalMod.  The transforms are encoded on the device
    at their first use, for the input scale they meet; another input scale re-encodes them.

    factors=(c2s_groups, s2c_groups), two tuples of positive integers that each sum to logSlots, replaces each dense transform by the sparse factors of
    dft_factors (any logSlots >= 1, past 1024 slots too) at one level per factor: Depth() = 10 + len(c2s_groups) + len(s2c_groups) at the defaults.
    CoeffsToSlots applies F_f^-1 first and F_1^-1 last, which leaves the grid coefficients in BIT-REVERSED slot order (C0^-1 = R F_1^-1 .. F_f^-1 and R is
    never applied); EvalMod is slot-wise; SlotsToCoeffs applies F_1 .. F_f to lo + i hi, and C0 = F_f .. F_1 R undoes the order.  The inverse factors
    are encoded with their entries times 2^g_t (modulus 1), and the 1 / n that is left goes into the declared scale.  factors=None is the dense
    object in every respect."""

    def __init__(self, params, K=16, double_angle=3, degree=31, level=None, factors=None):
        self.params, self.K, self.double_angle, self.degree = params, int(K), int(double_angle), int(degree)
        self.level = params.MaxLevel() if level is None else int(level)
        self.n = 1 << params.LogSlots()
        self.gap = params.N() // (2 * self.n)
        self.groups = None
        if factors is not None:
            if len(factors) != 2:
                raise MkheError("Bootstrapper: factors is (c2s_groups, s2c_groups), two tuples of group sizes")
            c2s, s2c = factors
            self.groups = (tuple(int(g) for g in c2s), tuple(int(g) for g in s2c))
            # [which] -> (strides, index sets) in the order the factors are APPLIED: F_f^-1 .. F_1^-1 (on the negated = the same index sets), then F_1 .. F_f
            shape = [dft_groups(params.LogSlots(), g, "Bootstrapper") for g in self.groups]
            self._shape = [(shape[0][0][::-1], shape[0][1][::-1]), shape[1]]
            self.plans = [[linear_transform_plan(idx, self.n, stride=s) for s, idx in zip(*sh)] for sh in self._shape]
        elif params.LogSlots() > BOOTSTRAP_MAX_LOG_SLOTS:
            raise MkheError("Bootstrapper: logSlots = %d, at most %d (one transform holds %d x %d diagonals)"
                            % (params.LogSlots(), BOOTSTRAP_MAX_LOG_SLOTS, PTXT_DOT_MAX_IN, PTXT_DOT_MAX_GIANT))
        if self.K < 1 or self.double_angle < 0 or not 1 <= self.degree <= CHEBYSHEV_MAX_DEGREE:
            raise MkheError("Bootstrapper: needs K >= 1, double_angle >= 0 and a degree between 1 and %d" % CHEBYSHEV_MAX_DEGREE)
        if self.level > params.MaxLevel() or self.level < self.Depth():
            raise MkheError("Bootstrapper: the chain must hold Depth() + 1 = %d moduli up to `level`, level = %d of %d"
                            % (self.Depth() + 1, self.level, params.MaxLevel()))
        self.coeffs = eval_mod_coeffs(self.K, self.double_angle, self.degree)
        if self.groups is None:
            self.plan = linear_transform_plan(range(self.n), self.n)
        self._lts = {}

    def _depths(self):
        """(levels of CoeffsToSlots without the split, levels of SlotsToCoeffs): one per factor, 1 for a dense transform"""
        return (1, 1) if self.groups is None else (len(self.groups[0]), len(self.groups[1]))

    def Depth(self):
        """levels between the raised ciphertext and the result: 1 + 1 + (ceil(log2(degree + 1)) + 1) + double_angle + 1; with `factors`, one per factor in
        place of the 1 of each transform"""
        return self._depths()[0] + 1 + self.degree.bit_length() + 1 + self.double_angle + self._depths()[1]

    def Rotations(self):
        """every index a party must hold a CRS slot and a rotation key for: n, 2n, .. N / 4 (SubSum: powers of two, so GenDefaultCRS and
        GenDefaultRotationKeys cover them) and the baby and giant steps of the two transforms"""
        sub = [self.n << i for i in range(self.gap.bit_length() - 1)]
        plans = [self.plan] if self.groups is None else self.plans[0] + self.plans[1]
        return sorted(set(sub) | {r for p in plans for r in p.babies + p.giants if r})

    def _transform(self, which, in_scale, out_scale):
        """the transform `which` (0: M1 at `level`; 1: C0 at level - Depth() + 1) for ciphertexts at in_scale, encoded once per (in_scale, out_scale)"""
        hit = self._lts.get(which)
        if hit is None or hit.in_scale != in_scale or hit.out_scale != out_scale:
            level = self.level if which == 0 else self.level - self.Depth() + self._depths()[1]
            if self.groups is None:
                M1, _, C0, _ = bootstrap_matrices(self.params)
                hit = LinearTransform.FromMatrix(self.params, M1 if which == 0 else C0, level, in_scale=in_scale, out_scale=out_scale)
            else:
                groups = self.groups[which]
                factors, _ = dft_factors(self.params.LogSlots(), groups, inverse=which == 0)
                if which == 0:              # 2^g_t F_t^-1, entries of modulus 1, last factor first; the caller declares the 1 / n
                    factors = [{k: d * 2.0 ** g for k, d in F.items()} for F, g in zip(factors, groups)][::-1]
                hit = FactoredTransform(self.params, factors, level, in_scale=in_scale, out_scale=out_scale, strides=self._shape[which][0])
            self._lts[which] = hit
        return hit

    def _apply(self, ev, ct, tr, rkSet):
        return ev.LinearTransformNew(ct, tr, rkSet) if self.groups is None else ev.FactoredTransformNew(ct, tr, rkSet)

    def CoeffsToSlotsNew(self, ct, rkSet, ckSet, ev=None):
        """(lo, hi): for the plaintext polynomial of ct with the 2n grid coefficients a (over ct.Scale), the slots of lo are a[:n] and those of hi are
        a[n:], real.  One transform w = M1 z, then lo = (w + conj w) / 2 and hi = (w - conj w) / 2i by one ConjugateNew and one LinCombsNew.  ct at
        `level` or above (LinearTransformNew drops a higher one to the transform's level first, and refuses a lower one); the halves are at level - 2 with Scale == params.Scale() exactly: the transform leaves at S Q[level - 1] / 2^B, B >= 1 chosen
        so that its plaintexts are encoded at about Q[level], and the weights 1/2 of the split are then the integers 2^(B - 1).
        With `factors` the slots come in BIT-REVERSED order: slot i of lo is a[bitrev(i)], slot i of hi is a[n + bitrev(i)] (bitrev over logSlots
        bits); the f factors take the levels level .. level - f + 1 and the halves are at level - f - 1.  The factors are encoded with entries of
        modulus 1, n C0^-1 in all, at about Q[their level]: their product leaves at S Q[level - f] / (2^B n), which is then declared as
        S Q[level - f] / 2^B, an exact division by n."""
        ev = Evaluator(self.params) if ev is None else ev
        params, S = self.params, self.params.Scale()
        top = S * float(params.Q[self.level - self._depths()[0]])
        norm = 1 if self.groups is None else self.n
        B = max(1, int(round(math.log2(top / (ct.Scale * norm)))))
        w = self._apply(ev, ct, self._transform(0, ct.Scale, top / 2.0 ** B / norm), rkSet)
        w.Scale = w.Scale * norm
        return ev.LinCombsNew([w, ev.ConjugateNew(w, ckSet)], [[0.5, 0.5], [-0.5j, 0.5j]], [0, 0], scales=S, rescale=True)

    def EvalModNew(self, ct, rlkSet, ratio=None, ev=None):
        """on a ciphertext whose slots are real and lie in (-1, 1), y = (m / ratio + I) / K with integers |I| <= K - 1: m in its slots (eval_mod_model).
        The series of eval_mod_coeffs on (-1, 1), then double_angle times LinCombNew([MulRelinRawNew(v, v)], [2], -1, ..), whose weight is the integer
        2; the factor ratio / (2 pi) is the declared Scale of the result.  ratio defaults to Q[0] / params.Scale().  ceil(log2(degree + 1)) + 1 +
        double_angle levels.  A BatchCiphertext goes through a BatchEvaluator of its length (ev, or a new one): every node is then one batched call."""
        if isinstance(ct, BatchCiphertext):
            ev = BatchEvaluator(self.params, len(ct)) if ev is None else ev
            if not isinstance(ev, BatchEvaluator) or ev.B != len(ct):
                raise MkheError("EvalModNew: a batch of %d ciphertexts needs a BatchEvaluator of that many inputs" % len(ct))
        ev = Evaluator(self.params) if ev is None else ev
        params = self.params
        ratio = float(params.Q[0]) / params.Scale() if ratio is None else float(ratio)
        v = ev.EvaluateChebyshevNew(ct, self.coeffs, (-1, 1), rlkSet)
        for _ in range(self.double_angle):
            prod = ev.MulRelinRawNew(v, v, rlkSet)
            l = prod.Level()
            v = ev.LinCombNew([prod], [2], -1, scale=prod.Scale / float(params.Q[l]), rescale=True, level=l)
        v.Scale = v.Scale * (2 * math.pi / ratio)
        return v

    def SlotsToCoeffsNew(self, ct_lo, ct_hi, rkSet, ev=None):
        """the ciphertext whose plaintext has the grid coefficients (slots of ct_lo, slots of ct_hi), both real: z = C0 (lo + i hi), C1 being i C0 -- one
        LinCombNew without rescale (the weights 1 and i are exact) and one transform.  Both halves carry one Scale; the result is at level - Depth()
        with Scale == params.Scale() exactly.  With `factors` the halves are taken in the BIT-REVERSED slot order in which CoeffsToSlotsNew leaves them
        (slot i of ct_lo is a[bitrev(i)], slot i of ct_hi is a[n + bitrev(i)]), and F_1 .. F_f are applied at one level each: z = F_f .. F_1 R w = C0 w."""
        ev = Evaluator(self.params) if ev is None else ev
        if ct_lo.Scale != ct_hi.Scale:
            raise MkheError("SlotsToCoeffsNew: the two halves must carry one scale")
        w = ev.LinCombNew([ct_lo, ct_hi], [1, 1j], 0, scale=ct_lo.Scale, rescale=False)
        return self._apply(ev, w, self._transform(1, w.Scale, self.params.Scale()), rkSet)

    def _refuse(self, ct, rlkSet, rkSet, ckSet):
        """every refusal of BootstrapNew that depends on the call: no engine call is made here"""
        params = self.params
        if ct.Level() != 0:
            raise MkheError("BootstrapNew: the ciphertext must be at level 0, it is at level %d" % ct.Level())
        ratio = float(params.Q[0]) / ct.Scale
        if ratio < BOOTSTRAP_MIN_RATIO:
            raise MkheError("BootstrapNew: Q[0] / scale = %g is below 2^8" % ratio)
        for idx in (-1, -2):
            if idx not in params.CRS:
                raise MkheError("BootstrapNew: no CRS slot %d" % idx)
        mkrlwe.rotation_keys(params, rkSet, ct.ids, self.Rotations(), "BootstrapNew")
        for i in ct.ids:
            rlkSet.GetRelinearizationKey(i)
            ckSet.GetConjugationKey(i)
        return ratio

    def BootstrapNew(self, ct, rlkSet, rkSet, ckSet, ev=None, pair=False):
        """ct at level 0 -> the same message under the same ids at level `level` - Depth() with Scale == params.Scale() exactly.  MkheError before any
        engine call when ct is not at level 0, Q[0] / ct.Scale < 2^8, or a key or CRS slot of Rotations(), a relinearisation or conjugation key or
        CRS slot -1 / -2 is missing (logSlots > 10 without `factors`, bad groups and a chain shorter than Depth() + 1 are refused by the constructor).  pair=True: the two halves
        go through EvalModNew once, as a batch of two on ev.Lanes(2), instead of one after the other -- the same ciphertext bit for bit."""
        ratio = self._refuse(ct, rlkSet, rkSet, ckSet)
        ev = Evaluator(self.params) if ev is None else ev
        raised = ev.ModRaiseNew(ct, self.level)
        sub = ev.SubSumNew(raised, rkSet)
        sub.Scale = sub.Scale * (self.K * ratio)                    # = Q[0] K gap: the slots of lo / hi are (m / ratio + I) / K
        lo, hi = self.CoeffsToSlotsNew(sub, rkSet, ckSet, ev)
        if pair:
            lo, hi = self.EvalModNew(BatchCiphertext([lo, hi]), rlkSet, ratio, ev.Lanes(2)).cts
        else:
            lo, hi = self.EvalModNew(lo, rlkSet, ratio, ev), self.EvalModNew(hi, rlkSet, ratio, ev)
        return self.SlotsToCoeffsNew(lo, hi, rkSet, ev)


def NewEvaluator(params):
    return Evaluator(params)


# ---------------------------------------------------------------- B inputs in lock step (round 4; include/mkhe.h "B independent operations")
class BatchCiphertext:
    """B ciphertexts of one shape (same ids, level, scale): what a BatchEvaluator consumes and returns.  cts[b] are ordinary Ciphertexts."""

    def __init__(self, cts):
        self.cts = list(cts)
        c0 = self.cts[0]
        for c in self.cts:
            if c.ids != c0.ids or c.Level() != c0.Level() or c.Scale != c0.Scale:
                raise MkheError("BatchCiphertext: the ciphertexts of a batch must have one shape and scale")
        self.ids, self._scale, self.params = c0.ids, c0.Scale, c0.params
        self._harr = handle_array([c.h for c in self.cts])          # (built once: every batched call passes it)

    @property
    def Scale(self): return self._scale

    @Scale.setter
    def Scale(self, scale):
        """a declared scale is one number for the batch: every member takes it (evaluate_poly and Bootstrapper.EvalModNew assign it)"""
        self._scale = scale
        for c in self.cts:
            c.Scale = scale

    def __len__(self): return len(self.cts)
    def IDSet(self): return set(self.ids)
    def Level(self): return self.cts[0].Level()
    def ScalingFactor(self): return self.Scale
    def download(self): return np.stack([c.download() for c in self.cts])


class BatchHoisted:
    """per input the hoisted forms of its party components (mkrlwe.HoistedCiphertext each)"""

    def __init__(self, hoisted):
        self.hoisted = list(hoisted)


class BatchEvaluator:
    """The mkckks.Evaluator surface on B inputs at a time: every method takes BatchCiphertexts (or, for an operand that is the same for every
    input -- the model of cnn -- a plain Ciphertext / HoistedCiphertext, which is broadcast) and issues ONE launch set for the B operations
    (mkhe_*_batch).  mkhe_kklss_amd.cnn runs on it unchanged.  Scale bookkeeping is the single-input evaluator's (one shape, one scale)."""

    def __init__(self, params, B, ev=None):
        self.params, self.B = params, int(B)
        self.ev = ev if ev is not None else Evaluator(params)
        self._bcast = {}                       # broadcast operands (the model ciphertexts of cnn): their (void*)[B], keyed by object

    def Fork(self):
        """a batch evaluator on a forked context (own stream, shared keys and ciphertexts): independent chains of a circuit overlap on the GPU"""
        return BatchEvaluator(self.params.Fork(), self.B)

    def Lanes(self, n):
        """n independent operations PER INPUT as one launch set: a BatchEvaluator of B * n items on the same context, lane-major (item j * B + b = lane j
        of input b).  The independent chains of cnn.Convolution / FC1Layer on B images: one rotation / hoisting / MulRelin launch set for all of them."""
        hit = self.__dict__.setdefault("_lanes", {}).get(n)
        if hit is None:
            hit = self._lanes[n] = BatchEvaluator(self.params, self.B * n, ev=self.ev)
        return hit

    def SumNew(self, cts):
        """out = cts[0]; for c in cts[1:]: out = AddNew(out, c), on batches (one batched Add per summand)"""
        out = cts[0]
        for c in cts[1:]:
            out = self.AddNew(out, c)
        return out

    # -- helpers
    def _cts(self, op):
        return op.cts if isinstance(op, BatchCiphertext) else [op] * self.B

    def _new(self, like_ids, level, scale):
        # (one block and one create / destroy call for the B outputs instead of B of each)
        return BatchCiphertext(mkrlwe.batch_ciphertexts(Ciphertext, self.params, like_ids, level, self.B, Scale=float(scale)))

    def _h(self, op):
        """the (void*)[B] of an operand: cached on a BatchCiphertext, built (and cached per evaluator) for a broadcast ciphertext"""
        if isinstance(op, BatchCiphertext):
            return op._harr
        if isinstance(op, list):
            return handle_array([c.h for c in op])
        key = id(op)
        hit = self._bcast.get(key)
        if hit is None or hit[0] is not op:
            if len(self._bcast) > 256:
                self._bcast.clear()
            hit = self._bcast[key] = (op, handle_array([op.h] * self.B))
        return hit[1]

    def _hoists(self, hoisted, ops):
        """flat [b * n + a] handle list, or None"""
        if hoisted is None:
            return None
        ids = tuple(ops[0].ids)
        cache = hoisted.__dict__.setdefault("_flat", {})
        arr = cache.get((ids, self.B))
        if arr is None:
            hs = hoisted.hoisted if isinstance(hoisted, BatchHoisted) else [hoisted] * self.B
            arr = cache[(ids, self.B)] = handle_array([hs[b].Value[i].h for b in range(self.B) for i in ids])
        return arr

    # -- HoistedForm (evaluator.go:543-553)
    def HoistedForm(self, ct):
        if not isinstance(ct, BatchCiphertext):
            return self.ev.HoistedForm(ct)
        if not ct.ids:                                            # no party component: nothing to hoist
            return BatchHoisted([mkrlwe.NewHoistedCiphertext() for _ in ct.cts])
        hs, keys, k = [], mkrlwe.batch_switching_keys(self.params, self.B * len(ct.ids)), 0
        for c in ct.cts:
            h = mkrlwe.NewHoistedCiphertext()
            for id in c.ids:
                h.Value[id] = keys[k]; k += 1
            hs.append(h)
        check(lib().mkhe_hoisted_form_batch(self.params.ctx, ct.Level(), self.B, self._h(ct),
                                            handle_array([hs[b].Value[id].h for b in range(self.B) for id in ct.cts[b].ids])))
        return BatchHoisted(hs)

    # -- AddNew / SubNew (evaluator.go:316-357)
    def _binary(self, op0, op1, opcode):
        a, b = self._cts(op0), self._cts(op1)
        s0, s1 = a[0].ScalingFactor(), b[0].ScalingFactor()
        if (s1 > s0 and math.floor(s1 / s0) > 1) or (s0 > s1 and math.floor(s0 / s1) > 1):
            # scale matching multiplies one operand by a constant first (evaluateInPlace :270-292): rare in the circuits this class serves -- per input
            fn = self.ev.AddNew if opcode == 0 else self.ev.SubNew
            return BatchCiphertext([fn(a[k], b[k]) for k in range(self.B)])
        out = self._new(a[0].IDSet() | b[0].IDSet(), min(a[0].Level(), b[0].Level()), max(s0, s1))
        check(lib().mkhe_ct_binary_batch(self.params.ctx, opcode, self.B, self._h(op0), self._h(op1), self._h(out)))
        return out

    def AddNew(self, op0, op1): return self._binary(op0, op1, 0)
    def SubNew(self, op0, op1): return self._binary(op0, op1, 1)

    # -- MulRelin[Hoisted]New (evaluator.go:416-443,558-581)
    def MulRelinNew(self, op0, op1, rlkSet):
        return self.MulRelinHoistedNew(op0, op1, None, None, rlkSet)

    def _product(self, op0, op1, op0Hoisted, op1Hoisted, rlkSet, rescale):
        """ONE mkhe_mul_relin_batch: the relinearised products at the level of the operands and the product of their scales, or (rescale) one level
        below at that scale over the dropped modulus"""
        a, b = self._cts(op0), self._cts(op1)
        params = self.params
        level, prod_scale = min(a[0].Level(), b[0].Level()), a[0].ScalingFactor() * b[0].ScalingFactor()
        if -1 not in params.CRS:
            raise MkheError("mkhe: CRS[-1] (u) has not been uploaded")
        out = self._new(a[0].IDSet() | b[0].IDSet(), level - 1 if rescale else level, prod_scale / float(params.Q[level]) if rescale else prod_scale)
        d0 = [rlkSet.GetRelinearizationKey(i).Value[1].h for i in a[0].ids]
        v0 = [rlkSet.GetRelinearizationKey(i).Value[2].h for i in a[0].ids]
        b1 = [rlkSet.GetRelinearizationKey(i).Value[0].h for i in b[0].ids]
        check(lib().mkhe_mul_relin_batch(params.ctx, self.B, self._h(op0), self._h(op1), self._hoists(op0Hoisted, a), self._hoists(op1Hoisted, b),
                                         handle_array(b1), handle_array(d0), handle_array(v0), params.CRS[-1].h, 1 if rescale else 0, self._h(out)))
        return out

    def MulRelinHoistedNew(self, op0, op1, op0Hoisted, op1Hoisted, rlkSet):
        a, b = self._cts(op0), self._cts(op1)
        params = self.params
        level, prod_scale = min(a[0].Level(), b[0].Level()), a[0].ScalingFactor() * b[0].ScalingFactor()
        nb1, scale1 = self.ev._nb_rescales(level, prod_scale, params.Scale())
        # the single evaluator's branch (Evaluator.MulRelinHoistedNew): the Rescale is folded into the engine call only when it is the usual single
        # one and fuse_rescale is set; otherwise the product is formed at its level and ONE mkhe_rescale(nb) per input follows, as there
        rescale = nb1 == 1 and level >= 1 and self.ev.fuse_rescale
        ids = a[0].IDSet() | b[0].IDSet()
        out = self._product(op0, op1, op0Hoisted, op1Hoisted, rlkSet, rescale)
        if rescale:
            return out
        nb, scale = self.ev.nbRescales(out.cts[0], params.Scale())
        if nb == 0 or out.cts[0].Level() == 0:
            return out
        res = self._new(ids, out.cts[0].Level() - nb, scale)
        for c, r in zip(out.cts, res.cts):              # (nb != 1 or fuse_rescale off: not in the circuits of the reference -- per input)
            check(lib().mkhe_rescale(params.ctx, c.h, nb, r.h))
        return res

    def MulRelinRawNew(self, op0, op1, rlkSet):
        """Evaluator.MulRelinRawNew on the batch: the products at level min(levels) with Scale = the product of the scales, no Rescale"""
        return self._product(op0, op1, None, None, rlkSet, False)

    def MulRelinOnceNew(self, op0, op1, rlkSet, scale=None):
        """Evaluator.MulRelinOnceNew on the batch: the batch MulRelinNew where that takes the usual MulRelinNew, otherwise the product with exactly ONE
        Rescale folded into the engine call; the declared scales are those of Evaluator"""
        a, b = self._cts(op0), self._cts(op1)
        level, prod = min(a[0].Level(), b[0].Level()), a[0].ScalingFactor() * b[0].ScalingFactor()
        if level < 1:
            raise MkheError("cannot Rescale: input Ciphertext already at level 0")
        if self.ev._nb_rescales(level, prod, self.params.Scale())[0] == 1:
            res = self.MulRelinNew(op0, op1, rlkSet)
        else:
            res = self._product(op0, op1, None, None, rlkSet, True)
        if scale is not None:
            res.Scale = float(scale)
        return res

    # -- weighted sums and polynomials (Evaluator.LinCombNew .. EvaluateChebyshevNew; no reference counterpart)
    def _lincomb_call(self, terms, block, l, scales, rescale):
        """ONE constants upload and ONE mkhe_ct_lincomb_batch: row g of `block` over `terms` (batches, or plain ciphertexts that every item shares) -> one batch per row"""
        params, B = self.params, self.B
        for c in terms:
            if isinstance(c, BatchCiphertext) and len(c) != B:
                raise MkheError("BatchEvaluator: a batch of %d ciphertexts on an evaluator of %d inputs" % (len(c), B))
        buf = _upload_consts(params, block)
        outs = [self._new(terms[0].IDSet(), l - (1 if rescale else 0), s) for s in scales]
        members = [self._cts(c) for c in terms]
        check(lib().mkhe_ct_lincomb_batch(params.ctx, B, len(terms), handle_array([m[b].h for b in range(B) for m in members]), len(outs), buf.devptr(),
                                          1 if rescale else 0, handle_array([o.cts[b].h for b in range(B) for o in outs])))
        return outs

    def LinCombNew(self, cts, weights, const=0, scale=None, rescale=True, level=None):
        """Evaluator.LinCombNew on every input of the batch (same arguments, defaults, rules and refusals): the one-row case of LinCombsNew"""
        terms, l, scale, block = _lincomb_plan(self.params, cts, weights, const, scale, rescale, level)
        return self._lincomb_call(terms, block[None], l, [scale], rescale)[0]

    def LinCombsNew(self, cts, weight_rows, consts, scales=None, rescale=True, level=None):
        """Evaluator.LinCombsNew on every input of the batch (same arguments, defaults, rules and refusals); cts are BatchCiphertexts, or plain Ciphertexts
        that every input shares.  The inputs of a batch carry one scale, so ONE constant block serves them all: one upload and ONE engine call
        (mkhe_ct_lincomb_batch) whatever B.  MkheError before any engine call on a shape error, a batch whose length is not B included."""
        terms, l, scales, block = _lincombs_plan(self.params, cts, weight_rows, consts, scales, rescale, level)
        return self._lincomb_call(terms, block, l, scales, rescale)

    def AddConstNew(self, ct, c):
        return self.LinCombNew([ct], [1], c, scale=ct.Scale, rescale=False)

    def EvaluatePolyNew(self, ct, coeffs, rlkSet, scale=None, fused=False):
        """Evaluator.EvaluatePolyNew on every input of the batch: the same schedule, every node one batched engine call"""
        return evaluate_poly(self, ct, coeffs, rlkSet, scale, fused)

    def EvaluateChebyshevNew(self, ct, coeffs, interval, rlkSet, scale=None, fused=True):
        """Evaluator.EvaluateChebyshevNew on every input of the batch: the same schedule, every node one batched engine call"""
        return evaluate_chebyshev(self, ct, coeffs, interval, rlkSet, scale, fused)

    # -- RotateNew / RotateHoistedNew (evaluator.go:485-525,585-617)
    def _rotate(self, ct, rotidx, hoisted, rkSet):
        params = self.params
        cts = self._cts(ct)
        out = self._new(cts[0].IDSet(), cts[0].Level(), cts[0].Scale)
        rk = [rkSet.GetRotationKey(i, rotidx).Value.h for i in cts[0].ids]
        check(lib().mkhe_rotate_batch(params.ctx, params.GaloisElementForColumnRotationBy(rotidx), self.B, self._h(ct), self._hoists(hoisted, cts),
                                      handle_array(rk), params.CRS[rotidx].h, self._h(out)))
        return out

    def RotateNew(self, ct, rotidx, rkSet):
        rotidx = self.ev._norm_rot(rotidx)
        if rotidx == 0:
            return BatchCiphertext([self.ev.RotateNew(c, 0, rkSet) for c in self._cts(ct)])
        if rotidx in self.params.CRS:
            return self._rotate(ct, rotidx, None, rkSet)
        tmp, k = ct, 1
        while rotidx > 0:                                   # power-of-two decomposition, :516-523
            if rotidx % 2:
                tmp = self._rotate(tmp, k, None, rkSet)
            rotidx //= 2
            k *= 2
        return tmp

    def RotateHoistedNew(self, ct, rotidx, ctHoisted, rkSet):
        if isinstance(rotidx, (list, tuple)):
            return self._rotate_multi(ct, [self.ev._norm_rot(r) for r in rotidx], ctHoisted, rkSet, None)
        rotidx = self.ev._norm_rot(rotidx)
        if rotidx == 0:
            return BatchCiphertext([self.ev.RotateNew(c, 0, rkSet) for c in self._cts(ct)])
        if rotidx not in self.params.CRS:
            raise MkheError("Hoisted rotation only works for precomputed rotation keys")
        return self._rotate(ct, rotidx, ctHoisted, rkSet)

    def _rotate_multi(self, ct, rots, hoisted, rkSet, post):
        """input b rotated by rots[b] (every index non-zero and with a CRS), each with its own keys: one launch set (mkhe_rotate_multi);
        post: BatchCiphertext / Ciphertext added to the rotated ciphertexts on the store, or None"""
        params = self.params
        cts = self._cts(ct)
        if len(rots) != self.B:
            raise MkheError("BatchEvaluator: one rotation index per input")
        for r in rots:
            if r == 0 or r not in params.CRS:
                raise MkheError("Hoisted rotation only works for precomputed rotation keys")
        out = self._new(cts[0].IDSet(), cts[0].Level(), cts[0].Scale)
        rk = [rkSet.GetRotationKey(i, r).Value.h for r in rots for i in cts[0].ids]
        gal = (C.c_uint64 * self.B)(*[params.GaloisElementForColumnRotationBy(r) for r in rots])
        check(lib().mkhe_rotate_multi(params.ctx, self.B, gal, self._h(ct), self._hoists(hoisted, cts), handle_array(rk),
                                      handle_array([params.CRS[r].h for r in rots]), self._h(post) if post is not None else None, self._h(out)))
        return out

    def RotateAndAddNew(self, ct, rotidx, rkSet):
        """AddNew(ct, RotateNew(ct, rotidx, rkSet)) for every input, the addition on the store of the rotation (Evaluator.RotateAndAddNew)"""
        rotidx = self.ev._norm_rot(rotidx)
        if rotidx == 0 or rotidx not in self.params.CRS:
            return self.AddNew(ct, self.RotateNew(ct, rotidx, rkSet))
        return self._rotate_multi(ct, [rotidx] * self.B, None, rkSet, ct)

    # -- MulPtxtNew (evaluator.go:465-481)
    def MulPtxtNew(self, ct, pt_value, pt_scale):
        params = self.params
        cts = self._cts(ct)
        level, scale = cts[0].Level(), cts[0].Scale * float(pt_scale)
        if isinstance(pt_value, mkrlwe.DeviceLimbs):
            pt = pt_value
            if pt.limbs != level + 1:
                raise MkheError("MulPtxtNew: the resident plaintext must have level + 1 limbs")
        else:
            pt = mkrlwe.DeviceLimbs(params, 1, level + 1).upload(np.ascontiguousarray(pt_value, dtype=np.uint64)[None, : level + 1])
        nb, rscale = (0, scale) if level == 0 else self.ev._nb_rescales(level, scale, params.Scale())
        out = self._new(cts[0].IDSet(), level - nb, rscale if nb else scale)
        check(lib().mkhe_ct_mul_ptxt_batch(params.ctx, self.B, self._h(ct), pt.devptr(), nb, self._h(out)))
        return out


# ---- messages, encoder, encryptor, decryptor (mkckks/elements.go:19-31, encryptor.go, decryptor.go)
class Message:
    """mkckks.Message (elements.go:19-21): Value = one complex number per slot"""

    def __init__(self, value):
        self.Value = np.asarray(value, dtype=np.complex128)

    def Slots(self):
        return len(self.Value)


def NewMessage(params):
    """elements.go:23-27: 2^logSlots zero slots"""
    return Message(np.zeros(1 << params.LogSlots(), dtype=np.complex128))


class Plaintext:
    """ckks.Plaintext as the encryptor sees it: an RNS polynomial (host uint64 [level+1][N], coefficient domain) and its scale"""

    def __init__(self, value, scale):
        """value: host uint64 [level+1][N], or the device plaintext (mkrlwe.DeviceLimbs [1][level+1][N]) of DeviceEncoder.Encode"""
        self.Value = value if isinstance(value, mkrlwe.DeviceLimbs) else np.asarray(value, dtype=np.uint64)
        self.Scale = float(scale)

    def Level(self):
        return (self.Value.limbs if isinstance(self.Value, mkrlwe.DeviceLimbs) else self.Value.shape[0]) - 1


class Encoder:
    """The canonical embedding of lattigo's ckks.Encoder on the HOST (numpy): n = 2^logSlots slots (default params.LogSlots()).  With M = 2n and
    the gap g = N / M a message is a polynomial in X^g: coefficient k g is coefficient k of the embedding for the ring of degree M -- slot j <->
    evaluation at zeta^(5^j), zeta = exp(i*pi/M), computed with one FFT of length 2M -- and every other coefficient is exactly 0.0.  Seen through
    the full embedding it is the n slots repeated g times.  Project and Decode read the coefficients on the grid only: for arbitrary coefficients
    that is the mean over the g replicas of the full projection.  logSlots = logN - 1 is full packing (g = 1)."""

    def __init__(self, params, logSlots=None):
        self.params = params
        self.N = params.N()
        self.logSlots = params.LogSlots() if logSlots is None else logSlots
        _check_log_slots("mkckks.Encoder", self.logSlots, params.LogN())
        self.n = 1 << self.logSlots
        self.M = 2 * self.n
        self.gap = self.N // self.M
        rot, r = np.empty(self.n, dtype=np.int64), 1
        for j in range(self.n):
            rot[j], r = r, r * mkrlwe.GALOIS_GEN % (2 * self.M)
        self.rot = rot

    def Embed(self, values):
        """slots -> real coefficients m with sum_k m_(k g) zeta_j^k = z_j:  m_(k g) = (2/M) Re sum_j z_j conj(zeta_j)^k, 0.0 off the grid"""
        z = np.asarray(values, dtype=np.complex128)
        if z.shape != (self.n,):
            raise MkheError("mkckks.Encoder: expected %d slots, got %r" % (self.n, z.shape))
        a = np.zeros(2 * self.M, dtype=np.complex128)
        a[self.rot] = z
        m = (2.0 / self.M) * np.real(np.fft.fft(a)[: self.M])
        if self.gap == 1:
            return m
        out = np.zeros(self.N, dtype=np.float64)
        out[:: self.gap] = m
        return out

    def Encode(self, values, level, scale):
        """-> RNS plaintext uint64 [level+1][N]: round(m * scale) per coefficient (half to even), reduced exactly whatever its size"""
        x = self.Embed(values) * float(scale)
        Q = self.params.Q[: level + 1]
        if np.abs(x).max(initial=0.0) < 2.0 ** 62:
            r = np.rint(x).astype(np.int64)
            return np.stack([np.mod(r, np.int64(q)).astype(np.uint64) for q in Q])
        r = np.array([int(round(float(v))) for v in x], dtype=object)
        return np.stack([np.array([int(v) for v in r % q], dtype=np.uint64) for q in Q])

    def Decode(self, poly, scale):
        """RNS polynomial [limbs][N] (canonical residues) at `scale` -> slots: CRT and centring of the coefficients on the grid, then the embedding"""
        poly = np.asarray(poly, dtype=np.uint64)[:, :: self.gap]
        Q = self.params.Q[: poly.shape[0]]
        Qp = 1
        for q in Q:
            Qp *= q
        x = np.zeros(self.M, dtype=object)
        for l, q in enumerate(Q):
            Mi = Qp // q
            x = x + poly[l].astype(object) * (Mi * pow(Mi, -1, q))
        x = x % Qp
        return self._project(np.array([float(v - Qp if v > Qp // 2 else v) for v in x]) / float(scale))

    def Project(self, m):
        """real coefficients [N] -> slots: z_j = sum_k m_(k g) zeta_j^k"""
        return self._project(np.asarray(m)[:: self.gap])

    def _project(self, m):
        a = np.zeros(2 * self.M, dtype=np.complex128)
        a[: self.M] = m
        return (2 * self.M) * np.fft.ifft(a)[self.rot]


def slot_permutation(logN):
    """t with t[j] = (5^j mod 2N - 1) / 4, a permutation of 0 .. N/2 - 1: slot j of a message is bin t[j] of the N/2-point transform
    of the twisted coefficient pairs (csrc/ckks_kernels.h)"""
    n = 1 << (logN - 1)
    t, g = np.empty(n, dtype=np.int64), 1
    for j in range(n):
        t[j], g = (g - 1) // 4, g * mkrlwe.GALOIS_GEN % (4 * n)
    return t


class DeviceEncoder:
    """The interface of Encoder on the DEVICE (mkhe_ckks_*: csrc/ckks_kernels.hip), plus batch forms.  Messages go up and come down as
    n = 2^logSlots complex slots (16 bytes each; default params.LogSlots()); plaintexts stay resident as mkrlwe.DeviceLimbs.  Same embedding
    convention as Encoder, sparse packing included (mkhe_ckks_*_sparse); float64 arithmetic with another factorisation, so the bits of an encoding
    differ from the host encoder's in the last places."""

    def __init__(self, params, logSlots=None):
        self.params = params
        self.N = params.N()
        self.logSlots = params.LogSlots() if logSlots is None else logSlots
        _check_log_slots("mkckks.DeviceEncoder", self.logSlots, params.LogN())
        self.n = 1 << self.logSlots
        self.full = self.logSlots == params.LogN() - 1

    def _call(self, stage, *args):
        """mkhe_ckks_<stage>(ctx, [level or limbs,] count, ..) or, below full packing, mkhe_ckks_<stage>_sparse with log_slots in front of count"""
        if self.full:
            check(getattr(lib(), "mkhe_ckks_" + stage)(self.params.ctx, *args))
        else:
            at = 0 if stage in ("embed", "project") else 1
            check(getattr(lib(), "mkhe_ckks_%s_sparse" % stage)(self.params.ctx, *args[:at], self.logSlots, *args[at:]))

    # a float64 array <-> a raw device buffer (one 8-byte word per double) of whole rows of N words
    def _up(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64).ravel()
        rows = -(-a.size // self.N)
        a = np.concatenate([a, np.zeros(rows * self.N - a.size)])
        return mkrlwe.DeviceLimbs(self.params, 1, rows).upload(a.view(np.uint64).reshape(1, rows, self.N))

    def _slot_buffer(self, count):
        return mkrlwe.DeviceLimbs(self.params, 1, -(-2 * self.n * count // self.N))

    def _slots(self, values):
        """-> (complex128 [count][n], whether the caller passed one message)"""
        z = np.asarray(values, dtype=np.complex128)
        one = z.ndim == 1
        z = z[None] if one else z
        if z.ndim != 2 or z.shape[0] < 1 or z.shape[1] != self.n:
            raise MkheError("mkckks.DeviceEncoder: expected %d slots per message, got %r" % (self.n, np.shape(values)))
        return np.ascontiguousarray(z), one

    def _down_slots(self, d, count, one):
        z = d.download().view(np.float64).ravel()[: count * self.n * 2].reshape(count, self.n, 2)
        z = z[..., 0] + 1j * z[..., 1]
        return z[0] if one else z

    def Embed(self, values):
        """slots [n] (or [count][n]) -> real coefficients [N] (or [count][N])"""
        z, one = self._slots(values)
        src, dst = self._up(z.view(np.float64)), mkrlwe.DeviceLimbs(self.params, len(z), 1)
        self._call("embed", len(z), src.devptr(), dst.devptr())
        m = dst.download().view(np.float64).reshape(len(z), self.N)
        return m[0] if one else m

    def Project(self, coeffs):
        """real coefficients [N] (or [count][N]) -> slots"""
        m = np.asarray(coeffs, dtype=np.float64)
        one = m.ndim == 1
        m = m[None] if one else m
        if m.ndim != 2 or m.shape[0] < 1 or m.shape[1] != self.N:
            raise MkheError("mkckks.DeviceEncoder: expected %d coefficients per message, got %r" % (self.N, np.shape(coeffs)))
        src, dst = self._up(m), self._slot_buffer(len(m))
        self._call("project", len(m), src.devptr(), dst.devptr())
        return self._down_slots(dst, len(m), one)

    def EncodeBatch(self, values, level, scale):
        """count messages -> device plaintexts [count][level+1][N] (coefficient domain, canonical) as one launch set"""
        z, _ = self._slots(values)
        src, pt = self._up(z.view(np.float64)), mkrlwe.DeviceLimbs(self.params, len(z), level + 1)
        self._call("encode", level, len(z), src.devptr(), float(scale), pt.devptr())
        return pt

    def Encode(self, values, level, scale):
        """-> device plaintext [1][level+1][N]: what mkrlwe.Encryptor.Encrypt and MulPtxtNew take as they are"""
        z, one = self._slots(values)
        if not one:
            raise MkheError("mkckks.DeviceEncoder: Encode takes one message (EncodeBatch takes several)")
        return self.EncodeBatch(z, level, scale)

    def Decode(self, poly, scale):
        """device plaintext(s) [count][limbs][N] (or a host polynomial [limbs][N]) at `scale` -> slots [n] ([count][n] for count > 1)"""
        if not isinstance(poly, mkrlwe.DeviceLimbs):
            poly = np.ascontiguousarray(poly, dtype=np.uint64)
            poly = mkrlwe.DeviceLimbs(self.params, 1, poly.shape[0]).upload(poly[None])
        dst = self._slot_buffer(poly.count)
        self._call("decode", poly.limbs, poly.count, poly.devptr(), float(scale), dst.devptr())
        return self._down_slots(dst, poly.count, poly.count == 1)


def _encoder(params, which):
    if which not in ("host", "device"):
        raise MkheError("mkckks: encoder must be \"host\" or \"device\"")
    return Encoder(params) if which == "host" else DeviceEncoder(params)


class Encryptor(mkrlwe.Encryptor):
    """mkckks.Encryptor (encryptor.go:7-27): mkrlwe.Encryptor + the encoder.  encoder="host" (default): the numpy Encoder, whose
    plaintext is uploaded; "device": DeviceEncoder, whose plaintext goes to mkhe_encrypt without touching the host."""

    def __init__(self, params, sampler=None, encoder="host"):
        super().__init__(params, sampler)
        self.encoder = _encoder(params, encoder)

    def _new_batch(self, id, level, count, like=None):
        return mkrlwe.batch_ciphertexts(Ciphertext, self.params, [id], level, count, Scale=self.params.Scale())

    def EncryptPtxt(self, plaintext, pk, ctOut, samples=None):
        """encryptor.go:33-36"""
        self.Encrypt(plaintext.Value, pk, ctOut, samples)
        ctOut.Scale = plaintext.Scale
        return ctOut

    def EncodeMsgNew(self, msg):
        """encryptor.go:60-64: at the maximum level and the default scale"""
        return Plaintext(self.encoder.Encode(msg.Value, self.params.MaxLevel(), self.params.Scale()), self.params.Scale())

    def EncryptMsg(self, msg, pk, ctOut, samples=None):
        """encryptor.go:42-45"""
        return self.EncryptPtxt(self.EncodeMsgNew(msg), pk, ctOut, samples)

    def EncryptMsgNew(self, msg, pk, samples=None):
        """encryptor.go:51-58"""
        ctOut = NewCiphertext(self.params, [pk.ID], self.params.MaxLevel(), self.params.Scale(), zero=False)
        return self.EncryptMsg(msg, pk, ctOut, samples)

    def EncryptPtxtBatch(self, plaintexts, pk, samples=None):
        """the plaintexts (one level, one scale) under one public key as one engine call (mkrlwe.Encryptor.EncryptBatch)"""
        cts = self.EncryptBatch([p.Value for p in plaintexts], pk, samples)
        for c, p in zip(cts, plaintexts):
            c.Scale = p.Scale
        return cts

    def EncryptMsgBatch(self, msgs, pk, samples=None):
        """EncryptMsgNew (encryptor.go:51-58) for several messages under one public key: one encode (one launch set with the device
        encoder) and one mkhe_encrypt call"""
        level, scale = self.params.MaxLevel(), self.params.Scale()
        if isinstance(self.encoder, DeviceEncoder):
            pts = self.encoder.EncodeBatch(np.stack([m.Value for m in msgs]), level, scale)
        else:
            pts = np.stack([self.encoder.Encode(m.Value, level, scale) for m in msgs])
        cts = self.EncryptBatch(pts, pk, samples)
        for c in cts:
            c.Scale = scale
        return cts


def NewEncryptor(params, sampler=None, encoder="host"):
    return Encryptor(params, sampler, encoder)


class SeededCiphertext(mkrlwe.SeededCiphertext):
    """mkrlwe.SeededCiphertext whose Expand() returns mkckks Ciphertexts with `scale` (default: the scale of the parameters)"""

    def __init__(self, params, id, level=None, count=1, scale=None):
        self.Scale = params.Scale() if scale is None else float(scale)
        super().__init__(params, id, params.MaxLevel() if level is None else level, count, cls=Ciphertext, Scale=self.Scale)


class SecretKeyEncryptor(mkrlwe.SecretKeyEncryptor):
    """mkrlwe.SecretKeyEncryptor + the encoder (no reference counterpart): a party encrypts its own slots under its secret key, at the maximum
    level and the default scale.  EncryptMsgSeeded returns the half-size form that travels; its Expand() gives what EncryptMsgBatch gives."""

    def __init__(self, params, sk, sampler=None, encoder="host", seed=None, insecure_test_only=False):
        super().__init__(params, sk, sampler, seed, insecure_test_only)
        self.encoder = _encoder(params, encoder)

    def _new_batch(self, level, count):
        return mkrlwe.batch_ciphertexts(Ciphertext, self.params, [self.sk.ID], level, count, Scale=self.params.Scale())

    def _new_seeded(self, level, count):
        return SeededCiphertext(self.params, self.sk.ID, level, count, self.params.Scale())

    def _encode(self, msgs):
        level, scale = self.params.MaxLevel(), self.params.Scale()
        if isinstance(self.encoder, DeviceEncoder):
            return self.encoder.EncodeBatch(np.stack([m.Value for m in msgs]), level, scale)
        return np.stack([self.encoder.Encode(m.Value, level, scale) for m in msgs])

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
    """mkckks.Decryptor (decryptor.go:6-24)"""

    def __init__(self, params, encoder="host"):
        super().__init__(params)
        self.encoder = _encoder(params, encoder)

    def _like(self, ct, ids):
        return NewCiphertext(self.params, ids, ct.Level(), ct.ScalingFactor(), zero=False)

    def DecryptPtxt(self, ct, skSet):
        """the decrypted RNS polynomial with the ciphertext's scale"""
        return Plaintext(mkrlwe.Decryptor.Decrypt(self, ct, skSet).download()[0], ct.ScalingFactor())

    def Decrypt(self, ct, skSet):
        """decryptor.go:34-43 -> Message.  With the device encoder the output buffer of mkhe_decrypt goes straight to mkhe_ckks_decode:
        only the slots come down."""
        if isinstance(self.encoder, DeviceEncoder):
            return Message(self.encoder.Decode(mkrlwe.Decryptor.Decrypt(self, ct, skSet), ct.ScalingFactor()))
        pt = self.DecryptPtxt(ct, skSet)
        return Message(self.encoder.Decode(pt.Value, pt.Scale))

    def FloodSlotBound(self, parties, flood_bits, scale):
        """how far a merge of `parties` shares with flood_bits bits moves a slot, at most: N * parties * 2^(flood_bits - 1) / scale (the sum of
        the flooding noises is below parties * 2^(flood_bits - 1) per coefficient, and a slot is a sum of N coefficients times unit-modulus roots).
        It remains an upper bound for sparse messages: a sparse slot is the mean of replicas that each meet it."""
        return self.params.N() * self.FloodBound(parties, flood_bits) / float(scale)

    def NoiseNorm(self, ct, skSet, msg):
        """The largest coefficient, centred, of phase(ct) - plaintext(msg) as a Python integer, measured on the device (mkhe_noise_norm): the
        reference is the DEVICE encoder's plaintext of msg at ct.Level() and ct.Scale, whichever encoder this Decryptor decodes with.  It is
        the noise of ct plus what the encoding of msg differs by from the encoding ct was made with (nothing for a ciphertext encrypted
        from the device encoder's plaintext of the same message)."""
        ref = DeviceEncoder(self.params).Encode(msg.Value, ct.Level(), ct.ScalingFactor())
        return mkrlwe.Decryptor.NoiseNorm(self, ct, skSet, ref)

    def NoiseBits(self, ct, skSet, msg):
        """NoiseNorm(ct, skSet, msg).bit_length(): what the flood_bits of ShareNew (Decryptor, Refresher, PublicKeySwitcher) must exceed"""
        return self.NoiseNorm(ct, skSet, msg).bit_length()

    def MergeSharesMsg(self, ct, shares):
        """the merge of the shares of all parties -> Message.  With the device encoder the merged buffer goes straight to mkhe_ckks_decode."""
        pt = self.MergeShares(ct, shares)
        if isinstance(self.encoder, DeviceEncoder):
            return Message(self.encoder.Decode(pt, ct.ScalingFactor()))
        return Message(self.encoder.Decode(pt.download()[0], ct.ScalingFactor()))


def NewDecryptor(params, encoder="host"):
    return Decryptor(params, encoder)


class Refresher(mkrlwe.Refresher):
    """The collective refresh of mkrlwe.Refresher on mkckks ciphertexts: the result keeps the input's Scale (the lift is exact and the
    re-encryptions cancel the masks, so the message and its scale are untouched; only fresh encryption noise is added: RefreshSlotBound)."""

    def _out(self, like, count, level_out):
        return mkrlwe.batch_ciphertexts(Ciphertext, self.params, like.ids, level_out, count, Scale=like.ScalingFactor())

    def MaxMaskBits(self, parties, level, scale, max_abs_slot=1.0):
        """mkrlwe.Refresher.MaxMaskBits for ciphertexts at `level` whose slots are at most max_abs_slot in modulus: msg_bits =
        ceil(log2(scale * max_abs_slot)) + 1 -- a coefficient of the embedding is at most max|z| * scale in magnitude, and one more bit is
        for the noise.  This holds for sparse messages too: a coefficient of the embedding of the ring of degree 2n is at most max|z| as well."""
        q = 1
        for m in self.params.Q[: level + 1]:
            q *= int(m)
        msg_bits = int(math.ceil(math.log2(float(scale) * float(max_abs_slot)))) + 1
        return mkrlwe.Refresher.MaxMaskBits(q, parties, msg_bits)

    def RefreshSlotBound(self, parties, scale, sigma=3.2):
        """how far a refresh moves a slot, at most: N * parties * (2N + 1) * floor(6 sigma) / scale.  Each party's fresh encryption adds
        |u e_pk + e0 + e1 s| <= (2N + 1) floor(6 sigma) per coefficient (u and s ternary, the table truncated at floor(6 sigma)); a slot moves
        by at most N times the coefficient error over the scale.  It remains an upper bound for sparse messages: a sparse slot is the mean of
        replicas that each meet it."""
        N = self.params.N()
        return N * int(parties) * (2 * N + 1) * int(6 * float(sigma)) / float(scale)


def NewRefresher(params):
    return Refresher(params)


class ShareConverter(mkrlwe.ShareConverter):
    """mkrlwe.ShareConverter on mkckks ciphertexts: the shares are over R_Q in the coefficient domain (a 120-bit mask does not survive a float64
    decode, so there is no slot form), and S2E gives mkckks.Ciphertexts at `scale` -- the Scale of the ciphertexts E2S started from, which
    the caller carries across (SecretShare.Scale is set by E2SShareBatch / E2SMergeBatch and kept by FoldPublic)."""

    def _new(self, ids, level, count, like=None):
        return mkrlwe.batch_ciphertexts(Ciphertext, self.params, ids, level, count, Scale=float(getattr(like, "Scale", 0.0) or 0.0))

    def E2SShareBatch(self, cts, sk, mask_bits, sampler, level_out=None):
        pub, sec = super().E2SShareBatch(cts, sk, mask_bits, sampler, level_out)
        sec.Scale = list(cts)[0].ScalingFactor()
        return pub, sec

    def E2SMergeBatch(self, cts, shares, level_out=None):
        out = super().E2SMergeBatch(cts, shares, level_out)
        out.Scale = list(cts)[0].ScalingFactor()
        return out

    def FoldPublic(self, secret, public):
        out = super().FoldPublic(secret, public)
        out.Scale = secret.Scale
        return out

    MaxMaskBits = Refresher.MaxMaskBits


def NewShareConverter(params):
    return ShareConverter(params)


class PublicKeySwitcher(mkrlwe.PublicKeySwitcher):
    """The collective key switch of mkrlwe.PublicKeySwitcher on mkckks ciphertexts: the result is a mkckks.Ciphertext over the recipient's id with
    the input's Scale (the message and its scale are untouched; only the noise of the shares is added: SwitchSlotBound)."""

    def _out(self, like, count, recipient_id):
        return mkrlwe.batch_ciphertexts(Ciphertext, self.params, [recipient_id], like.Level(), count, Scale=like.ScalingFactor())

    def SwitchSlotBound(self, parties, flood_bits, scale, bound=19):
        """how far a switch moves a slot, at most: N * NoiseBound(parties, flood_bits, N, bound) / scale (a slot is a sum of N coefficients times
        unit-modulus roots).  It remains an upper bound for sparse messages: a sparse slot is the mean of replicas that each meet it."""
        N = self.params.N()
        return N * self.NoiseBound(parties, flood_bits, N, bound) / float(scale)


def NewPublicKeySwitcher(params):
    return PublicKeySwitcher(params)


# ---- threshold secret keys (include/mkhe.h, "threshold secret keys"): keys are the ring's, so the classes are mkrlwe's
SecretKeyShare = mkrlwe.SecretKeyShare
Thresholdizer = mkrlwe.Thresholdizer
Combiner = mkrlwe.Combiner
NewThresholdizer = mkrlwe.NewThresholdizer
NewCombiner = mkrlwe.NewCombiner
