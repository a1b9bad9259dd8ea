"""Wall time of the message layer with the CKKS encoder on the host and on the device: Decrypt to slots of one PN15QP880
top-level ciphertext over 4 parties, the decode of one PN15QP880 plaintext with sparse packing (logSlots 14 = full, 10, 6), and encode + encrypt
of the 16 plaintexts of the cnn scenario (PN14QP433).  3 warm-ups, median of 7
(min .. max), every leg ends in a device synchronise.  Needs a GPU:  python tools/ckks_encoder_timing.py"""
import os, sys, time, types
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import harness as H
from mkhe_kklss_amd import mkckks, mkrlwe

def med(f, params):
    for _ in range(3):
        f(); params.sync()
    ts = []
    for _ in range(7):
        params.sync(); t0 = time.perf_counter(); f(); params.sync(); ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[3], ts[0], ts[-1]

def setup(p, names):
    params = mkckks.Parameters(p["logN"], p["Q"], p["P"], p["scale"])
    params.GenDefaultCRS(seed=5)
    sampler = mkrlwe.HostSampler(np.random.default_rng(1), insecure_test_only=True)
    kgen = mkrlwe.NewKeyGenerator(params, sampler)
    skSet, pks = mkrlwe.NewSecretKeySet(), {}
    for n in names:
        sk, pk = kgen.GenKeyPair(n); skSet.AddSecretKey(sk); pks[n] = pk
    return params, sampler, skSet, pks

rng = np.random.default_rng(0)
# leg 1
p = H.PN15QP880
names = ["u%d" % i for i in range(4)]
params, sampler, skSet, pks = setup(p, names)
n = 1 << (p["logN"] - 1)
enc = mkckks.NewEncryptor(params, sampler, encoder="device"); ev = mkckks.NewEvaluator(params)
zs = [rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n) for _ in names]
ct = None
for z, nm in zip(zs, names):
    c = enc.EncryptMsgNew(mkckks.Message(z), pks[nm]); ct = c if ct is None else ev.AddNew(ct, c)
dh, dd = mkckks.NewDecryptor(params), mkckks.NewDecryptor(params, encoder="device")
a, b = dh.Decrypt(ct, skSet).Value, dd.Decrypt(ct, skSet).Value
print("decrypt PN15QP880 4 parties: |host - sum| %.3g |dev - sum| %.3g" % (np.abs(a - sum(zs)).max(), np.abs(b - sum(zs)).max()))
print("  host decoder  ms median %.3f (min %.3f max %.3f)" % med(lambda: dh.Decrypt(ct, skSet), params))
print("  device decoder ms median %.3f (min %.3f max %.3f)" % med(lambda: dd.Decrypt(ct, skSet), params))
print("  mkhe_decrypt alone ms median %.3f (min %.3f max %.3f)" % med(lambda: mkrlwe.Decryptor.Decrypt(dd, ct, skSet), params))
# leg 3: mkhe_ckks_decode_sparse of one top-level plaintext (uniform residues) on device buffers, by slot count; logSlots 14 is full packing
from mkhe_kklss_amd._abi import check, lib
L, N = len(p["Q"]), 1 << p["logN"]
pt = mkrlwe.DeviceLimbs(params, 1, L).upload(H.uniform_poly(rng, p["Q"], N)[None])
out = mkrlwe.DeviceLimbs(params, 1, 1)
print("decode of one PN15QP880 plaintext, %d limbs (the call alone, buffers on the device):" % L)
for ls in (14, 10, 6):
    f = lambda ls=ls: check(lib().mkhe_ckks_decode_sparse(params.ctx, L, ls, 1, pt.devptr(), p["scale"], out.devptr()))
    print("  logSlots %2d ms median %.3f (min %.3f max %.3f)" % ((ls,) + med(f, params)))
params.close()
# leg 2
p = __import__("harness_cnn").PN14QP433
params, sampler, skSet, pks = setup(p, ["a", "b"])
n = 1 << (p["logN"] - 1)
msgs = [mkckks.Message(rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)) for _ in range(16)]
eh, ed = mkckks.NewEncryptor(params, sampler), mkckks.NewEncryptor(params, sampler, encoder="device")
def leg(e):
    return lambda: (e.EncryptMsgBatch(msgs[:1], pks["a"]), e.EncryptMsgBatch(msgs[1:], pks["b"]))
print("encode + encrypt 16 plaintexts PN14QP433 (two calls, 1 + 15):")
print("  host encoder   ms median %.3f (min %.3f max %.3f)" % med(leg(eh), params))
print("  device encoder ms median %.3f (min %.3f max %.3f)" % med(leg(ed), params))
enc_only_h = lambda: [eh.encoder.Encode(m.Value, params.MaxLevel(), params.Scale()) for m in msgs]
enc_only_d = lambda: ed.encoder.EncodeBatch(np.stack([m.Value for m in msgs]), params.MaxLevel(), params.Scale())
print("  encode only: host ms median %.3f (min %.3f max %.3f)" % med(enc_only_h, params))
print("  encode only: device ms median %.3f (min %.3f max %.3f)" % med(enc_only_d, params))
params.close()
