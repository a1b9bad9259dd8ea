/* mkhe.h -- C ABI of the MI355X multi-key RLWE key-switch engine (libmkhe_hip.so).
 *
 * Drop-in boundary for the hot path of SNUCP/MKHE-KKLSS (pure Go + lattigo v2.3.0).  The
 * reference has no FFI; the boundary is the method set of mkrlwe.KeySwitcher plus the lattigo
 * helpers it calls.  Every entry point cites the reference interface it
 * replaces as <file>:<line> relative to the reference root.  The cgo stubs a maintainer would
 * add are shown in INTEGRATION.md.
 *
 * Conventions
 *  - plain C: opaque handles, pointers and sizes only.  All polynomial data is uint64, limb-major.
 *  - SwitchingKey / hoisted digit vector : uint64[betaMax][nQ+nP][N]  (Q limbs then P limbs),
 *    stored exactly as the Go side stores it: NTT domain, Montgomery form for keys and CRS
 *    (mkrlwe/params.go:56, keygen.go:299-300), NTT domain non-Montgomery for hoisted digits.
 *  - Ciphertext : uint64[1+n][limbs][N], slot 0 = Value["0"], slot 1+i = Value[ids[i]]
 *    (mkrlwe/elements.go:17-19); coefficient domain.  level = limbs-1.
 *  - Party ids are arbitrary ints chosen by the caller (the shim maps Go's string ids).
 *  - Return value 0 = ok; non-zero = error, text via mkhe_last_error() (the reference panics
 *    at the same sites: keyswitch.go:126-132, keys.go:151-162,190-198; the shim re-panics).
 *  - One context per Evaluator, calls on a context serialized by the caller (the reference is
 *    not reentrant either: shared pools keyswitch.go:12-15).  All work is enqueued on the
 *    context's HIP stream; *_download and mkhe_ctx_sync synchronize.
 *
 * Environment (the COMPLETE list of variables libmkhe_hip.so reads; each once per process)
 *  - MKHE_NTT32   = 0 | 1 | 2   forward NTT at N = 2^15 where two kernels apply (same bits): two-pass, single-pass, or (default 2)
 *                               whichever a measurement inside the caller's workload finds faster; mkhe_ctx_set_ntt_choice pins it per context
 *  - MKHE_POOL_GB = <GiB>       device-wide bound of the buffer pools that recycle freed handles (default 32; fractions allowed; 0 = keep nothing)
 * Every other MKHE_* variable named in DESIGN.md section 6 is A/B instrumentation and exists only in the diagnostic build
 * libmkhe_hip_switches.so (csrc/switches.h, `make switches`); the product library ignores them.
 */
#ifndef MKHE_H
#define MKHE_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mkhe_ctx mkhe_ctx;
typedef struct mkhe_swk mkhe_swk;
typedef struct mkhe_ct  mkhe_ct;

const char* mkhe_last_error(void);
int mkhe_device_count(void);

/* ---- context: mkrlwe.NewKeySwitcher keyswitch.go:33-47 (+ NewDecomposer basis_extension.go:368,
 *      lattigo rlwe.NewKeySwitcher / ring.NewRing tables).  psiQ/psiP: optional primitive 2N-th
 *      roots (plain) per modulus, e.g. InvMForm(ring.NttPsi[i][N/2]); NULL = lattigo's own rule.
 *      Moduli: distinct primes < 2^60 with q = 1 mod 2N (every prime of the reference's parameter sets is <= 60 bits
 *      and < 2^60; the lazy butterflies need 4q < 2^62); logN in [10, 16]. */
int  mkhe_ctx_create(mkhe_ctx** out, int logN, const uint64_t* Q, int nQ, const uint64_t* P, int nP,
                     int gamma, const uint64_t* psiQ, const uint64_t* psiP, int device);
void mkhe_ctx_destroy(mkhe_ctx* ctx);
int  mkhe_ctx_sync(mkhe_ctx* ctx);
/* Several contexts over the same ring on one device (no reference counterpart: the Go evaluator is single-threaded): each
 * has its own stream and scratch pools; keys, CRS, hoisted forms and ciphertexts are plain device memory behind their
 * handles and may be used through any of them.  Independent operations issued through different contexts overlap on the
 * GPU.  mkhe_ctx_wait_for orders them without a host synchronisation: work enqueued on ctx after the call starts only
 * after everything enqueued on other before the call has finished.  A handle must be destroyed through the context that
 * created it, after every other context that used it has been waited for. */
int  mkhe_ctx_wait_for(mkhe_ctx* ctx, mkhe_ctx* other);
/* Capture of a fixed sequence of engine calls into a HIP graph (no reference counterpart).  Between mkhe_capture_begin and
 * mkhe_capture_end every call on ctx -- and on contexts ordered with mkhe_ctx_wait_for after the begin and joined back
 * with mkhe_ctx_wait_for(ctx, other) before the end -- is recorded instead of executed; mkhe_graph_launch replays the
 * whole sequence with one submission (launch-bound circuits of many small kernels: the cnn caller).  Rules: no upload /
 * download / sync / key generation inside a capture; the replay reads and writes exactly the device buffers the captured
 * calls used, so the handles created inside the capture must stay alive (their buffers are the graph's temporaries and
 * outputs) and new inputs are uploaded into the SAME input handles. */
typedef struct mkhe_graph mkhe_graph;
int  mkhe_capture_begin(mkhe_ctx* ctx);
int  mkhe_capture_end(mkhe_ctx* ctx, mkhe_graph** out);
int  mkhe_graph_launch(mkhe_ctx* ctx, mkhe_graph* graph);
void mkhe_graph_destroy(mkhe_graph* graph);
int  mkhe_ctx_alpha(const mkhe_ctx* ctx);                 /* Parameters.Alpha  params.go:63-65 */
int  mkhe_ctx_beta(const mkhe_ctx* ctx, int level);       /* Parameters.Beta   params.go:67-71 */
int  mkhe_ctx_n(const mkhe_ctx* ctx);
size_t mkhe_ctx_swk_words(const mkhe_ctx* ctx);           /* betaMax*(nQ+nP)*N */
uint64_t mkhe_ctx_psi(const mkhe_ctx* ctx, int modulus_index);   /* root in use (Q then P) */
void* mkhe_ctx_stream(mkhe_ctx* ctx);                     /* hipStream_t, for event timing */

/* ---- SwitchingKey handles: mkrlwe.SwitchingKey keys.go:23-25, NewSwitchingKey keys.go:245-255 */
int  mkhe_swk_create(mkhe_ctx* ctx, mkhe_swk** out);
/* same without the zero fill: for keys / hoisted forms that the next engine call writes (mkhe_hoisted_form, mkhe_decompose, key generation) */
int  mkhe_swk_create_uninit(mkhe_ctx* ctx, mkhe_swk** out);
void mkhe_swk_destroy(mkhe_ctx* ctx, mkhe_swk* swk);
int  mkhe_swk_upload(mkhe_ctx* ctx, mkhe_swk* swk, const uint64_t* host);
/* Go's []rlwe.PolyQP: one pointer per limb, order [digit][Q limbs..., P limbs...] */
int  mkhe_swk_upload_limbs(mkhe_ctx* ctx, mkhe_swk* swk, const uint64_t* const* limbs, int ndigits);
int  mkhe_swk_download(mkhe_ctx* ctx, const mkhe_swk* swk, uint64_t* host);
void* mkhe_swk_devptr(mkhe_swk* swk);

/* ---- Ciphertext handles: mkrlwe.Ciphertext elements.go:17-33 */
int  mkhe_ct_create(mkhe_ctx* ctx, int n, const int* ids, int limbs, mkhe_ct** out);
/* same without the zero fill: for ciphertexts that are the output of the next engine call (every entry point writes all
 * limbs of its ctOut), e.g. the result of Evaluator.MulRelinNew */
int  mkhe_ct_create_uninit(mkhe_ctx* ctx, int n, const int* ids, int limbs, mkhe_ct** out);
void mkhe_ct_destroy(mkhe_ctx* ctx, mkhe_ct* ct);
int  mkhe_ct_upload(mkhe_ctx* ctx, mkhe_ct* ct, const uint64_t* host);
int  mkhe_ct_upload_poly_limbs(mkhe_ctx* ctx, mkhe_ct* ct, int slot, const uint64_t* const* limbs);
int  mkhe_ct_download(mkhe_ctx* ctx, const mkhe_ct* ct, uint64_t* host);
int  mkhe_ct_download_poly_limbs(mkhe_ctx* ctx, const mkhe_ct* ct, int slot, uint64_t* const* limbs);
/* device-to-device copy of a ciphertext with the same ids and number of limbs (rlwe Ciphertext.CopyNew; rotation by 0) */
int  mkhe_ct_copy(mkhe_ctx* ctx, const mkhe_ct* in, mkhe_ct* out);
int  mkhe_ct_limbs(const mkhe_ct* ct);
int  mkhe_ct_nparties(const mkhe_ct* ct);
void* mkhe_ct_devptr(mkhe_ct* ct);

/* ---- raw device buffers of uint64 words (callers that keep polynomials resident themselves) */
int  mkhe_buf_alloc(mkhe_ctx* ctx, size_t words, void** dev_out);
void mkhe_buf_free(mkhe_ctx* ctx, void* dev);
int  mkhe_buf_upload(mkhe_ctx* ctx, void* dev, const uint64_t* host, size_t words);
int  mkhe_buf_download(mkhe_ctx* ctx, const void* dev, uint64_t* host, size_t words);

/* ---- lattigo ring.NTTLvl / InvNTTLvl / InvNTTLazyLvl on a raw device buffer [count][limbs][N];
 *      limb l uses modulus index mod_base+l (0..nQ-1 = Q, nQ.. = P).  keyswitch.go:29-30,58,114-115 */
int  mkhe_ntt(mkhe_ctx* ctx, const void* dev_src, void* dev_dst, int count, int limbs, int mod_base, int inverse, int lazy);

/* ---- KeySwitcher.Decompose keyswitch.go:49-73 (DecomposeSingleNTT :21-31, DecomposeAndSplit
 *      basis_extension.go:428-535).  Input poly = slot `slot` of ct; is_ntt mirrors ring.Poly.IsNTT. */
int  mkhe_decompose(mkhe_ctx* ctx, int level, int is_ntt, const mkhe_ct* ct, int slot, mkhe_swk* out);

/* ---- mkckks.Evaluator.HoistedForm evaluator.go:543-553: Decompose of every party component ct.Value[id] (slots 1..n, not
 *      slot 0) in one batched launch; out[i] receives h(ct.Value[ids[i]]). */
int  mkhe_hoisted_form(mkhe_ctx* ctx, int level, const mkhe_ct* ct, mkhe_swk* const* out);

/* ---- KeySwitcher.ExternalProduct keyswitch.go:79-118 / ExternalProductHoisted keyswitch_hoisted.go:10-40.
 *      Result (coefficient domain, canonical) is written to slot out_slot of out. */
int  mkhe_external_product(mkhe_ctx* ctx, int level, int is_ntt, const mkhe_ct* a, int slot,
                           const mkhe_swk* bg, mkhe_ct* out, int out_slot);
int  mkhe_external_product_hoisted(mkhe_ctx* ctx, int level, const mkhe_swk* a_hoisted,
                                   const mkhe_swk* bg, mkhe_ct* out, int out_slot);

/* ---- KeySwitcher.MulAndRelin keyswitch.go:122-230 / MulAndRelinHoisted keyswitch_hoisted.go:44-179.
 *      hoist0/hoist1: per-party hoisted forms aligned with op0/op1 ids, or NULL (engine hoists
 *      internally = mkckks.Evaluator.MulRelinNew evaluator.go:416-443).
 *      rlk_d0, rlk_v0 aligned with op0 ids (rlk.Value[1], Value[2]); rlk_b1 aligned with op1 ids
 *      (rlk.Value[0]) keys.go:34-37;  crs_u = params.CRS[-1] params.go:37.
 *      level is taken from out (keyswitch_hoisted.go:46); out ids must be the union. */
int  mkhe_mul_and_relin(mkhe_ctx* ctx, const mkhe_ct* op0, const mkhe_ct* op1,
                        const mkhe_swk* const* hoist0, const mkhe_swk* const* hoist1,
                        const mkhe_swk* const* rlk_b1, const mkhe_swk* const* rlk_d0,
                        const mkhe_swk* const* rlk_v0, const mkhe_swk* crs_u, mkhe_ct* out);
/* mkckks.Evaluator.mulRelinHoisted (mkckks/evaluator.go:558-581): MulAndRelin[Hoisted] followed by ONE Rescale (the usual case: the scale of
 * the product drops below 2 * params.Scale() after one division), as one call.  `out` is the RESCALED ciphertext: one level below
 * min(level(op0), level(op1)), ids = the union.  On one device with at most four parties per operand the DivRoundByLastModulus rides on the
 * store of the last ModDown (the level-L product is never written); otherwise the engine runs mkhe_mul_and_relin into a pooled temporary and
 * mkhe_rescale after it.  The same ciphertext, bit for bit, as the two calls (tests/test_gpu_parity.py). */
int  mkhe_mul_relin_rescale(mkhe_ctx* ctx, const mkhe_ct* op0, const mkhe_ct* op1,
                            const mkhe_swk* const* hoist0, const mkhe_swk* const* hoist1,
                            const mkhe_swk* const* rlk_b1, const mkhe_swk* const* rlk_d0,
                            const mkhe_swk* const* rlk_v0, const mkhe_swk* crs_u, mkhe_ct* out);

/* K products under ONE relinearisation tail (no reference counterpart: the reference relinearises every product, cnn/cnn.go:16-31,51-61):
 * out = [Rescale] sum_k op0[k] * op1[k].  Step F2 of MulAndRelinHoisted (keyswitch_hoisted.go:156-178) is linear in t_i = <h(c0_i), y>_P up to gadget
 * noise, so per pair k the engine computes x^k, y^k, the tensor terms, step E (out_j += <h(c1_j^k), x^k>_P) and t_i += <h(c0_i^k), y^k>_P, and then
 * ONCE per party i of op0: out_0 += <h(t_i), v_i>_P, out_i += <h(t_i), u>_P.  Every sum is a sum of separately ModDown'd products, canonical mod q_l:
 * K = 1 is mkhe_mul_and_relin bit for bit, and the result does not depend on the order of the pairs.
 *   1 <= K <= 16; every op0[k] carries the ids of op0[0], every op1[k] those of op1[0]; out carries the union and is distinct from every operand;
 *   level = limbs(out) - 1 + rescale (rescale: 0 or 1): every operand has at least level + 1 limbs, of which the first level + 1 are read; with
 *   rescale = 1 out receives what mkhe_rescale(.., 1) of the rescale = 0 result would, bit for bit;
 *   hoist0: flat [k * |ids0| + a], hoist1: flat [k * |ids1| + a], either NULL (the engine hoists that side itself); keys aligned as for
 *   mkhe_mul_and_relin.  CKKS / mkrlwe contexts that own every modulus; may allocate from the pools (not for capture). */
int  mkhe_mul_relin_sum(mkhe_ctx* ctx, int K, const mkhe_ct* const* op0, const mkhe_ct* const* op1,
                        const mkhe_swk* const* hoist0, const mkhe_swk* const* hoist1,
                        const mkhe_swk* const* rlk_b1, const mkhe_swk* const* rlk_d0, const mkhe_swk* const* rlk_v0,
                        const mkhe_swk* crs_u, int rescale, mkhe_ct* out);

/* ---- the same MulAndRelinHoisted split in phases for party-sharded multi-GPU evaluation
 *      (the reference is single-process).  Each rank passes sub-ciphertexts holding c_0
 *      and the party components it owns; x_part / y_part receive the rank's canonical partial sums
 *      sum_i d_i (.) h(c0_i), sum_j b_j (.) h(c1_j) WITHOUT MForm (keyswitch_hoisted.go:79-92,99-113).
 *      The caller sums them over ranks as uint64 (RCCL all-reduce; exact while ranks*q < 2^63), calls
 *      mkhe_swk_fold(.., mform=1) (= MFormLvl of the total, :94-96,115-117) and then mkhe_mr_finish
 *      (steps E-F, :146-178; the tensor step D, :119-144, is started by mkhe_mr_partial and written into
 *      `out`).  with_c0 != 0 on exactly one rank adds c0_0*c1_0 to out_0; out_0 and any
 *      out_i whose two operand components live on different ranks are partial sums to be reduced and
 *      folded with mkhe_ct_fold. */
int  mkhe_mr_partial(mkhe_ctx* ctx, const mkhe_ct* op0, const mkhe_ct* op1,
                     const mkhe_swk* const* hoist0, const mkhe_swk* const* hoist1,
                     const mkhe_swk* const* rlk_b1, const mkhe_swk* const* rlk_d0,
                     int with_c0, mkhe_ct* out, mkhe_swk* x_part, mkhe_swk* y_part);
/* In place on the active digits / moduli of `level`: word <- (word mod q) [* 2^64 mod q with mform != 0]; inactive limbs are not touched.  Exact for
 * every word < 2^63 (the domain of the engine's Montgomery product), which a sum over `ranks` canonical residues satisfies while ranks * (q - 1) < 2^63:
 * 8 ranks for 60-bit primes, 16 for 59-bit ones (mkhe_kklss_amd.dist.exact_sum_ok).  Words >= 2^63 give unspecified residues. */
int  mkhe_swk_fold(mkhe_ctx* ctx, mkhe_swk* swk, int level, int mform);
/* The reduction of x / y on a point-to-point mesh (xGMI: 7 links per GPU; SURVEY.md 8e(2) "prefer reduce-scatter + all-gather"): rank r receives slice
 * r of every rank's partial sum (one all-to-all), sums, folds and MForm's ITS slice -- this call: limbs [first_limb, first_limb + nlimbs) of a
 * switching-key buffer ([digit][modulus][N]: limb l = digit l / (nQ + nP), modulus l % (nQ + nP)), summand p of limb i at the device address
 * pieces + (p * piece_stride_words + i * N) words, result at dst + i * N words; limbs of inactive digits / moduli are skipped -- and the folded slices
 * are all-gathered.  Same integers as the all-reduce + mkhe_swk_fold (a sum of canonical residues, then MFormLvl: keyswitch_hoisted.go:94-96,115-117).
 *   The summands of active limbs are canonical (< q, as mkhe_mr_partial writes them); the sum is reduced per summand, so the result is exact for every
 *   accepted npieces, with no ranks * q bound.  1 <= npieces <= 64; 0 <= first_limb, 0 <= nlimbs, first_limb + nlimbs <= digits * (nQ + nP);
 *   piece_stride_words >= 0, and >= nlimbs * N when npieces > 1; pieces, dst non-null; level in range.  Anything else is refused before any launch
 *   (non-zero return, mkhe_last_error names fold_pieces) and dst is not written.  pieces is only read; nlimbs == 0 does nothing. */
int  mkhe_swk_fold_pieces(mkhe_ctx* ctx, const void* pieces, int npieces, long piece_stride_words, long first_limb, long nlimbs, int level, int mform, void* dst);
int  mkhe_mr_finish(mkhe_ctx* ctx, const mkhe_ct* op0, const mkhe_ct* op1, const mkhe_swk* x, const mkhe_swk* y,
                    const mkhe_swk* const* rlk_v0, const mkhe_swk* crs_u, mkhe_ct* out);
/* mkhe_mr_finish in two halves, so that the all-reduce of x can still be in flight while the part that needs y alone runs:
 * head = t_i = <h(c0_i), y>_P for every party of op0 (keyswitch_hoisted.go:165-169) and the Decompose of the t_i (:171);
 * tail = out_j += <h(c1_j), x>_P (:146-154), then out_0 += <h(t_i), v_i>_P and out_i += <h(t_i), u>_P (:173-177).
 * mkhe_mr_finish == head; tail.  Both take the operands of the preceding mkhe_mr_partial. */
int  mkhe_mr_finish_head(mkhe_ctx* ctx, const mkhe_ct* op0, const mkhe_ct* op1, const mkhe_swk* y, mkhe_ct* out);
int  mkhe_mr_finish_tail(mkhe_ctx* ctx, const mkhe_ct* op0, const mkhe_ct* op1, const mkhe_swk* x,
                         const mkhe_swk* const* rlk_v0, const mkhe_swk* crs_u, mkhe_ct* out);
/* In place on every limb of every polynomial of ct: word <- word mod q_limb.  Exact for every word < 2^63, as for mkhe_swk_fold. */
int  mkhe_ct_fold(mkhe_ctx* ctx, mkhe_ct* ct);

/* ---- limb-sharded multi-GPU MulAndRelin (no reference counterpart; mkhe_kklss_amd/dist.py LimbShardedMulRelin).
 *      A context may own a subset of the RNS moduli (indices over Q then P; n = 0: all).  With an ownership set the
 *      four phases below evaluate KeySwitcher.MulAndRelin (keyswitch.go:122-230) on full operands (all parties, every
 *      rank) for the owned moduli only: the per-party sums x, y are local; after each phase *words_out words of the
 *      caller's device buffer dev_stage (phase 4: of `out` itself) are all-reduced (sums of disjoint slices):
 *        1: tensor, hoisting, x, y, <h(c0_i), y> + InvNTT        -> P limbs of those products
 *        2: their ModDown = t_i on the owned limbs               -> t_i
 *        3: Decompose(t_i), <h(c1_j), x>, <h(t_i), v_i>, <h(t_i), u> + InvNTT  -> P limbs
 *        4: ModDown accumulated into out (owned limbs, zeros elsewhere)        -> out
 *      Keys: rlk_b1 / rlk_d0 for phase 1, rlk_v0 / crs_u for phase 3 (NULL otherwise). */
int  mkhe_ctx_set_owned(mkhe_ctx* ctx, const int* mod_idx, int n);
int  mkhe_lsh_phase(mkhe_ctx* ctx, int phase, const mkhe_ct* op0, const mkhe_ct* op1,
                    const mkhe_swk* const* rlk_b1, const mkhe_swk* const* rlk_d0, const mkhe_swk* const* rlk_v0,
                    const mkhe_swk* crs_u, mkhe_ct* out, void* dev_stage, size_t* words_out);

/* ---- KeySwitcher.Rotate keyswitch.go:234-298 / RotateHoisted keyswitch_hoisted.go:183-247.
 *      galEl = 5^rotidx mod 2N; rk aligned with ct ids (rkSet[id][rotidx]); crs = params.CRS[rotidx]. */
int  mkhe_rotate(mkhe_ctx* ctx, uint64_t galEl, const mkhe_ct* in, const mkhe_swk* const* hoist,
                 const mkhe_swk* const* rk, const mkhe_swk* crs, mkhe_ct* out);
/* ---- Rotate in two phases for a party-sharded evaluation: the key-switch part of keyswitch.go:251-265
 *      without the permutation (with_c0 = 0 leaves c_0 out of out_0: exactly one rank adds it), and the signed
 *      permutation :267-296 on its own.  mkhe_rotate == mkhe_rotate_partial(with_c0 = 1) + mkhe_ct_automorphism. */
int  mkhe_rotate_partial(mkhe_ctx* ctx, const mkhe_ct* in, const mkhe_swk* const* hoist,
                         const mkhe_swk* const* rk, const mkhe_swk* crs, int with_c0, mkhe_ct* out);
int  mkhe_ct_automorphism(mkhe_ctx* ctx, uint64_t galEl, const mkhe_ct* in, mkhe_ct* out);
/* ---- KeySwitcher.Conjugate keyswitch.go:302-332; galEl = 2N-1, crs = params.CRS[-2] */
int  mkhe_conjugate(mkhe_ctx* ctx, uint64_t galEl, const mkhe_ct* in, const mkhe_swk* const* ck,
                    const mkhe_swk* crs, mkhe_ct* out);

/* ---- body of mkckks.Evaluator.Rescale evaluator.go:385-391 = lattigo
 *      ring.DivRoundByLastModulusManyLvl on every poly; out has limbs(in)-nb limbs. */
int  mkhe_rescale(mkhe_ctx* ctx, const mkhe_ct* in, int nb, mkhe_ct* out);

/* ---- elementwise evaluator ops on resident ciphertexts ("next" row of SURVEY.md 8f):
 *      mkckks/evaluator.go:41-104 (evaluateInPlace, add, sub) and mkbfv/evaluator.go:27-76.  out carries the
 *      union of the id sets; components only one operand has are copied (Sub: negated when they come from op1). */
int  mkhe_ct_add(mkhe_ctx* ctx, const mkhe_ct* op0, const mkhe_ct* op1, mkhe_ct* out);
int  mkhe_ct_sub(mkhe_ctx* ctx, const mkhe_ct* op0, const mkhe_ct* op1, mkhe_ct* out);

/* mkckks.Evaluator.MultByConst body (mkckks/evaluator.go:150-196): per limb l < min(limbs(in), limbs(out)) the coefficients
 * [0, N/2) are multiplied by c_first[l], [N/2, N) by c_second[l] (host arrays, Montgomery form = the reference's
 * ring.MForm(scaledConst); the float64 getConstAndScale / scaleUpExact logic :40-94 stays on the host). */
int  mkhe_ct_mul_const(mkhe_ctx* ctx, const mkhe_ct* in, const uint64_t* c_first, const uint64_t* c_second, mkhe_ct* out);
/* out = in[0] + in[1] + ... + in[n-1] for n ciphertexts of one shape (same ids; out at its own level <= theirs, may be one of them when at
 * their level): the chain `out = eval.AddNew(out, temp)` over the products of a layer (cnn/cnn.go:19-30,58-62; equal scales: ring.Add per
 * component, mkckks/evaluator.go:316-327) as one launch.  Every partial sum is canonical, so the result is the chain's bit for bit. */
int  mkhe_ct_sum(mkhe_ctx* ctx, int n, const mkhe_ct* const* in, mkhe_ct* out);
/* out = sum_k (re_k + i im_k) in[k] + (add_re + i add_im), then nb_rescale (0 or 1) DivRoundByLastModulus steps, as ONE launch: every input limb
 * is read once, the sum before the division is never stored.  1 <= n <= 16 ciphertexts with the ids of out, each with at least
 * Lc = limbs(out) + nb_rescale limbs (their first Lc limbs are read: an implicit DropLevel, as in mkhe_ct_sum); out must not alias an input.
 * dev_consts = device uint64[n + 1][2][Lc] (mkhe_buf_alloc; read when the call executes, so the call is legal inside a capture):
 * row 0 = (add_re, add_im) as plain canonical residues, rows 1 .. n = (re_k, im_k) in Montgomery form, reduced.
 * This is NOT the MultByConst convention of the reference (mkhe_ct_mul_const, the half-split of mkckks/evaluator.go:150-196) and has no reference
 * counterpart: it is defined by i <-> X^(N/2) in the coefficient domain (every slot root zeta^(5^j) raised to N/2 is i, since 5^j = 1 mod 4).  With
 * h = N/2 and j < h, per limb l < Lc and for every polynomial of the ciphertexts, mod q_l and canonical:
 *   acc[j]     = sum_k re_k[l] x_k[j]     - im_k[l] x_k[j + h]
 *   acc[j + h] = sum_k re_k[l] x_k[j + h] + im_k[l] x_k[j]
 * and on polynomial 0 only acc[0] += add_re[l], acc[h] += add_im[l].  With nb_rescale = 1 out receives what mkhe_rescale(acc, 1) would, bit for bit. */
int  mkhe_ct_lincomb(mkhe_ctx* ctx, int n, const mkhe_ct* const* in, const void* dev_consts, int nb_rescale, mkhe_ct* out);
/* ==== Weighted sums, many at once: nout sums of mkhe_ct_lincomb from the same nin ciphertexts ===========
 * No reference counterpart; the MK-CKKS twin of mkhe_bfv_ct_lincomb: every inner sum of a baby-step / giant-step polynomial evaluation from the same
 * baby powers in one launch.
 *   out[g] = sum_b (re[g][b] + i im[g][b]) in[b] + (add_re[g] + i add_im[g]),      g < nout,
 * then nb_rescale (0 or 1) DivRoundByLastModulus steps.  i = X^(N/2) exactly as mkhe_ct_lincomb defines it: with h = N/2 and j < h, per limb l < Lc and
 * for every polynomial of the ciphertexts, mod q_l and canonical,
 *   acc_g[j]     = sum_b re[g][b][l] x_b[j]     - im[g][b][l] x_b[j + h]
 *   acc_g[j + h] = sum_b re[g][b][l] x_b[j + h] + im[g][b][l] x_b[j]
 * and on polynomial 0 only acc_g[0] += add_re[g][l], acc_g[h] += add_im[g][l].
 * Shapes: 1 <= nin <= 16, 1 <= nout <= 16; all handles carry the same ids; every output has the same number of limbs L; every input has at least
 * Lc = L + nb_rescale limbs, of which the first Lc are read (an implicit DropLevel); the outputs are distinct and alias no input.
 * dev_consts = device uint64[nout][nin + 1][2][Lc] (mkhe_buf_alloc): row [g][0] = (add_re, add_im) as plain canonical residues, row [g][1 + b] = (re, im)
 * in the engine's 2^64 Montgomery form, reduced.  The block is read when the call executes, and the call takes no pool allocation: it is legal between
 * mkhe_capture_begin and mkhe_capture_end, like mkhe_ct_lincomb.
 * Refusals: the counts (nin, nout, nb_rescale) are checked before the context is looked at; every error message starts with the name of the function;
 * a refused call enqueues nothing and leaves the context usable.  Accepted on mkckks / mkrlwe contexts that own every modulus (not on a BFV context,
 * whose call is mkhe_bfv_ct_lincomb, and not on a limb-sharded one).
 * Launch set: ONE kernel, one thread per coefficient pair (j, j + h) of one component; it reads every input limb once and writes every output limb
 * once, 8 N (1 + k) (nin Lc + nout L) bytes for k parties.  mkhe_ct_lincomb once per output reads the inputs nout times.  A pair (re, im) that is zero
 * under limb l costs no product for that limb, an im that is zero half of them (wave-uniform branches).
 * Bit-exactness: out[g] equals, bit for bit, mkhe_ct_lincomb(nin, in, row g of dev_consts, nb_rescale): both are the canonical residue of the same
 * integer, zero weights included. */
int  mkhe_ct_lincomb_multi(mkhe_ctx* ctx, int nin, const mkhe_ct* const* in, int nout, const void* dev_consts, int nb_rescale, mkhe_ct* const* out);
/* ==== Weighted sums in lock step: mkhe_ct_lincomb_multi on nbatch independent items with ONE constant block ===========
 * No reference counterpart; what mkckks.BatchEvaluator.LinCombsNew issues: item b is the nout sums of its own nin ciphertexts in[b * nin + k] into
 * out[b * nout + g], with the weights and constants all items share (the items of a batch carry one scale, so their encoded weights are the same).
 * Contract: for every item b, out[b * nout ..] equals, bit for bit, mkhe_ct_lincomb_multi(ctx, nin, in + b * nin, nout, dev_consts, nb_rescale,
 * out + b * nout); the formulas, dev_consts = device uint64[nout][nin + 1][2][Lc] and the rescale are that call's.
 * Shapes: nbatch >= 1 with no upper bound other than memory; 1 <= nin <= 16, 1 <= nout <= 16, nb_rescale 0 or 1; all handles carry the same ids; every
 * output has the same number of limbs L; input k has the same number of limbs in every item, at least Lc = L + nb_rescale (different k may differ;
 * the first Lc limbs are read).  The same handle may be input k of several items (a broadcast operand).  The outputs are pairwise distinct, and no
 * output is an input of ANY item, its own included.
 * Refusals: the counts (nbatch, nin, nout, nb_rescale) are checked before the context is looked at; every error message starts with
 * "mkhe_ct_lincomb_batch: "; a refused call enqueues nothing and leaves the context usable.  Accepted where mkhe_ct_lincomb_multi is: not on a BFV
 * context and not on a limb-sharded one.
 * Launch set: the item is a grid dimension next to the component, a thread is mkhe_ct_lincomb_multi's; 8 N (1 + k) nbatch (nin Lc + nout L) bytes.  The
 * base addresses of all handles travel in the kernel arguments: nothing is uploaded and no pool allocation is taken, so the call is legal between
 * mkhe_capture_begin and mkhe_capture_end.  One launch holds 384 / (nin + nout) items (12 at 16 x 16, 192 at 1 x 1); further items go into further
 * launches of the same kernel on the same stream. */
int  mkhe_ct_lincomb_batch(mkhe_ctx* ctx, int nbatch, int nin, const mkhe_ct* const* in /* [nbatch * nin], in[b * nin + k] */,
                           int nout, const void* dev_consts /* uint64[nout][nin + 1][2][Lc], the block of mkhe_ct_lincomb_multi */,
                           int nb_rescale, mkhe_ct* const* out /* [nbatch * nout], out[b * nout + g] */);
/* mkckks.Evaluator.MulPtxtNew body (evaluator.go:465-478) without its Rescale: every component times the plaintext
 * polynomial dev_pt = uint64[limbs][N] (coefficient domain, device), via NTT / MForm / InvNTT. */
int  mkhe_ct_mul_ptxt(mkhe_ctx* ctx, const mkhe_ct* in, const void* dev_pt, mkhe_ct* out);

/* ---- B independent operations of ONE shape per call (round 4; no reference counterpart: the reference evaluates one ciphertext at a time).
 *      On the small rings (PN14QP439, mkckks/mkckks_benchmark_test.go:13; cnn's PN14QP433, cnn/cnn_test.go:80-96) an operation is a chain of
 *      launches of a few dozen limbs each; B inputs in lock step are the same launches with B times the items.  All ciphertexts of one list
 *      have the same ids and limb count; keys and CRS are per party and shared by the inputs; an operand that is the same ciphertext for
 *      every input (cnn's model) is passed nbatch times; outputs are distinct handles, and output k must not be an INPUT of another item j != k
 *      (an error: the items of a batch run as one launch set, in no order; output k may be input k where the single operation may run in place).
 *      Hoisted forms are flat lists [b * n + a] (input b,
 *      party component a) or NULL (the engine hoists).  Each output equals the single-operation entry point's, bit for bit.
 *        mkhe_hoisted_form_batch : mkckks.Evaluator.HoistedForm            mkckks/evaluator.go:543-553
 *        mkhe_rotate_batch       : KeySwitcher.RotateHoisted / Rotate      mkrlwe/keyswitch_hoisted.go:183-247, keyswitch.go:234-298
 *        mkhe_mul_relin_batch    : KeySwitcher.MulAndRelin[Hoisted] (+ the single Rescale of mkckks.Evaluator.mulRelinHoisted when rescale != 0:
 *                                  out is then one level below the product)     keyswitch_hoisted.go:44-179, mkckks/evaluator.go:558-581
 *        mkhe_ct_binary_batch    : op 0 = AddNew, 1 = SubNew               mkckks/evaluator.go:316-356 */
/*      Handles for a batch in one call: nbatch ciphertexts of one shape (contents undefined, like mkhe_ct_create_uninit) / count switching keys,
 *      views into ONE pooled block that is returned when the last of them has been destroyed (one by one with mkhe_ct_destroy / mkhe_swk_destroy, or
 *      all of them with the *_destroy_batch calls). */
int  mkhe_ct_create_batch(mkhe_ctx* ctx, int nbatch, int n, const int* ids, int limbs, mkhe_ct** out);
void mkhe_ct_destroy_batch(mkhe_ctx* ctx, int nbatch, mkhe_ct* const* cts);
int  mkhe_swk_create_batch(mkhe_ctx* ctx, int count, mkhe_swk** out);
void mkhe_swk_destroy_batch(mkhe_ctx* ctx, int count, mkhe_swk* const* swks);
int  mkhe_hoisted_form_batch(mkhe_ctx* ctx, int level, int nbatch, const mkhe_ct* const* cts, mkhe_swk* const* out);
int  mkhe_rotate_batch(mkhe_ctx* ctx, uint64_t galEl, int nbatch, const mkhe_ct* const* in, const mkhe_swk* const* hoist,
                       const mkhe_swk* const* rk, const mkhe_swk* crs, mkhe_ct* const* out);
/*      nbatch rotations of nbatch ciphertexts of one shape, EACH by its own Galois element galEl[b] with its own keys -- rk flat [b * n + a]
 *      (rkSet.GetRotationKey(ids[a], rotidx_b)), crs[b] = params.CRS[rotidx_b], hoist flat [b * n + a] or NULL -- and, when post_add != NULL,
 *      out[b] = post_add[b] + Rotate(in[b]) with the addition of mkckks.Evaluator.AddNew (equal scales: ring.Add) on the store of the rotation:
 *      the independent rotate -> hoist -> MulRelin chains of cnn.Convolution / FC1Layer (cnn/cnn.go:16-30,51-62) as lanes of one launch set, and
 *      the "temp = RotateNew(x, r); x = AddNew(x, temp)" steps of its log-sums (:33-37,64-67,83-86,90-93) as one pass (nbatch = 1).  Bit for bit
 *      what mkhe_rotate followed by mkhe_ct_add(post_add[b], .) gives.  post_add[b] has the ids of in[b], at out's level or above, and is not an output. */
int  mkhe_rotate_multi(mkhe_ctx* ctx, int nbatch, const uint64_t* galEl, const mkhe_ct* const* in, const mkhe_swk* const* hoist,
                       const mkhe_swk* const* rk, const mkhe_swk* const* crs, const mkhe_ct* const* post_add, mkhe_ct* const* out);
int  mkhe_mul_relin_batch(mkhe_ctx* ctx, int nbatch, const mkhe_ct* const* op0, const mkhe_ct* const* op1,
                          const mkhe_swk* const* hoist0, const mkhe_swk* const* hoist1,
                          const mkhe_swk* const* rlk_b1, const mkhe_swk* const* rlk_d0, const mkhe_swk* const* rlk_v0,
                          const mkhe_swk* crs_u, int rescale, mkhe_ct* const* out);
int  mkhe_ct_binary_batch(mkhe_ctx* ctx, int op, int nbatch, const mkhe_ct* const* op0, const mkhe_ct* const* op1, mkhe_ct* const* out);
/*      mkckks.Evaluator.MulPtxtNew (mkckks/evaluator.go:465-481): mkhe_ct_mul_ptxt followed by nb_rescale >= 0 DivRoundByLastModulus steps (the
 *      Rescale of :480; the host decides nb_rescale from the scales, :376-384); out has limbs(in) - nb_rescale limbs */
int  mkhe_ct_mul_ptxt_batch(mkhe_ctx* ctx, int nbatch, const mkhe_ct* const* in, const void* dev_pt, int nb_rescale, mkhe_ct* const* out);

/* ---- Plaintext linear transform M z = sum_k d_k (.) rot_k(z) by baby steps and giant steps: the prepared plaintext and the dot product in the middle
 *      (no reference counterpart: the reference multiplies by one plaintext at a time, mkckks/evaluator.go:465-481).  mkckks contexts only: a BFV
 *      context and a context that owns a subset of the moduli are refused.  Every error message starts with the name of the function.
 *      pt uint64[count][limbs][N] (coefficient domain, canonical: what mkhe_ckks_encode writes) -> ptntt, same shape: MForm(NTT_l(pt_l)) under
 *      q_0 .. q_(limbs-1), i.e. mkhe_ntt (forward, not lazy) followed by x * 2^64 mod q_l: ONE forward launch of count * limbs limb-NTTs and one pointwise
 *      launch.  dev_ptntt may be dev_pt.  1 <= limbs <= nQ, 1 <= count <= 65535.  Not for use inside a capture (it may allocate). */
int  mkhe_ptxt_prepare(mkhe_ctx* ctx, int limbs, int count, const void* dev_pt, void* dev_ptntt);
/*      out[g] = sum over the set bits b of masks[g] of in[b] * P(g, b), g < ngiant: every component of in[b] times the plaintext, negacyclic product
 *      mod q_l, canonical.  P(g, b) are the prepared plaintexts (mkhe_ptxt_prepare) of pt_limbs limbs each, stored COMPACTLY in (g, b) order: plaintext
 *      number (set bits of masks[0 .. g-1]) + (set bits of masks[g] below b) lies at dev_ptntt + number * pt_limbs * N words.
 *      1 <= nin <= 16, 1 <= ngiant <= 64; every mask is non-zero and has no bit >= nin; all in and out handles carry the same ids; L = limbs(out[0])
 *      for every output; every input has >= L limbs, of which the first L are read (an implicit DropLevel, as in mkhe_ct_sum); pt_limbs >= L; the
 *      outputs are distinct and alias no input.  masks is a HOST array consumed at call time (it travels in the kernel arguments), the temporaries
 *      come from the context's pools: after one call of the shape the call is legal between mkhe_capture_begin and mkhe_capture_end.
 *      Launch set: one forward NTT of all nin * (1 + k) * L limbs, one product kernel that reads every transformed input limb once and every present
 *      plaintext word once per component, one inverse NTT of ngiant * (1 + k) * L limbs into the outputs.
 *      Bit-exactness: out[g] equals, bit for bit, mkhe_ct_sum over the set bits b of mkhe_ct_mul_ptxt(in[b] dropped to L limbs, pt(g, b)), pt being the
 *      coefficient-domain plaintext that mkhe_ptxt_prepare was given: both are the canonical residue of the same integer. */
int  mkhe_ct_ptxt_dot(mkhe_ctx* ctx, int nin, const mkhe_ct* const* in, int ngiant, const uint32_t* masks,
                      const void* dev_ptntt, int pt_limbs, mkhe_ct* const* out);

/* ==== mkbfv ========================================================================================
 * Context for mkbfv.NewParametersFromLiteral (mkbfv/params.go:28-76): rings Q, QMul (same length), R = Q||QMul,
 * P and the plaintext modulus T; replaces mkbfv.NewKeySwitcher (keyswitch.go:31-65) + NewFastBasisExtender
 * (basis_extension.go:20-47).  PCount/gamma must be 1 (one prime per gadget digit), as in both reference
 * parameter sets.  Every mkrlwe-level call above works on such a context too (BFV Rotate / Conjugate use
 * mkhe_rotate / mkhe_conjugate directly: mkbfv/evaluator.go:142-207).
 * PolyR device layout: uint64[2*nQ][N], limbs 0..nQ-1 under Q, nQ..2nQ-1 under QMul. */
int  mkhe_ctx_create_bfv(mkhe_ctx** out, int logN, const uint64_t* Q, const uint64_t* QMul, int nQ,
                         const uint64_t* P, int nP, int gamma, uint64_t T, int device);
/* FastBasisExtender.ModUpQtoR / Rescale / Quantize (mkbfv/basis_extension.go:49-96) on raw device buffers:
 * npolys polynomials, polyq = [npolys][nQ][N], polyr = [npolys][2nQ][N] (Quantize: polyr in the NTT domain). */
int  mkhe_bfv_modup_q_to_r(mkhe_ctx* ctx, const void* dev_polyq, void* dev_polyr, int npolys);
int  mkhe_bfv_rescale(mkhe_ctx* ctx, const void* dev_polyq, void* dev_polyr, int npolys);
int  mkhe_bfv_quantize(mkhe_ctx* ctx, const void* dev_polyr_ntt, void* dev_polyq, int npolys);
/* ringR.NTT / InvNTT (keyswitch_hoisted.go:128-129) on [count][2nQ][N] */
int  mkhe_bfv_ntt_r(mkhe_ctx* ctx, const void* dev_src, void* dev_dst, int count, int inverse);
/* KeySwitcher.DecomposeBFV (mkbfv/keyswitch.go:67-90): one PolyR (coefficient domain) -> ad1 (Q digits), ad2 (QMul digits) */
int  mkhe_bfv_decompose(mkhe_ctx* ctx, const void* dev_polyr, mkhe_swk* ad1, mkhe_swk* ad2);
/* KeySwitcher.ExternalProductBFV (mkbfv/keyswitch.go:83-113): the non-hoisted form -- DecomposeBFV of one PolyR (coefficient
 * domain) into the engine's own pool, then the product below; c = [nQ][N], coefficient domain, canonical */
int  mkhe_bfv_external_product(mkhe_ctx* ctx, const void* dev_polyr, const mkhe_swk* bg1, const mkhe_swk* bg2, void* dev_c);
/* KeySwitcher.ExternalProductBFVHoisted (keyswitch_hoisted.go:6-34): c = ModDown_P(sum bg1.ah1 + bg2.ah2), [nQ][N] */
int  mkhe_bfv_external_product_hoisted(mkhe_ctx* ctx, const mkhe_swk* ah1, const mkhe_swk* ah2,
                                       const mkhe_swk* bg1, const mkhe_swk* bg2, void* dev_c);
/* Evaluator.MulRelinNew (mkbfv/evaluator.go:78-82) = mulRelinHoisted (:118-140) + MulAndRelinBFVHoisted
 * (keyswitch_hoisted.go:36-206).  The reference's non-hoisted twin (Evaluator.mulRelin evaluator.go:95-113 ->
 * KeySwitcher.MulAndRelinBFV keyswitch.go:115-251) decomposes the same polynomials inside its loops and yields the same
 * ciphertext bit for bit (tests/test_bfv_oracle.py); it has its own device path below (mkhe_bfv_mul_relin_unhoisted).
 * Ciphertexts at the maximum level, coefficient domain.  Key lists aligned with
 * the operand ids: rlk_b1/b2[j] = rlkSet[ids1[j]].Value[0/1].Value[0], rlk_d1/d2[i] = rlkSet[ids0[i]].Value[0/1].Value[1],
 * rlk_v[i] = rlkSet[ids0[i]].Value[0].Value[2]; crs_u = params.CRS[-1]. */
int  mkhe_bfv_mul_relin(mkhe_ctx* ctx, const mkhe_ct* op0, const mkhe_ct* op1,
                        const mkhe_swk* const* rlk_b1, const mkhe_swk* const* rlk_b2,
                        const mkhe_swk* const* rlk_d1, const mkhe_swk* const* rlk_d2,
                        const mkhe_swk* const* rlk_v, const mkhe_swk* crs_u, mkhe_ct* out);
/* K MK-BFV products under ONE Quantize and ONE relinearisation tail (no reference counterpart; the MK-BFV twin of mkhe_mul_relin_sum):
 * out = sum_k op0[k] * op1[k], an encrypted inner product mod T.  With ExtB = ExternalProductBFVHoisted, ExtH = ExternalProductHoisted,
 * (h1, h2) = DecomposeBFV and every + over Q or R canonical, for every pair k
 *   r0 = ModUpQtoR(every polynomial of op0[k]) ;  r1 = Rescale(every polynomial of op1[k])                 (evaluator.go:118-140)
 *   f0 = NTT_R(r0) ;  f1 = NTT_R(r1)
 *   z_0 += f0_0 * f1_0 ;  z_i += f1_0 * f0_i (i in ids0) ;  z_j += f0_0 * f1_j (j in ids1)                 (mod the primes of R, NTT domain)
 *   x1 = MForm(sum_i d1_i (.) h1(r0_i)), x2 with d2, h2 ;  y1, y2 with b1, b2 over the r1_j               (keyswitch_hoisted.go:86-134)
 *   e_j += ExtB(h1(r1_j), h2(r1_j), x1, x2)                                                               (step E, :176-183)
 *   t_i += ExtB(h1(r0_i), h2(r0_i), y1, y2)                                                               (step F1, :190-197)
 * and then ONCE
 *   out_o = Quantize(z_o) for every output slot ;  out_j += e_j
 *   per party i of op0:  out_0 += ExtH(h(t_i), v_i) ;  out_i += ExtH(h(t_i), u)                            (step F2, :199-205)
 * Quantize(sum z) and sum Quantize(z) differ by the rounding only, and a wrap of the sum mod R = Q * QMul is a multiple of T * Q after the
 * scaling: the same message mod T, one rounding and one gadget noise of F2 instead of K.  K = 1 is mkhe_bfv_mul_relin
 * bit for bit, and the result does not depend on the order of the pairs.
 *   1 <= K <= 16; ciphertexts at the maximum level, coefficient domain; every op0[k] carries the ids of op0[0], every op1[k] those of op1[0];
 *   out carries exactly the union and is distinct from every operand; keys aligned as for mkhe_bfv_mul_relin; every prime of Q and QMul below
 *   2^60 (one 128-bit accumulator of 2 K <= 32 products per word of z).  BFV contexts that own every modulus.
 *   Scratch, in 8-byte words: ((K + 1) (2 + |ids0| + |ids1|) + 1 + |ids_out|) * 2 nQ N -- the pairs over R in the NTT domain, ONE pair in the
 *   coefficient domain (reused) and z -- beside what mkhe_bfv_mul_relin keeps ((|ids0| + |ids1|) nQ N more for the t_i and e_j).  Grow-only and
 *   allocated by the first call of a shape: inside a capture a call that would have to allocate is refused.
 * Every message starts with the name of the call; a refused call enqueues nothing and leaves the context usable. */
int  mkhe_bfv_mul_relin_sum(mkhe_ctx* ctx, int K, const mkhe_ct* const* op0, const mkhe_ct* const* op1,
                            const mkhe_swk* const* rlk_b1, const mkhe_swk* const* rlk_b2,
                            const mkhe_swk* const* rlk_d1, const mkhe_swk* const* rlk_d2,
                            const mkhe_swk* const* rlk_v, const mkhe_swk* crs_u, mkhe_ct* out);
/* Evaluator.mulRelin (mkbfv/evaluator.go:95-113) -> KeySwitcher.MulAndRelinBFV (mkbfv/keyswitch.go:115-251): the reference's NON-hoisted
 * twin as its own device path, in the reference's order and with its pool discipline -- one pair of digit vectors that every
 * DecomposeBFV overwrites (each party component is decomposed twice), x / y accumulated party by party, every ExternalProductBFV /
 * ExternalProduct on its own.  Same arguments and the same ciphertext, bit for bit, as mkhe_bfv_mul_relin (tests/test_gpu_bfv.py); 2 digit
 * vectors of scratch instead of 4k, about twice the forward NTTs. */
int  mkhe_bfv_mul_relin_unhoisted(mkhe_ctx* ctx, const mkhe_ct* op0, const mkhe_ct* op1,
                                  const mkhe_swk* const* rlk_b1, const mkhe_swk* const* rlk_b2,
                                  const mkhe_swk* const* rlk_d1, const mkhe_swk* const* rlk_d2,
                                  const mkhe_swk* const* rlk_v, const mkhe_swk* crs_u, mkhe_ct* out);
/* Party-sharded BFV MulRelinNew (no reference counterpart; mkhe_kklss_amd/dist.py ShardedBfvMulRelin; keyswitch_hoisted.go:76-206
 * is the structure being cut): every rank holds c_0 and BOTH components of the parties it owns (Quantize rounds, so the two tensor
 * terms of an output slot must meet on one rank).  mkhe_bfv_mr_partial: conversions, tensor + Quantize into `out` (out_0 only where
 * with_c0), DecomposeBFV, and the rank's canonical partial sums of x1, x2, y1, y2 -- to be summed over the ranks and folded with
 * mkhe_swk_fold(mform = 1); mkhe_bfv_mr_finish: steps E and F with the complete sums; out_0 and out_i are then partial
 * sums / owner slots to be exchanged and folded with mkhe_ct_fold.  mkhe_bfv_mul_relin == partial(with_c0 = 1) + finish on one rank. */
int  mkhe_bfv_mr_partial(mkhe_ctx* ctx, const mkhe_ct* op0, const mkhe_ct* op1,
                         const mkhe_swk* const* rlk_b1, const mkhe_swk* const* rlk_b2,
                         const mkhe_swk* const* rlk_d1, const mkhe_swk* const* rlk_d2, int with_c0, mkhe_ct* out,
                         mkhe_swk* x1, mkhe_swk* x2, mkhe_swk* y1, mkhe_swk* y2);
int  mkhe_bfv_mr_finish(mkhe_ctx* ctx, const mkhe_ct* op0, const mkhe_ct* op1, const mkhe_swk* x1, const mkhe_swk* x2,
                        const mkhe_swk* y1, const mkhe_swk* y2, const mkhe_swk* const* rlk_v, const mkhe_swk* crs_u, mkhe_ct* out);

/* ==== key generation and CRS expansion =========================================
 * mkrlwe/keygen.go, mkbfv/keygen.go, mkrlwe/params.go:16-61,77-99.  The reference draws secrets, errors and CRS from
 * lattigo's crypto PRNG (utils.NewPRNG: keygen.go:26, params.go:28,79), so no output of it can be reproduced bit for
 * bit; what is reproduced is the ring arithmetic applied to the samples:
 *  - secrets / errors are SAMPLES supplied by the caller as host int32 arrays, N small signed coefficients per
 *    polynomial (what ring.TernarySampler / ring.GaussianSampler draw; the Go shim copies them out of its own samplers,
 *    so the secret randomness never comes from the GPU),
 *  - a SecretKey is a device PolyQP buffer uint64[nQ+nP][N] (mkhe_buf_alloc), NTT domain, Montgomery form
 *    (SecretKey.Value, keygen.go:44-55),
 *  - keys are written into SwitchingKey handles in the layout every other entry point expects. */
/* genSecretKeyFromSampler keygen.go:44-55 */
int  mkhe_keygen_secret(mkhe_ctx* ctx, const int32_t* s, void* dev_sk);
/* GenSwitchingKey keygen.go:270-327: g*sk + e; e = int32[betaMax][N] */
int  mkhe_keygen_switching_key(mkhe_ctx* ctx, const void* dev_sk, const int32_t* e, mkhe_swk* out);
/* GenPublicKey keygen.go:88-109: dev_pk = uint64[2][nQ+nP][N], pk[0] = NTT(e) - sk*a, pk[1] = a = CRS[0].Value[0]; e = int32[N] */
int  mkhe_keygen_public_key(mkhe_ctx* ctx, const void* dev_sk, const int32_t* e, const mkhe_swk* crs_a, void* dev_pk);
/* GenRelinearizationKey keygen.go:137-187: (b, d, v) from sk, the auxiliary secret r, a = CRS[0], u = CRS[-1];
 * e = int32[3][betaMax][N], the errors of b, d, v in this order */
int  mkhe_keygen_relin_key(mkhe_ctx* ctx, const void* dev_sk, const void* dev_r, const int32_t* e,
                           const mkhe_swk* crs_a, const mkhe_swk* crs_u, mkhe_swk* b, mkhe_swk* d, mkhe_swk* v);
/* GenRotationKey keygen.go:190-229: galEl = 5^rotidx mod 2N, crs = CRS[rotidx]; e = int32[betaMax][N] */
int  mkhe_keygen_rotation_key(mkhe_ctx* ctx, uint64_t galEl, const void* dev_sk, const int32_t* e,
                              const mkhe_swk* crs, mkhe_swk* out);
/* GenConjugationKey keygen.go:240-268: crs = CRS[-2] */
int  mkhe_keygen_conjugation_key(mkhe_ctx* ctx, const void* dev_sk, const int32_t* e, const mkhe_swk* crs, mkhe_swk* out);
/* mkbfv GenBFVSwitchingKey (mkbfv/keygen.go:91-162), one of its two loops: g = uint64[betaMax][nQ+nP], the residues
 * (plain, < modulus) of the big-integer gadget scalars Gi (:104-116 resp. :137-149), computed by the caller */
int  mkhe_bfv_keygen_switching_key(mkhe_ctx* ctx, const void* dev_sk, const uint64_t* g, const int32_t* e, mkhe_swk* out);
/* mkbfv GenRelinearizationKey (mkbfv/keygen.go:24-88): a1 = CRS[0], a2 = CRS[-3], u = CRS[-1];
 * e = int32[5][betaMax][N] for b1, b2, d1, d2, v */
int  mkhe_bfv_keygen_relin_key(mkhe_ctx* ctx, const void* dev_sk, const void* dev_r, const uint64_t* g1, const uint64_t* g2,
                               const int32_t* e, const mkhe_swk* crs_a1, const mkhe_swk* crs_a2, const mkhe_swk* crs_u,
                               mkhe_swk* b1, mkhe_swk* b2, mkhe_swk* d1, mkhe_swk* d2, mkhe_swk* v);
/* CRS[idx] (params.go:47-59, AddCRS :77-99) expanded on the device from a public seed instead of uploaded (56 MiB each
 * at PN15QP880): limb (digit i, modulus j) coefficient w = MForm(first of the 64-bit words of
 * Philox4x32-10(key = seed, counter = {w, i*(nQ+nP)+j, idx, block}), block = 0, 1, ..., two words per block, masked to
 * bitlen(q_j) bits, that is < q_j) -- the mask-and-reject shape of lattigo's ring.UniformSampler.  Parties that share
 * the seed derive the same CRS. */
int  mkhe_crs_expand(mkhe_ctx* ctx, uint64_t seed, int32_t idx, mkhe_swk* out);

/* ==== public-key encryption and decryption ==========================================================
 * mkrlwe/encryptor.go:55-118 (ciphertexts are coefficient domain: the branch :95-112) and mkrlwe/decryptor.go:26-66, which
 * mkckks/{encryptor,decryptor}.go and mkbfv/{encryptor,decryptor}.go wrap; ring Q, on mkhe_ctx_create_bfv contexts too.
 * As in key generation the small-norm samples come from the caller (host int32) -- or, with mkhe_encrypt_seeded, from a ChaCha20
 * keystream expanded on the device -- and are wiped from the device scratch behind their last use.  Public keys are the device buffers of mkhe_keygen_public_key, secret keys those of
 * mkhe_keygen_secret; raw device buffers must be 16-byte aligned (mkhe_buf_alloc's are). */
/* Encrypt encryptor.go:55-118 for `count` plaintexts under one public key as one launch set: dev_pt = uint64[count][level+1][N],
 * coefficient domain or (pt_is_ntt, :107-109) NTT domain; samples = int32[count][3][N], per plaintext u (ternary), e0, e1
 * (Gaussian) in this order; out[b] = a ciphertext over exactly one party with level+1 limbs: c0 = u*pk0 + e0 + pt, c1 = u*pk1 + e1 */
int  mkhe_encrypt(mkhe_ctx* ctx, int level, int count, const void* dev_pk, const void* dev_pt, int pt_is_ntt,
                  const int32_t* samples, mkhe_ct* const* out);
/* ---- device-side sampling: u, e0, e1 drawn on the device from a ChaCha20 key ---------------------------------------
 * Opt-in: mkhe_encrypt above is unchanged, and key generation keeps taking host samples.  The stream is fully specified, so the
 * device path is bit-exact against a model (tests/device_sampler_model.py).
 *
 * Keystream.  The ChaCha20 block function of RFC 8439 section 2.3 (20 rounds, 32-bit words, feed-forward addition) on the state
 *   words 0-3  the constants 0x61707865 0x3320646e 0x79622d32 0x6b206574
 *   words 4-11 key[0..7]
 *   word 12    the block index c
 *   word 13    nonce & 0xffffffff
 *   word 14    nonce >> 32
 *   word 15    stream
 * One stream is one polynomial of N coefficients.  Coefficient i uses block c = i / 8 and there the output words w[2 (i % 8)] (low)
 * and w[2 (i % 8) + 1] (high): the 64-bit value r = lo + 2^32 hi.  Every coefficient consumes 64 bits whatever its kind.  (One GPU
 * thread computes one block: 8 consecutive coefficients, 32 contiguous bytes of int32.)
 *
 * Kinds.
 *   kind 0  ternary with P(0) = 1/2 (the u of Encrypt): 0 if r & 1, otherwise +1 if r & 2, else -1
 *   kind 1  table sampling: cdt[0 .. ncdt) are strictly increasing uint64 thresholds, ncdt even, 2 <= ncdt <= 64; the value is
 *           #{t : r >= cdt[t]} - ncdt/2.  The engine does not know sigma: the distribution is the table (mkrlwe.small_cdt /
 *           mkhe::mkrlwe::small_cdt build the rounded Gaussian truncated at 6 sigma).  Every threshold is visited for every
 *           coefficient with a full 64-bit unsigned comparison: no early exit, no sample-dependent branch.
 *
 * Rules.
 *   - A (key, nonce) pair must NEVER serve two calls: the second call would repeat the samples of the first.  The caller keeps a counter.
 *   - Both calls are refused between mkhe_capture_begin and mkhe_capture_end: a replay of the graph would repeat the keystream.
 *   - Both calls are refused on a context that owns a subset of the moduli (mkhe_ctx_set_owned).
 *   - The key travels in the kernel arguments of one launch.  The engine does not write it to device memory it owns, does not keep it in
 *     the context and does not quote it in an error message.
 *   - Every error message starts with the function's name; a refused call has enqueued nothing and leaves the context usable. */
/* dev_out = int32[count][N] (16-byte aligned device buffer); polynomial p is stream first_stream + p; first_stream + count <= 2^32;
 * 1 <= count <= 196605.  cdt / ncdt are read for kind 1 only (kind 0: NULL / 0).  A diagnostic and test entry point: the caller owns
 * (and wipes) what it asked for. */
int  mkhe_sample_small(mkhe_ctx* ctx, int kind, int count, const uint32_t key[8], uint64_t nonce, uint32_t first_stream,
                       const uint64_t* cdt, int ncdt, void* dev_out);
/* mkhe_encrypt with samples[b][j] = stream 3 b + j of (key, nonce): j = 0 is u (kind 0), j = 1, 2 are e0, e1 (kind 1) -- bit for bit.
 * CKKS, mkrlwe and BFV contexts alike.  Nothing but the arguments crosses the bus, and for count <= 16 the call does not synchronise
 * with the host (above that the output pointers are staged, as in mkhe_encrypt). */
int  mkhe_encrypt_seeded(mkhe_ctx* ctx, int level, int count, const void* dev_pk, const void* dev_pt, int pt_is_ntt,
                         const uint32_t key[8], uint64_t nonce, const uint64_t* cdt, int ncdt, mkhe_ct* const* out);
/* ---- secret-key encryption with a seeded c1: half-size fresh ciphertexts ------------------------------------------------------------
 * No reference counterpart (lattigo: NewEncryptor(params, sk), NewPRNGEncryptor); the definitions are this project's own.  A party that
 * encrypts its OWN data holds a secret key and needs no public key: c1 is a uniform polynomial a expanded from a PUBLIC 32-byte seed, and
 * c0 = pt + e - a s.  Only c0 and the seed travel (limbs * N * 8 + 40 bytes against 2 * limbs * N * 8), the phase error is e alone
 * (|e| <= ncdt / 2, against about sigma sqrt(N) of the public-key form), and one forward and one inverse NTT are run per ciphertext.
 *
 * Kind 6 of the keystream above: uniform mod q_j, keyed by a PUBLIC pair (a_key, a_nonce).  Row (b, j) is item b, limb j < limbs of Q; it owns
 * the streams 2 (b nQ + j) (lo) and 2 (b nQ + j) + 1 (hi), with nQ the context's number of Q primes -- NOT limbs: the rows of an item do not
 * depend on the level they are expanded at, and expanding fewer limbs is an implicit DropLevel.  Coefficient n takes the 64-bit values lo, hi of
 * coefficient n of the two streams (block n / 8, words 2 (n % 8) and 2 (n % 8) + 1) and, with r = hi 2^64 + lo,
 *     a[b][j][n] = (r q_j) >> 128,
 * which lies in [0, q_j) and is uniform to within q_j / 2^128 (< 2^-67).  No division, no rejection, no sample-dependent branch.  The value is
 * canonical and in the coefficient domain: a IS the c1 of the ciphertext.
 *
 * Ciphertext.  For item b, with s the party's secret (a mkhe_keygen_secret buffer, Q limbs read), out[b] is a ciphertext over exactly one
 * party with level + 1 limbs:
 *     c1[j][n] = a[b][j][n]
 *     c0[j][n] = (pt[b][j][n] + (e_b[n] mod q_j) - InvNTT(NTT(c1_j) * s_j)[n]) mod q_j        canonical
 * pt = uint64[count][level+1][N], canonical, coefficient domain or (pt_is_ntt) NTT domain: it then rides in the one inverse NTT, as in
 * mkhe_encrypt.  Consequently mkhe_decrypt(out[b], s) returns (pt + e) mod q_j EXACTLY: the phase error is e and nothing else.
 * One launch set whatever count is: sample, one forward NTT of count * limbs rows, product, one inverse NTT, finish.
 *
 * Rules: those of the seeded encryption for the two encrypt calls -- refused between mkhe_capture_begin and mkhe_capture_end and on a context
 * that owns a subset of the moduli; 1 <= count <= 65535; raw buffers 16-byte aligned; the ncdt rules of kind 1; outputs distinct, over one
 * party, with level + 1 limbs; messages start with the function's name; a refused call has enqueued nothing.  In addition:
 *   - An (a_key, a_nonce) pair serves ONE encrypt call under a given secret key: a repeated a with two plaintexts gives c0 - c0' =
 *     pt - pt' + e - e', which REVEALS THE DIFFERENCE of the plaintexts.  The caller keeps a counter.  (a_key, a_nonce) are public all the same.
 *   - a_key equal to e_key word for word is refused: the public seed would publish the key of the secret stream.
 *   - e_key travels in the kernel arguments of one launch only.  The work buffer that held NTT(c1) * s -- which gives s away, c1 being public --
 *     and the staged e are wiped behind the finish kernel.
 *   - CKKS, mkrlwe and BFV contexts alike. */
/* diagnostic / test: dev_out = uint64[count][limbs][N], rows (b, j) as defined above; 1 <= limbs <= nQ.  count > 16 stages a pointer table,
 * which synchronises (and is refused inside a capture). */
int  mkhe_sample_uniform(mkhe_ctx* ctx, int limbs, int count, const uint32_t a_key[8], uint64_t a_nonce, void* dev_out);
/* e = host int32[count][N] (as mkhe_encrypt takes its samples): e_b is row b */
int  mkhe_encrypt_sk(mkhe_ctx* ctx, int level, int count, const void* dev_sk, const void* dev_pt, int pt_is_ntt,
                     const uint32_t a_key[8], uint64_t a_nonce, const int32_t* e, mkhe_ct* const* out);
/* e_b = stream b of the SECRET (e_key, e_nonce), kind 1 on cdt: formed in registers by the finish kernel, never in memory -- bit for bit
 * mkhe_encrypt_sk on those samples.  Nothing but the arguments crosses the bus, and for count <= 16 the call does not synchronise with the host. */
int  mkhe_encrypt_sk_seeded(mkhe_ctx* ctx, int level, int count, const void* dev_sk, const void* dev_pt, int pt_is_ntt,
                            const uint32_t a_key[8], uint64_t a_nonce, const uint32_t e_key[8], uint64_t e_nonce,
                            const uint64_t* cdt, int ncdt, mkhe_ct* const* out);
/* receiver: writes polynomial 1 of out[b] (one party, any limb count <= nQ, the same for every out of the call) = rows (b, j), j < limbs(out[b]);
 * polynomial 0 is left untouched.  One launch; count > 16 stages a pointer table, which synchronises (and is refused inside a capture). */
int  mkhe_ct_expand_seeded(mkhe_ctx* ctx, int count, const uint32_t a_key[8], uint64_t a_nonce, mkhe_ct* const* out);
/* PartialDecrypt decryptor.go:26-43: slot = 1 .. n names the party (the ciphertext slot of its polynomial); out is over the ids of
 * `in` without that one, at the same level: out[0] = in[0] + c_slot*sk (one ring.Add), the other polynomials are copied.
 * WARNING: the output REVEALS THE SECRET KEY of whoever ran the call to anyone who sees it: in[0] and c_slot are public and c_slot is
 * invertible with overwhelming probability, so sk = (out[0] - in[0]) / c_slot.  The reference uses it only where one process holds every
 * key (its tests).  Between parties use mkhe_decrypt_share / mkhe_decrypt_merge below. */
int  mkhe_partial_decrypt(mkhe_ctx* ctx, const mkhe_ct* in, int slot, const void* dev_sk, mkhe_ct* out);
/* Decrypt decryptor.go:48-66: dev_sk[i] = the secret of the party at slot 1+i; dev_pt_out = uint64[limbs][N], canonical residues,
 * coefficient domain.  More than 16 parties stage the pointer tables of the keys and the polynomials, which synchronises (and is refused inside a
 * capture, with nothing enqueued). */
int  mkhe_decrypt(mkhe_ctx* ctx, const mkhe_ct* ct, const void* const* dev_sk, void* dev_pt_out);
/* ---- distributed decryption: flooded decryption shares and their merge (eprint 2022/347) ----------------------------
 * mkhe_decrypt needs every secret key in one place, and the output of mkhe_partial_decrypt gives the key away.  In the protocol of the
 * scheme party i publishes a SHARE mu_i = c_i * s_i + e_i, where e_i is a flooding ("smudging") noise much wider than the noise of the
 * ciphertext, and anyone forms c_0 + sum_i mu_i.
 *
 * Kind 2 of the keystream above: uniform, `bits` wide.  For 1 <= bits <= 62 coefficient i of stream s takes the same 64-bit r as kinds 0 and 1
 * (block i / 8, words 2 (i % 8) and 2 (i % 8) + 1) and
 *     e = (r >> (64 - bits)) - 2^(bits-1),   so that e is uniform on [-2^(bits-1), 2^(bits-1)).
 * bits = 0 means e = 0: no stream is read and the key may be NULL (tests only: such a share is PartialDecrypt's product and reveals the key).
 * The smudging lemma is stated for this uniform distribution; a wide Gaussian has no bit-exact definition from 64 bits per coefficient.
 * The sample is formed in registers by the kernel that adds it (one thread = one ChaCha20 block = 8 coefficients, reduced per limb without a
 * sample-dependent branch): it never exists in memory.  The engine does not choose `bits`: that depends on the noise of the ciphertext (mkhe_noise_norm measures it).
 *
 * Noise budget.  The merge adds sum_i e_i with |sum_i e_i| <= k 2^(bits-1) per coefficient (k parties).  CKKS: every slot moves by at most
 * N k 2^(bits-1) / scale (triangle inequality over the N unit-modulus roots of the embedding).  BFV: the message stays exact as long as
 * k 2^(bits-1) plus the noise of the ciphertext is below Q / (2 T).
 *
 * Rules: those of the seeded encryption.  A (key, nonce) pair serves ONE call; mkhe_decrypt_share with flood_bits > 0 is refused between
 * mkhe_capture_begin and mkhe_capture_end (a replay would repeat the keystream).  A call that draws no keystream MAY be captured as long as it
 * stages no pointer table: refused inside a capture are mkhe_decrypt_share with flood_bits = 0 and count > 16, mkhe_decrypt_merge with count > 16
 * or nshares > 16, and mkhe_decrypt of a ciphertext over more than 16 parties (a staged table is copied from the host and waited for, which a
 * capturing stream cannot do).  The scratch of these calls (the products, the pointer tables) is grow-only and allocated at the first call of
 * a shape: a call to be captured must have run once with that shape, or a larger one, BEFORE mkhe_capture_begin -- replacing a scratch block
 * waits for the stream, which invalidates the capture, and this the engine does not check.  The same holds for the other calls of the protocol
 * family that may be captured (mkhe_pcks_merge, mkhe_limbs_sum, mkhe_threshold_additive_key, mkhe_sample_uniform, mkhe_ct_expand_seeded).
 * Both calls are refused on a context that owns a subset of the moduli; the key travels only in
 * the kernel arguments of one launch and its host copy there is overwritten behind the launch; messages start with the function's name;
 * a refused call has enqueued nothing and leaves the context usable.  Also refused: flood_bits outside 0 .. 62, a slot out of range,
 * ciphertexts at different levels, ciphertexts over different ids in the merge, a misaligned buffer, a NULL key with flood_bits > 0. */
/* dev_shares = uint64[count][limbs][N]: share[b][j][n] = (InvNTT(NTT(c_slot) * sk)[j][n] + (e_b[n] mod q_j)) mod q_j, canonical, where c_slot is
 * polynomial slots[b] (1 .. n_b) of in[b] and e_b is stream b of (key, nonce), kind 2 with flood_bits bits.  All in[b] are at one level; their id
 * sets may differ.  One launch set whatever count is (one forward NTT of count polynomials, one product kernel, one inverse NTT, one finish
 * kernel); the unflooded product is wiped from the engine's scratch behind the finish kernel.  1 <= count <= 65535; count > 16 stages a
 * pointer table, which synchronises (and is refused inside a capture). */
int  mkhe_decrypt_share(mkhe_ctx* ctx, int count, const mkhe_ct* const* in, const int* slots, const void* dev_sk, const uint32_t key[8],
                        uint64_t nonce, int flood_bits, void* dev_shares);
/* dev_pt_out = uint64[count][limbs][N]: pt[b] = (c_0[b] + sum_i share_i[b]) mod q_j, canonical.  All in[b] are over the same ids and at the same
 * level; nshares = the number of parties, dev_shares[i] = the buffer uint64[count][limbs][N] of the party at slot 1 + i (what that party's
 * mkhe_decrypt_share wrote for the same batch).  One streaming launch.  With flood_bits = 0 shares the result is mkhe_decrypt's, bit for bit.
 * nshares = 0 on ciphertexts without parties reduces c_0.  count > 16 or nshares > 16 stages a pointer table, which synchronises (and is refused
 * inside a capture). */
int  mkhe_decrypt_merge(mkhe_ctx* ctx, int count, const mkhe_ct* const* in, int nshares, const void* const* dev_shares, void* dev_pt_out);
/* ---- collective refresh: masked shares, re-encryption, exact lift (the interactive bootstrapping of multiparty RLWE) -----------------
 * Every MulRelin drops a level and at level 0 the evaluator stops; there is no bootstrapping here.  Parties that publish decryption shares
 * are online anyway, and can REFRESH a ciphertext instead: every party masks its share with a secret uniform polynomial M_i and encrypts
 * -M_i under its own public key at the output level; anyone adds c_0 and the shares, lifts the sum -- the message plus sum_i M_i, which
 * hides it -- exactly to the output moduli and adds the re-encryptions, which cancel the masks.  The result encrypts the same message over
 * the same parties at the output level, and nobody has seen the message.
 *
 * Notation.  ct = (c_0, c_1 .. c_k) over ids, at level l, with Lin = l + 1 limbs and Q_l = q_0 .. q_l; Lout = the limbs of the output,
 * 1 <= Lout <= nQ.
 *
 * Kind 3 of the keystream: wide uniform, `bits` wide, 1 <= bits <= 120.  A mask polynomial uses TWO streams of (key, nonce_mask): coefficient n
 * takes the 64-bit value lo from stream 2 b under the block and word rule of kinds 0-2 (block n / 8, words 2 (n % 8) and 2 (n % 8) + 1) and hi
 * the same way from stream 2 b + 1.  With r = hi 2^64 + lo:
 *     M[n] = (r >> (128 - bits)) - 2^(bits-1),   uniform on [-2^(bits-1), 2^(bits-1)).
 * bits = 0 means M = 0: no mask stream is read (tests only: such a share is PartialDecrypt's product and reveals the key).  Every stream still
 * yields 64 bits per coefficient.  (Why two streams: at scale 2^54 a 62-bit flood hides the message by 8 bits only.)
 *
 * What the caller must ensure.  The engine cannot check that k 2^(bits-1) + |m + e| < Q_l / 2 for every coefficient (k parties, m + e the
 * message with its noise); otherwise the lift wraps.  bits minus the bit size of the message is the statistical hiding the caller gets.  The
 * engine does not choose bits.
 *
 * Rules: those of distributed decryption, on mkrlwe / CKKS contexts that own every modulus.  Refused: BFV contexts (a mask mod T is another
 * protocol: "collective refresh for MK-BFV" below); contexts with mkhe_ctx_set_owned; both calls between mkhe_capture_begin and mkhe_capture_end (the share would repeat its
 * keystream, the merge builds tables at its first use); mask_bits outside 0 .. 120; a slot out of range; inputs at different levels; in the
 * merge different ids, or a reenc that is not over exactly the id of its slot or has other than Lout limbs; an output that aliases an input; a
 * NULL key (mask_bits = 0 reads no mask stream, but the encryption draws its samples from the key all the same); a misaligned buffer; count
 * outside 1 .. 65535; mask_bits > 0 with nonce_mask == nonce_enc.  Each of the two nonces obeys the one-call rule of the seeded calls.
 * Messages start with the function's name; a refused call has enqueued nothing and leaves the context usable. */
/* Party side.  dev_shares = uint64[count][Lin][N]: share[b][j][n] = (InvNTT(NTT(c_slot) * sk)[j][n] + (M_b[n] mod q_j)) mod q_j, canonical: what
 * mkhe_decrypt_share computes, with M_b (kind 3, mask_bits bits, streams 2 b and 2 b + 1 of (key, nonce_mask)) in the place of the flood.
 * reenc[b] = a ciphertext over exactly the one id at slots[b] of in[b], with Lout limbs (its shape says what Lout is; the same for every b):
 * bit for bit what mkhe_encrypt_seeded(level = Lout - 1, count, dev_pk, pt, 0, key, nonce_enc, cdt, ncdt) writes for the plaintext
 * pt[b][j][n] = (-M_b[n]) mod q_j, canonical, coefficient domain (encryption streams 3 b, 3 b + 1, 3 b + 2 of nonce_enc).  Behind their last
 * use the engine wipes from its scratch the unmasked product (as mkhe_decrypt_share does), the plaintext -M and the samples; the key travels in
 * kernel arguments only.  count > 16 stages pointer tables, which synchronises. */
int  mkhe_refresh_share(mkhe_ctx* ctx, int count, const mkhe_ct* const* in, const int* slots, const void* dev_sk, const void* dev_pk,
                        const uint32_t key[8], uint64_t nonce_mask, uint64_t nonce_enc, int mask_bits, const uint64_t* cdt, int ncdt,
                        void* dev_shares, mkhe_ct* const* reenc);
/* Anyone.  out[b] is over the ids of in[b] with Lout limbs (its shape says what Lout is); all in[b] have the same ids and level; nshares = the
 * number of parties, dev_shares[i] and reenc[i * count + b] those of the party at slot 1 + i.
 *   1. R = (c_0 + sum_i share_i) mod Q_l: the residues mkhe_decrypt_merge gives.
 *   2. R~ = R if R <= (Q_l - 1) / 2, else R - Q_l: the exact centred integer.
 *   3. out_0[j] = ((R~ mod q_j) + sum_i reenc_i.c0[j]) mod q_j for j < Lout.
 *   4. out_(1+i) = reenc_i.c1.
 * Everything is canonical, and every limb of every component of out is written.  For j < Lin, R~ mod q_j is the residue of R itself.  With all
 * reenc zero and Lout = Lin the result is mkhe_decrypt_merge's plaintext in slot 0.  One streaming launch; the tables of the lift are built
 * at the first call. */
int  mkhe_refresh_merge(mkhe_ctx* ctx, int count, const mkhe_ct* const* in, int nshares, const void* const* dev_shares,
                        const mkhe_ct* const* reenc /* [i * count + b] */, mkhe_ct* const* out);
/* ---- collective refresh for MK-BFV: masked shares mod T, a wide flood, re-encryption, rounding -------------------------------------------
 * Every mkbfv ciphertext lives at the maximum level: depth is bounded by noise alone, and after a few MulRelin on a small ring the message is
 * gone.  The parties that publish decryption shares can reset the noise to that of a fresh encryption instead, and nobody sees the message.
 * Unlike the refresh above, which only moves a ciphertext up the modulus chain, this one REMOVES noise: the merge rounds to Z_T and scales up
 * again.  Every party masks its share with up(A_i), A_i secret and uniform mod T, floods it with e_i, and encrypts up(-A_i) under its own public
 * key; anyone adds c_0 and the shares, rounds the sum down to Z_T -- which gives (m + sum_i A_i) mod T, uniform -- scales that up and adds the
 * re-encryptions, which cancel the masks.
 *
 * Notation.  BFV context with Q = q_0 .. q_(nQ-1), plaintext modulus T, h = floor(T / 2), under the preconditions of the "BFV batch encoder"
 * section below (T prime, T = 1 mod 2N, T < 2^32, T not a prime of Q); the scaling tables are the encoder's.
 *     up(x)   = mkhe_bfv_scale_up of one coefficient:   floor((Q x + h) / T) mod q_l          for x in [0, T)
 *     down(R) = mkhe_bfv_scale_down:                    floor((T R + floor(Q / 2)) / Q) mod T for R in [0, Q)
 * ct = (c_0, c_1 .. c_k) over ids, nQ limbs, coefficient domain.
 *
 * Two more kinds of the keystream, under the block and word rule of kinds 0-3 (coefficient n of a stream takes block n / 8, words 2 (n % 8) and
 * 2 (n % 8) + 1; every stream yields 64 bits per coefficient).  Under (key, nonce_mask), item b of a call owns S = 2 + W consecutive streams
 * starting at b S, W = ceil(flood_bits / 64) (W = 0 for flood_bits = 0).
 *   Kind 4, uniform mod T (the mask): lo from stream b S, hi from stream b S + 1; with r = hi 2^64 + lo, A[n] = (r T) >> 128.  A is in [0, T) and
 *     uniform to within T / 2^128; no division, no sample-dependent branch.
 *   Kind 5, wide uniform (the flood): v_w = the 64-bit value of stream b S + 2 + w, w < W, the top word masked to its low flood_bits - 64 (W - 1)
 *     bits; F = sum_w v_w 2^(64 w), e[n] = F - 2^(flood_bits-1), uniform on [-2^(flood_bits-1), 2^(flood_bits-1)).  flood_bits = 0: e = 0, no
 *     flood stream is read.  (mkhe_decrypt_share keeps kind 2 and its 62 bits: the noise of a ciphertext worth refreshing has hundreds of bits
 *     and depends on the keys, so the flood here is as wide as the decryption margin allows.)
 *
 * Why it is right.  up(x) = Q x / T + eps with |eps| <= 1/2, so R = c_0 + sum_i share_i = (Q / T)(m + sum_i A_i) + delta mod Q with
 * delta = e_ct + sum_i e_i + sum eps, e_ct the noise of the input.  down gives w = (m + sum_i A_i) mod T exactly as long as
 *     |e_ct| + k 2^(flood_bits-1) + k / 2 < Q / (2 T),
 * and the output then decrypts to (Q / T) m plus the k fresh encryption noises plus at most (k + 1) / 2.  The engine cannot check the
 * condition and does not choose flood_bits: flood_bits minus the bit size of e_ct is the statistical hiding of the noise the caller gets.
 *
 * Rules: those of mkhe_refresh_share / mkhe_refresh_merge.  Refused: a context that is not a BFV context, or one with mkhe_ctx_set_owned; T
 * outside the encoder's preconditions; both calls between mkhe_capture_begin and mkhe_capture_end; mask other than 0 or 1; flood_bits < 0,
 * > 1024 or > bitlen(Q div 2T) - 1 (such a flood alone destroys the message; a BFV context holds at most 16 primes of Q, each below 2^60, so
 * this bound is at most 960 - bitlen(2T) on every context that can be created and it, not 1024, is the one that binds: the sixteen words of a
 * 1024-bit flood are reached by mkhe_pcks_share on a CKKS / mkrlwe chain only); a slot out of range; an input, reenc or out that does not have nQ
 * limbs; in the merge inputs over different ids, or a reenc that is not over exactly the id of its slot; an output that aliases an input; a
 * NULL key (the encryption draws its samples from it whatever mask and flood_bits are); a misaligned buffer; count outside 1 .. 65535;
 * nonce_mask == nonce_enc when mask = 1 or flood_bits > 0.  Each of the two nonces obeys the one-call rule of the seeded calls.  Messages
 * start with the function's name; a refused call has enqueued nothing and leaves the context usable. */
/* Party side.  For item b, with c_slot the polynomial slots[b] of in[b], dev_shares = uint64[count][nQ][N]:
 *     share[b][j][n] = (InvNTT(NTT(c_slot) * sk)[j][n] + up(A_b[n])[j] + (e_b[n] mod q_j)) mod q_j,   canonical.
 * reenc[b] = a ciphertext over exactly the one id at slots[b] of in[b]: bit for bit what mkhe_encrypt_seeded(level = nQ - 1, count, dev_pk, pt, 0,
 * key, nonce_enc, cdt, ncdt) writes for pt[b][j][n] = up((T - A_b[n]) mod T)[j] (encryption streams 3 b, 3 b + 1, 3 b + 2 of nonce_enc).
 * mask is 1 in normal use; mask = 0 sets A = 0, reads no mask stream and is for tests only: with flood_bits = 0 such a share is PartialDecrypt's
 * product and reveals the key.  A and e are formed in registers and never exist in memory; behind their last use the engine wipes from its
 * scratch the unmasked product, the plaintext and the samples; the key travels in kernel arguments only.  count > 16 stages pointer tables,
 * which synchronises. */
int  mkhe_bfv_refresh_share(mkhe_ctx* ctx, int count, const mkhe_ct* const* in, const int* slots, const void* dev_sk, const void* dev_pk,
                            const uint32_t key[8], uint64_t nonce_mask, uint64_t nonce_enc, int mask, int flood_bits,
                            const uint64_t* cdt, int ncdt, void* dev_shares /* uint64[count][nQ][N] */, mkhe_ct* const* reenc);
/* Anyone.  out[b] is over the ids of in[b]; all in[b] have the same ids; nshares = the number of parties, dev_shares[i] and
 * reenc[i * count + b] those of the party at slot 1 + i.
 *   1. R = (c_0 + sum_i share_i) mod Q: the residues mkhe_decrypt_merge gives.
 *   2. w = down(R), in [0, T).
 *   3. out_0[j] = (up(w)[j] + sum_i reenc_i.c0[j]) mod q_j for every j < nQ.
 *   4. out_(1+i) = reenc_i.c1.
 * Everything is canonical, and every limb of every component of out is written.  One streaming launch; w never reaches memory. */
int  mkhe_bfv_refresh_merge(mkhe_ctx* ctx, int count, const mkhe_ct* const* in, int nshares, const void* const* dev_shares,
                            const mkhe_ct* const* reenc /* [i * count + b] */, mkhe_ct* const* out);
/* ---- encryption to shares (E2S) and back (S2E): the seam of the two refreshes, opened --------------------------------------------------------
 * A collective refresh is E2S followed by S2E, welded shut: the party forms its mask, publishes the masked share, encrypts the negated mask and
 * forgets it.  The calls below stop in the middle.  E2S takes the parties from a ciphertext to ADDITIVE SHARES of its plaintext -- each party keeps
 * the negated mask it would have encrypted, anyone computes the public share from c_0 and the published shares -- and nobody sees the plaintext.
 * Between E2S and S2E the parties can do in ordinary secret sharing what no evaluator here can (comparisons, divisions, table look-ups, an arbitrary
 * shuffle).  S2E needs no entry point: every party encrypts its additive share as a plaintext (mkhe_encrypt / mkhe_encrypt_seeded) and anyone adds
 * the ciphertexts (mkhe_ct_add); the holder of the public share first adds it into its own (mkhe_limbs_sum; for BFV mod T by any means).
 *
 * mkrlwe / MK-CKKS: notation, keystream kind 3 and rules of "collective refresh" above.  The shares are exact over R_Q in the coefficient domain.
 *   mkhe_e2s_share  dev_shares = uint64[count][Lin][N]: bit for bit what mkhe_refresh_share writes to its dev_shares for the same (key, nonce_mask,
 *                   mask_bits) -- M_b from the streams 2 b and 2 b + 1.  dev_secret = uint64[count][secret_limbs][N], 1 <= secret_limbs <= nQ:
 *                   secret[b][j][n] = (-M_b[n]) mod q_j, canonical, coefficient domain: the plaintext mkhe_refresh_share encrypts when Lout =
 *                   secret_limbs.  It is the party's additive share, in a buffer the caller owns: the engine does not wipe it.  It still wipes
 *                   the unmasked product from its own scratch.  key may be NULL when mask_bits = 0 (no stream is read; tests only).
 *   mkhe_e2s_merge  steps 1-3 of mkhe_refresh_merge with no re-encryption: dev_pt_out = uint64[count][limbs_out][N], R~ mod q_j for j < limbs_out,
 *                   1 <= limbs_out <= nQ: polynomial 0 of mkhe_refresh_merge called with all-zero reenc, bit for bit.  The same kernel.
 * Identity: for j < Lin, (R~ + sum_i secret_i) mod q_j is mkhe_decrypt's plaintext, bit for bit, for any mask_bits: the masks cancel modulo every
 * prime.  Above Lin the sum is the exact centred lift of the message only under the caller's condition of "collective refresh".
 * Refused, with messages that start with the function's name: BFV contexts; contexts with mkhe_ctx_set_owned; both calls between mkhe_capture_begin
 * and mkhe_capture_end; mask_bits outside 0 .. 120; a NULL key with mask_bits > 0; a slot out of range; inputs at different levels (merge: over
 * different ids, nshares other than the number of parties); secret_limbs or limbs_out outside 1 .. nQ; a NULL or misaligned buffer; count outside
 * 1 .. 65535.  A refused call has enqueued nothing and leaves the context usable.  nonce_mask obeys the one-call rule of the seeded calls. */
int  mkhe_e2s_share(mkhe_ctx* ctx, int count, const mkhe_ct* const* in, const int* slots, const void* dev_sk, const uint32_t key[8],
                    uint64_t nonce_mask, int mask_bits, void* dev_shares /* uint64[count][Lin][N] */, int secret_limbs,
                    void* dev_secret /* uint64[count][secret_limbs][N] */);
int  mkhe_e2s_merge(mkhe_ctx* ctx, int count, const mkhe_ct* const* in, int nshares, const void* const* dev_shares, int limbs_out,
                    void* dev_pt_out /* uint64[count][limbs_out][N] */);
/* MK-BFV: notation, keystream kinds 4 and 5 and rules of "collective refresh for MK-BFV" above.  The shares are exact over Z_T, slot by slot.
 *   dev_shares = uint64[count][nQ][N]: bit for bit mkhe_bfv_refresh_share's dev_shares with mask = 1 and the same (key, nonce_mask, flood_bits); item
 *   b owns the streams b S .. b S + S - 1.  dev_secret = uint64[count][N]: secret[b][n] = (T - A_b[n]) mod T, coefficients over Z_T in the format
 *   mkhe_bfv_scale_down writes: mkhe_bfv_scale_up of it is exactly the plaintext mkhe_bfv_refresh_share encrypts, mkhe_bfv_coeffs_to_slots of it the
 *   party's additive share of the slots.  The caller owns it; the engine wipes the unmasked product from its scratch.
 * The public side needs no entry point: mkhe_decrypt_merge followed by mkhe_bfv_scale_down gives w = (m + sum_i A_i) mod T coefficient-wise (under
 * the condition on the noise stated there), so w + sum_i secret_i = m (mod T) coefficient-wise, and slot by slot after mkhe_bfv_coeffs_to_slots.
 * Refused: what mkhe_bfv_refresh_share refuses (there is no mask argument and no nonce_enc). */
int  mkhe_bfv_e2s_share(mkhe_ctx* ctx, int count, const mkhe_ct* const* in, const int* slots, const void* dev_sk, const uint32_t key[8],
                        uint64_t nonce_mask, int flood_bits, void* dev_shares /* uint64[count][nQ][N] */, void* dev_secret /* uint64[count][N], each < T */);
/* ---- collective public-key switch: shares under a recipient's public key and their merge (PCKS of multiparty RLWE) ------------------------
 * mkhe_decrypt_merge gives the plaintext in the clear to whoever merges and to everyone who sees the shares.  With this protocol a result goes to
 * ONE recipient -- a client who is not among the computing parties, or one of them alone: every party publishes one share made from its secret key
 * and the recipient's PUBLIC key, anyone adds the shares to c_0, and the result is an ordinary ciphertext over exactly the recipient's id, which the
 * recipient decrypts with mkhe_decrypt on its own key or goes on computing with.  Nobody else learns the message, and the recipient need not be
 * online.  No reference counterpart.
 *
 * Notation.  ct = (c_0, c_1 .. c_k) over ids, coefficient domain, L = level + 1 limbs, Q_l = q_0 .. q_l.  pk_R = (pk0, pk1) is the recipient's
 * public key as mkhe_keygen_public_key writes it: uint64[2][nQ+nP][N], NTT, Montgomery form; limb j of pk0 is row j, limb j of pk1 row nQ+nP + j.
 * Party i, for item b of a call, with c_slot the polynomial slots[b] of in[b]:
 *     h0 = InvNTT(NTT(c_slot) * sk_i + NTT(u) * pk0) + E      (mod q_j, canonical)
 *     h1 = InvNTT(                     NTT(u) * pk1) + e1     (mod q_j, canonical)
 *   u   kind 0 (ternary), stream b of the call's (key, nonce)
 *   e1  kind 1 (table cdt / ncdt), stream count + b
 *   E   kind 5 (wide uniform, flood_bits wide: "collective refresh for MK-BFV" above), W = ceil(flood_bits / 64) words: word w is stream
 *       2 count + b W + w, the top word masked to its low flood_bits - 64 (W - 1) bits, E = sum_w v_w 2^(64 w) - 2^(flood_bits-1).  The flood takes
 *       the place of the e0 of an encryption: there is no separate e0.  flood_bits = 0: E = 0 and no flood stream is read (TESTS ONLY: such a share is
 *       PartialDecrypt's product plus an encryption of zero without e0, and gives the key away to the recipient at least).
 *   The block and word rule is that of kinds 0-5 (coefficient n takes block n / 8, words 2 (n % 8) and 2 (n % 8) + 1).  u * pk0 and u * pk1 are bit
 *   for bit the two products of mkhe_encrypt on the same u; c_slot * sk_i is the product of mkhe_decrypt_share.
 * Merge, by anyone:   out.c0 = c_0 + sum_i h0_i,   out.c1 = sum_i h1_i   (mod q_j, canonical), a ciphertext over one id with the limbs of the input.
 * For CKKS the scale is that of the input.
 *
 * Noise budget.  With pk_R = (-a s_R + e_R, a), the result decrypts under s_R to the phase of ct plus sum_i (u_i e_R + E_i + e1_i s_R): per
 * coefficient at most k (2^(flood_bits-1) + 2 N B), k parties, B the truncation bound of the samplers (ncdt / 2 for e1; the bound of e_R is the key
 * generator's), s_R ternary.  The engine does not choose flood_bits: flood_bits minus the bit size of the noise of ct is the statistical hiding of
 * that noise (and with it of the secret keys) the parties get.  The engine cannot check whose key dev_pk_recipient is: the caller must know it
 * is the intended recipient's -- a share under another key delivers the message to that key's owner.
 *
 * Rules: those of the seeded encryption and of distributed decryption.  A (key, nonce) pair serves ONE call; the key travels only in kernel
 * arguments and its host copy there is overwritten behind the launch; it never appears in a message.  CKKS, mkrlwe and BFV contexts alike; on a BFV
 * context every input has nQ limbs.  Refused: a context with mkhe_ctx_set_owned; mkhe_pcks_share between mkhe_capture_begin and mkhe_capture_end
 * (a replay would repeat the keystream) -- mkhe_pcks_merge MAY be captured as long as count and nshares are at most 16 (above that it stages pointer
 * tables and is refused in a capture); flood_bits < 0, > 1024 or > bitlen(Q_l div 2T') - 1 with T' = T on BFV contexts and 1 otherwise (such a flood
 * alone destroys the message); a NULL key whatever flood_bits is (u and e1 are drawn from it); a NULL or bad table (ncdt odd or outside 2 .. 64,
 * thresholds not increasing); a slot out of range; inputs at different levels; in the merge inputs over different ids, nshares other than the
 * number of parties, an out that is not over exactly one id or does not have the limbs of the input, outputs that are not distinct, an output that
 * aliases an input; a NULL or misaligned buffer; count outside 1 .. 65535.  Messages start with the function's name; a refused call has enqueued
 * nothing and leaves the context usable. */
/* Party side.  dev_shares = uint64[count][2][L][N]: (h0, h1) of item b as defined above.  All in[b] are at one level; their id sets may differ.
 * One launch set whatever count is: the sampler of u, small_expand and its forward NTT, the gathering forward NTT of the c_slot, ONE product kernel
 * for both halves, one inverse NTT of 2 count polynomials, one finish kernel that forms E and e1 in registers (they never exist in memory).
 * Behind their last use the engine wipes from its scratch u (as int32 and expanded), c_slot * sk + u * pk0 and u * pk1.  The call stages no
 * pointer table and does not synchronise with the host, whatever count is. */
int  mkhe_pcks_share(mkhe_ctx* ctx, int count, const mkhe_ct* const* in, const int* slots, const void* dev_sk, const void* dev_pk_recipient,
                     const uint32_t key[8], uint64_t nonce, int flood_bits, const uint64_t* cdt, int ncdt,
                     void* dev_shares /* uint64[count][2][L][N] */);
/* Anyone.  All in[b] are over the same ids and at the same level; nshares = the number of parties, dev_shares[i] = the buffer of the party at slot
 * 1 + i (what that party's mkhe_pcks_share wrote for the same batch); out[b] = a ciphertext over exactly one id -- the recipient's: the engine
 * cannot check which -- with the limbs of the input.  Every limb of both polynomials of out is written.  One streaming launch; count > 16 or
 * nshares > 16 stages pointer tables, which synchronises.  nshares = 0 on ciphertexts without parties gives (c_0 reduced, 0). */
int  mkhe_pcks_merge(mkhe_ctx* ctx, int count, const mkhe_ct* const* in, int nshares, const void* const* dev_shares, mkhe_ct* const* out);
/* ---- threshold secret keys: t-of-n Shamir shares, additive keys, share fold (eprint 2022/780) -----------------------------------------------
 * Every share call above needs the party's secret key, so one party that is offline or has lost its key blocks the decryption, refresh or hand-over
 * of every ciphertext it contributed to.  The answer of multiparty RLWE is t-out-of-n thresholdisation (lattigo's drlwe.Thresholdizer / Combiner):
 * a party Shamir-shares its key among n holders; any t of them turn their Shamir share into an ADDITIVE share for that active set; and because every
 * share call here is linear in the key, those t holders run the existing share calls on their additive keys and their outputs add up to the absent
 * party's share.  No reference counterpart; the definitions are this project's own.
 *
 * Notation.  R = nQ + nP is the number of rows of a SecretKey buffer uint64[R][N] (NTT domain, Montgomery form, as mkhe_keygen_secret writes it);
 * m_j is the modulus of row j: the Q primes, then the P primes.  S[j][i] is the stored word of the secret, with no conversion: Shamir sharing is
 * linear over Z_{m_j}, so it is applied to the stored words directly.  A share is therefore itself a buffer of SecretKey shape in the same
 * representation, and ANY call that takes dev_sk accepts a share or an additive key.
 *
 * Kind 7 of the keystream: uniform mod m_j over all R rows, under a SECRET (key, nonce).  Coefficient polynomial k (1 <= k <= t - 1), row j < R, owns
 * the streams 2 ((k-1) R + j) (lo) and 2 ((k-1) R + j) + 1 (hi).  The block and word rule is that of kinds 0-6 (coefficient i takes block i / 8, words
 * 2 (i % 8) and 2 (i % 8) + 1); with r = hi 2^64 + lo,
 *     c_k[j][i] = (r m_j) >> 128:
 * the formula of kind 6, indexed over R rows instead of nQ.
 *
 * Shares.  The holders have public points x_0 .. x_(n-1), each a uint32, pairwise distinct, at least 1 and smaller than every m_j of the context
 * (refused otherwise): every x_a - x_p is then invertible mod every m_j.
 *     share_p[j][i] = (S[j][i] + sum_{k=1}^{t-1} c_k[j][i] x_p^k) mod m_j                          canonical
 * Fewer than t shares say nothing about S; the t shares of an active set together ARE the key.
 *
 * Additive key, for an active set A of at least t holders with p in A, given as its points (A may be larger than t: the interpolation still holds):
 *     lambda_p[j]  = prod_{a in A, a != p} x_a (x_a - x_p)^-1  mod m_j
 *     add_p[j][i]  = share_p[j][i] lambda_p[j]  mod m_j                                            canonical
 * so that sum_{p in A} add_p = S mod m_j, word for word.  An additive key is used exactly like a key -- in particular a share made from it must be
 * FLOODED exactly like one made from a key, and a party covered by t holders contributes t floods: where a bound counts k parties, count k - 1 + t.
 *
 * Fold.  dst[b][j][i] = sum_{s < nsrc} src_s[b][j][i] mod m_j, canonical, for buffers uint64[count][limbs][N]: the outputs that the t holders'
 * share calls wrote add up to the share of the absent party.  mkhe_decrypt_share: fold the buffers (limbs = level + 1).  mkhe_pcks_share: fold with
 * count * 2 items.  mkhe_refresh_share / mkhe_bfv_refresh_share: fold the share buffers and add the holders' re-encryptions with mkhe_ct_add; the
 * merge then runs unchanged.  With limbs = R the fold adds SecretKey buffers: the additive keys of an active set give S back (tests, key recovery).
 *
 * Rules: those of the seeded encryption and of distributed decryption.  Messages start with the function's name; a refused call has enqueued
 * nothing and leaves the context usable; all three are refused on a context with mkhe_ctx_set_owned; CKKS, mkrlwe and BFV contexts alike (on a BFV
 * context the rows are those of the Q / P primes, as for the secret key); raw buffers are 16-byte aligned. */
/* dev_out[p] = uint64[R][N] <- share_p, p < nshares, of the secret at dev_sk.  1 <= threshold <= nshares <= 32.  threshold = 1 reads no stream and
 * writes S to every output (TESTS ONLY: every holder then has the key).  ONE launch: points and output pointers travel in the kernel arguments,
 * nothing is staged and the call does not synchronise with the host; the c_k are formed in registers and never exist in memory.  The key travels in
 * the kernel arguments only and its host copy there is overwritten behind the launch; it never appears in a message.  A (key, nonce) pair serves
 * ONE call.  Refused: between mkhe_capture_begin and mkhe_capture_end (a replay would repeat the keystream); a NULL key, even at threshold 1; NULL,
 * misaligned or duplicate outputs, an output equal to dev_sk; bad points (see above); threshold or nshares out of range.  The shares are key
 * material: the caller guards (and wipes) its buffers. */
int  mkhe_threshold_gen_shares(mkhe_ctx* ctx, const void* dev_sk, int threshold, int nshares, const uint32_t* points, const uint32_t key[8],
                               uint64_t nonce, void* const* dev_out /* nshares buffers uint64[R][N] */);
/* dev_out = uint64[R][N] <- add_p for the holder at `point` and the active set active_points[0 .. nactive); dev_out may equal dev_share.  The
 * threshold is not an argument: the caller's protocol knows it, and fewer than t active holders simply do not add up to S.  1 <= nactive <= 32; the
 * points valid and distinct as above; `point` occurs in active_points exactly once.  The lambda_p[j] are computed on the host and
 * travel in Montgomery form in the kernel arguments: one streaming launch, nothing staged, so the call may be captured. */
int  mkhe_threshold_additive_key(mkhe_ctx* ctx, const void* dev_share, uint32_t point, int nactive, const uint32_t* active_points,
                                 void* dev_out /* uint64[R][N]; may equal dev_share */);
/* dev_dst = uint64[count][limbs][N] <- the fold of the nsrc buffers dev_src[s] of that shape.  limbs in 1 .. nQ (row j mod q_j: what the shares of
 * every protocol here look like) or limbs == R (SecretKey rows).  1 <= nsrc <= 32, 1 <= count <= 65535.  All inputs are canonical.  dev_dst may
 * equal one dev_src[s] exactly (partial overlap is refused).  One streaming launch; nsrc > 16 stages a pointer table, which synchronises (and is
 * refused inside a capture). */
int  mkhe_limbs_sum(mkhe_ctx* ctx, int count, int limbs, int nsrc, const void* const* dev_src, void* dev_dst /* may equal one dev_src[s] exactly */);
/* ---- noise measurement: the exact centred max norm of a phase (no reference counterpart) --------------------------------------------
 * Every share call above takes a width that the caller must put above the noise of the ciphertext.  This call measures that noise on the device,
 * from a phase: what mkhe_decrypt writes for whoever holds every key, or what mkhe_decrypt_merge writes for parties that hold only their own
 * (with unflooded shares, or up to the flood otherwise).  Nothing is estimated: without the keys or their shares there is nothing to measure.
 *
 * Definitions (integers only).  For item b and limbs q_0 .. q_(L-1), L = limbs, Q = q_0 * .. * q_(L-1), and for coefficient n:
 *   kind 0, residual       x = (phase[b][.][n] - ref[b][.][n]) mod Q, given by its residues; with dev_ref == NULL, x = phase.
 *   kind 1, BFV invariant  x = (T * phase[b][.][n]) mod Q: every limb times T mod q_l (a q_l may be smaller than T).
 *   r[n] = min(x, Q - x), the magnitude of the centred representative; the result for item b is max_n r[n] and the SMALLEST n that attains it.
 * The result is in mixed-radix form: out[b] = d_0 .. d_(L-1), then n, with r = d_0 + d_1 q_0 + d_2 q_0 q_1 + .. and d_i < q_i -- the host multiplies
 * it out; no big integer exists on the device.  There x > (Q-1)/2 is a comparison of digits, top digit first; the digits of Q - x are
 * q_i - 1 - d_i plus one with carry from digit 0; the maximum over n is the lexicographic one.
 *
 * The invariant value and the noise.  A BFV phase is up(m) + e with up(m) = floor((Q m + floor(T/2)) / T), so T phase = Q m + T e + rem with |rem| < T (the
 * rounding of up), and r = |T e + rem| as long as the noise has not wrapped (T |e| + T < Q / 2).  Then
 *     |e| <= floor((r + floor(T/2)) / T) + 1 <= |e| + 2,
 * which needs no message.  The noise budget of a BFV ciphertext is bitlen(Q) - bitlen(r) - 1 >= 0 (r <= (Q-1)/2): it falls to 0 as T |e| comes
 * near Q / 2, where decryption starts to fail.  With the message at hand, kind 0 against mkhe_bfv_encode(m) gives |e| itself; for CKKS the
 * reference is mkhe_ckks_encode of the expected slots at the level and scale of the ciphertext.
 *
 * Buffers: dev_phase uint64[count][limbs][N], canonical, coefficient domain; dev_ref the same shape, ref_stride_words = limbs * N words between
 * the references of consecutive items or 0 for one reference for all (the rule of mkhe_bfv_ct_add_ptxt); dev_out uint64[count][limbs + 1].
 * 1 <= limbs <= nQ, 1 <= count <= 65535 (the items are the second grid dimension).  Kind 1: a BFV context whose T meets the encoder's
 * preconditions (T prime, T = 1 mod 2N, T < 2^32, T not a prime of Q), limbs == nQ, dev_ref == NULL.
 * Bytes: the call reads 8 * count * limbs * N bytes of dev_phase once and, with a reference, as many of dev_ref (8 * limbs * N with stride 0), and
 * writes 8 * count * (limbs + 1).  Two launches: one thread per coefficient forms the digits in a scratch of the context's pool (each digit is read
 * again by every later limb), centres them, and every workgroup of 256 selects its candidate; one workgroup per item selects among the N / 256
 * candidates.  No atomics and no dependence on the order in which workgroups run: the result is a pure function of the inputs.  The digit scratch
 * and the candidates are the noise itself, which depends on the keys: both are wiped behind the second launch.  dev_out is the caller's to guard.
 *
 * Refused, with a message that starts with `mkhe_noise_norm: `, nothing enqueued and the context left usable: kind other than 0 or 1; count outside
 * 1 .. 65535; limbs outside 1 .. nQ; kind 1 with a reference, off a BFV context or with limbs != nQ; a NULL context (after the checks above that
 * need none); a NULL dev_phase or dev_out; a misaligned buffer; ref_stride_words other than 0 or limbs * N; a context with mkhe_ctx_set_owned.
 * NOT legal between mkhe_capture_begin and mkhe_capture_end (refused there): the call grows a scratch and builds tables at its first use, and its
 * result is for the host to read. */
int  mkhe_noise_norm(mkhe_ctx* ctx, int kind, int limbs, int count, const void* dev_phase, const void* dev_ref, long ref_stride_words,
                     void* dev_out /* uint64[count][limbs + 1] */);

/* ==== raising the modulus ============================================================================
 * No reference counterpart (the reference has no bootstrapping).  The first step of one: a ciphertext at level 0, whose phase is m + e mod q_0, read
 * as integer polynomials and written under the moduli q_0 .. q_(L-1) of a higher level, where its phase is m + e + q_0 I for a small integer
 * polynomial I (|I| is about sqrt((1 + total Hamming weight of the keys) / 12): sparse keys keep it small).  The rest of a bootstrapping removes
 * q_0 I homomorphically (mkckks.Bootstrapper of the Python mirror).
 *
 * Definition (integers only).  in is at level 0: one limb, coefficient domain, canonical.  out has L = limbs(out) >= 2 limbs.  For every polynomial
 * p of the ciphertext (1 + k of them) and every coefficient x = in[p][0][n] < q_0: the centred lift is v = x for x <= (q_0 - 1) / 2 and v = x - q_0
 * above it; out[p][l][n] is the canonical residue of v mod q_l for l < L (limb 0: x itself).  q_l may be shorter than q_0 (45 against 55 bits in
 * the PN16 chain): |v| is reduced for real, with the Montgomery constants of the context, and the sign is folded in by a select, so the result is
 * exact for negative v.
 * Bytes: one streaming launch that reads 8 N (1 + k) bytes once and writes 8 N (1 + k) L: a thread holds a row of 8 coefficients in registers and
 * stores it under every modulus with 16-byte accesses.  No LDS, no scratch, no table, no upload: legal between mkhe_capture_begin and
 * mkhe_capture_end.
 *
 * Refused, with a message that starts with `mkhe_ct_mod_raise: `, nothing enqueued and the context left usable: a NULL context, in or out; a BFV
 * context; a context with mkhe_ctx_set_owned; out aliasing in; in not at level 0; out at level 0 (or with more limbs than nQ); in and out over
 * different ids. */
int  mkhe_ct_mod_raise(mkhe_ctx* ctx, const mkhe_ct* in, mkhe_ct* out);

/* ==== CKKS encoder: slots <-> RNS plaintext =========================================================
 * The message layer of mkckks/encryptor.go:42-64 (EncryptMsg, EncodeMsgNew) and mkckks/decryptor.go:34-43 (Decrypt).  Those lines call
 * lattigo's ckks.Encoder, which is not in the reference tree: what these calls restate is the canonical embedding itself, not
 * lattigo's code path.  Full packing: n = N/2 slots, slot j = the evaluation of the real coefficient vector at exp(i pi 5^j / N).
 * Buffers are device buffers (mkhe_buf_alloc; 16-byte aligned); a double is one 8-byte word, so mkhe_buf_upload / mkhe_buf_download
 * carry them as bit patterns:
 *   slots   double[count][n][2]  (re, im)
 *   coeffs  double[count][N]
 *   pt      uint64[count][limbs][N], coefficient domain, canonical: what mkhe_encrypt takes as dev_pt and mkhe_decrypt writes (count = 1)
 * `count` messages are one launch set.  Arithmetic is IEEE float64, tables rounded once from long double.  Not available on BFV
 * contexts, on a context that owns a subset of the moduli, or between mkhe_capture_begin and mkhe_capture_end (the calls
 * allocate and upload at first use); scale must be finite and > 0; 0 <= level < nQ, 1 <= limbs <= nQ; 1 <= count <= 65535 (one
 * launch set: the messages are the second grid dimension). */
/* embed (encoder side of encryptor.go:60-64): coeffs m with sum_k m_k zeta_j^k = z_j:  m_k = (2/N) Re sum_j z_j conj(zeta_j)^k */
int  mkhe_ckks_embed(mkhe_ctx* ctx, int count, const void* dev_slots, void* dev_coeffs);
/* project (decoder side of decryptor.go:34-43): z_j = sum_{k<N} m_k zeta_j^k */
int  mkhe_ckks_project(mkhe_ctx* ctx, int count, const void* dev_coeffs, void* dev_slots);
/* scale_up (encryptor.go:60-64): pt = residues of rint(coeffs * scale) (one IEEE multiply, ties to even) under q_0 .. q_level, exact
 * for every size of the rounded value.  NaN or +-inf coefficients (or products) are the caller's error: the output is unspecified. */
int  mkhe_ckks_scale_up(mkhe_ctx* ctx, int level, int count, const void* dev_coeffs, double scale, void* dev_pt);
/* scale_down (decryptor.go:34-43): coeffs = (centred lift of pt to (-Q/2, Q/2), Q = q_0 .. q_(limbs-1)) / scale, relative error below
 * 4 limbs 2^-53; the sign is decided exactly.  A magnitude beyond the float64 range gives +-inf, never NaN. */
int  mkhe_ckks_scale_down(mkhe_ctx* ctx, int limbs, int count, const void* dev_pt, double scale, void* dev_coeffs);
/* EncodeMsgNew encryptor.go:60-64 == scale_up(embed), bit for bit */
int  mkhe_ckks_encode(mkhe_ctx* ctx, int level, int count, const void* dev_slots, double scale, void* dev_pt);
/* the decoding of Decrypt decryptor.go:34-43 == project(scale_down), bit for bit */
int  mkhe_ckks_decode(mkhe_ctx* ctx, int limbs, int count, const void* dev_pt, double scale, void* dev_slots);
/* Sparse packing: n = 2^log_slots slots, 0 <= log_slots <= logN - 1 (params.LogSlots() of mkckks/encryptor.go:18,43,62), slots
 * double[count][n][2]; coeffs and pt keep their full shapes.  With the gap g = N / 2n the message is a polynomial in X^g:
 * coeffs[k g] = m'[k], k < 2n, where m' is the embedding above for the ring of degree 2n (slot j = the evaluation at exp(i pi 5^j / 2n);
 * n = 1: m' = Re z + Y Im z), and exactly 0.0 elsewhere; seen through the full embedding it is the n slots repeated N / 2n times, so
 * the evaluator acts on it slot-wise and a rotation by k rotates it by k mod n.  embed and encode write every word of their output
 * (off the grid: 0.0, residue 0 in every limb); project and decode read only the 2n coefficients on the grid, which for arbitrary
 * coefficients is the mean over the N / 2n replicas of the full projection.  encode_sparse == scale_up(embed_sparse) and
 * decode_sparse == project_sparse(scale_down), bit for bit; log_slots = logN - 1 is the four calls above, bit for bit.  Refusals
 * as above, and "<entry>: log_slots must be 0 .. <logN - 1>". */
int  mkhe_ckks_embed_sparse(mkhe_ctx* ctx, int log_slots, int count, const void* dev_slots, void* dev_coeffs);
int  mkhe_ckks_project_sparse(mkhe_ctx* ctx, int log_slots, int count, const void* dev_coeffs, void* dev_slots);
int  mkhe_ckks_encode_sparse(mkhe_ctx* ctx, int level, int log_slots, int count, const void* dev_slots, double scale, void* dev_pt);
int  mkhe_ckks_decode_sparse(mkhe_ctx* ctx, int limbs, int log_slots, int count, const void* dev_pt, double scale, void* dev_slots);
/* log2 of the largest transform (N/2 points) that one workgroup does in LDS: 13 where the runtime grants 128 KiB of dynamic LDS, else 11;
 * larger transforms take two launches over a work buffer (same bits).  -1 = error.  mkhe_ctx_set_ckks_tile lowers the limit to 11 (or
 * puts it back: 0, or the granted value), so that the two-launch form of N/2 = 2^12, 2^13 can be run and tested on any machine. */
int  mkhe_ctx_ckks_tile(mkhe_ctx* ctx);
int  mkhe_ctx_set_ckks_tile(mkhe_ctx* ctx, int log_points);

/* ==== BFV batch encoder: slots over Z_T <-> RNS plaintext ===========================================
 * The message layer of mkbfv/encryptor.go:38-41 (EncryptMsg = EncodeInt, then Encrypt) and mkbfv/decryptor.go:52-54 (DecodeInt).  Those lines
 * call lattigo's bfv.Encoder, which is not in the reference tree: what these calls restate is the mathematics of the encoder, not lattigo's
 * code path.  Definitions (N the ring degree, T the plaintext modulus of the mkhe_ctx_create_bfv context, Q the product of its ciphertext primes):
 *   psi     the primitive 2N-th root of unity mod T chosen by the rule the engine uses for the ciphertext primes: g the smallest generator
 *           >= 3 of Z_T*, psi = g^((T-1)/2N).  mkhe_ctx_bfv_slot_psi returns it.
 *   slots   a message is N values.  Slot i (0 <= i < N/2) of m(X) in Z_T[X]/(X^N+1) is m(psi^(5^i)), slot N/2+i is m(psi^(-5^i)): two rows of
 *           N/2 (lattigo's index matrix).  A rotation by k moves slot i+k to slot i within each row, the conjugation swaps the rows, the
 *           ring operations act slot by slot mod T.
 *   values  int64.  Encoding takes any int64 and uses its residue in [0, T); decoding returns the centred representative in (-T/2, T/2].
 *   scale_up    pt_l[k] = floor((Q m_k + floor(T/2)) / T) mod q_l for every limb of Q, m_k in [0, T)
 *   scale_down  floor((T x + floor(Q/2)) / Q) mod T for the residues of x in [0, Q): exact for every x (integer arithmetic only)
 * The calls need T prime, T = 1 (mod 2N) and T < 2^32 (larger T is out of scope), and T different from every prime of Q; otherwise they return an
 * error (mkhe_ctx_create_bfv itself accepts any T >= 2).  Buffers are device buffers (mkhe_buf_alloc; 16-byte aligned):
 *   slots   int64[count][N]
 *   coeffs  uint64[count][N], written < T (as an input every 64-bit value is taken mod T)
 *   pt      uint64[count][nQ][N], coefficient domain, canonical, always at the maximum level: what mkhe_encrypt takes as dev_pt and
 *           mkhe_decrypt writes (count = 1)
 * `count` messages are one launch set, 1 <= count <= 65535 (the messages are the second grid dimension).  Not available on non-BFV contexts, on a
 * context that owns a subset of the moduli (mkhe_ctx_set_owned makes none of a BFV context today), or between mkhe_capture_begin and mkhe_capture_end (the calls allocate and upload at first use). */
int  mkhe_bfv_slots_to_coeffs(mkhe_ctx* ctx, int count, const void* dev_slots, void* dev_coeffs);
int  mkhe_bfv_coeffs_to_slots(mkhe_ctx* ctx, int count, const void* dev_coeffs, void* dev_slots);
int  mkhe_bfv_scale_up(mkhe_ctx* ctx, int count, const void* dev_coeffs, void* dev_pt);
int  mkhe_bfv_scale_down(mkhe_ctx* ctx, int count, const void* dev_pt, void* dev_coeffs);
/* EncodeInt of encryptor.go:38-41 == scale_up(slots_to_coeffs), bit for bit */
int  mkhe_bfv_encode(mkhe_ctx* ctx, int count, const void* dev_slots, void* dev_pt);
/* DecodeInt of decryptor.go:52-54 == coeffs_to_slots(scale_down), bit for bit */
int  mkhe_bfv_decode(mkhe_ctx* ctx, int count, const void* dev_pt, void* dev_slots);
/* log2 of the largest transform (N points of 32 bits) that one workgroup does in LDS: 15 where the runtime grants 128 KiB of dynamic LDS, else
 * 14; larger transforms take two launches over a work buffer (same bits).  -1 = error.  mkhe_ctx_set_bfv_tile lowers the limit to any value
 * from 10 up to the granted one (or puts it back: 0), so that the two-launch form can be run and tested at small N on any machine. */
int  mkhe_ctx_bfv_tile(mkhe_ctx* ctx);
int  mkhe_ctx_set_bfv_tile(mkhe_ctx* ctx, int log_points);
/* psi of the definitions above; 0 = error (the same conditions as the encoder calls) */
uint64_t mkhe_ctx_bfv_slot_psi(mkhe_ctx* ctx);
/* BFV slot map (no reference counterpart).  A slot map is out_slot[i] = mult[i] * in_slot[index[i]] mod T for 0 <= i < N, slots numbered as above (two
 * rows of N/2); index is ANY function into 0 .. N-1 (a permutation, a replication, ..), and every such map is Z_T-linear, so it commutes with
 * additive masks mod T: applied to the public and to the secret shares of "encryption to shares" it maps the message (mkbfv.Refresher.ShareMapBatch:
 * a refresh that permutes, with no rotation key and no key switch).
 *   mkhe_bfv_slot_map_prepare   dev_index uint32[N], dev_mult uint64[N] (taken mod T; NULL = all ones) -> dev_map uint64[N], opaque: the map composed
 *       with the encoder's position table, one word per position.  Downloads, validates on the host (an index[i] >= N is refused) and uploads:
 *       synchronous, once per map.
 *   mkhe_bfv_slot_map   coeffs_out = slots_to_coeffs(map(coeffs_to_slots(coeffs_in))), bit for bit; coeffs as in the encoder calls (inputs taken mod
 *       T, outputs < T); dev_coeffs_out may equal dev_coeffs_in.  N up to the tile of mkhe_ctx_bfv_tile: ONE launch, one workgroup per message --
 *       forward transform, gather, product, inverse transform on one tile in LDS.  Larger N, or a tile lowered with mkhe_ctx_set_bfv_tile: five launches
 *       around a work buffer (wiped behind the call).  The same bits.  Whatever dev_map holds, the kernels read inside the message and write values
 *       below T: a map that mkhe_bfv_slot_map_prepare did not write gives a wrong result, never a fault.
 * Refused: what the encoder calls refuse (non-BFV contexts, T outside the preconditions, captures, NULL or misaligned buffers, count outside
 * 1 .. 65535). */
int  mkhe_bfv_slot_map_prepare(mkhe_ctx* ctx, const void* dev_index /* uint32[N] */, const void* dev_mult /* uint64[N] or NULL */,
                               void* dev_map /* uint64[N] */);
int  mkhe_bfv_slot_map(mkhe_ctx* ctx, int count, const void* dev_coeffs_in /* uint64[count][N] */, const void* dev_map,
                       void* dev_coeffs_out /* uint64[count][N] */);

/* ==== BFV plaintext operands: AddPtxt, SubPtxt, MulPtxt ===============================================
 * No reference counterpart: mkbfv.Evaluator of the reference has no operation with a plaintext operand; the definitions are this project's own, in
 * the terms of the "BFV batch encoder" section above, whose preconditions (BFV context, T prime, T = 1 mod 2N, T < 2^32, 1 <= count <= 65535,
 * non-null 16-byte-aligned device buffers, not inside a capture, not on a context that owns a subset of the moduli) and refusals apply.
 *   lift      for m = coeffs[b][k] mod T the centred representative c = m (m <= floor(T/2)) or m - T: what mkhe_bfv_decode returns.
 *             ptmul_coeff[b][l][k] = MForm(c mod q_l): the canonical residue of c under EVERY limb (q_l may be smaller than T), in the engine's
 *             2^64 Montgomery form (lattigo ring.MForm).  Coefficient domain.
 *   ptmul     uint64[count][nQ][N], the PREPARED multiplication plaintext: the forward NTT over Q (mkhe_ntt) of the lift, limb by limb, still in
 *             Montgomery form.  The NTT is Z_q-linear, so it equals MForm(NTT(c mod q_l)).
 *   pt        uint64[count][nQ][N], the scaled plaintext of mkhe_bfv_encode (coefficient domain, canonical): the operand of add / sub.
 * Why the product is right: with pt(a) = round(Q a / T) and p the centred lift of b, pt(a) p = (Q/T) [a b]_T + Q k + eps p with |eps| <= 1/2 per
 * coefficient -- no Q mod T term -- so a ciphertext of noise e decrypts after the product to a b mod T slot by slot as long as
 * N (T/2) (|e| + 1/2) < Q / (2T).  No key is used and no party is added.
 * Ciphertext lists: nbatch ciphertexts that share their ids, all at the maximum level (nQ limbs), as one launch set.  out[b] has the ids of
 * in[b]; out[b] may be in[b]; it must not be the input of another item, and the outputs are distinct.  pt_stride_words = the words between the
 * plaintexts of consecutive items: nQ * N (one plaintext per item) or 0 (one for all); any other value is an error.  The plaintext is read where it
 * lies.  Every error message starts with the name of the function. */
/* stage of mkhe_bfv_encode_mul: coeffs uint64[count][N] (taken mod T) -> ptmul_coeff uint64[count][nQ][N] */
int  mkhe_bfv_lift(mkhe_ctx* ctx, int count, const void* dev_coeffs, void* dev_ptmul_coeff);
/* slots int64[count][N] -> ptmul == mkhe_ntt(mkhe_bfv_lift(mkhe_bfv_slots_to_coeffs(slots))), bit for bit: the slot transform with the lift on
 * its store where one workgroup holds the polynomial (else the lift is a launch of its own), then ONE forward NTT of count * nQ limbs */
int  mkhe_bfv_encode_mul(mkhe_ctx* ctx, int count, const void* dev_slots, void* dev_ptmul);
/* out[b] = in[b] * plaintext, component by component: one forward NTT of all nbatch (1 + k) components, one product kernel
 * MRed(component, ptmul) with the batch in its grid, one inverse NTT into the outputs; ptmul is not transformed again.  Canonical residues. */
int  mkhe_bfv_ct_mul_ptxt(mkhe_ctx* ctx, int nbatch, const mkhe_ct* const* in, const void* dev_ptmul, long pt_stride_words, mkhe_ct* const* out);
/* op 0: out[b]_0 = CRed(in[b]_0 + pt), op 1: CRed(in[b]_0 - pt); pt canonical.  The other components are copied (nothing is done for them where
 * out[b] == in[b]).  One launch for as many items as the component list of the elementwise kernel holds (65 components). */
int  mkhe_bfv_ct_add_ptxt(mkhe_ctx* ctx, int op, int nbatch, const mkhe_ct* const* in, const void* dev_pt, long pt_stride_words, mkhe_ct* const* out);

/* ==== BFV plaintext linear transform: the batched diagonal dot product ================================
 * No reference counterpart; the preconditions and refusals of "BFV plaintext operands" apply.  Let n = N/2.  A message is z[r][j], r in {0, 1},
 * j < n (the two slot rows of the "BFV batch encoder").  rot_k moves slot j + k to slot j in each row (a rotation by galEl 5^k); swap exchanges the
 * rows (the conjugation, galEl 2N - 1).  A Z_T-linear map is two sets of diagonals, int64 [2][n] each, taken mod T, indices mod n:
 *   (M z)[r][j] = sum_k d_k[r][j] z[r][(j + k) mod n] + sum_k e_k[r][j] z[1 - r][(j + k) mod n]      (mod T).
 * swap commutes with rot_k and with slot-wise products, so with e~_k[r] = e_k[1 - r]:  M z = LT_d(z) + swap(LT_e~(z)).  Each part is evaluated as
 * sum_g rot_g(sum_b d'_(g,b) (.) rot_b z) with k = g + b and d'_(g,b) = roll(d_(g+b), g) along the slot axis of each row; both parts share the baby
 * rotations rot_b z, and the row-swapping part costs one conjugation of its sum.  The call below is the middle of that schedule: every inner sum of
 * every part for nbatch encrypted vectors, as one launch set.
 *   out[b * ngiant + g] = sum over the set bits i of masks[g] of in[b * nin + i] * P(g, i),      b < nbatch, g < ngiant
 * component by component as a negacyclic product mod q_l, canonical.  P(g, i) are prepared multiplication plaintexts of nQ * N words each
 * (mkhe_bfv_encode_mul), stored COMPACTLY in (g, i) order with the numbering of mkhe_ct_ptxt_dot: plaintext number (set bits of masks[0 .. g-1]) +
 * (set bits of masks[g] below i) lies at dev_ptmul + number * nQ * N words.  The block is exactly what ONE mkhe_bfv_encode_mul(count = nnz) writes;
 * it is shared by all nbatch items and read where it lies.  1 <= nbatch <= 16, 1 <= nin <= 16, 1 <= ngiant <= 64; every mask is non-zero and has no
 * bit at or above nin; masks is a host array consumed at call time; all handles carry the same ids and nQ limbs; the outputs are distinct and
 * alias no input.  Launch set: the forward NTT of all nbatch * nin * (1 + k) components (64 ciphertexts per launch), ONE product kernel with the
 * item in its grid, the inverse NTT into the outputs; the temporaries are one pooled block.  out[b][g] equals, bit for bit, mkhe_ct_sum over the
 * set bits i of mkhe_bfv_ct_mul_ptxt(in[b][i], P(g, i)): both are the canonical residue of the same integer.  A refused call enqueues nothing and
 * leaves the context usable; it is refused between mkhe_capture_begin and mkhe_capture_end like the other calls of this family.
 * Noise of the whole transform: a baby rotation adds one key-switch error; the product multiplies the noise by at most N * T/2 per diagonal (above);
 * each giant rotation and the conjugation add one key-switch error.  The result decrypts exactly while the total stays below Q / (2T). */
int  mkhe_bfv_ct_ptxt_dot(mkhe_ctx* ctx, int nbatch, int nin, const mkhe_ct* const* in, int ngiant, const uint32_t* masks,
                          const void* dev_ptmul, mkhe_ct* const* out);

/* ==== BFV weighted sums: integer-weighted sums of ciphertexts and additive constants mod T =============
 * No reference counterpart (mkbfv.Evaluator of the reference adds, multiplies and rotates); the MK-BFV twin of mkhe_ct_lincomb, for nout sums of the
 * same nin ciphertexts at once: every inner sum of a baby-step / giant-step polynomial evaluation over Z_T in one launch.  The preconditions and
 * refusals of "BFV plaintext operands" apply: a BFV context that owns every modulus, T within the encoder's preconditions, not between
 * mkhe_capture_begin and mkhe_capture_end, every handle at the maximum level (nQ limbs) with the same ids, the outputs distinct and aliasing no
 * input, dev_consts non-null and 16-byte aligned.  1 <= nin <= 16, 1 <= nout <= 64; the counts are checked before the context is looked at.  Every
 * error message starts with the name of the function; a refused call enqueues nothing and leaves the context usable.
 *   out[g] = sum_b W[g][b] * in[b] + C[g],      g < nout
 * for every component and every limb l < nQ, mod q_l, canonical; C[g] is added to coefficient 0 of component 0 only (the all-c slot vector is the
 * constant polynomial c).  dev_consts = device uint64[nout][nin + 1][nQ] (mkhe_buf_alloc), read when the call executes:
 *   [g][0][l]      the additive constant as a plain canonical residue: for a slot constant c in [0, T) the scale_up of the "BFV batch encoder",
 *                  floor((Q c + floor(T/2)) / T) mod q_l
 *   [g][1 + b][l]  the weight in the engine's 2^64 Montgomery form, reduced: for an integer weight w mod T the lift of "BFV plaintext operands",
 *                  MForm(c mod q_l) with c the centred representative of w in (-T/2, T/2]
 * A weight whose residue is 0 under limb l costs no product for that limb (a wave-uniform branch); the input is loaded once for all outputs anyway.
 * Launch set: ONE kernel, one thread per coefficient of one component; it reads every input limb once and writes every output limb once,
 * 8 N nQ (1 + k) (nin + nout) bytes for k parties.  mkhe_ct_lincomb once per output moves nout * (nin_g + 1) passes of 8 N nQ (1 + k) instead.
 * Bit-exactness: out[g] is the canonical residue of the integer sum.  For nout = 1 it equals, bit for bit, mkhe_ct_lincomb on the same context with
 * every im_k = 0, the constant (C, 0) and nb_rescale = 0 (that call accepts a BFV context), and the chain mkhe_ct_mul_const, mkhe_ct_sum.
 * Noise: with pt(a) = round(Q a / T) and w the centred weight, w * pt(a) = (Q/T) [w a]_T + Q k + eps w with |eps| <= 1/2 -- no Q mod T term -- and
 * the constant adds its own rounding |eps| <= 1/2: a sum of ciphertexts of noise e_b has noise at most sum_b |w_b| (|e_b| + 1/2) + 1/2, and decrypts
 * to sum_b w_b a_b + c mod T slot by slot while that stays below Q / (2T).  No key is used and no party is added. */
int  mkhe_bfv_ct_lincomb(mkhe_ctx* ctx, int nin, const mkhe_ct* const* in, int nout, const void* dev_consts, mkhe_ct* const* out);

/* ---- measurement support (no reference counterpart): HIP-event timing per kernel class on the
 *      context stream, one record per kernel launch.  Classes (mkhe_prof_name gives the kernel symbol
 *      each class corresponds to in a rocprofv3 kernel trace). */
int  mkhe_prof_enable(mkhe_ctx* ctx, int on);
/* on = 0: no side-stream overlap, every kernel runs alone on the main stream (per-kernel timings that can be
 * compared with a rocprofv3 kernel trace); default on = 1 */
int  mkhe_set_overlap(mkhe_ctx* ctx, int on);
/* diagnostic: forward-NTT workgroups write {start, end (100 MHz ticks), HW_ID, XCC_ID} per job into dev_buf
 * (4 words per job of the NEXT launches; NULL switches it off) */
int  mkhe_ntt_trace(mkhe_ctx* ctx, void* dev_buf);
/* N = 2^15, where two forward kernels apply (same bits): by default (MKHE_NTT32=2) the context times a block of launches of each inside the caller's
 * workload and keeps the faster one per launch shape.  The kernel it has settled on for Decompose launches of `limbs` limb-NTTs: 1 = single-pass
 * (ntt32_fwd_kernel), 0 = two-pass (ntt16_fwd_kernel), -1 = still measuring, never launched, or fixed by MKHE_NTT32 = 0 / 1. */
int  mkhe_ntt_choice(mkhe_ctx* ctx, long limbs, int decompose);      /* -2: error (mkhe_last_error) */
/* Pins that choice instead of measuring it, so that a run can be repeated with the kernels of an earlier one (a bench line records
 * config.ntt_kernel_choice): choice 1 = single-pass, 0 = two-pass, -1 = forget and measure again.  limbs > 0: launches of that many limb-NTTs
 * (decompose = 1: Decompose launches, 0: plain forward transforms); limbs <= 0: every shape of the context, met so far or not.  Same bits either way. */
int  mkhe_ctx_set_ntt_choice(mkhe_ctx* ctx, long limbs, int decompose, int choice);
/* mkhe_mul_relin_batch at N = 2^15: inputs whose hoisting is at least `min_limbs` limb-NTTs ((n0 + n1) * beta * (level + 1 + nP); default 1536: four
 * parties at the top level of PN15QP880) are evaluated IN FLIGHT -- the single-operation path on this context and two internal ones, round robin, joined
 * before the call returns to the stream -- instead of in lock step: one such evaluation fills the chip with every big kernel, what a second one can use
 * is the first one's latency-bound stretches.  0: every batch of this ring in flight; < 0: always lock step.  Same results either way
 * (mkrlwe/keyswitch_hoisted.go:44-179 per input).  The internal contexts follow the caller's overlap setting and its pin for every shape
 * (mkhe_ctx_set_ntt_choice with limbs <= 0); pins of single launch shapes are the caller context's own. */
int  mkhe_ctx_set_batch_lanes(mkhe_ctx* ctx, long min_limbs);
/* The stream-ordered buffer pools (freed ciphertext / key handles are kept for reuse, bounded per DEVICE by MKHE_POOL_GB): bytes this context's
 * pool holds, and "hand everything the pools of this context's device hold back to the driver" (one device-wide synchronisation; the engine does
 * this by itself when an allocation fails for lack of memory and retries once). */
long long mkhe_pool_held_bytes(mkhe_ctx* ctx);                          /* -1: error */
int  mkhe_pool_trim(mkhe_ctx* ctx);
/* diagnostic, no device call: the schedule of ntt16_f2_kernel (N = 2^15: step F2 of MulAndRelin, mkrlwe/keyswitch_hoisted.go:161-178, computed inside
 * the Decompose NTT of the t_i) for `parties` parties of op0, `nb` gadget digits, `nslots` limb slots with the relative cost weights[slot] of a pass,
 * on `grid` workgroups (grid < 0: on the cheapest grid of at most -grid workgroups, as the engine plans it for a device of -grid CUs).  segs: |grid| * 3
 * records of 8 bytes {party, slot, half, first digit, digits, part, parts this run zeroes after its own, 0} (digits = 0: no run).  Returns the workgroups
 * used (0: no schedule within the kernel's limits) and the parts per product in *parts. */
int  mkhe_f2_schedule_probe(int parties, int nb, int nslots, const long* weights, int grid, unsigned char* segs, int* parts);
int  mkhe_prof_nclass(void);
const char* mkhe_prof_name(int cls);
int  mkhe_prof_collect(mkhe_ctx* ctx, double* ms, long* launches, double* alg_bytes);

#ifdef __cplusplus
}
#endif
#endif
