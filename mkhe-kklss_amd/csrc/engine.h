// engine.h -- device-resident multi-key RLWE key-switch engine (host-side C++ over HIP).
//
// One Context = one mkrlwe.KeySwitcher (mkrlwe/keyswitch.go:8-47): ring tables for Q and P in
// HBM, the ModDown / rescale constants, and the scratch pools the reference keeps in
// ks.Pool / swkPool1-3 / polyQPool (engine-internal here).  One HIP stream per context; calls
// on a context are serialized by the caller, exactly like the non-reentrant reference.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <atomic>
#include <mutex>
#include <map>
#include <memory>
#include <vector>
#include "device_memory.h"
#include "modarith.h"
#include "ntt_kernels.h"
#include "poly_kernels.h"
#include "keygen_kernels.h"
#include "encdec_kernels.h"
#include "decshare_kernels.h"
#include "refresh_kernels.h"
#include "bfv_refresh_kernels.h"
#include "pcks_kernels.h"
#include "skenc_kernels.h"
#include "threshold_kernels.h"
#include "noise_kernels.h"
#include "modraise_kernels.h"
#include "ckks_kernels.h"
#include "bfv_kernels.h"

namespace mkhe {

// A/B switches that several translation units ask for (csrc/switches.h: constants in the product library): x, y and step E inside the F1 kernel
int ab_fuse_x();
int ab_fuse_y();
int ab_fuse_e();

// host number theory of engine.hip that the encoders share: Miller-Rabin for 64-bit n, and the engine's choice of a primitive 2N-th root
// (g the smallest generator >= 3 of Z_q*, psi = g^((q-1)/2N)); q must be a prime = 1 mod 2N
bool is_prime(u64 n);
u64 default_psi(u64 q, u64 N);

// log2 of the largest tile one workgroup of an encoder's transform takes (tile_transform.h): what the runtime granted at the first call, and the
// limit in force.  set: 0 (back to the grant), the grant itself, or lo .. hi; anything else throws `what` + the closing words on the grant
struct TileLimit {
    int log, granted;
    void set(int log_points, int lo, int hi, const std::string& what);
};

// device SwitchingKey / hoisted digit vector: uint64[betaMax][nQ+nP][N]
struct Swk { u64* d = nullptr; bool owned = true; };
// device ciphertext: uint64[1+n][limbs][N], slot 0 = c_0, slot 1+i = party ids[i]
struct Ct { int n = 0; int limbs = 0; std::vector<int> ids; u64* d = nullptr; };
// one external product of a batch: dst (+)= ModDown_P( sum_i bg[i] (.) ah[i] )
struct ExtItem { const u64* ah; const u64* bg; u64* dst; bool accumulate; const u64* ah2 = nullptr; const u64* bg2 = nullptr;
                 const u64* xkey = nullptr;   /* F1 only: this party's d_i, for the x by-product (ExtInnerArgs::xkey) */
                 bool pre = false;            /* the inner products of this item exist already (step E computed by the F1 kernel): in its c1 slot, or ... */
                 const u64* pre_src = nullptr; /* ... at pre_src [mtot][N] (a batch: the inner kernel copies them into the slot instead of computing) */
                 const u64* xkey2 = nullptr;  /* mkbfv F1: this party's d2_i (second gadget) */
                 const u64* addend = nullptr; /* accumulate onto this polynomial instead of onto dst (Rotate: c_0 of the input) */
                 const u64* qadd = nullptr;   /* first product of a destination, not accumulating: an NTT-domain polynomial [L][N] (canonical, already
                                                 times P) that joins the summed Q parts of the merged batch -- dst = that term + the products */
                 unsigned gal = 0;            /* rotate_multi: this destination's own Galois element (0: the ext_batch call's); same for every product of a destination */
                 const u64* post = nullptr;   /* rotate_multi: polynomial [L][N] added to the finished destination at the STORED (permuted) position --
                                                 ring.Add(post, Rotate(..)) of AddNew(ct, RotateNew(ct, r)), cnn/cnn.go:33-37 -- by the last product of the destination */
                 int f2_party = -1;           /* >= 0: step F2 computed by ntt16_f2_kernel (ntt_kernels.h F2FusedArgs) from the party's t (ExtFuse::f2_src): `ah` is not read */
                 int f2_key = 0;              /* ... 0: the product with v_i, 1: with the CRS u */ };
// what one ext_batch call fuses into its product kernel (Context::ext_front); the default is the plain inner-product launch
struct ExtFuse {
    u64* xout = nullptr;                           // the x by-product of step F1
    u64* xout2 = nullptr;                          // ... and the second gadget's x (mkbfv)
    std::vector<const u64*> ykeys, yh;             // y computed inside the F1 kernel (ExtXyArgs::ykey / yh); with xmap (a batch): yh holds every
                                                   // input's digits in turn, ykeys.size() per input
    std::vector<const u64*> ykeys2, yh2;           // second gadget of ykeys / yh
    int e_slot = -1;                               // >= 0: the F1 kernel computes step E too: first c1 slot of the E products
    std::vector<std::pair<const u64*, u64*>> xmap; // batch.hip: (shared key y_b, x_b) per input of a batch's F1 call: one x per group
    std::vector<u64*> eouts;                       // a batch's F1 call that computes step E too: where input b's E products go ([n1][mtot][N])
    std::vector<const u64*> staged;                // the digit vectors, read by the items, that decompose_batch left staged (stage_only)
    std::vector<const u64*> f2_src;                // N = 2^15: the t_i by party of a batch whose F2 products come out of their Decompose NTT itself
                                                   // (ntt16_f2_kernel); the items carry ExtItem::f2_party
};

typedef unsigned long long seq_t;
// per handle: (uid of a context, that context's call counter at its latest use of the buffer); `exposed` once the raw device
// pointer was handed out (uses can no longer be seen by the C ABI)
struct HandleUsers { std::vector<std::pair<seq_t, seq_t>> v; bool exposed = false; };

class Context {
  public:
    // QMul / T: optional mkbfv extension (mkbfv/params.go:30-76): nqm = nq extra primes and the plaintext modulus
    Context(int logN, const u64* Q, int nq, const u64* P, int np, int gamma,
            const u64* psiQ, const u64* psiP, int device, const u64* QMul = nullptr, int nqm = 0, u64 T = 0);
    ~Context();

    int logN, N, nq, np, mtot, gamma, alpha, beta_max, device;
    int nqm = 0, mall = 0;          // QMul primes (BFV) and the total number of moduli with tables
    u64 bfv_t = 0;
    std::vector<u64> moduli;        // Q then P (then QMul)
    std::vector<u64> psi_plain;     // 2N-th roots actually used
    hipStream_t stream = nullptr;      // main stream: everything the caller observes is ordered on it
    hipStream_t stream2 = nullptr;     // side stream for independent sub-chains (always joined back into `stream`)

    int beta(int level) const { return (level + 1 + alpha - 1) / alpha; }
    size_t swk_words() const { return (size_t)beta_max * mtot * N; }
    size_t poly_words(int limbs) const { return (size_t)limbs * N; }

    // ---- ring-level entry points (tests / bench / callers that hold raw device buffers)
    // NTT of `count` polys of `limbs` limbs each; modulus of limb l is mod_base + l.
    void ntt(const u64* src, u64* dst, int count, int limbs, int mod_base, bool inverse, bool lazy);

    // ---- KeySwitcher method set (mkrlwe/keyswitch.go, keyswitch_hoisted.go)
    void decompose(int level, bool is_ntt, const u64* a /*[level+1.. ][N] device*/, u64* out_swk);
    void external_product_hoisted(int level, const u64* ah, const u64* bg, u64* c, bool accumulate);
    void external_product(int level, bool is_ntt, const u64* a, const u64* bg, u64* c, bool accumulate);
    void mul_and_relin(const Ct& op0, const Ct& op1, const Swk* const* hoist0, const Swk* const* hoist1,
                       const Swk* const* rlk_b1, const Swk* const* rlk_d0, const Swk* const* rlk_v0,
                       const Swk& crs_u, Ct& out);
    void rotate(u64 galEl, const Ct& in, const Swk* const* hoist, const Swk* const* rk, const Swk& crs, Ct& out);
    void conjugate(u64 galEl, const Ct& in, const Swk* const* ck, const Swk& crs, Ct& out);
    void rotate_partial(const Ct& in, const Swk* const* hoist, const Swk* const* rk, const Swk& crs, bool with_c0, Ct& out);
    void rotate_core(const Ct& in, const Swk* const* hoist, const Swk* const* rk, const Swk& crs, bool with_c0, Ct& out, u64 galEl);
    void automorphism(u64 galEl, const Ct& in, Ct& out);
    // ---- mkbfv (mkbfv/basis_extension.go, keyswitch.go, keyswitch_hoisted.go, evaluator.go); PolyR = [2nq][N]
    bool is_bfv() const { return nqm > 0; }
    void bfv_modup_q_to_r(const u64* polyq, u64* polyr, int npolys);          // conv.ModUpQtoR
    void bfv_rescale(const u64* polyq, u64* polyr, int npolys);               // conv.Rescale
    void bfv_quantize(const u64* polyr_ntt, u64* polyq, int npolys);          // conv.Quantize (polyr_ntt is consumed)
    void bfv_decompose_batch(const std::vector<const u64*>& srcr, const std::vector<u64*>& ad1, const std::vector<u64*>& ad2, bool internal = false);
    void bfv_external_product_hoisted(const u64* ah1, const u64* ah2, const u64* bg1, const u64* bg2, u64* c);
    void bfv_external_product(const u64* polyr, const u64* bg1, const u64* bg2, u64* c);
    void bfv_mr_partial(const Ct& op0, const Ct& op1, const Swk* const* rlk_b1, const Swk* const* rlk_b2,
                        const Swk* const* rlk_d1, const Swk* const* rlk_d2, bool with_c0, bool mform, Ct& out,
                        u64* x1, u64* x2, u64* y1, u64* y2, bool fuse_x = false, bool fuse_y = false);
    void bfv_mr_finish(const Ct& op0, const Ct& op1, const u64* x1, const u64* x2, const u64* y1, const u64* y2,
                       const Swk* const* rlk_v, const Swk& crs_u, Ct& out);
    void mul_relin_rescale(const Ct& op0, const Ct& op1, const Swk* const* hoist0, const Swk* const* hoist1, const Swk* const* rlk_b1,
                           const Swk* const* rlk_d0, const Swk* const* rlk_v0, const Swk& crs_u, Ct& out);
    void bfv_mul_relin_unhoisted(const Ct& op0, const Ct& op1, const Swk* const* rlk_b1, const Swk* const* rlk_b2,
                                 const Swk* const* rlk_d1, const Swk* const* rlk_d2, const Swk* const* rlk_v, const Swk& crs_u, Ct& out);
    void bfv_mul_relin(const Ct& op0, const Ct& op1, const Swk* const* rlk_b1, const Swk* const* rlk_b2,
                       const Swk* const* rlk_d1, const Swk* const* rlk_d2, const Swk* const* rlk_v,
                       const Swk& crs_u, Ct& out);                            // Evaluator.MulRelinNew
    // out = sum_k op0[k] * op1[k] under ONE Quantize and ONE relinearisation tail (engine_bfv_sum.hip; no reference counterpart): per pair the
    // conversions, the transforms over R, x, y, t_i += ExtB(h(c0_i), y) and e_j += ExtB(h(c1_j), x); then one tensor_sum_kernel over R, one Quantize,
    // out_j += e_j and step F2 on the summed t_i.  1 <= K <= TSUM_MAX_K; BFV contexts that own every modulus
    void bfv_mul_relin_sum(const std::vector<const Ct*>& op0, const std::vector<const Ct*>& op1, const Swk* const* rlk_b1, const Swk* const* rlk_b2,
                           const Swk* const* rlk_d1, const Swk* const* rlk_d2, const Swk* const* rlk_v, const Swk& crs_u, Ct& out);
    // elementwise evaluator ops (mkckks/evaluator.go:41-300, mkbfv/evaluator.go:27-76): op 0 add, 1 sub
    void ct_binary(int op, const Ct& a, const Ct& b, Ct& out);
    // mkckks MultByConst body (evaluator.go:150-196) and MulPtxtNew body without its Rescale (:471-478)
    void ct_mul_const(const Ct& in, const u64* c_first, const u64* c_second, Ct& out);
    void ct_mul_ptxt(const Ct& in, const u64* dev_pt, Ct& out);
    void ntt_r(const u64* src, u64* dst, int count, bool inverse);            // ringR.NTT / InvNTT
    // mkckks Rescale body: nb successive DivRoundByLastModulus on every poly (evaluator.go:385-391)
    void rescale(const Ct& in, int nb, Ct& out);
    // MulAndRelin split in phases (party-sharded multi-GPU evaluation: the x / y partial sums and out_0
    // are reduced across devices between the phases)
    void mr_prepare(const Ct& op0, const Ct& op1, const Swk* const* hoist0, const Swk* const* hoist1, bool with_c0, Ct& out);
    // defer_x: x is accumulated on the side stream and joined by mr_finish just before its first use (step E), so that it
    // overlaps the latency-bound part of step F; false (split-phase ABI): x and y are both complete on the main stream
    // fuse_x: x is not computed here but by the F1 kernel of mr_finish_head (one pass over h(c0_i) less); needs 1 <= n0 <= 4
    // fuse_y (with fuse_x, n1 == n0 <= 4): y is not computed here either but inside the same F1 kernel, from the b_j and h(c1_j), and never stored
    void mr_xy(const Swk* const* rlk_b1, const Swk* const* rlk_d0, u64* x, u64* y, bool mform, bool defer_x = false, bool fuse_x = false, bool fuse_y = false);
    void mr_finish_head(const Ct& op0, const Ct& op1, const u64* y, Ct& out);          // F1 + Decompose(t_i): needs y only
    void mr_finish_tail(const Ct& op0, const Ct& op1, const u64* x, const Swk* const* rlk_v0, const Swk& crs_u, Ct& out);
    void mr_finish(const Ct& op0, const Ct& op1, const u64* x, const u64* y, const Swk* const* rlk_v0,
                   const Swk& crs_u, Ct& out);
    void mr_f2_hoist(bool e_free);     // F2: h(t_i) of plan_.f2_tbuf for the tail batch; e_free: that batch computes no step-E product itself
    // out = [Rescale] sum_k op0[k] * op1[k] under ONE relinearisation tail (engine_mulrelin_sum.hip; no reference counterpart): per pair the tensor
    // terms (one launch for all pairs), x^k, y^k, step E into out and t_i += <h(c0_i^k), y^k>_P; then step F2 once on the summed t_i.  Hoisted forms
    // flat [k * n + a] or empty (the engine hoists that side); 1 <= K <= TSUM_MAX_K; CKKS contexts that own every modulus
    void mul_relin_sum(const std::vector<const Ct*>& op0, const std::vector<const Ct*>& op1, const std::vector<const Swk*>& hoist0,
                       const std::vector<const Swk*>& hoist1, const Swk* const* rlk_b1, const Swk* const* rlk_d0, const Swk* const* rlk_v0,
                       const Swk& crs_u, bool rescale_out, Ct& out);
    void fold(u64* buf, bool qp_shaped, int level, int npolys, long poly_stride, bool mform);
    // the reduce-scatter half of a mesh exchange of x / y (dist.py): limbs [first_limb, first_limb + nlimbs) of a switching-key buffer, summed over
    // npieces pieces, folded and MForm'ed into dst (limb i of the range at dst + i * N)
    void fold_pieces(const u64* pieces, int npieces, long piece_stride, long first_limb, long nlimbs, int level, bool mform, u64* dst);
    // ---- B independent operations of one shape as one launch set (batch.hip; small rings: DESIGN.md section 8).  Flat lists: hoisted forms are
    // [b * n + a] (input b, party component a) or empty (the engine hoists); keys are per party, shared by the inputs.
    void hoisted_form_batch(int level, const std::vector<const Ct*>& cts, const std::vector<Swk*>& outs);
    void rotate_batch(u64 galEl, const std::vector<const Ct*>& ins, const std::vector<const Swk*>& hoists, const Swk* const* rk, const Swk& crs,
                      const std::vector<Ct*>& outs);
    void mul_relin_batch(const std::vector<const Ct*>& op0, const std::vector<const Ct*>& op1, const std::vector<const Swk*>& hoist0,
                         const std::vector<const Swk*>& hoist1, const Swk* const* rlk_b1, const Swk* const* rlk_d0, const Swk* const* rlk_v0,
                         const Swk& crs_u, bool rescale_out, const std::vector<Ct*>& outs);
    // B rotations in one launch set, each with its own Galois element and keys (rk flat [b * n + a], crs per input), optionally
    // out[b] = post_add[b] + Rotate(in[b]) (batch.hip; nbatch = 1: the fused rotate-and-add of one ciphertext)
    void rotate_multi(const std::vector<u64>& galEl, const std::vector<const Ct*>& ins, const std::vector<const Swk*>& hoists, const std::vector<const Swk*>& rk,
                      const std::vector<const Swk*>& crs, const std::vector<const Ct*>& post_add, const std::vector<Ct*>& outs);
    // out = ins[0] + ... + ins[n-1] (one shape; out at its own level <= theirs): the AddNew chain over the lanes' products as one launch
    void ct_sum(const std::vector<const Ct*>& ins, Ct& out);
    // out = sum_k (re_k + i im_k) ins[k] + (add_re + i add_im), i = X^(N/2), then nb_rescale (0 or 1) divisions by the last modulus, as one launch
    // (no reference counterpart).  dev_consts: device uint64[n + 1][2][Lc], Lc = out.limbs + nb_rescale (poly_kernels.h, CtLincombArgs)
    void ct_lincomb(const std::vector<const Ct*>& ins, const u64* dev_consts, int nb_rescale, Ct& out);
    // outs[g] = sum_b W[g][b] ins[b] + C[g] for 1 .. 64 outputs from 1 .. 16 inputs as one launch, every handle with the same ids and nQ limbs (no
    // reference counterpart).  dev_consts: device uint64[nout][nin + 1][nQ] (poly_kernels.h, BfvLincombArgs); refusals under `what`, before the launch
    void bfv_ct_lincomb(const char* what, const std::vector<const Ct*>& ins, const u64* dev_consts, const std::vector<Ct*>& outs);
    // outs[g] = sum_b (re[g][b] + i im[g][b]) ins[b] + (add_re[g] + i add_im[g]), then nb_rescale (0 or 1) divisions by the last modulus, for 1 .. 16
    // outputs of one shape from 1 .. 16 inputs as one launch: row g is ct_lincomb's sum, bit for bit (no reference counterpart).  dev_consts: device
    // uint64[nout][nin + 1][2][Lc], Lc = limbs(outs) + nb_rescale (poly_kernels.h, CtLincombMultiArgs); refusals under `what`, before the launch
    void ct_lincomb_multi(const char* what, const std::vector<const Ct*>& ins, const u64* dev_consts, int nb_rescale, const std::vector<Ct*>& outs);
    // ct_lincomb_multi on nbatch = ins.size() / nin items in lock step that share dev_consts: item i sums ins[i * nin ..] into outs[i * nout ..], bit for bit
    // what ct_lincomb_multi gives on them.  Input k has one limb count in all items; the same Ct may be an input of several items; no output overlaps
    // an input of any item or another output.  Base addresses in the kernel arguments (no upload, no allocation), as many launches as they need
    void ct_lincomb_batch(const char* what, const std::vector<const Ct*>& ins, int nin, const u64* dev_consts, int nb_rescale, const std::vector<Ct*>& outs,
                          int nout);
    // plaintext linear transform (no reference counterpart; batch.hip): ptntt = MForm(NTT(pt)) for count plaintexts [limbs][N] (ptntt may be pt), and
    // the dot of both schemes for nbatch items that share masks and plaintexts: outs[b][g] = sum over the set bits i of masks[g] of ins[b][i] * P(g, i),
    // ins = [nbatch][nin] with at least L limbs, outs = [nbatch][masks.size()] with L limbs, pt = the compact block of prepared plaintexts in (g, i)
    // order, pt_words apart.  Every refusal is under `what` (the C entry point) and comes before the first launch
    void ptxt_prepare(int limbs, int count, const u64* pt, u64* ptntt);
    void ct_ptxt_dot(const char* what, int nbatch, const std::vector<const Ct*>& ins, const std::vector<unsigned int>& masks, const u64* pt, long pt_words,
                     int L, const std::vector<Ct*>& outs);
    void ct_binary_batch(int op, const std::vector<const Ct*>& a, const std::vector<const Ct*>& b, const std::vector<Ct*>& outs);
    // MulPtxtNew body (ct_mul_ptxt) for the batch, followed by nb >= 0 divisions by the last modulus (outs have limbs(in) - nb limbs)
    void ct_mul_ptxt_batch(const std::vector<const Ct*>& ins, const u64* dev_pt, int nb, const std::vector<Ct*>& outs);
    u64* pool_x() { return x_; }
    u64* pool_y() { return y_; }
    // batched building blocks (all parties in one launch)
    // internal = true: the digits stay inside the engine (hoist pools): their forward NTT skips the final
    // normalisation (values < 34q with the same residues; every consumer is a Montgomery product)
    // stage_only (alpha = 1, N = 2^14, engine-internal): digit spread + the three cross stages only -- the digits are then consumed by ext_batch through
    // ext_fused_lds_kernel (ExtFuse::staged names them), which finishes the transform in LDS and multiplies in the same kernel (ntt_kernels.h, ExtFusedArgs)
    void decompose_batch(int level, const std::vector<const u64*>& src, const std::vector<u64*>& dst, bool internal = false, bool stage_only = false);
    // the staged list transform: polynomials [L][N] number 0 .. npolys - 1 of src[i] (src_poly words apart) -> the same of dst[i] (dst_poly words apart),
    // NTT_MAX_ITEMS items per launch, forward or inverse, under the first L moduli of Q
    void ntt_items(bool inverse, const std::vector<const u64*>& src, long src_poly, const std::vector<u64*>& dst, long dst_poly, int npolys, int L);
    // out [nouter][mtot][N] = [MForm] sum_a keys[a] (.) digits[a] over the active moduli of `level`: the x / y sums of MulAndRelin, on the active stream
    void key_inner_product(const u64* const* keys, const u64* const* digits, int n, u64* out, int level, int nouter, bool mform);
    bool ext_fused_ok(int level, int nvec) const;
    // stage 0: whole external products; 1: front half only (inner products + inverse NTT into the c1 pool);
    // 2: back half only (ModDown of the c1 pool filled by the preceding stage-1 call with the same items)
    void ext_batch(int level, const std::vector<ExtItem>& items, int join_before_moddown = -1, int stage = 0, u64 galEl = 0, const ExtFuse& fuse = {});
    std::vector<const u64*> staged_open_; // digit vectors left after the cross stages that no product kernel has finished yet: an ext_batch that reads one of them as a
                                          // full transform is an engine bug and throws (round 5: mkhe_rotate_batch did, for one afternoon, on launches only a fuzz run reached)
    struct F2Sched { F2Seg* d_segs = nullptr; int nwg = 0, parts = 1; };
    std::map<long, F2Sched> f2_sched_;                   // by (parties, level): the runs of every workgroup, in device memory
    const F2Sched& f2_schedule(int nparties, int level);
    bool f2_fused_ok(int level, int n0, int n1);         // (fills the f2_sched_ entry of the shape)
    // External products that ModDown adds into ONE destination are merged (ModDown is linear in the Q part, see NttBatch::vi and
    // ModDownMergedArgs): virtual item v = up to VI_MAX items of the batch with the same destination; their Q limbs are summed in the
    // NTT domain at the load of ONE inverse NTT, their P limbs are transformed and lifted one by one.  MKHE_EXT_MERGE=0 switches it off.
    struct ExtMerge {
        int nvi = 0, members_max = 0;
        unsigned char cnt[64] = {}, mem[64][4] = {}, accumulate[64] = {};
        u64* dst[64] = {};
        const u64* addend[64] = {};
        const u64* qadd[64] = {};
        unsigned gal[64] = {};
        const u64* post[64] = {};
    };
    int ext_merge_members(int level) const;      // members a virtual item may have at this level (< 2: no merging)
    bool ext_plan_merge(int level, const ExtItem* items, int n, ExtMerge& mp) const;
    void ext_front(int level, const ExtItem* items, int n, u64* c1, const ExtMerge* mp, const ExtFuse& fuse);   // inner products + lazy inverse NTT into c1 [n][mtot][N]
    // the product kernels of ext_front's fused forms
    bool ext_front_f2(int level, const ExtItem* items, int n, u64* c1, ExtInnerArgs& ia, const ExtFuse& fuse, unsigned short* f2_parts);
    bool ext_front_staged(int level, const ExtItem* items, int n, u64* c1, const ExtFuse& fuse);
    void ext_front_xy(int level, const ExtItem* items, int n, u64* c1, const ExtFuse& fuse);
    void ext_front_xy_batch(int level, const ExtItem* items, int n, u64* c1, const ExtFuse& fuse);
    void ext_back(int level, const ExtItem* items, int n, const u64* c1, u64 galEl = 0, const ExtMerge* mp = nullptr);   // ModDown of c1 into / onto the destinations [signed-permuted]

    // ---- limb-sharded multi-GPU evaluation (mkhe_kklss_amd/dist.py LimbShardedMulRelin): this context owns a subset of
    // the RNS moduli ("slots"); NTTs, inner products and ModDown outputs are computed for the owned slots only, all
    // parties.  The per-party sums x, y are then LOCAL; what crosses the links are the P limbs of the external
    // products, t_i and the output ciphertext (about 40 MB per step instead of 130 MB for party sharding).
    void set_owned(const int* mod_idx, int n);          // n == 0: everything (single-device behaviour)
    bool masked() const { return masked_; }
    // MulAndRelin in four phases around three exchanges through `stage` (device, caller-owned); each returns the number
    // of words of `stage` to all-reduce (sum of disjoint slices) before the next phase.  After phase 4 `out` holds the
    // owned limbs (zeros elsewhere) and is all-reduced itself.
    size_t lsh_phase(int phase, const Ct& op0, const Ct& op1, const Swk* const* rlk_b1, const Swk* const* rlk_d0,
                     const Swk* const* rlk_v0, const Swk* crs_u, Ct& out, u64* stage);

    // ---- key generation and CRS expansion (mkrlwe/keygen.go, mkbfv/keygen.go, params.go:16-99).
    // Secrets and errors are SAMPLES supplied by the caller (host int32, N per polynomial: what lattigo's ternary /
    // Gaussian samplers draw); secret keys are device PolyQP buffers [nq+np][N] (NTT, Montgomery form).
    void keygen_secret(const int32_t* s, u64* dev_sk);                                         // keygen.go:44-55
    void keygen_switching_key(const u64* sk, const int32_t* e, u64* out);                      // keygen.go:270-327
    void keygen_public_key(const u64* sk, const int32_t* e, const u64* crs_a, u64* dev_pk);    // keygen.go:88-109
    void keygen_relin_key(const u64* sk, const u64* r, const int32_t* e, const u64* crs_a, const u64* crs_u,
                          u64* b, u64* d, u64* v);                                             // keygen.go:137-187
    void keygen_rotation_key(u64 galEl, const u64* sk, const int32_t* e, const u64* crs, u64* out);   // keygen.go:190-229
    void keygen_conjugation_key(const u64* sk, const int32_t* e, const u64* crs, u64* out);    // keygen.go:240-268
    // mkbfv/keygen.go:91-162 (one gadget) and :24-88; g1 / g2: host residues [beta][nq+np] of the big-integer scalars Gi
    void bfv_keygen_switching_key(const u64* sk, const u64* g, const int32_t* e, u64* out);
    void bfv_keygen_relin_key(const u64* sk, const u64* r, const u64* g1, const u64* g2, const int32_t* e,
                              const u64* crs_a1, const u64* crs_a2, const u64* crs_u, u64* b1, u64* b2, u64* d1, u64* d2, u64* v);
    void crs_expand(u64 seed, int32_t idx, u64* out);                                          // params.go:47-59,91-98

    // ---- public-key encryption and decryption (encdec.hip; mkrlwe/encryptor.go:55-118, decryptor.go:26-66), ring Q at `level`.
    // samples: host int32 [count][3][N] (u, e0, e1); pk: device [2][nq+np][N]; pt: device [count][level+1][N]; outs[b]: [2][level+1][N]
    void encrypt(int level, int count, const u64* pk, const u64* pt, bool pt_is_ntt, const int32_t* samples, u64* const* outs);
    // the same with samples[b][j] = stream 3 b + j of the ChaCha20 keystream (key, nonce), drawn on the device (encdec_kernels.h small_sample_kernel;
    // include/mkhe.h "device-side sampling"); cdt: host, ncdt thresholds.  No host synchronisation for count <= ED_INLINE.
    void encrypt_seeded(int level, int count, const u64* pk, const u64* pt, bool pt_is_ntt, const u32* key, u64 nonce, const u64* cdt, int ncdt,
                        u64* const* outs);
    // dev_out int32 [count][N] <- streams first_stream .. first_stream + count - 1 of (key, nonce), all of one kind
    void sample_small(int kind, int count, const u32* key, u64 nonce, u32 first_stream, const u64* cdt, int ncdt, int32_t* dev_out);
    void partial_decrypt(const Ct& in, int slot, const u64* sk, Ct& out);                      // decryptor.go:26-43
    void decrypt(const Ct& ct, const u64* const* sks, u64* pt_out);                            // decryptor.go:48-66
    // distributed decryption (include/mkhe.h): shares [count][limbs][N] <- NTT^-1(NTT(ins[b] polynomial slots[b]) * sk) + e_b, e_b = kind 2 of the
    // keystream (bits wide; 0: none, key unread) on stream b of (key, nonce).  The caller (capi.hip) has checked slots, levels and the capture.
    void decrypt_share(const std::vector<const Ct*>& ins, const int* slots, const u64* sk, const u32* key, u64 nonce, int bits, u64* shares);
    // pt [count][limbs][N] <- ins[b] polynomial 0 + sum_i shares[i][b], canonical; ins are over the same ids (shares.size() of them) at one level
    void decrypt_merge(const std::vector<const Ct*>& ins, const std::vector<const u64*>& shares, u64* pt);
    // collective refresh (include/mkhe.h; refresh_kernels.h): shares [count][Lin][N] <- the product of decrypt_share + M_b, M_b = kind 3 of the
    // keystream (bits wide; 0: none, key unread) on the streams 2 b, 2 b + 1 of (key, nonce_mask); outs[b] [2][lout][N] <- encrypt_seeded of the
    // plaintext -M_b at level lout - 1 under (key, nonce_enc).  The caller (capi.hip) has checked slots, levels, shapes and the capture.
    void refresh_share(const std::vector<const Ct*>& ins, const int* slots, const u64* sk, const u64* pk, const u32* key, u64 nonce_mask, u64 nonce_enc,
                       int bits, const u64* cdt, int ncdt, u64* shares, int lout, u64* const* outs);
    // outs[b] [1 + k][lout][N] <- the exact centred lift of ins[b] polynomial 0 + sum_i shares[i][b] from Q_l to the first lout moduli, plus
    // polynomial 0 of reenc[i * count + b]; polynomial 1 + i = polynomial 1 of reenc[i * count + b].  Builds its tables at the first use.
    void refresh_merge(const std::vector<const Ct*>& ins, const std::vector<const u64*>& shares, const std::vector<const u64*>& reenc, int lout,
                       u64* const* outs);
    // encryption to shares (include/mkhe.h): the share of refresh_share, bit for bit, and its plaintext -M_b under the first secret_limbs moduli into
    // the caller's secret [count][secret_limbs][N] instead of an encryption; the merge of refresh_merge without re-encryptions, R~ into pt
    // [count][lout][N].  The caller (capi.hip) has checked slots, levels, limbs and the capture.
    void e2s_share(const std::vector<const Ct*>& ins, const int* slots, const u64* sk, const u32* key, u64 nonce_mask, int bits, u64* shares,
                   int secret_limbs, u64* secret);
    void e2s_merge(const std::vector<const Ct*>& ins, const std::vector<const u64*>& shares, int lout, u64* pt);
    // the same for MK-BFV: the share of bfv_refresh_share with mask = 1, bit for bit, and secret [count][N] <- (T - A_b) mod T over Z_T
    void bfv_e2s_share(const std::vector<const Ct*>& ins, const int* slots, const u64* sk, const u32* key, u64 nonce_mask, int flood_bits, u64* shares,
                       u64* secret);
    // collective refresh for MK-BFV (include/mkhe.h; bfv_refresh_kernels.h), every ciphertext with nq limbs: shares [count][nq][N] <- the product of
    // decrypt_share + up(A_b) + e_b, A_b = kind 4 (mask = 0: none) and e_b = kind 5 (flood_bits wide; 0: none) of the keystream on the streams
    // b S .. b S + S - 1 of (key, nonce_mask), S = 2 + ceil(flood_bits / 64); outs[b] [2][nq][N] <- encrypt_seeded of the plaintext up(-A_b) at the
    // maximum level under (key, nonce_enc).  The caller (capi.hip) has checked slots, shapes, flood_bits and the capture.
    void bfv_refresh_share(const std::vector<const Ct*>& ins, const int* slots, const u64* sk, const u64* pk, const u32* key, u64 nonce_mask, u64 nonce_enc,
                           int mask, int flood_bits, const u64* cdt, int ncdt, u64* shares, u64* const* outs);
    // outs[b] [1 + k][nq][N] <- polynomial 0 = up(down(ins[b] polynomial 0 + sum_i shares[i][b])) + polynomial 0 of reenc[i * count + b];
    // polynomial 1 + i = polynomial 1 of reenc[i * count + b]
    void bfv_refresh_merge(const std::vector<const Ct*>& ins, const std::vector<const u64*>& shares, const std::vector<const u64*>& reenc, u64* const* outs);
    // the tables of the BFV encoder, which both calls (and mkhe_bfv_ct_ptxt_dot) read, built here if no encoder call has built them (what = the C
    // entry point: T outside the encoder's preconditions is refused under its name), and the widest flood a share takes: bitlen(Q div 2 T) - 1
    void bfv_prepare(const char* what) { bf_init(what); }
    int bfv_refresh_max_flood() const { return flood_room(nq, bfv_t); }
    // bitlen((q_0 .. q_(limbs-1)) div 2 t) - 1: the widest flood that alone leaves a message scaled by Q / t standing (t = 1: a CKKS / mkrlwe ring)
    int flood_room(int limbs, u64 t) const;
    // collective key switch to a recipient's public key (include/mkhe.h; pcks_kernels.h): shares [count][2][L][N] <- (h0_b, h1_b), h0 = the product
    // of decrypt_share + u_b * pk0 + E_b, h1 = u_b * pk1 + e1_b, with u_b = kind 0 on stream b, e1_b = kind 1 on stream count + b and E_b = kind 5
    // (flood_bits wide; 0: none) on the streams 2 count + b W .. of (key, nonce), W = ceil(flood_bits / 64); pk: the recipient's [2][nq+np][N].  One
    // launch set, no host synchronisation whatever count is.  The caller (capi.hip) has checked slots, levels, flood_bits and the capture.
    void pcks_share(const std::vector<const Ct*>& ins, const int* slots, const u64* sk, const u64* pk, const u32* key, u64 nonce, int flood_bits,
                    const u64* cdt, int ncdt, u64* shares);
    // outs[b] [2][L][N] <- (ins[b] polynomial 0 + sum_i shares[i][b][0], sum_i shares[i][b][1]), canonical
    void pcks_merge(const std::vector<const Ct*>& ins, const std::vector<const u64*>& shares, u64* const* outs);
    // noise measurement (include/mkhe.h; noise_kernels.h): out [count][limbs + 1] <- the mixed-radix digits of max_n min(x, Q - x) and the smallest n
    // that attains it, x = phase - ref (kind 0; ref null: phase; ref_stride 0: one reference for all) or T phase (kind 1: BFV context, limbs = nq)
    // mod Q = q_0 .. q_(limbs-1).  Two launches; the digits and the candidates, which are the noise itself, are wiped behind them.  The caller
    // (capi.hip) has checked kind, shapes and the capture, and has had noise_norm_prepare build the tables the kernels read.
    void noise_norm_prepare(int kind) { if (kind == 1) bf_init("mkhe_noise_norm"); garner_table(); }
    void noise_norm(int kind, int limbs, int count, const u64* phase, const u64* ref, long ref_stride, u64* out);
    // secret-key encryption with a seeded c1 (include/mkhe.h; skenc_kernels.h): polynomial 1 of outs[b] [2][level+1][N] <- the rows (b, j) of kind 6
    // of the keystream under the PUBLIC (a_key, a_nonce), polynomial 0 <- pt + e_b - c1 * sk.  e != null: host int32 [count][N] (e_key, cdt unread);
    // e == null: e_b = kind 1 on stream b of the SECRET (e_key, e_nonce), formed in registers.  what = the C entry point (for messages).  No host
    // synchronisation for count <= ED_INLINE and e == null.  The caller (capi.hip) has checked shapes, keys and the capture.
    void encrypt_sk(int level, int count, const u64* sk, const u64* pt, bool pt_is_ntt, const u32* a_key, u64 a_nonce, const int32_t* e,
                    const u32* e_key, u64 e_nonce, const u64* cdt, int ncdt, u64* const* outs, const char* what);
    // dev_out [count][limbs][N] <- the rows (b, j), j < limbs, of kind 6 under (key, nonce)
    void sample_uniform(int limbs, int count, const u32* key, u64 nonce, u64* dev_out);
    // polynomial 1 of outs[b] [2][limbs][N] <- the rows (b, j), j < limbs; polynomial 0 is not touched
    void ct_expand_seeded(int count, int limbs, const u32* key, u64 nonce, u64* const* outs);
    // threshold secret keys (include/mkhe.h; threshold_kernels.h).  outs[p] [mtot][N] <- the Shamir share of sk [mtot][N] at points[p], p < n, the
    // coefficient polynomials c_1 .. c_(t-1) = kind 7 under the SECRET (key, nonce): one launch, nothing staged, the c_k in registers only.
    void threshold_gen_shares(const u64* sk, int t, int n, const u32* points, const u32* key, u64 nonce, u64* const* outs);
    // out [mtot][N] <- share * lambda_j, lambda_j = prod_{a != point} x_a (x_a - point)^-1 mod m_j over the active points (host_modarith.h), which
    // travel as MForm values in the kernel arguments: one streaming launch, nothing staged.  out may be share.
    void threshold_additive_key(const u64* share, u32 point, int nactive, const u32* active, u64* out);
    // dst [count][limbs][N] <- the sum of the sources mod mods[j], canonical; more than ED_INLINE sources stage their table, which synchronises
    void limbs_sum(int count, int limbs, const std::vector<const u64*>& src, u64* dst);
    // raising the modulus (include/mkhe.h; modraise_kernels.h): out [1 + k][out.limbs][N] <- the centred representatives of the level-0 ciphertext
    // in [1 + k][1][N] under the first out.limbs moduli.  One launch, no table, no scratch.  The caller (capi.hip) has checked levels, ids and aliasing.
    void mod_raise(const Ct& in, Ct& out);

    // ---- CKKS encoder (ckks_encode.hip, ckks_kernels.h): full packing, n = N/2 slots.  Device buffers: slots double[count][n][2] (re, im),
    // coeffs double[count][N], pt uint64[count][limbs][N] (coefficient domain, canonical).  encode = scale_up(embed), decode = project(scale_down).
    void ckks_embed(int count, const double* slots, double* coeffs);
    void ckks_project(int count, const double* coeffs, double* slots);
    void ckks_scale_up(int level, int count, const double* coeffs, double scale, u64* pt);
    void ckks_scale_down(int limbs, int count, const u64* pt, double scale, double* coeffs);
    void ckks_encode(int level, int count, const double* slots, double scale, u64* pt);
    void ckks_decode(int limbs, int count, const u64* pt, double scale, double* slots);
    // sparse packing, n = 2^log_slots slots (0 .. logN - 1; logN - 1 is the calls above): slots double[count][n][2]; coeffs and pt as above, with the
    // message on the grid of stride N / 2n and zero off it (ckks_kernels.h)
    void ckks_embed_sparse(int log_slots, int count, const double* slots, double* coeffs);
    void ckks_project_sparse(int log_slots, int count, const double* coeffs, double* slots);
    void ckks_encode_sparse(int level, int log_slots, int count, const double* slots, double scale, u64* pt);
    void ckks_decode_sparse(int limbs, int log_slots, int count, const u64* pt, double scale, double* slots);
    // log2 of the largest transform one workgroup does in LDS (CK_TILE_LOG_BIG, or CK_TILE_LOG when the runtime grants no more LDS), and a way
    // to lower it to CK_TILE_LOG so that the two-launch form of n = 2^12, 2^13 can be run where the runtime does grant it (0: back to the grant)
    int ckks_tile();
    void ckks_set_tile(int log_points);

    // ---- BFV batch encoder (bfv_encode.hip, bfv_kernels.h): N slots over Z_T.  Device buffers: slots int64[count][N], coeffs uint64[count][N] (< T),
    // pt uint64[count][nq][N] (coefficient domain, canonical).  encode = scale_up(slots_to_coeffs), decode = coeffs_to_slots(scale_down).
    void bfv_slots_to_coeffs(int count, const u64* slots, u64* coeffs);
    void bfv_coeffs_to_slots(int count, const u64* coeffs, u64* slots);
    void bfv_scale_up(int count, const u64* coeffs, u64* pt);
    void bfv_scale_down(int count, const u64* pt, u64* coeffs);
    void bfv_encode(int count, const u64* slots, u64* pt);
    void bfv_decode(int count, const u64* pt, u64* slots);
    // plaintext operands: ptmul = uint64[count][nQ][N], Montgomery form (bfv_kernels.h); bfv_lift leaves the coefficient domain, bfv_encode_mul the
    // NTT domain (the prepared plaintext of bfv_ct_mul_ptxt)
    void bfv_lift(int count, const u64* coeffs, u64* ptmul_coeff);
    void bfv_encode_mul(int count, const u64* slots, u64* ptmul);
    // MulPtxt / AddPtxt / SubPtxt on B ciphertexts of one shape at the maximum level (batch.hip); pt_stride = words between the plaintexts of
    // consecutive items, 0 = one plaintext for all.  what = the C entry point, for the messages.
    void bfv_ct_mul_ptxt(const char* what, const std::vector<const Ct*>& ins, const u64* ptmul, long pt_stride, const std::vector<Ct*>& outs);
    void bfv_ct_add_ptxt(const char* what, int op, const std::vector<const Ct*>& ins, const u64* pt, long pt_stride, const std::vector<Ct*>& outs);
    // slot map (bfv_kernels.h): dev_map uint64[N] <- the map out_slot[i] = mult[i] * in_slot[index[i]] by position (index uint32[N], mult uint64[N] or
    // null = ones; downloads, validates on the host, uploads: synchronous); coeffs_out = slots_to_coeffs(map(coeffs_to_slots(coeffs_in))), one launch
    // when one workgroup holds the polynomial, else five around bf_work_ (two buffers of 32-bit words, wiped behind the call).  out may be in.
    void bfv_slot_map_prepare(const u32* dev_index, const u64* dev_mult, u64* dev_map);
    void bfv_slot_map(int count, const u64* coeffs_in, const u64* dev_map, u64* coeffs_out);
    // log2 of the largest transform one workgroup does in LDS (BF_TILE_LOG_BIG, or BF_TILE_LOG_DEF when the runtime grants no more LDS), and a way
    // to lower it (BF_TILE_LOG_MIN .. the grant; 0: back to the grant) so that the two-launch form can be run at small N
    int bfv_tile();
    void bfv_set_tile(int log_points);
    u64 bfv_slot_psi();

    bool overlap = true;               // false: everything on the main stream (clean per-kernel timings)
    u64* ntt_trace = nullptr;          // diagnostic buffer handed to the forward NTT kernels (mkhe_ntt_trace)
    // stream-ordered buffer cache for ciphertext / switching-key handles: freeing a handle does not
    // synchronise or hipFree, the words go back to a size-keyed free list and are reused by the next
    // create (all work of a context is ordered on its main stream, so reuse is safe).
    u64* pool_alloc(size_t words);
    size_t pool_take_all(std::vector<u64*>& out);      // empties the free list into `out` (the caller synchronises the device, then frees); words taken
    size_t pool_held_words();                          // what this context's free list holds
    size_t pool_trim_device();                         // every context's free list of this device back to the driver; words released
    void pool_free(u64* p, size_t words, const HandleUsers* users = nullptr);   // users == nullptr / exposed: every live context counts
    void sync() { const unsigned long long s0 = seq_.load(); MKHE_HIP(hipStreamSynchronize(stream)); if (completed_.load() < s0) completed_.store(s0); }
    // cross-context ordering on one device: everything enqueued on this context from now on starts after everything
    // enqueued on `other` so far has finished (event on other's stream; no host synchronisation).  Contexts over the same
    // ring share keys / CRS / ciphertext handles freely (handles are plain device memory): independent operations issued
    // through different contexts overlap on the GPU.
    void wait_for(Context& other);

    // ---- per-kernel-class timing with HIP events on the context stream (bench.py roofline leg)
    // (the classes of the NTT launches lead the list: PROF_NTT_DECOMP = 0 .. PROF_NTT_INV, ntt_route.h)
    enum { PROF_INNER = PROF_NTT_CLASSES, PROF_EXT_INNER,
           PROF_MODDOWN, PROF_TENSOR, PROF_BASISCONV, PROF_SPREAD, PROF_NTT_F2, PROF_OTHER, PROF_NCLASS };
    void prof_enable(bool on);
    void prof_collect(double* ms, long* launches, double* alg_bytes);
    void recover();             // after an exception: active stream back to the main stream, plans dropped, both streams drained   // arrays of PROF_NCLASS; syncs and resets

    // device tables (public for the C ABI accessors / tests)
    Mod* d_mods = nullptr;
    u64 *d_psi = nullptr, *d_psiinv = nullptr, *d_inv_aux = nullptr;
    u64* d_psi31b = nullptr;                     // [mall][16][64][2]: the pairs of stages 5..9 per wave of ntt32_kernels.hip (NttBatch::psi31b)
    u64* d_psi31c = nullptr;                     // [mall][16][31][64][2]: the pairs of stages 10..14 in the load order of ntt32_kernels.hip (NttBatch::psi31c)
    u64* d_psi31n = nullptr;                     // [mall][4][2]: pairs of -psi[1..3] (NttBatch::psi31n)
    u64 *d_psiinv31 = nullptr, *d_inv31c = nullptr;   // inverse twiddles as pairs [mall][N][2]; last-stage constants [mall][8][6] (NttBatch::inv31c)
    unsigned long long small_mods_ = 0;          // bit m set = modulus m has 31 q < 2^62
    u64* d_psif = nullptr;                       // [mall][N] forward twiddles as doubles, N = 2^16 only (NttBatch::psif)
    unsigned long long f_mods_ = 0;              // bit m set = modulus m is of the F class (80 q < 2^52)
    std::vector<unsigned char> h16_sched_;       // per modulus: NttBatch::sched
    unsigned long long u_mods_ = 0;              // bit m: modulus m is of the H16 kernel's U class (NttBatch::u_mods)
    u64* d_psi31 = nullptr;                      // logN >= 15: twiddle pairs of the H16 kernel's one-round product (NttBatch::psi31)
    bool h16_gap_ = false;                       // some modulus has 31q < 2^62 <= 48q: H16's signed ranges do not cover it
    int *d_map_qp = nullptr, *d_map_id = nullptr;
    u64 *d_md_qoverqiinvqi = nullptr, *d_md_qoverqimodp = nullptr, *d_md_vtimes = nullptr, *d_md_down = nullptr;
    u64* d_pmodq = nullptr;                      // [nq] MForm(P mod q_j)
    u64* d_rescale = nullptr;
    u64 *d_dec_a = nullptr, *d_dec_b = nullptr, *d_dec_c = nullptr;     // Decomposer tables (alpha >= 2)
    u64 *d_tb30 = nullptr, *d_tw30 = nullptr;                           // ... and those of the radix-4 spread (alpha = 2, N = 2^16, moduli < 2^57)
    // mkbfv tables: convQQMul in both directions, ModDown constants, mFormQMul, MForm(t) per limb of R
    int* d_map_r = nullptr;
    u64 *d_bq_qoverqiinvqi = nullptr, *d_bq_qoverqimodp = nullptr, *d_bq_vtimes = nullptr;     // Q -> QMul
    u64 *d_bm_qoverqiinvqi = nullptr, *d_bm_qoverqimodp = nullptr, *d_bm_vtimes = nullptr;     // QMul -> Q
    u64 *d_down_q_in_m = nullptr, *d_down_m_in_q = nullptr, *d_mform_qmul = nullptr, *d_t_mont = nullptr;

  private:
    // Every table above and every pool, lazily built table and Scratch buffer below is a block of mem_ (device_memory.h): the members are non-owning
    // pointers into it and release_all names none of them.  (Handles are not in it: pool_free.)  Then the scratch pools:
    // The tables of a first-use build (kg_*, ck_tab_, d_bf_*) keep stale values after a build that failed and was rolled back: read them only behind
    // their *_ready_ flag, never test them for null.
    DeviceMemory mem_;
    u64 *x_ = nullptr, *y_ = nullptr, *swk3_ = nullptr;      // swkPool1..3
    u64* c1_ = nullptr;                                      // ks.Pool[1]  (PolyQP)
    u64* polyq_[3] = {nullptr, nullptr, nullptr};            // polyQPool
    u64* invntt_ = nullptr;                                  // ks.PoolInvNTT
    Scratch nttbuf_;                                         // tensor inputs in NTT form
    Scratch ctbuf_;                                          // rotate / rescale staging
    std::vector<Swk> hoist_pool_[5];                         // rlkSet.HoistPool[0/1] + h(t_i) of step F; [3],[4]: BFV HoistPool2[0/1]
    u64 *x2_ = nullptr, *y2_ = nullptr;                      // BFV swkPool4 / swkPool6
    Scratch rbuf_;                                           // BFV: operands over R, their NTTs, tensor output
    Scratch c1b_;                                            // batched ks.Pool[1]
    Scratch tbuf_;                                           // t_i of step F
    // mul_relin_rescale / mul_relin_batch: Rescale folded into the store of the last merged ModDown.  One entry per product that is not to be
    // written: its (unwritten) base, the rescaled output one level down, its polynomials; `done` once a launch has covered all of them
    struct RsMap { const u64* full; u64* out; int npolys; int out_limbs; bool done; };
    std::vector<RsMap> rs_maps_;
    Scratch spreadbuf_;                                      // N = 2^16: staging of the spread digits (decompose_batch), so that the sub-transforms run out of place
    Scratch tens_;                                           // tensor term kept in the NTT domain (times P) for the merged E / F2 batch
    // key generation scratch: uploaded samples, gadget constants (slot 0: mkrlwe gadget, 1: caller's), permuted secret
    int32_t* kg_small_ = nullptr; u64 *kg_g_ = nullptr, *kg_sk_ = nullptr;
    void wipe_samples(size_t count);
    bool kg_ready_ = false;
    void kg_init();
    // out <- NTT(e_i) for beta_max error polynomials, then the combine pass (keygen_kernels.h); gadget: 0 none, 1 mkrlwe
    // (P on the limbs of digit i, keygen.go:288-323), 2 the constants last uploaded with kg_upload_g
    void kg_key(const int32_t* e, int gadget, const u64* skA, const u64* crs, const u64* skB, int sign, bool neg, u64* out);
    void kg_upload_g(const u64* g_plain);
    // encryption / decryption scratch: work polynomials, uploaded samples, staged pointer tables (encdec.hip)
    Scratch ed_w_, ed_small_, ed_tab_;                       // (int32 samples in ed_small_, const u64* entries in ed_tab_: sized in 8-byte words and cast at the use)
    EdTable ed_table(const std::vector<const u64*>& v, size_t tab_offset);
    void ed_mac(int k, const u64* ch, const u64* const* sks, int limbs, u64* acc);
    // the product chain of a share: w [count][L][N] <- InvNTT(NTT(polynomial slots[b] of ins[b]) * sk); stages its tables at entries 0 .. 2 count of ed_tab_
    void share_product(const std::vector<const Ct*>& ins, const int* slots, const u64* sk, u64* w);
    // w [count][L][N] <- NTT(polynomial slots[b] of ins[b]): one gathering forward transform (per NTT_MAX_ITEMS items)
    void share_gather_ntt(const std::vector<const Ct*>& ins, const int* slots, u64* w);
    // w [count][L][N] <- NTT(src[b] [L][N]), the same gathering transform on bare polynomials (ntt_items with one polynomial per item)
    void gather_ntt(const std::vector<const u64*>& src, int L, u64* w);
    // collective refresh: MForm(q_i mod q_j) and (q_0 .. q_l) mod q_j, [nq][nq] each in one block, built at the first merge; the digits of R
    u64* d_rf_tab_ = nullptr;
    Scratch rf_dig_;
    // Encrypt behind "the samples are on the device": small = int32 [count][3][N] + the count rows of u gathered behind it, w = [3][count][L][N];
    // small_expand .. encrypt_finish and the three wipes
    void encrypt_core(int level, int count, const u64* pk, const u64* pt, bool pt_is_ntt, u64* w, int32_t* small, const EdTable& ot);
    // the same behind "the samples are streams 3 b + j of (key, nonce)": one sampler launch into small, then encrypt_core
    void encrypt_sampled(int level, int count, const u64* pk, const u64* pt, bool pt_is_ntt, const u32* key, u64 nonce, const u64* cdt, int ncdt,
                         u64* w, int32_t* small, const EdTable& ot);
    // the party side of both refreshes: scratch and output table, share_product, the caller's finish kernel (product -> public share and plaintext),
    // the wipe of the product, encrypt_sampled of the plaintext at lout limbs, the wipe of the plaintext
    template <class F> void refresh_share_chain(const std::vector<const Ct*>& ins, const int* slots, const u64* sk, const u64* pk, const u32* key,
                                                u64 nonce_enc, const u64* cdt, int ncdt, int lout, u64* const* outs, double finish_bytes, F finish);
    // the body of refresh_merge and e2s_merge (reenc empty: none is read, outs[b] is one polynomial)
    void refresh_merge_launch(const std::vector<const Ct*>& ins, const std::vector<const u64*>& shares, const std::vector<const u64*>& reenc, int lout,
                              u64* const* outs);
    struct MergeTables { EdTable ot, ct, st, rt; };
    MergeTables merge_tables(const std::vector<const Ct*>& ins, const std::vector<const u64*>& shares, const std::vector<const u64*>& reenc,
                             u64* const* outs);
    // the entry points of encdec.hip refuse a context that owns a subset of the moduli under their own name
    void need_unmasked(const char* what) const;
    // both encoders: the Garner constants [nq][nq], built at the first use, and the two launches of a transform that one tile does not hold:
    // forward the pass over the column tiles (the stages that span the rows) first, inverse last; launch() runs once per pass on the filled-in p
    u64* d_garner_ = nullptr;
    const u64* garner_table();
    template <class F> static void tile_two_pass(TilePass& p, bool inverse, int rows_log, F launch) {
        for (int pass = 0; pass < 2; ++pass) {
            p.first = pass == 0; p.last = pass == 1;
            p.a_log = (pass == 0) != inverse ? rows_log : 0;
            launch();
        }
    }
    // CKKS encoder: tables per slot count n = 2^logn built at its first use (n >= 16: twiddles [n/2][2], twist [n][2], permutation [n]; below:
    // the roots [n][n][2] of the direct sum), the largest FFT one workgroup does in LDS, and the scratch for the two-launch FFT, the Garner digits
    // and the coefficients of the fused calls (sparse packing: compact [count][2n])
    struct CkTables { double *w = nullptr, *twist = nullptr, *root = nullptr; u32* pos = nullptr; bool ready = false; };
    std::vector<CkTables> ck_tab_;                           // by logn < logN
    bool ck_ready_ = false;
    TileLimit ck_tile_{CK_TILE_LOG, CK_TILE_LOG};
    Scratch ck_work_, ck_dig_, ck_coeff_;
    void ck_init(const char* what);
    const CkTables& ck_tables(int logn);
    int ck_sparse_init(const char* what, int log_slots);     // ck_init + the range of log_slots; -> gap_log
    void ck_fft(bool inverse, int logn, int count, const double* in, double* out);
    void ck_scale_up(int level, int count, const double* coeffs, double scale, u64* pt);
    void ck_scale_down(int limbs, int count, const u64* pt, double scale, double* coeffs);
    // BFV batch encoder: tables built at the first call (bf_init), scratch that holds message-derived values (zeroed behind its last use)
    uint2 *d_bf_w = nullptr, *d_bf_winv = nullptr, *d_bf_twist = nullptr, *d_bf_itwist = nullptr, *d_bf_qlt = nullptr;
    u32* d_bf_pos = nullptr;
    u64 *d_bf_tinv = nullptr, *d_bf_tmont = nullptr;
    BfvT bf_t_{};
    u64 bf_psi_ = 0;
    bool bf_ready_ = false;
    TileLimit bf_tile_{BF_TILE_LOG_DEF, BF_TILE_LOG_DEF};
    Scratch bf_work_, bf_dig_, bf_coeff_, bf_lift_;
    void bf_init(const char* what);
    BfvScale bf_scale() const;
    void bf_ntt(bool inverse, int fuse, int count, const u64* in, u64* out);
    void bf_scale_up(int count, const u64* coeffs, u64* pt);
    void bf_lift(int count, const u64* coeffs, u64* ptmul);
    void bf_ptxt_shapes(const char* what, const std::vector<const Ct*>& ins, long pt_stride, const std::vector<Ct*>& outs);
    void bf_scale_down(int count, const u64* pt, u64* coeffs);

    u64* alloc_words(size_t words) { return static_cast<u64*>(mem_.alloc(words * sizeof(u64))); }
    u64* scratch(Scratch& s, size_t want) { return mem_.grow(s, want, stream); }      // grow-only; a larger block waits for the main stream first
    Swk& hoist_slot(int which, int idx);
    const int* map_qp(int level) const { return (masked_ ? d_map_own : d_map_qp) + (size_t)level * mtot; }
    int nslots_qp(int level) const { return masked_ ? own_cnt_[level] : level + 1 + np; }
    // slot ownership (limb sharding)
    bool masked_ = false;
    std::vector<char> own_;                                  // per modulus index < mtot
    std::vector<std::vector<int>> own_list_;                 // per level: owned active modulus indices (Q limbs first)
    std::vector<int> own_cnt_, ownq_;                        // per level: size of own_list_; owned Q limbs, ascending
    int *d_map_own = nullptr, *d_ownq = nullptr;
    int nq_owned(int level) const { int c = 0; for (int l : ownq_) if (l <= level) ++c; return c; }
    void slots_q_owned(NttBatch& b, int L) const;            // plain polynomials: owned Q limbs < L
    void zero_unowned(u64* base, int npolys, long poly_stride, int first_mod, int nlimbs);
    std::vector<ExtItem> lsh_items_;
    void check_level(int level) const;
    void slots_qp(NttBatch& b, int level) const;
    void slots_range(NttBatch& b, int mod_base, int limbs) const;
    void ntt_fwd_launch(const NttBatch& b, bool decompose);
    void ntt_inv_launch(NttBatch& b);       // fills in the tables of the H16-class inverse kernel, then the steps of ntt_inv_route
    NttShape ntt_shape(const NttBatch& b, bool decompose, bool inverse) const;
    std::vector<unsigned char> small_q_;                     // per modulus: 34q < 2^63
    std::vector<unsigned char> small16_;                     // per modulus: 48q < 2^62 -- the short class of the H16 / H32 kernels (ntt16_kernels.hip)
    void ext_core(int level, const u64* ah, const u64* bg, u64* c, bool accumulate);

    struct MrPlan {
        bool valid = false;
        int level = 0, L = 0, n0 = 0, n1 = 0, nout = 0;
        std::vector<int> slot0, slot1;
        std::vector<const u64*> h0, h1;
        bool own0 = false, own1 = false;     // hoisted digits computed by the engine itself
        bool x_pending = false;              // x still running on the side stream (chain 2)
        const u64* tens = nullptr;           // the tensor term stays in the NTT domain (times P) and joins the E / F2 batch
        bool head_done = false;              // mr_finish_head ran, mr_finish_tail still to come
        std::vector<const u64*> xkeys;       // non-empty: x is produced by the F1 kernel of mr_finish_head (into xfused) instead of by mr_xy
        u64* xfused = nullptr;
        std::vector<const u64*> ykeys;       // non-empty: y is computed inside the F1 kernel from these keys (b_j) and h1 (never stored)
        bool f2_staged = false;              // the digits of the t_i were left after the cross stages (decompose_batch stage_only): the tail batch finishes them
        bool f2_fused = false;               // N = 2^15: no Decompose launch for the t_i at all -- the tail batch's product kernel is ntt16_f2_kernel
        const u64* f2_tbuf = nullptr;
        bool e_done = false;                 // ... and so was step E: its products sit in the c1 slots 2 n0 .. 2 n0 + n1 - 1 of the scratch, for the tail batch
        bool e_summed = false;               // mul_relin_sum: step E of every pair (with the tensor terms of those slots) is in `out` already: the tail runs F2 only
    } plan_;
    // bfv_mr_partial -> bfv_mr_finish
    struct BfvPlan {
        bool valid = false;
        std::vector<const u64*> xk1, xk2;        // single-device MulRelinNew: d1_i, d2_i for the fused x1, x2
        std::vector<const u64*> yk1, yk2;        // ... and b1_j, b2_j when y1, y2 (and step E) are computed inside the F1 kernel too
        u64 *xout1 = nullptr, *xout2 = nullptr;  // fused: where the F1 kernel of bfv_mr_finish stores x1, x2
    } bfv_plan_;

    // Stream-ordered buffer pool.  A buffer freed through this context may still be in use by kernels that ANOTHER context of the
    // same device enqueued (handles are shared freely between forked contexts).  Ordering between contexts is tracked with one
    // counter per context: seq_ counts the C-ABI calls that named the context (anything it may have enqueued), completed_ is seq_ at
    // its last host-side drain, and synced_ holds, per other context, the seq_ value this context's stream is known to be ordered
    // after (wait_for, fences).  A free records for which contexts that knowledge is behind at that moment; pool_alloc makes the
    // stream wait for exactly those (one event each) unless a wait_for / drain has caught up in the meantime.  The joins an
    // application needs for its own data flow therefore make the pool free of charge; single-context processes never fence.
    // Which contexts enqueued work on a handle's buffer is recorded in the handle (HandleUsers, filled by the C ABI on every call
    // that names the handle), so a temporary that never left its context costs nothing and never orders independent forks.
    struct FreeEntry { size_t words; u64* p; std::vector<std::pair<seq_t, seq_t>> behind; };      // (uid of a context, its seq_ at the free)
    std::vector<FreeEntry> free_list_;
    std::mutex pool_mu_;                                      // guards free_list_ (a trim may come from another context's thread); taken AFTER the registry mutex, never before
    hipEvent_t fence_ev_ = nullptr;
    void registry_add();
    void init(const u64* Q, const u64* P, const u64* psiQ, const u64* psiP, const u64* QMul, int nqm_, u64 T);     // the constructor's body
    void release_all() noexcept;                              // mem_, the handle pool, events, streams (destructor; constructor that throws)
    void registry_remove();
    seq_t uid_ = 0;
    std::atomic<seq_t> seq_{1}, completed_{0};
    std::atomic<seq_t> enqueued_{0};                         // seq_ as of the last C-ABI call that has FINISHED enqueuing its work: the clock an event
                                                             // recorded on this context's stream by ANOTHER thread may claim to cover (seq_ runs ahead of it
                                                             // while a call is in flight)
    std::atomic<bool> external_{false};                      // stream handed out (mkhe_ctx_stream): work may arrive without a C-ABI call
    std::vector<std::pair<seq_t, seq_t>> synced_;            // (uid, seq_) pairs, guarded by the registry mutex
    seq_t synced_with(seq_t uid) const { for (auto& e : synced_) if (e.first == uid) return e.second; return 0; }
    void set_synced(seq_t uid, seq_t v) { for (auto& e : synced_) if (e.first == uid) { if (e.second < v) e.second = v; return; } synced_.push_back({uid, v}); }
  public:
    void note_use(HandleUsers& u);                            // this context is about to enqueue work on the handle's buffer
    void touch() { seq_.fetch_add(1, std::memory_order_relaxed); }
    void mark_enqueued() { const seq_t s = seq_.load(); if (enqueued_.load() < s) enqueued_.store(s); }
    void mark_external() { external_.store(true); }
    seq_t now_seq() { return external_.load() ? seq_.fetch_add(1) + 1 : seq_.load(); }
  private:

    struct ProfRec { hipEvent_t e0, e1; int cls; double bytes; };
  public:
    // MKHE_NTT32=2 (default): which forward kernel a launch shape takes when both apply (H32 and H16 give the same bits), measured in the caller's own
    // workload.  The single-pass kernel wins by 2-5 % inside a MulRelin on most parts and loses 6 % on some (same library, same call:
    // profiles/README.md) -- back to back it is ahead on all of them, so a calibration outside the workload would pick wrongly; so did a first version
    // that alternated the kernels over the first dozen launches (the first milliseconds run on ramping clocks with power to spare), and a second that
    // timed the kernel alone (with the side stream on, a kernel's duration says little about the operation's).  What is measured is the PERIOD of the
    // shape -- the time from one of its launches to the next on the GPU's clock, i.e. the whole operation around it in a running service.  Per shape:
    // WARM launches on H16, then a block on H32 and a block on H16 (SETTLE launches, then TIMED periods); the medians decide, the choice stays.
    // A smaller shape follows the largest one unless the other kernel is 3 % ahead.
    struct NttTune { static constexpr int WARM = 64, SETTLE = 16, TIMED = 32, RING = 2 * (TIMED + 1); int n[2] = {0, 0}, req[2] = {0, 0}, blk[2] = {0, 0}; float t[2][TIMED];
                     int decided = -1, seen = 0;
                     // start events of the timed launches that have not been turned into periods yet (the host runs ahead of the GPU): ring[head .. head + inflight)
                     hipEvent_t e0[RING] = {}; int which[RING] = {}; int head = 0, inflight = 0; int slot = -1; };
    std::map<long, NttTune> ntt_tune_;
    int ntt_forced_ = -1;                            // mkhe_ctx_set_ntt_choice(limbs <= 0): the answer for every shape that has no entry of its own
    long batch_lanes_min_ = 1536;      // mkhe_ctx_set_batch_lanes: hoisted limb-NTTs per input from which mul_relin_batch runs its inputs in flight (< 0: never)
    void ntt_reset(NttTune& t, int choice);          // pins a shape (0 / 1) or makes it measure again (-1); samples in flight are dropped
    int ntt_pick(long key, NttTune*& sampling);      // 1 = H32, 0 = H16; sampling != nullptr: this launch is timed (record e0[slot] in front of it)
  private:
    bool prof_on_ = false;
    std::vector<ProfRec> prof_recs_;
    std::vector<hipEvent_t> prof_pool_;
    hipEvent_t prof_event();
    hipStream_t s_ = nullptr;                                // active stream of the launch helpers
    hipEvent_t ev_[8] = {};                                  // fork/join events of the side stream
    hipEvent_t xev_ = nullptr;                               // wait_for
    // mul_relin_batch at N >= 2^15: the B evaluations go through the single-operation path on this context and two internal ones, round robin -- in
    // flight side by side (the latency-bound stretches of one beside the other's kernels) instead of in lock step (batch.hip)
    std::vector<std::unique_ptr<Context>> lanes_;
    Context* lane(int i);
    bool batch_lanes_ok(size_t B, long limbs) const;
    void fork_side(int k);      // side stream waits for everything enqueued so far on the active stream
    void side_done(int k);      // marks the end of side chain k
    void join_side(int k);      // active stream waits for side chain k
  public:
    struct ProfScope {
        Context* c; size_t idx; bool on; hipStream_t st;
        ProfScope(Context* c_, int cls, double bytes);
        ~ProfScope();
    };
};

// slot0[a] / slot1[a] = where out carries id a of op0 / op1; out's ids must be exactly the union (newCiphertextBinary, mkckks/evaluator.go:306-313).
// out_name opens the refusals ("mkhe: ctOut")
void union_slots(const Ct& op0, const Ct& op1, const Ct& out, const char* out_name, std::vector<int>& slot0, std::vector<int>& slot1);
// the term table of tensor_sum_kernel for a pair laid out c0_0, c0_i, c1_0, c1_j (poly_kernels.h, TensorSumArgs::term)
void tensor_sum_terms(TensorSumArgs& ta, int n0, int n1, const std::vector<int>& slot0, const std::vector<int>& slot1, int nout);
// conv.Quantize behind its MulScalar and inverse NTT (basis_extension.go:66-80): ModDownQPtoQ of polyr [npolys][2 nQ][N] with QMul as "P"
void quantize_tail_args(BasisConvArgs& a, const Context& c, u64* polyr, u64* polyq, int npolys);

}  // namespace mkhe
