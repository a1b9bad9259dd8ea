// capi.hip -- extern "C" boundary (include/mkhe.h) over mkhe::Context.
#include "../../include/mkhe.h"
#include "engine.h"
#include <string>
#include <vector>

using namespace mkhe;

struct mkhe_ctx { Context* c; };
// handles created in one call (mkhe_ct_create_batch / mkhe_swk_create_batch) are views into ONE pooled block, which goes back to the pool when the last
// of them is destroyed -- behind the uses of all of them
struct mkhe_block { u64* base; size_t words; int refs; HandleUsers users; };
struct mkhe_swk { Swk s; mutable HandleUsers users; mkhe_block* blk = nullptr; };
struct mkhe_ct { Ct c; mutable HandleUsers users; mkhe_block* blk = nullptr; };
static mkhe_block* block_new(Context* c, size_t words, int refs) {
    mkhe_block* b = new mkhe_block();
    b->words = words; b->refs = refs; b->base = nullptr;
    try { b->base = c->pool_alloc(words); } catch (...) { delete b; throw; }
    return b;
}
static void block_release(mkhe_ctx* ctx, mkhe_block* b, const HandleUsers& u) {
    for (const auto& e : u.v) {
        bool found = false;
        for (auto& f : b->users.v) if (f.first == e.first) { if (e.second > f.second) f.second = e.second; found = true; }
        if (!found) b->users.v.push_back(e);
    }
    b->users.exposed = b->users.exposed || u.exposed;
    if (--b->refs > 0) return;
    if (ctx) ctx->c->pool_free(b->base, b->words, &b->users); else (void)hipFree(b->base);
    delete b;
}
struct mkhe_graph { hipGraphExec_t exec; };

static thread_local std::string g_err;

// An exception may leave the context in the middle of a forked chain (active stream still the side stream, a side chain that
// writes into the caller's output never joined, a MulAndRelin plan half executed): recover() puts the context back into its
// idle state and drains both streams before the error is reported, so that the caller may free its handles safely.
static thread_local Context* g_last_ctx = nullptr;
// g_last_ctx is reset first, so that a call that fails before it reaches need() -- mkhe_ctx_create, a null-argument check -- never drains or
// invalidates the plan of whichever context this thread happened to use last (which may even be gone).
#define MKHE_TRY(body) g_last_ctx = nullptr; try { body; if (g_last_ctx) g_last_ctx->mark_enqueued(); return 0; } \
    catch (const std::exception& e) { g_err = e.what(); if (g_last_ctx) g_last_ctx->recover(); return 1; } \
    catch (...) { g_err = "mkhe: unknown error"; if (g_last_ctx) g_last_ctx->recover(); return 1; }

// every entry point goes through this: a null context is an error of the caller, reported like any other
static Context* need(const mkhe_ctx* ctx) {
    if (!ctx || !ctx->c) { g_last_ctx = nullptr; throw Error("mkhe: null context"); }
    g_last_ctx = ctx->c;
    ctx->c->touch();                 // anything this call enqueues is counted (Context::seq_, the pool's ordering clock)
    return ctx->c;
}

// Every entry point names the handles it is about to enqueue work on (Context::note_use: the pool of whichever context the buffer
// is freed into later orders itself behind exactly these uses, csrc/engine.h).
static void mark1(Context* c, const mkhe_ct* h) { if (h) c->note_use(h->users); }
static void mark1(Context* c, const mkhe_swk* h) { if (h) c->note_use(h->users); }
template <class... H> static void mark(const mkhe_ctx* ctx, H... hs) { if (ctx && ctx->c) { (mark1(ctx->c, hs), ...); } }

static std::vector<const Swk*> swk_list(const mkhe_ctx* ctx, const mkhe_swk* const* v, int n) {
    std::vector<const Swk*> r;
    if (!v) return r;
    r.resize(n);
    for (int i = 0; i < n; ++i) { if (!v[i]) throw Error("mkhe: null key handle in a per-party key list"); mark(ctx, v[i]); r[i] = &v[i]->s; }
    return r;
}

// ---- the guard of the sampler, protocol and encoder entry points: whether a call may run at all -- off a limb-sharded context, outside a
// capture whose replay would draw the same stream again or that cannot hold what the call does, and without recover()ing a context (or ending a
// capture) that the call never touched.  Every step is written once, here; an entry calls the steps it needs in its own order.  enter() leaves g_last_ctx null, so that a refusal is reported with nothing drained; commit() arms it behind the last check that can
// refuse with nothing enqueued.  A key is never quoted in a message.  enter(ctx, null) reports a null context with need()'s own message.
static Context* enter(const mkhe_ctx* ctx, const char* what) {
    if (what && !ctx) throw Error(std::string(what) + ": null context");
    Context* c = need(ctx);
    g_last_ctx = nullptr;
    return c;
}
// last(): the refusals that need the device selected (tables built at the first use)
template <class F> static void commit(Context* c, F last) {
    MKHE_HIP(hipSetDevice(c->device));
    last();
    g_last_ctx = c;
}
static void commit(Context* c) { commit(c, [] {}); }
static void count_ok(const char* what, int count) {
    if (count < 1 || count > 65535) throw Error(std::string(what) + ": count must be 1 .. 65535");
}
static void need_aligned(const void* p, const char* what) {
    if ((uintptr_t)p & 15) throw Error(std::string(what) + ": device buffers must be 16-byte aligned");
}
static void scheme_ok(const Context* c, const char* what, bool bfv, const char* why) {
    if (c->is_bfv() != bfv) throw Error(std::string(what) + why);
}
static void unmasked(const Context* c, const char* what) {
    if (c->masked()) throw Error(std::string(what) + ": not available on a context that owns a subset of the moduli");
}
// why closes the message: what a replay would do, or what the call does that a capture cannot hold
static const char* const REPLAYS = "(a replay would repeat the keystream)";
static const char* const UPLOADS = "(the call allocates and uploads)";
static const char* const STAGES = "with more than 16 ciphertexts or shares (the pointer tables are staged)";
static void not_captured(const Context* c, const char* what, const char* why) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(c->stream, &cs);
    if (cs != hipStreamCaptureStatusNone) throw Error(std::string(what) + ": not available inside mkhe_capture_begin .. mkhe_capture_end " + why);
}
// the inputs of a batch: present and at one level -- `limbs` of them (why_limbs says so), or (limbs = 0) as many as the first has
static const Ct& ct_at(const mkhe_ct* const* v, int i, const char* what) {
    if (!v[i]) throw Error(std::string(what) + ": null ciphertext in the batch");
    return v[i]->c;
}
static void batch_ok(const char* what, int count, const mkhe_ct* const* in, int limbs = 0, const char* why_limbs = nullptr) {
    for (int b = 0; b < count; ++b)
        if (ct_at(in, b, what).limbs != (limbs ? limbs : in[0]->c.limbs))
            throw Error(std::string(what) + (limbs ? why_limbs : ": every ciphertext must be at the same level"));
}
static void slots_ok(const char* what, int count, const mkhe_ct* const* in, const int* slots) {
    for (int b = 0; b < count; ++b)
        if (slots[b] < 1 || slots[b] > in[b]->c.n) throw Error(std::string(what) + ": slot out of range (party slots are 1 .. n)");
}
// the inputs of a merge are over the same ids, with one share per party
static void merge_shape(const char* what, int count, const mkhe_ct* const* in, int nshares) {
    for (int b = 0; b < count; ++b)
        if (in[b]->c.ids != in[0]->c.ids) throw Error(std::string(what) + ": every ciphertext must be over the same ids");
    if (nshares != in[0]->c.n) throw Error(std::string(what) + ": nshares must be the number of parties of the ciphertexts (one share per party, in slot order)");
}
static const u64* share_at(const void* const* v, int i, const char* what) {
    if (!v[i]) throw Error(std::string(what) + ": null share in the per-party list");
    need_aligned(v[i], what);
    return (const u64*)v[i];
}
static std::vector<const u64*> share_list(const void* const* v, int n, const char* what) {
    std::vector<const u64*> r(n);
    for (int i = 0; i < n; ++i) r[i] = share_at(v, i, what);
    return r;
}

extern "C" {

const char* mkhe_last_error(void) { return g_err.c_str(); }

int mkhe_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }

int mkhe_ctx_create(mkhe_ctx** out, int logN, const uint64_t* Q, int nQ, const uint64_t* P, int nP,
                    int gamma, const uint64_t* psiQ, const uint64_t* psiP, int device) {
    MKHE_TRY({
        if (!out || !Q || !P) throw Error("mkhe_ctx_create: null argument");
        *out = new mkhe_ctx{new Context(logN, Q, nQ, P, nP, gamma, psiQ, psiP, device)};
    })
}
void mkhe_ctx_destroy(mkhe_ctx* ctx) { if (ctx) { if (g_last_ctx == ctx->c) g_last_ctx = nullptr; delete ctx->c; delete ctx; } }
int mkhe_ctx_sync(mkhe_ctx* ctx) { MKHE_TRY(need(ctx)->sync()) }
int mkhe_capture_begin(mkhe_ctx* ctx) {
    MKHE_TRY({
        MKHE_HIP(hipSetDevice(need(ctx)->device));
        // the engine captures several streams (side stream, forked contexts) that join each other in both directions; the
        // HIP runtime of ROCm 7.0 (e.g. the one bundled with PyTorch 2.10, which a process that imported torch first
        // binds to) recurses without end in hipStreamEndCapture on such a capture.  Refuse instead of crashing.
        int rv = 0;
        MKHE_HIP(hipRuntimeGetVersion(&rv));
        if (rv < 70200000) throw Error("mkhe_capture_begin: the HIP runtime loaded in this process (version " + std::to_string(rv) +
                                       ") cannot end a multi-stream capture; graph capture needs the ROCm >= 7.2 runtime");
        MKHE_HIP(hipStreamBeginCapture(need(ctx)->stream, hipStreamCaptureModeRelaxed));
    })
}
int mkhe_capture_end(mkhe_ctx* ctx, mkhe_graph** out) {
    MKHE_TRY({
        if (!out) throw Error("mkhe_capture_end: null argument");
        hipGraph_t g = nullptr;
        MKHE_HIP(hipStreamEndCapture(need(ctx)->stream, &g));
        hipGraphExec_t ex = nullptr;
        const hipError_t e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (e != hipSuccess) throw Error(std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
        *out = new mkhe_graph{ex};
    })
}
int mkhe_graph_launch(mkhe_ctx* ctx, mkhe_graph* graph) {
    MKHE_TRY({ if (!graph) throw Error("mkhe_graph_launch: null argument"); MKHE_HIP(hipGraphLaunch(graph->exec, need(ctx)->stream)); })
}
void mkhe_graph_destroy(mkhe_graph* graph) { if (graph) { (void)hipGraphExecDestroy(graph->exec); delete graph; } }
int mkhe_ctx_wait_for(mkhe_ctx* ctx, mkhe_ctx* other) {
    MKHE_TRY({ if (!ctx || !other) throw Error("mkhe_ctx_wait_for: null argument"); need(ctx)->wait_for(*need(other)); })
}
int mkhe_ctx_alpha(const mkhe_ctx* ctx) { if (!ctx) return 0; return ctx->c->alpha; }
int mkhe_ctx_beta(const mkhe_ctx* ctx, int level) { if (!ctx) return 0; return ctx->c->beta(level); }
int mkhe_ctx_n(const mkhe_ctx* ctx) { if (!ctx) return 0; return ctx->c->N; }
size_t mkhe_ctx_swk_words(const mkhe_ctx* ctx) { if (!ctx) return 0; return ctx->c->swk_words(); }
uint64_t mkhe_ctx_psi(const mkhe_ctx* ctx, int i) { if (!ctx) return 0; return (i >= 0 && i < ctx->c->mall) ? ctx->c->psi_plain[i] : 0; }
void* mkhe_ctx_stream(mkhe_ctx* ctx) { if (!ctx) return 0; ctx->c->mark_external(); return (void*)ctx->c->stream; }

// ---- switching keys
static void swk_create(mkhe_ctx* ctx, mkhe_swk** out, bool zero) {
    Context* c = need(ctx);
    MKHE_HIP(hipSetDevice(c->device));
    if (!out) throw Error("mkhe_swk_create: null argument");
    mkhe_swk* s = new mkhe_swk();
    try { s->s.d = c->pool_alloc(c->swk_words()); } catch (...) { delete s; throw; }
    if (zero) { c->note_use(s->users); MKHE_HIP(hipMemsetAsync(s->s.d, 0, c->swk_words() * sizeof(u64), c->stream)); }
    *out = s;
}
int mkhe_swk_create(mkhe_ctx* ctx, mkhe_swk** out) { MKHE_TRY(swk_create(ctx, out, true)) }
int mkhe_swk_create_uninit(mkhe_ctx* ctx, mkhe_swk** out) { MKHE_TRY(swk_create(ctx, out, false)) }
void mkhe_swk_destroy(mkhe_ctx* ctx, mkhe_swk* swk) {
    if (!swk) return;
    if (swk->blk) block_release(ctx, swk->blk, swk->users);
    else if (swk->s.d && swk->s.owned) { if (ctx) ctx->c->pool_free(swk->s.d, ctx->c->swk_words(), &swk->users); else (void)hipFree(swk->s.d); }
    delete swk;
}
int mkhe_swk_create_batch(mkhe_ctx* ctx, int count, mkhe_swk** out) {
    MKHE_TRY({
        Context* c = need(ctx);
        if (!out || count < 1) throw Error("mkhe_swk_create_batch: bad argument");
        MKHE_HIP(hipSetDevice(c->device));
        mkhe_block* b = block_new(c, (size_t)count * c->swk_words(), count);
        for (int i = 0; i < count; ++i) { mkhe_swk* s = new mkhe_swk(); s->s.d = b->base + (size_t)i * c->swk_words(); s->s.owned = false; s->blk = b; out[i] = s; }
    })
}
void mkhe_swk_destroy_batch(mkhe_ctx* ctx, int count, mkhe_swk* const* swks) {
    if (!swks) return;
    for (int i = 0; i < count; ++i) mkhe_swk_destroy(ctx, swks[i]);
}
int mkhe_swk_upload(mkhe_ctx* ctx, mkhe_swk* swk, const uint64_t* host) {
    MKHE_TRY({ mark(ctx, swk);
        Context* c = need(ctx);
        if (!swk || !host) throw Error("mkhe_swk_upload: null argument");
        MKHE_HIP(hipMemcpyAsync(swk->s.d, host, c->swk_words() * sizeof(u64), hipMemcpyHostToDevice, c->stream));
        c->sync();
    })
}
int mkhe_swk_upload_limbs(mkhe_ctx* ctx, mkhe_swk* swk, const uint64_t* const* limbs, int ndigits) {
    MKHE_TRY({ mark(ctx, swk);
        Context* c = need(ctx);
        if (!swk || !limbs) throw Error("mkhe_swk_upload_limbs: null argument");
        if (ndigits < 0 || ndigits > c->beta_max) throw Error("mkhe_swk_upload_limbs: bad digit count");
        for (int i = 0; i < ndigits * c->mtot; ++i)
            MKHE_HIP(hipMemcpyAsync(swk->s.d + (size_t)i * c->N, limbs[i], (size_t)c->N * sizeof(u64), hipMemcpyHostToDevice, c->stream));
        c->sync();
    })
}
int mkhe_swk_download(mkhe_ctx* ctx, const mkhe_swk* swk, uint64_t* host) {
    MKHE_TRY({ mark(ctx, swk);
        Context* c = need(ctx);
        if (!swk || !host) throw Error("mkhe_swk_download: null argument");
        MKHE_HIP(hipMemcpyAsync(host, swk->s.d, c->swk_words() * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        c->sync();
    })
}
void* mkhe_swk_devptr(mkhe_swk* swk) { if (swk) swk->users.exposed = true; return swk ? swk->s.d : nullptr; }

// ---- ciphertexts
static void ct_create(mkhe_ctx* ctx, int n, const int* ids, int limbs, bool zero, mkhe_ct** out);
int mkhe_ct_create(mkhe_ctx* ctx, int n, const int* ids, int limbs, mkhe_ct** out) {
    MKHE_TRY(ct_create(ctx, n, ids, limbs, true, out))
}
int mkhe_ct_create_uninit(mkhe_ctx* ctx, int n, const int* ids, int limbs, mkhe_ct** out) {
    MKHE_TRY(ct_create(ctx, n, ids, limbs, false, out))
}
} // extern "C"
static void ct_create(mkhe_ctx* ctx, int n, const int* ids, int limbs, bool zero, mkhe_ct** out) {
    {
        Context* c = need(ctx);
        if (!out || (n > 0 && !ids)) throw Error("mkhe_ct_create: null argument");
        if (n < 0 || n > 32 || limbs < 1 || limbs > c->nq) throw Error("mkhe_ct_create: bad shape");
        MKHE_HIP(hipSetDevice(c->device));
        mkhe_ct* t = new mkhe_ct();
        t->c.n = n; t->c.limbs = limbs; t->c.ids.assign(ids, ids + n);
        for (int i = 0; i < n; ++i) for (int j = 0; j < i; ++j) if (ids[i] == ids[j]) { delete t; throw Error("mkhe_ct_create: repeated id"); }
        const size_t w = (size_t)(1 + n) * limbs * c->N;
        try { t->c.d = c->pool_alloc(w); } catch (...) { delete t; throw; }
        if (zero) { c->note_use(t->users); MKHE_HIP(hipMemsetAsync(t->c.d, 0, w * sizeof(u64), c->stream)); }
        *out = t;
    }
}
extern "C" {
void mkhe_ct_destroy(mkhe_ctx* ctx, mkhe_ct* ct) {
    if (!ct) return;
    if (ct->blk) block_release(ctx, ct->blk, ct->users);
    else if (ct->c.d) { if (ctx) ctx->c->pool_free(ct->c.d, (size_t)(1 + ct->c.n) * ct->c.limbs * ctx->c->N, &ct->users); else (void)hipFree(ct->c.d); }
    delete ct;
}
int mkhe_ct_create_batch(mkhe_ctx* ctx, int nbatch, int n, const int* ids, int limbs, mkhe_ct** out) {
    MKHE_TRY({
        Context* c = need(ctx);
        if (!out || nbatch < 1 || (n > 0 && !ids)) throw Error("mkhe_ct_create_batch: bad argument");
        if (n < 0 || n > 32 || limbs < 1 || limbs > c->nq) throw Error("mkhe_ct_create_batch: bad shape");
        for (int i = 0; i < n; ++i) for (int j = 0; j < i; ++j) if (ids[i] == ids[j]) throw Error("mkhe_ct_create_batch: repeated id");
        MKHE_HIP(hipSetDevice(c->device));
        const size_t w = (size_t)(1 + n) * limbs * c->N;
        mkhe_block* b = block_new(c, (size_t)nbatch * w, nbatch);
        for (int k = 0; k < nbatch; ++k) {
            mkhe_ct* t = new mkhe_ct();
            t->c.n = n; t->c.limbs = limbs; t->c.ids.assign(ids, ids + n); t->c.d = b->base + (size_t)k * w; t->blk = b;
            out[k] = t;
        }
    })
}
void mkhe_ct_destroy_batch(mkhe_ctx* ctx, int nbatch, mkhe_ct* const* cts) {
    if (!cts) return;
    for (int k = 0; k < nbatch; ++k) mkhe_ct_destroy(ctx, cts[k]);
}
int mkhe_ct_upload(mkhe_ctx* ctx, mkhe_ct* ct, const uint64_t* host) {
    MKHE_TRY({ mark(ctx, ct);
        Context* c = need(ctx);
        if (!ct || !host) throw Error("mkhe_ct_upload: null argument");
        const size_t w = (size_t)(1 + ct->c.n) * ct->c.limbs * c->N;
        MKHE_HIP(hipMemcpyAsync(ct->c.d, host, w * sizeof(u64), hipMemcpyHostToDevice, c->stream));
        c->sync();
    })
}
int mkhe_ct_copy(mkhe_ctx* ctx, const mkhe_ct* in, mkhe_ct* out) {
    MKHE_TRY({ mark(ctx, in, out);
        if (!in || !out) throw Error("mkhe_ct_copy: null argument");
        if (in->c.n != out->c.n || in->c.limbs != out->c.limbs || in->c.ids != out->c.ids) throw Error("mkhe_ct_copy: shapes differ");
        const size_t w = (size_t)(1 + in->c.n) * in->c.limbs * need(ctx)->N;
        MKHE_HIP(hipMemcpyAsync(out->c.d, in->c.d, w * sizeof(u64), hipMemcpyDeviceToDevice, need(ctx)->stream));
    })
}
int mkhe_ct_upload_poly_limbs(mkhe_ctx* ctx, mkhe_ct* ct, int slot, const uint64_t* const* limbs) {
    MKHE_TRY({ mark(ctx, ct);
        Context* c = need(ctx);
        if (!ct || !limbs) throw Error("mkhe_ct_upload_poly_limbs: null argument");
        if (slot < 0 || slot > ct->c.n) throw Error("mkhe_ct_upload_poly_limbs: bad slot");
        for (int l = 0; l < ct->c.limbs; ++l)
            MKHE_HIP(hipMemcpyAsync(ct->c.d + ((size_t)slot * ct->c.limbs + l) * c->N, limbs[l], (size_t)c->N * sizeof(u64), hipMemcpyHostToDevice, c->stream));
        c->sync();
    })
}
int mkhe_ct_download(mkhe_ctx* ctx, const mkhe_ct* ct, uint64_t* host) {
    MKHE_TRY({ mark(ctx, ct);
        Context* c = need(ctx);
        if (!ct || !host) throw Error("mkhe_ct_download: null argument");
        const size_t w = (size_t)(1 + ct->c.n) * ct->c.limbs * c->N;
        MKHE_HIP(hipMemcpyAsync(host, ct->c.d, w * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        c->sync();
    })
}
int mkhe_ct_download_poly_limbs(mkhe_ctx* ctx, const mkhe_ct* ct, int slot, uint64_t* const* limbs) {
    MKHE_TRY({ mark(ctx, ct);
        Context* c = need(ctx);
        if (!ct || !limbs) throw Error("mkhe_ct_download_poly_limbs: null argument");
        if (slot < 0 || slot > ct->c.n) throw Error("mkhe_ct_download_poly_limbs: bad slot");
        for (int l = 0; l < ct->c.limbs; ++l)
            MKHE_HIP(hipMemcpyAsync(limbs[l], ct->c.d + ((size_t)slot * ct->c.limbs + l) * c->N, (size_t)c->N * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        c->sync();
    })
}
int mkhe_ct_limbs(const mkhe_ct* ct) { return ct ? ct->c.limbs : 0; }
int mkhe_ct_nparties(const mkhe_ct* ct) { return ct ? ct->c.n : 0; }
void* mkhe_ct_devptr(mkhe_ct* ct) { if (ct) ct->users.exposed = true; return ct ? ct->c.d : nullptr; }

// ---- raw buffers
int mkhe_buf_alloc(mkhe_ctx* ctx, size_t words, void** dev_out) {
    MKHE_TRY({
        MKHE_HIP(hipSetDevice(need(ctx)->device));
        void* d = nullptr;
        MKHE_HIP(hipMalloc(&d, (words ? words : 1) * sizeof(u64)));
        *dev_out = d;
    })
}
void mkhe_buf_free(mkhe_ctx* ctx, void* dev) {
    if (!dev) return;
    if (ctx) (void)hipStreamSynchronize(ctx->c->stream);
    (void)hipFree(dev);
}
int mkhe_buf_upload(mkhe_ctx* ctx, void* dev, const uint64_t* host, size_t words) {
    MKHE_TRY({
        MKHE_HIP(hipMemcpyAsync(dev, host, words * sizeof(u64), hipMemcpyHostToDevice, need(ctx)->stream));
        need(ctx)->sync();
    })
}
int mkhe_buf_download(mkhe_ctx* ctx, const void* dev, uint64_t* host, size_t words) {
    MKHE_TRY({
        MKHE_HIP(hipMemcpyAsync(host, dev, words * sizeof(u64), hipMemcpyDeviceToHost, need(ctx)->stream));
        need(ctx)->sync();
    })
}

// ---- ring level
int mkhe_ntt(mkhe_ctx* ctx, const void* src, void* dst, int count, int limbs, int mod_base, int inverse, int lazy) {
    MKHE_TRY({ if (!src || !dst || count < 1 || limbs < 1) throw Error("mkhe_ntt: bad argument"); need(ctx)->ntt((const u64*)src, (u64*)dst, count, limbs, mod_base, inverse != 0, lazy != 0); })
}

// ---- KeySwitcher
static const u64* ct_slot(const Context* c, const mkhe_ct* ct, int slot, int level) {
    if (!ct) throw Error("mkhe: null ciphertext");
    if (slot < 0 || slot > ct->c.n) throw Error("mkhe: bad ciphertext slot");
    if (ct->c.limbs < level + 1) throw Error("mkhe: ciphertext level below requested level");
    return ct->c.d + (size_t)slot * ct->c.limbs * c->N;
}
int mkhe_decompose(mkhe_ctx* ctx, int level, int is_ntt, const mkhe_ct* ct, int slot, mkhe_swk* out) {
    MKHE_TRY({ mark(ctx, ct, out); if (!out) throw Error("mkhe_decompose: null argument"); need(ctx)->decompose(level, is_ntt != 0, ct_slot(need(ctx), ct, slot, level), out->s.d); })
}
int mkhe_hoisted_form(mkhe_ctx* ctx, int level, const mkhe_ct* ct, mkhe_swk* const* out) {
    MKHE_TRY({ mark(ctx, ct);
        if (!ct || (ct->c.n > 0 && !out)) throw Error("mkhe_hoisted_form: null argument");
        std::vector<const u64*> src; std::vector<u64*> dst;
        for (int i = 0; i < ct->c.n; ++i) {
            if (!out[i]) throw Error("mkhe_hoisted_form: null output handle");
            mark(ctx, out[i]);
            src.push_back(ct_slot(need(ctx), ct, 1 + i, level)); dst.push_back(out[i]->s.d);
        }
        if (!src.empty()) need(ctx)->decompose_batch(level, src, dst, false);
    })
}
int mkhe_external_product(mkhe_ctx* ctx, int level, int is_ntt, const mkhe_ct* a, int slot,
                          const mkhe_swk* bg, mkhe_ct* out, int out_slot) {
    MKHE_TRY({ mark(ctx, a, bg, out);
        if (!out || !bg) throw Error("mkhe_external_product: null argument");
        if (out->c.limbs != level + 1) throw Error("mkhe_external_product: out must have level+1 limbs");
        need(ctx)->external_product(level, is_ntt != 0, ct_slot(need(ctx), a, slot, level), bg->s.d,
                                 const_cast<u64*>(ct_slot(need(ctx), out, out_slot, level)), false);
    })
}
int mkhe_external_product_hoisted(mkhe_ctx* ctx, int level, const mkhe_swk* ah, const mkhe_swk* bg, mkhe_ct* out, int out_slot) {
    MKHE_TRY({ mark(ctx, ah, bg, out);
        if (!out || !ah || !bg) throw Error("mkhe_external_product_hoisted: null argument");
        if (out->c.limbs != level + 1) throw Error("mkhe_external_product_hoisted: out must have level+1 limbs");
        need(ctx)->external_product_hoisted(level, ah->s.d, bg->s.d, const_cast<u64*>(ct_slot(need(ctx), out, out_slot, level)), false);
    })
}
int mkhe_mul_and_relin(mkhe_ctx* ctx, const mkhe_ct* op0, const mkhe_ct* op1,
                       const mkhe_swk* const* hoist0, const mkhe_swk* const* hoist1,
                       const mkhe_swk* const* rlk_b1, const mkhe_swk* const* rlk_d0,
                       const mkhe_swk* const* rlk_v0, const mkhe_swk* crs_u, mkhe_ct* out) {
    MKHE_TRY({ mark(ctx, op0, op1, crs_u, out);
        if (!op0 || !op1 || !out || !crs_u || !rlk_b1 || !rlk_d0 || !rlk_v0) throw Error("mkhe_mul_and_relin: null argument");
        auto h0 = swk_list(ctx, hoist0, op0->c.n); auto h1 = swk_list(ctx, hoist1, op1->c.n);
        auto b1 = swk_list(ctx, rlk_b1, op1->c.n); auto d0 = swk_list(ctx, rlk_d0, op0->c.n); auto v0 = swk_list(ctx, rlk_v0, op0->c.n);
        const bool same = (op0 == op1) && (hoist0 == hoist1);
        need(ctx)->mul_and_relin(op0->c, same ? op0->c : op1->c, hoist0 ? h0.data() : nullptr,
                              hoist1 ? (same ? h0.data() : h1.data()) : nullptr,
                              b1.data(), d0.data(), v0.data(), crs_u->s, out->c);
    })
}
int mkhe_mul_relin_rescale(mkhe_ctx* ctx, const mkhe_ct* op0, const mkhe_ct* op1,
                           const mkhe_swk* const* hoist0, const mkhe_swk* const* hoist1,
                           const mkhe_swk* const* rlk_b1, const mkhe_swk* const* rlk_d0,
                           const mkhe_swk* const* rlk_v0, const mkhe_swk* crs_u, mkhe_ct* out) {
    MKHE_TRY({ mark(ctx, op0, op1, crs_u, out);
        if (!op0 || !op1 || !out || !crs_u || !rlk_b1 || !rlk_d0 || !rlk_v0) throw Error("mkhe_mul_relin_rescale: null argument");
        auto h0 = swk_list(ctx, hoist0, op0->c.n); auto h1 = swk_list(ctx, hoist1, op1->c.n);
        auto b1 = swk_list(ctx, rlk_b1, op1->c.n); auto d0 = swk_list(ctx, rlk_d0, op0->c.n); auto v0 = swk_list(ctx, rlk_v0, op0->c.n);
        const bool same = (op0 == op1) && (hoist0 == hoist1);
        need(ctx)->mul_relin_rescale(op0->c, same ? op0->c : op1->c, hoist0 ? h0.data() : nullptr,
                                     hoist1 ? (same ? h0.data() : h1.data()) : nullptr,
                                     b1.data(), d0.data(), v0.data(), crs_u->s, out->c);
    })
}
int mkhe_mr_partial(mkhe_ctx* ctx, const mkhe_ct* op0, const mkhe_ct* op1,
                    const mkhe_swk* const* hoist0, const mkhe_swk* const* hoist1,
                    const mkhe_swk* const* rlk_b1, const mkhe_swk* const* rlk_d0,
                    int with_c0, mkhe_ct* out, mkhe_swk* x_part, mkhe_swk* y_part) {
    MKHE_TRY({ mark(ctx, op0, op1, out, x_part, y_part);
        if (!op0 || !op1 || !out || !x_part || !y_part || !rlk_b1 || !rlk_d0) throw Error("mkhe_mr_partial: null argument");
        auto h0 = swk_list(ctx, hoist0, op0->c.n); auto h1 = swk_list(ctx, hoist1, op1->c.n);
        auto b1 = swk_list(ctx, rlk_b1, op1->c.n); auto d0 = swk_list(ctx, rlk_d0, op0->c.n);
        need(ctx)->mr_prepare(op0->c, op1->c, hoist0 ? h0.data() : nullptr, hoist1 ? h1.data() : nullptr, with_c0 != 0, out->c);
        need(ctx)->mr_xy(b1.data(), d0.data(), x_part->s.d, y_part->s.d, false);
    })
}
int mkhe_swk_fold(mkhe_ctx* ctx, mkhe_swk* swk, int level, int mform) {
    MKHE_TRY({ mark(ctx, swk); if (!swk) throw Error("mkhe_swk_fold: null argument"); need(ctx)->fold(swk->s.d, true, level, need(ctx)->beta(level), (long)need(ctx)->mtot * need(ctx)->N, mform != 0); })
}
int mkhe_swk_fold_pieces(mkhe_ctx* ctx, const void* pieces, int npieces, long piece_stride_words, long first_limb, long nlimbs, int level, int mform, void* dst) {
    MKHE_TRY({ mark(ctx); need(ctx)->fold_pieces((const u64*)pieces, npieces, piece_stride_words, first_limb, nlimbs, level, mform != 0, (u64*)dst); })
}
int mkhe_mr_finish(mkhe_ctx* ctx, const mkhe_ct* op0, const mkhe_ct* op1, const mkhe_swk* x, const mkhe_swk* y,
                   const mkhe_swk* const* rlk_v0, const mkhe_swk* crs_u, mkhe_ct* out) {
    MKHE_TRY({ mark(ctx, op0, op1, x, y, crs_u, out);
        if (!op0 || !op1 || !x || !y || !rlk_v0 || !crs_u || !out) throw Error("mkhe_mr_finish: null argument");
        auto v0 = swk_list(ctx, rlk_v0, op0->c.n);
        need(ctx)->mr_finish(op0->c, op1->c, x->s.d, y->s.d, v0.data(), crs_u->s, out->c);
    })
}
int mkhe_mr_finish_head(mkhe_ctx* ctx, const mkhe_ct* op0, const mkhe_ct* op1, const mkhe_swk* y, mkhe_ct* out) {
    MKHE_TRY({ mark(ctx, op0, op1, y, out);
        if (!op0 || !op1 || !y || !out) throw Error("mkhe_mr_finish_head: null argument");
        need(ctx)->mr_finish_head(op0->c, op1->c, y->s.d, out->c);
    })
}
int mkhe_mr_finish_tail(mkhe_ctx* ctx, const mkhe_ct* op0, const mkhe_ct* op1, const mkhe_swk* x,
                        const mkhe_swk* const* rlk_v0, const mkhe_swk* crs_u, mkhe_ct* out) {
    MKHE_TRY({ mark(ctx, op0, op1, x, crs_u, out);
        if (!op0 || !op1 || !x || !rlk_v0 || !crs_u || !out) throw Error("mkhe_mr_finish_tail: null argument");
        auto v0 = swk_list(ctx, rlk_v0, op0->c.n);
        need(ctx)->mr_finish_tail(op0->c, op1->c, x->s.d, v0.data(), crs_u->s, out->c);
    })
}
int mkhe_ct_fold(mkhe_ctx* ctx, mkhe_ct* ct) {
    MKHE_TRY({ mark(ctx, ct); if (!ct) throw Error("mkhe_ct_fold: null argument"); need(ctx)->fold(ct->c.d, false, ct->c.limbs - 1, 1 + ct->c.n, (long)ct->c.limbs * need(ctx)->N, false); })
}
int mkhe_rotate(mkhe_ctx* ctx, uint64_t galEl, const mkhe_ct* in, const mkhe_swk* const* hoist,
                const mkhe_swk* const* rk, const mkhe_swk* crs, mkhe_ct* out) {
    MKHE_TRY({ mark(ctx, in, crs, out);
        if (!in || !out || !rk || !crs) throw Error("mkhe_rotate: null argument");
        auto h = swk_list(ctx, hoist, in->c.n); auto r = swk_list(ctx, rk, in->c.n);
        need(ctx)->rotate(galEl, in->c, hoist ? h.data() : nullptr, r.data(), crs->s, out->c);
    })
}
int mkhe_ctx_set_owned(mkhe_ctx* ctx, const int* mod_idx, int n) {
    MKHE_TRY({ if (n < 0 || (n > 0 && !mod_idx)) throw Error("mkhe_ctx_set_owned: bad argument"); need(ctx)->set_owned(mod_idx, n); })
}
int mkhe_lsh_phase(mkhe_ctx* ctx, int phase, const mkhe_ct* op0, const mkhe_ct* op1,
                   const mkhe_swk* const* rlk_b1, const mkhe_swk* const* rlk_d0, const mkhe_swk* const* rlk_v0,
                   const mkhe_swk* crs_u, mkhe_ct* out, void* dev_stage, size_t* words_out) {
    MKHE_TRY({ mark(ctx, op0, op1, crs_u, out);
        if (!op0 || !op1 || !out || !words_out) throw Error("mkhe_lsh_phase: null argument");
        auto b1 = swk_list(ctx, rlk_b1, op1->c.n); auto d0 = swk_list(ctx, rlk_d0, op0->c.n); auto v0 = swk_list(ctx, rlk_v0, op0->c.n);
        *words_out = need(ctx)->lsh_phase(phase, op0->c, op1->c, rlk_b1 ? b1.data() : nullptr, rlk_d0 ? d0.data() : nullptr,
                                       rlk_v0 ? v0.data() : nullptr, crs_u ? &crs_u->s : nullptr, out->c, (u64*)dev_stage);
    })
}
int mkhe_rotate_partial(mkhe_ctx* ctx, const mkhe_ct* in, const mkhe_swk* const* hoist,
                        const mkhe_swk* const* rk, const mkhe_swk* crs, int with_c0, mkhe_ct* out) {
    MKHE_TRY({ mark(ctx, in, crs, out);
        if (!in || !out || !rk || !crs) throw Error("mkhe_rotate_partial: null argument");
        auto h = swk_list(ctx, hoist, in->c.n); auto r = swk_list(ctx, rk, in->c.n);
        need(ctx)->rotate_partial(in->c, hoist ? h.data() : nullptr, r.data(), crs->s, with_c0 != 0, out->c);
    })
}
int mkhe_ct_automorphism(mkhe_ctx* ctx, uint64_t galEl, const mkhe_ct* in, mkhe_ct* out) {
    MKHE_TRY({ mark(ctx, in, out); if (!in || !out) throw Error("mkhe_ct_automorphism: null argument"); need(ctx)->automorphism(galEl, in->c, out->c); })
}
int mkhe_conjugate(mkhe_ctx* ctx, uint64_t galEl, const mkhe_ct* in, const mkhe_swk* const* ck,
                   const mkhe_swk* crs, mkhe_ct* out) {
    MKHE_TRY({ mark(ctx, in, crs, out);
        if (!in || !out || !ck || !crs) throw Error("mkhe_conjugate: null argument");
        auto k = swk_list(ctx, ck, in->c.n);
        need(ctx)->conjugate(galEl, in->c, k.data(), crs->s, out->c);
    })
}
int mkhe_rescale(mkhe_ctx* ctx, const mkhe_ct* in, int nb, mkhe_ct* out) {
    MKHE_TRY({ mark(ctx, in, out); if (!in || !out) throw Error("mkhe_rescale: null argument"); need(ctx)->rescale(in->c, nb, out->c); })
}

int mkhe_ct_add(mkhe_ctx* ctx, const mkhe_ct* op0, const mkhe_ct* op1, mkhe_ct* out) {
    MKHE_TRY({ mark(ctx, op0, op1, out); if (!op0 || !op1 || !out) throw Error("mkhe_ct_add: null argument"); need(ctx)->ct_binary(0, op0->c, op1->c, out->c); })
}
int mkhe_ct_sub(mkhe_ctx* ctx, const mkhe_ct* op0, const mkhe_ct* op1, mkhe_ct* out) {
    MKHE_TRY({ mark(ctx, op0, op1, out); if (!op0 || !op1 || !out) throw Error("mkhe_ct_sub: null argument"); need(ctx)->ct_binary(1, op0->c, op1->c, out->c); })
}
int mkhe_ct_sum(mkhe_ctx* ctx, int n, const mkhe_ct* const* in, mkhe_ct* out) {
    MKHE_TRY({ mark(ctx, out);
        if (n < 1 || !in || !out) throw Error("mkhe_ct_sum: bad argument");
        std::vector<const Ct*> v(n);
        for (int i = 0; i < n; ++i) { if (!in[i]) throw Error("mkhe_ct_sum: null ciphertext"); mark(ctx, in[i]); v[i] = &in[i]->c; }
        need(ctx)->ct_sum(v, out->c);
    })
}
int mkhe_ct_lincomb(mkhe_ctx* ctx, int n, const mkhe_ct* const* in, const void* dev_consts, int nb_rescale, mkhe_ct* out) {
    MKHE_TRY({ mark(ctx, out);
        if (n < 1 || !in || !dev_consts || !out) throw Error("mkhe_ct_lincomb: bad argument");
        std::vector<const Ct*> v(n);
        for (int i = 0; i < n; ++i) { if (!in[i]) throw Error("mkhe_ct_lincomb: null ciphertext"); mark(ctx, in[i]); v[i] = &in[i]->c; }
        need(ctx)->ct_lincomb(v, (const u64*)dev_consts, nb_rescale, out->c);
    })
}
int mkhe_ct_mul_const(mkhe_ctx* ctx, const mkhe_ct* in, const uint64_t* c_first, const uint64_t* c_second, mkhe_ct* out) {
    MKHE_TRY({ mark(ctx, in, out); if (!in || !out || !c_first || !c_second) throw Error("mkhe_ct_mul_const: null argument"); need(ctx)->ct_mul_const(in->c, c_first, c_second, out->c); })
}
int mkhe_ct_mul_ptxt(mkhe_ctx* ctx, const mkhe_ct* in, const void* dev_pt, mkhe_ct* out) {
    MKHE_TRY({ mark(ctx, in, out); if (!in || !out || !dev_pt) throw Error("mkhe_ct_mul_ptxt: null argument"); need(ctx)->ct_mul_ptxt(in->c, (const u64*)dev_pt, out->c); })
}

// ---- B operations of one shape per call (batch.hip)
static std::vector<const Ct*> ct_list(const mkhe_ctx* ctx, const mkhe_ct* const* v, int n, const char* what) {
    if (!v) throw Error(std::string(what) + ": null ciphertext list");
    std::vector<const Ct*> r(n);
    for (int i = 0; i < n; ++i) { r[i] = &ct_at(v, i, what); mark(ctx, v[i]); }
    return r;
}
static std::vector<Ct*> ct_list_out(const mkhe_ctx* ctx, mkhe_ct* const* v, int n, const char* what) {
    if (!v) throw Error(std::string(what) + ": null output list");
    std::vector<Ct*> r(n);
    for (int i = 0; i < n; ++i) {
        if (!v[i]) throw Error(std::string(what) + ": null output in the batch");
        for (int k = 0; k < i; ++k) if (v[k] == v[i]) throw Error(std::string(what) + ": the outputs of a batch must be distinct");
        mark(ctx, v[i]); r[i] = &v[i]->c;
    }
    return r;
}
static std::vector<const Swk*> swk_flat(const mkhe_ctx* ctx, const mkhe_swk* const* v, size_t n) {
    std::vector<const Swk*> r;
    if (!v) return r;
    r.resize(n);
    for (size_t i = 0; i < n; ++i) { if (!v[i]) throw Error("mkhe: null hoisted form in a batch"); mark(ctx, v[i]); r[i] = &v[i]->s; }
    return r;
}
// nout sums of mkhe_ct_lincomb from the same inputs (engine_ops.hip); the counts first, then the context.  Nothing is allocated or uploaded: legal
// inside a capture, like mkhe_ct_lincomb
int mkhe_ct_lincomb_multi(mkhe_ctx* ctx, int nin, const mkhe_ct* const* in, int nout, const void* dev_consts, int nb_rescale, mkhe_ct* const* out) {
    MKHE_TRY({
        const char* what = "mkhe_ct_lincomb_multi";
        const std::string w = std::string(what) + ": ";
        if (nin < 1 || nin > CTLM_MAX_IN) throw Error(w + "nin must be 1 .. " + std::to_string(CTLM_MAX_IN));
        if (nout < 1 || nout > CTLM_MAX_OUT) throw Error(w + "nout must be 1 .. " + std::to_string(CTLM_MAX_OUT));
        if (nb_rescale != 0 && nb_rescale != 1) throw Error(w + "nb_rescale must be 0 or 1");
        Context* c = enter(ctx, what);
        if (!in || !dev_consts || !out) throw Error(w + "null argument");
        scheme_ok(c, what, false, ": needs a CKKS or mkrlwe context (mkhe_bfv_ct_lincomb is the BFV call)");
        unmasked(c, what);
        for (int i = 0; i < nin; ++i) ct_at(in, i, what);
        for (int i = 0; i < nout; ++i) if (!out[i]) throw Error(w + "null output in the batch");
        commit(c);
        auto i = ct_list(ctx, in, nin, what);
        auto o = ct_list_out(ctx, out, nout, what);
        c->ct_lincomb_multi(what, i, (const u64*)dev_consts, nb_rescale, o);
    })
}
// mkhe_ct_lincomb_multi on nbatch items that share the constants (engine_ops.hip); the counts first, then the context.  Nothing is allocated or uploaded
// on the device: legal inside a capture.  (Distinct outputs are the engine's check, by address: the handle lists may be long.)
int mkhe_ct_lincomb_batch(mkhe_ctx* ctx, int nbatch, int nin, const mkhe_ct* const* in, int nout, const void* dev_consts, int nb_rescale, mkhe_ct* const* out) {
    MKHE_TRY({
        const char* what = "mkhe_ct_lincomb_batch";
        const std::string w = std::string(what) + ": ";
        if (nbatch < 1) throw Error(w + "nbatch must be at least 1");
        if (nin < 1 || nin > CTLM_MAX_IN) throw Error(w + "nin must be 1 .. " + std::to_string(CTLM_MAX_IN));
        if (nout < 1 || nout > CTLM_MAX_OUT) throw Error(w + "nout must be 1 .. " + std::to_string(CTLM_MAX_OUT));
        if (nb_rescale != 0 && nb_rescale != 1) throw Error(w + "nb_rescale must be 0 or 1");
        Context* c = enter(ctx, what);
        if (!in || !dev_consts || !out) throw Error(w + "null argument");
        scheme_ok(c, what, false, ": needs a CKKS or mkrlwe context (mkhe_bfv_ct_lincomb is the BFV call)");
        unmasked(c, what);
        const size_t ni = (size_t)nbatch * nin;
        const size_t no = (size_t)nbatch * nout;
        for (size_t i = 0; i < ni; ++i) if (!in[i]) throw Error(w + "null ciphertext in the batch");
        for (size_t i = 0; i < no; ++i) if (!out[i]) throw Error(w + "null output in the batch");
        commit(c);
        std::vector<const Ct*> vi(ni);
        std::vector<Ct*> vo(no);
        for (size_t i = 0; i < ni; ++i) { mark(ctx, in[i]); vi[i] = &in[i]->c; }
        for (size_t i = 0; i < no; ++i) { mark(ctx, out[i]); vo[i] = &out[i]->c; }
        c->ct_lincomb_batch(what, vi, nin, (const u64*)dev_consts, nb_rescale, vo, nout);
    })
}
int mkhe_hoisted_form_batch(mkhe_ctx* ctx, int level, int nbatch, const mkhe_ct* const* cts, mkhe_swk* const* out) {
    MKHE_TRY({
        if (nbatch < 1) throw Error("mkhe_hoisted_form_batch: empty batch");
        auto c = ct_list(ctx, cts, nbatch, "mkhe_hoisted_form_batch");
        const size_t n = (size_t)nbatch * c[0]->n;
        if (n && !out) throw Error("mkhe_hoisted_form_batch: null argument");
        std::vector<Swk*> o(n);
        for (size_t i = 0; i < n; ++i) { if (!out[i]) throw Error("mkhe_hoisted_form_batch: null output handle"); mark(ctx, out[i]); o[i] = &out[i]->s; }
        need(ctx)->hoisted_form_batch(level, c, o);
    })
}
int mkhe_rotate_batch(mkhe_ctx* ctx, uint64_t galEl, int nbatch, const mkhe_ct* const* in, const mkhe_swk* const* hoist,
                      const mkhe_swk* const* rk, const mkhe_swk* crs, mkhe_ct* const* out) {
    MKHE_TRY({ mark(ctx, crs);
        if (nbatch < 1 || !rk || !crs) throw Error("mkhe_rotate_batch: bad argument");
        auto i = ct_list(ctx, in, nbatch, "mkhe_rotate_batch");
        auto o = ct_list_out(ctx, out, nbatch, "mkhe_rotate_batch");
        auto h = swk_flat(ctx, hoist, (size_t)nbatch * i[0]->n);
        auto k = swk_list(ctx, rk, i[0]->n);
        need(ctx)->rotate_batch(galEl, i, h, k.data(), crs->s, o);
    })
}
int mkhe_rotate_multi(mkhe_ctx* ctx, int nbatch, const uint64_t* galEl, const mkhe_ct* const* in, const mkhe_swk* const* hoist,
                      const mkhe_swk* const* rk, const mkhe_swk* const* crs, const mkhe_ct* const* post_add, mkhe_ct* const* out) {
    MKHE_TRY({
        if (nbatch < 1 || !galEl || !rk || !crs) throw Error("mkhe_rotate_multi: bad argument");
        auto i = ct_list(ctx, in, nbatch, "mkhe_rotate_multi");
        auto o = ct_list_out(ctx, out, nbatch, "mkhe_rotate_multi");
        auto h = swk_flat(ctx, hoist, (size_t)nbatch * i[0]->n);
        auto k = swk_flat(ctx, rk, (size_t)nbatch * i[0]->n);
        auto c = swk_flat(ctx, crs, (size_t)nbatch);
        std::vector<const Ct*> p;
        if (post_add) p = ct_list(ctx, post_add, nbatch, "mkhe_rotate_multi");
        need(ctx)->rotate_multi(std::vector<u64>(galEl, galEl + nbatch), i, h, k, c, p, o);
    })
}
int mkhe_mul_relin_batch(mkhe_ctx* ctx, int nbatch, const mkhe_ct* const* op0, const mkhe_ct* const* op1,
                         const mkhe_swk* const* hoist0, const mkhe_swk* const* hoist1,
                         const mkhe_swk* const* rlk_b1, const mkhe_swk* const* rlk_d0, const mkhe_swk* const* rlk_v0,
                         const mkhe_swk* crs_u, int rescale, mkhe_ct* const* out) {
    MKHE_TRY({ mark(ctx, crs_u);
        if (nbatch < 1 || !crs_u || !rlk_b1 || !rlk_d0 || !rlk_v0) throw Error("mkhe_mul_relin_batch: bad argument");
        auto a = ct_list(ctx, op0, nbatch, "mkhe_mul_relin_batch");
        auto b = ct_list(ctx, op1, nbatch, "mkhe_mul_relin_batch");
        auto o = ct_list_out(ctx, out, nbatch, "mkhe_mul_relin_batch");
        auto h0 = swk_flat(ctx, hoist0, (size_t)nbatch * a[0]->n); auto h1 = swk_flat(ctx, hoist1, (size_t)nbatch * b[0]->n);
        auto b1 = swk_list(ctx, rlk_b1, b[0]->n); auto d0 = swk_list(ctx, rlk_d0, a[0]->n); auto v0 = swk_list(ctx, rlk_v0, a[0]->n);
        need(ctx)->mul_relin_batch(a, b, h0, h1, b1.data(), d0.data(), v0.data(), crs_u->s, rescale != 0, o);
    })
}
// (a function of its own: the commas of its declarations would split the argument of MKHE_TRY)
static void mul_relin_sum_body(mkhe_ctx* ctx, int K, const mkhe_ct* const* op0, const mkhe_ct* const* op1,
                               const mkhe_swk* const* hoist0, const mkhe_swk* const* hoist1,
                               const mkhe_swk* const* rlk_b1, const mkhe_swk* const* rlk_d0, const mkhe_swk* const* rlk_v0,
                               const mkhe_swk* crs_u, int rescale, mkhe_ct* out) {
    const std::string what = "mkhe_mul_relin_sum";
    try {
        if (!ctx) throw Error(what + ": null context");
        if (K < 1 || K > TSUM_MAX_K) throw Error(what + ": takes 1 to " + std::to_string(TSUM_MAX_K) + " pairs");      // (before the lists are read)
        if (!out || !crs_u || !rlk_b1 || !rlk_d0 || !rlk_v0) throw Error(what + ": null argument");
        if (rescale != 0 && rescale != 1) throw Error(what + ": rescale is 0 or 1");
        auto a = ct_list(ctx, op0, K, what.c_str());
        auto b = ct_list(ctx, op1, K, what.c_str());
        const int n0 = a[0]->n;           // (that every pair carries these ids, and that out is none of the operands, is the engine's check)
        const int n1 = b[0]->n;
        auto keys = [&](const mkhe_swk* const* v, size_t n, const char* name) {
            std::vector<const Swk*> r(n);
            for (size_t i = 0; i < n; ++i) { if (!v[i]) throw Error(what + ": null handle in " + name); mark(ctx, v[i]); r[i] = &v[i]->s; }
            return r;
        };
        std::vector<const Swk*> h0;
        std::vector<const Swk*> h1;
        if (hoist0) h0 = keys(hoist0, (size_t)K * n0, "hoist0");
        if (hoist1) h1 = keys(hoist1, (size_t)K * n1, "hoist1");
        auto b1 = keys(rlk_b1, n1, "rlk_b1");
        auto d0 = keys(rlk_d0, n0, "rlk_d0");
        auto v0 = keys(rlk_v0, n0, "rlk_v0");
        need(ctx)->mul_relin_sum(a, b, h0, h1, b1.data(), d0.data(), v0.data(), crs_u->s, rescale != 0, out->c);
    } catch (const std::exception& e) {
        // every message of this entry point starts with its name, whichever layer raised it
        const std::string m = e.what();
        if (m.compare(0, what.size(), what) == 0) throw;
        throw Error(what + ": " + m);
    }
}
int mkhe_mul_relin_sum(mkhe_ctx* ctx, int K, const mkhe_ct* const* op0, const mkhe_ct* const* op1,
                       const mkhe_swk* const* hoist0, const mkhe_swk* const* hoist1,
                       const mkhe_swk* const* rlk_b1, const mkhe_swk* const* rlk_d0, const mkhe_swk* const* rlk_v0,
                       const mkhe_swk* crs_u, int rescale, mkhe_ct* out) {
    MKHE_TRY({ mark(ctx, crs_u, out); mul_relin_sum_body(ctx, K, op0, op1, hoist0, hoist1, rlk_b1, rlk_d0, rlk_v0, crs_u, rescale, out); })
}
int mkhe_ct_mul_ptxt_batch(mkhe_ctx* ctx, int nbatch, const mkhe_ct* const* in, const void* dev_pt, int nb_rescale, mkhe_ct* const* out) {
    MKHE_TRY({
        if (nbatch < 1 || !dev_pt) throw Error("mkhe_ct_mul_ptxt_batch: bad argument");
        auto i = ct_list(ctx, in, nbatch, "mkhe_ct_mul_ptxt_batch");
        auto o = ct_list_out(ctx, out, nbatch, "mkhe_ct_mul_ptxt_batch");
        need(ctx)->ct_mul_ptxt_batch(i, (const u64*)dev_pt, nb_rescale, o);
    })
}
int mkhe_ptxt_prepare(mkhe_ctx* ctx, int limbs, int count, const void* dev_pt, void* dev_ptntt) {
    MKHE_TRY({ if (!ctx) throw Error("mkhe_ptxt_prepare: null context"); need(ctx)->ptxt_prepare(limbs, count, (const u64*)dev_pt, (u64*)dev_ptntt); })
}
int mkhe_ct_ptxt_dot(mkhe_ctx* ctx, int nin, const mkhe_ct* const* in, int ngiant, const uint32_t* masks, const void* dev_ptntt, int pt_limbs,
                     mkhe_ct* const* out) {
    MKHE_TRY({
        const char* what = "mkhe_ct_ptxt_dot";
        const std::string w = std::string(what) + ": ";
        if (!ctx) throw Error(w + "null context");
        if (nin < 1 || nin > CTDOT_MAX_IN) throw Error(w + "takes 1 to " + std::to_string(CTDOT_MAX_IN) + " input ciphertexts");
        if (ngiant < 1 || ngiant > CTDOT_MAX_GIANT) throw Error(w + "takes 1 to " + std::to_string(CTDOT_MAX_GIANT) + " outputs");
        if (!masks || !dev_ptntt) throw Error(w + "null argument");
        auto i = ct_list(ctx, in, nin, what);
        auto o = ct_list_out(ctx, out, ngiant, what);
        Context* c = need(ctx);
        scheme_ok(c, what, false, ": needs a CKKS context");
        unmasked(c, what);
        // the outputs set the level; inputs and plaintexts may sit above it (the call may be captured: nothing here allocates, stages or synchronises)
        const int L = o[0]->limbs;
        if (L < 1 || L > c->nq) throw Error(w + "the outputs' limb count lies outside the moduli of Q");
        if (pt_limbs < L) throw Error(w + "the prepared plaintexts have fewer limbs than the outputs");
        c->ct_ptxt_dot(what, 1, i, std::vector<unsigned int>(masks, masks + ngiant), (const u64*)dev_ptntt, (long)pt_limbs * c->N, L, o);
    })
}
int mkhe_ct_binary_batch(mkhe_ctx* ctx, int op, int nbatch, const mkhe_ct* const* op0, const mkhe_ct* const* op1, mkhe_ct* const* out) {
    MKHE_TRY({
        if (nbatch < 1 || (op != 0 && op != 1)) throw Error("mkhe_ct_binary_batch: bad argument");
        auto a = ct_list(ctx, op0, nbatch, "mkhe_ct_binary_batch");
        auto b = ct_list(ctx, op1, nbatch, "mkhe_ct_binary_batch");
        auto o = ct_list_out(ctx, out, nbatch, "mkhe_ct_binary_batch");
        need(ctx)->ct_binary_batch(op, a, b, o);
    })
}

// ---- key generation / CRS expansion
int mkhe_keygen_secret(mkhe_ctx* ctx, const int32_t* s, void* dev_sk) {
    MKHE_TRY({ if (!s || !dev_sk) throw Error("mkhe_keygen_secret: null argument"); need(ctx)->keygen_secret(s, (u64*)dev_sk); })
}
int mkhe_keygen_switching_key(mkhe_ctx* ctx, const void* dev_sk, const int32_t* e, mkhe_swk* out) {
    MKHE_TRY({ mark(ctx, out); if (!dev_sk || !e || !out) throw Error("mkhe_keygen_switching_key: null argument"); need(ctx)->keygen_switching_key((const u64*)dev_sk, e, out->s.d); })
}
int mkhe_keygen_public_key(mkhe_ctx* ctx, const void* dev_sk, const int32_t* e, const mkhe_swk* crs_a, void* dev_pk) {
    MKHE_TRY({ mark(ctx, crs_a); if (!dev_sk || !e || !crs_a || !dev_pk) throw Error("mkhe_keygen_public_key: null argument"); need(ctx)->keygen_public_key((const u64*)dev_sk, e, crs_a->s.d, (u64*)dev_pk); })
}
int mkhe_keygen_relin_key(mkhe_ctx* ctx, const void* dev_sk, const void* dev_r, const int32_t* e,
                          const mkhe_swk* crs_a, const mkhe_swk* crs_u, mkhe_swk* b, mkhe_swk* d, mkhe_swk* v) {
    MKHE_TRY({ mark(ctx, crs_a, crs_u, b, d, v);
        if (!dev_sk || !dev_r || !e || !crs_a || !crs_u || !b || !d || !v) throw Error("mkhe_keygen_relin_key: null argument");
        need(ctx)->keygen_relin_key((const u64*)dev_sk, (const u64*)dev_r, e, crs_a->s.d, crs_u->s.d, b->s.d, d->s.d, v->s.d);
    })
}
int mkhe_keygen_rotation_key(mkhe_ctx* ctx, uint64_t galEl, const void* dev_sk, const int32_t* e, const mkhe_swk* crs, mkhe_swk* out) {
    MKHE_TRY({ mark(ctx, crs, out); if (!dev_sk || !e || !crs || !out) throw Error("mkhe_keygen_rotation_key: null argument"); need(ctx)->keygen_rotation_key(galEl, (const u64*)dev_sk, e, crs->s.d, out->s.d); })
}
int mkhe_keygen_conjugation_key(mkhe_ctx* ctx, const void* dev_sk, const int32_t* e, const mkhe_swk* crs, mkhe_swk* out) {
    MKHE_TRY({ mark(ctx, crs, out); if (!dev_sk || !e || !crs || !out) throw Error("mkhe_keygen_conjugation_key: null argument"); need(ctx)->keygen_conjugation_key((const u64*)dev_sk, e, crs->s.d, out->s.d); })
}
int mkhe_bfv_keygen_switching_key(mkhe_ctx* ctx, const void* dev_sk, const uint64_t* g, const int32_t* e, mkhe_swk* out) {
    MKHE_TRY({ mark(ctx, out); if (!dev_sk || !g || !e || !out) throw Error("mkhe_bfv_keygen_switching_key: null argument"); need(ctx)->bfv_keygen_switching_key((const u64*)dev_sk, g, e, out->s.d); })
}
int mkhe_bfv_keygen_relin_key(mkhe_ctx* ctx, const void* dev_sk, const void* dev_r, const uint64_t* g1, const uint64_t* g2,
                              const int32_t* e, const mkhe_swk* a1, const mkhe_swk* a2, const mkhe_swk* u,
                              mkhe_swk* b1, mkhe_swk* b2, mkhe_swk* d1, mkhe_swk* d2, mkhe_swk* v) {
    MKHE_TRY({ mark(ctx, a1, a2, u, b1, b2, d1, d2, v);
        if (!dev_sk || !dev_r || !g1 || !g2 || !e || !a1 || !a2 || !u || !b1 || !b2 || !d1 || !d2 || !v) throw Error("mkhe_bfv_keygen_relin_key: null argument");
        need(ctx)->bfv_keygen_relin_key((const u64*)dev_sk, (const u64*)dev_r, g1, g2, e, a1->s.d, a2->s.d, u->s.d,
                                     b1->s.d, b2->s.d, d1->s.d, d2->s.d, v->s.d);
    })
}
int mkhe_crs_expand(mkhe_ctx* ctx, uint64_t seed, int32_t idx, mkhe_swk* out) {
    MKHE_TRY({ mark(ctx, out); if (!out) throw Error("mkhe_crs_expand: null argument"); need(ctx)->crs_expand(seed, idx, out->s.d); })
}

// ---- public-key encryption / decryption (encdec.hip)
// the outputs of an encryption: present, distinct, each over exactly one party, with `limbs` limbs or (limbs = 0) all at one level
static std::vector<u64*> fresh_outputs(mkhe_ctx* ctx, const char* what, int count, int limbs, mkhe_ct* const* out) {
    auto o = ct_list_out(ctx, out, count, what);
    std::vector<u64*> d(count);
    for (int b = 0; b < count; ++b) {
        if (o[b]->n != 1) throw Error(std::string(what) + ": every out must be a ciphertext over exactly one party");
        if (o[b]->limbs != (limbs ? limbs : o[0]->limbs)) throw Error(std::string(what) + (limbs ? ": every out must have level+1 limbs" : ": every out must be at the same level"));
        for (int k = 0; k < b; ++k) if (d[k] == o[b]->d) throw Error(std::string(what) + ": the outputs of a batch must be distinct");
        d[b] = o[b]->d;
    }
    return d;
}
int mkhe_encrypt(mkhe_ctx* ctx, int level, int count, const void* dev_pk, const void* dev_pt, int pt_is_ntt, const int32_t* samples, mkhe_ct* const* out) {
    MKHE_TRY({
        Context* c = need(ctx);
        if (!dev_pk || !dev_pt || !samples || !out) throw Error("mkhe_encrypt: null argument");
        if (level < 0 || level >= c->nq) throw Error("mkhe_encrypt: level out of range");
        count_ok("mkhe_encrypt", count);
        need_aligned(dev_pk, "mkhe_encrypt"); need_aligned(dev_pt, "mkhe_encrypt");
        auto d = fresh_outputs(ctx, "mkhe_encrypt", count, level + 1, out);
        c->encrypt(level, count, (const u64*)dev_pk, (const u64*)dev_pt, pt_is_ntt != 0, samples, d.data());
    })
}
// device-side sampling from a SECRET key: refused inside a capture, armed before the arguments are looked at
static void smp_table_ok(const char* what, const uint64_t* cdt, int ncdt) {
    if (!cdt) throw Error(std::string(what) + ": null table");
    if (ncdt < 2 || ncdt > SMP_MAX_CDT || (ncdt & 1)) throw Error(std::string(what) + ": ncdt must be even and 2 .. 64");
    for (int t = 1; t < ncdt; ++t) if (cdt[t] <= cdt[t - 1]) throw Error(std::string(what) + ": the thresholds of the table must be strictly increasing");
}
static Context* smp_enter(mkhe_ctx* ctx, const char* what, const uint32_t* key, bool table, const uint64_t* cdt, int ncdt) {
    Context* c = enter(ctx, what);
    if (!key) throw Error(std::string(what) + ": null key");
    if (table) smp_table_ok(what, cdt, ncdt);
    unmasked(c, what);
    not_captured(c, what, REPLAYS);
    commit(c);
    return c;
}
int mkhe_sample_small(mkhe_ctx* ctx, int kind, int count, const uint32_t key[8], uint64_t nonce, uint32_t first_stream, const uint64_t* cdt, int ncdt,
                      void* dev_out) {
    MKHE_TRY({
        if (kind != 0 && kind != 1) throw Error("mkhe_sample_small: kind must be 0 (ternary) or 1 (table)");
        Context* c = smp_enter(ctx, "mkhe_sample_small", key, kind == 1, cdt, ncdt);
        if (!dev_out) throw Error("mkhe_sample_small: null output");
        if (count < 1 || count > 3 * 65535) throw Error("mkhe_sample_small: count must be 1 .. 196605");
        if ((uint64_t)first_stream + (uint64_t)count > (1ull << 32)) throw Error("mkhe_sample_small: first_stream + count exceeds 2^32");
        need_aligned(dev_out, "mkhe_sample_small");
        c->sample_small(kind, count, key, nonce, first_stream, cdt, ncdt, (int32_t*)dev_out);
    })
}
int mkhe_encrypt_seeded(mkhe_ctx* ctx, int level, int count, const void* dev_pk, const void* dev_pt, int pt_is_ntt, const uint32_t key[8], uint64_t nonce,
                        const uint64_t* cdt, int ncdt, mkhe_ct* const* out) {
    MKHE_TRY({
        Context* c = smp_enter(ctx, "mkhe_encrypt_seeded", key, true, cdt, ncdt);
        if (!dev_pk || !dev_pt || !out) throw Error("mkhe_encrypt_seeded: null argument");
        if (level < 0 || level >= c->nq) throw Error("mkhe_encrypt_seeded: level out of range");
        count_ok("mkhe_encrypt_seeded", count);
        need_aligned(dev_pk, "mkhe_encrypt_seeded"); need_aligned(dev_pt, "mkhe_encrypt_seeded");
        auto d = fresh_outputs(ctx, "mkhe_encrypt_seeded", count, level + 1, out);
        c->encrypt_seeded(level, count, (const u64*)dev_pk, (const u64*)dev_pt, pt_is_ntt != 0, key, nonce, cdt, ncdt, d.data());
    })
}
// secret-key encryption with a seeded c1.  The two encrypt calls are under the rules of the seeded encryption (smp_enter); the sampler and the
// expansion read a PUBLIC stream and may be captured as long as they stage no pointer table (count at most 16).
static Context* sku_enter(mkhe_ctx* ctx, const char* what, int count, const uint32_t* key) {
    Context* c = enter(ctx, what);
    if (!key) throw Error(std::string(what) + ": null key");
    count_ok(what, count);
    unmasked(c, what);
    if (count > ED_INLINE) not_captured(c, what, "with more than 16 items (the pointer table is staged)");
    return c;
}
int mkhe_sample_uniform(mkhe_ctx* ctx, int limbs, int count, const uint32_t a_key[8], uint64_t a_nonce, void* dev_out) {
    MKHE_TRY({
        const char* what = "mkhe_sample_uniform";
        Context* c = sku_enter(ctx, what, count, a_key);
        if (!dev_out) throw Error("mkhe_sample_uniform: null output");
        if (limbs < 1 || limbs > c->nq) throw Error("mkhe_sample_uniform: limbs must be 1 .. nQ");
        need_aligned(dev_out, what);
        commit(c);
        c->sample_uniform(limbs, count, a_key, a_nonce, (u64*)dev_out);
    })
}
int mkhe_ct_expand_seeded(mkhe_ctx* ctx, int count, const uint32_t a_key[8], uint64_t a_nonce, mkhe_ct* const* out) {
    MKHE_TRY({
        const char* what = "mkhe_ct_expand_seeded";
        Context* c = sku_enter(ctx, what, count, a_key);
        if (!out) throw Error("mkhe_ct_expand_seeded: null argument");
        auto d = fresh_outputs(ctx, what, count, 0, out);
        commit(c);
        c->ct_expand_seeded(count, out[0]->c.limbs, a_key, a_nonce, d.data());
    })
}
static void sk_encrypt_args_ok(Context* c, const char* what, int level, int count, const void* dev_sk, const void* dev_pt, const uint32_t* a_key, mkhe_ct* const* out) {
    if (!dev_sk || !dev_pt || !a_key || !out) throw Error(std::string(what) + ": null argument");
    if (level < 0 || level >= c->nq) throw Error(std::string(what) + ": level out of range");
    count_ok(what, count);
    need_aligned(dev_sk, what); need_aligned(dev_pt, what);
}
int mkhe_encrypt_sk(mkhe_ctx* ctx, int level, int count, const void* dev_sk, const void* dev_pt, int pt_is_ntt, const uint32_t a_key[8], uint64_t a_nonce,
                    const int32_t* e, mkhe_ct* const* out) {
    MKHE_TRY({
        const char* what = "mkhe_encrypt_sk";
        Context* c = smp_enter(ctx, what, a_key, false, nullptr, 0);
        if (!e) throw Error("mkhe_encrypt_sk: null argument");
        sk_encrypt_args_ok(c, what, level, count, dev_sk, dev_pt, a_key, out);
        auto d = fresh_outputs(ctx, what, count, level + 1, out);
        c->encrypt_sk(level, count, (const u64*)dev_sk, (const u64*)dev_pt, pt_is_ntt != 0, a_key, a_nonce, e, nullptr, 0, nullptr, 0, d.data(), what);
    })
}
int mkhe_encrypt_sk_seeded(mkhe_ctx* ctx, int level, int count, const void* dev_sk, const void* dev_pt, int pt_is_ntt, const uint32_t a_key[8],
                           uint64_t a_nonce, const uint32_t e_key[8], uint64_t e_nonce, const uint64_t* cdt, int ncdt, mkhe_ct* const* out) {
    MKHE_TRY({
        const char* what = "mkhe_encrypt_sk_seeded";
        Context* c = smp_enter(ctx, what, e_key, true, cdt, ncdt);
        sk_encrypt_args_ok(c, what, level, count, dev_sk, dev_pt, a_key, out);
        bool same = true;
        for (int i = 0; i < 8; ++i) same = same && a_key[i] == e_key[i];
        if (same) throw Error("mkhe_encrypt_sk_seeded: a_key must differ from e_key (the public seed would publish the key of the secret stream)");
        auto d = fresh_outputs(ctx, what, count, level + 1, out);
        c->encrypt_sk(level, count, (const u64*)dev_sk, (const u64*)dev_pt, pt_is_ntt != 0, a_key, a_nonce, nullptr, e_key, e_nonce, cdt, ncdt, d.data(), what);
    })
}
int mkhe_partial_decrypt(mkhe_ctx* ctx, const mkhe_ct* in, int slot, const void* dev_sk, mkhe_ct* out) {
    MKHE_TRY({ mark(ctx, in, out);
        if (!in || !dev_sk || !out) throw Error("mkhe_partial_decrypt: null argument");
        need_aligned(dev_sk, "mkhe_partial_decrypt");
        need(ctx)->partial_decrypt(in->c, slot, (const u64*)dev_sk, out->c);
    })
}
int mkhe_decrypt(mkhe_ctx* ctx, const mkhe_ct* ct, const void* const* dev_sk, void* dev_pt_out) {
    MKHE_TRY({ mark(ctx, ct);
        if (!ct || !dev_pt_out || (ct->c.n > 0 && !dev_sk)) throw Error("mkhe_decrypt: null argument");
        need_aligned(dev_pt_out, "mkhe_decrypt");
        std::vector<const u64*> sk(ct->c.n);
        for (int i = 0; i < ct->c.n; ++i) {
            if (!dev_sk[i]) throw Error("mkhe_decrypt: null secret key in the per-party list");
            need_aligned(dev_sk[i], "mkhe_decrypt");
            sk[i] = (const u64*)dev_sk[i];
        }
        if (ct->c.n > ED_INLINE) not_captured(enter(ctx, nullptr), "mkhe_decrypt", "on a ciphertext over more than 16 parties (the pointer tables are staged)");
        need(ctx)->decrypt(ct->c, sk.data(), (u64*)dev_pt_out);
    })
}
// distributed decryption: a share with a flood draws from the keystream and is refused inside a capture; without one the share, and the merge, may be
// captured as long as they stage no table (count and nshares at most 16)
static Context* ds_enter(mkhe_ctx* ctx, const char* what, int count, const mkhe_ct* const* in, const void* out, bool keystream) {
    Context* c = enter(ctx, what);
    count_ok(what, count);
    if (!in || !out) throw Error(std::string(what) + ": null argument");
    need_aligned(out, what);
    batch_ok(what, count, in);
    unmasked(c, what);
    if (keystream) not_captured(c, what, REPLAYS);
    else if (count > ED_INLINE) not_captured(c, what, STAGES);
    return c;
}
int mkhe_decrypt_share(mkhe_ctx* ctx, int count, const mkhe_ct* const* in, const int* slots, const void* dev_sk, const uint32_t key[8], uint64_t nonce,
                       int flood_bits, void* dev_shares) {
    MKHE_TRY({
        if (flood_bits < 0 || flood_bits > SHF_MAX_BITS) throw Error("mkhe_decrypt_share: flood_bits must be 0 .. 62");
        if (flood_bits > 0 && !key) throw Error("mkhe_decrypt_share: null key");
        Context* c = ds_enter(ctx, "mkhe_decrypt_share", count, in, dev_shares, flood_bits > 0);
        if (!slots || !dev_sk) throw Error("mkhe_decrypt_share: null argument");
        need_aligned(dev_sk, "mkhe_decrypt_share");
        slots_ok("mkhe_decrypt_share", count, in, slots);
        commit(c);
        auto i = ct_list(ctx, in, count, "mkhe_decrypt_share");
        c->decrypt_share(i, slots, (const u64*)dev_sk, key, nonce, flood_bits, (u64*)dev_shares);
    })
}
int mkhe_decrypt_merge(mkhe_ctx* ctx, int count, const mkhe_ct* const* in, int nshares, const void* const* dev_shares, void* dev_pt_out) {
    MKHE_TRY({
        Context* c = ds_enter(ctx, "mkhe_decrypt_merge", count, in, dev_pt_out, false);
        merge_shape("mkhe_decrypt_merge", count, in, nshares);
        if (nshares > 0 && !dev_shares) throw Error("mkhe_decrypt_merge: null argument");
        auto sh = share_list(dev_shares, nshares, "mkhe_decrypt_merge");
        if (nshares > ED_INLINE) not_captured(c, "mkhe_decrypt_merge", STAGES);
        commit(c);
        auto i = ct_list(ctx, in, count, "mkhe_decrypt_merge");
        c->decrypt_merge(i, sh, (u64*)dev_pt_out);
    })
}
// noise measurement: the scalars that need no context first, then the guard of the protocol family; the tables (and, kind 1, the encoder's
// preconditions on T) behind the last refusal that needs no device
int mkhe_noise_norm(mkhe_ctx* ctx, int kind, int limbs, int count, const void* dev_phase, const void* dev_ref, long ref_stride_words, void* dev_out) {
    MKHE_TRY({
        const char* what = "mkhe_noise_norm";
        const std::string w(what);
        if (kind != 0 && kind != 1) throw Error(w + ": kind must be 0 (residual) or 1 (BFV invariant)");
        count_ok(what, count);
        if (limbs < 1) throw Error(w + ": limbs out of range");
        if (kind == 1 && dev_ref) throw Error(w + ": kind 1 takes no reference (dev_ref must be NULL)");
        Context* c = enter(ctx, what);
        if (!dev_phase || !dev_out) throw Error(w + ": null argument");
        need_aligned(dev_phase, what); need_aligned(dev_ref, what); need_aligned(dev_out, what);
        if (limbs > c->nq) throw Error(w + ": limbs out of range");
        if (ref_stride_words != 0 && ref_stride_words != (long)limbs * c->N) throw Error(w + ": ref_stride_words must be 0 (one reference for all) or limbs * N");
        if (kind == 1) {
            scheme_ok(c, what, true, ": kind 1 (BFV invariant) needs a BFV context");
            if (limbs != c->nq) throw Error(w + ": kind 1 takes the nQ limbs of the context");
        }
        unmasked(c, what);
        not_captured(c, what, UPLOADS);
        commit(c, [&] { c->noise_norm_prepare(kind); });
        c->noise_norm(kind, limbs, count, (const u64*)dev_phase, (const u64*)dev_ref, ref_stride_words, (u64*)dev_out);
    })
}
// raising the modulus: every refusal before the launch, under the guard of the protocol family; one launch without table or scratch, so a capture holds it
int mkhe_ct_mod_raise(mkhe_ctx* ctx, const mkhe_ct* in, mkhe_ct* out) {
    MKHE_TRY({
        const char* what = "mkhe_ct_mod_raise";
        const std::string w(what);
        Context* c = enter(ctx, what);
        if (!in || !out) throw Error(w + ": null argument");
        scheme_ok(c, what, false, ": not available on a BFV context (its ciphertexts live at one level)");
        unmasked(c, what);
        if (in == out || in->c.d == out->c.d) throw Error(w + ": out must not alias in");
        if (in->c.limbs != 1) throw Error(w + ": in must be at level 0");
        if (out->c.limbs < 2) throw Error(w + ": out must be above level 0");
        if (out->c.limbs > c->nq) throw Error(w + ": out has more limbs than the context has moduli");
        if (in->c.n != out->c.n || in->c.ids != out->c.ids) throw Error(w + ": in and out must carry the same ids");
        commit(c);
        mark(ctx, in, out);
        c->mod_raise(in->c, out->c);
    })
}
// collective refresh, for the CKKS side and for MK-BFV (every ciphertext of a BFV context that the calls take has nq limbs): under the rules of
// distributed decryption; why_capture closes the capture message
static Context* refresh_enter(mkhe_ctx* ctx, const char* what, bool bfv, int count, const mkhe_ct* const* in, const char* why_capture,
                              const char* why_scheme = nullptr) {
    Context* c = enter(ctx, what);
    count_ok(what, count);
    if (!in) throw Error(std::string(what) + ": null argument");
    if (!bfv) batch_ok(what, count, in);
    scheme_ok(c, what, bfv, why_scheme ? why_scheme : bfv ? ": needs a BFV context (mkhe_refresh_share / mkhe_refresh_merge serve the others)"
                                                          : ": not available on a BFV context (a mask mod T is another protocol)");
    unmasked(c, what);
    if (bfv) batch_ok(what, count, in, c->nq, ": every ciphertext must have the nQ limbs of the context");
    not_captured(c, what, why_capture);
    return c;
}
// the outputs of a refresh call: present, distinct, none of them an input
static void rf_outputs(const char* what, int count, const mkhe_ct* const* in, int nin, mkhe_ct* const* out) {
    for (int b = 0; b < count; ++b) {
        if (!out[b]) throw Error(std::string(what) + ": null output in the batch");
        for (int k = 0; k < b; ++k) if (out[k] == out[b] || out[k]->c.d == out[b]->c.d) throw Error(std::string(what) + ": the outputs of a batch must be distinct");
        for (int k = 0; k < nin; ++k) if (in[k] == out[b] || in[k]->c.d == out[b]->c.d) throw Error(std::string(what) + ": an output aliases an input");
    }
}
// the limbs of the outputs: on a BFV context the nQ limbs of the context, else those of the first output, 1 .. nQ
static int refresh_limbs(const Context* c, const std::string& w, bool bfv, const mkhe_ct* first, const char* name) {
    if (bfv) return c->nq;
    if (first->c.limbs < 1 || first->c.limbs > c->nq) throw Error(w + ": the limbs of " + name + " are out of range");
    return first->c.limbs;
}
// both refresh shares; bits: mask_bits, or (bfv) mask with flood_bits behind it
static void refresh_share_entry(mkhe_ctx* ctx, const char* what, bool bfv, int count, const mkhe_ct* const* in, const int* slots, const void* dev_sk,
                                const void* dev_pk, const uint32_t* key, uint64_t nonce_mask, uint64_t nonce_enc, int bits, int flood_bits,
                                const uint64_t* cdt, int ncdt, void* dev_shares, mkhe_ct* const* reenc) {
    const std::string w(what);
    Context* c = refresh_enter(ctx, what, bfv, count, in, REPLAYS);
    if (!slots || !dev_sk || !dev_pk || !dev_shares || !reenc) throw Error(w + ": null argument");
    smp_table_ok(what, cdt, ncdt);
    need_aligned(dev_sk, what); need_aligned(dev_pk, what); need_aligned(dev_shares, what);
    slots_ok(what, count, in, slots);
    rf_outputs(what, count, in, count, reenc);
    const int lout = refresh_limbs(c, w, bfv, reenc[0], "reenc");
    std::vector<u64*> d(count);
    for (int b = 0; b < count; ++b) {
        const Ct& o = reenc[b]->c;
        if (o.n != 1 || o.ids[0] != in[b]->c.ids[slots[b] - 1]) throw Error(w + ": every reenc must be a ciphertext over exactly the id at the slot of its input");
        if (o.limbs != lout) throw Error(w + (bfv ? ": every reenc must have the nQ limbs of the context" : ": every reenc must have the same number of limbs"));
        d[b] = o.d;
    }
    commit(c, [&] {
        if (!bfv) return;
        c->bfv_prepare(what);                                           // T outside the encoder's preconditions: refused here
        const int most = c->bfv_refresh_max_flood();
        if (flood_bits > most)
            throw Error(w + ": flood_bits must be at most bitlen(Q div 2T) - 1 = " + std::to_string(most) + " (a wider flood alone destroys the message)");
    });
    auto i = ct_list(ctx, in, count, what);
    ct_list_out(ctx, reenc, count, what);
    const u64 *sk = (const u64*)dev_sk, *pk = (const u64*)dev_pk;
    if (bfv) c->bfv_refresh_share(i, slots, sk, pk, key, nonce_mask, nonce_enc, bits, flood_bits, cdt, ncdt, (u64*)dev_shares, d.data());
    else c->refresh_share(i, slots, sk, pk, key, nonce_mask, nonce_enc, bits, cdt, ncdt, (u64*)dev_shares, lout, d.data());
}
int mkhe_refresh_share(mkhe_ctx* ctx, int count, const mkhe_ct* const* in, const int* slots, const void* dev_sk, const void* dev_pk, const uint32_t key[8],
                       uint64_t nonce_mask, uint64_t nonce_enc, int mask_bits, const uint64_t* cdt, int ncdt, void* dev_shares, mkhe_ct* const* reenc) {
    MKHE_TRY({
        if (mask_bits < 0 || mask_bits > RF_MAX_BITS) throw Error("mkhe_refresh_share: mask_bits must be 0 .. 120");
        if (!key) throw Error("mkhe_refresh_share: null key");                  // (mask_bits = 0 reads no mask stream, the encryption still draws its samples)
        if (mask_bits > 0 && nonce_mask == nonce_enc) throw Error("mkhe_refresh_share: nonce_mask and nonce_enc must differ (the mask and the encryption would share streams)");
        refresh_share_entry(ctx, "mkhe_refresh_share", false, count, in, slots, dev_sk, dev_pk, key, nonce_mask, nonce_enc, mask_bits, 0, cdt, ncdt, dev_shares, reenc);
    })
}
int mkhe_bfv_refresh_share(mkhe_ctx* ctx, int count, const mkhe_ct* const* in, const int* slots, const void* dev_sk, const void* dev_pk, const uint32_t key[8],
                           uint64_t nonce_mask, uint64_t nonce_enc, int mask, int flood_bits, const uint64_t* cdt, int ncdt, void* dev_shares,
                           mkhe_ct* const* reenc) {
    MKHE_TRY({
        if (mask != 0 && mask != 1) throw Error("mkhe_bfv_refresh_share: mask must be 0 or 1");
        if (flood_bits < 0 || flood_bits > BRF_MAX_FLOOD) throw Error("mkhe_bfv_refresh_share: flood_bits must be 0 .. 1024");
        if (!key) throw Error("mkhe_bfv_refresh_share: null key");              // (mask = 0 and flood_bits = 0 read no stream of nonce_mask, the encryption still draws its samples)
        if ((mask || flood_bits > 0) && nonce_mask == nonce_enc)
            throw Error("mkhe_bfv_refresh_share: nonce_mask and nonce_enc must differ (the mask and the encryption would share streams)");
        refresh_share_entry(ctx, "mkhe_bfv_refresh_share", true, count, in, slots, dev_sk, dev_pk, key, nonce_mask, nonce_enc, mask, flood_bits, cdt, ncdt, dev_shares, reenc);
    })
}
// both refresh merges
static void refresh_merge_entry(mkhe_ctx* ctx, const char* what, bool bfv, int count, const mkhe_ct* const* in, int nshares, const void* const* dev_shares,
                                const mkhe_ct* const* reenc, mkhe_ct* const* out) {
    const std::string w(what);
    Context* c = refresh_enter(ctx, what, bfv, count, in, UPLOADS);
    if (!out) throw Error(w + ": null argument");
    merge_shape(what, count, in, nshares);
    if (nshares > 0 && (!dev_shares || !reenc)) throw Error(w + ": null argument");
    rf_outputs(what, count, in, count, out);
    const int lout = refresh_limbs(c, w, bfv, out[0], "out");
    std::vector<const u64*> sh(nshares);
    std::vector<const u64*> re((size_t)nshares * count);
    std::vector<u64*> d(count);
    for (int b = 0; b < count; ++b) {
        if (out[b]->c.ids != in[0]->c.ids) throw Error(w + ": every out must be over the ids of the inputs");
        if (out[b]->c.limbs != lout) throw Error(w + (bfv ? ": every out must have the nQ limbs of the context" : ": every out must have the same number of limbs"));
        d[b] = out[b]->c.d;
    }
    for (int i = 0; i < nshares; ++i) {
        sh[i] = share_at(dev_shares, i, what);
        for (int b = 0; b < count; ++b) {
            const mkhe_ct* r = reenc[(size_t)i * count + b];
            if (!r) throw Error(w + ": null reenc in the list");
            if (r->c.n != 1 || r->c.ids[0] != in[0]->c.ids[i]) throw Error(w + ": reenc[i * count + b] must be a ciphertext over exactly the id at slot 1 + i");
            if (r->c.limbs != lout) throw Error(w + (bfv ? ": every reenc must have the nQ limbs of the context" : ": every reenc must have the limbs of out"));
            for (int k = 0; k < count; ++k) if (out[k] == r || out[k]->c.d == r->c.d) throw Error(w + ": an output aliases an input");
            re[(size_t)i * count + b] = r->c.d;
        }
    }
    commit(c, [&] { if (bfv) c->bfv_prepare(what); });
    auto i = ct_list(ctx, in, count, what);
    if (nshares > 0) ct_list(ctx, reenc, nshares * count, what);
    ct_list_out(ctx, out, count, what);
    if (bfv) c->bfv_refresh_merge(i, sh, re, d.data());
    else c->refresh_merge(i, sh, re, lout, d.data());
}
int mkhe_refresh_merge(mkhe_ctx* ctx, int count, const mkhe_ct* const* in, int nshares, const void* const* dev_shares, const mkhe_ct* const* reenc,
                       mkhe_ct* const* out) {
    MKHE_TRY(refresh_merge_entry(ctx, "mkhe_refresh_merge", false, count, in, nshares, dev_shares, reenc, out))
}
int mkhe_bfv_refresh_merge(mkhe_ctx* ctx, int count, const mkhe_ct* const* in, int nshares, const void* const* dev_shares, const mkhe_ct* const* reenc,
                           mkhe_ct* const* out) {
    MKHE_TRY(refresh_merge_entry(ctx, "mkhe_bfv_refresh_merge", true, count, in, nshares, dev_shares, reenc, out))
}
// encryption to shares: the guard, the order of the refusals and their words are those of the refresh calls, under the new names
int mkhe_e2s_share(mkhe_ctx* ctx, int count, const mkhe_ct* const* in, const int* slots, const void* dev_sk, const uint32_t key[8], uint64_t nonce_mask,
                   int mask_bits, void* dev_shares, int secret_limbs, void* dev_secret) {
    MKHE_TRY({
        const char* what = "mkhe_e2s_share";
        const std::string w(what);
        if (mask_bits < 0 || mask_bits > RF_MAX_BITS) throw Error(w + ": mask_bits must be 0 .. 120");
        if (mask_bits > 0 && !key) throw Error(w + ": null key");
        Context* c = refresh_enter(ctx, what, false, count, in, REPLAYS);
        if (!slots || !dev_sk || !dev_shares || !dev_secret) throw Error(w + ": null argument");
        if (secret_limbs < 1 || secret_limbs > c->nq) throw Error(w + ": secret_limbs must be 1 .. nQ");
        need_aligned(dev_sk, what); need_aligned(dev_shares, what); need_aligned(dev_secret, what);
        slots_ok(what, count, in, slots);
        commit(c);
        auto i = ct_list(ctx, in, count, what);
        c->e2s_share(i, slots, (const u64*)dev_sk, key, nonce_mask, mask_bits, (u64*)dev_shares, secret_limbs, (u64*)dev_secret);
    })
}
int mkhe_e2s_merge(mkhe_ctx* ctx, int count, const mkhe_ct* const* in, int nshares, const void* const* dev_shares, int limbs_out, void* dev_pt_out) {
    MKHE_TRY({
        const char* what = "mkhe_e2s_merge";
        const std::string w(what);
        Context* c = refresh_enter(ctx, what, false, count, in, UPLOADS);
        if (!dev_pt_out) throw Error(w + ": null argument");
        merge_shape(what, count, in, nshares);
        if (nshares > 0 && !dev_shares) throw Error(w + ": null argument");
        if (limbs_out < 1 || limbs_out > c->nq) throw Error(w + ": limbs_out must be 1 .. nQ");
        need_aligned(dev_pt_out, what);
        auto sh = share_list(dev_shares, nshares, what);
        commit(c);
        auto i = ct_list(ctx, in, count, what);
        c->e2s_merge(i, sh, limbs_out, (u64*)dev_pt_out);
    })
}
int mkhe_bfv_e2s_share(mkhe_ctx* ctx, int count, const mkhe_ct* const* in, const int* slots, const void* dev_sk, const uint32_t key[8], uint64_t nonce_mask,
                       int flood_bits, void* dev_shares, void* dev_secret) {
    MKHE_TRY({
        const char* what = "mkhe_bfv_e2s_share";
        const std::string w(what);
        if (flood_bits < 0 || flood_bits > BRF_MAX_FLOOD) throw Error(w + ": flood_bits must be 0 .. 1024");
        if (!key) throw Error(w + ": null key");                                // (the mask is always drawn)
        Context* c = refresh_enter(ctx, what, true, count, in, REPLAYS, ": needs a BFV context (mkhe_e2s_share / mkhe_e2s_merge serve the others)");
        if (!slots || !dev_sk || !dev_shares || !dev_secret) throw Error(w + ": null argument");
        need_aligned(dev_sk, what); need_aligned(dev_shares, what); need_aligned(dev_secret, what);
        slots_ok(what, count, in, slots);
        commit(c, [&] {
            c->bfv_prepare(what);                                               // T outside the encoder's preconditions: refused here
            const int most = c->bfv_refresh_max_flood();
            if (flood_bits > most)
                throw Error(w + ": flood_bits must be at most bitlen(Q div 2T) - 1 = " + std::to_string(most) + " (a wider flood alone destroys the message)");
        });
        auto i = ct_list(ctx, in, count, what);
        c->bfv_e2s_share(i, slots, (const u64*)dev_sk, key, nonce_mask, flood_bits, (u64*)dev_shares, (u64*)dev_secret);
    })
}
// collective key switch to a recipient's public key, under the rules of distributed decryption.  The share draws from the keystream and is refused
// inside a capture; the merge allocates nothing, uploads nothing that outlives the call and may be captured as long as it stages no table (count
// and nshares at most 16).
static Context* pcks_enter(mkhe_ctx* ctx, const char* what, int count, const mkhe_ct* const* in, bool keystream) {
    Context* c = enter(ctx, what);
    count_ok(what, count);
    if (!in) throw Error(std::string(what) + ": null argument");
    batch_ok(what, count, in, c->is_bfv() ? c->nq : 0, ": on a BFV context every ciphertext must have the nQ limbs of the context");
    unmasked(c, what);
    if (keystream) not_captured(c, what, REPLAYS);
    else if (count > ED_INLINE) not_captured(c, what, STAGES);
    return c;
}
int mkhe_pcks_share(mkhe_ctx* ctx, int count, const mkhe_ct* const* in, const int* slots, const void* dev_sk, const void* dev_pk_recipient,
                    const uint32_t key[8], uint64_t nonce, int flood_bits, const uint64_t* cdt, int ncdt, void* dev_shares) {
    MKHE_TRY({
        const char* what = "mkhe_pcks_share";
        if (flood_bits < 0 || flood_bits > PCKS_MAX_FLOOD) throw Error("mkhe_pcks_share: flood_bits must be 0 .. 1024");
        if (!key) throw Error("mkhe_pcks_share: null key");                     // (flood_bits = 0 reads no flood stream, u and e1 are drawn from the key all the same)
        Context* c = pcks_enter(ctx, what, count, in, true);
        if (!slots || !dev_sk || !dev_pk_recipient || !dev_shares) throw Error("mkhe_pcks_share: null argument");
        smp_table_ok(what, cdt, ncdt);
        need_aligned(dev_sk, what); need_aligned(dev_pk_recipient, what); need_aligned(dev_shares, what);
        slots_ok(what, count, in, slots);
        const int most = c->flood_room(in[0]->c.limbs, c->is_bfv() ? c->bfv_t : 1);
        if (flood_bits > most)
            throw Error("mkhe_pcks_share: flood_bits must be at most bitlen(Q_l div 2T') - 1 = " + std::to_string(most) + " (a wider flood alone destroys the message)");
        commit(c);
        auto i = ct_list(ctx, in, count, what);
        c->pcks_share(i, slots, (const u64*)dev_sk, (const u64*)dev_pk_recipient, key, nonce, flood_bits, cdt, ncdt, (u64*)dev_shares);
    })
}
int mkhe_pcks_merge(mkhe_ctx* ctx, int count, const mkhe_ct* const* in, int nshares, const void* const* dev_shares, mkhe_ct* const* out) {
    MKHE_TRY({
        const char* what = "mkhe_pcks_merge";
        Context* c = pcks_enter(ctx, what, count, in, false);
        if (!out) throw Error("mkhe_pcks_merge: null argument");
        merge_shape(what, count, in, nshares);
        if (nshares > 0 && !dev_shares) throw Error("mkhe_pcks_merge: null argument");
        rf_outputs(what, count, in, count, out);
        std::vector<u64*> d(count);
        for (int b = 0; b < count; ++b) {
            if (out[b]->c.n != 1) throw Error("mkhe_pcks_merge: every out must be a ciphertext over exactly one id (the recipient's)");
            if (out[b]->c.limbs != in[0]->c.limbs) throw Error("mkhe_pcks_merge: every out must have the limbs of the inputs");
            d[b] = out[b]->c.d;
        }
        auto sh = share_list(dev_shares, nshares, what);
        if (nshares > ED_INLINE) not_captured(c, what, STAGES);
        commit(c);
        auto i = ct_list(ctx, in, count, what);
        ct_list_out(ctx, out, count, what);
        c->pcks_merge(i, sh, d.data());
    })
}
// threshold secret keys, under the rules of the protocol family.  The sharing draws from a SECRET keystream and is refused inside a capture; the
// additive key and the fold allocate nothing and may be captured as long as they stage no table (the fold: at most 16 sources).  points_ok: the
// points of a sharing or of an active set are 1 .. 32, pairwise distinct, at least 1 and below every modulus of the rows.
static void points_ok(const Context* c, const char* what, const char* name, int n, const uint32_t* x) {
    const std::string w(what);
    if (n < 1 || n > THR_MAX) throw Error(w + ": " + name + " must be 1 .. 32");
    if (!x) throw Error(w + ": null points");
    for (int p = 0; p < n; ++p) {
        if (x[p] < 1) throw Error(w + ": every point must be at least 1 (0 is where the secret sits)");
        for (int j = 0; j < c->mtot; ++j)
            if ((u64)x[p] >= c->moduli[j]) throw Error(w + ": every point must be smaller than every modulus of the context");
        for (int k = 0; k < p; ++k) if (x[k] == x[p]) throw Error(w + ": the points must be pairwise distinct");
    }
}
int mkhe_threshold_gen_shares(mkhe_ctx* ctx, const void* dev_sk, int threshold, int nshares, const uint32_t* points, const uint32_t key[8],
                              uint64_t nonce, void* const* dev_out) {
    MKHE_TRY({
        const char* what = "mkhe_threshold_gen_shares";
        const std::string w(what);
        Context* c = enter(ctx, what);
        if (!key) throw Error(w + ": null key");                                // (threshold = 1 reads no stream: the rule is that of mkhe_pcks_share)
        if (!dev_sk || !dev_out) throw Error(w + ": null argument");
        points_ok(c, what, "nshares", nshares, points);
        if (threshold < 1 || threshold > nshares) throw Error(w + ": threshold must be 1 .. nshares");
        need_aligned(dev_sk, what);
        std::vector<u64*> o(nshares);
        for (int p = 0; p < nshares; ++p) {
            if (!dev_out[p]) throw Error(w + ": null output in the per-holder list");
            need_aligned(dev_out[p], what);
            if (dev_out[p] == dev_sk) throw Error(w + ": an output must not be the secret key's buffer");
            for (int k = 0; k < p; ++k) if (dev_out[k] == dev_out[p]) throw Error(w + ": the outputs must be distinct");
            o[p] = (u64*)dev_out[p];
        }
        unmasked(c, what);
        not_captured(c, what, REPLAYS);
        commit(c);
        c->threshold_gen_shares((const u64*)dev_sk, threshold, nshares, points, key, nonce, o.data());
    })
}
int mkhe_threshold_additive_key(mkhe_ctx* ctx, const void* dev_share, uint32_t point, int nactive, const uint32_t* active_points, void* dev_out) {
    MKHE_TRY({
        const char* what = "mkhe_threshold_additive_key";
        const std::string w(what);
        Context* c = enter(ctx, what);
        if (!dev_share || !dev_out) throw Error(w + ": null argument");
        points_ok(c, what, "nactive", nactive, active_points);
        int found = 0;
        for (int i = 0; i < nactive; ++i) found += active_points[i] == point ? 1 : 0;
        if (found != 1) throw Error(w + ": point must occur in active_points exactly once");
        need_aligned(dev_share, what); need_aligned(dev_out, what);
        static_assert(THR_MAX_ROWS >= NTT_MAX_SLOTS, "the Lagrange coefficients of every row of a context travel in the kernel arguments");
        unmasked(c, what);
        commit(c);
        c->threshold_additive_key((const u64*)dev_share, point, nactive, active_points, (u64*)dev_out);
    })
}
int mkhe_limbs_sum(mkhe_ctx* ctx, int count, int limbs, int nsrc, const void* const* dev_src, void* dev_dst) {
    MKHE_TRY({
        const char* what = "mkhe_limbs_sum";
        const std::string w(what);
        Context* c = enter(ctx, what);
        count_ok(what, count);
        if (!(limbs >= 1 && limbs <= c->nq) && limbs != c->mtot) throw Error(w + ": limbs must be 1 .. nQ, or nQ + nP (the rows of a secret key)");
        if (nsrc < 1 || nsrc > THR_MAX) throw Error(w + ": nsrc must be 1 .. 32");
        if (!dev_src || !dev_dst) throw Error(w + ": null argument");
        need_aligned(dev_dst, what);
        std::vector<const u64*> src(nsrc);
        const size_t bytes = (size_t)count * limbs * c->N * sizeof(u64);
        for (int s = 0; s < nsrc; ++s) {
            if (!dev_src[s]) throw Error(w + ": null source in the list");
            need_aligned(dev_src[s], what);
            const uintptr_t a = (uintptr_t)dev_src[s];
            const uintptr_t d = (uintptr_t)dev_dst;
            if (a != d && a < d + bytes && d < a + bytes) throw Error(w + ": dst may equal a source exactly, not overlap it");
            src[s] = (const u64*)dev_src[s];
        }
        unmasked(c, what);
        if (nsrc > ED_INLINE) not_captured(c, what, "with more than 16 sources (the pointer table is staged)");
        commit(c);
        c->limbs_sum(count, limbs, src, (u64*)dev_dst);
    })
}

// ---- CKKS encoder (ckks_encode.hip)
// the argument checks every call of the two encoders shares (the BFV batch encoder is bfv_encode.hip); their null context is need()'s
static Context* encoder_enter(mkhe_ctx* ctx, bool bfv, const char* what, int count, const void* a, const void* b) {
    Context* c = enter(ctx, nullptr);
    if (!a || !b) throw Error(std::string(what) + ": null argument");
    count_ok(what, count);
    need_aligned(a, what); need_aligned(b, what);
    scheme_ok(c, what, bfv, bfv ? ": the BFV encoder needs a BFV context" : ": the CKKS encoder needs a CKKS context");
    unmasked(c, what);
    not_captured(c, what, UPLOADS);
    commit(c);
    return c;
}
static Context* encoder_enter(mkhe_ctx* ctx, bool bfv, const char* what) {
    alignas(16) static const u64 dummy[2] = {0, 0};         // (no buffers in these calls)
    return encoder_enter(ctx, bfv, what, 1, dummy, dummy);
}
int mkhe_ctx_ckks_tile(mkhe_ctx* ctx) {
    g_last_ctx = nullptr;
    try { return encoder_enter(ctx, false, "mkhe_ctx_ckks_tile")->ckks_tile(); }
    catch (const std::exception& e) { g_err = e.what(); return -1; }
    catch (...) { g_err = "mkhe: unknown error"; return -1; }
}
int mkhe_ctx_set_ckks_tile(mkhe_ctx* ctx, int log_points) { MKHE_TRY({ encoder_enter(ctx, false, "mkhe_ctx_set_ckks_tile")->ckks_set_tile(log_points); }) }
static void ck_scale_ok(double scale, const char* what) {
    if (!(scale > 0.0) || scale > 1.7976931348623157e308) throw Error(std::string(what) + ": scale must be finite and positive");
}
static void ck_limbs_ok(const Context* c, int limbs, const char* what, const char* name) {
    if (limbs < 1 || limbs > c->nq) throw Error(std::string(what) + ": " + name + " out of range");
}
int mkhe_ckks_embed(mkhe_ctx* ctx, int count, const void* dev_slots, void* dev_coeffs) {
    MKHE_TRY({ encoder_enter(ctx, false, "mkhe_ckks_embed", count, dev_slots, dev_coeffs)->ckks_embed(count, (const double*)dev_slots, (double*)dev_coeffs); })
}
int mkhe_ckks_project(mkhe_ctx* ctx, int count, const void* dev_coeffs, void* dev_slots) {
    MKHE_TRY({ encoder_enter(ctx, false, "mkhe_ckks_project", count, dev_coeffs, dev_slots)->ckks_project(count, (const double*)dev_coeffs, (double*)dev_slots); })
}
int mkhe_ckks_scale_up(mkhe_ctx* ctx, int level, int count, const void* dev_coeffs, double scale, void* dev_pt) {
    MKHE_TRY({
        ck_scale_ok(scale, "mkhe_ckks_scale_up");
        Context* c = encoder_enter(ctx, false, "mkhe_ckks_scale_up", count, dev_coeffs, dev_pt);
        ck_limbs_ok(c, level + 1, "mkhe_ckks_scale_up", "level");
        c->ckks_scale_up(level, count, (const double*)dev_coeffs, scale, (u64*)dev_pt);
    })
}
int mkhe_ckks_scale_down(mkhe_ctx* ctx, int limbs, int count, const void* dev_pt, double scale, void* dev_coeffs) {
    MKHE_TRY({
        ck_scale_ok(scale, "mkhe_ckks_scale_down");
        Context* c = encoder_enter(ctx, false, "mkhe_ckks_scale_down", count, dev_pt, dev_coeffs);
        ck_limbs_ok(c, limbs, "mkhe_ckks_scale_down", "limbs");
        c->ckks_scale_down(limbs, count, (const u64*)dev_pt, scale, (double*)dev_coeffs);
    })
}
int mkhe_ckks_encode(mkhe_ctx* ctx, int level, int count, const void* dev_slots, double scale, void* dev_pt) {
    MKHE_TRY({
        ck_scale_ok(scale, "mkhe_ckks_encode");
        Context* c = encoder_enter(ctx, false, "mkhe_ckks_encode", count, dev_slots, dev_pt);
        ck_limbs_ok(c, level + 1, "mkhe_ckks_encode", "level");
        c->ckks_encode(level, count, (const double*)dev_slots, scale, (u64*)dev_pt);
    })
}
int mkhe_ckks_decode(mkhe_ctx* ctx, int limbs, int count, const void* dev_pt, double scale, void* dev_slots) {
    MKHE_TRY({
        ck_scale_ok(scale, "mkhe_ckks_decode");
        Context* c = encoder_enter(ctx, false, "mkhe_ckks_decode", count, dev_pt, dev_slots);
        ck_limbs_ok(c, limbs, "mkhe_ckks_decode", "limbs");
        c->ckks_decode(limbs, count, (const u64*)dev_pt, scale, (double*)dev_slots);
    })
}
int mkhe_ckks_embed_sparse(mkhe_ctx* ctx, int log_slots, int count, const void* dev_slots, void* dev_coeffs) {
    MKHE_TRY({
        encoder_enter(ctx, false, "mkhe_ckks_embed_sparse", count, dev_slots, dev_coeffs)->ckks_embed_sparse(log_slots, count, (const double*)dev_slots,
                                                                                                             (double*)dev_coeffs);
    })
}
int mkhe_ckks_project_sparse(mkhe_ctx* ctx, int log_slots, int count, const void* dev_coeffs, void* dev_slots) {
    MKHE_TRY({
        encoder_enter(ctx, false, "mkhe_ckks_project_sparse", count, dev_coeffs, dev_slots)->ckks_project_sparse(log_slots, count, (const double*)dev_coeffs,
                                                                                                                 (double*)dev_slots);
    })
}
int mkhe_ckks_encode_sparse(mkhe_ctx* ctx, int level, int log_slots, int count, const void* dev_slots, double scale, void* dev_pt) {
    MKHE_TRY({
        ck_scale_ok(scale, "mkhe_ckks_encode_sparse");
        Context* c = encoder_enter(ctx, false, "mkhe_ckks_encode_sparse", count, dev_slots, dev_pt);
        ck_limbs_ok(c, level + 1, "mkhe_ckks_encode_sparse", "level");
        c->ckks_encode_sparse(level, log_slots, count, (const double*)dev_slots, scale, (u64*)dev_pt);
    })
}
int mkhe_ckks_decode_sparse(mkhe_ctx* ctx, int limbs, int log_slots, int count, const void* dev_pt, double scale, void* dev_slots) {
    MKHE_TRY({
        ck_scale_ok(scale, "mkhe_ckks_decode_sparse");
        Context* c = encoder_enter(ctx, false, "mkhe_ckks_decode_sparse", count, dev_pt, dev_slots);
        ck_limbs_ok(c, limbs, "mkhe_ckks_decode_sparse", "limbs");
        c->ckks_decode_sparse(limbs, log_slots, count, (const u64*)dev_pt, scale, (double*)dev_slots);
    })
}

// ---- BFV batch encoder (bfv_encode.hip)
int mkhe_ctx_bfv_tile(mkhe_ctx* ctx) {
    g_last_ctx = nullptr;
    try { return encoder_enter(ctx, true, "mkhe_ctx_bfv_tile")->bfv_tile(); }
    catch (const std::exception& e) { g_err = e.what(); return -1; }
    catch (...) { g_err = "mkhe: unknown error"; return -1; }
}
int mkhe_ctx_set_bfv_tile(mkhe_ctx* ctx, int log_points) { MKHE_TRY({ encoder_enter(ctx, true, "mkhe_ctx_set_bfv_tile")->bfv_set_tile(log_points); }) }
uint64_t mkhe_ctx_bfv_slot_psi(mkhe_ctx* ctx) {
    g_last_ctx = nullptr;
    try { return encoder_enter(ctx, true, "mkhe_ctx_bfv_slot_psi")->bfv_slot_psi(); }
    catch (const std::exception& e) { g_err = e.what(); return 0; }
    catch (...) { g_err = "mkhe: unknown error"; return 0; }
}
int mkhe_bfv_slots_to_coeffs(mkhe_ctx* ctx, int count, const void* dev_slots, void* dev_coeffs) {
    MKHE_TRY({ encoder_enter(ctx, true, "mkhe_bfv_slots_to_coeffs", count, dev_slots, dev_coeffs)->bfv_slots_to_coeffs(count, (const u64*)dev_slots, (u64*)dev_coeffs); })
}
int mkhe_bfv_coeffs_to_slots(mkhe_ctx* ctx, int count, const void* dev_coeffs, void* dev_slots) {
    MKHE_TRY({ encoder_enter(ctx, true, "mkhe_bfv_coeffs_to_slots", count, dev_coeffs, dev_slots)->bfv_coeffs_to_slots(count, (const u64*)dev_coeffs, (u64*)dev_slots); })
}
int mkhe_bfv_scale_up(mkhe_ctx* ctx, int count, const void* dev_coeffs, void* dev_pt) {
    MKHE_TRY({ encoder_enter(ctx, true, "mkhe_bfv_scale_up", count, dev_coeffs, dev_pt)->bfv_scale_up(count, (const u64*)dev_coeffs, (u64*)dev_pt); })
}
int mkhe_bfv_scale_down(mkhe_ctx* ctx, int count, const void* dev_pt, void* dev_coeffs) {
    MKHE_TRY({ encoder_enter(ctx, true, "mkhe_bfv_scale_down", count, dev_pt, dev_coeffs)->bfv_scale_down(count, (const u64*)dev_pt, (u64*)dev_coeffs); })
}
int mkhe_bfv_encode(mkhe_ctx* ctx, int count, const void* dev_slots, void* dev_pt) {
    MKHE_TRY({ encoder_enter(ctx, true, "mkhe_bfv_encode", count, dev_slots, dev_pt)->bfv_encode(count, (const u64*)dev_slots, (u64*)dev_pt); })
}
int mkhe_bfv_decode(mkhe_ctx* ctx, int count, const void* dev_pt, void* dev_slots) {
    MKHE_TRY({ encoder_enter(ctx, true, "mkhe_bfv_decode", count, dev_pt, dev_slots)->bfv_decode(count, (const u64*)dev_pt, (u64*)dev_slots); })
}
// slot map: the encoder's guard; prepare downloads and validates on the host (the index check is the call's own refusal, behind the guard)
int mkhe_bfv_slot_map_prepare(mkhe_ctx* ctx, const void* dev_index, const void* dev_mult, void* dev_map) {
    MKHE_TRY({
        const char* what = "mkhe_bfv_slot_map_prepare";
        enter(ctx, nullptr);
        need_aligned(dev_mult, what);
        encoder_enter(ctx, true, what, 1, dev_index, dev_map)->bfv_slot_map_prepare((const u32*)dev_index, (const u64*)dev_mult, (u64*)dev_map);
    })
}
int mkhe_bfv_slot_map(mkhe_ctx* ctx, int count, const void* dev_coeffs_in, const void* dev_map, void* dev_coeffs_out) {
    MKHE_TRY({
        const char* what = "mkhe_bfv_slot_map";
        enter(ctx, nullptr);
        if (!dev_map) throw Error(std::string(what) + ": null argument");
        need_aligned(dev_map, what);
        encoder_enter(ctx, true, what, count, dev_coeffs_in, dev_coeffs_out)->bfv_slot_map(count, (const u64*)dev_coeffs_in, (const u64*)dev_map, (u64*)dev_coeffs_out);
    })
}
int mkhe_bfv_lift(mkhe_ctx* ctx, int count, const void* dev_coeffs, void* dev_ptmul_coeff) {
    MKHE_TRY({ encoder_enter(ctx, true, "mkhe_bfv_lift", count, dev_coeffs, dev_ptmul_coeff)->bfv_lift(count, (const u64*)dev_coeffs, (u64*)dev_ptmul_coeff); })
}
int mkhe_bfv_encode_mul(mkhe_ctx* ctx, int count, const void* dev_slots, void* dev_ptmul) {
    MKHE_TRY({ encoder_enter(ctx, true, "mkhe_bfv_encode_mul", count, dev_slots, dev_ptmul)->bfv_encode_mul(count, (const u64*)dev_slots, (u64*)dev_ptmul); })
}
int mkhe_bfv_ct_mul_ptxt(mkhe_ctx* ctx, int nbatch, const mkhe_ct* const* in, const void* dev_ptmul, long pt_stride_words, mkhe_ct* const* out) {
    MKHE_TRY({
        const char* what = "mkhe_bfv_ct_mul_ptxt";
        Context* c = encoder_enter(ctx, true, what, nbatch, dev_ptmul, dev_ptmul);
        auto i = ct_list(ctx, in, nbatch, what);
        auto o = ct_list_out(ctx, out, nbatch, what);
        c->bfv_ct_mul_ptxt(what, i, (const u64*)dev_ptmul, pt_stride_words, o);
    })
}
// the counts are checked before the context is looked at, so that they can be refused without a device; the masks before anything is armed
int mkhe_bfv_ct_ptxt_dot(mkhe_ctx* ctx, int nbatch, int nin, const mkhe_ct* const* in, int ngiant, const uint32_t* masks, const void* dev_ptmul,
                         mkhe_ct* const* out) {
    MKHE_TRY({
        const char* what = "mkhe_bfv_ct_ptxt_dot";
        const std::string w = std::string(what) + ": ";
        if (nbatch < 1 || nbatch > CTDOT_MAX_BATCH) throw Error(w + "nbatch must be 1 .. " + std::to_string(CTDOT_MAX_BATCH));
        if (nin < 1 || nin > CTDOT_MAX_IN) throw Error(w + "nin must be 1 .. " + std::to_string(CTDOT_MAX_IN));
        if (ngiant < 1 || ngiant > CTDOT_MAX_GIANT) throw Error(w + "ngiant must be 1 .. " + std::to_string(CTDOT_MAX_GIANT));
        Context* c = enter(ctx, what);
        if (!in || !masks || !dev_ptmul || !out) throw Error(w + "null argument");
        need_aligned(dev_ptmul, what);
        scheme_ok(c, what, true, ": needs a BFV context");
        unmasked(c, what);
        not_captured(c, what, "(the call may allocate or stage)");
        for (int g = 0; g < ngiant; ++g) {
            if (!masks[g]) throw Error(w + "a mask is zero");
            if (masks[g] >> nin) throw Error(w + "a mask has a bit at or above nin");
        }
        for (int i = 0; i < nbatch * nin; ++i) ct_at(in, i, what);
        for (int i = 0; i < nbatch * ngiant; ++i) if (!out[i]) throw Error(w + "null output in the batch");
        commit(c);
        auto i = ct_list(ctx, in, nbatch * nin, what);
        auto o = ct_list_out(ctx, out, nbatch * ngiant, what);
        c->bfv_prepare(what);
        for (const Ct* x : i) if (x->limbs != c->nq) throw Error(w + "BFV ciphertexts sit at the maximum level (nQ limbs)");
        for (const Ct* x : o) if (x->limbs != c->nq) throw Error(w + "BFV ciphertexts sit at the maximum level (nQ limbs)");
        c->ct_ptxt_dot(what, nbatch, i, std::vector<unsigned int>(masks, masks + ngiant), (const u64*)dev_ptmul, (long)c->nq * c->N, c->nq, o);
    })
}
// BFV weighted sums (engine_ops.hip); the counts first, as above
int mkhe_bfv_ct_lincomb(mkhe_ctx* ctx, int nin, const mkhe_ct* const* in, int nout, const void* dev_consts, mkhe_ct* const* out) {
    MKHE_TRY({
        const char* what = "mkhe_bfv_ct_lincomb";
        const std::string w = std::string(what) + ": ";
        if (nin < 1 || nin > BLIN_MAX_IN) throw Error(w + "nin must be 1 .. " + std::to_string(BLIN_MAX_IN));
        if (nout < 1 || nout > BLIN_MAX_OUT) throw Error(w + "nout must be 1 .. " + std::to_string(BLIN_MAX_OUT));
        Context* c = enter(ctx, what);
        if (!in || !dev_consts || !out) throw Error(w + "null argument");
        need_aligned(dev_consts, what);
        scheme_ok(c, what, true, ": needs a BFV context");
        unmasked(c, what);
        not_captured(c, what, "(the call may allocate or stage)");
        for (int i = 0; i < nin; ++i) ct_at(in, i, what);
        for (int i = 0; i < nout; ++i) if (!out[i]) throw Error(w + "null output in the batch");
        commit(c);
        auto i = ct_list(ctx, in, nin, what);
        auto o = ct_list_out(ctx, out, nout, what);
        c->bfv_prepare(what);
        c->bfv_ct_lincomb(what, i, (const u64*)dev_consts, o);
    })
}
int mkhe_bfv_ct_add_ptxt(mkhe_ctx* ctx, int op, int nbatch, const mkhe_ct* const* in, const void* dev_pt, long pt_stride_words, mkhe_ct* const* out) {
    MKHE_TRY({
        const char* what = "mkhe_bfv_ct_add_ptxt";
        Context* c = encoder_enter(ctx, true, what, nbatch, dev_pt, dev_pt);
        if (op != 0 && op != 1) throw Error(std::string(what) + ": op must be 0 (add) or 1 (sub)");
        auto i = ct_list(ctx, in, nbatch, what);
        auto o = ct_list_out(ctx, out, nbatch, what);
        c->bfv_ct_add_ptxt(what, op, i, (const u64*)dev_pt, pt_stride_words, o);
    })
}

// ---- mkbfv
int mkhe_ctx_create_bfv(mkhe_ctx** out, int logN, const uint64_t* Q, const uint64_t* QMul, int nQ,
                        const uint64_t* P, int nP, int gamma, uint64_t T, int device) {
    MKHE_TRY({
        if (!out || !Q || !QMul || !P) throw Error("mkhe_ctx_create_bfv: null argument");
        *out = new mkhe_ctx{new Context(logN, Q, nQ, P, nP, gamma, nullptr, nullptr, device, QMul, nQ, T)};
    })
}
int mkhe_bfv_modup_q_to_r(mkhe_ctx* ctx, const void* q, void* r, int npolys) {
    MKHE_TRY({ if (!q || !r || npolys < 1) throw Error("mkhe_bfv_modup_q_to_r: bad argument"); need(ctx)->bfv_modup_q_to_r((const u64*)q, (u64*)r, npolys); })
}
int mkhe_bfv_rescale(mkhe_ctx* ctx, const void* q, void* r, int npolys) {
    MKHE_TRY({ if (!q || !r || npolys < 1) throw Error("mkhe_bfv_rescale: bad argument"); need(ctx)->bfv_rescale((const u64*)q, (u64*)r, npolys); })
}
int mkhe_bfv_quantize(mkhe_ctx* ctx, const void* r, void* q, int npolys) {
    MKHE_TRY({ if (!q || !r || npolys < 1) throw Error("mkhe_bfv_quantize: bad argument"); need(ctx)->bfv_quantize((const u64*)r, (u64*)q, npolys); })
}
int mkhe_bfv_ntt_r(mkhe_ctx* ctx, const void* src, void* dst, int count, int inverse) {
    MKHE_TRY({ if (!src || !dst || count < 1) throw Error("mkhe_bfv_ntt_r: bad argument"); need(ctx)->ntt_r((const u64*)src, (u64*)dst, count, inverse != 0); })
}
int mkhe_bfv_decompose(mkhe_ctx* ctx, const void* polyr, mkhe_swk* ad1, mkhe_swk* ad2) {
    MKHE_TRY({ mark(ctx, ad1, ad2);
        if (!polyr || !ad1 || !ad2) throw Error("mkhe_bfv_decompose: null argument");
        need(ctx)->bfv_decompose_batch({(const u64*)polyr}, {ad1->s.d}, {ad2->s.d});
    })
}
int mkhe_bfv_external_product(mkhe_ctx* ctx, const void* dev_polyr, const mkhe_swk* bg1, const mkhe_swk* bg2, void* dev_c) {
    MKHE_TRY({ mark(ctx, bg1, bg2);
        if (!dev_polyr || !bg1 || !bg2 || !dev_c) throw Error("mkhe_bfv_external_product: null argument");
        need(ctx)->bfv_external_product((const u64*)dev_polyr, bg1->s.d, bg2->s.d, (u64*)dev_c);
    })
}
int mkhe_bfv_external_product_hoisted(mkhe_ctx* ctx, const mkhe_swk* ah1, const mkhe_swk* ah2,
                                      const mkhe_swk* bg1, const mkhe_swk* bg2, void* dev_c) {
    MKHE_TRY({ mark(ctx, ah1, ah2, bg1, bg2);
        if (!ah1 || !ah2 || !bg1 || !bg2 || !dev_c) throw Error("mkhe_bfv_external_product_hoisted: null argument");
        need(ctx)->bfv_external_product_hoisted(ah1->s.d, ah2->s.d, bg1->s.d, bg2->s.d, (u64*)dev_c);
    })
}
int mkhe_bfv_mul_relin(mkhe_ctx* ctx, const mkhe_ct* op0, const mkhe_ct* op1,
                       const mkhe_swk* const* rlk_b1, const mkhe_swk* const* rlk_b2,
                       const mkhe_swk* const* rlk_d1, const mkhe_swk* const* rlk_d2,
                       const mkhe_swk* const* rlk_v, const mkhe_swk* crs_u, mkhe_ct* out) {
    MKHE_TRY({ mark(ctx, op0, op1, crs_u, out);
        if (!op0 || !op1 || !out || !crs_u || !rlk_b1 || !rlk_b2 || !rlk_d1 || !rlk_d2 || !rlk_v) throw Error("mkhe_bfv_mul_relin: null argument");
        auto b1 = swk_list(ctx, rlk_b1, op1->c.n); auto b2 = swk_list(ctx, rlk_b2, op1->c.n);
        auto d1 = swk_list(ctx, rlk_d1, op0->c.n); auto d2 = swk_list(ctx, rlk_d2, op0->c.n); auto v = swk_list(ctx, rlk_v, op0->c.n);
        need(ctx)->bfv_mul_relin(op0->c, op1->c, b1.data(), b2.data(), d1.data(), d2.data(), v.data(), crs_u->s, out->c);
    })
}

// (a function of its own, as mul_relin_sum_body)
static void bfv_mul_relin_sum_body(mkhe_ctx* ctx, int K, const mkhe_ct* const* op0, const mkhe_ct* const* op1,
                                   const mkhe_swk* const* rlk_b1, const mkhe_swk* const* rlk_b2,
                                   const mkhe_swk* const* rlk_d1, const mkhe_swk* const* rlk_d2,
                                   const mkhe_swk* const* rlk_v, const mkhe_swk* crs_u, mkhe_ct* out) {
    const std::string what = "mkhe_bfv_mul_relin_sum";
    try {
        if (!ctx) throw Error(what + ": null context");
        if (K < 1 || K > TSUM_MAX_K) throw Error(what + ": takes 1 to " + std::to_string(TSUM_MAX_K) + " pairs");      // (before the lists are read)
        if (!out || !crs_u || !rlk_b1 || !rlk_b2 || !rlk_d1 || !rlk_d2 || !rlk_v) throw Error(what + ": null argument");
        auto a = ct_list(ctx, op0, K, what.c_str());
        auto b = ct_list(ctx, op1, K, what.c_str());
        const int n0 = a[0]->n, n1 = b[0]->n;      // (that every pair carries these ids, and that out is none of the operands, is the engine's check)
        auto keys = [&](const mkhe_swk* const* v, size_t n, const char* name) {
            std::vector<const Swk*> r(n);
            for (size_t i = 0; i < n; ++i) { if (!v[i]) throw Error(what + ": null handle in " + name); mark(ctx, v[i]); r[i] = &v[i]->s; }
            return r;
        };
        auto b1 = keys(rlk_b1, n1, "rlk_b1"); auto b2 = keys(rlk_b2, n1, "rlk_b2");
        auto d1 = keys(rlk_d1, n0, "rlk_d1"); auto d2 = keys(rlk_d2, n0, "rlk_d2");
        auto v = keys(rlk_v, n0, "rlk_v");
        need(ctx)->bfv_mul_relin_sum(a, b, b1.data(), b2.data(), d1.data(), d2.data(), v.data(), crs_u->s, out->c);
    } catch (const std::exception& e) {
        // every message of this entry point starts with its name, whichever layer raised it
        const std::string m = e.what();
        if (m.compare(0, what.size() + 1, what + ":") == 0) throw;
        throw Error(what + ": " + m);
    }
}
int mkhe_bfv_mul_relin_sum(mkhe_ctx* ctx, int K, const mkhe_ct* const* op0, const mkhe_ct* const* op1,
                           const mkhe_swk* const* rlk_b1, const mkhe_swk* const* rlk_b2,
                           const mkhe_swk* const* rlk_d1, const mkhe_swk* const* rlk_d2,
                           const mkhe_swk* const* rlk_v, const mkhe_swk* crs_u, mkhe_ct* out) {
    MKHE_TRY({ mark(ctx, crs_u, out); bfv_mul_relin_sum_body(ctx, K, op0, op1, rlk_b1, rlk_b2, rlk_d1, rlk_d2, rlk_v, crs_u, out); })
}

int mkhe_bfv_mul_relin_unhoisted(mkhe_ctx* ctx, const mkhe_ct* op0, const mkhe_ct* op1,
                                 const mkhe_swk* const* rlk_b1, const mkhe_swk* const* rlk_b2,
                                 const mkhe_swk* const* rlk_d1, const mkhe_swk* const* rlk_d2,
                                 const mkhe_swk* const* rlk_v, const mkhe_swk* crs_u, mkhe_ct* out) {
    MKHE_TRY({ mark(ctx, op0, op1, crs_u, out);
        if (!op0 || !op1 || !out || !crs_u || !rlk_b1 || !rlk_b2 || !rlk_d1 || !rlk_d2 || !rlk_v) throw Error("mkhe_bfv_mul_relin_unhoisted: null argument");
        auto b1 = swk_list(ctx, rlk_b1, op1->c.n); auto b2 = swk_list(ctx, rlk_b2, op1->c.n);
        auto d1 = swk_list(ctx, rlk_d1, op0->c.n); auto d2 = swk_list(ctx, rlk_d2, op0->c.n); auto v = swk_list(ctx, rlk_v, op0->c.n);
        need(ctx)->bfv_mul_relin_unhoisted(op0->c, op1->c, b1.data(), b2.data(), d1.data(), d2.data(), v.data(), crs_u->s, out->c);
    })
}

int mkhe_bfv_mr_partial(mkhe_ctx* ctx, const mkhe_ct* op0, const mkhe_ct* op1,
                        const mkhe_swk* const* rlk_b1, const mkhe_swk* const* rlk_b2,
                        const mkhe_swk* const* rlk_d1, const mkhe_swk* const* rlk_d2, int with_c0, mkhe_ct* out,
                        mkhe_swk* x1, mkhe_swk* x2, mkhe_swk* y1, mkhe_swk* y2) {
    MKHE_TRY({ mark(ctx, op0, op1, out, x1, x2, y1, y2);
        if (!op0 || !op1 || !out || !rlk_b1 || !rlk_b2 || !rlk_d1 || !rlk_d2 || !x1 || !x2 || !y1 || !y2) throw Error("mkhe_bfv_mr_partial: null argument");
        auto b1 = swk_list(ctx, rlk_b1, op1->c.n); auto b2 = swk_list(ctx, rlk_b2, op1->c.n);
        auto d1 = swk_list(ctx, rlk_d1, op0->c.n); auto d2 = swk_list(ctx, rlk_d2, op0->c.n);
        need(ctx)->bfv_mr_partial(op0->c, op1->c, b1.data(), b2.data(), d1.data(), d2.data(), with_c0 != 0, false, out->c,
                                  x1->s.d, x2->s.d, y1->s.d, y2->s.d);
    })
}
int mkhe_bfv_mr_finish(mkhe_ctx* ctx, const mkhe_ct* op0, const mkhe_ct* op1, const mkhe_swk* x1, const mkhe_swk* x2,
                       const mkhe_swk* y1, const mkhe_swk* y2, const mkhe_swk* const* rlk_v, const mkhe_swk* crs_u, mkhe_ct* out) {
    MKHE_TRY({ mark(ctx, op0, op1, x1, x2, y1, y2, crs_u, out);
        if (!op0 || !op1 || !out || !x1 || !x2 || !y1 || !y2 || !rlk_v || !crs_u) throw Error("mkhe_bfv_mr_finish: null argument");
        auto v = swk_list(ctx, rlk_v, op0->c.n);
        need(ctx)->bfv_mr_finish(op0->c, op1->c, x1->s.d, x2->s.d, y1->s.d, y2->s.d, v.data(), crs_u->s, out->c);
    })
}

int mkhe_set_overlap(mkhe_ctx* ctx, int on) { MKHE_TRY({ need(ctx)->sync(); need(ctx)->overlap = on != 0; }) }
int mkhe_ntt_trace(mkhe_ctx* ctx, void* dev_buf) { need(ctx)->ntt_trace = (u64*)dev_buf; return 0; }
int mkhe_prof_enable(mkhe_ctx* ctx, int on) { MKHE_TRY(need(ctx)->prof_enable(on != 0)) }
int mkhe_ntt_choice(mkhe_ctx* ctx, long limbs, int decompose) {
    g_last_ctx = nullptr;
    try {
        Context* c = need(ctx);
        for (int lazy = 0; lazy < 2; ++lazy) {
            auto it = c->ntt_tune_.find((limbs << 2) | (decompose ? 2 : 0) | lazy);
            if (it != c->ntt_tune_.end() && it->second.decided >= 0) return it->second.decided;
        }
        return c->ntt_forced_ >= 0 ? c->ntt_forced_ : -1;
    }
    catch (const std::exception& e) { g_err = e.what(); return -2; }
    catch (...) { g_err = "mkhe: unknown error"; return -2; }
}
int mkhe_ctx_set_ntt_choice(mkhe_ctx* ctx, long limbs, int decompose, int choice) {
    MKHE_TRY({
        Context* c = need(ctx);
        if (choice < -1 || choice > 1) throw Error("mkhe: ntt choice must be -1 (measure), 0 (two-pass) or 1 (single-pass)");
        if (limbs <= 0) { c->ntt_forced_ = choice; for (auto& kv : c->ntt_tune_) c->ntt_reset(kv.second, choice); }
        else for (int lazy = 0; lazy < 2; ++lazy) c->ntt_reset(c->ntt_tune_[(limbs << 2) | (decompose ? 2 : 0) | lazy], choice);
    })
}
int mkhe_ctx_set_batch_lanes(mkhe_ctx* ctx, long min_limbs) { MKHE_TRY({ need(ctx)->batch_lanes_min_ = min_limbs; }) }
long long mkhe_pool_held_bytes(mkhe_ctx* ctx) {
    g_last_ctx = nullptr;
    try { return (long long)(need(ctx)->pool_held_words() * sizeof(u64)); }
    catch (const std::exception& e) { g_err = e.what(); return -1; }
    catch (...) { g_err = "mkhe: unknown error"; return -1; }
}
int mkhe_pool_trim(mkhe_ctx* ctx) { MKHE_TRY(need(ctx)->pool_trim_device()) }
int mkhe_f2_schedule_probe(int parties, int nb, int nslots, const long* weights, int grid, unsigned char* segs, int* parts) {
    static_assert(sizeof(F2Seg) == 8 && F2_SEGS == 3, "include/mkhe.h documents the record");
    int p = 0;
    if (!weights || !segs || grid == 0 || grid < -65536 || grid > 65536) { if (parts) *parts = 0; return 0; }
    try {
        const int n = grid > 0 ? f2_build_schedule(parties, nb, nslots, weights, grid, reinterpret_cast<F2Seg*>(segs), &p)
                               : f2_plan_schedule(parties, nb, nslots, weights, -grid, reinterpret_cast<F2Seg*>(segs), &p);
        if (parts) *parts = p;
        return n;
    } catch (...) { if (parts) *parts = 0; return 0; }
}
int mkhe_prof_nclass(void) { return Context::PROF_NCLASS; }
const char* mkhe_prof_name(int cls) {
    static const char* names[] = {"ntt_fwd_kernel<N,1,true>  (Decompose, q<2^57)", "ntt_fwd_kernel<N,0,true>  (Decompose, q>=2^57)",
                                  "ntt_fwd_kernel<N,2,true>  (Decompose, both modulus classes in one persistent launch)",
                                  "ntt16_fwd_kernel<true>  (Decompose, 16 coefficients per thread, two workgroups per CU)", "ntt16_fwd_kernel<false>",
                                  "ntt32_fwd_kernel<true>  (Decompose, ONE pass per limb: 32 coefficients per thread, one workgroup per CU)", "ntt32_fwd_kernel<false>",
                                  "ntt14_fwd_split_kernel  (N = 2^16 Decompose after decomp_spread4_kernel: four one-pass 2^14-point sub-transforms per limb)",
                                  "ntt_fwd_kernel<N,1,false>", "ntt_fwd_kernel<N,0,false>", "ntt_inv_kernel<N>",
                                  "inner_product_kernel", "ext_inner_kernel", "moddown[_batch]_kernel", "tensor_kernel", "basis_conv_kernel", "decomp_spread_kernel",
                                  "ntt16_f2_kernel  (Decompose of the t_i with the step-F2 products in registers)", "other"};
    static_assert(sizeof(names) / sizeof(names[0]) == Context::PROF_NCLASS, "one name per timing class");
    return (cls >= 0 && cls < Context::PROF_NCLASS) ? names[cls] : "";
}
int mkhe_prof_collect(mkhe_ctx* ctx, double* ms, long* launches, double* alg_bytes) {
    MKHE_TRY(need(ctx)->prof_collect(ms, launches, alg_bytes))
}

}  // extern "C"
