// C ABI of libparq_hip.so (include/parq_hip.h): handle, weight arena, workspace carving and
// the host-side orchestration of the kernel chain.  Nothing here synchronises with the
// device, allocates device memory or touches torch; the caller owns every buffer.
#include "../../include/parq_hip.h"
#include "common.hpp"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

using namespace parq;

namespace {
// attention mode 4: smallest row sum of probabilities (relative to the row's reference maximum) it keeps.  Measured on the kernels at
// BASELINE cfg 3's size (profiles/r05_split8_guard_sweep.txt): rows down to a sum of 255 keep the mode within 2.4e-5 of mode 1 on smooth
// (FPN-like) features and within 6e-6 on white noise; at sums of 75 .. 87 smooth features are at 3.5e-5 (the round-4 threshold of 64 let
// those through).  The benchmark's synthetic workload: smallest sum 3200 .. 4600.
constexpr float kPeakyL = 256.f;

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) return fail(PARQ_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

constexpr int64_t kAlign = 64;   // floats (256 B)
int64_t align_up(int64_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

struct WeightRef { const float* p; int64_t n; };

// offsets (in floats) into the packed arena
struct LayerW {
    int64_t self_in_w, self_in_b, self_out_w, self_out_b;
    int64_t cross_in_w, cross_in_b, cross_out_w, cross_out_b;
    int64_t lin1_w, lin1_b, lin2_w, lin2_b;
    int64_t n1_w, n1_b, n2_w, n2_b, n3_w, n3_b;
    int64_t kv_whi, kv_wlo;           // fp16 hi/lo split of in_proj_weight[C:3C] (each 2C*C halfs)
    // the position MLP's last layer folded into its two consumers (inference): (x + h W2^T + b2) W^T = x W^T + h (W W2)^T + W b2
    int64_t self_in_w2, self_in_b2;   // [3C][C]: rows < 2C = W_qk W2, rows >= 2C zero | [3C]: b_qk + W_qk b2, then b_v
    int64_t cross_q_w2, cross_q_b2;   // [C][C] = W_q W2 | [C] = b_q + W_q b2
    // norm1 pushed through the cross-attention query projection (chain.hip seam_tile; inference):
    //   q  = rstd1 (U - mean1 q_s) + V:   U = sa (Wq g1 Wo_s)^T + tgt (Wq g1)^T + qu_b,   V = pe_h cross_q_w2^T + qv_b
    int64_t qg_w, qo_w, qu_b, q_s, qv_b;       // [C][C] Wq diag(g1) | [C][C] (Wq diag(g1)) Wo_self | [C] (Wq diag(g1)) bo_self | [C] row sums | [C] cross_q_b2 + Wq beta1
};
struct Arena {
    std::vector<LayerW> layers;
    int64_t refpoint, pe0_w, pe0_b, pe2_w, pe2_b;
    int64_t heads1_w, heads1_b;       // [NH1][C]: centre.0 | rotation.0 | sem_cls | size | zero pad
    int64_t gn1_g, gn1_b;             // [2][C]  (centre, rotation) GroupNorm after layer 0
    int64_t heads2_w;                 // [2][C][C]  centre.4 | rotation.4
    int64_t gn2_g, gn2_b;             // [2][C]
    int64_t heads3_w, heads3_b;       // [2][6][C], [2][6]: centre.8 padded to 6 rows | rotation.8
    int64_t mean_sizes, dim_t;
    int64_t early_begin = 0, early_end = 0;   // [early_begin, early_end): gradients final after phase 1 of parq_backward (nl = 1)
    int64_t rowmajor_total;           // end of the tensors above = size of the gradient arena (same layout)
    int64_t tile_off;                 // start of the tile-ordered mirror: matrix at offset o has its chain.hip copy at tile_off + o
    int64_t half_off = -1;            // start of the fp16 hi / lo mirror (LinearArgs::Wh) or -1: widths whose chain contracts over >= 768
    int64_t hscale_off = -1;          // its column scales: matrix at offset o has them at hscale_off + hscale_slot(o)
    int64_t total;
};

struct Workspace {
    int64_t T_cl, kv, ref, ref_next, emb, pe_h, pos, tgt, qkv, attn, xa, qc, xb, ffn, xc;
    int64_t h1, h2, gn_sums, ln1, ln2, flash;     // gn_sums: [2 layers][B][2 heads][2] fp64 moments; ln*: [M][2]
    int64_t kvc, flags;               // split-fp16 K/V cache, int flags (overflow)
    int64_t seam_flags, lnp1;         // the norm1 seam inside one launch (chain.hip seam_tile): flags [M / 16][4], fp64 partial row sums of xa ([M][C/64][2])
    int64_t xsplit;                   // fp16 hi/lo copy of the tokens for the large-C K/V projection (kvproj_big.hip), else empty
    int64_t tok32;                    // attention mode 0 with 16-bit tokens: their exact fp32 widening, read by the fp32 K/V projection; else empty
    int64_t cam, ind;                 // a captured forward: this call's cameras and pointer block (common.hpp CallPtrs), left by its prologue
    int64_t total;
    int self_split, cross_split;
    // batch-invariant inference (parq_set_batch_invariant; carve_workspace's `inv`): every launch geometry is chosen as for one scene.
    // gn_inv: the GroupNorm moments with gn_slots slots per (scene, head) — one per 16 x 16 sub-tile of a scene's block — behind every
    // buffer of the default layout, so that what parq_prepare leaves in a workspace sits at the same offsets under either setting
    bool inv;
    int gn_slots;
    int64_t gn_inv;
    // per-iteration activations live in [iter_begin, iter_end); a training forward keeps one copy per iteration:
    // iteration k > 0 uses the same offsets shifted by stash + (k - 1) * (iter_end - iter_begin) - iter_begin
    int64_t sa, ln3, lse_s, lse_c, refk;
    int64_t iter_begin, iter_end, stash;
    // backward scratch (training workspace only)
    int64_t g_a, g_b, g_c, g_pos, g_tmp, g_ffh, g_h1, g_h2, g_z, g_act, g_h3, g_qkv, g_emb, g_ref, g_D, g_bs, wT, g_kv, g_dqp, g_drop, kv_train, g_do, g_res, g_dq, g_Dall, g_kvmax, g_pack, g_mat;
    int64_t g_det, g_det_floats;      // deterministic mode: scratch of the fixed-order reductions (common.hpp DetScratch), else empty
    int64_t g_set_stride;             // floats between two copies of the per-iteration backward scratch [g_a, g_drop]
    int g_sets;                       // copies of it: iterations of the batched backward run on that many streams at once
    bool bwd_batched;                 // cross-attention backward of all iterations in one launch (shared layer weights, split cache)
    int64_t train_total;
    int64_t shift(int k) const { return k == 0 ? 0 : stash + (int64_t)(k - 1) * (iter_end - iter_begin) - iter_begin; }
};

struct ProfEvent { hipEvent_t a, b; int which; };

// what the last call that ran an iteration in a workspace left there (host-side note, keyed by the workspace address): the layer whose
// K cache that iteration read and the settings the cache was written under.  parq_attention_map reads "cross_q" and that cache.
// A call that rewrites a workspace drops its note on entry and leaves a new one only once it has enqueued everything; the handle keeps
// the kMapRecs most recently written notes (it never learns that a workspace was freed: a note for a freed address is only ever
// replaced by the next call that runs at that address).
struct MapRec {
    int B, V, h, w, li, mode, tok, state;     // state: 1 inference / stepping iteration, 2 training forward, 3 view-sharded iteration
    uint32_t safe;
    uint64_t seq;                             // order of writing: the oldest note is the one evicted
};
constexpr size_t kMapRecs = 256;

// what the K/V cache of a workspace was last built with, whole, by an inference forward (host-side note keyed by the workspace address,
// as MapRec): parq_forward_views projects a subset of the views only into a cache whose note equals the handle's present state.
// Dropped on entry by every call that rewrites the cache or the token copies next to it, written once a forward is enqueued whole.
struct CacheRec {
    int B, V, h, w, mode, tok, inv;
    uint32_t safe;
    const void* arena; uint64_t pack_gen;
    const int* mirror;                        // the range mirror word of that forward (NULL: none)
    uint64_t seq;
};
typedef std::vector<std::pair<int, int>> RowRuns;      // token-row ranges [first, second) of every scene, ascending and disjoint

}  // namespace

struct parq_ctx {
    parq_config cfg;
    int C, Q, H, dh, F, I, ncls, NH1, nl;
    ScaleBox sb;
    std::map<std::string, WeightRef> named;
    Arena ar;
    const float* arena = nullptr;     // device arena after pack
    bool packed = false;
    bool derived_valid = false;       // build_derived_weights ran since the last parq_pack_weights
    bool prepared = false;
    bool emb_valid = false;           // workspace emb holds pos2posemb3d of the chained reference points
    int ref_state = 0;                // 0: none, 1: ws.ref valid
    int attn_mode = 1;                // 0: fp32 MFMA, 1: split fp16x3, 2: fp16, 3: bf16 (1..3: head dims 64 and 256), 4: split with fp8 cross terms
    int kv16_state = 1;               // what the arena's 16-bit W_kv copy currently holds (same numbering)
    int tok_type = 0;                 // parq_set_token_type: element type of every scene's tokens (kTokF32 / kTokF16 / kTokBF16)
    int train_tok_type = 0;           // parq_set_train_token_type: the type parq_forward_train / parq_backward accept (they run when it equals tok_type)
    float drop_p = 0.f;               // training dropout (decoder layer, transformer_parq.py:339-386) and its base seed
    uint32_t drop_seed = 0;
    uint32_t site_seed(int k, int site) const { return rng_stream(drop_seed, (uint32_t)(k * 8 + site)); }
    // split K/V cache in use: head dim 64 (all cache modes) or head dim 256 in split mode (a head = 4 virtual heads of 64)
    bool cache_mode() const { return attn_mode >= 1 && (dh == 64 || dh == 256); }
    int vheads() const { return C / 64; }            // heads of the cache layout
    int terms() const { return attn_mode == 1 || attn_mode == 4 ? 3 : 1; }
    // mode 4 (flash_split8.hip) where its kernels apply — inference, head dim 64, d = 256, whole 64-key stages — and mode 1 otherwise:
    // 8 = the stage cache with fp8 cross-term planes (same size as the split cache for such N)
    // training: only where the backward reads the forward's cache itself (bwd_reads_cache: `stage_bwd`) — there is no fp32 rebuild from stages
    // per-head tiers (parq_set_head_tiers): heads of `safe_mask` run the fp16 x 3 kernel on the split layout inside a mode-4 forward
    // (inference only; a training forward with any safe head runs as mode 1, and so does a forward whose heads are all safe)
    int terms_for(int64_t N, bool train, bool stage_bwd = false) const {
        const bool m4 = attn_mode == 4 && (!train || stage_bwd) && C == 256 && flash_split8_supported(dh, (int)(N > INT32_MAX ? 0 : N));
        if (!m4 || safe_heads() == all_heads() || (train && safe_heads() != 0)) return terms();
        return 8;
    }
    uint32_t seam_epoch = 0;          // one value per seam launch of this handle (chain.hip seam_tile flags); 0 is never used
    uint32_t next_epoch() { if (++seam_epoch == 0) ++seam_epoch; return seam_epoch; }
    uint32_t safe_mask = 0;           // bit h: head h runs the fp16 x 3 kernel where the handle is in attention mode 4
    int peaky_poison = 0;             // mode-4 heads that meet a too-peaked row: write that iteration's outputs (and what follows) as NaN
    uint32_t all_heads() const { return H >= 32 ? 0xffffffffu : ((1u << H) - 1u); }
    uint32_t safe_heads() const { return safe_mask & all_heads(); }
    bool mixed_tiers(int64_t N, bool train, bool stage_bwd = false) const { return terms_for(N, train, stage_bwd) == 8 && safe_heads() != 0; }
    int w16_state() const { return attn_mode == 4 ? 1 : attn_mode; }      // what the 16-bit copy of W_kv has to hold
    int kind() const { return attn_mode == 3 ? kBF16 : kF16; }
    int* range_mirror = nullptr;      // host-visible word raised when outputs are poisoned (parq_set_range_mirror)
    int* progress_word = nullptr;     // host-visible word that receives progress_epoch once a forward can raise no more flags (parq_set_progress)
    int progress_epoch = 0;
    bool seam_fusion = false;         // parq_set_seam_fusion: in-launch hand-offs of the chain (off by default since round 6: every dependent stage its own launch)
    bool bwd_batched_env = true;      // parq_set_backward_batched (the parity test compares the two settings)
    int bwd_streams = 8;              // parq_set_backward_streams: iterations of the chain backward in flight at once (1 = in turn)
    bool deterministic = false;       // parq_set_deterministic: fixed-order reductions in parq_forward_train / parq_backward
    bool batch_invariant = false;     // parq_set_batch_invariant: inference launch geometry chosen as for one scene (training / sharded: ignored)
    float dim_t_host[128];            // 10000^(2*(i//2)/128): uploaded by parq_pack_weights from this persistent buffer (no stream sync)
    hipStream_t cap_stream = nullptr;       // parq_forward_capture records on a stream of the handle's own
    hipStream_t aux_stream[7] = {nullptr};  // batched backward: iterations 1 .. g_sets-1 (mod g_sets) of a phase run here, 0 on the caller's stream
    hipEvent_t fork_ev = nullptr, join_ev[7] = {nullptr};
    hipEvent_t bucket_done[2] = {nullptr, nullptr};   // parq_backward: gradient bucket 0 / 1 final on the caller's stream (parq_backward_wait_bucket)
    bool bucket_recorded = false;
    hipEvent_t iter_done[16] = {nullptr};   // parq_forward_train records one after every iteration (parq_wait_iteration)
    bool iter_recorded[16] = {false};
    bool profiling = false;
    std::vector<ProfEvent> events;
    double prof_ms[PARQ_PROF_COUNT] = {0};
    int64_t prof_n[PARQ_PROF_COUNT] = {0};
    std::map<const void*, MapRec> map_recs;       // parq_attention_map: the last iteration of every workspace this handle ran in
    void note_iteration(const void* wsp, const parq_scene* sc, int layer_num, int state) {
        if (!map_recs.count(wsp) && map_recs.size() >= kMapRecs) {
            auto oldest = map_recs.begin();
            for (auto it = map_recs.begin(); it != map_recs.end(); ++it)
                if (it->second.seq < oldest->second.seq) oldest = it;
            map_recs.erase(oldest);
        }
        map_recs[wsp] = MapRec{sc->B, sc->V, sc->h, sc->w, cfg.share_weights ? 0 : layer_num, attn_mode, tok_type, state, safe_heads(), ++map_seq};
    }
    uint64_t map_seq = 0;
    std::map<const void*, CacheRec> cache_recs;   // parq_forward_views: what the cache of a workspace was built with
    uint64_t pack_gen = 0;                        // counts parq_pack_weights calls
    void note_cache(const void* wsp, const parq_scene* sc) {
        if (!cache_recs.count(wsp) && cache_recs.size() >= kMapRecs) {
            auto oldest = cache_recs.begin();
            for (auto it = cache_recs.begin(); it != cache_recs.end(); ++it)
                if (it->second.seq < oldest->second.seq) oldest = it;
            cache_recs.erase(oldest);
        }
        cache_recs[wsp] = CacheRec{sc->B, sc->V, sc->h, sc->w, attn_mode, tok_type, batch_invariant ? 1 : 0, safe_heads(), arena, pack_gen, range_mirror, ++map_seq};
    }
};

namespace {

void build_arena(parq_ctx* c) {
    Arena& a = c->ar;
    int64_t off = 0;
    auto take = [&](int64_t n) { int64_t o = off; off += align_up(n); return o; };
    const int64_t C = c->C, F = c->F, Q = c->Q;
    // Order = when a tensor's GRADIENT is final inside parq_backward, so that data-parallel training can all-reduce the arena
    // in two contiguous buckets (parq_grad_bucket): first everything that is only complete at the END of the backward (phase 2
    // of the iterations and the hoisted K/V projection: reference points, position MLP, both in-projections, self out-proj,
    // norm1), then what is complete after PHASE 1 (cross out-proj, FFN, norm2, norm3, all heads) — with shared layer weights
    // (nl = 1) the split is one offset, `early_begin`; the derived inference tensors (no gradient) come last.
    a.refpoint = take(Q * 3);
    a.pe0_w = take(C * 384); a.pe0_b = take(C); a.pe2_w = take(C * C); a.pe2_b = take(C);
    a.layers.resize(c->nl);
    for (auto& L : a.layers) {
        L.self_in_w = take(3 * C * C); L.self_in_b = take(3 * C);
        L.self_out_w = take(C * C);    L.self_out_b = take(C);
        L.cross_in_w = take(3 * C * C); L.cross_in_b = take(3 * C);
        L.n1_w = take(C); L.n1_b = take(C);
        if (&L == &a.layers.back()) a.early_begin = off;
        L.cross_out_w = take(C * C);   L.cross_out_b = take(C);
        L.lin1_w = take(F * C); L.lin1_b = take(F);
        L.lin2_w = take(C * F); L.lin2_b = take(C);
        L.n2_w = take(C); L.n2_b = take(C); L.n3_w = take(C); L.n3_b = take(C);
    }
    a.heads1_w = take((int64_t)c->NH1 * C); a.heads1_b = take(c->NH1);
    a.gn1_g = take(2 * C); a.gn1_b = take(2 * C);
    a.heads2_w = take(2 * C * C);
    a.gn2_g = take(2 * C); a.gn2_b = take(2 * C);
    a.heads3_w = take(2 * 6 * C); a.heads3_b = take(12);
    a.early_end = off;
    a.mean_sizes = take((int64_t)c->cfg.num_mean_sizes * 3);
    a.dim_t = take(128);
    for (auto& L : a.layers) {
        L.kv_whi = take(C * C); L.kv_wlo = take(C * C);
        L.self_in_w2 = take(3 * C * C); L.self_in_b2 = take(3 * C);
        L.cross_q_w2 = take(C * C); L.cross_q_b2 = take(C);
        L.qg_w = take(C * C); L.qo_w = take(C * C); L.qu_b = take(C); L.q_s = take(C); L.qv_b = take(C);
    }
    a.rowmajor_total = off;
    // tile-ordered copies of the matrices the per-iteration chain multiplies by (LinearArgs::Wp): same offsets, shifted
    a.tile_off = off;
    a.total = 2 * off;
    // fp16 hi / lo mirror for the fp16 x 3 chain tile (chain.hip chain_linear_h3_kernel: contractions over 1024 or 768 only)
    if (C % 256 == 0 && C >= 768) {
        a.half_off = 2 * off;
        a.hscale_off = (3 * off + 63) / 64 * 64;
        a.total = a.hscale_off + ((off + 255) / 256 + 63) / 64 * 64 + 64;
    }
}

// column scales of the fp16 hi / lo mirror: the matrix at arena offset o ([N][K], K >= 768) keeps its N scales at hscale_off + this
// (16-byte aligned; disjoint: the next matrix starts N K / 256 >= 3 N slots further)
inline int64_t hscale_slot(int64_t off) { return ((off >> 8) + 3) & ~(int64_t)3; }

bool chain_h3_on() {
    static const bool on = [] { const char* e = dev_env("PARQ_CHAIN_H3"); return !(e && e[0] == '0'); }();     // 0: fp32 MFMA tiles at every width (A/B)
    return on;
}

bool kvproj_big_on() {
    static const bool on = [] { const char* e = dev_env("PARQ_KVPROJ_BIG"); return !(e && e[0] == '0'); }();   // 0: keep the tiled kernel at C > 256 (A/B)
    return on;
}

// Training: the cross-attention backward of all recurrent iterations can run as ONE launch when the iterations share the layer
// weights (hence K / V) and the split-precision kernel applies (head dim 64, long key axis); parq_set_backward_batched(h, 0) restores the
// per-iteration launches.
int bwd_sets(int I) {          // concurrent iterations of the batched chain backward: up to 8
    return I < 1 ? 1 : (I > 8 ? 8 : I);
}
bool bwd_batched_ok(const parq_ctx* c, int64_t N);
// the batched cross-attention backward at head dim 64 takes K / V straight from the forward's 16-bit cache: no fp32 rebuild
// (kvsplit_to_f32: 0.57 ms and 1.5 GB of traffic per 4-scene step at cfg 3), no second copy of K / V in the training workspace
bool bwd_reads_cache(const parq_ctx* c, const Workspace& ws) { return ws.bwd_batched && c->cache_mode() && c->dh == 64 && c->nl == 1; }
bool bwd_batched_ok(const parq_ctx* c, int64_t N) {
    // head dim 64: the register-resident split kernel (long key axes); head dim 256: the composition from split-precision GEMMs
    return c->bwd_batched_env && c->nl == 1 && ((c->dh == 64 && N >= 2048) || c->dh == 256) && c->I > 1 && c->I <= 16;
}

// inv: carve for batch-invariant inference (the inference entry points pass the handle's setting; training and the view-sharded
// iteration always carve the default layout, whose buffers in front of `flash` lie at the same offsets)
int carve_workspace(const parq_ctx* c, int B, int V, int h, int w, Workspace* ws, bool inv) {
    const int64_t C = c->C, Q = c->Q, F = c->F;
    const int64_t M = (int64_t)B * Q;
    const int64_t N = (int64_t)V * h * w;
    int64_t off = 0;
    auto take = [&](int64_t n) { int64_t o = off; off += align_up(n); return o; };
    ws->T_cl = take((int64_t)B * V * 12 * 2);      // float64 poses
    const bool split_mode = c->cache_mode();
    ws->kv = take(split_mode ? 0 : (int64_t)c->nl * B * 2 * N * C);      // fp32 head-major K/V (fp32 mode only)
    ws->ref = take(M * 3); ws->ref_next = take(M * 3);
    ws->emb = take(M * 384); ws->pe_h = take(M * C); ws->pos = take(M * C);
    ws->tgt = take(M * C); ws->qkv = take(M * 3 * C); ws->attn = take(M * C);
    ws->xa = take(M * C); ws->qc = take(M * C);
    ws->xb = take(M * C); ws->ffn = take(M * F);
    ws->xc = take(M * C);
    ws->h1 = take(M * c->NH1); ws->h2 = take(M * 2 * C);
    ws->gn_sums = take((int64_t)2 * B * 4 * kGnSlots * 2);  // doubles: [2 layers][B][2 heads][kGnSlots][2]
    ws->ln1 = take(M * 2); ws->ln2 = take(M * 2); ws->ln3 = take(M * 2);
    ws->sa = take(M * C);
    ws->lse_s = take((int64_t)B * c->H * flash_lq_pad((int)Q)); ws->lse_c = take((int64_t)B * c->H * flash_lq_pad((int)Q));
    ws->refk = take(M * 3);
    ws->iter_begin = ws->emb; ws->iter_end = off;
    const int cus = device_num_cus();
    // key splits: as many as fill the chip with the call's (scene, head, query tile) triples — batch-invariant: with ONE scene's, so
    // that a scene's partials are the same sums whatever shares its call (the partial buffers below hold B times that many)
    const int Bg = inv ? 1 : B;
    ws->inv = inv;
    ws->self_split = flash_pick_splits(Bg, c->H, c->Q, c->Q, c->dh, cus);
    ws->cross_split = split_mode ? (c->dh == 256 ? flash_split256_pick_splits(Bg, c->H, c->Q, (int)N, cus)
                                                 : flash_split_pick_splits(Bg, c->H, c->Q, (int)N, cus))
                                 : flash_pick_splits(Bg, c->H, c->Q, (int)N, c->dh, cus);
    ws->kvc = take(split_mode ? (int64_t)(c->nl * kvsplit_cache_bytes(B, c->vheads(), (int)N, c->terms()) / sizeof(float)) : 0);
    ws->flags = take(64);
    ws->seam_flags = take((M / 16 + 1) * 4);         // directly behind `flags`: the forward prologue clears both in one go
    ws->lnp1 = take(M * (C / 64) * 4);
    ws->xsplit = take(split_mode && kvproj_big_on() ? (int64_t)kvproj_big_scratch_floats(B, (int)N, C) : 0);
    ws->tok32 = take(!split_mode && c->tok_type != kTokF32 ? (int64_t)B * N * C : 0);
    const size_t fs = flash_scratch_bytes(B, c->H, c->Q, c->dh, ws->self_split);
    size_t fc = flash_scratch_bytes(B, c->H, c->Q, c->dh, ws->cross_split);
    if (c->attn_mode == 4 && c->dh == 64 && c->H <= 16) {
        // per-head tiers: the mode-4 heads and the fp16 x 3 heads run as two launches, each with the key-split count that fills the
        // chip with ITS heads, each with its own partials — room for the worst division of the heads
        for (int nf = 1; nf < c->H; ++nf) {
            const size_t two = flash_scratch_bytes(B, nf, c->Q, c->dh, flash_split_pick_splits(Bg, nf, c->Q, (int)N, cus)) +
                               flash_scratch_bytes(B, c->H - nf, c->Q, c->dh, flash_split_pick_splits(Bg, c->H - nf, c->Q, (int)N, cus));
            fc = two > fc ? two : fc;
        }
    }
    ws->flash = take((int64_t)((fs > fc ? fs : fc) / sizeof(float)));
    ws->cam = take((int64_t)B * V * 6);
    ws->ind = take(16);                               // 8 pointers
    // batch-invariant: a slot for every 16 x 16 sub-tile of a scene's [Q][C] block (the producers store, never add; the consumers sum
    // the slots in slot order), in 64s for the consumers' lanes; never fewer than the default
    ws->gn_slots = kGnSlots;
    if (inv && Q % 16 == 0 && C % 16 == 0) {
        const int64_t sub = (Q / 16) * (C / 16);
        if (sub > kGnSlots) ws->gn_slots = (int)((sub + 63) / 64 * 64);
    }
    ws->gn_inv = take(inv ? (int64_t)2 * B * 4 * ws->gn_slots * 2 : 0);
    ws->total = off;
    // ---- training extras: activation stash of iterations 1..I-1, backward scratch
    ws->stash = take((int64_t)(c->I - 1) * (ws->iter_end - ws->iter_begin));
    const int64_t NH1 = c->NH1;
    const int64_t g_set_begin = off;
    ws->g_a = take(M * C); ws->g_b = take(M * C); ws->g_c = take(M * C); ws->g_pos = take(M * C); ws->g_tmp = take(M * C);
    ws->g_ffh = take(M * F); ws->g_h1 = take(M * NH1); ws->g_h2 = take(M * 2 * C); ws->g_z = take(M * 2 * C);
    ws->g_act = take(M * 2 * C); ws->g_h3 = take(M * 16); ws->g_qkv = take(M * 3 * C); ws->g_emb = take(M * 384);
    ws->g_ref = take(M * 3); ws->g_D = take((int64_t)B * c->H * flash_lq_pad((int)Q)); ws->g_bs = take((int64_t)B * 2 * 2 * 2);
    ws->g_drop = take(M * C);
    // Given the stash the iterations are independent (reference points are detached between them), and the chain backward of one
    // iteration is ~70 small dependent launches: in the batched backward up to 8 iterations run at once (measured 1 / 2 / 4 / 8 at once: 29.3 / 27.5 / 27.7 / 27.2 ms per step), each on its own stream
    // with its own copy of the scratch above (weight gradients meet in the arena through atomics).  Only where every dW product
    // takes the row-split kernel (its plain read-modify-write form and the 64 x 64-tile kernel are not safe for that).
    ws->g_set_stride = off - g_set_begin;
    // (deterministic mode: one stream — the fixed-order forms share one scratch and accumulate in place)
    ws->g_sets = (!c->deterministic && bwd_batched_ok(c, N) && c->dh == 64 && (int64_t)F * C < (1 << 19) && (int64_t)3 * C * C < (1 << 19) && true)
                     ? (bwd_sets(c->I) < c->bwd_streams ? bwd_sets(c->I) : c->bwd_streams) : 1;
    take((ws->g_sets - 1) * ws->g_set_stride);
    // transposed weight copies of one layer: heads1 [C][NH1], heads2 2x[C][C], lin1^T [C][F], lin2^T [F][C],
    // cross_out^T, cross_q^T, self_out^T [C][C] each, self_in^T [C][3C], pe2^T [C][C], pe0^T [384][C]
    ws->wT = take(C * NH1 + 2 * C * C + 2 * C * F + 3 * C * C + 3 * C * C + C * C + 384 * C);
    ws->g_kv = take((int64_t)c->nl * B * 2 * N * C);
    ws->bwd_batched = bwd_batched_ok(c, N);
    // fp32 K / V rebuilt from the 16-bit cache for the backward — not needed where the backward reads the cache (bwd_reads_cache)
    ws->kv_train = take(split_mode && !bwd_reads_cache(c, *ws) ? (int64_t)c->nl * B * 2 * N * C : 0);
    // batched cross-attention backward (see parq_backward): per-iteration dO, residual gradient, dQ and D rows, and one set of
    // dQ partials per iteration
    ws->bwd_batched = bwd_batched_ok(c, N);
    const int64_t nit = ws->bwd_batched ? c->I : 1;
    // (batched head-dim-64 backward: a workgroup of attn_bwd_split2_kernel keeps one slot for its group of key blocks)
    ws->g_dqp = take(nit * (int64_t)attn_bwd_dq_partial_floats(B, c->H, (int)Q, (int)N, c->dh, ws->bwd_batched && c->dh == 64));
    ws->g_do = take(ws->bwd_batched ? nit * M * C : 0);
    ws->g_res = take(ws->bwd_batched ? nit * M * C : 0);
    ws->g_dq = take(ws->bwd_batched ? nit * M * C : 0);
    ws->g_Dall = take(ws->bwd_batched ? nit * (int64_t)B * c->H * flash_lq_pad((int)Q) : 0);
    ws->g_pack = take(ws->bwd_batched ? (int64_t)attn_bwd_pack_floats(B, c->H, (int)Q, (int)nit) : 0);
    // head dims without a register-resident attention backward (not 32 / 64): score-matrix scratch of the materialised path
    {
        int64_t mat = (c->dh == 64 || c->dh == 32) ? 0 : (int64_t)attn_bwd_mat_scratch_floats((int)Q, (int)(N > Q ? N : Q), c->dh);
        if (ws->bwd_batched && c->dh == 256) {        // S^T / dP^T of all iterations of one (scene, head): 3.1 GB at cfg 3
            const int64_t b256 = (int64_t)attn_bwd_batched256_scratch_floats(c->I, (int)Q, (int)N);
            mat = b256 > mat ? b256 : mat;
        }
        ws->g_mat = take(mat);
    }
    ws->g_kvmax = take(4);                            // [0] bits of max |dK|, |dV| (batched backward), [1] the derived scale
    // deterministic mode: one scratch shared by the fixed-order forms (each consumes its partials before the next launch writes them):
    // row-split slabs, the gather records of project + sample, dQ partials of the short-key attention backward, GroupNorm block sums
    ws->g_det_floats = 0;
    if (c->deterministic) {
        int64_t dq = c->dh == 64 ? det_attn_dq_floats(B, c->H, (int)Q, (int)Q) : 0;
        if (c->dh == 64 && N < 2048) {
            const int64_t dqc = det_attn_dq_floats(B, c->H, (int)Q, (int)N);
            dq = dqc > dq ? dqc : dq;
        }
        int64_t other = (int64_t)B * 2 * ceil_div64(Q * C, 1024) * 4;              // GroupNorm backward block sums
        if (dq > other) other = dq;
        if (ws->bwd_batched || (c->cache_mode() && C % 256 == 0)) {                // row ranges of the split-precision dW_kv / dQ slices
            const int64_t kv = det_kvbwd_floats();
            if (kv > other) other = kv;
        }
        ws->g_det_floats = det_scratch_floats(M * V, other);
    }
    ws->g_det = take(ws->g_det_floats);
    ws->train_total = off;
    return PARQ_OK;
}

// the tokens as the backward reads them: the caller's rows in the handle's token type, or — attention mode 0 / head dims without the
// split cache, where the training forward widened 16-bit tokens into the workspace (do_prepare) — that fp32 copy
const void* bwd_tokens(const parq_ctx* c, const parq_scene* sc, const float* wsp, const Workspace& ws, int* type) {
    if (c->tok_type != kTokF32 && !c->cache_mode()) {
        *type = kTokF32;
        return wsp + ws.tok32;
    }
    *type = c->tok_type;
    return sc->tokens;
}

int check_scene(const parq_ctx* c, const parq_scene* s) {
    if (!s) return fail(PARQ_ERR_ARG, "scene is NULL");
    if (s->B < 1 || s->V < 1 || s->h < 2 || s->w < 2) return fail(PARQ_ERR_ARG, "bad scene dims B=%d V=%d h=%d w=%d", s->B, s->V, s->h, s->w);
    if (!s->tokens || !s->camera || !s->T_camera_pseudoCam || !s->T_world_pseudoCam || !s->T_world_local)
        return fail(PARQ_ERR_ARG, "scene has a NULL tensor");
    if ((int64_t)s->B * c->Q > (1 << 22)) return fail(PARQ_ERR_ARG, "B*Q too large");
    return PARQ_OK;
}

struct Prof {
    parq_ctx* c; hipStream_t s; int which; hipEvent_t a = nullptr, b = nullptr;
    Prof(parq_ctx* c_, hipStream_t s_, int w) : c(c_), s(s_), which(w) {
        if (c->profiling) {
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { a = b = nullptr; return; }
            (void)hipEventRecord(a, s);
        }
    }
    ~Prof() {
        if (a && b) {
            (void)hipEventRecord(b, s);
            c->events.push_back({a, b, which});
        }
    }
};

LinearArgs lin(const float* X, int64_t ldx, const float* W, int64_t ldw, const float* bias, float* Y, int64_t ldy,
               int M, int N, int K) {
    LinearArgs a;
    memset(&a, 0, sizeof(a));
    a.X = X; a.ldx = ldx; a.W = W; a.ldw = ldw; a.bias = bias; a.Y = Y;
    a.M = M; a.N = N; a.K = K;
    a.rows_per_batch = M; a.y_batch = 0; a.y_row = ldy; a.col_blk = N; a.y_blk = 0;
    return a;
}

// the arena's 16-bit copy of W_kv follows the attention mode: hi/lo split, or one round-to-nearest fp16 / bf16 copy
int settle_weight_state(parq_ctx* c, hipStream_t s) {
    if (c->cache_mode() && c->kv16_state != c->w16_state()) {
        const float* A = c->arena;
        const int C = c->C;
        for (int li = 0; li < c->nl; ++li) {
            const LayerW& L = c->ar.layers[li];
            float* Aw = const_cast<float*>(A);
            if (c->terms() == 3) HIPCHK(launch_split_f32(A + L.cross_in_w + C * C, Aw + L.kv_whi, Aw + L.kv_wlo, 2 * C * C, s));
            else HIPCHK(launch_cvt16(A + L.cross_in_w + C * C, Aw + L.kv_whi, 2 * C * C, c->kind(), s));
        }
        c->kv16_state = c->w16_state();
    }
    return PARQ_OK;
}

// which kernel projects K / V in cache mode, hence what a row range is aligned to (kvproj_big.hip: a 32-key cache block)
bool kvproj_uses_big(const parq_ctx* c, int B, int64_t N) { return kvproj_big_on() && kvproj_big_scratch_floats(B, (int)N, c->C) > 0; }
int kvproj_granule(const parq_ctx* c, int B, int64_t N) { return kvproj_uses_big(c, B, N) ? 32 : kvproj_split_granule(c->C); }

// runs (parq_forward_views): the token rows of every scene whose K / V are projected, nullptr = all of them.  Cache modes only: one
// launch per layer and run; attention mode 0 (no cache) projects everything unless the list is empty.
int do_prepare(parq_ctx* c, const parq_scene* sc, float* wsp, const Workspace& ws, hipStream_t s, bool train = false,
               const parq_outputs* call_outs = nullptr, bool forward_call = false, const RowRuns* runs = nullptr) {
    const float* A = c->arena;
    const int B = sc->B, V = sc->V;
    const int64_t N = (int64_t)V * sc->h * sc->w;
    const int C = c->C;
    {
        // T_camera_local (float64), sigmoid(refpoint) tiled over the scenes, its sine embedding for iteration 0 and the cleared range
        // flags: one launch
        Prof p(c, s, PARQ_PROF_OTHER);
        // call_outs (parq_forward_replay): the launch also leaves this call's token / output pointers and cameras in the workspace for
        // the recorded iterations (common.hpp CallPtrs)
        PrologueCall pc;
        memset(&pc, 0, sizeof(pc));
        if (forward_call) {             // this call's epoch (the progress word's value once no flag can follow, LinearArgs::pub_epoch)
            pc.ind = reinterpret_cast<const void**>(wsp + ws.ind);
            pc.ptrs.p[7] = reinterpret_cast<const void*>((uintptr_t)(unsigned)c->progress_epoch);
        }
        if (call_outs) {
            pc.cam_src = sc->camera; pc.cam_dst = wsp + ws.cam; pc.ncam = B * V * 6;
            pc.ind = reinterpret_cast<const void**>(wsp + ws.ind);
            pc.ptrs.p[0] = sc->tokens; pc.ptrs.p[1] = call_outs->pred_logits; pc.ptrs.p[2] = call_outs->center_unnormalized;
            pc.ptrs.p[3] = call_outs->size_unnormalized; pc.ptrs.p[4] = call_outs->ortho6d; pc.ptrs.p[5] = call_outs->sem_cls_prob;
            pc.ptrs.p[6] = call_outs->coord_pos;
        }
        // a forward that skips rows of the projection (parq_forward_views with a subset) keeps flag word 0 as the forward before it left
        // it: the range flag comes from the projection, so one raised by the forward that projected the skipped rows — possibly still
        // in flight, its mirror word not yet raised for the host to see — poisons this forward too and is published again, in stream order
        const int keep0 = runs ? 1 : 0;
        HIPCHK(launch_forward_prologue(sc->T_camera_pseudoCam, sc->T_world_pseudoCam, sc->T_world_local, B, V,
                                       reinterpret_cast<double*>(wsp + ws.T_cl), A + c->ar.refpoint, c->Q, wsp + ws.ref, A + c->ar.dim_t,
                                       wsp + ws.emb, wsp + ws.flags + keep0, (int)(ws.lnp1 - ws.flags) - keep0, s,      // the 64 flag words and the seam flags behind them
                                       pc.ind ? &pc : nullptr));
    }
    // hoisted K/V in-projection of the memory tokens: one GEMM per distinct layer,
    // written head-major [b][{K heads, V heads}][N][dh] so the attention kernel streams contiguous panels
    if ((int64_t)B * N > (int64_t)INT32_MAX) return fail(PARQ_ERR_ARG, "B*N too large");
    { const int rc = settle_weight_state(c, s); if (rc) return rc; }
    const RowRuns whole(1, std::make_pair(0, (int)N));
    const RowRuns& rr = runs ? *runs : whole;
    for (int li = 0; li < c->nl && !rr.empty(); ++li) {
        Prof p(c, s, PARQ_PROF_KV_PROJ);
        const LayerW& L = c->ar.layers[li];
        if (c->cache_mode()) {
            char* cache = reinterpret_cast<char*>(wsp + ws.kvc) + (size_t)li * kvsplit_cache_bytes(B, c->vheads(), (int)N, c->terms());
            for (const auto& r : rr) {
                if (kvproj_uses_big(c, B, N))
                    HIPCHK(launch_kvproj_big(sc->tokens, A + L.kv_whi, A + L.kv_wlo, A + L.cross_in_b + C, B, (int)N, C, cache,
                                             reinterpret_cast<int*>(wsp + ws.flags), wsp + ws.xsplit, s, c->terms(), c->kind(), c->tok_type,
                                             r.first, r.second));
                else
                    HIPCHK(launch_kvproj_split(sc->tokens, A + L.kv_whi, A + L.kv_wlo, A + L.cross_in_b + C, B, (int)N, C, c->vheads(),
                                               cache, reinterpret_cast<int*>(wsp + ws.flags), s,
                                               c->mixed_tiers(N, train, train && bwd_reads_cache(c, ws)) ? 11 : c->terms_for(N, train, train && bwd_reads_cache(c, ws)),
                                               c->kind(), c->safe_heads(), c->tok_type, r.first, r.second));
            }
        } else {
            // 16-bit tokens: the fp32 GEMM reads their exact widening (once per forward, in front of the first layer)
            const float* X = sc->tokens;
            if (c->tok_type != kTokF32) {
                if (li == 0) HIPCHK(launch_widen_tokens(sc->tokens, wsp + ws.tok32, (int64_t)B * N * C, c->tok_type, s));
                X = wsp + ws.tok32;
            }
            LinearArgs a = lin(X, C, A + L.cross_in_w + (int64_t)C * C, C, A + L.cross_in_b + C,
                               wsp + ws.kv + (int64_t)li * B * 2 * N * C, 0, (int)(B * N), 2 * C, C);
            a.rows_per_batch = (int)N; a.y_batch = 2 * N * C; a.y_row = c->dh; a.col_blk = c->dh; a.y_blk = N * c->dh;
            if (ws.inv && !train) a.geom_M = (int)N;          // batch-invariant: the tile edge as for one scene's rows
            HIPCHK(launch_linear(a, 1, s));
        }
    }
    c->prepared = true;
    c->emb_valid = true;              // the prologue left pos2posemb3d(ws.ref) in ws.emb
    c->ref_state = 1;
    return PARQ_OK;
}

// Weights DERIVED from the packed tensors for the inference chain (chain.hip): the position MLP's last layer folded into its two
// consumers and the tile-ordered mirror of every matrix the chain multiplies by.  Built lazily by the first inference iteration
// after parq_pack_weights (a training loop re-packs every step and never reads them: its forward keeps the reference's layer order
// and row-major weights), on the caller's stream, into the caller's arena.
int build_derived_weights(parq_ctx* c, hipStream_t s) {
    float* A = const_cast<float*>(c->arena);
    const Arena& ar = c->ar;
    const int64_t C = c->C, F = c->F;
    // float64-accumulated products, rounded once
    for (int li = 0; li < c->nl; ++li) {
        const LayerW& L = c->ar.layers[li];
        HIPCHK(launch_fold_pos_weights(A + L.self_in_w, A + L.self_in_b, A + ar.pe2_w, A + ar.pe2_b, (int)(2 * C), (int)C, A + L.self_in_w2, A + L.self_in_b2, s));
        HIPCHK(hipMemcpyAsync(A + L.self_in_b2 + 2 * C, A + L.self_in_b + 2 * C, (size_t)C * sizeof(float), hipMemcpyDeviceToDevice, s));   // b_v unchanged
        HIPCHK(launch_fold_pos_weights(A + L.cross_in_w, A + L.cross_in_b, A + ar.pe2_w, A + ar.pe2_b, (int)C, (int)C, A + L.cross_q_w2, A + L.cross_q_b2, s));
        // norm1 pushed through the cross-attention query projection (LayerW)
        HIPCHK(launch_ln_fold(A + L.cross_in_w, A + L.cross_q_b2, A + L.n1_w, A + L.n1_b, (int)C, (int)C, A + L.qg_w, A + L.q_s, A + L.qv_b, s));
        HIPCHK(launch_matmul_fold(A + L.qg_w, A + L.self_out_w, A + L.self_out_b, (int)C, (int)C, A + L.qo_w, A + L.qu_b, s));
    }
    // tile-ordered mirror of the chain's matrices (chain.hip: one contiguous KB per wave-wide fragment load)
    {
        const int64_t T = ar.tile_off;
        auto tile = [&](int64_t off, int64_t N, int64_t K) { return launch_pack_w_tiles(A + off, K, (int)N, (int)K, A + T + off, s); };
        for (int li = 0; li < c->nl; ++li) {
            const LayerW& L = c->ar.layers[li];
            HIPCHK(tile(L.self_in_w, 3 * C, C)); HIPCHK(tile(L.self_out_w, C, C));
            HIPCHK(tile(L.cross_in_w, C, C));                                      // the query rows (K / V rows: kv_whi / kv_wlo)
            HIPCHK(tile(L.cross_out_w, C, C));
            HIPCHK(tile(L.self_in_w2, 3 * C, C)); HIPCHK(tile(L.cross_q_w2, C, C));
            HIPCHK(tile(L.qg_w, C, C)); HIPCHK(tile(L.qo_w, C, C));
            if (F % 16 == 0) { HIPCHK(tile(L.lin1_w, F, C)); HIPCHK(tile(L.lin2_w, C, F)); }
        }
        HIPCHK(tile(ar.pe0_w, C, 384)); HIPCHK(tile(ar.pe2_w, C, C));
        if (c->NH1 % 16 == 0) HIPCHK(tile(ar.heads1_w, c->NH1, C));
        HIPCHK(tile(ar.heads2_w, C, C)); HIPCHK(tile(ar.heads2_w + C * C, C, C));
    }
    if (ar.half_off >= 0) {
        const int64_t H = ar.half_off, SC = ar.hscale_off;
        // gamma / beta / bias: the LayerNorm in front of the launch that multiplies by this matrix, folded (chain.hip pack_w_half_kernel):
        // gamma into the mirror unless an addend follows the LayerNorm, W beta + bias into the N floats behind the column scales
        auto half = [&](int64_t off, int64_t N, int64_t K, const float* gamma = nullptr, const float* beta = nullptr, const float* bias = nullptr) {
            if (N % 16 != 0 || !(K == 1024 || K == 768)) return hipSuccess;
            float* scp = A + SC + hscale_slot(off);
            return launch_pack_w_half(A + off, K, (int)N, (int)K, A + H + off, scp, s, gamma, beta, bias, beta ? scp + N : nullptr);
        };
        for (int li = 0; li < c->nl; ++li) {
            const LayerW& L = c->ar.layers[li];
            HIPCHK(half(L.self_in_w, 3 * C, C)); HIPCHK(half(L.self_out_w, C, C));
            HIPCHK(half(L.cross_in_w, C, C, nullptr, A + L.n1_b, A + L.cross_in_b));                 // q rows: norm1, then + pos
            HIPCHK(half(L.cross_out_w, C, C));
            HIPCHK(half(L.lin1_w, F, C, A + L.n2_w, A + L.n2_b, A + L.lin1_b)); HIPCHK(half(L.lin2_w, C, F));
        }
        HIPCHK(half(ar.pe2_w, C, C));
        if (c->nl == 1) HIPCHK(half(ar.heads1_w, c->NH1, C, A + ar.layers[0].n3_w, A + ar.layers[0].n3_b, A + ar.heads1_b));      // one norm3 in front of the shared heads
        else HIPCHK(half(ar.heads1_w, c->NH1, C));                     // a norm3 per layer: no fold (that launch keeps the fp32 tile)
        HIPCHK(half(ar.heads2_w, C, C)); HIPCHK(half(ar.heads2_w + C * C, C, C));
    }
    c->derived_valid = true;
    return PARQ_OK;
}

// shift: offset (floats) of this iteration's activation copy (0 in inference: every iteration reuses one set);
// emb_next: where the decode kernel leaves the next iteration's sine embedding; train: also keep what backward needs
// View-sharded scenes (parq_iterate_sharded): an iteration runs in three phases around two exchanges the caller performs.
//   phase bit 1: position MLP + project/sample of the LOCAL views -> `out` = [M*C undivided sums | M valid-view counts]
//   phase bit 2: `in` = the ranks' pairs added up -> tgt; self-attention block, cross-attention over the LOCAL keys ->
//                `out` = [M*C normalised attention outputs | B*H*Lq_pad log2 log-sum-exp rows]
//   phase bit 4: `in` = `nranks` such records -> merged attention output; cross out-proj, FFN, heads, decode
// mask 7 with in = out = nullptr is the ordinary iteration.
struct ShardIO { int mask = 7; const float* in = nullptr; float* out = nullptr; int nranks = 1; };

int do_iterate(parq_ctx* c, const parq_scene* sc, float* wsp, const Workspace& ws, int layer_num, const float* ref,
               bool emb_valid, const parq_outputs* o, float* ref_out, hipStream_t s, int64_t shift = 0,
               float* emb_next = nullptr, bool train = false, const ShardIO& sh = ShardIO(), int64_t captured_row0 = -1,
               bool last_of_forward = false) {
    // captured_row0 >= 0 (parq_forward_capture): the iteration is being RECORDED — tokens, cameras and the six outputs are taken from the
    // workspace's CallPtrs block / camera copy that the prologue of every replay fills in (`sc->tokens`, `sc->camera`, `o` are unused);
    // captured_row0 = first output row of this iteration (k * B * Q)
    const void* const* ind = captured_row0 >= 0 ? reinterpret_cast<const void* const*>(wsp + ws.ind) : nullptr;
    const float* cam_in = ind ? wsp + ws.cam : sc->camera;
    const int64_t row0 = captured_row0 >= 0 ? captured_row0 : 0;
    float* wi = wsp + shift;
    const bool sharded = sh.mask != 7;
    if (!emb_next) emb_next = wi + ws.emb;
    const float dp = train ? c->drop_p : 0.f;          // dropout exists in training only (nn.Dropout / MHA dropout)
    const float* A = c->arena;
    const Arena& ar = c->ar;
    if (!train && !c->derived_valid) { const int rc = build_derived_weights(c, s); if (rc) return rc; }
    // tile-ordered mirror of the chain's matrices (LinearArgs::Wp); the training forward reads the row-major tensors
    const float* TP = train ? nullptr : A + ar.tile_off;
    // fp16 hi / lo mirror (LinearArgs::Wh: the fp16 x 3 tile of chain.hip for contractions over 1024 / 768) — inference, every attention
    // mode but the exact-fp32 one (mode 0 keeps fp32 MFMA products in the chain as well)
    const bool h3 = !train && ar.half_off >= 0 && c->attn_mode != 0 && chain_h3_on();
    // fold: what build_derived_weights folded of the LayerNorm in front of this launch (LinearArgs::wh_fold)
    auto halfw = [&](LinearArgs& la, int64_t off, int fold = 0) {
        if (h3) {
            la.Wh = A + ar.half_off + off; la.wh_scale = A + ar.hscale_off + hscale_slot(off);
            if (fold) { la.wh_bias = la.wh_scale + la.N; la.wh_fold = fold; }
        }
    };
    const int li = c->cfg.share_weights ? 0 : layer_num;
    const LayerW& L = ar.layers[li];
    const int B = sc->B, C = c->C, Q = c->Q, H = c->H, dh = c->dh, F = c->F;
    const int M = B * Q;
    const int64_t N = (int64_t)sc->V * sc->h * sc->w;
    const float eps = 1e-5f;
    // batch-invariant inference (parq_set_batch_invariant): every launcher below chooses its geometry from ONE scene — Q rows, one scene's
    // (head, query tile) count — and the GroupNorm moments keep a slot per sub-tile of a scene's block (Workspace::gn_inv)
    const bool inv = ws.inv && !train && !sharded;
    const int geomM = inv ? Q : 0, geomB = inv ? 1 : 0;
    const int nsl = inv ? ws.gn_slots : kGnSlots;
    // where the generic kernel (linear.hip) produces the moments it stores them per tile too; a query count that is no multiple of 16
    // lets its tiles straddle scenes: there the moments are recomputed in a fixed order behind the launch (as deterministic training does)
    const bool gn_own = inv && Q % 16 == 0 && C % 16 == 0;
    double* gn1 = reinterpret_cast<double*>(inv ? wsp + ws.gn_inv : wi + ws.gn_sums);          // [B][2][slots][2]
    double* gn2 = gn1 + (int64_t)B * 4 * nsl;
    auto lin = [geomM, nsl, gn_own](const float* X, int64_t ldx, const float* W, int64_t ldw, const float* bias, float* Y, int64_t ldy,
                                    int M_, int N_, int K_) {
        LinearArgs a = ::lin(X, ldx, W, ldw, bias, Y, ldy, M_, N_, K_);
        a.geom_M = geomM; a.gn_slots = nsl; a.gn_own = gn_own ? 1 : 0;
        return a;
    };
    // the two consumers of the position embedding, either with pos = pe2(h) as an addend on the A operand (reference order,
    // transformer_parq.py:372-377) or with the position MLP's last layer folded into them (second operand pair h x (W W2)^T)
    auto self_in_args = [&](bool fold) {
        LinearArgs a = lin(wi + ws.tgt, C, A + L.self_in_w, C, A + (fold ? L.self_in_b2 : L.self_in_b), wi + ws.qkv, 3 * C, M, 3 * C, C);
        a.ldx2 = C; a.x2_ncols = 2 * C; a.Wp = TP ? TP + L.self_in_w : nullptr; halfw(a, L.self_in_w);
        if (fold) { a.X2 = wi + ws.pe_h; a.W2 = A + L.self_in_w2; a.W2p = TP ? TP + L.self_in_w2 : nullptr; }
        else a.X2 = wi + ws.pos;
        return a;
    };
    auto cross_q_args = [&](bool fold) {
        LinearArgs a = lin(wi + ws.xa, C, A + L.cross_in_w, C, A + (fold ? L.cross_q_b2 : L.cross_in_b), wi + ws.qc, C, M, C, C);
        a.ln_gamma = A + L.n1_w; a.ln_beta = A + L.n1_b; a.ln_stats_out = wi + ws.ln1; a.norm_eps = eps;
        a.ldx2 = C; a.x2_ncols = C; a.Wp = TP ? TP + L.cross_in_w : nullptr; halfw(a, L.cross_in_w, 2);
        if (fold) { a.X2 = wi + ws.pe_h; a.W2 = A + L.cross_q_w2; a.W2p = TP ? TP + L.cross_q_w2 : nullptr; }
        else a.X2 = wi + ws.pos;
        return a;
    };
    // inference only (the backward differentiates the unfolded layers from the stashed pos), and only where chain.hip has the kernels
    // (profiles/r03_ab_fold_pos_mlp.txt)
    const bool fold_pos = !train && chain_linear_supported(self_in_args(true), 1) && chain_linear_supported(cross_q_args(true), 1);
    // the norm1 seam (self out-projection | cross-attention query projection) as ONE launch (chain.hip seam_tile): inference at d = 256
    // where the caller asks for it: parq_set_seam_fusion(h, 1).  Two launches are the default since round 6
    // (profiles/r05_ab_seam_q.txt; under graph replay: profiles/r06_ab_seam_q_under_graph_replay.txt)
    const bool seam_ok = !train && !sharded && fold_pos && C == 256 && TP != nullptr && (inv ? Q : M) % 16 == 0 && c->seam_fusion;

    if (sh.mask & 1) {
    // K3: sine embedding (written by the previous iteration's decode kernel when chained) -> position MLP
    // (transformer_parq.py:317)
    if (!emb_valid) { Prof p(c, s, PARQ_PROF_OTHER); HIPCHK(launch_posemb(ref, A + ar.dim_t, M, wi + ws.emb, s)); }
    LinearArgs pe1 = lin(wi + ws.emb, 384, A + ar.pe0_w, 384, A + ar.pe0_b, wi + ws.pe_h, C, M, C, 384);
    pe1.relu = 1; pe1.Wp = TP ? TP + ar.pe0_w : nullptr;
    float* sample_out = sharded ? sh.out : wi + ws.tgt;
    float* sample_cnt = sharded ? sh.out + (int64_t)M * C : nullptr;
    // the position MLP's first layer and project + sample are independent (both read only what the previous decode left): one
    // launch when the chain kernels apply; the profiled pass keeps them apart so that the per-kernel groups stay per kernel
    // (profiles/r03_ab_fused_pe1_sample.txt)
    bool fused = false;
    if (!train && !c->profiling) {
        const hipError_t e = launch_pe1_sample(pe1, sc->tokens, reinterpret_cast<const double*>(wsp + ws.T_cl), cam_in, ref, c->sb, B, sc->V,
                                               sc->h, sc->w, C, Q, sample_out, o->coord_pos, gn1, B * 8 * nsl, sample_cnt, s, ind, row0 * 3,
                                               c->tok_type);
        if (e == hipSuccess) fused = true;
        else if (e != hipErrorNotSupported) return fail(PARQ_ERR_HIP, "launch_pe1_sample failed: %s", hipGetErrorString(e));
    }
    {
        Prof p(c, s, PARQ_PROF_LINEAR);
        if (!fused) HIPCHK(launch_linear(pe1, 1, s));
        if (!fold_pos) {
            LinearArgs a = lin(wi + ws.pe_h, C, A + ar.pe2_w, C, A + ar.pe2_b, wi + ws.pos, C, M, C, C);
            a.Wp = TP ? TP + ar.pe2_w : nullptr; halfw(a, ar.pe2_w);
            HIPCHK(launch_linear(a, 1, s));
        }
    }
    // K4+K5: project + sample (transformer_parq.py:321); also clears this iteration's GroupNorm moments
    if (!fused) {
        Prof p(c, s, PARQ_PROF_PROJECT_SAMPLE);
        HIPCHK(launch_project_sample_f64(sc->tokens, reinterpret_cast<const double*>(wsp + ws.T_cl), cam_in, ref, c->sb,
                                         B, sc->V, sc->h, sc->w, C, Q, sample_out, o->coord_pos, gn1, B * 8 * nsl, s, sample_cnt, ind, row0 * 3,
                                         c->tok_type));
    }
    // view-sharded: this rank's fp16-range flag travels as the last float of the record (the caller's all-reduce adds the ranks')
    if (sharded) HIPCHK(launch_shard_range_flag(c->cache_mode() && c->kind() == kF16 ? reinterpret_cast<const int*>(wsp + ws.flags) : nullptr,
                                                sh.out + (int64_t)M * C + M, s));
    }   // phase bit 1
    if (sh.mask & 2) {
    if (sharded) {
        Prof p(c, s, PARQ_PROF_PROJECT_SAMPLE);
        HIPCHK(launch_sample_finalize(sh.in, sh.in + (int64_t)M * C, M, C, wi + ws.tgt, s, sh.in + (int64_t)M * C + M,
                                      c->cache_mode() && c->kind() == kF16 ? reinterpret_cast<int*>(wsp + ws.flags) : nullptr));
    }
    // K6: self-attention, q = k = tgt + pos, v = tgt (transformer_parq.py:372-376)
    {
        Prof p(c, s, PARQ_PROF_LINEAR);
        LinearArgs a = self_in_args(fold_pos);
        HIPCHK(launch_linear(a, 1, s));
    }
    FlashArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.B = B; fa.H = H; fa.Lq = Q; fa.dh = dh; fa.geom_B = geomB;
    fa.out = wi + ws.sa; fa.out_batch = (int64_t)Q * C; fa.out_row = C;
    {
        Prof p(c, s, PARQ_PROF_SELF_ATTN);
        if (dh <= 64 || ((dh == 128 || dh == 256) && Q <= 1024)) {
            // one launch: a workgroup = 16 queries of one head against all keys (the 256-key self-attention has no long axis to split)
            HIPCHK(launch_self_attn(wi + ws.qkv, 3 * C, B, H, Q, dh, wi + ws.sa, C, s, train ? wi + ws.lse_s : nullptr, dp,
                                    c->site_seed(layer_num, 0)));
        } else {
            fa.q = wi + ws.qkv;         fa.q_batch = (int64_t)Q * 3 * C; fa.q_head = dh; fa.q_row = 3 * C;
            fa.k = wi + ws.qkv + C;     fa.k_batch = fa.q_batch; fa.k_head = dh; fa.k_row = 3 * C;
            fa.v = wi + ws.qkv + 2 * C; fa.v_batch = fa.q_batch; fa.v_head = dh; fa.v_row = 3 * C;
            fa.Lk = Q; fa.nsplit = ws.self_split;
            const int64_t lp = flash_lq_pad(Q);
            fa.o_part = wsp + ws.flash;
            fa.m_part = fa.o_part + (int64_t)B * H * fa.nsplit * dh * lp;
            fa.l_part = fa.m_part + (int64_t)B * H * fa.nsplit * lp;
            fa.lse = train ? wi + ws.lse_s : nullptr;
            fa.drop_p = dp; fa.drop_seed = c->site_seed(layer_num, 0);
            HIPCHK(launch_flash(fa, s));
            HIPCHK(launch_flash_merge(fa, s));
        }
    }
    fa.out = sharded ? sh.out : wi + ws.attn;
    fa.lse = sharded ? sh.out + (int64_t)M * C : (train ? wi + ws.lse_c : nullptr);
    fa.drop_p = dp; fa.drop_seed = c->site_seed(layer_num, 2);
    bool fused_q = false;
    {
        // xa = tgt + self_attn @ Wo  (pre-LayerNorm; norm1 is applied by the consumers)
        Prof p(c, s, PARQ_PROF_LINEAR);
        LinearArgs a = lin(wi + ws.sa, C, A + L.self_out_w, C, A + L.self_out_b, wi + ws.xa, C, M, C, C);
        a.R = wi + ws.tgt; a.ldr = C; a.Wp = TP ? TP + L.self_out_w : nullptr; halfw(a, L.self_out_w);
        a.drop_p = dp; a.drop_seed = c->site_seed(layer_num, 1);
        if (seam_ok) {
            // ... and, in the same launch, the query projection behind norm1 (chain.hip seam_tile): q tiles contract sa, tgt and pe_h with
            // pack-time weight products and take norm1's statistics from the partial row sums the xa tiles publish
            a.lnp_out = reinterpret_cast<double*>(wi + ws.lnp1);
            a.lnp_flags = reinterpret_cast<unsigned*>(wsp + ws.seam_flags);
            a.lnp_epoch = c->next_epoch();
            SeamArgs q;
            memset(&q, 0, sizeof(q));
            q.X1 = wi + ws.sa; q.ldx1 = C; q.W1p = TP + L.qo_w;
            q.X2 = wi + ws.tgt; q.ldx2 = C; q.W2p = TP + L.qg_w;
            q.X3 = wi + ws.pe_h; q.ldx3 = C; q.W3p = TP + L.cross_q_w2;
            q.b1 = A + L.qu_b; q.srow = A + L.q_s; q.b2 = A + L.qv_b;
            q.Y = wi + ws.qc; q.ldy = C; q.M = M; q.N = C;
            q.part = a.lnp_out; q.flags = a.lnp_flags; q.epoch = a.lnp_epoch; q.nparts = C / 64; q.width = C; q.eps = eps;
            q.ln_out = wi + ws.ln1;               // norm1's statistics for the residual of the cross out-projection
            q.err = reinterpret_cast<int*>(wsp + ws.flags);
            const hipError_t e = launch_seam_q(a, q, s);
            if (e == hipSuccess) fused_q = true;
            else if (e != hipErrorNotSupported) return fail(PARQ_ERR_HIP, "launch_seam_q failed: %s", hipGetErrorString(e));
            a.lnp_out = nullptr; a.lnp_flags = nullptr;
        }
        if (!fused_q) {
            HIPCHK(launch_linear(a, 1, s));
            // K7: cross-attention query = (norm1(xa) + pos) @ Wq; publishes norm1's row statistics
            a = cross_q_args(fold_pos);
            HIPCHK(launch_linear(a, 1, s));
        }
    }
    bool merged = false;              // the cross-attention launches below already merged their partials (per-head tiers)
    {
        // dense cross-attention against the cached K/V (transformer_parq.py:377-382)
        Prof p(c, s, PARQ_PROF_CROSS_ATTN);
        fa.q = wi + ws.qc; fa.q_batch = (int64_t)Q * C; fa.q_head = dh; fa.q_row = C;
        fa.Lk = (int)N; fa.nsplit = ws.cross_split;
        // odd iterations sweep the K/V cache backwards (Infinity Cache reuse)
        fa.flags = (layer_num & 1) ? 2 : 0;
        const int64_t lp = flash_lq_pad(Q);
        fa.o_part = wsp + ws.flash;
        fa.m_part = fa.o_part + (int64_t)B * H * fa.nsplit * dh * lp;
        fa.l_part = fa.m_part + (int64_t)B * H * fa.nsplit * lp;
        if (c->cache_mode()) {
            const char* cache = reinterpret_cast<const char*>(wsp + ws.kvc) + (size_t)li * kvsplit_cache_bytes(B, c->vheads(), (int)N, c->terms());
            if (dh == 256) HIPCHK(launch_flash_split256(fa, cache, s, c->terms(), c->kind()));
            else if (c->terms_for(N, train, train && bwd_reads_cache(c, ws)) == 8) {
                // rows whose probability sum (relative to the row's reference maximum) is under kPeakyL are carried by too few keys for
                // this mode's error model: bit h of flags[1] (and of flags[8 + iteration]) -> bits 1 and 8 + h of
                // the range mirror -> the caller moves head h to the fp16 x 3 tier (parq_set_head_tiers)
                int* flg = reinterpret_cast<int*>(wsp + ws.flags);
                fa.peaky = sharded ? nullptr : flg + 1;
                fa.peaky_it = sharded ? nullptr : flg + 8 + (layer_num % 56);
                fa.peaky_min = sharded ? nullptr : flg + 2;
                fa.head_min = (sharded || H > 16) ? nullptr : flg + 32;    // flags[32 + h]: every head's smallest row sum of this forward
                fa.peaky_l = kPeakyL;
                const uint32_t safe = c->safe_heads();
                if (safe == 0) HIPCHK(launch_flash_split8(fa, cache, s));
                else {
                    // per-head tiers: two launches over complementary head sets, each with the split count that fills the chip with its
                    // heads and its own partials; every (scene, head) region of the cache spans the split layout's size (launch_kvproj_split)
                    FlashArgs f8 = fa, f3 = fa;
                    for (int hh = 0; hh < H; ++hh) {
                        FlashArgs& t = ((safe >> hh) & 1u) ? f3 : f8;
                        t.hmap |= (unsigned long long)hh << (4 * t.nh);
                        ++t.nh;
                    }
                    const int cus = device_num_cus();
                    f8.nsplit = flash_split_pick_splits(inv ? 1 : B, f8.nh, Q, (int)N, cus);
                    f3.nsplit = flash_split_pick_splits(inv ? 1 : B, f3.nh, Q, (int)N, cus);
                    f8.cache_head_bytes = f3.cache_head_bytes = kv_blk_head_bytes((int)N, 3);
                    f8.m_part = f8.o_part + (int64_t)B * f8.nh * f8.nsplit * dh * lp;
                    f8.l_part = f8.m_part + (int64_t)B * f8.nh * f8.nsplit * lp;
                    f3.o_part = f8.l_part + (int64_t)B * f8.nh * f8.nsplit * lp;
                    f3.m_part = f3.o_part + (int64_t)B * f3.nh * f3.nsplit * dh * lp;
                    f3.l_part = f3.m_part + (int64_t)B * f3.nh * f3.nsplit * lp;
                    f3.peaky = nullptr; f3.peaky_it = nullptr; f3.peaky_min = nullptr;
                    HIPCHK(launch_flash_split8(f8, cache, s));
                    HIPCHK(launch_flash_split(f3, cache, s, 3, kF16));
                    { Prof pm(c, s, PARQ_PROF_MERGE); HIPCHK(launch_flash_merge(f8, s)); HIPCHK(launch_flash_merge(f3, s)); }
                    merged = true;
                }
            }
            else {
                // a mode-4 handle whose heads are all on the fp16 x 3 tier: the per-head row sums are still recorded (a head may return)
                if (c->attn_mode == 4 && !train && !sharded && H <= 16 && dh == 64) fa.head_min = reinterpret_cast<int*>(wsp + ws.flags) + 32;
                HIPCHK(launch_flash_split(fa, cache, s, c->terms(), c->kind()));
            }
        } else {
            const float* kv = wsp + ws.kv + (int64_t)li * B * 2 * N * C;
            fa.k = kv;                       fa.k_batch = 2 * N * C; fa.k_head = N * dh; fa.k_row = dh;
            fa.v = kv + (int64_t)H * N * dh; fa.v_batch = 2 * N * C; fa.v_head = N * dh; fa.v_row = dh;
            HIPCHK(launch_flash(fa, s));
        }
    }
    if (!merged) { Prof p(c, s, PARQ_PROF_MERGE); HIPCHK(launch_flash_merge(fa, s)); }
    }   // phase bit 2
    if (!(sh.mask & 4)) return PARQ_OK;
    if (sharded) {
        Prof p(c, s, PARQ_PROF_MERGE);
        const int64_t rec = (int64_t)M * C + (int64_t)B * H * flash_lq_pad(Q);
        HIPCHK(launch_attn_combine(sh.in, sh.nranks, rec, B, H, Q, flash_lq_pad(Q), dh, wi + ws.attn, s));
    }
    {
        Prof p(c, s, PARQ_PROF_LINEAR);
        // xb = norm1(xa) + cross_attn @ Wo   (residual recomputed from the published statistics)
        LinearArgs a = lin(wi + ws.attn, C, A + L.cross_out_w, C, A + L.cross_out_b, wi + ws.xb, C, M, C, C);
        a.R = wi + ws.xa; a.ldr = C; a.rln_stats = wi + ws.ln1; a.rln_gamma = A + L.n1_w; a.rln_beta = A + L.n1_b; a.Wp = TP ? TP + L.cross_out_w : nullptr; halfw(a, L.cross_out_w);
        a.drop_p = dp; a.drop_seed = c->site_seed(layer_num, 3);
        if (last_of_forward && c->progress_word != nullptr) {
            // the last iteration's cross-attention has been merged: nothing behind this launch raises a flag (range: the K/V projection;
            // hand-off timeouts: the seam launch in front of the cross-attention; too-peaked rows: the merge).  Tell the host now.
            a.pub_flags = reinterpret_cast<const int*>(wsp + ws.flags);
            a.pub_mirror = c->range_mirror; a.pub_word = c->progress_word;
            a.pub_epoch = reinterpret_cast<const int*>(wsp + ws.ind) + 14;        // CallPtrs::p[7], low word
            a.pub_mask = (c->cache_mode() && c->kind() == kF16) ? ~0 : 4;
            a.pub_peaky = c->terms_for(N, false) == 8 ? 1 : 0;
        }
        HIPCHK(launch_linear(a, 1, s));
        // K8: FFN (transformer_parq.py:383-385): relu(norm2(xb) @ W1), publishes norm2's statistics
        a = lin(wi + ws.xb, C, A + L.lin1_w, C, A + L.lin1_b, wi + ws.ffn, F, M, F, C);
        a.ln_gamma = A + L.n2_w; a.ln_beta = A + L.n2_b; a.ln_stats_out = wi + ws.ln2; a.norm_eps = eps;
        a.relu = 1; a.Wp = TP ? TP + L.lin1_w : nullptr; halfw(a, L.lin1_w, 1);
        a.drop_p = dp; a.drop_seed = c->site_seed(layer_num, 4);
        HIPCHK(launch_linear(a, 1, s));
        // xc = norm2(xb) + ffn @ W2
        a = lin(wi + ws.ffn, F, A + L.lin2_w, F, A + L.lin2_b, wi + ws.xc, C, M, C, F);
        a.R = wi + ws.xb; a.ldr = C; a.rln_stats = wi + ws.ln2; a.rln_gamma = A + L.n2_w; a.rln_beta = A + L.n2_b; a.Wp = TP ? TP + L.lin2_w : nullptr; halfw(a, L.lin2_w);
        a.drop_p = dp; a.drop_seed = c->site_seed(layer_num, 5);
        HIPCHK(launch_linear(a, 1, s));
        // K9: heads (transformer_parq.py:234-252; generic_mlp.py:85-110) on norm3(xc); the first layers of the
        // four heads are one GEMM, which also accumulates the GroupNorm moments of the two hidden blocks
        const int NH1 = c->NH1;
        a = lin(wi + ws.xc, C, A + ar.heads1_w, C, A + ar.heads1_b, wi + ws.h1, NH1, M, NH1, C);
        a.ln_gamma = A + L.n3_w; a.ln_beta = A + L.n3_b; a.norm_eps = eps;
        if (train) a.ln_stats_out = wi + ws.ln3;
        if (NH1 % 16 == 0) { a.Wp = TP ? TP + ar.heads1_w : nullptr; halfw(a, ar.heads1_w, c->nl == 1 ? 1 : 0); }
        a.gn_out_sums = gn1; a.gn_out_ncols = 2 * C; a.gn_out_group_cols = C; a.gn_out_rows_per_scene = Q; a.gn_out_ngroups = 2;
        HIPCHK(launch_linear(a, 1, s));
        // deterministic training: the moments the GEMM added with float64 atomics, recomputed in a fixed order (parq_set_deterministic)
        if ((train && c->deterministic) || (inv && !gn_own)) HIPCHK(launch_gn_moments_det(wi + ws.h1, NH1, C, 2, Q, B, gn1, s));
        a = lin(wi + ws.h1, NH1, A + ar.heads2_w, C, nullptr, wi + ws.h2, 2 * C, M, C, C);
        a.gn_sums = gn1; a.gn_gamma = A + ar.gn1_g; a.gn_beta = A + ar.gn1_b; a.norm_eps = eps;
        a.gn_rows_per_scene = Q; a.gn_ngroups = 2;
        a.gX = C; a.gW = (int64_t)C * C; a.gY = C; a.gGamma = C; a.Wp = TP ? TP + ar.heads2_w : nullptr; halfw(a, ar.heads2_w);
        a.gn_out_sums = gn2; a.gn_out_ncols = C; a.gn_out_group_cols = C; a.gn_out_rows_per_scene = Q; a.gn_out_ngroups = 2;
        HIPCHK(launch_linear(a, 2, s));
        if ((train && c->deterministic) || (inv && !gn_own)) HIPCHK(launch_gn_moments_det(wi + ws.h2, 2 * C, C, 2, Q, B, gn2, s));
    }
    // K10: last head layers + box decode + reference point update + next sine embedding
    // (transformer_parq.py:242-279, 331-332)
    {
        Prof p(c, s, PARQ_PROF_OTHER);
        BoxDecodeArgs d;
        memset(&d, 0, sizeof(d));
        d.h1 = wi + ws.h1 + 2 * C; d.ld1 = c->NH1;
        d.h2 = wi + ws.h2; d.ld2 = 2 * C;
        d.gn_sums = gn2; d.gn_gamma = A + ar.gn2_g; d.gn_beta = A + ar.gn2_b;
        d.w3 = A + ar.heads3_w; d.b3 = A + ar.heads3_b; d.C = C; d.rows_per_scene = Q; d.eps = eps;
        d.ref = ref; d.mean_sizes = A + ar.mean_sizes; d.n_mean = c->cfg.num_mean_sizes; d.dim_t = A + ar.dim_t;
        // fp16-operand modes: a range violation seen while the cache was built must not produce plausible wrong numbers
        d.poison = reinterpret_cast<const int*>(wsp + ws.flags);
        d.poison_mask = (c->cache_mode() && c->kind() == kF16) ? ~0 : 4;     // (a hand-off timeout reaches the mirror in every attention mode)
        // (the last iteration of a forward with an early completion signal has published its bits already — LinearArgs::pub_mirror — and
        // the host may have taken them by now: a second copy from here would be charged to the NEXT forward of the workspace)
        d.poison_mirror = (last_of_forward && c->progress_word != nullptr) ? nullptr : c->range_mirror;
        d.peaky = (!sharded && c->terms_for(N, train, train && bwd_reads_cache(c, ws)) == 8) ? reinterpret_cast<const int*>(wsp + ws.flags) + 1 : nullptr;
        d.peaky_poison = c->peaky_poison;
        d.sb = c->sb; d.M = M; d.ncls = c->ncls;
        d.logits = o->pred_logits; d.center = o->center_unnormalized; d.size = o->size_unnormalized;
        d.rot = o->ortho6d; d.prob = o->sem_cls_prob; d.ref_next = ref_out; d.emb_next = emb_next;
        d.ind = ind; d.out_row0 = row0;
        d.gn_slots = nsl; d.geom_M = geomM;
        HIPCHK(launch_box_decode(d, s));
    }
    return PARQ_OK;
}


// =============================================================================== training: backward chain
// One iteration of the decoder, reversed.  Activations come from the training forward's stash
// (Workspace::shift(k)); gradients of the packed weights accumulate into `G`, an arena with the layout of the weight
// arena; dK/dV of the hoisted K/V projection accumulate in ws.g_kv over the iterations and are pushed through the
// projection once at the end.  Reference points are detached between iterations (transformer_parq.py:331-332): only
// iteration 0 sends gradient to refpoint.weight, through the sine embedding, the projection and the centre update.
struct BwdIO {
    const float* g_logits; const float* g_center; const float* g_size; const float* g_rot;     // this iteration, may be null
    const float* center; const float* size;                                                    // forward outputs
};

// transposed copies of layer li's weights for the dX GEMMs (layout: see do_backward_iter)
int do_backward_transposes(parq_ctx* c, float* wsp, const Workspace& ws, int li, hipStream_t s) {
    const float* A = c->arena;
    const Arena& ar = c->ar;
    const LayerW& L = ar.layers[li];
    const int C = c->C, F = c->F, NH1 = c->NH1;
    float* wT = wsp + ws.wT;
    float* h1T = wT;
    float* h2T = h1T + (int64_t)C * NH1;
    float* l1T = h2T + 2 * (int64_t)C * C;
    float* l2T = l1T + (int64_t)C * F;
    float* coT = l2T + (int64_t)C * F;
    float* cqT = coT + (int64_t)C * C;
    float* soT = cqT + (int64_t)C * C;
    float* siT = soT + (int64_t)C * C;
    float* p2T = siT + 3 * (int64_t)C * C;
    float* p0T = p2T + (int64_t)C * C;
    HIPCHK(launch_transpose(A + ar.heads1_w, C, h1T, NH1, NH1, C, s));
    HIPCHK(launch_transpose(A + ar.heads2_w, C, h2T, C, C, C, s));
    HIPCHK(launch_transpose(A + ar.heads2_w + (int64_t)C * C, C, h2T + (int64_t)C * C, C, C, C, s));
    HIPCHK(launch_transpose(A + L.lin1_w, C, l1T, F, F, C, s));
    HIPCHK(launch_transpose(A + L.lin2_w, F, l2T, C, C, F, s));
    HIPCHK(launch_transpose(A + L.cross_out_w, C, coT, C, C, C, s));
    HIPCHK(launch_transpose(A + L.cross_in_w, C, cqT, C, C, C, s));
    HIPCHK(launch_transpose(A + L.self_out_w, C, soT, C, C, C, s));
    HIPCHK(launch_transpose(A + L.self_in_w, C, siT, 3 * C, 3 * C, C, s));
    HIPCHK(launch_transpose(A + ar.pe2_w, C, p2T, C, C, C, s));
    HIPCHK(launch_transpose(A + ar.pe0_w, 384, p0T, C, C, 384, s));
    return PARQ_OK;
}

// phase 0: the whole iteration.  Batched mode (Workspace::bwd_batched) cuts the chain at the cross-attention: phase 1 runs from the
// outputs down to dO (kept per iteration in ws.g_do, with the residual gradient in ws.g_res and the D rows in ws.g_Dall), the
// attention backward of all iterations is one launch in parq_backward, and phase 2 continues from that iteration's dQ (ws.g_dq).
int do_backward_iter(parq_ctx* c, const parq_scene* sc, float* wsp, const Workspace& ws, int k, const BwdIO& io, float* G,
                     float* g_tokens, hipStream_t s, int phase = 0, int set = 0) {
    const float* A = c->arena;
    const Arena& ar = c->ar;
    const int li = c->cfg.share_weights ? 0 : k;
    const LayerW& L = ar.layers[li];
    const int B = sc->B, C = c->C, Q = c->Q, H = c->H, dh = c->dh, F = c->F, NH1 = c->NH1;
    const int M = B * Q;
    const int64_t N = (int64_t)sc->V * sc->h * sc->w;
    const float eps = 1e-5f;
    float* wi = wsp + ws.shift(k);
    const double* gn1 = reinterpret_cast<const double*>(wi + ws.gn_sums);
    const double* gn2 = gn1 + (int64_t)B * 4 * kGnSlots;
    const float* ref = wi + ws.refk;
    float* gsp = wsp + (int64_t)set * ws.g_set_stride;      // this stream's copy of the scratch (set 0 when the iterations run in turn)
    const int acc = ws.g_sets > 1 ? 2 : 1;                   // dW accumulation: 2 = always by atomics (other iterations add concurrently)
    float *gA = gsp + ws.g_a, *gB = gsp + ws.g_b, *gC = gsp + ws.g_c, *gPos = gsp + ws.g_pos, *tmp = gsp + ws.g_tmp;
    float *gFfh = gsp + ws.g_ffh, *gH1 = gsp + ws.g_h1, *gH2 = gsp + ws.g_h2, *gZ = gsp + ws.g_z, *act = gsp + ws.g_act;
    float *gH3 = gsp + ws.g_h3, *gQkv = gsp + ws.g_qkv, *gEmb = gsp + ws.g_emb, *gRef = gsp + ws.g_ref, *Dd = gsp + ws.g_D;
    double* bs = reinterpret_cast<double*>(gsp + ws.g_bs);
    float* gD = gsp + ws.g_drop;                       // gradient entering a dropout site's branch
    const float dp = c->drop_p;
    const float inv_keep = dp > 0.f ? 1.f / (1.f - dp) : 1.f;
    // the gradient that flows into a dropped branch: g * keep / (1 - p); the residual path keeps the plain g
    auto through_dropout = [&](const float* g, int site) -> const float* {
        if (!(dp > 0.f)) return g;
        if (launch_dropout_apply(g, gD, M, C, dp, c->site_seed(k, site), s) != hipSuccess) return nullptr;
        return gD;
    };
    // transposed weight copies of this layer
    float* wT = wsp + ws.wT;
    float* h1T = wT;                      // [C][NH1]
    float* h2T = h1T + (int64_t)C * NH1;  // 2 x [C][C]
    float* l1T = h2T + 2 * (int64_t)C * C;   // lin1^T [C][F]
    float* l2T = l1T + (int64_t)C * F;       // lin2^T [F][C]
    float* coT = l2T + (int64_t)C * F;       // cross out^T
    float* cqT = coT + (int64_t)C * C;       // cross q^T
    float* soT = cqT + (int64_t)C * C;       // self out^T
    float* siT = soT + (int64_t)C * C;       // self in^T [C][3C]
    float* p2T = siT + 3 * (int64_t)C * C;   // pe2^T
    float* p0T = p2T + (int64_t)C * C;       // pe0^T [384][C]
    if (phase == 0) {
        int rc = do_backward_transposes(c, wsp, ws, li, s);
        if (rc) return rc;
    }

    auto mm = [&](const float* X, int64_t ldx, const float* WT, int K, int Nn, float* Y, int64_t ldy) {   // Y = X W  (W^T given [Nn][K])
        return lin(X, ldx, WT, K, nullptr, Y, ldy, M, Nn, K);
    };
    const int64_t MC = (int64_t)M * C;
    if (phase == 2) {                                  // resume below the cross-attention with this iteration's dQ and residual gradient
        gC = wsp + ws.g_dq + k * MC;
        gB = wsp + ws.g_res + k * MC;
    }
    if (phase != 2) {
    HIPCHK(hipMemsetAsync(gRef, 0, (size_t)M * 3 * sizeof(float), s));

    // ---- heads (transformer_parq.py:234-279)
    HIPCHK(launch_decode_bwd(io.g_logits, io.g_center, io.g_size, io.g_rot, io.center, io.size, ref, c->sb, M, c->ncls, NH1, C, gH3, gH1,
                             k == 0 ? gRef : nullptr, s));
    // last layers: w3 rows 0..2 centre (input h2act[:, :C]), rows 6..11 rotation (input h2act[:, C:])
    HIPCHK(launch_gn_apply(wi + ws.h2, 2 * C, gn2, A + ar.gn2_g, A + ar.gn2_b, M, C, 2, Q, eps, act, 2 * C, s));
    // (every dW product below also leaves the bias gradient = column sums of its dY operand: launch_gemm_tn's last arguments)
    HIPCHK(launch_gemm_tn(gH3, 16, act, 2 * C, G + ar.heads3_w, C, M, 3, C, acc, s, G + ar.heads3_b));
    HIPCHK(launch_gemm_tn(gH3 + 3, 16, act + C, 2 * C, G + ar.heads3_w + 6 * (int64_t)C, C, M, 6, C, acc, s, G + ar.heads3_b + 6));
    HIPCHK(launch_head3_bwd(gH3, A + ar.heads3_w, gZ, M, C, s));                       // gZ = d loss / d h2act
    HIPCHK(launch_gn_bwd(wi + ws.h2, 2 * C, gn2, A + ar.gn2_g, A + ar.gn2_b, M, C, 2, Q, eps, gZ, 2 * C, act, bs, gH2, 2 * C,
                         G + ar.gn2_g, G + ar.gn2_b, s));
    // second layers (grouped): h2[:, g] = h1act[:, g] W2g^T
    HIPCHK(launch_gn_apply(wi + ws.h1, NH1, gn1, A + ar.gn1_g, A + ar.gn1_b, M, C, 2, Q, eps, act, 2 * C, s));   // act = h1act
    for (int g = 0; g < 2; ++g) {
        HIPCHK(launch_gemm_tn(gH2 + g * C, 2 * C, act + g * C, 2 * C, G + ar.heads2_w + (int64_t)g * C * C, C, M, C, C, acc, s));
        LinearArgs a = mm(gH2 + g * C, 2 * C, h2T + (int64_t)g * C * C, C, C, gZ + g * C, 2 * C);       // gZ = d / d h1act
        HIPCHK(launch_linear(a, 1, s));
    }
    HIPCHK(launch_gn_bwd(wi + ws.h1, NH1, gn1, A + ar.gn1_g, A + ar.gn1_b, M, C, 2, Q, eps, gZ, 2 * C, act, bs, gH1, NH1,
                         G + ar.gn1_g, G + ar.gn1_b, s));
    // fused first layers on x3 = norm3(xc)
    HIPCHK(launch_layernorm(wi + ws.xc, A + L.n3_w, A + L.n3_b, tmp, M, C, eps, s));           // tmp = x3
    HIPCHK(launch_gemm_tn(gH1, NH1, tmp, C, G + ar.heads1_w, C, M, NH1, C, acc, s, G + ar.heads1_b, 2 * C));   // columns < 2C: GroupNorm follows, no bias
    {
        LinearArgs a = mm(gH1, NH1, h1T, NH1, C, gA, C);                                       // gA = d / d x3
        HIPCHK(launch_linear(a, 1, s));
    }
    // ---- norm3 / FFN (transformer_parq.py:383-385)
    HIPCHK(launch_ln_bwd(gA, wi + ws.xc, wi + ws.ln3, A + L.n3_w, gB, M, C, 0, G + L.n3_w, G + L.n3_b, s));   // gB = d / d xc
    {
        const float* gd = through_dropout(gB, 5);
        if (!gd) return fail(PARQ_ERR_HIP, "dropout_apply failed");
        HIPCHK(launch_gemm_tn(gd, C, wi + ws.ffn, F, G + L.lin2_w, F, M, C, F, acc, s, G + L.lin2_b));
        LinearArgs a = mm(gd, C, l2T, C, F, gFfh, F);                // d / d ffn hidden, through dropout (the stash holds the dropped,
        a.relu_mask = wi + ws.ffn; a.ldmask = F; a.mask_scale = inv_keep;   // rescaled hidden: zero = dropped or ReLU-inactive) and the ReLU
        HIPCHK(launch_linear(a, 1, s));
    }
    HIPCHK(launch_layernorm(wi + ws.xb, A + L.n2_w, A + L.n2_b, tmp, M, C, eps, s));           // tmp = x2
    HIPCHK(launch_gemm_tn(gFfh, F, tmp, C, G + L.lin1_w, C, M, F, C, acc, s, G + L.lin1_b));
    {
        LinearArgs a = mm(gFfh, F, l1T, F, C, gA, C);                                          // gA = d / d x2 = gB + gFfh W1
        a.R = gB; a.ldr = C;
        HIPCHK(launch_linear(a, 1, s));
    }
    // ---- norm2 / cross-attention (transformer_parq.py:377-382)
    if (phase == 1) gB = wsp + ws.g_res + k * MC;                                              // the residual gradient outlives this call
    float* gDo = phase == 1 ? wsp + ws.g_do + k * MC : gA;
    float* Dc = phase == 1 ? wsp + ws.g_Dall + (int64_t)k * B * H * flash_lq_pad(Q) : Dd;
    HIPCHK(launch_ln_bwd(gA, wi + ws.xb, wi + ws.ln2, A + L.n2_w, gB, M, C, 0, G + L.n2_w, G + L.n2_b, s));   // gB = d / d xb
    {
        const float* gd = through_dropout(gB, 3);
        if (!gd) return fail(PARQ_ERR_HIP, "dropout_apply failed");
        HIPCHK(launch_gemm_tn(gd, C, wi + ws.attn, C, G + L.cross_out_w, C, M, C, C, acc, s, G + L.cross_out_b));
        LinearArgs a = mm(gd, C, coT, C, C, gDo, C);                                           // d / d attention output
        HIPCHK(launch_linear(a, 1, s));
    }
    HIPCHK(launch_attn_bwd_rowdot(gDo, wi + ws.attn, (int64_t)Q * C, C, B, H, Q, dh, Dc, s));
    if (phase == 1) return PARQ_OK;
    HIPCHK(hipMemsetAsync(gC, 0, (size_t)M * C * sizeof(float), s));                           // gC = d / d q (atomics)
    {
        const float* kv = wsp + (c->cache_mode() ? ws.kv_train : ws.kv) + (int64_t)li * B * 2 * N * C;
        // dK | dV accumulate token-major: g_kv[layer][b][n][2C], K heads at columns h*dh, V heads at C + h*dh
        float* gkv = wsp + ws.g_kv + (int64_t)li * B * 2 * N * C;
        HIPCHK(launch_attn_bwd(wi + ws.qc, (int64_t)Q * C, dh, C, kv, 2 * N * C, N * dh, dh, kv + (int64_t)H * N * dh, 2 * N * C, N * dh, dh,
                               gA, (int64_t)Q * C, dh, C, wi + ws.lse_c, Dd, gC, (int64_t)Q * C, dh, C, gkv, 2 * N * C, dh, 2 * C,
                               gkv + C, 2 * N * C, dh, 2 * C, B, H, Q, (int)N, dh, 1, s,
                               attn_bwd_dq_partial_floats(B, H, Q, (int)N, dh) ? wsp + ws.g_dqp : nullptr, dp, c->site_seed(k, 2),
                               reinterpret_cast<unsigned int*>(wsp + ws.g_bs),        // g_bs: free between the GroupNorm passes
                               (dh == 64 || dh == 32) ? nullptr : wsp + ws.g_mat));
    }
    }   // phase != 2
    // q = (x1 + pos) Wq^T + bq,  x1 = norm1(xa)
    HIPCHK(launch_layernorm(wi + ws.xa, A + L.n1_w, A + L.n1_b, tmp, M, C, eps, s));
    HIPCHK(launch_add(tmp, wi + ws.pos, tmp, (int64_t)M * C, s));                              // tmp = x1 + pos
    HIPCHK(launch_gemm_tn(gC, C, tmp, C, G + L.cross_in_w, C, M, C, C, acc, s, G + L.cross_in_b));
    {
        LinearArgs a = mm(gC, C, cqT, C, C, gPos, C);                                          // gPos = d / d (x1 + pos) [cross]
        HIPCHK(launch_linear(a, 1, s));
    }
    HIPCHK(launch_add(gB, gPos, gA, (int64_t)M * C, s));                                       // gA = d / d x1 (residual + query path)
    // ---- norm1 / self-attention (transformer_parq.py:372-376)
    HIPCHK(launch_ln_bwd(gA, wi + ws.xa, wi + ws.ln1, A + L.n1_w, gB, M, C, 0, G + L.n1_w, G + L.n1_b, s));   // gB = d / d xa
    {
        const float* gd = through_dropout(gB, 1);
        if (!gd) return fail(PARQ_ERR_HIP, "dropout_apply failed");
        HIPCHK(launch_gemm_tn(gd, C, wi + ws.sa, C, G + L.self_out_w, C, M, C, C, acc, s, G + L.self_out_b));
        LinearArgs a = mm(gd, C, soT, C, C, gA, C);                                            // gA = d / d self-attention output
        HIPCHK(launch_linear(a, 1, s));
    }
    HIPCHK(launch_attn_bwd_rowdot(gA, wi + ws.sa, (int64_t)Q * C, C, B, H, Q, dh, Dd, s));
    HIPCHK(hipMemsetAsync(gQkv, 0, (size_t)M * 3 * C * sizeof(float), s));
    HIPCHK(launch_attn_bwd(wi + ws.qkv, (int64_t)Q * 3 * C, dh, 3 * C, wi + ws.qkv + C, (int64_t)Q * 3 * C, dh, 3 * C,
                           wi + ws.qkv + 2 * C, (int64_t)Q * 3 * C, dh, 3 * C, gA, (int64_t)Q * C, dh, C, wi + ws.lse_s, Dd,
                           gQkv, (int64_t)Q * 3 * C, dh, 3 * C, gQkv + C, (int64_t)Q * 3 * C, dh, 3 * C, gQkv + 2 * C,
                           (int64_t)Q * 3 * C, dh, 3 * C, B, H, Q, Q, dh, 0, s, nullptr, dp, c->site_seed(k, 0), nullptr,
                           (dh == 64 || dh == 32) ? nullptr : wsp + ws.g_mat));
    // in-projection: [q | k] = (tgt + pos) Wqk^T, v = tgt Wv^T
    HIPCHK(launch_add(wi + ws.tgt, wi + ws.pos, tmp, (int64_t)M * C, s));                      // tmp = tgt + pos
    HIPCHK(launch_gemm_tn(gQkv, 3 * C, tmp, C, G + L.self_in_w, C, M, 2 * C, C, acc, s, G + L.self_in_b));
    HIPCHK(launch_gemm_tn(gQkv + 2 * C, 3 * C, wi + ws.tgt, C, G + L.self_in_w + 2 * (int64_t)C * C, C, M, C, C, acc, s, G + L.self_in_b + 2 * C));
    {
        // d / d (tgt + pos) through q and k: rows 0 .. 2C-1 of W_in, i.e. columns 0 .. 2C-1 of W_in^T ([C][3C])
        LinearArgs a = lin(gQkv, 3 * C, siT, 3 * C, nullptr, gA, C, M, C, 2 * C);
        HIPCHK(launch_linear(a, 1, s));
        HIPCHK(launch_add(gPos, gA, gPos, (int64_t)M * C, s));                                  // gPos = total d / d pos
        // d / d tgt = gB (residual) + gA (q, k path) + gQkv_v Wv
        a = lin(gQkv + 2 * C, 3 * C, siT + 2 * C, 3 * C, nullptr, gC, C, M, C, C);
        a.R = gA; a.ldr = C;
        HIPCHK(launch_linear(a, 1, s));
        HIPCHK(launch_add(gC, gB, gC, (int64_t)M * C, s));                                      // gC = d / d tgt
    }
    // ---- project + sample (transformer_parq.py:321)
    {
        int tt;
        const void* tok = bwd_tokens(c, sc, wsp, ws, &tt);
        HIPCHK(launch_sample_bwd(tok, reinterpret_cast<const double*>(wsp + ws.T_cl), sc->camera, ref, c->sb, B, sc->V, sc->h, sc->w,
                                 C, Q, gC, g_tokens, k == 0 ? gRef : nullptr, s, tt));
    }
    // ---- position MLP (transformer_parq.py:176-180,317): pos = relu(emb W0^T + b0) W2^T + b2
    HIPCHK(launch_gemm_tn(gPos, C, wi + ws.pe_h, C, G + ar.pe2_w, C, M, C, C, acc, s, G + ar.pe2_b));
    {
        LinearArgs a = mm(gPos, C, p2T, C, C, gA, C);                                          // gA = d / d pe hidden
        a.relu_mask = wi + ws.pe_h; a.ldmask = C;
        HIPCHK(launch_linear(a, 1, s));
    }
    HIPCHK(launch_gemm_tn(gA, C, wi + ws.emb, 384, G + ar.pe0_w, 384, M, C, 384, acc, s, G + ar.pe0_b));
    if (k == 0) {
        LinearArgs a = lin(gA, C, p0T, C, nullptr, gEmb, 384, M, 384, C);
        HIPCHK(launch_linear(a, 1, s));
        HIPCHK(launch_posemb_bwd(gEmb, ref, A + ar.dim_t, M, gRef, s));
        HIPCHK(launch_refpoint_bwd(gRef, ref, B, Q, G + ar.refpoint, s));
    }
    return PARQ_OK;
}

// hoisted K/V projection backward: [K | V] = tokens W_kv^T + b_kv per layer; g_kv is token-major [layer][b][n][2C], so the
// whole projection is one TN GEMM (dW_kv = g^T tokens), one column sum (db_kv) and one GEMM (d tokens += g W_kv)
int do_backward_kvproj(parq_ctx* c, const parq_scene* sc, float* wsp, const Workspace& ws, float* G, float* g_tokens, hipStream_t s) {
    const float* A = c->arena;
    const int B = sc->B, C = c->C;
    const int64_t N = (int64_t)sc->V * sc->h * sc->w;
    if ((int64_t)B * N > (int64_t)INT32_MAX) return fail(PARQ_ERR_ARG, "B*N too large");
    float* wT = wsp + ws.wT;            // W_kv^T [C][2C]
    int tt;
    const void* tok = bwd_tokens(c, sc, wsp, ws, &tt);
    const size_t tb = tt == kTokF32 ? 4 : 2;
    for (int li = 0; li < c->nl; ++li) {
        const LayerW& L = c->ar.layers[li];
        const float* g = wsp + ws.g_kv + (int64_t)li * B * 2 * N * C;          // [B*N][2C]
        const int Mr = (int)(B * N);
        const bool split_ok = ws.bwd_batched;                                    // the batched backward leaves max |g| in g_kvmax
        if (split_ok && kvproj_bwd_split_supported(C)) {
            // dW, db on the fp16 matrix pipe (hi/lo split); g is scaled by the power of two derived from max |g| (attention epilogue)
            HIPCHK(launch_kvproj_bwd_split(g, tok, Mr, C, G + L.cross_in_w + (int64_t)C * C, G + L.cross_in_b + C,
                                           reinterpret_cast<const unsigned int*>(wsp + ws.g_kvmax), wsp + ws.g_kvmax + 1, s, tt));
        } else if (split_ok && C % 256 == 0) {
            // wider models (C = 1024: 805 GFLOP): the same kernel per 512 x 256 block of dW_kv; the bias gradient falls out of the
            // blocks of the first column slice
            float* dW = G + L.cross_in_w + (int64_t)C * C;
            float* db = G + L.cross_in_b + C;
            for (int n0 = 0; n0 < 2 * C; n0 += 512)
                for (int k0 = 0; k0 < C; k0 += 256)
                    HIPCHK(launch_tn_split_512x256(g + n0, 2 * C, reinterpret_cast<const char*>(tok) + k0 * tb, C, Mr, dW + (int64_t)n0 * C + k0, C,
                                                   k0 == 0 ? db + n0 : nullptr, reinterpret_cast<const unsigned int*>(wsp + ws.g_kvmax),
                                                   wsp + ws.g_kvmax + 1, s, tt));
        } else {
            HIPCHK(launch_gemm_tn(g, 2 * C, tok, C, G + L.cross_in_w + (int64_t)C * C, C, Mr, 2 * C, C, 1, s, nullptr, 0, tt));
            HIPCHK(launch_colsum(g, 2 * C, Mr, 2 * C, G + L.cross_in_b + C, 1, s));
        }
        if (g_tokens) {
            HIPCHK(launch_transpose(A + L.cross_in_w + (int64_t)C * C, C, wT, 2 * C, 2 * C, C, s));
            if (split_ok && (kvproj_bwd_split_supported(C) || C % 256 == 0)) {        // (the dW launch above left the scale in g_kvmax[1])
                // d tokens += g W_kv on the fp16 matrix pipe (201 GFLOP per scene at C = 256, 805 at C = 1024): W_kv^T split hi/lo
                // once, g scaled by the power of two of the dW kernel (g_kvmax[1], written by the launch above) while it is split
                _Float16* whi = reinterpret_cast<_Float16*>(wT + (int64_t)C * 2 * C);
                _Float16* wlo = whi + (int64_t)C * 2 * C;
                HIPCHK(launch_split_f32(wT, whi, wlo, (int64_t)C * 2 * C, s));
                HIPCHK(launch_gemm_split(g, 2 * C, whi, wlo, nullptr, g_tokens, C, Mr, C, 2 * C, 0, nullptr, 1, s, wsp + ws.g_kvmax + 1, 1.f,
                                         wsp + ws.g_kvmax + 1, 1));
            } else {
                LinearArgs a = lin(g, 2 * C, wT, 2 * C, nullptr, g_tokens, C, Mr, C, 2 * C);
                a.R = g_tokens; a.ldr = C;
                HIPCHK(launch_linear(a, 1, s));
            }
        }
    }
    return PARQ_OK;
}

int check_outs(const parq_outputs* o) {
    if (!o || !o->pred_logits || !o->center_unnormalized || !o->size_unnormalized || !o->ortho6d || !o->sem_cls_prob ||
        !o->coord_pos)
        return fail(PARQ_ERR_ARG, "outputs has a NULL tensor");
    return PARQ_OK;
}

}  // namespace

// =============================================================================== C ABI

extern "C" {

const char* parq_last_error(void) { return g_err; }
const char* parq_version(void) {
#ifdef PARQ_DEV_PROBES
    return "parq_hip 0.3-dev (gfx950; DEVELOPMENT build: environment A/B switches, probe kernels and time stamps compiled in)";
#else
    return "parq_hip 0.4 (gfx950; cross-attention: fp16 hi/lo split MFMA products, cross terms as MX-fp8 products in mode 4, exact fp32 MFMA on request)";
#endif
}

int parq_create(const parq_config* cfg, parq_handle* out) {
    if (!cfg || !out) return fail(PARQ_ERR_ARG, "NULL argument");
    if (cfg->dim < 32 || cfg->dim % 32 != 0 || cfg->dim > 1024) return fail(PARQ_ERR_ARG, "dim=%d must be a multiple of 32 in [32,1024]", cfg->dim);
    if (cfg->num_heads < 1 || cfg->dim % cfg->num_heads != 0) return fail(PARQ_ERR_ARG, "dim %% num_heads != 0");
    const int dh = cfg->dim / cfg->num_heads;
    if (!(dh == 32 || dh == 64 || dh == 128 || dh == 256)) return fail(PARQ_ERR_ARG, "head dim %d unsupported (32/64/128/256)", dh);
    if (cfg->ffn_dim < 32 || cfg->ffn_dim % 32 != 0) return fail(PARQ_ERR_ARG, "ffn_dim must be a multiple of 32");
    if (cfg->num_queries < 1 || cfg->num_layers < 1) return fail(PARQ_ERR_ARG, "num_queries/num_layers must be >= 1");
    if (cfg->num_classes < 2 || cfg->num_classes > 32) return fail(PARQ_ERR_ARG, "num_classes must be in [2,32]");
    if (cfg->num_mean_sizes < 1) return fail(PARQ_ERR_ARG, "num_mean_sizes must be >= 1");
    for (int i = 0; i < 3; ++i)
        if (!(cfg->scale[2 * i + 1] > cfg->scale[2 * i])) return fail(PARQ_ERR_ARG, "scale must be increasing per axis");
    parq_ctx* c = new parq_ctx();
    c->cfg = *cfg;
    c->C = cfg->dim; c->Q = cfg->num_queries; c->H = cfg->num_heads; c->dh = dh; c->F = cfg->ffn_dim;
    c->I = cfg->num_layers; c->ncls = cfg->num_classes;
    c->nl = cfg->share_weights ? 1 : cfg->num_layers;
    c->NH1 = 2 * c->C + ((c->ncls + 3 + 3) / 4) * 4;
    for (int i = 0; i < 3; ++i) { c->sb.lo[i] = cfg->scale[2 * i]; c->sb.hi[i] = cfg->scale[2 * i + 1]; }
    // dim_t[i] = 10000^(2*(i//2)/128) in float32 (transformer_parq.py:49-50)
    for (int i = 0; i < 128; ++i) c->dim_t_host[i] = powf(10000.0f, 2.0f * (float)(i / 2) / 128.0f);
    build_arena(c);
    *out = c;
    return PARQ_OK;
}

#ifdef PARQ_DEV_PROBES
// development build only (not declared in include/parq_hip.h): device buffer of in-kernel time stamps, see common.hpp.
// buf = [cursor, 3 unused, records of 4 x u64 ...] with room for `cap` records; NULL switches the stamps off.  Synchronises.
extern "C" int parq_dev_timeline(unsigned long long* buf, unsigned int cap) {
    if (buf) HIPCHK(hipMemset(buf, 0, 32));
    HIPCHK(tl_set_linear(buf, cap)); HIPCHK(tl_set_elementwise(buf, cap)); HIPCHK(tl_set_flash(buf, cap));
    HIPCHK(tl_set_flash_split(buf, cap)); HIPCHK(tl_set_flash_split8(buf, cap)); HIPCHK(tl_set_kvproj_split(buf, cap)); HIPCHK(tl_set_chain(buf, cap));
    return PARQ_OK;
}
#endif

int parq_set_backward_batched(parq_handle h, int32_t on) {
    if (!h) return fail(PARQ_ERR_ARG, "NULL handle");
    h->bwd_batched_env = on != 0;
    return PARQ_OK;
}

/* Iterations of the chain backward in flight at once (default 8 = up to eight streams; their weight gradients meet in the arena
 * through float atomics, so the summation order — and the last bits of the gradients — vary from run to run).  1 runs the
 * iterations in turn on the caller's stream with plain accumulation: reproducible gradients for the chain (the hoisted K/V
 * projection's row-split and the set loss still reduce with atomics).  Changes the training workspace size: call before
 * parq_train_workspace_bytes. */
int parq_set_backward_streams(parq_handle h, int32_t n) {
    if (!h || n < 1 || n > 8) return fail(PARQ_ERR_ARG, "parq_set_backward_streams: 1 <= n <= 8");
    h->bwd_streams = n;
    return PARQ_OK;
}

/* Fixed-order reductions in parq_forward_train / parq_backward (include/parq_hip.h).  Changes the training workspace size and runs
 * the backward on the caller's stream only (carve_workspace): call before parq_train_workspace_bytes. */
int parq_set_deterministic(parq_handle h, int32_t on) {
    if (!h) return fail(PARQ_ERR_ARG, "NULL handle");
    if (on != 0 && on != 1) return fail(PARQ_ERR_ARG, "parq_set_deterministic: on must be 0 or 1");
    h->deterministic = on != 0;
    return PARQ_OK;
}

int parq_destroy(parq_handle h) {
    if (!h) return PARQ_OK;
    for (hipEvent_t e : h->bucket_done) if (e) (void)hipEventDestroy(e);
    for (auto& e : h->events) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    for (hipEvent_t e : h->iter_done) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->join_ev) if (e) (void)hipEventDestroy(e);
    if (h->fork_ev) (void)hipEventDestroy(h->fork_ev);
    for (hipStream_t st : h->aux_stream) if (st) (void)hipStreamDestroy(st);
    if (h->cap_stream) (void)hipStreamDestroy(h->cap_stream);
    delete h;
    return PARQ_OK;
}

int parq_set_weight(parq_handle h, const char* name, const float* dev, int64_t numel) {
    if (!h || !name || !dev || numel <= 0) return fail(PARQ_ERR_ARG, "bad argument to parq_set_weight");
    std::string n(name);
    const std::string dup = "parq_module.decoder.mlp_heads.";      // same storage as mlp_heads.* (parq_decoder.py:66)
    if (n.compare(0, dup.size(), dup) == 0) n = "mlp_heads." + n.substr(dup.size());
    h->named[n] = WeightRef{dev, numel};
    h->packed = false;
    return PARQ_OK;
}

size_t parq_packed_weights_bytes(parq_handle h) { return h ? (size_t)h->ar.total * sizeof(float) : 0; }

int parq_pack_weights(parq_handle h, void* arena_v, size_t arena_bytes, parq_stream stream) {
    if (!h || !arena_v) return fail(PARQ_ERR_ARG, "NULL argument");
    if (arena_bytes < (size_t)h->ar.total * sizeof(float)) return fail(PARQ_ERR_WORKSPACE, "weight arena too small");
    hipStream_t s = (hipStream_t)stream;
    float* A = (float*)arena_v;
    parq_ctx* c = h;
    const int64_t C = c->C, F = c->F, Q = c->Q;
    int rc = PARQ_OK;
    auto get = [&](const std::string& name, int64_t numel) -> const float* {
        auto it = c->named.find(name);
        if (it == c->named.end()) { rc = fail(PARQ_ERR_STATE, "weight '%s' was never set", name.c_str()); return nullptr; }
        if (it->second.n != numel) { rc = fail(PARQ_ERR_ARG, "weight '%s' has %lld elements, expected %lld", name.c_str(), (long long)it->second.n, (long long)numel); return nullptr; }
        return it->second.p;
    };
    GatherArgs gq;
    gq.count = 0;
    auto copy = [&](const std::string& name, int64_t dst, int64_t numel) -> bool {
        const float* p = get(name, numel);
        if (!p) return false;
        // queued: the tensors go in launches of up to kGatherMax copies (a training step re-packs ~50 tensors after every
        // optimizer step; one hipMemcpyAsync each was ~50 dependent 3 us operations)
        if (gq.count == kGatherMax) {
            hipError_t e = launch_gather_copy(gq, s);
            if (e != hipSuccess) { rc = fail(PARQ_ERR_HIP, "gather copy (%s): %s", name.c_str(), hipGetErrorString(e)); return false; }
            gq.count = 0;
        }
        gq.src[gq.count] = p; gq.dst[gq.count] = A + dst; gq.n[gq.count] = numel; ++gq.count;
        return true;
    };
    auto flush = [&]() -> int {
        HIPCHK(launch_gather_copy(gq, s));
        gq.count = 0;
        return PARQ_OK;
    };
    HIPCHK(hipMemsetAsync(A, 0, (size_t)c->ar.total * sizeof(float), s));
    for (int li = 0; li < c->nl; ++li) {
        const LayerW& L = c->ar.layers[li];
        const std::string p = "parq_module.decoder.layers." + std::to_string(li) + ".";
        if (!copy(p + "self_attn.in_proj_weight", L.self_in_w, 3 * C * C) || !copy(p + "self_attn.in_proj_bias", L.self_in_b, 3 * C) ||
            !copy(p + "self_attn.out_proj.weight", L.self_out_w, C * C) || !copy(p + "self_attn.out_proj.bias", L.self_out_b, C) ||
            !copy(p + "multihead_attn.in_proj_weight", L.cross_in_w, 3 * C * C) || !copy(p + "multihead_attn.in_proj_bias", L.cross_in_b, 3 * C) ||
            !copy(p + "multihead_attn.out_proj.weight", L.cross_out_w, C * C) || !copy(p + "multihead_attn.out_proj.bias", L.cross_out_b, C) ||
            !copy(p + "linear1.weight", L.lin1_w, F * C) || !copy(p + "linear1.bias", L.lin1_b, F) ||
            !copy(p + "linear2.weight", L.lin2_w, C * F) || !copy(p + "linear2.bias", L.lin2_b, C) ||
            !copy(p + "norm1.weight", L.n1_w, C) || !copy(p + "norm1.bias", L.n1_b, C) ||
            !copy(p + "norm2.weight", L.n2_w, C) || !copy(p + "norm2.bias", L.n2_b, C) ||
            !copy(p + "norm3.weight", L.n3_w, C) || !copy(p + "norm3.bias", L.n3_b, C))
            return rc;
    }
    c->kv16_state = 1;
    const Arena& ar = c->ar;
    const std::string d = "parq_module.decoder.";
    const std::string hc = "mlp_heads.center_head.layers.", hr = "mlp_heads.rotation_head.layers.";
    const int ncls = c->ncls;
    if (!copy("refpoint.weight", ar.refpoint, Q * 3) ||
        !copy(d + "position_encoder.0.weight", ar.pe0_w, C * 384) || !copy(d + "position_encoder.0.bias", ar.pe0_b, C) ||
        !copy(d + "position_encoder.2.weight", ar.pe2_w, C * C) || !copy(d + "position_encoder.2.bias", ar.pe2_b, C) ||
        // fused first head layer: [centre.0 ; rotation.0 ; sem_cls ; size]
        !copy(hc + "0.weight", ar.heads1_w, C * C) || !copy(hr + "0.weight", ar.heads1_w + C * C, C * C) ||
        !copy("mlp_heads.sem_cls_head.layers.0.weight", ar.heads1_w + 2 * C * C, ncls * C) ||
        !copy("mlp_heads.size_head.layers.0.weight", ar.heads1_w + (2 * C + ncls) * C, 3 * C) ||
        !copy("mlp_heads.sem_cls_head.layers.0.bias", ar.heads1_b + 2 * C, ncls) ||
        !copy("mlp_heads.size_head.layers.0.bias", ar.heads1_b + 2 * C + ncls, 3) ||
        !copy(hc + "1.weight", ar.gn1_g, C) || !copy(hr + "1.weight", ar.gn1_g + C, C) ||
        !copy(hc + "1.bias", ar.gn1_b, C) || !copy(hr + "1.bias", ar.gn1_b + C, C) ||
        !copy(hc + "4.weight", ar.heads2_w, C * C) || !copy(hr + "4.weight", ar.heads2_w + C * C, C * C) ||
        !copy(hc + "5.weight", ar.gn2_g, C) || !copy(hr + "5.weight", ar.gn2_g + C, C) ||
        !copy(hc + "5.bias", ar.gn2_b, C) || !copy(hr + "5.bias", ar.gn2_b + C, C) ||
        !copy(hc + "8.weight", ar.heads3_w, 3 * C) || !copy(hr + "8.weight", ar.heads3_w + 6 * C, 6 * C) ||
        !copy(hc + "8.bias", ar.heads3_b, 3) || !copy(hr + "8.bias", ar.heads3_b + 6, 6) ||
        !copy("mean_sizes", ar.mean_sizes, (int64_t)c->cfg.num_mean_sizes * 3))
        return rc;
    if ((rc = flush()) != PARQ_OK) return rc;
    for (int li = 0; li < c->nl; ++li) {                // hi/lo split of the K/V projection weights, from the packed copy
        const LayerW& L = c->ar.layers[li];
        HIPCHK(launch_split_f32(A + L.cross_in_w + C * C, A + L.kv_whi, A + L.kv_wlo, 2 * C * C, s));
    }
    // small host table kept in the handle, so the copy needs no synchronisation with the stream
    HIPCHK(hipMemcpyAsync(A + ar.dim_t, c->dim_t_host, sizeof(c->dim_t_host), hipMemcpyHostToDevice, s));
    c->derived_valid = false;          // folded position-MLP weights + tile-ordered mirror: built by the first inference iteration
    c->arena = A;
    c->packed = true;
    c->prepared = false;
    ++c->pack_gen;                     // every K/V cache was projected with the weights of an earlier pack
    c->cache_recs.clear();
    return PARQ_OK;
}

size_t parq_workspace_bytes(parq_handle h, int32_t B, int32_t V, int32_t hh, int32_t ww) {
    if (!h || B < 1 || V < 1 || hh < 1 || ww < 1) return 0;
    Workspace ws;
    carve_workspace(h, B, V, hh, ww, &ws, h->batch_invariant);
    return (size_t)ws.total * sizeof(float);
}

int parq_prepare(parq_handle h, const parq_scene* scene, void* workspace, size_t workspace_bytes, parq_stream stream) {
    if (!h || !workspace) return fail(PARQ_ERR_ARG, "NULL argument");
    if (!h->packed) return fail(PARQ_ERR_STATE, "parq_pack_weights must be called first");
    int rc = check_scene(h, scene);
    if (rc) return rc;
    Workspace ws;
    carve_workspace(h, scene->B, scene->V, scene->h, scene->w, &ws, h->batch_invariant);
    if (workspace_bytes < (size_t)ws.total * sizeof(float)) return fail(PARQ_ERR_WORKSPACE, "workspace too small: %zu < %zu", workspace_bytes, (size_t)ws.total * sizeof(float));
    h->map_recs.erase(workspace);         // the K cache is rewritten: "cross_q" of an earlier iteration no longer belongs to it
    h->cache_recs.erase(workspace);       // (a stepping driver owns the workspace from here on)
    return do_prepare(h, scene, (float*)workspace, ws, (hipStream_t)stream);
}

int parq_iterate(parq_handle h, const parq_scene* scene, void* workspace, size_t workspace_bytes, int32_t layer_num,
                 const float* ref_in, const parq_outputs* outs, float* ref_out, parq_stream stream) {
    if (!h || !workspace) return fail(PARQ_ERR_ARG, "NULL argument");
    if (!h->packed || !h->prepared) return fail(PARQ_ERR_STATE, "parq_prepare must be called first");
    int rc = check_scene(h, scene);
    if (rc) return rc;
    rc = check_outs(outs);
    if (rc) return rc;
    if (layer_num < 0 || layer_num >= h->I) return fail(PARQ_ERR_ARG, "layer_num out of range");
    Workspace ws;
    carve_workspace(h, scene->B, scene->V, scene->h, scene->w, &ws, h->batch_invariant);
    if (workspace_bytes < (size_t)ws.total * sizeof(float)) return fail(PARQ_ERR_WORKSPACE, "workspace too small");
    float* wsp = (float*)workspace;
    hipStream_t s = (hipStream_t)stream;
    const float* ref = ref_in ? ref_in : wsp + ws.ref;
    h->map_recs.erase(workspace);         // "cross_q" is rewritten: the note returns once the iteration is enqueued whole
    rc = do_iterate(h, scene, wsp, ws, layer_num, ref, ref_in == nullptr && h->emb_valid, outs, wsp + ws.ref_next, s);
    h->emb_valid = (rc == PARQ_OK);        // the decode kernel left pos2posemb3d(ref_next) in the workspace
    if (rc) return rc;
    const size_t rb = (size_t)scene->B * h->Q * 3 * sizeof(float);
    HIPCHK(hipMemcpyAsync(wsp + ws.ref, wsp + ws.ref_next, rb, hipMemcpyDeviceToDevice, s));
    if (ref_out) HIPCHK(hipMemcpyAsync(ref_out, wsp + ws.ref_next, rb, hipMemcpyDeviceToDevice, s));
    h->note_iteration(workspace, scene, layer_num, 1);
    return PARQ_OK;
}

size_t parq_shard_exchange_floats(parq_handle h, int32_t B, int32_t which) {
    if (!h || B < 1 || which < 0 || which > 1) return 0;
    const int64_t M = (int64_t)B * h->Q;
    // which = 0: [M*C sample sums | M valid-view counts | 1 fp16-range flag] (SUM all-reduce); 1: [M*C outputs | lse rows] (all-gather)
    return (size_t)(which == 0 ? M * h->C + M + 1 : M * h->C + (int64_t)B * h->H * flash_lq_pad(h->Q));
}

int parq_iterate_sharded(parq_handle h, const parq_scene* scene, void* workspace, size_t workspace_bytes, int32_t layer_num,
                         int32_t phase, const float* ref_in, const parq_outputs* outs, float* ref_out, const float* xchg_in,
                         float* xchg_out, int32_t nranks, parq_stream stream) {
    if (!h || !workspace) return fail(PARQ_ERR_ARG, "NULL argument");
    if (h->tok_type != kTokF32) return fail(PARQ_ERR_ARG, "parq_iterate_sharded reads fp32 tokens only: set token type 0");
    if (!h->packed || !h->prepared) return fail(PARQ_ERR_STATE, "parq_prepare must be called first");
    int rc = check_scene(h, scene);
    if (rc) return rc;
    rc = check_outs(outs);
    if (rc) return rc;
    if (layer_num < 0 || layer_num >= h->I) return fail(PARQ_ERR_ARG, "layer_num out of range");
    if (phase < 0 || phase > 2) return fail(PARQ_ERR_ARG, "phase must be 0, 1 or 2");
    if ((phase <= 1 && !xchg_out) || (phase >= 1 && !xchg_in)) return fail(PARQ_ERR_ARG, "exchange buffer is NULL for phase %d", phase);
    if (phase == 2 && nranks < 1) return fail(PARQ_ERR_ARG, "nranks must be >= 1");
    Workspace ws;
    carve_workspace(h, scene->B, scene->V, scene->h, scene->w, &ws, false);
    if (workspace_bytes < (size_t)ws.total * sizeof(float)) return fail(PARQ_ERR_WORKSPACE, "workspace too small");
    float* wsp = (float*)workspace;
    hipStream_t s = (hipStream_t)stream;
    const float* ref = ref_in ? ref_in : wsp + ws.ref;
    ShardIO sh;
    sh.mask = 1 << phase; sh.in = xchg_in; sh.out = xchg_out; sh.nranks = nranks;
    h->map_recs.erase(workspace);
    h->cache_recs.erase(workspace);
    rc = do_iterate(h, scene, wsp, ws, layer_num, ref, ref_in == nullptr && h->emb_valid, outs, wsp + ws.ref_next, s, 0, nullptr, false, sh);
    if (rc) return rc;
    if (phase == 2) {
        h->emb_valid = true;                   // the decode kernel left pos2posemb3d(ref_next) in the workspace
        const size_t rb = (size_t)scene->B * h->Q * 3 * sizeof(float);
        HIPCHK(hipMemcpyAsync(wsp + ws.ref, wsp + ws.ref_next, rb, hipMemcpyDeviceToDevice, s));
        if (ref_out) HIPCHK(hipMemcpyAsync(ref_out, wsp + ws.ref_next, rb, hipMemcpyDeviceToDevice, s));
    }
    h->note_iteration(workspace, scene, layer_num, 3);
    return PARQ_OK;
}

// the I iterations behind the prologue; captured: being recorded by parq_forward_capture (do_iterate)
static int forward_iterations(parq_ctx* h, const parq_scene* scene, float* wsp, const Workspace& ws, const parq_outputs* outs, hipStream_t s,
                              bool captured) {
    const int64_t M = (int64_t)scene->B * h->Q;
    float* ra = wsp + ws.ref;
    float* rb = wsp + ws.ref_next;
    for (int k = 0; k < h->I; ++k) {
        parq_outputs o;
        memset(&o, 0, sizeof(o));
        if (!captured) {
            o.pred_logits = outs->pred_logits + k * M * h->ncls;
            o.center_unnormalized = outs->center_unnormalized + k * M * 3;
            o.size_unnormalized = outs->size_unnormalized + k * M * 3;
            o.ortho6d = outs->ortho6d + k * M * 6;
            o.sem_cls_prob = outs->sem_cls_prob + k * M * h->ncls;
            o.coord_pos = outs->coord_pos + k * M * 3;
        }
        const int rc = do_iterate(h, scene, wsp, ws, k, ra, true, &o, rb, s, 0, nullptr, false, ShardIO(),      // ping-pong the reference points; the sine
                                  captured ? k * M : -1, k + 1 == h->I);                                        // embedding of iteration 0 comes from the
        if (rc) return rc;                                                                                      // prologue, later ones from the previous decode
        float* t = ra; ra = rb; rb = t;
    }
    h->ref_state = 0;       // ws.ref / ws.ref_next roles depend on parity; stepping must re-prepare
    h->prepared = false;
    return PARQ_OK;
}

static int forward_checks(parq_handle h, const parq_scene* scene, void* workspace, size_t workspace_bytes, const parq_outputs* outs, Workspace* ws) {
    if (!h || !workspace) return fail(PARQ_ERR_ARG, "NULL argument");
    if (!h->packed) return fail(PARQ_ERR_STATE, "parq_pack_weights must be called first");
    int rc = check_scene(h, scene);
    if (rc) return rc;
    rc = check_outs(outs);
    if (rc) return rc;
    carve_workspace(h, scene->B, scene->V, scene->h, scene->w, ws, h->batch_invariant);
    if (workspace_bytes < (size_t)ws->total * sizeof(float)) return fail(PARQ_ERR_WORKSPACE, "workspace too small: %zu < %zu", workspace_bytes, (size_t)ws->total * sizeof(float));
    return PARQ_OK;
}

int parq_forward(parq_handle h, const parq_scene* scene, void* workspace, size_t workspace_bytes,
                 const parq_outputs* outs, parq_stream stream) {
    Workspace ws;
    int rc = forward_checks(h, scene, workspace, workspace_bytes, outs, &ws);
    if (rc) return rc;
    h->map_recs.erase(workspace);         // the cache and "cross_q" are rewritten: the notes return once the forward is enqueued whole
    h->cache_recs.erase(workspace);
    rc = do_prepare(h, scene, (float*)workspace, ws, (hipStream_t)stream, false, nullptr, true);
    if (rc) return rc;
    rc = forward_iterations(h, scene, (float*)workspace, ws, outs, (hipStream_t)stream, false);
    if (rc == PARQ_OK) { h->note_iteration(workspace, scene, h->I - 1, 1); h->note_cache(workspace, scene); }
    return rc;
}

/* ---- a captured forward (include/parq_hip.h) ---------------------------------------------------------------------------------- */
// what a graph was recorded with: parq_forward_replay refuses a graph whose recording no longer matches the handle or the call
struct GraphKey {
    int B, V, h, w, mode, seam, poison, tok, inv;
    uint32_t safe;
    const void* ws; const void* arena; const void* mirror; const void* progress;
    bool operator==(const GraphKey& o) const {
        return B == o.B && V == o.V && h == o.h && w == o.w && mode == o.mode && seam == o.seam && poison == o.poison && tok == o.tok && inv == o.inv && safe == o.safe &&
               ws == o.ws && arena == o.arena && mirror == o.mirror && progress == o.progress;
    }
};
static GraphKey graph_key(const parq_ctx* c, int B, int V, int hh, int ww, const void* wsp) {
    return GraphKey{B, V, hh, ww, c->attn_mode, c->seam_fusion ? 1 : 0, c->peaky_poison, c->tok_type, c->batch_invariant ? 1 : 0, c->safe_heads(), wsp, c->arena, c->range_mirror,
                    c->progress_word};
}
struct parq_graph { hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; size_t nodes = 0; GraphKey key; };

int parq_forward_capture(parq_handle h, int32_t B, int32_t V, int32_t hh, int32_t ww, void* workspace, size_t workspace_bytes,
                         parq_stream stream, parq_graph_t* out) {
    if (!h || !workspace || !out) return fail(PARQ_ERR_ARG, "NULL argument");
    *out = nullptr;
    if (!h->packed) return fail(PARQ_ERR_STATE, "parq_pack_weights must be called first");
    if (h->profiling) return fail(PARQ_ERR_STATE, "parq_forward_capture: switch parq_profile_enable off (its events are host-side records)");
    parq_scene scene;
    memset(&scene, 0, sizeof(scene));
    scene.B = B; scene.V = V; scene.h = hh; scene.w = ww;
    // (the recorded iterations take tokens / cameras / outputs from the workspace; the scene's pointers are never read)
    scene.tokens = scene.camera = scene.T_camera_pseudoCam = scene.T_world_pseudoCam = scene.T_world_local = reinterpret_cast<const float*>(workspace);
    int rc = check_scene(h, &scene);
    if (rc) return rc;
    Workspace ws;
    carve_workspace(h, B, V, hh, ww, &ws, h->batch_invariant);
    if (workspace_bytes < (size_t)ws.total * sizeof(float)) return fail(PARQ_ERR_WORKSPACE, "workspace too small: %zu < %zu", workspace_bytes, (size_t)ws.total * sizeof(float));
    // Lazily built state must not end up inside the graph (it would be rebuilt by every replay): the derived inference weights are
    // settled on the caller's stream, in front of the first replay.  (The mode's 16-bit copy of W_kv belongs to the K/V projection,
    // which every replay launches directly.)
    hipStream_t s = (hipStream_t)stream;
    if (!h->derived_valid) { rc = build_derived_weights(h, s); if (rc) return rc; }
    // recorded on a stream of the handle's own (the caller's may be the legacy default stream, which cannot capture); relaxed mode:
    // other threads of the process (a data loader allocating, another module's launches) are not affected by the capture
    if (!h->cap_stream) HIPCHK(hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking));
    HIPCHK(hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeRelaxed));
    rc = forward_iterations(h, &scene, (float*)workspace, ws, nullptr, h->cap_stream, true);
    parq_graph* g = new parq_graph();
    const hipError_t e = hipStreamEndCapture(h->cap_stream, &g->graph);
    if (rc != PARQ_OK || e != hipSuccess || !g->graph) {
        if (g->graph) (void)hipGraphDestroy(g->graph);
        delete g;
        (void)hipGetLastError();
        return rc != PARQ_OK ? rc : fail(PARQ_ERR_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
    }
    (void)hipGraphGetNodes(g->graph, nullptr, &g->nodes);
    const hipError_t e2 = hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0);
    if (e2 != hipSuccess) {
        (void)hipGraphDestroy(g->graph);
        delete g;
        return fail(PARQ_ERR_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(e2));
    }
    g->key = graph_key(h, B, V, hh, ww, workspace);
    *out = g;
    return PARQ_OK;
}

int parq_forward_replay(parq_handle h, parq_graph_t g, const parq_scene* scene, void* workspace, size_t workspace_bytes,
                        const parq_outputs* outs, parq_stream stream) {
    if (!g || !g->exec) return fail(PARQ_ERR_ARG, "NULL graph");
    Workspace ws;
    int rc = forward_checks(h, scene, workspace, workspace_bytes, outs, &ws);
    if (rc) return rc;
    if (!(g->key == graph_key(h, scene->B, scene->V, scene->h, scene->w, workspace)) || !h->derived_valid)
        return fail(PARQ_ERR_STATE, "parq_forward_replay: the graph was recorded for another shape / workspace / weight arena / range mirror or under "
                                    "other attention settings (mode, head tiers, seam fusion, batch invariance) or token type: capture again");
    hipStream_t s = (hipStream_t)stream;
    h->map_recs.erase(workspace);
    h->cache_recs.erase(workspace);
    // launched directly with THIS call's pointers: prologue (which also leaves them in the workspace for the recorded part) + K/V projection
    rc = do_prepare(h, scene, (float*)workspace, ws, s, false, outs, true);
    if (rc) return rc;
    HIPCHK(hipGraphLaunch(g->exec, s));
    h->ref_state = 0;
    h->prepared = false;
    h->note_iteration(workspace, scene, h->I - 1, 1);
    h->note_cache(workspace, scene);
    return PARQ_OK;
}

/* ---- a forward that re-projects the listed views only (include/parq_hip.h) ---------------------------------------------------------- */
// view slots -> maximal runs of adjacent slots -> token rows, widened outward to `gran` rows and clamped to N; runs that touch
// after widening are merged (parq_amd/view_window.py row_ranges is the same function, for callers that plan ahead)
static RowRuns view_row_runs(std::vector<int> views, int hw, int64_t N, int gran) {
    std::sort(views.begin(), views.end());
    RowRuns out;
    for (int v : views) {
        const int64_t r0 = (int64_t)v * hw / gran * gran;
        int64_t r1 = ((int64_t)(v + 1) * hw + gran - 1) / gran * gran;
        if (r1 > N) r1 = N;
        if (!out.empty() && r0 <= out.back().second) { if (r1 > out.back().second) out.back().second = (int)r1; }
        else out.emplace_back((int)r0, (int)r1);
    }
    return out;
}

int (parq_forward_views)(parq_handle h, parq_graph_t g, const parq_scene* scene, void* workspace, size_t workspace_bytes,
                         const parq_outputs* outs, const int32_t* views, int32_t n_views, int64_t* rows_projected, parq_stream stream) {
    if (g && !g->exec) return fail(PARQ_ERR_ARG, "NULL graph");
    Workspace ws;
    int rc = forward_checks(h, scene, workspace, workspace_bytes, outs, &ws);
    if (rc) return rc;
    const int V = scene->V, hw = scene->h * scene->w;
    const int64_t N = (int64_t)V * hw;
    if (n_views < 0 || n_views > V || (n_views > 0 && !views)) return fail(PARQ_ERR_ARG, "parq_forward_views: n_views = %d for %d views (or a NULL list)", n_views, V);
    if ((int64_t)scene->B * N > (int64_t)INT32_MAX) return fail(PARQ_ERR_ARG, "B*N too large");
    std::vector<int> list(views, views + n_views);
    {
        std::vector<char> seen((size_t)V, 0);
        for (int v : list) {
            if (v < 0 || v >= V) return fail(PARQ_ERR_ARG, "parq_forward_views: view index %d outside [0, %d)", v, V);
            if (seen[(size_t)v]) return fail(PARQ_ERR_ARG, "parq_forward_views: view index %d listed twice", v);
            seen[(size_t)v] = 1;
        }
    }
    if (g && (!(g->key == graph_key(h, scene->B, scene->V, scene->h, scene->w, workspace)) || !h->derived_valid))
        return fail(PARQ_ERR_STATE, "parq_forward_views: the graph was recorded for another shape / workspace / weight arena / range mirror or under "
                                    "other attention settings (mode, head tiers, seam fusion, batch invariance) or token type: capture again");
    const bool all = n_views == V;
    if (!all) {
        // the views that are not listed are read from the cache as it stands: it must have been built whole in the handle's present state
        const auto it = h->cache_recs.find(workspace);
        if (it == h->cache_recs.end())
            return fail(PARQ_ERR_STATE, "parq_forward_views: no record of a whole K/V cache in this workspace (never filled, or rewritten by parq_prepare / "
                                        "parq_forward_train / a view-sharded iteration / a re-pack since): list all %d views", V);
        const CacheRec& r = it->second;
        const char* what = nullptr;
        if (r.B != scene->B || r.V != scene->V || r.h != scene->h || r.w != scene->w) what = "shape";
        else if (r.mode != h->attn_mode) what = "attention mode";
        else if (r.safe != h->safe_heads()) what = "head-tier mask";
        else if (r.tok != h->tok_type) what = "token type";
        else if (r.arena != h->arena || r.pack_gen != h->pack_gen) what = "packed weight arena";
        else if (r.inv != (h->batch_invariant ? 1 : 0)) what = "batch-invariant flag";
        else if (r.mirror != h->range_mirror) what = "range mirror word";      // (only the handle's present word is ever read below)
        if (what) return fail(PARQ_ERR_STATE, "parq_forward_views: the K/V cache in this workspace was built under another %s: list all %d views", what, V);
        if (h->range_mirror && __atomic_load_n(h->range_mirror, __ATOMIC_ACQUIRE) != 0)
            return fail(PARQ_ERR_STATE, "parq_forward_views: a range / too-peaked flag is raised in the mirror word of the forward that built this cache: "
                                        "list all %d views, so that the flag is raised again rather than lost with the rows that are skipped", V);
    }
    RowRuns runs;
    int64_t rows = N;
    if (!all) {
        if (h->cache_mode()) {
            runs = view_row_runs(list, hw, N, kvproj_granule(h, scene->B, N));
            rows = 0;
            for (const auto& r : runs) rows += r.second - r.first;
        } else {
            // attention mode 0 has no cache layout to address by key: one fp32 GEMM over all rows, or none
            if (n_views > 0) runs.emplace_back(0, (int)N);
            rows = n_views > 0 ? N : 0;
        }
    }
    hipStream_t s = (hipStream_t)stream;
    h->map_recs.erase(workspace);
    h->cache_recs.erase(workspace);
    rc = do_prepare(h, scene, (float*)workspace, ws, s, false, g ? outs : nullptr, true, all ? nullptr : &runs);
    if (rc) return rc;
    if (g) {
        HIPCHK(hipGraphLaunch(g->exec, s));
        h->ref_state = 0;
        h->prepared = false;
    } else {
        rc = forward_iterations(h, scene, (float*)workspace, ws, outs, s, false);
        if (rc) return rc;
    }
    h->note_iteration(workspace, scene, h->I - 1, 1);
    h->note_cache(workspace, scene);
    if (rows_projected) *rows_projected = rows;
    return PARQ_OK;
}

/* ---- cross-attention maps (include/parq_hip.h; attn_map.hip) --------------------------------------------------------------------- */
size_t parq_attention_map_scratch_bytes(parq_handle h, int32_t B, int32_t V, int32_t hh, int32_t ww, int32_t n_sel) {
    if (!h || B < 1 || V < 1 || hh < 1 || ww < 1) return 0;
    if ((int64_t)V * hh * ww > INT32_MAX) return 0;
    const int nsel = n_sel > 0 ? n_sel : h->Q;
    return attn_map_scratch_bytes(B, h->H, h->dh, V * hh * ww, V, hh * ww, nsel);
}

int parq_attention_map(parq_handle h, const parq_scene* scene, const void* workspace, size_t workspace_bytes, const int32_t* query_index,
                       int32_t n_sel, int32_t what, int32_t out_type, void* out, void* scratch, size_t scratch_bytes, parq_stream stream) {
    if (!h || !workspace || !out || !scratch) return fail(PARQ_ERR_ARG, "NULL argument");
    if (!scene || scene->B < 1 || scene->V < 1 || scene->h < 2 || scene->w < 2) return fail(PARQ_ERR_ARG, "bad scene dims");
    if (what < 0 || what > 2) return fail(PARQ_ERR_ARG, "what must be 0 (head mean), 1 (per head) or 2 (view mass)");
    if (out_type != PARQ_MAP_F32 && out_type != PARQ_MAP_F16) return fail(PARQ_ERR_ARG, "out_type must be 0 (fp32) or 1 (fp16)");
    if (query_index ? n_sel < 1 : (n_sel != 0 && n_sel != h->Q)) return fail(PARQ_ERR_ARG, "n_sel must be >= 1 with query_index, 0 or num_queries without");
    if (((uintptr_t)scratch & 15) != 0) return fail(PARQ_ERR_ARG, "scratch must be 16-byte aligned");
    const auto it = h->map_recs.find(workspace);
    if (it == h->map_recs.end()) return fail(PARQ_ERR_STATE, "parq_attention_map: no iteration has run in this workspace since it was prepared");
    const MapRec& r = it->second;
    if (r.state == 2) return fail(PARQ_ERR_STATE, "parq_attention_map: the last call in this workspace was a training forward; maps are computed after inference forwards and parq_iterate only");
    if (r.state == 3) return fail(PARQ_ERR_STATE, "parq_attention_map: the last iteration in this workspace was view-sharded (its keys are one rank's views); not supported");
    if (r.B != scene->B || r.V != scene->V || r.h != scene->h || r.w != scene->w) return fail(PARQ_ERR_ARG, "parq_attention_map: the scene dims differ from those of the iteration that ran in this workspace");
    if (r.mode != h->attn_mode || r.tok != h->tok_type)
        return fail(PARQ_ERR_STATE, "parq_attention_map: attention mode / token type changed since the iteration ran (the workspace is carved differently)");
    const int B = scene->B, V = scene->V, C = h->C;
    const int64_t N64 = (int64_t)V * scene->h * scene->w;
    if (N64 > INT32_MAX) return fail(PARQ_ERR_ARG, "too many keys");
    const int N = (int)N64;
    Workspace ws;
    carve_workspace(h, B, V, scene->h, scene->w, &ws, h->batch_invariant);
    if (workspace_bytes < (size_t)ws.total * sizeof(float)) return fail(PARQ_ERR_WORKSPACE, "workspace too small: %zu < %zu", workspace_bytes, (size_t)ws.total * sizeof(float));
    const int nsel = query_index ? n_sel : h->Q;
    const size_t need = attn_map_scratch_bytes(B, h->H, h->dh, N, V, scene->h * scene->w, nsel);
    if (scratch_bytes < need) return fail(PARQ_ERR_WORKSPACE, "scratch too small: %zu < %zu", scratch_bytes, need);
    const float* wsp = reinterpret_cast<const float*>(workspace);
    AttnMapArgs a;
    memset(&a, 0, sizeof(a));
    a.B = B; a.H = h->H; a.dh = h->dh; a.C = C; a.N = N; a.V = V; a.hw = scene->h * scene->w; a.nsel = nsel;
    a.what = what; a.out_f16 = out_type == PARQ_MAP_F16; a.out = out;
    if (h->cache_mode()) {
        // the layer's cache, read as the forward's cross-attention reads it (do_iterate)
        a.kbase = reinterpret_cast<const char*>(wsp + ws.kvc) + (size_t)r.li * kvsplit_cache_bytes(B, h->vheads(), N, h->terms());
        // (the head tiers the cache was WRITTEN under, which a guard may have changed on the handle since: ctx terms_for with r.safe)
        const bool m4 = h->attn_mode == 4 && C == 256 && flash_split8_supported(h->dh, N);
        const int tf = (m4 && r.safe != h->all_heads()) ? 8 : h->terms();
        if (tf == 8) {
            a.klayout = kMapStage8;
            a.safe_mask = r.safe;
            a.head_bytes = a.safe_mask ? kv_blk_head_bytes(N, 3) : kv_stage_head_bytes(N);
        } else if (tf == 3) {
            a.klayout = kMapSplit3; a.head_bytes = kv_blk_head_bytes(N, 3);
        } else {
            a.klayout = h->kind() == kBF16 ? kMapBF16 : kMapF16; a.head_bytes = kv_blk_head_bytes(N, 1);
        }
    } else {
        a.klayout = kMapF32;
        a.kbase = wsp + ws.kv + (int64_t)r.li * B * 2 * N * C;
    }
    HIPCHK(launch_attn_map(a, wsp + ws.qc, query_index, h->Q, scratch, (hipStream_t)stream));
    return PARQ_OK;
}

int64_t parq_graph_nodes(parq_graph_t g) { return g ? (int64_t)g->nodes : 0; }

int parq_graph_destroy(parq_graph_t g) {
    if (!g) return PARQ_OK;
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    if (g->graph) (void)hipGraphDestroy(g->graph);
    delete g;
    return PARQ_OK;
}

int parq_set_progress(parq_handle h, int32_t* host_visible_word, int32_t epoch) {
    if (!h) return fail(PARQ_ERR_ARG, "NULL handle");
    h->progress_word = host_visible_word;
    h->progress_epoch = epoch;
    return PARQ_OK;
}

int32_t parq_mirror_take(int32_t* host_visible_flag) {
    return host_visible_flag ? __atomic_exchange_n(host_visible_flag, 0, __ATOMIC_ACQ_REL) : 0;
}

int parq_workspace_lookup(parq_handle h, int32_t B, int32_t V, int32_t hh, int32_t ww, const char* name,
                          size_t* offset_floats, size_t* numel) {
    if (!h || !name || !offset_floats || !numel) return fail(PARQ_ERR_ARG, "NULL argument");
    Workspace ws;
    carve_workspace(h, B, V, hh, ww, &ws, h->batch_invariant);
    const int64_t C = h->C, Q = h->Q, F = h->F, M = (int64_t)B * Q, N = (int64_t)V * hh * ww;
    struct E { const char* n; int64_t off, cnt; };
    const E table[] = {
        {"T_camera_local_f64", ws.T_cl, (int64_t)B * V * 24},
        {"kv_cache", ws.kv, h->cache_mode() ? 0 : (int64_t)h->nl * B * 2 * N * C},
        {"kv_cache16", ws.kvc, h->cache_mode() ? (int64_t)(h->nl * kvsplit_cache_bytes(B, h->vheads(), (int)N, h->terms()) / sizeof(float)) : 0},
        {"ref", ws.ref, M * 3}, {"ref_next", ws.ref_next, M * 3}, {"posemb", ws.emb, M * 384}, {"pos_hidden", ws.pe_h, M * C}, {"pos_feat", ws.pos, M * C},
        {"tgt", ws.tgt, M * C}, {"self_qkv", ws.qkv, M * 3 * C}, {"attn", ws.attn, M * C}, {"xa_prenorm1", ws.xa, M * C},
        {"cross_q", ws.qc, M * C}, {"xb_prenorm2", ws.xb, M * C}, {"ffn_hidden", ws.ffn, M * F},
        {"xc_prenorm3", ws.xc, M * C}, {"heads1", ws.h1, M * h->NH1}, {"heads2", ws.h2, M * 2 * C},
        {"gn_sums_f64", ws.inv ? ws.gn_inv : ws.gn_sums, (int64_t)2 * B * 4 * (ws.inv ? ws.gn_slots : kGnSlots) * 2}, {"ln1_stats", ws.ln1, M * 2}, {"ln2_stats", ws.ln2, M * 2},
        {"flags", ws.flags, 64}};
    for (const E& e : table)
        if (strcmp(e.n, name) == 0) { *offset_floats = (size_t)e.off; *numel = (size_t)e.cnt; return PARQ_OK; }
    return fail(PARQ_ERR_ARG, "unknown workspace buffer '%s'", name);
}

int parq_set_attention_mode(parq_handle h, int32_t mode) {
    if (!h || mode < 0 || mode > 4) return fail(PARQ_ERR_ARG, "attention mode must be 0 (fp32 MFMA), 1 (split fp16x3), 2 (fp16), 3 (bf16) or 4 (split, fp8 cross terms)");
    if (mode == 4 && !(h->dh == 64 || h->dh == 256)) return fail(PARQ_ERR_ARG, "attention mode 4 needs a head dim of 64 (256: runs as mode 1)");
    if (mode >= 2 && mode <= 3 && !((h->dh == 64 && h->C <= 256 && (2 * h->C) % 256 == 0) || (h->dh == 256 && h->C % 128 == 0 && (h->C == 256 || kvproj_big_on())))) 
        return fail(PARQ_ERR_ARG, "the fp16 / bf16 attention modes need head dim 64 with dim in {128, 256}, or head dim 256 with dim a multiple of 128");
    h->attn_mode = mode;
    h->prepared = false;
    return PARQ_OK;
}

int parq_set_token_type(parq_handle h, int32_t type) {
    if (!h) return fail(PARQ_ERR_ARG, "NULL handle");
    if (type != kTokF32 && type != kTokF16 && type != kTokBF16) return fail(PARQ_ERR_ARG, "token type must be 0 (fp32), 1 (fp16) or 2 (bf16), not %d", type);
    if (type != h->tok_type) h->prepared = false;     // a prepared scene's tokens were read as the previous type
    h->tok_type = type;
    return PARQ_OK;
}

int parq_set_train_token_type(parq_handle h, int32_t type) {
    if (!h) return fail(PARQ_ERR_ARG, "NULL handle");
    if (type != kTokF32 && type != kTokF16 && type != kTokBF16) return fail(PARQ_ERR_ARG, "token type must be 0 (fp32), 1 (fp16) or 2 (bf16), not %d", type);
    h->train_tok_type = type;
    return PARQ_OK;
}

int parq_set_head_tiers(parq_handle h, uint32_t safe_mask, int32_t poison_on_peaked) {
    if (!h) return fail(PARQ_ERR_ARG, "NULL handle");
    if (safe_mask != 0 && h->H > 16) return fail(PARQ_ERR_ARG, "per-head tiers need at most 16 heads");
    if ((safe_mask & h->all_heads()) != h->safe_heads()) h->prepared = false;      // the K/V cache is laid out per tier
    h->safe_mask = safe_mask;
    h->peaky_poison = poison_on_peaked ? 1 : 0;
    return PARQ_OK;
}

int parq_set_seam_fusion(parq_handle h, int32_t on) {
    if (!h) return fail(PARQ_ERR_ARG, "NULL handle");
    h->seam_fusion = on != 0;
    return PARQ_OK;
}

int parq_set_batch_invariant(parq_handle h, int32_t on) {
    if (!h) return fail(PARQ_ERR_ARG, "NULL handle");
    if (on != 0 && on != 1) return fail(PARQ_ERR_ARG, "parq_set_batch_invariant: on must be 0 or 1");
    if ((on != 0) != h->batch_invariant) h->prepared = false;      // the workspace is carved differently: a prepared scene is prepared again
    h->batch_invariant = on != 0;
    return PARQ_OK;
}

int parq_set_range_mirror(parq_handle h, int32_t* host_visible_flag) {
    if (!h) return fail(PARQ_ERR_ARG, "NULL handle");
    h->range_mirror = host_visible_flag;
    return PARQ_OK;
}

/* ---- training ---------------------------------------------------- */
size_t parq_train_workspace_bytes(parq_handle h, int32_t B, int32_t V, int32_t hh, int32_t ww) {
    if (!h || B < 1 || V < 1 || hh < 1 || ww < 1) return 0;
    Workspace ws;
    carve_workspace(h, B, V, hh, ww, &ws, false);
    return (size_t)ws.train_total * sizeof(float);
}

int parq_set_dropout(parq_handle h, float p, uint32_t seed) {
    if (!h || !(p >= 0.f) || !(p < 1.f)) return fail(PARQ_ERR_ARG, "dropout probability must be in [0, 1)");
    h->drop_p = p;
    h->drop_seed = seed;
    return PARQ_OK;
}

int parq_k_dropout_mask(parq_handle h, int32_t iteration, int32_t site, int64_t rows, int64_t cols, float* out, parq_stream stream) {
    if (!h || !out || rows < 1 || cols < 1 || rows * cols > INT32_MAX) return fail(PARQ_ERR_ARG, "bad argument");
    if (!(h->drop_p > 0.f)) return fail(PARQ_ERR_STATE, "dropout is off");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(launch_fill(out, 1.f, rows * cols, s));
    HIPCHK(launch_dropout_apply(out, out, (int)rows, (int)cols, h->drop_p, h->site_seed(iteration, site), s));
    return PARQ_OK;
}

size_t parq_grad_arena_bytes(parq_handle h) { return h ? (size_t)h->ar.rowmajor_total * sizeof(float) : 0; }

int parq_forward_train(parq_handle h, const parq_scene* scene, void* workspace, size_t workspace_bytes, const parq_outputs* outs,
                       parq_stream stream) {
    if (!h || !workspace) return fail(PARQ_ERR_ARG, "NULL argument");
    if (h->tok_type != h->train_tok_type)
        return fail(PARQ_ERR_ARG, "parq_forward_train reads fp32 tokens only unless parq_set_train_token_type names the token type (token type %d, training token type %d)", h->tok_type, h->train_tok_type);
    if (!h->packed) return fail(PARQ_ERR_STATE, "parq_pack_weights must be called first");
    if (h->dh % 16 != 0) return fail(PARQ_ERR_ARG, "training needs a head dim that is a multiple of 16");
    int rc = check_scene(h, scene);
    if (rc) return rc;
    rc = check_outs(outs);
    if (rc) return rc;
    Workspace ws;
    carve_workspace(h, scene->B, scene->V, scene->h, scene->w, &ws, false);
    if (workspace_bytes < (size_t)ws.train_total * sizeof(float)) return fail(PARQ_ERR_WORKSPACE, "training workspace too small: %zu < %zu", workspace_bytes, (size_t)ws.train_total * sizeof(float));
    float* wsp = (float*)workspace;
    hipStream_t s = (hipStream_t)stream;
    h->note_iteration(workspace, scene, h->I - 1, 2);     // (before anything is enqueued: whatever an inference forward left here is gone)
    h->cache_recs.erase(workspace);
    rc = do_prepare(h, scene, wsp, ws, s, true);
    if (rc) return rc;
    const int64_t M = (int64_t)scene->B * h->Q;
    // the reference points of iteration k live in that iteration's stash (initial_ref wrote ws.ref)
    HIPCHK(hipMemcpyAsync(wsp + ws.shift(0) + ws.refk, wsp + ws.ref, (size_t)M * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    for (int k = 0; k < h->I; ++k) {
        parq_outputs o;
        o.pred_logits = outs->pred_logits + k * M * h->ncls;
        o.center_unnormalized = outs->center_unnormalized + k * M * 3;
        o.size_unnormalized = outs->size_unnormalized + k * M * 3;
        o.ortho6d = outs->ortho6d + k * M * 6;
        o.sem_cls_prob = outs->sem_cls_prob + k * M * h->ncls;
        o.coord_pos = outs->coord_pos + k * M * 3;
        const bool last = k + 1 == h->I;
        float* ref_next = last ? wsp + ws.ref_next : wsp + ws.shift(k + 1) + ws.refk;
        float* emb_next = last ? wsp + ws.g_emb : wsp + ws.shift(k + 1) + ws.emb;
        rc = do_iterate(h, scene, wsp, ws, k, wsp + ws.shift(k) + ws.refk, true, &o, ref_next, s, ws.shift(k), emb_next, true);   // ws.emb of iteration 0: prologue
        if (rc) return rc;
        // outputs of iteration k are final from here on: a host that matches predictions to boxes per iteration (the set loss)
        // can start on them while the later iterations run (parq_wait_iteration)
        if (k < 16) {
            if (!h->iter_done[k]) HIPCHK(hipEventCreateWithFlags(&h->iter_done[k], hipEventDisableTiming));
            HIPCHK(hipEventRecord(h->iter_done[k], s));
            h->iter_recorded[k] = true;
        }
    }
    // (after the iterations, which do not read it: the stream gets to this while the host evaluates the loss)
    if (h->cache_mode() && !bwd_reads_cache(h, ws)) {
        // cache modes: the forward streams the 16-bit cache; the backward gets fp32 K / V rebuilt from it (hi + lo; in the fp16 /
        // bf16 modes the rounded values themselves: the gradient is taken straight through the rounding).  Not at head dim 64 with
        // the batched backward: attn_bwd_split2_kernel reads the cache itself (bwd_reads_cache)
        const int64_t N = (int64_t)scene->V * scene->h * scene->w;
        const int C = h->C, dh = h->dh, H = h->H, B = scene->B;
        for (int li = 0; li < h->nl; ++li) {
            const char* cache = reinterpret_cast<const char*>(wsp + ws.kvc) + (size_t)li * kvsplit_cache_bytes(B, h->vheads(), (int)N, h->terms());
            float* kv = wsp + ws.kv_train + (int64_t)li * B * 2 * N * C;
            HIPCHK(launch_kvsplit_to_f32(cache, B, h->vheads(), (int)N, kv, kv + (int64_t)H * N * dh, 2 * N * C, N * dh, 2 * N * C, N * dh, s,
                                         dh / 64, h->terms(), h->kind()));
        }
    }
    h->ref_state = 0;
    h->prepared = false;
    return PARQ_OK;
}

int parq_wait_iteration(parq_handle h, int32_t k) {
    if (!h || k < 0 || k >= 16 || k >= h->I) return fail(PARQ_ERR_ARG, "bad iteration index");
    if (!h->iter_recorded[k]) return fail(PARQ_ERR_STATE, "parq_wait_iteration: no parq_forward_train has been enqueued");
    HIPCHK(hipEventSynchronize(h->iter_done[k]));
    return PARQ_OK;
}

int parq_backward(parq_handle h, const parq_scene* scene, void* workspace, size_t workspace_bytes, const parq_outputs* outs,
                  const parq_output_grads* g, float* grad_arena, float* d_tokens, parq_stream stream) {
    if (!h || !workspace || !outs || !g || !grad_arena) return fail(PARQ_ERR_ARG, "NULL argument");
    if (h->tok_type != h->train_tok_type)
        return fail(PARQ_ERR_ARG, "parq_backward reads fp32 tokens only unless parq_set_train_token_type names the token type (token type %d, training token type %d)", h->tok_type, h->train_tok_type);
    if (!h->packed) return fail(PARQ_ERR_STATE, "parq_pack_weights must be called first");
    int rc = check_scene(h, scene);
    if (rc) return rc;
    Workspace ws;
    carve_workspace(h, scene->B, scene->V, scene->h, scene->w, &ws, false);
    if (workspace_bytes < (size_t)ws.train_total * sizeof(float)) return fail(PARQ_ERR_WORKSPACE, "training workspace too small");
    float* wsp = (float*)workspace;
    hipStream_t s = (hipStream_t)stream;
    const int64_t M = (int64_t)scene->B * h->Q;
    const int64_t N = (int64_t)scene->V * scene->h * scene->w;
    if (h->deterministic && h->dh == 32) return fail(PARQ_ERR_ARG, "deterministic mode: no fixed-order attention backward at head dim 32");
    // deterministic mode: every reduction below runs in its fixed-order form (common.hpp DetScratch), on the caller's stream only
    DetScope det(h->deterministic ? wsp + ws.g_det : nullptr, ws.g_det_floats);
    HIPCHK(hipMemsetAsync(grad_arena, 0, (size_t)h->ar.rowmajor_total * sizeof(float), s));
    if (!ws.bwd_batched) HIPCHK(hipMemsetAsync(wsp + ws.g_kv, 0, (size_t)h->nl * scene->B * 2 * N * h->C * sizeof(float), s));
    if (d_tokens) HIPCHK(hipMemsetAsync(d_tokens, 0, (size_t)scene->B * N * h->C * sizeof(float), s));
    auto iter_io = [&](int k) {
        BwdIO io;
        io.g_logits = g->pred_logits ? g->pred_logits + k * M * h->ncls : nullptr;
        io.g_center = g->center_unnormalized ? g->center_unnormalized + k * M * 3 : nullptr;
        io.g_size = g->size_unnormalized ? g->size_unnormalized + k * M * 3 : nullptr;
        io.g_rot = g->ortho6d ? g->ortho6d + k * M * 6 : nullptr;
        io.center = outs->center_unnormalized + k * M * 3;
        io.size = outs->size_unnormalized + k * M * 3;
        return io;
    };
    for (int i = 0; i < 2; ++i)
        if (!h->bucket_done[i]) HIPCHK(hipEventCreateWithFlags(&h->bucket_done[i], hipEventDisableTiming));
    auto finish = [&](bool early_too) -> int {          // the end of the backward: every gradient is final
        const int r = do_backward_kvproj(h, scene, wsp, ws, grad_arena, d_tokens, s);
        if (r) return r;
        if (early_too) HIPCHK(hipEventRecord(h->bucket_done[0], s));
        HIPCHK(hipEventRecord(h->bucket_done[1], s));
        h->bucket_recorded = true;
        return PARQ_OK;
    };
    if (!ws.bwd_batched) {
        for (int k = h->I - 1; k >= 0; --k) {
            rc = do_backward_iter(h, scene, wsp, ws, k, iter_io(k), grad_arena, d_tokens, s);
            if (rc) return rc;
        }
        return finish(true);
    }
    // ---- batched: (1) every iteration from its outputs down to dO, (2) ONE cross-attention backward over all iterations
    // (dK / dV written once, accumulated in registers), (3) every iteration from its dQ down to the sampled features
    const int I = h->I, B = scene->B, C = h->C, H = h->H, dh = h->dh, Q = h->Q;
    rc = do_backward_transposes(h, wsp, ws, 0, s);
    if (rc) return rc;
    // the iterations of a phase on ws.g_sets streams (the caller's + the handle's own), joined back before the phase ends
    const int ns = h->profiling ? 1 : ws.g_sets;
    if (ns > 1 && !h->fork_ev) {
        HIPCHK(hipEventCreateWithFlags(&h->fork_ev, hipEventDisableTiming));
        for (int i = 0; i < 7; ++i) {
            HIPCHK(hipStreamCreateWithFlags(&h->aux_stream[i], hipStreamNonBlocking));
            HIPCHK(hipEventCreateWithFlags(&h->join_ev[i], hipEventDisableTiming));
        }
    }
    auto run_phase = [&](int phase) -> int {
        if (ns > 1) {
            HIPCHK(hipEventRecord(h->fork_ev, s));
            for (int i = 0; i + 1 < ns; ++i) HIPCHK(hipStreamWaitEvent(h->aux_stream[i], h->fork_ev, 0));
        }
        int r = PARQ_OK;
        for (int k = I - 1, n = 0; k >= 0 && r == PARQ_OK; --k, ++n) {
            const int set = n % ns;
            r = do_backward_iter(h, scene, wsp, ws, k, iter_io(k), grad_arena, d_tokens, set == 0 ? s : h->aux_stream[set - 1], phase, set);
        }
        // joined on the error path too: whatever the auxiliary streams were given must not outlive the call on a stream the
        // caller does not know about
        for (int i = 0; i + 1 < ns; ++i) {
            const hipError_t e1 = hipEventRecord(h->join_ev[i], h->aux_stream[i]);
            const hipError_t e2 = hipStreamWaitEvent(s, h->join_ev[i], 0);
            if (r == PARQ_OK && (e1 != hipSuccess || e2 != hipSuccess)) r = fail(PARQ_ERR_HIP, "joining the backward's auxiliary streams failed");
        }
        return r;
    };
    rc = run_phase(1);
    if (rc) return rc;
    // gradients of everything above the cross-attention (cross out-proj, FFN, norm2 / norm3, the heads) are final: a data-parallel
    // caller may start all-reducing that bucket on another stream while the attention backward runs (parq_backward_wait_bucket)
    HIPCHK(hipEventRecord(h->bucket_done[0], s));
    {
        int64_t q_off[16], lse_off[16];
        uint32_t seeds[16];
        for (int k = 0; k < I; ++k) {
            q_off[k] = ws.shift(k);
            lse_off[k] = ws.shift(k);
            seeds[k] = h->site_seed(k, 2);
        }
        const float* kv = wsp + (h->cache_mode() ? ws.kv_train : ws.kv);
        float* gkv = wsp + ws.g_kv;
        const int64_t MC = M * C;
        HIPCHK(hipMemsetAsync(wsp + ws.g_dq, 0, (size_t)I * MC * sizeof(float), s));      // the partial-sum reduction accumulates
        HIPCHK(launch_attn_bwd_batched(wsp + ws.qc, q_off, (int64_t)Q * C, dh, C, kv, 2 * N * C, N * dh, dh, kv + (int64_t)H * N * dh,
                                       2 * N * C, N * dh, dh, wsp + ws.g_do, MC, (int64_t)Q * C, dh, C, wsp + ws.lse_c, lse_off,
                                       wsp + ws.g_Dall, (int64_t)B * H * flash_lq_pad(Q), wsp + ws.g_dq, MC, (int64_t)Q * C, dh, C, gkv,
                                       2 * N * C, dh, 2 * C, gkv + C, 2 * N * C, dh, 2 * C, B, H, Q, (int)N, dh, I, s, wsp + ws.g_dqp,
                                       h->drop_p, seeds, reinterpret_cast<unsigned int*>(wsp + ws.g_bs),
                                       reinterpret_cast<unsigned int*>(wsp + ws.g_kvmax), wsp + ws.g_pack, wsp + ws.g_mat,
                                       bwd_reads_cache(h, ws) ? reinterpret_cast<const void*>(wsp + ws.kvc) : nullptr,
                                       h->terms_for(N, true, bwd_reads_cache(h, ws)), h->kind()));
        if (dh == 256) {                          // max |dK|, |dV| for the split-precision dW_kv GEMM (the dh = 64 kernel records it itself)
            HIPCHK(hipMemsetAsync(wsp + ws.g_kvmax, 0, sizeof(unsigned int), s));
            HIPCHK(launch_absmax(gkv, (int64_t)B * 2 * N * C, reinterpret_cast<unsigned int*>(wsp + ws.g_kvmax), s));
        }
    }
    rc = run_phase(2);
    if (rc) return rc;
    return finish(false);
}

/* Data-parallel gradient buckets (train.py:103 DDP buckets its all-reduces and overlaps them with the backward): the gradient
 * arena in the order its parts become final inside parq_backward.  Bucket 0 = [offset, offset + count) floats final after phase
 * 1 of the batched backward (cross out-proj, FFN, norm2, norm3, every head: everything above the cross-attention), bucket 1 =
 * the rest of the arena's front, final at the end.  With unshared layer weights (several layers interleave) bucket 0 is empty
 * and bucket 1 is the whole arena. */
int parq_grad_bucket(parq_handle h, int32_t bucket, int64_t* offset, int64_t* count) {
    if (!h || !offset || !count || bucket < 0 || bucket > 1) return fail(PARQ_ERR_ARG, "bad argument");
    const Arena& ar = h->ar;
    const bool two = h->nl == 1 && ar.early_end > ar.early_begin;
    if (bucket == 0) { *offset = two ? ar.early_begin : 0; *count = two ? ar.early_end - ar.early_begin : 0; }
    else { *offset = 0; *count = two ? ar.early_begin : ar.rowmajor_total; }
    return PARQ_OK;
}

int parq_backward_wait_bucket(parq_handle h, int32_t bucket, parq_stream stream) {
    if (!h || bucket < 0 || bucket > 1) return fail(PARQ_ERR_ARG, "bad argument");
    if (!h->bucket_recorded) return fail(PARQ_ERR_STATE, "parq_backward_wait_bucket: no parq_backward has been enqueued");
    HIPCHK(hipStreamWaitEvent((hipStream_t)stream, h->bucket_done[bucket], 0));
    return PARQ_OK;
}

/* offset (in floats) and element count of a named reference tensor inside the packed weight / gradient arena;
 * `rows` x `cols` with row stride `ld` (fused head matrices are row slices of a wider block) */
int parq_arena_lookup(parq_handle h, const char* name, int64_t* offset, int64_t* rows, int64_t* cols, int64_t* ld) {
    if (!h || !name || !offset || !rows || !cols || !ld) return fail(PARQ_ERR_ARG, "NULL argument");
    const int64_t C = h->C, F = h->F, Q = h->Q, ncls = h->ncls;
    const Arena& ar = h->ar;
    struct E { std::string n; int64_t off, r, c; };
    std::vector<E> t;
    for (int li = 0; li < h->nl; ++li) {
        const LayerW& L = ar.layers[li];
        const std::string p = "parq_module.decoder.layers." + std::to_string(li) + ".";
        t.push_back({p + "self_attn.in_proj_weight", L.self_in_w, 3 * C, C}); t.push_back({p + "self_attn.in_proj_bias", L.self_in_b, 1, 3 * C});
        t.push_back({p + "self_attn.out_proj.weight", L.self_out_w, C, C}); t.push_back({p + "self_attn.out_proj.bias", L.self_out_b, 1, C});
        t.push_back({p + "multihead_attn.in_proj_weight", L.cross_in_w, 3 * C, C}); t.push_back({p + "multihead_attn.in_proj_bias", L.cross_in_b, 1, 3 * C});
        t.push_back({p + "multihead_attn.out_proj.weight", L.cross_out_w, C, C}); t.push_back({p + "multihead_attn.out_proj.bias", L.cross_out_b, 1, C});
        t.push_back({p + "linear1.weight", L.lin1_w, F, C}); t.push_back({p + "linear1.bias", L.lin1_b, 1, F});
        t.push_back({p + "linear2.weight", L.lin2_w, C, F}); t.push_back({p + "linear2.bias", L.lin2_b, 1, C});
        t.push_back({p + "norm1.weight", L.n1_w, 1, C}); t.push_back({p + "norm1.bias", L.n1_b, 1, C});
        t.push_back({p + "norm2.weight", L.n2_w, 1, C}); t.push_back({p + "norm2.bias", L.n2_b, 1, C});
        t.push_back({p + "norm3.weight", L.n3_w, 1, C}); t.push_back({p + "norm3.bias", L.n3_b, 1, C});
    }
    const std::string d = "parq_module.decoder.";
    const std::string hc = "mlp_heads.center_head.layers.", hr = "mlp_heads.rotation_head.layers.";
    t.push_back({"refpoint.weight", ar.refpoint, Q, 3});
    t.push_back({d + "position_encoder.0.weight", ar.pe0_w, C, 384}); t.push_back({d + "position_encoder.0.bias", ar.pe0_b, 1, C});
    t.push_back({d + "position_encoder.2.weight", ar.pe2_w, C, C}); t.push_back({d + "position_encoder.2.bias", ar.pe2_b, 1, C});
    t.push_back({hc + "0.weight", ar.heads1_w, C, C}); t.push_back({hr + "0.weight", ar.heads1_w + C * C, C, C});
    t.push_back({"mlp_heads.sem_cls_head.layers.0.weight", ar.heads1_w + 2 * C * C, ncls, C});
    t.push_back({"mlp_heads.size_head.layers.0.weight", ar.heads1_w + (2 * C + ncls) * C, 3, C});
    t.push_back({"mlp_heads.sem_cls_head.layers.0.bias", ar.heads1_b + 2 * C, 1, ncls});
    t.push_back({"mlp_heads.size_head.layers.0.bias", ar.heads1_b + 2 * C + ncls, 1, 3});
    t.push_back({hc + "1.weight", ar.gn1_g, 1, C}); t.push_back({hr + "1.weight", ar.gn1_g + C, 1, C});
    t.push_back({hc + "1.bias", ar.gn1_b, 1, C}); t.push_back({hr + "1.bias", ar.gn1_b + C, 1, C});
    t.push_back({hc + "4.weight", ar.heads2_w, C, C}); t.push_back({hr + "4.weight", ar.heads2_w + C * C, C, C});
    t.push_back({hc + "5.weight", ar.gn2_g, 1, C}); t.push_back({hr + "5.weight", ar.gn2_g + C, 1, C});
    t.push_back({hc + "5.bias", ar.gn2_b, 1, C}); t.push_back({hr + "5.bias", ar.gn2_b + C, 1, C});
    t.push_back({hc + "8.weight", ar.heads3_w, 3, C}); t.push_back({hr + "8.weight", ar.heads3_w + 6 * C, 6, C});
    t.push_back({hc + "8.bias", ar.heads3_b, 1, 3}); t.push_back({hr + "8.bias", ar.heads3_b + 6, 1, 6});
    for (const E& e : t)
        if (e.n == name) { *offset = e.off; *rows = e.r; *cols = e.c; *ld = e.c; return PARQ_OK; }
    return fail(PARQ_ERR_ARG, "unknown tensor '%s'", name);
}

int parq_profile_enable(parq_handle h, int32_t on) {
    if (!h) return fail(PARQ_ERR_ARG, "NULL handle");
    h->profiling = on != 0;
    return PARQ_OK;
}

int parq_profile_read(parq_handle h, int32_t which, double* total_ms, int64_t* launches) {
    if (!h || which < 0 || which >= PARQ_PROF_COUNT) return fail(PARQ_ERR_ARG, "bad argument");
    for (auto& e : h->events) {
        HIPCHK(hipEventSynchronize(e.b));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e.a, e.b));
        h->prof_ms[e.which] += ms;
        h->prof_n[e.which] += 1;
        (void)hipEventDestroy(e.a);
        (void)hipEventDestroy(e.b);
    }
    h->events.clear();
    if (total_ms) *total_ms = h->prof_ms[which];
    if (launches) *launches = h->prof_n[which];
    h->prof_ms[which] = 0;
    h->prof_n[which] = 0;
    return PARQ_OK;
}

// ------------------------------------------------------------------ single kernels

int parq_k_camera_local(const float* T_cp, const float* T_wp, const float* T_wl, int32_t B, int32_t V, float* T_cl,
                        parq_stream stream) {
    if (!T_cp || !T_wp || !T_wl || !T_cl || B < 1 || V < 1) return fail(PARQ_ERR_ARG, "bad argument");
    HIPCHK(launch_camera_local(T_cp, T_wp, T_wl, B, V, T_cl, (hipStream_t)stream));
    return PARQ_OK;
}

int parq_k_project_sample(const float* tokens, const float* T_cl, const float* camera, const float* ref,
                          const float* scale6_host, int32_t B, int32_t V, int32_t hh, int32_t ww, int32_t C, int32_t Q,
                          float* tgt, float* coord_pos, parq_stream stream) {
    if (!tokens || !T_cl || !camera || !ref || !scale6_host || !tgt) return fail(PARQ_ERR_ARG, "NULL argument");
    if (B < 1 || V < 1 || hh < 2 || ww < 2 || Q < 1 || C % 4 != 0 || C > 1024) return fail(PARQ_ERR_ARG, "bad dims");
    ScaleBox sb;
    for (int i = 0; i < 3; ++i) { sb.lo[i] = scale6_host[2 * i]; sb.hi[i] = scale6_host[2 * i + 1]; }
    HIPCHK(launch_project_sample(tokens, T_cl, camera, ref, sb, B, V, hh, ww, C, Q, tgt, coord_pos, (hipStream_t)stream));
    return PARQ_OK;
}

size_t parq_k_project_sample_backward_scratch_bytes(int32_t B, int32_t V, int32_t Q) {
    if (B < 1 || V < 1 || Q < 1) return 0;
    return (size_t)B * Q * V * 8 * sizeof(float);
}

int parq_k_project_sample_backward(const void* tokens, int32_t token_type, const double* T_cl, const float* camera, const float* ref,
                                   const float* scale6_host, int32_t B, int32_t V, int32_t hh, int32_t ww, int32_t C, int32_t Q,
                                   const float* g_tgt, float* g_tokens, float* g_ref, void* det_scratch, size_t det_scratch_bytes,
                                   parq_stream stream) {
    if (!tokens || !T_cl || !camera || !ref || !scale6_host || !g_tgt) return fail(PARQ_ERR_ARG, "NULL argument");
    if (B < 1 || V < 1 || hh < 2 || ww < 2 || Q < 1 || C % 4 != 0 || C > 1024) return fail(PARQ_ERR_ARG, "bad dims");
    if (token_type != kTokF32 && token_type != kTokF16 && token_type != kTokBF16)
        return fail(PARQ_ERR_ARG, "token type must be 0 (fp32), 1 (fp16) or 2 (bf16), not %d", token_type);
    if ((det_scratch == nullptr) != (det_scratch_bytes == 0)) return fail(PARQ_ERR_ARG, "det_scratch and det_scratch_bytes: both or neither");
    if (det_scratch && (det_scratch_bytes < parq_k_project_sample_backward_scratch_bytes(B, V, Q) ||
                        (reinterpret_cast<uintptr_t>(det_scratch) & 3u)))
        return fail(PARQ_ERR_ARG, "det_scratch: B * Q * V * 8 floats, 4-byte aligned");
    ScaleBox sb;
    for (int i = 0; i < 3; ++i) { sb.lo[i] = scale6_host[2 * i]; sb.hi[i] = scale6_host[2 * i + 1]; }
    if (det_scratch) {                 // launch_sample_bwd takes the gather form while a DetScope is alive on this thread
        DetScope det(static_cast<float*>(det_scratch), (int64_t)(det_scratch_bytes / sizeof(float)));
        HIPCHK(launch_sample_bwd(tokens, T_cl, camera, ref, sb, B, V, hh, ww, C, Q, g_tgt, g_tokens, g_ref, (hipStream_t)stream, token_type));
        return PARQ_OK;
    }
    HIPCHK(launch_sample_bwd(tokens, T_cl, camera, ref, sb, B, V, hh, ww, C, Q, g_tgt, g_tokens, g_ref, (hipStream_t)stream, token_type));
    return PARQ_OK;
}

// ------------------------------------------------------------------ the attention backward, one launcher call at a time
// Float offsets of the parts of the one scratch both entries carve (each part a multiple of 64 floats); n_it = 0: the single call.
namespace {
struct AttnBwdCarve { int64_t D, absmax, kvmax, part, pack, mat, flag, cache, total; };
AttnBwdCarve attn_bwd_carve(int B, int H, int Lq, int Lk, int dh, int n_it, int cache_terms) {
    AttnBwdCarve c;
    int64_t off = 0;
    auto take = [&](int64_t n) { const int64_t o = off; off += (n + 63) / 64 * 64; return o; };
    const int nt = n_it > 0 ? n_it : 1;
    c.D = take((int64_t)nt * B * H * flash_lq_pad(Lq));
    c.absmax = take(2);                                   // bits of max |dO|, the derived scale
    c.kvmax = take(n_it > 0 ? 2 : 0);
    c.part = take((int64_t)nt * (int64_t)attn_bwd_dq_partial_floats(B, H, Lq, Lk, dh, n_it > 0));
    c.pack = take(n_it > 0 && dh == 64 ? (int64_t)attn_bwd_pack_floats(B, H, Lq, n_it) : 0);
    if (n_it > 0) c.mat = take(dh == 256 ? (int64_t)attn_bwd_batched256_scratch_floats(n_it, Lq, Lk) : 0);
    else c.mat = take(dh != 64 && dh != 32 ? (int64_t)attn_bwd_mat_scratch_floats(Lq, Lk, dh) : 0);
    c.flag = take(cache_terms ? 64 : 0);                  // overflow flag of the cache conversion
    c.cache = take(cache_terms ? (int64_t)(kvsplit_cache_bytes(B, H, Lk, cache_terms == 1 ? 1 : 3) / sizeof(float)) : 0);
    c.total = off;
    return c;
}
bool attn_bwd_dims_ok(int B, int H, int Lq, int Lk, int dh) {
    return B >= 1 && H >= 1 && Lq >= 1 && Lk >= 1 && (dh == 32 || dh == 64 || dh == 128 || dh == 256) &&
           (int64_t)B * H * Lq * (int64_t)Lk < ((int64_t)1 << 40) && (int64_t)B * H * flash_lq_pad(Lq) < INT32_MAX;
}
// keep-masks [B*H*Lq][Lk] of stream `seed`: a dropout of ones (1 / (1 - p) where kept, 0 where dropped), row index bh * Lq + i
hipError_t attn_bwd_hook_masks(float* out, int B, int H, int Lq, int Lk, float p, uint32_t seed, hipStream_t s) {
    hipError_t e = launch_fill(out, 1.f, (int64_t)B * H * Lq * Lk, s);
    if (e != hipSuccess) return e;
    return launch_dropout_apply(out, out, B * H * Lq, Lk, p, seed, s);
}
}  // namespace

size_t parq_k_attention_backward_scratch_bytes(int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t dh, int32_t n_it, int32_t cache_terms) {
    if (!attn_bwd_dims_ok(B, H, Lq, Lk, dh) || n_it < 0 || n_it > 16) return 0;
    if (!(cache_terms == 0 || cache_terms == 1 || cache_terms == 3 || cache_terms == 8) || (cache_terms && (n_it == 0 || dh != 64))) return 0;
    return (size_t)attn_bwd_carve(B, H, Lq, Lk, dh, n_it, cache_terms).total * sizeof(float);
}

int parq_k_attention_backward(const float* q, const float* k, const float* v, const float* dO, const float* O, const float* lse,
                              int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t dh, int32_t layout, int32_t accumulate_kv,
                              int32_t use_absmax, float drop_p, uint32_t seed, float* gq, float* gk, float* gv, void* scratch,
                              size_t scratch_bytes, void* det_scratch, size_t det_scratch_bytes, float* D_out, float* masks_out,
                              int32_t* plan, parq_stream stream) {
    if (!attn_bwd_dims_ok(B, H, Lq, Lk, dh)) return fail(PARQ_ERR_ARG, "bad dims (head dim 32 / 64 / 128 / 256)");
    if (layout != PARQ_ATTN_BWD_LAYOUT_SELF && layout != PARQ_ATTN_BWD_LAYOUT_CROSS) return fail(PARQ_ERR_ARG, "layout must be 0 (packed q | k | v) or 1 (cross-attention), not %d", layout);
    if ((accumulate_kv != 0 && accumulate_kv != 1) || (use_absmax != 0 && use_absmax != 1)) return fail(PARQ_ERR_ARG, "accumulate_kv and use_absmax must be 0 or 1");
    if (!(drop_p >= 0.f && drop_p < 1.f)) return fail(PARQ_ERR_ARG, "drop_p must be in [0, 1)");
    if ((det_scratch == nullptr) != (det_scratch_bytes == 0)) return fail(PARQ_ERR_ARG, "det_scratch and det_scratch_bytes: both or neither");
    if (det_scratch && dh != 64) return fail(PARQ_ERR_ARG, "the deterministic form exists at head dim 64 only");
    if (det_scratch && (det_scratch_bytes < (size_t)det_attn_dq_floats(B, H, Lq, Lk) * sizeof(float) || (reinterpret_cast<uintptr_t>(det_scratch) & 15u)))
        return fail(PARQ_ERR_ARG, "det_scratch: B * H * ceil(Lk / 64) * pad32(Lq) * 64 floats, 16-byte aligned");
    const int Lq_pad = flash_lq_pad(Lq);
    const AttnBwdCarve cv = attn_bwd_carve(B, H, Lq, Lk, dh, 0, 0);
    // the kernel family: the order of the tests in launch_attn_bwd (attn_bwd.hip); the slot count from the size functions it uses
    if (plan) {
        const bool long_keys = Lk >= 2048;
        int fam = PARQ_ATTN_BWD_VALU32;
        if (dh != 64 && dh != 32) fam = PARQ_ATTN_BWD_MATERIALISED;
        else if (dh == 64 && long_keys && use_absmax) fam = PARQ_ATTN_BWD_SPLIT;
        else if (dh == 64) fam = long_keys ? PARQ_ATTN_BWD_MFMA8 : PARQ_ATTN_BWD_MFMA2;
        const int64_t slot = (int64_t)B * H * Lq_pad * 64;
        int64_t slots = (int64_t)attn_bwd_dq_partial_floats(B, H, Lq, Lk, dh, false) / slot;
        if (fam == PARQ_ATTN_BWD_MFMA2) slots = det_scratch ? det_attn_dq_floats(B, H, Lq, Lk) / slot : 0;
        plan[0] = fam; plan[1] = 1; plan[2] = (int32_t)slots; plan[3] = 0;
        if (!q) return PARQ_OK;                            // the plan alone: no device is touched
    }
    if (!q || !k || !v || !dO || !O || !lse || !gq || !gk || !gv || !scratch) return fail(PARQ_ERR_ARG, "NULL argument");
    if (masks_out && !(drop_p > 0.f)) return fail(PARQ_ERR_ARG, "masks_out needs drop_p > 0");
    if (scratch_bytes < (size_t)cv.total * sizeof(float) || (reinterpret_cast<uintptr_t>(scratch) & 15u))
        return fail(PARQ_ERR_WORKSPACE, "scratch: parq_k_attention_backward_scratch_bytes(), 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    float* sp = static_cast<float*>(scratch);
    const int64_t C = (int64_t)H * dh;
    float* D = sp + cv.D;
    HIPCHK(launch_attn_bwd_rowdot(dO, O, (int64_t)Lq * C, C, B, H, Lq, dh, D, s));
    // self-attention: every operand a column block of a packed [B][rows][3C] buffer; cross-attention: q token-major, K / V head-major,
    // gK | gV the two halves of a token-major [B][Lk][2C] buffer (the strides of do_backward_iter's two calls)
    const bool self = layout == PARQ_ATTN_BWD_LAYOUT_SELF;
    const int64_t qb = self ? (int64_t)Lq * 3 * C : (int64_t)Lq * C, qr = self ? 3 * C : C;
    const int64_t kb = self ? (int64_t)Lk * 3 * C : (int64_t)H * Lk * dh, kh = self ? dh : (int64_t)Lk * dh, kr = self ? 3 * C : dh;
    const int64_t gb = self ? (int64_t)Lk * 3 * C : (int64_t)Lk * 2 * C, gr = self ? 3 * C : 2 * C;
    float* part = attn_bwd_dq_partial_floats(B, H, Lq, Lk, dh) ? sp + cv.part : nullptr;
    unsigned int* absmax = use_absmax ? reinterpret_cast<unsigned int*>(sp + cv.absmax) : nullptr;
    float* mat = (dh == 64 || dh == 32) ? nullptr : sp + cv.mat;
    auto run = [&]() {
        return launch_attn_bwd(q, qb, dh, qr, k, kb, kh, kr, v, kb, kh, kr, dO, (int64_t)Lq * C, dh, C, lse, D, gq, qb, dh, qr, gk, gb, dh, gr,
                               gv, gb, dh, gr, B, H, Lq, Lk, dh, accumulate_kv, s, part, drop_p, seed, absmax, mat);
    };
    if (det_scratch) {                 // launch_attn_bwd takes its fixed-order forms while a DetScope is alive on this thread
        DetScope det(static_cast<float*>(det_scratch), (int64_t)(det_scratch_bytes / sizeof(float)));
        HIPCHK(run());
    } else {
        HIPCHK(run());
    }
    if (D_out) HIPCHK(hipMemcpyAsync(D_out, D, (size_t)B * H * Lq_pad * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (masks_out) HIPCHK(attn_bwd_hook_masks(masks_out, B, H, Lq, Lk, drop_p, seed, s));
    return PARQ_OK;
}

int parq_k_attention_backward_batched(const float* q, const float* k, const float* v, const float* dO, const float* O, const float* lse,
                                      int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t dh, int32_t n_it, int32_t cache_terms,
                                      int32_t cache_kind, float drop_p, const uint32_t* seeds, float* gq, float* gkv, void* scratch,
                                      size_t scratch_bytes, float* D_out, float* masks_out, int32_t* plan, parq_stream stream) {
    if (!attn_bwd_dims_ok(B, H, Lq, Lk, dh)) return fail(PARQ_ERR_ARG, "bad dims");
    if (n_it < 1 || n_it > 16) return fail(PARQ_ERR_ARG, "1 <= n_it <= 16");
    if (!(dh == 256 || (dh == 64 && Lk >= 2048))) return fail(PARQ_ERR_ARG, "the batched backward serves head dim 64 with Lk >= 2048, and head dim 256");
    if (!(cache_terms == 0 || cache_terms == 1 || cache_terms == 3 || cache_terms == 8)) return fail(PARQ_ERR_ARG, "cache_terms must be 0, 1, 3 or 8");
    if (cache_terms && dh != 64) return fail(PARQ_ERR_ARG, "the backward reads the 16-bit cache at head dim 64 only");
    if (cache_terms == 8 && !flash_split8_supported(64, Lk)) return fail(PARQ_ERR_ARG, "cache_terms 8 needs a key count that is a multiple of 64");
    if (cache_kind != kF16 && cache_kind != kBF16) return fail(PARQ_ERR_ARG, "cache_kind must be 0 (fp16) or 1 (bf16)");
    if (cache_kind == kBF16 && cache_terms != 1) return fail(PARQ_ERR_ARG, "bf16 is a single-product cache (cache_terms 1)");
    if (!(drop_p >= 0.f && drop_p < 1.f)) return fail(PARQ_ERR_ARG, "drop_p must be in [0, 1)");
    if (drop_p > 0.f && !seeds) return fail(PARQ_ERR_ARG, "drop_p > 0 needs seeds[n_it]");
    const int Lq_pad = flash_lq_pad(Lq);
    const AttnBwdCarve cv = attn_bwd_carve(B, H, Lq, Lk, dh, n_it, cache_terms);
    if (plan) {
        const int64_t slot = (int64_t)B * H * Lq_pad * 64;
        plan[0] = dh == 256 ? PARQ_ATTN_BWD_BATCHED256 : PARQ_ATTN_BWD_SPLIT2;
        plan[1] = dh == 256 ? 1 : attn_bwd_kb_group(B, H, Lk);
        plan[2] = (int32_t)((int64_t)attn_bwd_dq_partial_floats(B, H, Lq, Lk, dh, true) / slot);
        // QP out of the scratch size: attn_bwd_batched256_scratch_floats = QP (2 Lk + 1281) + 1040
        plan[3] = dh == 256 ? (int32_t)(((int64_t)attn_bwd_batched256_scratch_floats(n_it, Lq, Lk) - 1040) / (2 * (int64_t)Lk + 1281)) : 0;
        if (!q) return PARQ_OK;                            // the plan alone: no device is touched
    }
    if (!q || !k || !v || !dO || !O || !lse || !gq || !gkv || !scratch) return fail(PARQ_ERR_ARG, "NULL argument");
    if (masks_out && !(drop_p > 0.f)) return fail(PARQ_ERR_ARG, "masks_out needs drop_p > 0");
    if (scratch_bytes < (size_t)cv.total * sizeof(float) || (reinterpret_cast<uintptr_t>(scratch) & 15u))
        return fail(PARQ_ERR_WORKSPACE, "scratch: parq_k_attention_backward_scratch_bytes(), 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    float* sp = static_cast<float*>(scratch);
    const int64_t C = (int64_t)H * dh, MC = (int64_t)B * Lq * C, D_it = (int64_t)B * H * Lq_pad;
    float* D = sp + cv.D;
    int64_t q_off[16], lse_off[16];
    for (int t = 0; t < n_it; ++t) {
        q_off[t] = t * MC;
        lse_off[t] = t * D_it;
        HIPCHK(launch_attn_bwd_rowdot(dO + t * MC, O + t * MC, (int64_t)Lq * C, C, B, H, Lq, dh, D + t * D_it, s));
    }
    const void* cache = nullptr;
    if (cache_terms) {                 // the cache as the forward's projection leaves it, built from the fp32 K / V
        char* cb = reinterpret_cast<char*>(sp + cv.cache);
        const int64_t kb = (int64_t)H * Lk * dh, kh = (int64_t)Lk * dh;
        if (cache_terms == 8) {
            HIPCHK(launch_kvsplit8_convert(k, v, kb, kh, dh, kb, kh, dh, B, H, Lk, cb, s));
        } else {
            int* flag = reinterpret_cast<int*>(sp + cv.flag);
            HIPCHK(hipMemsetAsync(flag, 0, 256, s));
            HIPCHK(launch_kvsplit_convert(k, v, kb, kh, dh, kb, kh, dh, B, H, Lk, cb, flag, s, cache_terms, cache_kind));
        }
        cache = cb;
    }
    HIPCHK(launch_attn_bwd_batched(q, q_off, (int64_t)Lq * C, dh, C, k, (int64_t)H * Lk * dh, (int64_t)Lk * dh, dh, v, (int64_t)H * Lk * dh,
                                   (int64_t)Lk * dh, dh, dO, MC, (int64_t)Lq * C, dh, C, lse, lse_off, D, D_it, gq, MC, (int64_t)Lq * C, dh, C,
                                   gkv, (int64_t)Lk * 2 * C, dh, 2 * C, gkv + C, (int64_t)Lk * 2 * C, dh, 2 * C, B, H, Lq, Lk, dh, n_it, s,
                                   dh == 64 ? sp + cv.part : nullptr, drop_p, seeds, reinterpret_cast<unsigned int*>(sp + cv.absmax),
                                   reinterpret_cast<unsigned int*>(sp + cv.kvmax), dh == 64 ? sp + cv.pack : nullptr,
                                   dh == 256 ? sp + cv.mat : nullptr, cache, cache_terms, cache_kind));
    if (D_out) HIPCHK(hipMemcpyAsync(D_out, D, (size_t)n_it * D_it * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (masks_out)
        for (int t = 0; t < n_it; ++t) HIPCHK(attn_bwd_hook_masks(masks_out + (int64_t)t * B * H * Lq * Lk, B, H, Lq, Lk, drop_p, seeds[t], s));
    return PARQ_OK;
}

int parq_k_linear(const float* X, const float* X2, const float* W, const float* bias, const float* R, float* Y,
                  int32_t M, int32_t N, int32_t K, int32_t relu, parq_stream stream) {
    if (!X || !W || !Y || M < 1 || N < 1 || K < 32 || K % 32 != 0) return fail(PARQ_ERR_ARG, "bad argument (K must be a multiple of 32)");
    LinearArgs a = lin(X, K, W, K, bias, Y, N, M, N, K);
    a.X2 = X2; a.ldx2 = K; a.x2_ncols = N;
    a.R = R; a.ldr = N; a.relu = relu;
    HIPCHK(launch_linear(a, 1, (hipStream_t)stream));
    return PARQ_OK;
}

int parq_k_linear_half(const float* X, const float* X2, const float* W, const float* bias, const float* R, float* Y,
                       int32_t M, int32_t N, int32_t K, int32_t relu, void* scratch, size_t scratch_bytes, parq_stream stream) {
    if (!X || !W || !Y || !scratch || M < 16 || N < 16 || M % 16 != 0 || N % 16 != 0 || !(K == 1024 || K == 768))
        return fail(PARQ_ERR_ARG, "bad argument (K in {1024, 768}, M and N multiples of 16)");
    if (scratch_bytes < ((size_t)N * K + N) * sizeof(float) || (reinterpret_cast<uintptr_t>(scratch) & 15u))
        return fail(PARQ_ERR_ARG, "scratch: N * K * 4 + N * 4 bytes, 16-byte aligned");
    float* wh = static_cast<float*>(scratch);
    float* sc = wh + (size_t)N * K;
    HIPCHK(launch_pack_w_half(W, K, N, K, wh, sc, (hipStream_t)stream));
    LinearArgs a = lin(X, K, W, K, bias, Y, N, M, N, K);
    a.X2 = X2; a.ldx2 = K; a.x2_ncols = N;
    a.R = R; a.ldr = N; a.relu = relu;
    a.Wh = wh; a.wh_scale = sc;
    const hipError_t e = launch_chain_linear(a, 1, (hipStream_t)stream);
    if (e == hipErrorNotSupported) return fail(PARQ_ERR_ARG, "no fp16 x 3 tile for this combination of addend / bias / ReLU / residual");
    HIPCHK(e);
    return PARQ_OK;
}

size_t parq_k_attention_scratch_bytes(int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t dh) {
    const int ns = flash_pick_splits(B, H, Lq, Lk, dh, device_num_cus());
    return flash_scratch_bytes(B, H, Lq, dh, ns);
}

int parq_k_attention(const float* q, const float* k, const float* v, float* out, int32_t B, int32_t H, int32_t Lq,
                     int32_t Lk, int32_t dh, void* scratch, size_t scratch_bytes, parq_stream stream) {
    if (!q || !k || !v || !out || !scratch) return fail(PARQ_ERR_ARG, "NULL argument");
    if (!(dh == 32 || dh == 64 || dh == 128 || dh == 256) || B < 1 || H < 1 || Lq < 1 || Lk < 1) return fail(PARQ_ERR_ARG, "bad dims");
    FlashArgs fa;
    memset(&fa, 0, sizeof(fa));
    const int64_t C = (int64_t)H * dh;
    fa.B = B; fa.H = H; fa.Lq = Lq; fa.Lk = Lk; fa.dh = dh;
    fa.q = q; fa.q_batch = Lq * C; fa.q_head = dh; fa.q_row = C;
    fa.k = k; fa.k_batch = Lk * C; fa.k_head = dh; fa.k_row = C;
    fa.v = v; fa.v_batch = Lk * C; fa.v_head = dh; fa.v_row = C;
    fa.out = out; fa.out_batch = Lq * C; fa.out_row = C;
    fa.nsplit = flash_pick_splits(B, H, Lq, Lk, dh, device_num_cus());
    if (scratch_bytes < flash_scratch_bytes(B, H, Lq, dh, fa.nsplit)) return fail(PARQ_ERR_WORKSPACE, "attention scratch too small");
    const int64_t lp = flash_lq_pad(Lq);
    fa.o_part = (float*)scratch;
    fa.m_part = fa.o_part + (int64_t)B * H * fa.nsplit * dh * lp;
    fa.l_part = fa.m_part + (int64_t)B * H * fa.nsplit * lp;
    HIPCHK(launch_flash(fa, (hipStream_t)stream));
    HIPCHK(launch_flash_merge(fa, (hipStream_t)stream));
    return PARQ_OK;
}

size_t parq_k_attention_split_scratch_bytes(int32_t B, int32_t H, int32_t Lq, int32_t Lk) {
    const int ns = flash_split_pick_splits(B, H, Lq, Lk, device_num_cus());
    return flash_scratch_bytes(B, H, Lq, 64, ns) + kvsplit_cache_bytes(B, H, Lk) + 256;
}

int parq_k_attention_split(const float* q, const float* k, const float* v, float* out, int32_t B, int32_t H, int32_t Lq,
                           int32_t Lk, void* scratch, size_t scratch_bytes, parq_stream stream) {
    if (!q || !k || !v || !out || !scratch) return fail(PARQ_ERR_ARG, "NULL argument");
    if (B < 1 || H < 1 || Lq < 1 || Lk < 1) return fail(PARQ_ERR_ARG, "bad dims");
    if (scratch_bytes < parq_k_attention_split_scratch_bytes(B, H, Lq, Lk)) return fail(PARQ_ERR_WORKSPACE, "attention scratch too small");
    hipStream_t s = (hipStream_t)stream;
    const int dh = 64;
    const int64_t C = (int64_t)H * dh;
    FlashArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.B = B; fa.H = H; fa.Lq = Lq; fa.Lk = Lk; fa.dh = dh;
    fa.q = q; fa.q_batch = Lq * C; fa.q_head = dh; fa.q_row = C;
    fa.out = out; fa.out_batch = Lq * C; fa.out_row = C;
    fa.nsplit = flash_split_pick_splits(B, H, Lq, Lk, device_num_cus());
    const int64_t lp = flash_lq_pad(Lq);
    char* base = (char*)scratch;
    int* flag = (int*)base;
    char* cache = base + 256;
    fa.o_part = (float*)(cache + kvsplit_cache_bytes(B, H, Lk));
    fa.m_part = fa.o_part + (int64_t)B * H * fa.nsplit * dh * lp;
    fa.l_part = fa.m_part + (int64_t)B * H * fa.nsplit * lp;
    HIPCHK(hipMemsetAsync(flag, 0, 256, s));
    HIPCHK(launch_kvsplit_convert(k, v, Lk * C, dh, C, Lk * C, dh, C, B, H, Lk, cache, flag, s));
    HIPCHK(launch_flash_split(fa, cache, s));
    HIPCHK(launch_flash_merge(fa, s));
    return PARQ_OK;
}

/* mode 4: hi.hi on the fp16 matrix pipe, the cross terms as MX-scaled fp8 products (flash_split8.hip); Lk % 64 == 0 */
int parq_k_attention_split8(const float* q, const float* k, const float* v, float* out, int32_t B, int32_t H, int32_t Lq,
                            int32_t Lk, void* scratch, size_t scratch_bytes, parq_stream stream) {
    if (!q || !k || !v || !out || !scratch) return fail(PARQ_ERR_ARG, "NULL argument");
    if (B < 1 || H < 1 || Lq < 1 || Lk < 1) return fail(PARQ_ERR_ARG, "bad dims");
    if (!flash_split8_supported(64, Lk)) return fail(PARQ_ERR_ARG, "attention mode 4 needs a key count that is a multiple of 64");
    if (scratch_bytes < parq_k_attention_split_scratch_bytes(B, H, Lq, Lk)) return fail(PARQ_ERR_WORKSPACE, "attention scratch too small");
    hipStream_t s = (hipStream_t)stream;
    const int dh = 64;
    const int64_t C = (int64_t)H * dh;
    FlashArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.B = B; fa.H = H; fa.Lq = Lq; fa.Lk = Lk; fa.dh = dh;
    fa.q = q; fa.q_batch = Lq * C; fa.q_head = dh; fa.q_row = C;
    fa.out = out; fa.out_batch = Lq * C; fa.out_row = C;
    fa.nsplit = flash_split_pick_splits(B, H, Lq, Lk, device_num_cus());
    const int64_t lp = flash_lq_pad(Lq);
    char* cache = (char*)scratch + 256;
    fa.o_part = (float*)(cache + kvsplit_cache_bytes(B, H, Lk));
    fa.m_part = fa.o_part + (int64_t)B * H * fa.nsplit * dh * lp;
    fa.l_part = fa.m_part + (int64_t)B * H * fa.nsplit * lp;
    HIPCHK(launch_kvsplit8_convert(k, v, Lk * C, dh, C, Lk * C, dh, C, B, H, Lk, cache, s));
    HIPCHK(launch_flash_split8(fa, cache, s));
    HIPCHK(launch_flash_merge(fa, s));
    return PARQ_OK;
}

size_t parq_k_attention_split256_scratch_bytes(int32_t B, int32_t H, int32_t Lq, int32_t Lk) {
    const int ns = flash_split256_pick_splits(B, H, Lq, Lk, device_num_cus());
    return flash_scratch_bytes(B, H, Lq, 256, ns) + kvsplit_cache_bytes(B, 4 * H, Lk) + 256;
}

/* head dim 256: a head is stored as 4 virtual heads of 64 in the split cache (flash_split256.hip) */
int parq_k_attention_split256(const float* q, const float* k, const float* v, float* out, int32_t B, int32_t H, int32_t Lq,
                              int32_t Lk, void* scratch, size_t scratch_bytes, parq_stream stream) {
    if (!q || !k || !v || !out || !scratch) return fail(PARQ_ERR_ARG, "NULL argument");
    if (B < 1 || H < 1 || Lq < 1 || Lk < 1) return fail(PARQ_ERR_ARG, "bad dims");
    if (scratch_bytes < parq_k_attention_split256_scratch_bytes(B, H, Lq, Lk)) return fail(PARQ_ERR_WORKSPACE, "attention scratch too small");
    hipStream_t s = (hipStream_t)stream;
    const int dh = 256;
    const int64_t C = (int64_t)H * dh;
    FlashArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.B = B; fa.H = H; fa.Lq = Lq; fa.Lk = Lk; fa.dh = dh;
    fa.q = q; fa.q_batch = Lq * C; fa.q_head = dh; fa.q_row = C;
    fa.out = out; fa.out_batch = Lq * C; fa.out_row = C;
    fa.nsplit = flash_split256_pick_splits(B, H, Lq, Lk, device_num_cus());
    const int64_t lp = flash_lq_pad(Lq);
    char* base = (char*)scratch;
    int* flag = (int*)base;
    char* cache = base + 256;
    fa.o_part = (float*)(cache + kvsplit_cache_bytes(B, 4 * H, Lk));
    fa.m_part = fa.o_part + (int64_t)B * H * fa.nsplit * dh * lp;
    fa.l_part = fa.m_part + (int64_t)B * H * fa.nsplit * lp;
    HIPCHK(hipMemsetAsync(flag, 0, 256, s));
    HIPCHK(launch_kvsplit_convert(k, v, Lk * C, 64, C, Lk * C, 64, C, B, 4 * H, Lk, cache, flag, s));     // 4 H virtual heads of 64
    HIPCHK(launch_flash_split256(fa, cache, s));
    HIPCHK(launch_flash_merge(fa, s));
    return PARQ_OK;
}

size_t parq_k_attention_half_scratch_bytes(int32_t B, int32_t H, int32_t Lq, int32_t Lk) {
    return parq_k_attention_split_scratch_bytes(B, H, Lq, Lk);      // the single-term cache is half the split one
}

int parq_k_attention_half(const float* q, const float* k, const float* v, float* out, int32_t B, int32_t H, int32_t Lq,
                          int32_t Lk, int32_t bf16, void* scratch, size_t scratch_bytes, parq_stream stream) {
    if (!q || !k || !v || !out || !scratch) return fail(PARQ_ERR_ARG, "NULL argument");
    if (B < 1 || H < 1 || Lq < 1 || Lk < 1) return fail(PARQ_ERR_ARG, "bad dims");
    if (scratch_bytes < parq_k_attention_half_scratch_bytes(B, H, Lq, Lk)) return fail(PARQ_ERR_WORKSPACE, "attention scratch too small");
    hipStream_t s = (hipStream_t)stream;
    const int dh = 64, kind = bf16 ? kBF16 : kF16;
    const int64_t C = (int64_t)H * dh;
    FlashArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.B = B; fa.H = H; fa.Lq = Lq; fa.Lk = Lk; fa.dh = dh;
    fa.q = q; fa.q_batch = Lq * C; fa.q_head = dh; fa.q_row = C;
    fa.out = out; fa.out_batch = Lq * C; fa.out_row = C;
    fa.nsplit = flash_split_pick_splits(B, H, Lq, Lk, device_num_cus());
    const int64_t lp = flash_lq_pad(Lq);
    char* base = (char*)scratch;
    int* flag = (int*)base;
    char* cache = base + 256;
    fa.o_part = (float*)(cache + kvsplit_cache_bytes(B, H, Lk, 3));
    fa.m_part = fa.o_part + (int64_t)B * H * fa.nsplit * dh * lp;
    fa.l_part = fa.m_part + (int64_t)B * H * fa.nsplit * lp;
    HIPCHK(hipMemsetAsync(flag, 0, 256, s));
    HIPCHK(launch_kvsplit_convert(k, v, Lk * C, dh, C, Lk * C, dh, C, B, H, Lk, cache, flag, s, 1, kind));
    HIPCHK(launch_flash_split(fa, cache, s, 1, kind));
    HIPCHK(launch_flash_merge(fa, s));
    return PARQ_OK;
}

// ------------------------------------------------------------------ AddRayPE + tokenisation
static int64_t raype_align(int64_t x) { return (x + 63) / 64 * 64; }

// Workspace layout: [hidden [M][C] — only when the hidden layer is kept] | W1 hi/lo (C*K1 halfs each) | W2 hi/lo (C*C halfs each)
// | W2 in fragment order (one-pass path) | pose + depth tables (float64) | points [M][K1] (generic path only).
// The hidden layer is kept (first region: parq_ray_pe_backward reads it there) unless the caller passes PARQ_RAYPE_NO_HIDDEN on
// the one-pass path (C = 256, 64 samples), where it never leaves the CU; the generic path needs it as an intermediate.
static bool raype_keeps_hidden(int32_t C, int32_t num_samples, int32_t flags) {
    return !((flags & PARQ_RAYPE_NO_HIDDEN) && C == 256 && num_samples == 64);
}
size_t parq_ray_pe_workspace_bytes_flags(int32_t B, int32_t V, int32_t hh, int32_t ww, int32_t C, int32_t num_samples, int32_t flags) {
    if (B < 1 || V < 1 || hh < 1 || ww < 1 || C < 1 || num_samples < 1) return 0;
    const int64_t M = (int64_t)B * V * hh * ww, K1 = 3 * (int64_t)num_samples;
    const bool fused = (C == 256 && num_samples == 64);
    const int64_t floats = (raype_keeps_hidden(C, num_samples, flags) ? raype_align(M * C) : 0) + raype_align(C * K1) +
                           2 * raype_align((int64_t)C * C) + raype_align(2 * ((int64_t)B * V * 12 + num_samples)) +
                           (fused ? 0 : raype_align(M * K1));
    return (size_t)floats * sizeof(float);
}
size_t parq_ray_pe_workspace_bytes(int32_t B, int32_t V, int32_t hh, int32_t ww, int32_t C, int32_t num_samples) {
    return parq_ray_pe_workspace_bytes_flags(B, V, hh, ww, C, num_samples, 0);
}

// parq_ray_pe and parq_ray_pe_fpn: the feature maps come from features_nchw, or (fpn != nullptr) are gathered from a pyramid
static int ray_pe_impl(const float* camera, const float* T_cp, const float* T_wp, const float* T_wl, const float* w1,
                       const float* b1, const float* w2, const float* b2, const float* scale6_host, float min_depth,
                       float max_depth, int32_t num_samples, int32_t B, int32_t V, int32_t hh, int32_t ww, int32_t C,
                       const float* features_nchw, const FpnDev* fpn, float* tokens_out, int32_t flags, void* workspace,
                       size_t workspace_bytes, parq_stream stream) {
    const int32_t nchw_out = flags & PARQ_RAYPE_NCHW_OUT;
    // 16-bit token rows (inference: the hidden layer is not kept for a backward; channels-last)
    const int out16 = (flags & PARQ_RAYPE_OUT_F16) ? kTokF16 : (flags & PARQ_RAYPE_OUT_BF16) ? kTokBF16 : kTokF32;
    if ((flags & PARQ_RAYPE_OUT_F16) && (flags & PARQ_RAYPE_OUT_BF16)) return fail(PARQ_ERR_ARG, "ray-PE: one 16-bit output type at a time");
    if (out16 != kTokF32 && (nchw_out || !(flags & PARQ_RAYPE_NO_HIDDEN)))
        return fail(PARQ_ERR_ARG, "ray-PE: 16-bit tokens are an inference output (no-hidden flag, channels-last)");
    if (!camera || !T_cp || !T_wp || !T_wl || !w1 || !b1 || !w2 || !b2 || !scale6_host || !tokens_out || !workspace)
        return fail(PARQ_ERR_ARG, "NULL argument");
    if (B < 1 || V < 1 || hh < 1 || ww < 1 || num_samples < 1) return fail(PARQ_ERR_ARG, "bad dims");
    if ((3 * num_samples) % 64 != 0 || C % 64 != 0) return fail(PARQ_ERR_ARG, "3*num_samples and C must be multiples of 64");
    if (!(max_depth > min_depth && min_depth > 0.f)) return fail(PARQ_ERR_ARG, "need 0 < min_depth < max_depth");
    if (workspace_bytes < parq_ray_pe_workspace_bytes_flags(B, V, hh, ww, C, num_samples, flags)) return fail(PARQ_ERR_WORKSPACE, "ray-PE workspace too small");
    const int64_t M64 = (int64_t)B * V * hh * ww;
    if (M64 > INT32_MAX) return fail(PARQ_ERR_ARG, "too many tokens");
    const int M = (int)M64, K1 = 3 * num_samples;
    hipStream_t s = (hipStream_t)stream;
    float* wsp = (float*)workspace;
    const bool keep = raype_keeps_hidden(C, num_samples, flags);
    float* Hd = keep ? wsp : nullptr;
    float* W1s = wsp + (keep ? raype_align((int64_t)M * C) : 0);
    float* W2s = W1s + raype_align((int64_t)C * K1);
    float* W2f = W2s + raype_align((int64_t)C * C);
    double* tabs = reinterpret_cast<double*>(W2f + raype_align((int64_t)C * C));
    float* P = reinterpret_cast<float*>(tabs) + raype_align(2 * ((int64_t)B * V * 12 + num_samples));
    char* w1hi = (char*)W1s; char* w1lo = w1hi + (size_t)C * K1 * 2;
    char* w2hi = (char*)W2s; char* w2lo = w2hi + (size_t)C * C * 2;
    const bool cached = (flags & PARQ_RAYPE_WEIGHTS_CACHED) != 0;       // the workspace still holds this w1 / w2, split and packed
    if (!cached) {
        HIPCHK(launch_split_f32(w1, w1hi, w1lo, (int64_t)C * K1, s));
        HIPCHK(launch_split_f32(w2, w2hi, w2lo, (int64_t)C * C, s));
    }
    if (C == 256 && num_samples == 64) {
        // one pass (against the hidden tensor written and re-read by two kernels: profiles/r04_raype_onepass.txt)
        HIPCHK(launch_raype_fused(camera, T_cp, T_wp, T_wl, scale6_host, min_depth, max_depth, B, V, hh, ww, w1hi, w1lo, b1,
                                  w2hi, w2lo, b2, features_nchw, Hd, tabs, tabs + (int64_t)B * V * 12, tokens_out,
                                  nchw_out ? 1 : 0, s, W2f, cached ? 1 : 0, out16, fpn));
        return PARQ_OK;
    }
    if (nchw_out) return fail(PARQ_ERR_ARG, "NCHW output needs the fused path (C = 256, 64 samples)");
    HIPCHK(launch_raype_points(camera, T_cp, T_wp, T_wl, scale6_host, min_depth, max_depth, B, V, hh, ww, num_samples, P, s));
    HIPCHK(launch_gemm_split(P, K1, w1hi, w1lo, b1, Hd, C, M, C, K1, 1, nullptr, 1, s));
    HIPCHK(launch_gemm_split(Hd, C, w2hi, w2lo, b2, tokens_out, C, M, C, C, 0, features_nchw, hh * ww, s, nullptr, 1.f, nullptr, 0, out16,
                             fpn));
    return PARQ_OK;
}

int parq_ray_pe(const float* camera, const float* T_cp, const float* T_wp, const float* T_wl, const float* w1,
                const float* b1, const float* w2, const float* b2, const float* scale6_host, float min_depth,
                float max_depth, int32_t num_samples, int32_t B, int32_t V, int32_t hh, int32_t ww, int32_t C,
                const float* features_nchw, float* tokens_out, int32_t flags, void* workspace, size_t workspace_bytes,
                parq_stream stream) {
    return ray_pe_impl(camera, T_cp, T_wp, T_wl, w1, b1, w2, b2, scale6_host, min_depth, max_depth, num_samples, B, V, hh, ww, C,
                       features_nchw, nullptr, tokens_out, flags, workspace, workspace_bytes, stream);
}

// the pyramid's geometry against the tokens' (B*V images of hh x ww, C channels): PARQ_OK or PARQ_ERR_ARG with a message
static int fpn_check(const parq_fpn_levels* lv, int32_t hh, int32_t ww, int32_t C, FpnDev& f) {
    if (!lv) return fail(PARQ_ERR_ARG, "NULL pyramid");
    if (C < 4 || C % 4 != 0 || (C / 4) % 16 != 0)
        return fail(PARQ_ERR_ARG, "pyramid: C = %d must be 4 levels of a multiple of 16 channels", (int)C);
    if (lv->layer < 0 || lv->layer > 3) return fail(PARQ_ERR_ARG, "pyramid: layer %d outside 0..3", (int)lv->layer);
    for (int l = 0; l < 4; ++l) {
        if (!lv->level[l]) return fail(PARQ_ERR_ARG, "pyramid: level %d is NULL", l);
        if (lv->h[l] < 1 || lv->w[l] < 1) return fail(PARQ_ERR_ARG, "pyramid: level %d is %d x %d", l, (int)lv->h[l], (int)lv->w[l]);
        if ((int64_t)lv->h[l] * lv->w[l] * (C / 4) > INT32_MAX / 4) return fail(PARQ_ERR_ARG, "pyramid: level %d too large", l);
        f.lv[l] = lv->level[l];
        f.h[l] = lv->h[l];
        f.w[l] = lv->w[l];
    }
    if (lv->h[lv->layer] != hh || lv->w[lv->layer] != ww)
        return fail(PARQ_ERR_ARG, "pyramid: target level %d is %d x %d but the tokens are %d x %d per view", (int)lv->layer,
                    (int)lv->h[lv->layer], (int)lv->w[lv->layer], (int)hh, (int)ww);
    f.layer = lv->layer;
    f.cl = C / 4;
    return PARQ_OK;
}

int parq_ray_pe_fpn(const float* camera, const float* T_cp, const float* T_wp, const float* T_wl, const float* w1,
                    const float* b1, const float* w2, const float* b2, const float* scale6_host, float min_depth,
                    float max_depth, int32_t num_samples, int32_t B, int32_t V, int32_t hh, int32_t ww, int32_t C,
                    const parq_fpn_levels* levels, float* tokens_out, int32_t flags, void* workspace, size_t workspace_bytes,
                    parq_stream stream) {
    if (flags & PARQ_RAYPE_NCHW_OUT) return fail(PARQ_ERR_ARG, "pyramid: channels-last tokens only (no NCHW output)");
    FpnDev f;
    if (int rc = fpn_check(levels, hh, ww, C, f); rc != PARQ_OK) return rc;
    return ray_pe_impl(camera, T_cp, T_wp, T_wl, w1, b1, w2, b2, scale6_host, min_depth, max_depth, num_samples, B, V, hh, ww, C,
                       nullptr, &f, tokens_out, flags, workspace, workspace_bytes, stream);
}

int parq_fpn_backward(const float* d_tokens, int32_t B, int32_t V, int32_t C, const parq_fpn_levels* levels, float* const d_level[4],
                      parq_stream stream) {
    if (!d_tokens || !d_level || !d_level[0] || !d_level[1] || !d_level[2] || !d_level[3]) return fail(PARQ_ERR_ARG, "NULL argument");
    if (B < 1 || V < 1) return fail(PARQ_ERR_ARG, "bad dims");
    if (!levels) return fail(PARQ_ERR_ARG, "NULL pyramid");
    const int l = levels->layer;
    if (l < 0 || l > 3) return fail(PARQ_ERR_ARG, "pyramid: layer %d outside 0..3", l);
    FpnDev f;
    if (int rc = fpn_check(levels, levels->h[l], levels->w[l], C, f); rc != PARQ_OK) return rc;
    if ((int64_t)B * V * levels->h[l] * levels->w[l] * C > INT32_MAX) return fail(PARQ_ERR_ARG, "too many tokens");
    HIPCHK(launch_fpn_backward(d_tokens, B * V, f, d_level, (hipStream_t)stream));
    return PARQ_OK;
}

size_t parq_ray_pe_backward_workspace_bytes_flags(int32_t B, int32_t V, int32_t hh, int32_t ww, int32_t C, int32_t num_samples,
                                                  int32_t flags) {
    if (B < 1 || V < 1 || hh < 1 || ww < 1 || C < 1 || num_samples < 1 || (flags & ~PARQ_RAYPE_BWD_DETERMINISTIC)) return 0;
    const int64_t M = (int64_t)B * V * hh * ww, K1 = 3 * (int64_t)num_samples;
    // points [M][K1] | d hidden [M][C] | W2^T [C][C] | deterministic mode: the row-split slabs
    const int64_t det = (flags & PARQ_RAYPE_BWD_DETERMINISTIC) ? raype_align(det_scratch_floats(0, 0)) : 0;
    return (size_t)(raype_align(M * K1) + raype_align(M * C) + raype_align((int64_t)C * C) + det) * sizeof(float);
}
size_t parq_ray_pe_backward_workspace_bytes(int32_t B, int32_t V, int32_t hh, int32_t ww, int32_t C, int32_t num_samples) {
    return parq_ray_pe_backward_workspace_bytes_flags(B, V, hh, ww, C, num_samples, 0);
}

int parq_ray_pe_backward(const float* camera, const float* T_cp, const float* T_wp, const float* T_wl, const float* w2,
                         const float* scale6_host, float min_depth, float max_depth, int32_t num_samples, int32_t B, int32_t V,
                         int32_t hh, int32_t ww, int32_t C, const float* d_tokens, const void* fwd_workspace, void* bwd_workspace,
                         size_t bwd_workspace_bytes, float* dw1, float* db1, float* dw2, float* db2, float* d_features_nchw,
                         parq_stream stream) {
    return parq_ray_pe_backward_flags(camera, T_cp, T_wp, T_wl, w2, scale6_host, min_depth, max_depth, num_samples, B, V, hh, ww, C,
                                      d_tokens, fwd_workspace, bwd_workspace, bwd_workspace_bytes, dw1, db1, dw2, db2, d_features_nchw, 0,
                                      stream);
}

int parq_ray_pe_backward_flags(const float* camera, const float* T_cp, const float* T_wp, const float* T_wl, const float* w2,
                               const float* scale6_host, float min_depth, float max_depth, int32_t num_samples, int32_t B, int32_t V,
                               int32_t hh, int32_t ww, int32_t C, const float* d_tokens, const void* fwd_workspace, void* bwd_workspace,
                               size_t bwd_workspace_bytes, float* dw1, float* db1, float* dw2, float* db2, float* d_features_nchw,
                               int32_t flags, parq_stream stream) {
    if (flags & ~PARQ_RAYPE_BWD_DETERMINISTIC) return fail(PARQ_ERR_ARG, "unknown ray-PE backward flags 0x%x", (unsigned)flags);
    if (!camera || !T_cp || !T_wp || !T_wl || !w2 || !scale6_host || !d_tokens || !fwd_workspace || !bwd_workspace || !dw1 || !db1 ||
        !dw2 || !db2)
        return fail(PARQ_ERR_ARG, "NULL argument");
    if (B < 1 || V < 1 || hh < 1 || ww < 1 || num_samples < 1 || (3 * num_samples) % 64 != 0 || C % 64 != 0) return fail(PARQ_ERR_ARG, "bad dims");
    if (bwd_workspace_bytes < parq_ray_pe_backward_workspace_bytes_flags(B, V, hh, ww, C, num_samples, flags))
        return fail(PARQ_ERR_WORKSPACE, "ray-PE backward workspace too small");
    const int64_t M64 = (int64_t)B * V * hh * ww;
    if (M64 > INT32_MAX) return fail(PARQ_ERR_ARG, "too many tokens");
    const int M = (int)M64, K1 = 3 * num_samples;
    hipStream_t s = (hipStream_t)stream;
    const float* Hd = (const float*)fwd_workspace;                  // hidden activations of the forward (first region)
    float* P = (float*)bwd_workspace;
    float* gHd = P + raype_align((int64_t)M * K1);
    float* W2T = gHd + raype_align((int64_t)M * C);
    // PARQ_RAYPE_BWD_DETERMINISTIC: the column sums and weight products below take their fixed-order forms (common.hpp DetScratch)
    const bool det_on = (flags & PARQ_RAYPE_BWD_DETERMINISTIC) != 0;
    DetScope det(det_on ? W2T + raype_align((int64_t)C * C) : nullptr, det_on ? det_scratch_floats(0, 0) : 0);
    // tokens = features + relu(p W1^T + b1) W2^T + b2   (ray_positional_encoding.py:128-136, parq_lightning.py:75)
    HIPCHK(hipMemsetAsync(db2, 0, (size_t)C * sizeof(float), s));
    HIPCHK(hipMemsetAsync(db1, 0, (size_t)C * sizeof(float), s));
    HIPCHK(launch_colsum(d_tokens, C, M, C, db2, 1, s));
    HIPCHK(hipMemsetAsync(dw2, 0, (size_t)C * C * sizeof(float), s));
    HIPCHK(launch_gemm_tn(d_tokens, C, Hd, C, dw2, C, M, C, C, 1, s));
    HIPCHK(launch_transpose(w2, C, W2T, C, C, C, s));
    {
        LinearArgs a = lin(d_tokens, C, W2T, C, nullptr, gHd, C, M, C, C);
        a.relu_mask = Hd; a.ldmask = C;
        HIPCHK(launch_linear(a, 1, s));
    }
    HIPCHK(launch_colsum(gHd, C, M, C, db1, 1, s));
    HIPCHK(launch_raype_points(camera, T_cp, T_wp, T_wl, scale6_host, min_depth, max_depth, B, V, hh, ww, num_samples, P, s));
    HIPCHK(hipMemsetAsync(dw1, 0, (size_t)C * K1 * sizeof(float), s));
    HIPCHK(launch_gemm_tn(gHd, C, P, K1, dw1, K1, M, C, K1, 1, s));
    if (d_features_nchw) {
        const int hw = hh * ww;
        for (int i = 0; i < B * V; ++i)                                 // (hw, C) -> (C, hw) per image
            HIPCHK(launch_transpose(d_tokens + (int64_t)i * hw * C, C, d_features_nchw + (int64_t)i * C * hw, hw, hw, C, s));
    }
    return PARQ_OK;
}

int parq_parse_pred(const float* center, const float* size, const float* ortho6d, const float* sem_cls_prob, int32_t B, int32_t Q,
                    int32_t num_classes, const float* track_scale6_host, int32_t for_vis, int32_t enable_nms, float* obbs_out,
                    unsigned char* mask_out, parq_stream stream) {
    if (!center || !size || !ortho6d || !sem_cls_prob || !track_scale6_host || !obbs_out || !mask_out) return fail(PARQ_ERR_ARG, "NULL argument");
    if (B < 1 || Q < 1 || Q > 1024 || num_classes < 2) return fail(PARQ_ERR_ARG, "bad dims (1 <= Q <= 1024)");
    HIPCHK(launch_parse_pred(center, size, ortho6d, sem_cls_prob, B, Q, num_classes, num_classes - 1, track_scale6_host, for_vis,
                             enable_nms, obbs_out, mask_out, (hipStream_t)stream));
    return PARQ_OK;
}

int parq_obb_iou(const double* boxes_a, int64_t n_a_total, const double* boxes_b, int64_t n_b_total, const int64_t* segments, int32_t S,
                 int64_t total_pairs, double* iou3d_out, double* iou2d_out, parq_stream stream) {
    if (S < 0 || total_pairs < 0 || n_a_total < 0 || n_b_total < 0) return fail(PARQ_ERR_ARG, "parq_obb_iou: negative count");
    if (S == 0 || total_pairs == 0) return PARQ_OK;                     // nothing to compute: no launch
    if (!boxes_a || !boxes_b || !segments || !iou3d_out) return fail(PARQ_ERR_ARG, "parq_obb_iou: NULL argument");
    if (n_a_total < 1 || n_b_total < 1) return fail(PARQ_ERR_ARG, "parq_obb_iou: %lld pairs of no boxes", (long long)total_pairs);
    if ((total_pairs + 63) / 64 > (int64_t)INT32_MAX) return fail(PARQ_ERR_ARG, "parq_obb_iou: too many pairs");
    HIPCHK(launch_obb_iou(boxes_a, boxes_b, segments, S, total_pairs, n_a_total, n_b_total, iou3d_out, iou2d_out, (hipStream_t)stream));
    return PARQ_OK;
}

size_t parq_assign_max_workspace_bytes(int32_t S, int32_t max_rows, int32_t max_cols) {
    if (S < 0 || max_rows < 0 || max_cols < 0 || max_rows > 2048 || max_cols > 2048) return 0;
    return ((size_t)S * ((size_t)max_rows + (size_t)max_cols) * 8 + 15) & ~(size_t)15;
}

int parq_assign_max(const float* m, int64_t m_total, const int64_t* segments, int32_t S, int32_t max_rows, int32_t max_cols,
                    void* workspace, size_t workspace_bytes, int32_t* row_to_col, int64_t out_total, parq_stream stream) {
    if (S < 0 || m_total < 0 || out_total < 0 || max_rows < 0 || max_cols < 0) return fail(PARQ_ERR_ARG, "parq_assign_max: negative count");
    if (max_rows > 2048 || max_cols > 2048) return fail(PARQ_ERR_ARG, "parq_assign_max: max_rows = %d, max_cols = %d; at most 2048 each", max_rows, max_cols);
    if (S == 0) return PARQ_OK;                                         // nothing to solve: no launch
    if (!segments || (m_total > 0 && !m) || (out_total > 0 && !row_to_col)) return fail(PARQ_ERR_ARG, "parq_assign_max: NULL argument");
    const size_t need = parq_assign_max_workspace_bytes(S, max_rows, max_cols);
    if (need > 0 && !workspace) return fail(PARQ_ERR_ARG, "parq_assign_max: NULL workspace");
    if (workspace_bytes < need) return fail(PARQ_ERR_ARG, "parq_assign_max: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    if ((uintptr_t)workspace & 15) return fail(PARQ_ERR_ARG, "parq_assign_max: the workspace must be 16-byte aligned");
    HIPCHK(launch_assign_max(m, m_total, segments, S, max_rows, max_cols, static_cast<double*>(workspace), row_to_col, out_total,
                             (hipStream_t)stream));
    return PARQ_OK;
}

size_t parq_tracks_store_bytes(int32_t S_cap, int32_t max_tracks) {
    if (S_cap < 0 || max_tracks < 1 || max_tracks > 2048) return 0;
    return (size_t)S_cap * (2 + 26 * (size_t)max_tracks) * 4;
}

size_t parq_tracks_update_workspace_bytes(int32_t B, int32_t Q, int32_t max_tracks) {
    if (B < 0 || Q < 1 || Q > 2048 || max_tracks < 1 || max_tracks > 2048) return 0;
    return tracks_update_workspace_bytes(B, Q, max_tracks);
}

int parq_tracks_update(void* store, int32_t S_cap, int32_t max_tracks, const int32_t* slots_host, int32_t B, const float* corners_world,
                       const float* sem_cls_prob, const unsigned char* pred_mask, int32_t Q, int32_t K, float conf_thresh,
                       float iou_thresh, void* workspace, size_t workspace_bytes, int32_t* track_id, float* iou_out, parq_stream stream) {
    if (B < 0 || S_cap < 0) return fail(PARQ_ERR_ARG, "parq_tracks_update: negative count");
    if (Q < 1 || Q > 2048 || max_tracks < 1 || max_tracks > 2048 || K < 2)
        return fail(PARQ_ERR_ARG, "parq_tracks_update: Q = %d, max_tracks = %d, K = %d; 1 <= Q, max_tracks <= 2048 and K >= 2", Q, max_tracks, K);
    if (B == 0) return PARQ_OK;                                         // no scene: no launch
    if (!store || !slots_host || !corners_world || !sem_cls_prob || !pred_mask || !workspace || !track_id)
        return fail(PARQ_ERR_ARG, "parq_tracks_update: NULL argument");
    {
        std::vector<char> seen((size_t)S_cap, 0);
        for (int b = 0; b < B; ++b) {
            const int32_t sl = slots_host[b];
            if (sl < 0 || sl >= S_cap) return fail(PARQ_ERR_ARG, "parq_tracks_update: slot %d of scene %d outside [0, %d)", sl, b, S_cap);
            if (seen[(size_t)sl]) return fail(PARQ_ERR_ARG, "parq_tracks_update: slot %d listed twice in one call", sl);
            seen[(size_t)sl] = 1;
        }
    }
    const size_t need = parq_tracks_update_workspace_bytes(B, Q, max_tracks);
    if (workspace_bytes < need) return fail(PARQ_ERR_ARG, "parq_tracks_update: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    if ((uintptr_t)workspace & 15) return fail(PARQ_ERR_ARG, "parq_tracks_update: the workspace must be 16-byte aligned");
    for (int b0 = 0; b0 < B; b0 += kTrackChunk)
        HIPCHK(launch_tracks_update(static_cast<int32_t*>(store), max_tracks, slots_host, b0, std::min(B - b0, (int)kTrackChunk), corners_world,
                                    sem_cls_prob, pred_mask, Q, K, conf_thresh, iou_thresh, workspace, track_id, iou_out,
                                    (hipStream_t)stream));
    return PARQ_OK;
}

size_t parq_gt_tracks_update_workspace_bytes(int32_t B, int32_t P, int32_t max_tracks) {
    if (B < 0 || P < 1 || P > 2048 || max_tracks < 1 || max_tracks > 2048) return 0;
    return gt_tracks_update_workspace_bytes(B, P, max_tracks);
}

int parq_gt_tracks_update(void* store, int32_t S_cap, int32_t max_tracks, const int32_t* slots_host, const int32_t* visits_host, int32_t B,
                          const float* corners_world, const int32_t* labels, const unsigned char* valid, int32_t P, float iou_thresh,
                          uint64_t seed, void* workspace, size_t workspace_bytes, float* iou_out, parq_stream stream) {
    if (B < 0 || S_cap < 0) return fail(PARQ_ERR_ARG, "parq_gt_tracks_update: negative count");
    if (P < 1 || P > 2048 || max_tracks < 1 || max_tracks > 2048)
        return fail(PARQ_ERR_ARG, "parq_gt_tracks_update: P = %d, max_tracks = %d; 1 <= P, max_tracks <= 2048", P, max_tracks);
    if (B == 0) return PARQ_OK;                                         // no scene: no launch
    if (!store || !slots_host || !visits_host || !corners_world || !labels || !valid || !workspace)
        return fail(PARQ_ERR_ARG, "parq_gt_tracks_update: NULL argument");
    {
        std::vector<char> seen((size_t)S_cap, 0);
        for (int b = 0; b < B; ++b) {
            const int32_t sl = slots_host[b];
            if (sl < 0 || sl >= S_cap) return fail(PARQ_ERR_ARG, "parq_gt_tracks_update: slot %d of scene %d outside [0, %d)", sl, b, S_cap);
            if (seen[(size_t)sl]) return fail(PARQ_ERR_ARG, "parq_gt_tracks_update: slot %d listed twice in one call", sl);
            if (visits_host[b] < 0) return fail(PARQ_ERR_ARG, "parq_gt_tracks_update: visit %d of scene %d is negative", visits_host[b], b);
            seen[(size_t)sl] = 1;
        }
    }
    const size_t need = parq_gt_tracks_update_workspace_bytes(B, P, max_tracks);
    if (workspace_bytes < need) return fail(PARQ_ERR_ARG, "parq_gt_tracks_update: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    if ((uintptr_t)workspace & 15) return fail(PARQ_ERR_ARG, "parq_gt_tracks_update: the workspace must be 16-byte aligned");
    for (int b0 = 0; b0 < B; b0 += kTrackChunk)
        HIPCHK(launch_gt_tracks_update(static_cast<int32_t*>(store), max_tracks, slots_host, visits_host, b0, std::min(B - b0, (int)kTrackChunk), B,
                                       corners_world, labels, valid, P, iou_thresh, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32),
                                       workspace, iou_out, (hipStream_t)stream));
    return PARQ_OK;
}

size_t parq_f1_counts_workspace_bytes(int32_t S, int32_t gt_max_tracks, int32_t T, int32_t K) {
    if (S < 0 || S > 65535 || gt_max_tracks < 1 || gt_max_tracks > 2048 || T < 1 || T > kF1MaxThresholds || K < 1 || K > kF1MaxClasses) return 0;
    return f1_counts_workspace_bytes(S, gt_max_tracks, T, K);
}

int parq_f1_counts(const void* pred_store, int32_t pred_max_tracks, const void* gt_store, int32_t gt_max_tracks, int32_t S,
                   const double* thresholds_host, int32_t T, int32_t K, void* workspace, size_t workspace_bytes, int64_t* counts,
                   int64_t* invalid, double* best_iou, parq_stream stream) {
    if (S < 0) return fail(PARQ_ERR_ARG, "parq_f1_counts: negative count");
    if (S > 65535 || pred_max_tracks < 1 || pred_max_tracks > 2048 || gt_max_tracks < 1 || gt_max_tracks > 2048 || T < 1 || T > kF1MaxThresholds ||
        K < 1 || K > kF1MaxClasses)
        return fail(PARQ_ERR_ARG, "parq_f1_counts: S = %d, capacities %d / %d, T = %d, K = %d; S <= 65535, 1 <= capacity <= 2048, 1 <= T <= %d, "
                    "1 <= K <= %d", S, pred_max_tracks, gt_max_tracks, T, K, kF1MaxThresholds, kF1MaxClasses);
    if (!thresholds_host || !counts || !invalid) return fail(PARQ_ERR_ARG, "parq_f1_counts: NULL argument");
    if (S == 0) {                                                       // no scene: the counts are zero
        HIPCHK(hipMemsetAsync(counts, 0, (size_t)(2 + T) * K * 8, (hipStream_t)stream));
        HIPCHK(hipMemsetAsync(invalid, 0, 16, (hipStream_t)stream));
        return PARQ_OK;
    }
    if (!pred_store || !gt_store || !workspace) return fail(PARQ_ERR_ARG, "parq_f1_counts: NULL argument");
    const size_t need = parq_f1_counts_workspace_bytes(S, gt_max_tracks, T, K);
    if (workspace_bytes < need) return fail(PARQ_ERR_ARG, "parq_f1_counts: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    if ((uintptr_t)workspace & 15) return fail(PARQ_ERR_ARG, "parq_f1_counts: the workspace must be 16-byte aligned");
    F1Thresholds thr;
    for (int t = 0; t < kF1MaxThresholds; ++t) thr.thr[t] = t < T ? thresholds_host[t] : 0.0;
    HIPCHK(launch_f1_counts(static_cast<const int32_t*>(pred_store), pred_max_tracks, static_cast<const int32_t*>(gt_store), gt_max_tracks, S,
                            thr, T, K, workspace, counts, invalid, best_iou, (hipStream_t)stream));
    return PARQ_OK;
}

size_t parq_average_precision_workspace_bytes(int32_t S, int32_t pred_max_tracks, int32_t gt_max_tracks, int32_t T, int32_t K) {
    if (S < 0 || S > 65535 || pred_max_tracks < 1 || pred_max_tracks > 2048 || gt_max_tracks < 1 || gt_max_tracks > 2048 || T < 1 ||
        T > kF1MaxThresholds || K < 1 || K > kF1MaxClasses || (int64_t)S * pred_max_tracks > kApMaxPositions)
        return 0;
    return average_precision_workspace_bytes(S, pred_max_tracks, T, K);
}

int parq_average_precision(const void* pred_store, int32_t pred_max_tracks, const void* gt_store, int32_t gt_max_tracks, int32_t S,
                           const double* thresholds_host, int32_t T, int32_t K, void* workspace, size_t workspace_bytes, double* ap,
                           int64_t* counts, int64_t* invalid, int32_t* order, int32_t* class_start, int32_t* cum_tp, double* pred_best,
                           int32_t* pred_target, parq_stream stream) {
    if (S < 0) return fail(PARQ_ERR_ARG, "parq_average_precision: negative count");
    if (S > 65535 || pred_max_tracks < 1 || pred_max_tracks > 2048 || gt_max_tracks < 1 || gt_max_tracks > 2048 || T < 1 || T > kF1MaxThresholds ||
        K < 1 || K > kF1MaxClasses)
        return fail(PARQ_ERR_ARG, "parq_average_precision: S = %d, capacities %d / %d, T = %d, K = %d; S <= 65535, 1 <= capacity <= 2048, "
                    "1 <= T <= %d, 1 <= K <= %d", S, pred_max_tracks, gt_max_tracks, T, K, kF1MaxThresholds, kF1MaxClasses);
    if ((int64_t)S * pred_max_tracks > kApMaxPositions)
        return fail(PARQ_ERR_ARG, "parq_average_precision: S * pred_max_tracks = %lld; at most %d positions are ranked",
                    (long long)S * pred_max_tracks, kApMaxPositions);
    if (!thresholds_host || !ap || !counts || !invalid) return fail(PARQ_ERR_ARG, "parq_average_precision: NULL argument");
    const int given = (order != nullptr) + (class_start != nullptr) + (cum_tp != nullptr) + (pred_best != nullptr) + (pred_target != nullptr);
    if (given != 0 && given != 5)
        return fail(PARQ_ERR_ARG, "parq_average_precision: order, class_start, cum_tp, pred_best and pred_target are given together or all NULL");
    if (S == 0) {                                                       // no scene: everything is zero
        HIPCHK(hipMemsetAsync(ap, 0, (size_t)T * K * 8, (hipStream_t)stream));
        HIPCHK(hipMemsetAsync(counts, 0, (size_t)2 * K * 8, (hipStream_t)stream));
        HIPCHK(hipMemsetAsync(invalid, 0, 16, (hipStream_t)stream));
        if (class_start) HIPCHK(hipMemsetAsync(class_start, 0, (size_t)(K + 1) * 4, (hipStream_t)stream));
        return PARQ_OK;
    }
    if (!pred_store || !gt_store || !workspace) return fail(PARQ_ERR_ARG, "parq_average_precision: NULL argument");
    const size_t need = parq_average_precision_workspace_bytes(S, pred_max_tracks, gt_max_tracks, T, K);
    if (workspace_bytes < need) return fail(PARQ_ERR_ARG, "parq_average_precision: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    if ((uintptr_t)workspace & 15) return fail(PARQ_ERR_ARG, "parq_average_precision: the workspace must be 16-byte aligned");
    F1Thresholds thr;
    for (int t = 0; t < kF1MaxThresholds; ++t) thr.thr[t] = t < T ? thresholds_host[t] : 0.0;
    HIPCHK(launch_average_precision(static_cast<const int32_t*>(pred_store), pred_max_tracks, static_cast<const int32_t*>(gt_store),
                                    gt_max_tracks, S, thr, T, K, workspace, ap, counts, invalid, order, class_start, cum_tp, pred_best,
                                    pred_target, (hipStream_t)stream));
    return PARQ_OK;
}

size_t parq_tracks_life_bytes(int32_t S_cap, int32_t max_tracks) {
    if (S_cap < 0 || max_tracks < 1 || max_tracks > 2048) return 0;
    return (size_t)S_cap * (4 + 4 * (size_t)max_tracks) * 4;
}

// the slots of a life call: each inside [0, S_cap) and listed once
static int check_life_slots(const char* who, const int32_t* slots_host, int32_t B, int32_t S_cap) {
    std::vector<char> seen((size_t)S_cap, 0);
    for (int b = 0; b < B; ++b) {
        const int32_t sl = slots_host[b];
        if (sl < 0 || sl >= S_cap) return fail(PARQ_ERR_ARG, "%s: slot %d of scene %d outside [0, %d)", who, sl, b, S_cap);
        if (seen[(size_t)sl]) return fail(PARQ_ERR_ARG, "%s: slot %d listed twice in one call", who, sl);
        seen[(size_t)sl] = 1;
    }
    return PARQ_OK;
}

int parq_tracks_note(const void* store, void* life, int32_t S_cap, int32_t max_tracks, const int32_t* slots_host, int32_t B,
                     const int32_t* track_id, int32_t Q, int32_t* uid_out, int32_t* hits_out, parq_stream stream) {
    if (B < 0 || S_cap < 0) return fail(PARQ_ERR_ARG, "parq_tracks_note: negative count");
    if (Q < 1 || Q > 2048 || max_tracks < 1 || max_tracks > 2048)
        return fail(PARQ_ERR_ARG, "parq_tracks_note: Q = %d, max_tracks = %d; 1 <= Q, max_tracks <= 2048", Q, max_tracks);
    if (B == 0) return PARQ_OK;                                         // no scene: no launch
    if (!store || !life || !slots_host || !track_id) return fail(PARQ_ERR_ARG, "parq_tracks_note: NULL argument");
    if (int rc = check_life_slots("parq_tracks_note", slots_host, B, S_cap)) return rc;
    for (int b0 = 0; b0 < B; b0 += kTrackChunk)
        HIPCHK(launch_tracks_note(static_cast<const int32_t*>(store), static_cast<int32_t*>(life), max_tracks, slots_host, b0,
                                  std::min(B - b0, (int)kTrackChunk), track_id, Q, uid_out, hits_out, (hipStream_t)stream));
    return PARQ_OK;
}

int parq_tracks_retire(void* store, void* life, int32_t S_cap, int32_t max_tracks, const int32_t* slots_host, int32_t B, int32_t min_hits,
                       int32_t max_age, int32_t tentative_age, int32_t* remap_out, parq_stream stream) {
    if (B < 0 || S_cap < 0) return fail(PARQ_ERR_ARG, "parq_tracks_retire: negative count");
    if (max_tracks < 1 || max_tracks > 2048) return fail(PARQ_ERR_ARG, "parq_tracks_retire: max_tracks = %d; 1 <= max_tracks <= 2048", max_tracks);
    if (min_hits < 1) return fail(PARQ_ERR_ARG, "parq_tracks_retire: min_hits = %d; a confirmed track has at least one hit", min_hits);
    if (B == 0) return PARQ_OK;                                         // no scene: no launch
    if (!store || !life || !slots_host) return fail(PARQ_ERR_ARG, "parq_tracks_retire: NULL argument");
    if (int rc = check_life_slots("parq_tracks_retire", slots_host, B, S_cap)) return rc;
    for (int b0 = 0; b0 < B; b0 += kTrackChunk)
        HIPCHK(launch_tracks_retire(static_cast<int32_t*>(store), static_cast<int32_t*>(life), max_tracks, slots_host, b0,
                                    std::min(B - b0, (int)kTrackChunk), min_hits, max_age, tentative_age, remap_out, (hipStream_t)stream));
    return PARQ_OK;
}

size_t parq_set_match_workspace_bytes(int32_t I, int32_t B, int32_t Q, int32_t nmax) {
    if (I < 0 || B < 0 || Q < 1 || Q > 2048 || nmax < 1 || nmax > 2048 || (int64_t)I * B * Q > (int64_t)(1 << 28)) return 0;
    return set_match_workspace_bytes(I, B, Q, nmax);
}

int parq_set_match(const float* pred_logits, const float* coord_pos, int32_t I, int32_t B, int32_t Q, int32_t num_classes,
                   const float* t_center, const int32_t* t_label, const int32_t* t_count, int32_t nmax, float cost_class, float cost_bbox,
                   float ratio, int32_t max_padding, uint32_t seed_lo, uint32_t seed_hi, uint32_t step, void* workspace,
                   size_t workspace_bytes, int32_t* row_to_col, int32_t* pairs, float* pair_coef, float* row_weight, int32_t* stats,
                   float* cost_out, unsigned char* near_out, parq_stream stream) {
    if (I < 0 || B < 0 || max_padding < 0) return fail(PARQ_ERR_ARG, "parq_set_match: negative count");
    if (Q < 1 || Q > 2048 || nmax < 1 || nmax > 2048 || num_classes < 2)
        return fail(PARQ_ERR_ARG, "parq_set_match: Q = %d, nmax = %d, num_classes = %d; 1 <= Q, nmax <= 2048 and num_classes >= 2", Q, nmax,
                    num_classes);
    if ((int64_t)I * B * Q > (int64_t)(1 << 28)) return fail(PARQ_ERR_ARG, "parq_set_match: I * B * Q above 2^28");
    if (I == 0 || B == 0) return PARQ_OK;                               // no problem: no launch
    if (!pred_logits || !coord_pos || !t_center || !t_label || !t_count || !workspace || !row_to_col || !pairs || !pair_coef || !row_weight ||
        !stats)
        return fail(PARQ_ERR_ARG, "parq_set_match: NULL argument");
    const size_t need = parq_set_match_workspace_bytes(I, B, Q, nmax);
    if (workspace_bytes < need) return fail(PARQ_ERR_ARG, "parq_set_match: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    if ((uintptr_t)workspace & 15) return fail(PARQ_ERR_ARG, "parq_set_match: the workspace must be 16-byte aligned");
    HIPCHK(launch_set_match(pred_logits, coord_pos, I, B, Q, num_classes, t_center, t_label, t_count, nmax, cost_class, cost_bbox, ratio,
                            max_padding, seed_lo, seed_hi, step, workspace, row_to_col, pairs, pair_coef, row_weight, stats, cost_out,
                            near_out, (hipStream_t)stream));
    return PARQ_OK;
}

size_t parq_draw_boxes_workspace_bytes(int32_t B, int32_t T, int32_t M) {
    if (B < 1 || T < 1 || M < 0 || M > (1 << 24) || (int64_t)B * T > 65535) return 0;
    return draw_minmax_bytes(B, T) + (size_t)B * T * M * 12 * 8;
}

int parq_draw_boxes(const float* images, const float* camera, const float* T_camera_pseudoCam, const float* T_world_pseudoCam,
                    const float* corners_world, const int32_t* labels, const unsigned char* keep, const int32_t* count, const float* colors,
                    int32_t num_classes, int32_t B, int32_t T, int32_t H, int32_t W, int32_t M, void* workspace, size_t workspace_bytes,
                    void* out, int32_t out_uint8, parq_stream stream) {
    if (B < 1 || T < 1 || H < 1 || W < 1 || M < 0 || M > (1 << 24) || (int64_t)B * T > 65535)
        return fail(PARQ_ERR_ARG, "parq_draw_boxes: bad dims (B, T, H, W >= 1, 0 <= M <= 2^24, B * T <= 65535)");
    if (H > 8192 || W > 8192) return fail(PARQ_ERR_ARG, "parq_draw_boxes: H = %d, W = %d; at most 8192 each", H, W);
    if (!images || !camera || !T_camera_pseudoCam || !T_world_pseudoCam || !workspace || !out)
        return fail(PARQ_ERR_ARG, "parq_draw_boxes: NULL argument");
    if (M > 0 && (!corners_world || !labels || !colors)) return fail(PARQ_ERR_ARG, "parq_draw_boxes: NULL boxes, labels or colours with M = %d", M);
    if (M > 0 && num_classes < 2) return fail(PARQ_ERR_ARG, "parq_draw_boxes: num_classes = %d (the last class is the background)", num_classes);
    if (out_uint8 != 0 && out_uint8 != 1) return fail(PARQ_ERR_ARG, "parq_draw_boxes: out_uint8 must be 0 or 1");
    const size_t need = parq_draw_boxes_workspace_bytes(B, T, M);
    if (workspace_bytes < need) return fail(PARQ_ERR_ARG, "parq_draw_boxes: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    if ((uintptr_t)workspace & 15) return fail(PARQ_ERR_ARG, "parq_draw_boxes: the workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    char* slots = static_cast<char*>(workspace) + draw_minmax_bytes(B, T);
    HIPCHK(launch_draw_minmax(images, B, T, H, W, workspace, s));
    if (M > 0)
        HIPCHK(launch_draw_project(camera, T_camera_pseudoCam, T_world_pseudoCam, corners_world, labels, keep, count, num_classes, B, T, M,
                                   slots, s));
    HIPCHK(launch_draw_raster(images, workspace, slots, labels, colors, B, T, H, W, M, out, out_uint8, s));
    return PARQ_OK;
}

int parq_frames_resize(const unsigned char* frames, int32_t N, int32_t H_in, int32_t W_in, int32_t pad_left, int32_t pad_top, int32_t pad_right,
                       int32_t pad_bottom, const int32_t* plan_x, const int32_t* plan_y, int32_t H_out, int32_t W_out, void* out,
                       int32_t out_uint8, parq_stream stream) {
    if (!frames || !plan_x || !plan_y || !out) return fail(PARQ_ERR_ARG, "parq_frames_resize: NULL argument");
    if (out_uint8 != 0 && out_uint8 != 1) return fail(PARQ_ERR_ARG, "parq_frames_resize: out_uint8 must be 0 or 1");
    if (!frames_sizes_ok(N, H_in, W_in, pad_left, pad_top, pad_right, pad_bottom, H_out, W_out))
        return fail(PARQ_ERR_ARG, "parq_frames_resize: N = %d frames of %d x %d, pad (%d, %d, %d, %d), to %d x %d (W x H): 1 <= N <= 65535, "
                    "sizes >= 1, pads >= 0, every side (padded too) at most 8192 and at most 8 times the output's",
                    N, W_in, H_in, pad_left, pad_top, pad_right, pad_bottom, W_out, H_out);
    HIPCHK(launch_frames_resize(frames, N, H_in, W_in, pad_left, pad_top, pad_right, pad_bottom, plan_x, plan_y, H_out, W_out, out, out_uint8,
                                (hipStream_t)stream));
    return PARQ_OK;
}

size_t parq_snippet_targets_workspace(int32_t B, int32_t T, int32_t Hd, int32_t Wd, int32_t N) {
    if (!snippet_sizes_ok(B, T, Hd, Wd, N)) return 0;
    return snippet_workspace_bytes(B, T, Hd, Wd, N);
}

int parq_snippet_targets(const uint16_t* depth, int32_t B, int32_t T, int32_t Hd, int32_t Wd, const float* depth_intrinsics_inv,
                         const float* color_intrinsics, int32_t color_h, int32_t color_w, const double* T_world_camera, const float* obbs,
                         const double* corners_world, const void* sym, int32_t sym_is_int, int32_t S, int32_t N, int32_t max_box,
                         const int32_t* level_counts_host, const float* level_ratios_host, int32_t n_levels, int32_t max_level,
                         float depth_scale, void* workspace, size_t workspace_bytes, float* obbs_padded, void* sym_out, int32_t* num_valid,
                         int32_t* frame_points, float* frame_truncation, int32_t* points_inside, float* truncation, int32_t* difficulty,
                         int32_t* valid, parq_stream stream) {
    if (!depth || !depth_intrinsics_inv || !color_intrinsics || !T_world_camera || !obbs || !level_counts_host || !level_ratios_host ||
        !workspace || !obbs_padded || !num_valid || !frame_points || !frame_truncation || !points_inside || !truncation || !difficulty || !valid)
        return fail(PARQ_ERR_ARG, "parq_snippet_targets: NULL argument");
    if (S < 0 || (S > 0 && (!sym || !sym_out))) return fail(PARQ_ERR_ARG, "parq_snippet_targets: S = %d with sym %p, sym_out %p", S, sym, sym_out);
    if (!snippet_sizes_ok(B, T, Hd, Wd, N))
        return fail(PARQ_ERR_ARG, "parq_snippet_targets: B = %d scenes of T = %d frames of %d x %d (W x H), N = %d boxes: 1 <= B <= 1023, "
                    "1 <= T <= 64, 1 <= N <= 128, every side in [1, 8192]", B, T, Wd, Hd, N);
    if (color_h < 1 || color_w < 1 || color_h > 8192 || color_w > 8192)
        return fail(PARQ_ERR_ARG, "parq_snippet_targets: colour image of %d x %d (W x H): every side in [1, 8192]", color_w, color_h);
    if (max_box < 1 || max_box > (1 << 20)) return fail(PARQ_ERR_ARG, "parq_snippet_targets: max_box = %d", max_box);
    if (S > (1 << 20)) return fail(PARQ_ERR_ARG, "parq_snippet_targets: S = %d", S);
    if (sym_is_int != 0 && sym_is_int != 1) return fail(PARQ_ERR_ARG, "parq_snippet_targets: sym_is_int must be 0 or 1");
    if (n_levels < 1 || n_levels > 8 || max_level < 0 || max_level > n_levels)
        return fail(PARQ_ERR_ARG, "parq_snippet_targets: n_levels = %d, max_level = %d: 1 <= n_levels <= 8, 0 <= max_level <= n_levels", n_levels,
                    max_level);
    if (!(depth_scale > 0.0f)) return fail(PARQ_ERR_ARG, "parq_snippet_targets: depth_scale must be above 0");
    if ((uintptr_t)depth & 1) return fail(PARQ_ERR_ARG, "parq_snippet_targets: the depth must be 2-byte aligned");
    const size_t need = parq_snippet_targets_workspace(B, T, Hd, Wd, N);
    if (workspace_bytes < need) return fail(PARQ_ERR_ARG, "parq_snippet_targets: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    if ((uintptr_t)workspace & 15) return fail(PARQ_ERR_ARG, "parq_snippet_targets: the workspace must be 16-byte aligned");
    HIPCHK(launch_snippet_targets(depth, B, T, Hd, Wd, depth_intrinsics_inv, color_intrinsics, color_h, color_w, T_world_camera, obbs,
                                  corners_world, sym, sym_is_int, S, N, max_box, level_counts_host, level_ratios_host, n_levels, max_level,
                                  depth_scale, workspace, obbs_padded, sym_out, num_valid, frame_points, frame_truncation, points_inside,
                                  truncation, difficulty, valid, (hipStream_t)stream));
    return PARQ_OK;
}

int parq_set_loss(const float* pred_logits, const float* center_unnormalized, const float* size_unnormalized, const float* ortho6d,
                  int32_t I, int32_t B, int32_t Q, int32_t num_classes, const float* t_center, const float* t_size, const float* t_rot,
                  const int32_t* t_label, const int32_t* t_sym, int32_t nmax, const int32_t* pairs, const float* pair_coef, int32_t P,
                  const float* row_weight, const float* class_weight, const float* loss_weight4_host, float* terms, float* g_logits,
                  float* g_center, float* g_size, float* g_ortho6d, int32_t* class_scratch, parq_stream stream) {
    return parq_set_loss_flags(pred_logits, center_unnormalized, size_unnormalized, ortho6d, I, B, Q, num_classes, t_center, t_size, t_rot,
                               t_label, t_sym, nmax, pairs, pair_coef, P, row_weight, class_weight, loss_weight4_host, terms, g_logits,
                               g_center, g_size, g_ortho6d, class_scratch, 0, stream);
}

size_t parq_set_loss_scratch_bytes(int32_t I, int32_t B, int32_t Q, int32_t P, int32_t flags) {
    if (I < 1 || B < 1 || Q < 1 || P < 0 || (flags & ~PARQ_SETLOSS_DETERMINISTIC)) return 0;
    const int64_t rows = (int64_t)I * B * Q;
    return (size_t)(rows + ((flags & PARQ_SETLOSS_DETERMINISTIC) ? setloss_part_floats(P, rows) : 0)) * 4;
}

int parq_set_loss_flags(const float* pred_logits, const float* center_unnormalized, const float* size_unnormalized, const float* ortho6d,
                        int32_t I, int32_t B, int32_t Q, int32_t num_classes, const float* t_center, const float* t_size, const float* t_rot,
                        const int32_t* t_label, const int32_t* t_sym, int32_t nmax, const int32_t* pairs, const float* pair_coef, int32_t P,
                        const float* row_weight, const float* class_weight, const float* loss_weight4_host, float* terms, float* g_logits,
                        float* g_center, float* g_size, float* g_ortho6d, int32_t* class_scratch, int32_t flags, parq_stream stream) {
    if (flags & ~PARQ_SETLOSS_DETERMINISTIC) return fail(PARQ_ERR_ARG, "unknown set-loss flags 0x%x", (unsigned)flags);
    if (!pred_logits || !center_unnormalized || !size_unnormalized || !ortho6d || !t_center || !t_size || !t_rot || !t_label || !row_weight ||
        !class_weight || !loss_weight4_host || !terms || !g_logits || !g_center || !g_size || !g_ortho6d || !class_scratch)
        return fail(PARQ_ERR_ARG, "NULL argument");
    if (I < 1 || B < 1 || Q < 1 || num_classes < 2 || nmax < 1 || P < 0 || (P > 0 && (!pairs || !pair_coef))) return fail(PARQ_ERR_ARG, "bad dims");
    // deterministic: the term partials live behind the I*B*Q class targets (parq_set_loss_scratch_bytes)
    float* det_part = (flags & PARQ_SETLOSS_DETERMINISTIC) ? reinterpret_cast<float*>(class_scratch + (int64_t)I * B * Q) : nullptr;
    HIPCHK(launch_set_loss(pred_logits, center_unnormalized, size_unnormalized, ortho6d, I, B, Q, num_classes, t_center, t_size, t_rot,
                           t_label, t_sym, nmax, pairs, pair_coef, P, row_weight, class_weight, loss_weight4_host, num_classes - 1, terms,
                           g_logits, g_center, g_size, g_ortho6d, class_scratch, (hipStream_t)stream, det_part));
    return PARQ_OK;
}

int parq_k_layernorm(const float* X, const float* gamma, const float* beta, float* Y, int32_t M, int32_t C, float eps,
                     parq_stream stream) {
    if (!X || !gamma || !beta || !Y || M < 1 || C < 1 || C > 1024) return fail(PARQ_ERR_ARG, "bad argument");
    HIPCHK(launch_layernorm(X, gamma, beta, Y, M, C, eps, (hipStream_t)stream));
    return PARQ_OK;
}

}  // extern "C"
