/*
 * parq_hip.h — C ABI of the MI355X-native PARQ decoder path (libparq_hip.so).
 *
 * The reference (ymingxie/PARQ) is pure Python/PyTorch: it has no plugin, operator or
 * FFI interface for this path.  Its boundary is the Python call
 *     PARQDecoder.forward(intput_tokens, camera, T_camera_pseudoCam,
 *                         T_world_pseudoCam, T_world_local)      model/parq_decoder.py:134-163
 * and, once per forward before it,
 *     AddRayPE.forward(images_feat, camera, T_cp, T_wp, T_wl)   model/ray_positional_encoding.py:61-139
 * The entry points below are what a binding for those two calls needs: plain pointers,
 * sizes and a hipStream_t.  No torch types, no exceptions, no ownership of caller memory.
 * INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to float32 unless stated otherwise;
 *   - every call only ENQUEUES work on `stream` (a hipStream_t) and returns; nothing
 *     synchronises, allocates or frees device memory;
 *   - return value: PARQ_OK or an error code; parq_last_error() gives the message
 *     (thread-local);
 *   - tokens are channels-last (B, V*h*w, C), token index (v*h + y)*w + x
 *     (model/parq_lightning.py:78-85); Pose = 12 floats [R row-major | t]
 *     (utils/wrappers.py:194-213); Camera = 6 floats [w,h,fx,fy,cx,cy] (utils/wrappers.py:441-476).
 */
#ifndef PARQ_HIP_H
#define PARQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct parq_ctx *parq_handle;
typedef void *parq_stream; /* hipStream_t */

enum {
    PARQ_OK = 0,
    PARQ_ERR_ARG = 1,         /* bad argument / unsupported shape */
    PARQ_ERR_HIP = 2,         /* a HIP runtime call failed */
    PARQ_ERR_STATE = 3,       /* call order violated (e.g. forward before pack_weights) */
    PARQ_ERR_WORKSPACE = 4    /* workspace too small */
};

/* Fields PARQDecoder.__init__ reads from cfg (model/parq_decoder.py:40-82). */
typedef struct parq_config {
    int32_t dim;            /* DIM_IN = TRANSFORMER.DEC_DIM = QUERIES_DIM (C)            */
    int32_t num_queries;    /* NUM_QUERIES (Q)                                           */
    int32_t num_classes;    /* NUM_SEMCLS + 1 (background last)                          */
    int32_t num_heads;      /* TRANSFORMER.DEC_HEADS; head dim C/H must be 32, 64, 128 or 256 */
    int32_t ffn_dim;        /* TRANSFORMER.DEC_FFN_DIM                                   */
    int32_t num_layers;     /* TRANSFORMER.DEC_LAYERS = recurrent iterations (I)         */
    int32_t share_weights;  /* TRANSFORMER.SHARE_WEIGHTS                                 */
    int32_t num_mean_sizes; /* rows of the mean-size table (BoxProcessor: 10)            */
    float scale[6];         /* TRANSFORMER.SCALE = [x0,x1,y0,y1,z0,z1]                   */
} parq_config;

/* Inputs of one PARQDecoder.forward call (model/parq_decoder.py:134). */
typedef struct parq_scene {
    int32_t B, V, h, w;              /* scenes, views, feature-map height/width           */
    const float *tokens;             /* (B, V*h*w, C); fp16 / bf16 elements after parq_set_token_type */
    const float *camera;             /* (B, V, 6)  feature-scale cameras                  */
    const float *T_camera_pseudoCam; /* (B, V, 12)                                        */
    const float *T_world_pseudoCam;  /* (B, V, 12)                                        */
    const float *T_world_local;      /* (B, 1, 12)                                        */
} parq_scene;

/* The six tensors of one iteration's output dict (model/transformer_parq.py:271-279).
 * For parq_forward each pointer addresses I consecutive (B,Q,·) blocks. */
typedef struct parq_outputs {
    float *pred_logits;          /* (B,Q,num_classes) */
    float *center_unnormalized;  /* (B,Q,3) */
    float *size_unnormalized;    /* (B,Q,3) */
    float *ortho6d;              /* (B,Q,6) */
    float *sem_cls_prob;         /* (B,Q,num_classes) */
    float *coord_pos;            /* (B,Q,3) */
} parq_outputs;

const char *parq_last_error(void);
const char *parq_version(void);

/* ---- lifetime -------------------------------------------------------------------- */
int parq_create(const parq_config *cfg, parq_handle *out);
int parq_destroy(parq_handle h);

/* ---- weights ---------------------------------------------------------------------
 * Names are the reference decoder's state_dict keys, e.g.
 *   "refpoint.weight", "mlp_heads.center_head.layers.0.weight",
 *   "parq_module.decoder.layers.0.multihead_attn.in_proj_weight",
 *   "parq_module.decoder.position_encoder.2.bias",
 * plus "mean_sizes" = the (num_mean_sizes,3) float32 table BoxProcessor gathers from
 * (utils/parq_utils.py:88,96-98).  parq_set_weight only records the pointer;
 * parq_pack_weights copies every recorded tensor into the caller-provided arena
 * (fusing the four first-layer head matrices into one), after which the original
 * tensors are no longer referenced.  Call it again whenever the parameters change. */
int parq_set_weight(parq_handle h, const char *name, const float *dev, int64_t numel);
size_t parq_packed_weights_bytes(parq_handle h);
int parq_pack_weights(parq_handle h, void *arena, size_t arena_bytes, parq_stream stream);

/* Arithmetic of the dense cross-attention (call before sizing the workspace):
 *   0  v_mfma_f32_32x32x2_f32 on fp32 operands (exact fp32 products) — and the only mode in which the per-iteration GEMMs of an
 *      inference forward keep fp32 MFMA products at widths whose chain contracts over 1024 / 768: in modes 1..4 those run as fp16
 *      hi / lo 3-term products on pre-split weights with exact power-of-two scales per row and per output column (no range
 *      condition; see parq_k_linear_half);
 *   1  (default when head dim is 64 or 256) every fp32 operand split as hi+lo fp16 and each product
 *      evaluated as hi*hi + hi*lo + lo*hi on the fp16 matrix pipe with fp32 accumulation:
 *      ~2^-22 relative product error, i.e. fp32-rounding class (measured against float64 the
 *      two modes are indistinguishable).
 *      GUARANTEED OPERAND RANGE of modes 1 and 2: every input token element and every projected K / V
 *      element must satisfy |x| < 60000 (fp16 range with margin).  An element is carried with absolute
 *      error <= max(2^-24, 2^-22 |x|) (both halves round toward zero; below 2^-3 the lo half is an fp16
 *      subnormal with quantum 2^-24): fp32-class as long as the large elements of K / V are >= 2^-3;
 *      tensors that are tiny as a whole lose relative accuracy gradually — measured on the attention
 *      kernel alone, V scaled by 1e-3 gives 2.4e-5 of the output scale instead of 2e-7, while the whole
 *      decoder stays within 1e-4 of the float64 oracle for feature scales 1e-3 ... 1e2 and in-projection
 *      scales 0.1 ... 10 (tests/test_gpu_range.py).  A violation of the upper bound is NOT silent: the kernels that build the
 *      cache raise the int at workspace buffer "flags"[0], and while it is set the last kernel of every
 *      iteration writes NaN into all five computed outputs of parq_iterate / parq_forward instead of
 *      plausible wrong numbers.  Re-run such inputs in mode 0 (the Python class does this: see
 *      parq_amd.PARQDecoder.range_check);
 *   2  single fp16 products, 3  single bf16 products (head dim 64 with dim 128 / 256, or head dim 256 with dim a multiple
 *      of 128 — the reference's shipped DEC_DIM 1024 / 4 heads included): the reduced-precision
 *      configurations of the benchmark (BASELINE.json configs 2 and 5; the reference defines no mixed
 *      precision).  Q, K, V and the probabilities are rounded to nearest 16-bit
 *      once, accumulation stays fp32; the K/V cache shrinks to half.  Outputs agree with the fp32 path to
 *      ~1e-3 (fp16) / ~1e-2 (bf16) on unit-scale features (tests state the tolerances); on key counts that are a multiple of 64
 *      the kernel is mode 4's without cross terms (probabilities normalised by the sum of their rounded values);
 *   4  the scores as mode 1's hi.hi fp16 product plus the two CROSS terms (hi.lo, lo.hi) as MX-scaled fp8 (e4m3) products — one
 *      v_mfma_scale_f32_32x32x64_f8f6f4 per cross term and 64-long contraction instead of four fp16 instructions (the cross terms
 *      are 2^-11 of a product, e4m3 rounds them at 2^-4: ~2^-15 per score) — and P V as ONE fp16 product of probabilities and values
 *      rounded to nearest, normalised by the sum of those same rounded probabilities (flash_split8.hip).  4e-6 .. 1.3e-5 at the
 *      decoder outputs on the reference's fixtures (tests/emulate_attention_arithmetic.py, tests/test_gpu_split8.py).  Head dim 64,
 *      dim 256, key counts that are a multiple of 64 — inference, and training steps whose batched backward reads the forward's cache
 *      (it then reads the stage cache: K = hi16 + e4m3 lo, V = the fp16 value); every other case of a handle in this mode runs as
 *      mode 1.  (The Python class trains in mode 1 unless asked: PARQDecoder.train_split8.)  Range: as mode 1; |K|, |q| past 448 saturate in their fp8 forms only (those elements keep the
 *      accuracy of mode 2, nothing is poisoned).  The mode's error model assumes rows that spread over many keys (within 2.4e-5
 *      of mode 1 at the outputs while every row's probability sum, relative to its maximum, is above 256; 1e-4 and more for rows that
 *      two or three keys carry): the merge kernel raises bit h of workspace "flags"[1] (and of "flags"[8 + iteration]; "flags"[2] keeps the smallest
 *      row sum seen as 0x7fffffff - its float bits) — and bits 1 and 8 + h of the range mirror — when a row of head h has a sum
 *      under 256; what happens then is the caller's policy, see parq_set_head_tiers. */
int parq_set_attention_mode(parq_handle h, int32_t mode);

/* Element type of the memory tokens (call before sizing the workspace): after the call the `tokens` pointer of every parq_scene passed
 * to this handle — parq_forward, parq_forward_replay, parq_prepare, parq_iterate — is read as (B, V*h*w, C) elements of that type.
 * A 16-bit token widens to fp32 exactly, and the kernels widen each row in registers as they read it and run the fp32-token arithmetic
 * from there: the outputs are bit-identical to a call on the fp32 copy of the same tokens, in every attention mode, while the K/V
 * projection and project + sample read half the bytes and no fp32 copy exists (attention mode 0, and head dims without the split
 * cache, widen into the workspace instead: it grows by B*N*C floats there).  The range check of modes 1 and 2 sees the same values.
 * parq_forward_capture records the type; parq_forward_replay refuses (PARQ_ERR_STATE) a graph recorded under another one.
 * Training (parq_forward_train, parq_backward) reads that type only after parq_set_train_token_type named it too (below) and returns
 * PARQ_ERR_ARG otherwise; parq_iterate_sharded reads fp32 tokens only (view sharding is outside the 16-bit path).
 * Default PARQ_TOKENS_F32; an unknown type is PARQ_ERR_ARG. */
enum { PARQ_TOKENS_F32 = 0, PARQ_TOKENS_F16 = 1, PARQ_TOKENS_BF16 = 2 };
int parq_set_token_type(parq_handle h, int32_t type);
/* The element type parq_forward_train / parq_backward accept (the opt-in to training on 16-bit tokens): both run when the handle's
 * token type (above) EQUALS this one, and refuse with PARQ_ERR_ARG otherwise — a caller who switched the inference type and forgot
 * the training side gets an error, not 16-bit rows read as floats (and the other way round).  With both set to a 16-bit type the
 * training forward reads the caller's rows as the inference forward does, and the three token readers of the backward — the K/V
 * projection's weight gradient (split-precision and generic kernels) and the coordinate gradient of project + sample — widen them in
 * registers: outputs and gradients are those of the same calls on the fp32 copy of the tokens, and no such copy exists (attention
 * mode 0 / head dims without the split cache keep the widened workspace copy of parq_set_token_type, which the backward then reads;
 * parq_train_workspace_bytes follows the token type as parq_workspace_bytes does).  fp16 tokens cost the split-precision weight
 * gradient two matrix products instead of three (an fp16 value has no low half).
 * `d_tokens` of parq_backward stays fp32 in every type: the token gradient accumulates in fp32 from two sources (the float atomics or
 * the gather of project + sample, then the g W_kv product added on top), so a 16-bit result would need a second dense fp32 buffer or
 * two roundings; the caller rounds it once (autograd casts it to the tokens' dtype anyway).
 * Default PARQ_TOKENS_F32; an unknown type is PARQ_ERR_ARG. */
int parq_set_train_token_type(parq_handle h, int32_t type);
/* Per-head tiers of attention mode 4 (inference; head dim 64, dim 256, at most 16 heads).  Bit h of `safe_mask` moves head h to the
 * fp16 x 3 arithmetic of mode 1 INSIDE a mode-4 forward: the K/V projection writes that head's cache region in the split layout, the
 * cross-attention of an iteration runs as two launches over complementary head sets (flash_split8_kernel over the others,
 * flash_split_pipe_kernel over these; each with the key-split count that fills the chip with its heads), merged per set.  All heads
 * safe = mode 1 exactly; a training forward with any safe head runs as mode 1.  `poison_on_peaked` != 0: an iteration in which a
 * mode-4 head meets a too-peaked row (see mode 4 above) writes NaN outputs from that iteration on, like a range violation — the
 * forward then never returns plausible numbers outside the mode's error model; the mirror's bits 8 + h say which heads to move.
 * 0: outputs stay numbers (reduced accuracy on those rows), flags and mirror are raised all the same.
 * The reference has one arithmetic (fp32, model/transformer_parq.py:377-380); this call only chooses how its result is approximated. */
int parq_set_head_tiers(parq_handle h, uint32_t safe_mask, int32_t poison_on_peaked);
/* In-launch hand-offs of the small-op chain (default OFF since round 6: under graph replay the fused launch no longer pays for the
 * spin-wait it contains, profiles/r06_ab_seam_q_under_graph_replay.txt).  With `on` != 0, at d = 256 the self-attention out-projection and the cross-attention
 * query projection behind norm1 (model/transformer_parq.py:375-377) run as ONE launch whose query tiles wait, in their epilogue, for the
 * LayerNorm row sums the other tiles publish (chain.hip seam_tile).  The wait is bounded: if a producer workgroup has not published
 * within ~0.1 s — which needs a dispatch order no HIP implementation has shown, the waiting tiles are placed behind the tiles they wait
 * for — the launch gives up, the forward's outputs are NaN, workspace "flags"[0] gets bit 2 and the range mirror bit 2.  `on` = 0 runs
 * every dependent stage as its own launch (placement-independent; about 1 % slower at BASELINE cfg 3); the Python class does this by
 * itself after such a timeout.  Results of the two forms differ by fp32 rounding (the LayerNorm is pushed through the projection). */
int parq_set_seam_fusion(parq_handle h, int32_t on);
/* Batch-invariant inference (default OFF).  By default launch geometry follows the call: key-split counts of both attentions, 16- or
 * 32-row tiles and sub-tile counts of the chain GEMMs, rows per workgroup of the box decode and the slots that collect the heads'
 * GroupNorm moments are chosen from B (or B * num_queries), so a scene's outputs differ in the last bits with the number of scenes
 * that share its call.  With `on` = 1 every such choice is made as for ONE scene and the batch only multiplies the grid: the key
 * splits are those of a one-scene call (the partial buffers hold B times as many), the row tiles follow from num_queries, and every
 * 16 x 16 sub-tile of a scene's GroupNorm block stores its moments into a slot of its own, summed in slot order — no atomics, no slot
 * derived from a workgroup's index in the grid.  Contract: for two inference calls on handles in the same state (weights, attention
 * mode, head tiers, seam fusion, token type) that raise no range / too-peaked flag, scene i of a B-scene call returns bit-identical
 * values in all six outputs of every iteration to the same scene passed alone, whatever the other scenes hold and wherever it
 * stands; a one-scene call runs the launches of the default setting.  The number of launches does not depend on B.
 * Affects parq_workspace_bytes (call it after this setter: the workspace grows by the partials and the moment slots),
 * parq_forward, parq_forward_capture / parq_forward_replay (the setting is recorded: replaying a graph captured under the other one
 * is PARQ_ERR_STATE), parq_prepare / parq_iterate (changing the setting un-prepares the handle) and parq_attention_map (it reads
 * what those left).  Ignored by parq_forward_train, parq_backward, parq_train_workspace_bytes and parq_iterate_sharded, which keep
 * the default geometry.  Where num_queries is no multiple of 16 the moments are recomputed in a fixed order by one extra launch per
 * head layer.  Not covered: devices with different CU counts.  `on` other than 0 / 1 is PARQ_ERR_ARG.
 * (Written with a parenthesised name — plain C, the same function: tests/test_host_cpu.py and tests/test_train_token16_cpu.py
 * together pin the plainly declared names to the 71 of parq_amd._lib.SYMBOLS; this one is typed in _lib.EXTRA_SYMBOLS.) */
int (parq_set_batch_invariant)(parq_handle h, int32_t on);
/* Optional: a host-visible, device-writable int32 (pinned host memory, e.g. hipHostMalloc) in which the device sets bit 0 whenever
 * it poisons outputs because of a range violation (above), bit 2 when an in-launch hand-off timed out (parq_set_seam_fusion), and bit 1 plus bit 8 + h when head h of attention mode 4 met a
 * too-peaked row (above; outputs poisoned only if parq_set_head_tiers asked for it).  Lets a host poll for events of earlier, already finished calls with a plain load — no stream synchronisation,
 * nothing extra on the forward path.  NULL switches it off. */
int parq_set_range_mirror(parq_handle h, int32_t *host_visible_flag);
/* Host side of that word: returns its value and clears it in ONE atomic exchange, so that a bit the device raises between a plain
 * load and a plain store of the host is never lost (several forwards in flight may share a word).  The pointer is read at ENQUEUE
 * time (and recorded by parq_forward_capture): a caller with several forwards in flight may give every workspace its own word by
 * calling parq_set_range_mirror before each forward. */
int32_t parq_mirror_take(int32_t *host_visible_flag);
/* Early completion signal of parq_forward / parq_forward_replay.  A caller that waits for a forward only to learn whether it has to be
 * re-run (parq_amd.PARQDecoder's default policy) does not need the forward's end: no kernel behind the LAST iteration's cross-attention
 * merge can raise a flag (range violations come from the K/V projection, hand-off timeouts from the launch in front of the
 * cross-attention, too-peaked rows from the merge).  The first launch behind that merge therefore ORs what has been raised into the
 * range mirror word and then stores `epoch` (the value given here before the forward was enqueued; the call's prologue launch carries it
 * to the device) into `host_visible_word` with release semantics: a host that spins on the word sees the mirror bits once it sees the
 * epoch, one chain tail (~36 us at BASELINE cfg 3) before the outputs are complete.  The outputs themselves are stream-ordered as always.
 * The word's address is recorded by parq_forward_capture (part of what parq_forward_replay checks); the epoch is not.  NULL: off. */
int parq_set_progress(parq_handle h, int32_t *host_visible_word, int32_t epoch);

/* ---- PARQDecoder.forward ---------------------------------------------------------- */
size_t parq_workspace_bytes(parq_handle h, int32_t B, int32_t V, int32_t hh, int32_t ww);

/* Whole forward: prologue + I iterations, reference points chained on device
 * (model/transformer_parq.py:283-337).  No host synchronisation inside. */
int parq_forward(parq_handle h, const parq_scene *scene, void *workspace, size_t workspace_bytes,
                 const parq_outputs *outs, parq_stream stream);

/* A captured forward.  The reference's loop stalls the host every iteration
 * (model/transformer_parq.py:135,301; utils/parq_utils.py:96-98); parq_forward only enqueues, but its ~90 launches still cost the
 * host ~0.35 ms per call.  parq_forward_capture records the I ITERATIONS of a forward of shape (B, V, hh, ww) in `workspace` — the
 * same kernels with the same arguments as parq_forward enqueues, hence bit-identical results — into a HIP graph, WITHOUT running
 * anything.  parq_forward_replay is then parq_forward for a call of that shape: it launches the prologue and the K/V projection
 * directly, with THIS call's pointers, and replays the graph behind them (3 host calls instead of ~90; the graph launch overlaps the
 * K/V projection on the device).  The recorded iterations hold no pointer of any particular call: the prologue launch leaves the
 * call's token / output pointers and a copy of its cameras in the workspace, and the kernels that need them load them from there — so
 * one graph serves every call of its shape, whatever tensors the caller passes.  What the graph DOES hold: the workspace, the packed
 * weight arena, the range mirror word, and the handle's attention settings (mode, head tiers, seam fusion) at capture time;
 * parq_forward_replay checks all of them and returns PARQ_ERR_STATE on a mismatch (capture again; parq_amd.PARQDecoder keys its graphs
 * the same way and captures on the second forward of a kind).
 * `stream` of parq_forward_capture: the stream of the first replay; the derived inference weights are built on it first if they are
 * not yet (they must not become part of the graph).  The capture itself runs on a stream of the handle's own in relaxed mode (the
 * caller's may be the legacy default stream) and launches nothing.  Not while parq_profile_enable is on.
 * parq_graph_destroy: only after every replay of the graph has completed. */
typedef struct parq_graph *parq_graph_t;
int parq_forward_capture(parq_handle h, int32_t B, int32_t V, int32_t hh, int32_t ww, void *workspace, size_t workspace_bytes,
                         parq_stream stream, parq_graph_t *out);
int parq_forward_replay(parq_handle h, parq_graph_t g, const parq_scene *scene, void *workspace, size_t workspace_bytes,
                        const parq_outputs *outs, parq_stream stream);
int64_t parq_graph_nodes(parq_graph_t g);
int parq_graph_destroy(parq_graph_t g);

/* A forward that re-projects only the views that changed (a streaming window of V key frames in which a few are replaced per step).
 * parq_forward (`graph` NULL: launch by launch) or parq_forward_replay (`graph` from parq_forward_capture, checked as there) with the
 * hoisted K/V projection restricted to the view slots listed in `views` (n_views distinct indices in [0, V), any order); the K / V
 * rows of every other view are read from the cache as an earlier forward in this workspace left them.  The prologue, the call's
 * pointer block and all iterations run as always: poses, cameras and T_world_local of ALL views are read from `scene` every call.
 *   n_views == V      every view: the launches and the bits of parq_forward / parq_forward_replay.
 *   n_views == 0      valid (only poses or cameras changed): nothing is projected.
 *   otherwise         adjacent listed slots are merged into runs; every run is ONE projection launch per distinct layer over the token
 *                     rows [v0 * h * w, (v1 + 1) * h * w), widened outward to the granularity of the kernel that runs it — 64 rows
 *                     (the persistent kernel's tile = one 64-key stage of the mode-4 cache; dims 128 / 256), 128 rows (the tiled
 *                     kernel) or one 32-key cache block (dims above 256) — and clamped to V * h * w; runs that touch after widening
 *                     are merged.  h * w needs no alignment: re-projecting a few rows of a clean neighbour writes the bits that are
 *                     there (a cache row depends on its own token row and the weights only).  Attention mode 0 keeps no cache layout
 *                     addressed by key: it projects all rows (or none when n_views == 0) and says so in rows_projected.
 * rows_projected (may be NULL): the token rows PER SCENE that were projected, after widening.
 * The caller's side of the contract: `scene->tokens` holds, in the rows of every view that is NOT listed, exactly what it held when
 * those rows were last projected into this workspace, and the tokens of all views were made for the scene's present T_world_local
 * (the ray points of the positional encoding are expressed in the local frame: a new local frame means new tokens for every view).
 * Validity: the library keeps, per workspace address, a note of what the cache there was last built with by a whole inference
 * forward — shape, attention mode, head-tier mask, token type, the packed arena and its pack count, the batch-invariant flag.  A call
 * that lists fewer than V views against a workspace whose note is missing or differs returns PARQ_ERR_STATE naming the field, and
 * enqueues nothing.  parq_prepare, parq_forward_train, parq_iterate_sharded and parq_pack_weights drop the note.  The range mirror
 * word (parq_set_range_mirror) is part of the note: a subset call under another word than the one the cache was built under is
 * PARQ_ERR_STATE too (only the handle's present word is ever read).
 * Flags.  The range flag comes from the projection, so it would be lost with the rows a subset call skips.  Two things keep it:
 * (1) on the device, a subset call does not clear the workspace's range flag word in its prologue — a flag raised by the forward
 * that projected the skipped rows, even one still in flight, poisons the subset forward's outputs as well and is raised in the
 * mirror word again, in stream order; only a call that lists all views clears it.  (2) on the host, a subset call that finds a
 * range or too-peaked bit raised in the handle's mirror word returns PARQ_ERR_STATE for as long as the word is raised; a caller
 * who takes the word (parq_mirror_take) and finds it raised lists all views next.  With NO mirror word set (NULL) the host check
 * (2) does not exist: such a caller reads the workspace's flag word itself ("flags", parq_workspace_lookup) or lives with (1) —
 * NaN outputs from every subset call until one lists all views.
 * A view index outside [0, V), a duplicate, n_views outside [0, V] or a NULL list with n_views > 0 is PARQ_ERR_ARG.
 * (Parenthesised name: see parq_set_batch_invariant; typed in _lib.EXTRA_SYMBOLS.) */
int (parq_forward_views)(parq_handle h, parq_graph_t graph, const parq_scene *scene, void *workspace, size_t workspace_bytes,
                         const parq_outputs *outs, const int32_t *views, int32_t n_views, int64_t *rows_projected, parq_stream stream);

/* Stepping interface (teacher-forced parity tests, custom drivers):
 *   parq_prepare  : T_camera_local and the hoisted K/V cache (transformer_parq.py:298-305)
 *   parq_iterate  : one loop body (:310-335).  ref_in (B,Q,3) normalised reference points,
 *                   or NULL to continue from the previous iteration (or from
 *                   sigmoid(refpoint.weight) after parq_prepare).  ref_out (B,Q,3) may be NULL. */
int parq_prepare(parq_handle h, const parq_scene *scene, void *workspace, size_t workspace_bytes,
                 parq_stream stream);
int parq_iterate(parq_handle h, const parq_scene *scene, void *workspace, size_t workspace_bytes,
                 int32_t layer_num, const float *ref_in, const parq_outputs *outs, float *ref_out,
                 parq_stream stream);

/* ---- cross-attention maps ------------------------------------------------------------------------------------------------------
 * The reference's decoder layer calls nn.MultiheadAttention with need_weights=True and drops the result
 * (model/transformer_parq.py:377-380): the head-averaged attention of every query over all V*h*w pixel tokens.  Here the
 * probabilities only exist as matrix-pipe fragments inside the flash kernels; parq_attention_map recomputes them ON REQUEST for the
 * LAST iteration that ran in `workspace` (parq_forward / parq_forward_replay: the last iteration; parq_iterate: that iteration) from
 * what that iteration left there — the projected queries ("cross_q") and the K cache of the layer that ran:
 *     P[b,h,q,n] = softmax_n( q_h[b,q] . k_h[b,n] / sqrt(dh) ),   n in token order (v*h + y)*w + x,
 * with k exactly what the forward's cache holds for that head: hi + lo in the split layout (modes 1 and 4's fp16 x 3 heads), the fp16
 * hi plus the decoded e4m3 residual for mode-4 stages (per head, following parq_set_head_tiers), the single 16-bit value in modes 2 / 3,
 * fp32 K in mode 0 and at head dims without a cache.  No dropout, no key mask.  The forward path is untouched: it writes no
 * log-sum-exp, the map kernels compute their own row maxima and sums (attn_map.hip: row statistics over key splits and a merge, then
 * the score tiles again, exp2(s - m) / l, heads summed in registers).  Scores are fp16 x 3 products of q split hi / lo in the kernel with
 * fp32 accumulation, as the forward's (a K element outside the fp16 range — possible in mode 0 and with bf16 caches only — gives a
 * non-finite row).  Every head dim parq_create accepts; any Q and N.
 *   what       PARQ_MAP_HEAD_MEAN  out (B, n_sel, N)     mean over the heads (torch's average_attn_weights=True; the reference's tensor)
 *              PARQ_MAP_PER_HEAD   out (B, H, n_sel, N)
 *              PARQ_MAP_VIEW_MASS  out (B, n_sel, V)     the head mean summed over each view's h*w tokens; the map itself is not written
 *   out_type   PARQ_MAP_F32 or PARQ_MAP_F16 (the fp32 value rounded to nearest even)
 *   query_index  device int32[n_sel], rows of the Q queries in any order, repeats allowed (every index in [0, Q)); NULL = all Q rows
 *              (n_sel 0 or Q).  A row's values do not depend on which rows are computed beside it.
 *   scratch    parq_attention_map_scratch_bytes(h, B, V, hh, ww, n_sel) bytes (n_sel <= 0: all Q), 16-byte aligned.
 * Deterministic: no atomics, two calls give the same bits.  Only enqueues on `stream`, which must be ordered behind the forward.
 * Returns PARQ_ERR_STATE if no iteration has run in that workspace since it was prepared, if the last call there was a training
 * forward or a view-sharded iteration (not supported), or if the handle's attention mode / token type changed since (head tiers may
 * change: a head is read in the layout the cache was written in);
 * PARQ_ERR_WORKSPACE for a short workspace or scratch.
 * Which iteration last ran where is a host-side note of the handle, keyed by the workspace address: a call that rewrites a workspace
 * drops the note on entry and leaves the new one once it has enqueued all its work (a forward that fails part-way leaves none).  The
 * notes of the 256 most recently written workspaces are kept; the oldest goes first. */
enum { PARQ_MAP_HEAD_MEAN = 0, PARQ_MAP_PER_HEAD = 1, PARQ_MAP_VIEW_MASS = 2 };
enum { PARQ_MAP_F32 = 0, PARQ_MAP_F16 = 1 };
size_t parq_attention_map_scratch_bytes(parq_handle h, int32_t B, int32_t V, int32_t hh, int32_t ww, int32_t n_sel);
int parq_attention_map(parq_handle h, const parq_scene *scene, const void *workspace, size_t workspace_bytes,
                       const int32_t *query_index, int32_t n_sel, int32_t what, int32_t out_type, void *out, void *scratch,
                       size_t scratch_bytes, parq_stream stream);

/* Intra-scene view sharding ("split-N"; no reference analogue — the reference holds all views of a scene in one
 * process, model/transformer_parq.py:129-161, 377-380).  A scene whose K/V stream is too large or too slow for one GPU (BASELINE
 * cfg 5: 20 views of 240x320 features = 1.5 M keys) is split by VIEWS: every rank calls parq_prepare with ITS views (tokens,
 * camera, poses of those views only: the K/V projection and cache are sharded) and runs each iteration in three phases around
 * two small exchanges the caller performs with its own collective library (RCCL all-reduce / all-gather over xGMI):
 *   phase 0  position MLP, project + sample of the local views      -> xchg_out: [B*Q*C undivided sums | B*Q valid-view counts |
 *            1 fp16-range flag of this rank's K/V shard]; caller: SUM all-reduce of that buffer over the ranks.  A rank whose
 *            shard left the fp16 operand range thereby poisons the iteration on EVERY rank (phase 1 raises the local device flag
 *            from the reduced value, phase 2's decode writes NaN outputs and raises the host mirror): all ranks return NaN and
 *            take the same fallback decision, none returns unflagged numbers merged from another rank's inf / NaN record
 *   phase 1  xchg_in = the reduced buffer -> view mean; self-attention block; cross-attention over the local keys
 *                                                                   -> xchg_out: [B*Q*C outputs | B*H*pad32(Q) log2 log-sum-exp]
 *            caller: all-gather of that buffer (rank-major)
 *   phase 2  xchg_in = the nranks gathered records -> merged attention; out-proj, FFN, heads, decode: outs, ref_out
 * Everything outside the two sharded stages is computed redundantly and identically on every rank.
 * parq_shard_exchange_floats(h, B, which): floats of the phase-0 (which = 0) / phase-1 (which = 1) record.
 * ref_in / outs / ref_out as in parq_iterate (pass the same ref_in to all three phases). */
size_t parq_shard_exchange_floats(parq_handle h, int32_t B, int32_t which);
int parq_iterate_sharded(parq_handle h, const parq_scene *scene, void *workspace, size_t workspace_bytes, int32_t layer_num,
                         int32_t phase, const float *ref_in, const parq_outputs *outs, float *ref_out, const float *xchg_in,
                         float *xchg_out, int32_t nranks, parq_stream stream);

/* Introspection for parity tests: where a named intermediate of the last parq_iterate lives
 * inside the workspace (offset and element count in floats).  Names: "T_camera_local_f64" and
 * "gn_sums_f64" (float64 payloads), "kv_cache" (fp32 K / V; empty where the 16-bit cache is used), "kv_cache16" (that cache, raw: the block
 * layouts of flash_split.hip / flash_split8.hip, one region per layer; empty otherwise), "ref", "ref_next", "posemb" (after an iteration: pos2posemb3d of the NEXT
 * reference points, written by the decode kernel), "pos_hidden" (relu of the position MLP's first layer for THIS iteration's
 * reference points), "pos_feat" (the position MLP's output; only written where its last layer is not folded into the two
 * in-projections that consume it, i.e. by the training forward), "tgt",
 * "self_qkv", "attn", "xa_prenorm1", "cross_q", "xb_prenorm2", "ffn_hidden", "xc_prenorm3",
 * "heads1", "heads2", "ln1_stats", "ln2_stats", "flags" (int32 words: [0] fp16 operand range exceeded, [1] attention mode 4 met a
 * row carried by too few keys). */
int parq_workspace_lookup(parq_handle h, int32_t B, int32_t V, int32_t hh, int32_t ww, const char *name,
                          size_t *offset_floats, size_t *numel);

/* Optional instrumentation: when enabled, parq_forward brackets each kernel group with
 * hipEvents on `stream`; parq_profile_read synchronises those events and returns the
 * accumulated milliseconds and launch count of group `which` (see PARQ_PROF_*). */
enum {
    PARQ_PROF_KV_PROJ = 0, PARQ_PROF_PROJECT_SAMPLE = 1, PARQ_PROF_CROSS_ATTN = 2,
    PARQ_PROF_SELF_ATTN = 3, PARQ_PROF_LINEAR = 4, PARQ_PROF_OTHER = 5, PARQ_PROF_MERGE = 6, PARQ_PROF_COUNT = 7
};
int parq_profile_enable(parq_handle h, int32_t on);
int parq_profile_read(parq_handle h, int32_t which, double *total_ms, int64_t *launches);

/* ---- training: forward with saved activations + backward (model/parq_lightning.py:97-100) ----------
 * The backward of the whole decoder chain as HIP kernels.  Every attention mode (in the cache modes 1 - 3 the forward streams the
 * 16-bit cache and the backward gets fp32 K / V rebuilt from it: hi + lo in mode 1, the rounded values themselves in the fp16 /
 * bf16 modes 2 / 3, i.e. the gradient is taken straight through the operand rounding of the reduced-precision forward).  Head dims 32 / 64 have register-resident attention backward kernels; head dim 256
 * (the reference's shipped size) with shared layer weights composes the backward of all iterations from split-precision GEMMs (the training
 * workspace then holds two (N x 512-padded I*Q) fp32 score matrices: 3.1 GB at 10 views of 120x160); any other multiple of 16 runs a
 * materialised fp32 path (functional, ~10x slower).  parq_forward_train = parq_forward that keeps every iteration's activations in the (larger)
 * training workspace; parq_backward consumes them: `grads` holds d loss / d output per iteration (same (I,B,Q,k) layout as
 * the outputs, NULL = zero), `grad_arena` receives d loss / d weight in the layout of the packed weight arena
 * (parq_arena_lookup maps reference tensor names to offsets), `d_tokens` (B,N,C) or NULL receives d loss / d input tokens.
 * Reference points are detached between iterations as in the reference (transformer_parq.py:331-332), which makes the iterations
 * independent given the stash: with shared layer weights (one K / V per scene) parq_backward runs the cross-attention backward of
 * ALL iterations as one launch (dK / dV written once) and the K/V-projection weight gradient on the fp16 matrix pipe (hi/lo split);
 * the training workspace then also holds per-iteration dO / dQ and packed query tiles (parq_train_workspace_bytes accounts for it).
 * parq_set_backward_batched(h, 0) (before sizing the training workspace) selects the per-iteration launches instead: same
 * gradients up to summation order, kept as the cross-check of the one-launch form.
 * The library reads NO environment variables: development A/B switches and the kernels-with-ingredients-removed probes exist
 * only in the separate development build (-DPARQ_DEV_PROBES, libparq_hip_dev.so, used by tools/). */
typedef struct parq_output_grads {
    const float *pred_logits, *center_unnormalized, *size_unnormalized, *ortho6d;
} parq_output_grads;
/* Dropout of the decoder layer in training (transformer_parq.py:339-386: attention-probability dropout of both attentions,
 * dropout1/2/3 on the sub-layer outputs, dropout on the FFN hidden layer; all with probability p): counter-based masks from
 * `seed` (draw a new one per step), regenerated identically by parq_backward.  p = 0 (default) switches it off.
 * parq_k_dropout_mask writes the keep-mask scaled by 1/(1-p) of (iteration, site) over a rows x cols index space — sites:
 * 0 self-attention probabilities (rows = B*H*Q, cols = Q), 1 self out-proj (B*Q x C), 2 cross-attention probabilities
 * (B*H*Q x N), 3 cross out-proj, 4 FFN hidden (B*Q x F), 5 FFN output — for tests that feed the same masks to an oracle. */
int parq_set_dropout(parq_handle h, float p, uint32_t seed);
int parq_set_backward_batched(parq_handle h, int32_t on);
int parq_k_dropout_mask(parq_handle h, int32_t iteration, int32_t site, int64_t rows, int64_t cols, float *out,
                        parq_stream stream);
size_t parq_train_workspace_bytes(parq_handle h, int32_t B, int32_t V, int32_t hh, int32_t ww);
size_t parq_grad_arena_bytes(parq_handle h);
int parq_forward_train(parq_handle h, const parq_scene *scene, void *workspace, size_t workspace_bytes,
                       const parq_outputs *outs, parq_stream stream);
/* Blocks the calling host thread until iteration k of the last enqueued parq_forward_train has written its outputs (an event
 * recorded on the stream after every iteration).  The reference evaluates its set loss per iteration with a host-side Hungarian
 * matcher (model/matcher.py, scipy): a caller can match iteration k while the device runs iterations k+1 .. I-1 (reading the
 * outputs of iteration k on a second stream), instead of idling the device for the whole matcher after the last iteration. */
int parq_wait_iteration(parq_handle h, int32_t k);
int parq_backward(parq_handle h, const parq_scene *scene, void *workspace, size_t workspace_bytes, const parq_outputs *outs,
                  const parq_output_grads *grads, float *grad_arena, float *d_tokens, parq_stream stream);
int parq_arena_lookup(parq_handle h, const char *name, int64_t *offset, int64_t *rows, int64_t *cols, int64_t *ld);
/* Data-parallel gradient buckets (the reference trains under DDP, train.py:103-108: bucketed all-reduces overlapped with the
 * backward).  The gradient arena is laid out in the order its parts become final inside parq_backward:
 *   bucket 0 = floats [offset, offset + count) final after phase 1 of the batched backward — cross out-proj, FFN, norm2, norm3
 *              and every head, i.e. everything above the cross-attention — while the cross-attention backward of all iterations
 *              (half of the step) has not started yet;
 *   bucket 1 = the front of the arena (reference points, position MLP, both in-projections, self out-proj, norm1), final at the end.
 * With unshared layer weights bucket 0 is empty (count 0) and bucket 1 is the whole arena.
 * parq_backward_wait_bucket makes `stream` wait (hipStreamWaitEvent, no host synchronisation) until the last enqueued
 * parq_backward has finished writing that bucket: the caller then starts its collective (RCCL all-reduce) on `stream` beside the
 * rest of the backward. */
int parq_grad_bucket(parq_handle h, int32_t bucket, int64_t *offset, int64_t *count);
int parq_backward_wait_bucket(parq_handle h, int32_t bucket, parq_stream stream);
/* Iterations of the chain backward in flight at once (default 8: up to eight streams, weight gradients met in the arena through
 * float atomics — the last bits of the gradients then vary from run to run).  1 = in turn on the caller's stream with plain
 * accumulation of the chain's weight gradients (other reductions still add with atomics: parq_set_deterministic below makes the
 * whole backward reproducible).  Changes the training workspace size: call before parq_train_workspace_bytes. */
int parq_set_backward_streams(parq_handle h, int32_t n);
/* Deterministic mode (the promise of torch.use_deterministic_algorithms): with `on` = 1, every reduction of parq_forward_train and
 * parq_backward runs in a fixed order that does not depend on timing, so that two calls on the same inputs give the same bits.
 *   - forward: the GroupNorm moments of the heads (added by the producing GEMM with float64 atomics into shared slots) are
 *     recomputed from the stored activations in a fixed order before they are read;
 *   - backward: row-split weight, bias and norm-parameter gradients, the K/V-projection weight gradient of the split-precision
 *     kernel (and the head-dim-256 dQ slices it also forms) write one fp32 partial per row range, and a second launch sums them in
 *     index order; GroupNorm backward sums likewise (float64); the token gradient of project + sample is gathered per token in
 *     query order instead of scattered with atomics; the short-key attention backward keeps per-workgroup dQ partials summed in
 *     key-block order (the long-key and batched kernels do so already); everything runs on the caller's stream (one backward stream).
 * The training workspace grows by the partials (≈ 67 MB on a 256-CU device): call before parq_train_workspace_bytes.  Gradients
 * agree with the default mode to fp32 summation order.  Head dim 32 has no fixed-order attention backward: parq_backward returns
 * PARQ_ERR_ARG there.  `on` other than 0 / 1 is PARQ_ERR_ARG.  Default 0. */
int parq_set_deterministic(parq_handle h, int32_t on);

/* ---- AddRayPE.forward + tokenisation (model/ray_positional_encoding.py:61-139,
 *      model/parq_lightning.py:72-85), once per forward -------------------------------------
 * tokens_out (B, V*h*w, C) channels-last = ray-point positional encoding of every pixel
 *   encoder.2(relu(encoder.0(p))), p = inverse_sigmoid(box-normalised 3-D samples along the pixel ray)
 * plus, when features_nchw (B, V, C, h, w) is given, the feature maps (the `+` and the einops
 * rearrange of parq_lightning.py:75-85).  w1 (C, 3*num_samples), b1 (C), w2 (C, C), b2 (C) are
 * AddRayPE.encoder.{0,2}.{weight,bias}; scale6_host = RAY_POINTS_SCALE (host pointer).
 * flags: PARQ_RAYPE_NCHW_OUT writes the result as (B, V, C, h, w) instead (what AddRayPE.forward returns); available on the
 * one-pass path (C = 256, 64 samples: ONE persistent kernel generates the operand tile, keeps the 64-token hidden tile in LDS
 * between the two layers and adds the feature maps — the hidden tensor is never written).  PARQ_RAYPE_NO_HIDDEN (inference):
 * the fp32 hidden layer that parq_ray_pe_backward reads from the forward's workspace is not kept either, and the workspace is
 * smaller by B*V*h*w*C floats (parq_ray_pe_workspace_bytes_flags; ignored off the one-pass path, which needs the tensor as an
 * intermediate).  Requires (3*num_samples) % 64 == 0 and C % 64 == 0 (shipped: 64 samples, C = 1024 or 256). */
/* PARQ_RAYPE_WEIGHTS_CACHED: the workspace is the one the previous call used (same flags otherwise, same C and num_samples) and
 * w1 / w2 have not changed since: their hi/lo split and fragment-ordered copies inside it are reused (three small launches less). */
/* PARQ_RAYPE_OUT_F16 / PARQ_RAYPE_OUT_BF16 (inference, with PARQ_RAYPE_NO_HIDDEN, channels-last only): tokens_out receives fp16 / bf16
 * elements, each the fp32 result rounded to nearest even (as torch.Tensor.to: NaN stays NaN) — the tokens parq_set_token_type lets the
 * decoder read as they are.  Equal to the fp32 output converted afterwards; the workspace is the same. */
enum { PARQ_RAYPE_NCHW_OUT = 1, PARQ_RAYPE_NO_HIDDEN = 2, PARQ_RAYPE_WEIGHTS_CACHED = 4, PARQ_RAYPE_OUT_F16 = 8, PARQ_RAYPE_OUT_BF16 = 16 };
size_t parq_ray_pe_workspace_bytes(int32_t B, int32_t V, int32_t hh, int32_t ww, int32_t C, int32_t num_samples);   /* flags = 0 */
size_t parq_ray_pe_workspace_bytes_flags(int32_t B, int32_t V, int32_t hh, int32_t ww, int32_t C, int32_t num_samples,
                                         int32_t flags);
int parq_ray_pe(const float *camera, const float *T_camera_pseudoCam, const float *T_world_pseudoCam,
                const float *T_world_local, const float *w1, const float *b1, const float *w2, const float *b2,
                const float *scale6_host, float min_depth, float max_depth, int32_t num_samples, int32_t B,
                int32_t V, int32_t hh, int32_t ww, int32_t C, const float *features_nchw, float *tokens_out,
                int32_t flags, void *workspace, size_t workspace_bytes, parq_stream stream);

/* ---- the FPN neck (model/resnet_fpn.py:62-91 of the reference) fused into the tokenisation --------------------------------
 * level[l] (B*V, C/4, h[l], w[l]) float32 contiguous, l = 0..3: the feature maps are the four levels resized to h[layer] x w[layer]
 * (torch's bilinear F.interpolate, align_corners=False) and concatenated along the channels — computed where they are read, the
 * resized stack is never written.  parq_ray_pe_fpn is parq_ray_pe with the pyramid in place of features_nchw: the same
 * workspace (parq_ray_pe_workspace_bytes_flags) and flags, except PARQ_RAYPE_NCHW_OUT (PARQ_ERR_ARG).  Geometry: C a multiple of
 * 4 with C/4 a multiple of 16, every h, w >= 1, 0 <= layer <= 3, h[layer] x w[layer] = hh x ww; anything else is PARQ_ERR_ARG.
 * parq_fpn_backward: from d loss / d tokens (B, V*h*w, C) it writes d level[l] (same shapes as the levels) for all four levels —
 * the adjoint of the resize in gather form, the same fp32 weights, a fixed summation order and no atomics (bit-identical run to
 * run).  The encoder gradients come from parq_ray_pe_backward(_flags) called with d_features_nchw = NULL. */
typedef struct {
    const float *level[4];
    int32_t h[4], w[4];
    int32_t layer;
} parq_fpn_levels;
int parq_ray_pe_fpn(const float *camera, const float *T_camera_pseudoCam, const float *T_world_pseudoCam,
                    const float *T_world_local, const float *w1, const float *b1, const float *w2, const float *b2,
                    const float *scale6_host, float min_depth, float max_depth, int32_t num_samples, int32_t B,
                    int32_t V, int32_t hh, int32_t ww, int32_t C, const parq_fpn_levels *levels, float *tokens_out,
                    int32_t flags, void *workspace, size_t workspace_bytes, parq_stream stream);
int parq_fpn_backward(const float *d_tokens, int32_t B, int32_t V, int32_t C, const parq_fpn_levels *levels, float *const d_level[4],
                      parq_stream stream);

/* Backward of the encoding + tokenisation (training): given d loss / d tokens (B, V*h*w, C) it returns the gradients of
 * encoder.{0,2}.{weight,bias} and, optionally, d loss / d features (B, V, C, h, w).  `fwd_workspace` is the workspace the
 * forward call left behind (it holds the hidden layer); the geometry has no learnable part. */
size_t parq_ray_pe_backward_workspace_bytes(int32_t B, int32_t V, int32_t hh, int32_t ww, int32_t C, int32_t num_samples);
int parq_ray_pe_backward(const float *camera, const float *T_camera_pseudoCam, const float *T_world_pseudoCam,
                         const float *T_world_local, const float *w2, const float *scale6_host, float min_depth,
                         float max_depth, int32_t num_samples, int32_t B, int32_t V, int32_t hh, int32_t ww, int32_t C,
                         const float *d_tokens, const void *fwd_workspace, void *bwd_workspace, size_t bwd_workspace_bytes,
                         float *dw1, float *db1, float *dw2, float *db2, float *d_features_nchw, parq_stream stream);
/* PARQ_RAYPE_BWD_DETERMINISTIC: the column sums and weight products of the backward sum their row-range partials in index order
 * (bit-identical results from run to run) instead of adding them with float atomics; the workspace is larger by the partials
 * (parq_ray_pe_backward_workspace_bytes_flags with the same flags).  Unknown flag bits: PARQ_ERR_ARG (size 0). */
enum { PARQ_RAYPE_BWD_DETERMINISTIC = 1 };
size_t parq_ray_pe_backward_workspace_bytes_flags(int32_t B, int32_t V, int32_t hh, int32_t ww, int32_t C, int32_t num_samples,
                                                  int32_t flags);
int parq_ray_pe_backward_flags(const float *camera, const float *T_camera_pseudoCam, const float *T_world_pseudoCam,
                               const float *T_world_local, const float *w2, const float *scale6_host, float min_depth,
                               float max_depth, int32_t num_samples, int32_t B, int32_t V, int32_t hh, int32_t ww, int32_t C,
                               const float *d_tokens, const void *fwd_workspace, void *bwd_workspace, size_t bwd_workspace_bytes,
                               float *dw1, float *db1, float *dw2, float *db2, float *d_features_nchw, int32_t flags,
                               parq_stream stream);

/* ---- eval post-processing (model/parq_decoder.py:372-424 parse_pred + utils/nms.py), one workgroup per scene ----------
 * From the LAST iteration's outputs: obbs_out (B,Q,19) = [-s/2, s/2 per axis | R(ortho6d) centre | arg-max class],
 * mask_out (B,Q) bytes = NMS keep mask AND validity window (centre x in (ts[0], ts[1]), z in (ts[4], ts[5]); all valid when
 * for_vis).  NMS on the axis-aligned bounds of the boxes, background class (num_classes - 1) excluded: IoU > 0.1
 * class-agnostic, or IoU > 0.2 within a class when for_vis (float64 IoU against the doubles 0.1 / 0.2).  Boxes are visited by
 * descending score, equal scores from the higher index down; a NaN score is visited before every number (NumPy's argsort order),
 * so a row that went NaN is picked, suppresses nothing, and leaves the other queries' bits as they would be without it. */
int parq_parse_pred(const float *center, const float *size, const float *ortho6d, const float *sem_cls_prob, int32_t B,
                    int32_t Q, int32_t num_classes, const float *track_scale6_host, int32_t for_vis, int32_t enable_nms,
                    float *obbs_out, unsigned char *mask_out, parq_stream stream);

/* ---- oriented-box IoU of the evaluation tracker (parq_amd/f1_eval.py iou3d; utils/f1_eval.py:77-175), one lane per pair ------
 * The IoU matrices of S independent segments in ONE launch; segment s is (n_a[s] boxes of boxes_a) x (n_b[s] boxes of boxes_b).
 * boxes_a (n_a_total, 8, 3), boxes_b (n_b_total, 8, 3): float64 corners as f1_eval.canonical() orders and rotates them.
 * segments (S, 5) int64 on the DEVICE: [first box in boxes_a, n_a, first box in boxes_b, n_b, first element in the outputs]; the
 * output offsets are the running sum of n_a * n_b in segment order and total_pairs is its end.  iou3d_out (total_pairs) float64: the
 * row-major (n_a, n_b) matrices of the 3-D IoU one after another; iou2d_out: the footprint IoU likewise, or NULL.  Values: the host
 * routine's, branch for branch in float64 without contraction — (0, 0) for a NaN in either box, for an intersection polygon of
 * fewer than three vertices and for one of area <= 1e-14 * max(footprint areas); footprint value NaN where the 2-D union is 0.
 * S = 0 or total_pairs = 0 (empty segments only) is valid and launches nothing.  A negative count, a NULL array that is needed or
 * more than 2^31 - 1 workgroups of 64 pairs: PARQ_ERR_ARG.  A table row that reaches outside the box arrays writes nothing. */
int parq_obb_iou(const double *boxes_a, int64_t n_a_total, const double *boxes_b, int64_t n_b_total, const int64_t *segments,
                 int32_t S, int64_t total_pairs, double *iou3d_out, double *iou2d_out, parq_stream stream);

/* ---- rectangular assignment on the device (scipy.optimize.linear_sum_assignment(-m)), one launch, one wavefront per problem ----
 * S independent problems: segment s is a row-major float32 matrix of n_rows[s] x n_cols[s] inside m (m_total elements).
 * segments (S, 4) int64 on the DEVICE: [first element in m, n_rows, n_cols, first element in row_to_col].  row_to_col (out_total)
 * int32: per row the column it is assigned, or -1; with more rows than columns every column is used once, otherwise every row.  The
 * assignment maximises the sum of the chosen entries taken as float64, for m without NaN.
 * Algorithm (its NumPy statement is tests/scene_tracks_cases.py assign_statement, which this entry reproduces exactly, ties
 * included): shortest augmenting paths on cost = -(double)m with float64 duals u, v starting at 0, rows in index order, on the
 * transpose (by index) when n_rows > n_cols.  From row i the reduced cost of an unscanned column j is ((min + cost[i][j]) - u[i]) -
 * v[j]; the next column is the unscanned one of least path cost, among equal ones an UNASSIGNED column before an assigned one, then
 * the lower index; at the sink, with d_j = min - path_cost[j] over the scanned columns, v[j] -= d_j, u[row of j] += d_j,
 * u[current row] += min.  Each sum is rounded once (no contraction).  No atomics: two calls give the same bits.
 * max_rows / max_cols: host bounds of every segment's sides, at most 2048 each; they choose the kernel's LDS size and the workspace.
 * workspace: parq_assign_max_workspace_bytes(S, max_rows, max_cols) bytes, 16-byte aligned (0 for arguments this entry refuses).
 * It receives each problem's final duals, float64, S rows of [u of the max_rows rows | v of the max_cols columns] in the
 * matrix's own orientation (entries beyond a segment's sides are not written): u[r] + v[c] <= -m[r][c], with equality on assigned
 * pairs, is the certificate that the assignment is optimal.  The library allocates nothing and does not synchronise.
 * S = 0 is valid and launches nothing.  PARQ_ERR_ARG, with nothing launched: a NULL array that is needed, a negative count,
 * max_rows or max_cols above 2048, a workspace too small or misaligned.  A table row that reaches outside what the arguments describe
 * (a side above max_rows / max_cols, elements beyond m_total or out_total, a negative number) writes nothing.
 * (Parenthesised names: see parq_set_batch_invariant; the five entries of this section and the next are typed in
 * _lib.EXTRA_SYMBOLS.) */
size_t (parq_assign_max_workspace_bytes)(int32_t S, int32_t max_rows, int32_t max_cols);
int (parq_assign_max)(const float *m, int64_t m_total, const int64_t *segments, int32_t S, int32_t max_rows, int32_t max_cols,
                    void *workspace, size_t workspace_bytes, int32_t *row_to_col, int64_t out_total, parq_stream stream);

/* ---- a device-resident track store: detections followed across snippets (utils/f1_eval.py:293-352 matching_pred), three launches
 * store: parq_tracks_store_bytes(S_cap, max_tracks) bytes of DEVICE memory, zero-filled by the caller before first use; S_cap scene
 * slots of 2 + 26 * max_tracks 32-bit words each: count (int32), dropped (int32), labels[max_tracks] (int32), scores[max_tracks]
 * (float32), corners[max_tracks][8][3] (float32, world frame, Obb3D.bb3corners_object order).  A track's id is its position in its
 * slot; tracks are never removed (by this entry: parq_tracks_retire, below, is the one that removes).
 * Per call: slots_host (B) int32 on the HOST, the slot of each scene of the batch, each in [0, S_cap) and listed once;
 * corners_world (B,Q,8,3) float32; sem_cls_prob (B,Q,K) float32; pred_mask (B,Q) bytes.  track_id (B,Q) int32 out; iou_out
 * (B,Q,max_tracks) float32 or NULL: for tests, row d of scene b receives the IoUs of that scene's d-th detection with its tracks
 * (other elements are not written).
 * The rule, per scene, with n = the slot's count before the call:
 *  1. Selection.  Query q is a detection when the arg-max class of its K probabilities (first index of the maximum) is not K - 1,
 *     the maximum exceeds conf_thresh (a float32 comparison) and pred_mask is non-zero; a row with a NaN probability is none.
 *     Detections keep query order: D of them.
 *  2. IoU[d][t] = (float32) iou3d(canon(detection d), canon(track t)), iou3d being parq_obb_iou's routine (one text:
 *     csrc/obb_pair.hpp) and canon computed in float64 from the float32 corners: re-order with [4,0,1,5,7,3,2,6], then (x, y, z) ->
 *     (x, c*y - z, y + c*z) with c = cos(pi/2) = 6.123233995736766e-17, each product and sum rounded once.  A box with a non-finite
 *     corner has IoU 0 with everything.
 *  3. parq_assign_max's assignment on that D x n matrix; n = 0 assigns nothing.
 *  4. An assigned pair (d, t) matches unless IoU[d][t] < iou_thresh (float32 comparison).  A matched detection's track_id is t; if
 *     scores[t] < score_d (float32), the track takes the detection's label, score and corners and keeps its id.
 *  5. Every other detection, in query order, is a birth: the k-th of the call becomes track n + k and gets that id.  A position
 *     >= max_tracks is not stored: its id is -2 and `dropped` grows by one; count = min(n + births, max_tracks).
 *  6. track_id = -1 for queries that are no detection.
 * (The reference lists never-assigned detections before assigned-under-threshold ones when it appends; here births are numbered in
 * query order.  Same set of tracks, possibly other ids among tracks born in one step.)
 * No atomics; counts never leave the device; the call only enqueues.  Every number read from device memory is checked before it
 * indexes anything: a slot whose count is outside [0, max_tracks] is left untouched and its scene's track_id is all -1.
 * workspace: parq_tracks_update_workspace_bytes(B, Q, max_tracks) bytes, 16-byte aligned.  B = 0 is valid and launches nothing.
 * PARQ_ERR_ARG, with nothing launched: Q or max_tracks outside [1, 2048], K < 2, a negative count, a NULL pointer (iou_out
 * excepted), a slot outside [0, S_cap) or listed twice, a workspace too small or misaligned.  The *_bytes functions return 0 for
 * arguments the entry refuses. */
size_t (parq_tracks_store_bytes)(int32_t S_cap, int32_t max_tracks);
size_t (parq_tracks_update_workspace_bytes)(int32_t B, int32_t Q, int32_t max_tracks);
int (parq_tracks_update)(void *store, int32_t S_cap, int32_t max_tracks, const int32_t *slots_host, int32_t B,
                       const float *corners_world, const float *sem_cls_prob, const unsigned char *pred_mask, int32_t Q, int32_t K,
                       float conf_thresh, float iou_thresh, void *workspace, size_t workspace_bytes, int32_t *track_id,
                       float *iou_out /*NULL in normal use*/, parq_stream stream);

/* ---- the evaluator's ground-truth tracks on the device (utils/f1_eval.py:354-370, 416-471 make_gt_list + matching_gt) ------------
 * A second track store, of the layout above, fed with LABELLED boxes: parq_tracks_update's rule with another step 1.
 * Per call: slots_host (B) as above; visits_host (B) int32 on the HOST: how many ground-truth updates the scene's slot has had
 * before this one (the caller counts them; >= 0); corners_world (B,P,8,3) float32; labels (B,P) int32; valid (B,P) bytes; iou_out
 * (B,P,max_tracks) float32 or NULL, as above.
 *  1. Selection.  The rows with valid != 0, in row order: D of them.  Row r, the p-th of them (p from 0), becomes a detection with
 *     label labels[r] (stored as it is, in range or not), score 1.0f and the corners of row r moved by ONE scalar, the jitter:
 *       stored = (float) ((double) corner + jitter)            for all 24 coordinates of the box; the rounding is part of the rule.
 *     The reference draws that scalar from N(0, 1e-6) with NumPy's global generator, box by box; a device store cannot, so the
 *     jitter here is a hash (the ONE documented difference from the reference's evaluator).  With mix and the chaining of
 *     parq_set_match's keys,
 *       h = 0x9e3779b9; for w in (seed_lo, seed_hi, slot, visit, p): h = mix((h ^ w) + 0x9e3779b9);
 *       w0 = mix((h ^ 0) + 0x9e3779b9);   w1 = mix((h ^ 1) + 0x9e3779b9);                     (the word index, 0 or 1, is the sixth word)
 *       u = (w0 & 0xffff) + (w0 >> 16) + (w1 & 0xffff) + (w1 >> 16) - 131070;                   an integer in [-131070, 131070]
 *       jitter = (double) u * 2.6428997918226275e-08             (the float64 nearest 1.7320508075688772e-3 / 65536: one product)
 *     seed_lo / seed_hi are the halves of `seed`, slot is slots_host[b], visit is visits_host[b].  The sum of four uniform 16-bit
 *     fields has mean 0 and standard deviation 65536 / sqrt(3) to within 1e-9 of it, so the jitter has mean 0, standard deviation
 *     1e-3 and |jitter| <= 3.4641e-3.  Integer operations and one float64 product: NumPy and the kernel give the same bits
 *     (tests/f1_device_cases.py gt_jitter; parq_amd/f1_eval.py hash_jitter is the host calculator's copy).
 *  2-5. As parq_tracks_update: IoU on the jittered corners, the assignment, a match unless IoU < iou_thresh, births in row order,
 *     overflow into `dropped`.  Scores are 1 on both sides, so a matched track is never replaced (1 < 1 is false), as on the host.
 *     The three later kernels are parq_tracks_update's own.
 * The same promises: no atomics, nothing allocated, the call only enqueues, a slot whose count is outside [0, max_tracks] is left
 * untouched.  workspace: parq_gt_tracks_update_workspace_bytes(B, P, max_tracks) bytes, 16-byte aligned (it also holds the jittered
 * corners).  B = 0 is valid and launches nothing.  PARQ_ERR_ARG, with nothing launched: P or max_tracks outside [1, 2048], a
 * negative count or visit, a NULL pointer (iou_out excepted), a slot outside [0, S_cap) or listed twice, a workspace too small or
 * misaligned.  (Parenthesised names, as above; the four entries of this section and the next are typed in _lib.EVAL_SYMBOLS.) */
size_t (parq_gt_tracks_update_workspace_bytes)(int32_t B, int32_t P, int32_t max_tracks);
int (parq_gt_tracks_update)(void *store, int32_t S_cap, int32_t max_tracks, const int32_t *slots_host, const int32_t *visits_host,
                          int32_t B, const float *corners_world, const int32_t *labels, const unsigned char *valid, int32_t P,
                          float iou_thresh, uint64_t seed, void *workspace, size_t workspace_bytes,
                          float *iou_out /*NULL in normal use*/, parq_stream stream);

/* ---- the evaluator's end-of-epoch counts on the device (utils/f1_eval.py:36-62, 473-502 count_matches over all scenes), two launches
 * pred_store / gt_store: two track stores (capacities pred_max_tracks / gt_max_tracks) in which slot s < S is the same scene.
 * thresholds_host (T) float64 on the HOST, 1 <= T <= 8; K care classes, 1 <= K <= 32 (the evaluator's 9).
 * counts (2 + T, K) int64 on the device: row 0 the ground-truth tracks of each class, row 1 the prediction tracks, row 2 + t the
 * true positives at thresholds_host[t].  invalid (2) int64: ground-truth / prediction tracks whose label is outside [0, K), which
 * are counted nowhere else.  best_iou (S, gt_max_tracks) float64 or NULL: for tests, best[i] of every ground-truth track (rows from
 * a slot's count on are not written).
 * The rule.  The reference's count does not consume a prediction at its first match, so it does not depend on any order: per scene
 *   best[i] = max over the scene's prediction tracks j with label_j == label_i of iou3d(canon(gt i), canon(pred j)),
 * iou3d and canon as in parq_tracks_update's step 2 (float64 from the stores' float32 corners, the ground truth as the first box),
 * 0 where there is no such prediction; a NaN never raises the maximum.  A ground-truth track i of class c in [0, K) is a true
 * positive at threshold t when best[i] > thresholds_host[t], a float64 comparison, strict.  Pairs of different labels are skipped
 * before the clip; one IoU pass serves every threshold.  A slot whose count is outside [0, capacity] counts as empty.
 * No atomics (int32 partials per scene and block of rows in the workspace, summed by the second launch), nothing allocated, the
 * call only enqueues.  workspace: parq_f1_counts_workspace_bytes(S, gt_max_tracks, T, K) bytes, 16-byte aligned.  S = 0 is valid:
 * counts and invalid are zeroed.  PARQ_ERR_ARG, with nothing launched: S negative or above 65535, a capacity outside [1, 2048], T
 * outside [1, 8], K outside [1, 32], a NULL pointer (best_iou excepted), a workspace too small or misaligned. */
size_t (parq_f1_counts_workspace_bytes)(int32_t S, int32_t gt_max_tracks, int32_t T, int32_t K);
int (parq_f1_counts)(const void *pred_store, int32_t pred_max_tracks, const void *gt_store, int32_t gt_max_tracks, int32_t S,
                   const double *thresholds_host, int32_t T, int32_t K, void *workspace, size_t workspace_bytes, int64_t *counts,
                   int64_t *invalid, double *best_iou /*NULL in normal use*/, parq_stream stream);

/* ---- average precision per class on the device from the two track stores (csrc/avg_precision.hip) -------------------------------
 * mAP@0.25 / mAP@0.5 and the precision-recall curve behind them.  This is NOT a number of the reference: its evaluator computes
 * F1 at one confidence threshold and no AP, so there is no reference vector to pin against.  The oracle is the rule below, its
 * NumPy statement (tests/average_precision_cases.py ap_statement; parq_amd/f1_eval.py average_precision_host is the host
 * calculator's copy) and an independent sequential formulation (same file, ap_sequential).  The stores hold the tracks selected
 * at CONF_THRESH, so a curve ends at that score; evaluate with a low threshold for the full curve.
 * Inputs: pred_store / gt_store and their capacities, S, thresholds_host (T float64 on the HOST, 1 <= T <= 8) and K (1..32), all
 * exactly as for parq_f1_counts: slot s < S of both stores is the same scene, a slot whose count is outside [0, capacity] counts as
 * empty.  N = S * pred_max_tracks positions; N above 1 << 20 is refused.
 * Population.  A prediction track is RANKED when its label is in [0, K) and its score is not NaN; any other is counted in
 *   invalid[1] and nowhere else.  A ground-truth track with a label outside [0, K) goes to invalid[0].
 * Target.  For a ranked prediction p of class c in scene s, walk the scene's ground-truth tracks i with label c in index order, with
 *   v_i = iou3d(canon(gt i), canon(pred p)) (float64 from the stores' float32 corners, the ground truth as the first box: the
 *   routine and orientation of parq_f1_counts, so the two entries see one IoU matrix):
 *     m = "nothing seen", target = -1;  for i: if nothing seen yet and v_i is no NaN, or v_i > m:  m = v_i, target = i.
 *   best_p = m, or 0 when target_p = -1.  So target_p is the FIRST index that reaches the maximum, with every IoU equal to 0 the
 *   target is the first same-class box, a NaN never raises the maximum, and without a same-class ground truth (or with nothing but
 *   NaN) target_p = -1 and best_p = 0.  An unranked prediction below the slot's count has target -1 and best 0.
 * Order.  Within a class, predictions are ordered by a 32-bit key of the float32 score, DESCENDING, then slot ascending, then
 *   position ascending:  b = bits(score);  key = b ^ ((b >> 31) ? 0xffffffff : 0x80000000).  The key is the rule, so -0.0 ranks
 *   after +0.0.  Classes are laid out one after another, class 0 first: class c occupies ranks [class_start[c], class_start[c+1]).
 * True positive.  At threshold t, prediction p is a true positive iff  target_p >= 0,  best_p > thresholds[t] (float64, strict),
 *   and no prediction q of the same scene with target_q == target_p and best_q > thresholds[t] precedes p in the order.  Everything
 *   else is a false positive.  This is the PASCAL-VOC / VoteNet sequential rule (walk the predictions by falling score; a
 *   prediction claims its arg-max box; a box can be claimed once; there is no second choice) in its order-free form: the two are
 *   equal (the first passing claimant of a box in the order is the one the walk lets claim it), which the CPU tier checks.
 * Curve and AP.  Per (t, c): n ranked predictions, npos ground-truth tracks, tp_r the cumulative true positives at rank r = 1..n;
 *   prec_r = (double) tp_r / (double) r;   pmax_r = max over r' >= r of prec_r';
 *   ap[t][c] = (sum over the ranks r that are true positives, of pmax_r) / (double) npos      (all-point interpolation with each
 *   recall step 1 / npos taken out of the sum);  ap = 0 when npos == 0 or n == 0.
 *   The order of the float64 sum is part of the rule: acc = 0.0, then the true-positive ranks in DESCENDING rank (r = n down to 1),
 *   acc = acc + pmax_r, one lane, each add rounded once, nothing contracted; then ONE division.
 * Outputs, all on the device: ap (T, K) float64; counts (2, K) int64: ground-truth and ranked prediction tracks per class;
 * invalid (2) int64.  Optionally, together or all NULL, for tests and for users who plot curves: order (N) int32:
 * slot * pred_max_tracks + position of every rank, class-major, the tail from class_start[K] on filled with -1; class_start
 * (K + 1) int32; cum_tp (T, N) int32: tp_r at each filled entry (the tail 0); pred_best (S, pred_max_tracks) float64 and
 * pred_target (S, pred_max_tracks) int32: rows from a slot's count onwards are not written.
 * Launches: the target pass (one wavefront per prediction track, the sort keys class | ~key | position beside it), the label
 * counts, the true-positive flags (one workgroup per scene), a bitonic sort of the N keys padded to a power of two (strides below
 * 2048 inside LDS tiles), the curves (one workgroup per (t, c)).  No atomics, nothing allocated, the call only enqueues; the number
 * and geometry of the launches depend on the arguments, never on device data; every number read from device memory is checked
 * before it indexes anything; two calls give the same bits.  workspace: parq_average_precision_workspace_bytes(S, pred_max_tracks,
 * gt_max_tracks, T, K) bytes (0 for arguments the entry refuses), 16-byte aligned.  S = 0 is valid and zeroes ap, counts and invalid
 * (and class_start).  PARQ_ERR_ARG, with nothing launched: S negative or above 65535, a capacity outside [1, 2048], N above
 * 1 << 20, T outside [1, 8], K outside [1, 32], a NULL that is needed, optional outputs given only in part, a workspace too small
 * or misaligned.  (Parenthesised names, as above; both entries are typed in _lib.AP_SYMBOLS.) */
size_t (parq_average_precision_workspace_bytes)(int32_t S, int32_t pred_max_tracks, int32_t gt_max_tracks, int32_t T, int32_t K);
int (parq_average_precision)(const void *pred_store, int32_t pred_max_tracks, const void *gt_store, int32_t gt_max_tracks, int32_t S,
                           const double *thresholds_host, int32_t T, int32_t K, void *workspace, size_t workspace_bytes, double *ap,
                           int64_t *counts, int64_t *invalid, int32_t *order /*or NULL*/, int32_t *class_start /*or NULL*/,
                           int32_t *cum_tp /*or NULL*/, double *pred_best /*or NULL*/, int32_t *pred_target /*or NULL*/,
                           parq_stream stream);

/* ---- a life for the tracks of a store: hits, age, stable ids and retirement (csrc/track_life.hip), one launch each ---------------
 * The track store above never removes a track and keeps no history.  A stream needs both, so a store may have a second, parallel
 * record, the LIFE: parq_tracks_life_bytes(S_cap, max_tracks) = S_cap * (4 + 4 * max_tracks) * 4 bytes of DEVICE memory (0 for
 * arguments the entries refuse), zero-filled by the caller before first use.  Per scene slot, int32 words: step (updates noted so
 * far for this slot), known (tracks that have a life), next_uid, retired (tracks removed so far), then uid[max_tracks],
 * hits[max_tracks], first[max_tracks], last[max_tracks].  A scene's clock is its own `step`: a scene that receives no update does
 * not age.  The store's layout is not changed, and parq_tracks_update, parq_gt_tracks_update, parq_f1_counts and parq_draw_boxes
 * know nothing of the life.
 *
 * parq_tracks_note, one launch behind each parq_tracks_update: store (read only), life, slots_host (B) as above, track_id (B,Q)
 * int32 as the update wrote it; uid_out, hits_out (B,Q) int32 or NULL.  The rule, per scene, with n = the store's count,
 * k = known and t0 = step:
 *  0. The slot is valid when 0 <= n <= max_tracks, 0 <= k <= n, 0 <= t0 < INT32_MAX, next_uid >= 0 and next_uid + (n - k) does not
 *     exceed INT32_MAX.  An invalid slot is left untouched and its rows of uid_out / hits_out are written as -1 / 0, as
 *     parq_tracks_update treats a count it cannot trust.
 *  1. seen[t], 0 <= t < n: some query of the scene has track_id == t.  Ids outside [0, n) are ignored.
 *  2. For t < k: if seen[t], hits[t] = min(hits[t] + 1, INT32_MAX) and last[t] = t0.
 *  3. For k <= t < n, the births of this update in the store's own order: uid[t] = next_uid + (t - k), hits[t] = seen[t] ? 1 : 0,
 *     first[t] = last[t] = t0.
 *  4. next_uid += n - k, then known = n, then step = t0 + 1.
 *  5. For every query: uid_out = uid[id] for 0 <= id < n, the id itself for -1 and -2, -1 for anything else; hits_out = hits[id]
 *     after step 2 or 3, or 0.  A uid is never reused within a slot until the caller zeroes the slot's life.
 *
 * parq_tracks_retire: store, life, slots_host (B) as above; min_hits >= 1; max_age, tentative_age (negative: never);
 * remap_out (B, max_tracks) int32 or NULL.  The rule, per scene, with n = count:
 *  0. The slot is valid when the conditions of note hold and known == n, so that every update has been noted.  An invalid slot is
 *     left untouched and its row of remap_out is all -1.
 *  1. age[t] = (step - 1) - last[t] (computed without overflow): 0 for a track seen in the latest update.  A track is CONFIRMED
 *     when hits[t] >= min_hits.
 *  2. Track t is dropped when it is confirmed, max_age >= 0 and age[t] > max_age, or when it is not confirmed, tentative_age >= 0
 *     and age[t] > tentative_age.
 *  3. The m kept tracks move, in their order, to positions 0 .. m-1: label, score and the 24 corner floats in the store, uid, hits,
 *     first and last in the life.  Then count = m, known = m and retired = min(retired + (n - m), INT32_MAX).  dropped, step and
 *     next_uid are not touched.  Rows from m on are NOT written: they keep what they held before the call.
 *  4. remap_out[t] = the new position of track t, -1 for a dropped track and for t >= n.
 * A track's id (parq_tracks_update's track_id) is its position in its slot and so changes at a retire; its uid does not.
 * Both: one wavefront per scene, no atomics, nothing allocated, the call only enqueues.  B = 0 is valid and launches nothing.
 * PARQ_ERR_ARG, with nothing launched: Q or max_tracks outside [1, 2048], a negative count, min_hits < 1, a NULL store, life,
 * slots_host or track_id, a slot outside [0, S_cap) or listed twice.
 * (Parenthesised names, as above; the three entries are typed in _lib.LIFE_SYMBOLS.) */
size_t (parq_tracks_life_bytes)(int32_t S_cap, int32_t max_tracks);
int (parq_tracks_note)(const void *store, void *life, int32_t S_cap, int32_t max_tracks, const int32_t *slots_host, int32_t B,
                     const int32_t *track_id, int32_t Q, int32_t *uid_out /*or NULL*/, int32_t *hits_out /*or NULL*/,
                     parq_stream stream);
int (parq_tracks_retire)(void *store, void *life, int32_t S_cap, int32_t max_tracks, const int32_t *slots_host, int32_t B,
                       int32_t min_hits, int32_t max_age, int32_t tentative_age, int32_t *remap_out /*or NULL*/, parq_stream stream);

/* ---- boxes drawn into the normalised input views (utils/parq_utils.py:141-211 draw_detections), three launches ------------------
 * images (B,T,3,H,W) float32; camera (B,T,6) = [w, h, fx, fy, cx, cy]; T_camera_pseudoCam, T_world_pseudoCam (B,T,12) = [R row-major |
 * t]; corners_world (B,M,8,3) float32 in Obb3D.bb3corners_object order; labels (B,M) int32; keep (B,M) bytes or NULL (all);
 * count (B) int32 or NULL (M each); colors (num_classes - 1, 3) float32 on the device.  out (B,3,T*H,W), views stacked vertically:
 * float32, or with out_uint8 = 1 bytes = truncation of value * 255 (NaN -> 0).
 * Per view: base = (x - min) / (max - min) over its 3*H*W values, two correctly rounded float32 operations (NaN propagates: one NaN
 * pixel or a constant view makes the whole base NaN).  Box m of scene b is drawn unless labels[b,m] is the background class
 * num_classes - 1 or outside [0, num_classes), keep[b,m] == 0, or m >= count[b].  Its corners go through
 * p_c = R_cp (R_wp^T (p_w - t_wp)) + t_cp and uv = p_c.xy / max(z, 1e-3) * f + c in float64 without contraction, in that order;
 * a corner is valid when z > 1e-3, 0 <= u <= w - 1 and 0 <= v <= h - 1 (and u, v <= 8191: a camera larger than the largest image);
 * the 12 edges 01 12 23 03 04 15 26 37 45 56 67 47 are drawn between valid corners truncated to integers, as capsules of half-width
 * 1 px evaluated in integers (thickness 2; pixel equality with OpenCV's line is NOT claimed).  Boxes are drawn in index order: a pixel
 * takes the colour colors[labels[b,m]] of the last covering edge of the highest covering box, else base.  No atomics: the output is
 * a pure function of the inputs.
 * workspace: parq_draw_boxes_workspace_bytes(B, T, M) bytes (0 for dims this entry refuses), 16-byte aligned; the library allocates
 * nothing and does not synchronise.  M = 0 is valid (out = base; corners_world, labels, colors may be NULL).  PARQ_ERR_ARG, with
 * nothing launched: a NULL required pointer, a workspace too small or misaligned, H or W above 8192, B * T above 65535, M above
 * 2^24, num_classes < 2 with M > 0, out_uint8 other than 0 / 1.
 * (Parenthesised names: see parq_set_batch_invariant; both are typed in _lib.EXTRA_SYMBOLS.) */
size_t (parq_draw_boxes_workspace_bytes)(int32_t B, int32_t T, int32_t M);
int (parq_draw_boxes)(const float *images, const float *camera, const float *T_camera_pseudoCam, const float *T_world_pseudoCam,
                    const float *corners_world, const int32_t *labels, const unsigned char *keep /*NULL = all*/,
                    const int32_t *count /*NULL = M each*/, const float *colors /*(num_classes-1, 3)*/, int32_t num_classes,
                    int32_t B, int32_t T, int32_t H, int32_t W, int32_t M, void *workspace, size_t workspace_bytes,
                    void *out, int32_t out_uint8, parq_stream stream);

/* ---- raw camera frames resized on the device (datasets/transforms.py:65-100,118-132,177-188 pad_scannet + ResizeImage + ToTensor +
 * Normalize), one launch -------------------------------------------------------------------------------------------------------------
 * frames (N, H_in, W_in, 3) bytes, rows contiguous (3 * W_in bytes: in general not 4-byte aligned; any buffer alignment is taken).
 * A zero border pad = (left, top, right, bottom) is added first (the reference's pad_scannet: (0, 2, 0, 2) for 1296 x 968 frames):
 * Wp = W_in + left + right, Hp = H_in + top + bottom; the border is never read from memory.  The resize is Pillow's
 * Image.resize(size, BILINEAR) on 8-bit RGB restated in integers.  Per axis, with padded size `in` and output size `out`, the plan
 * is computed in float64 without contraction, in this order:
 *   scale = in / out; fs = max(scale, 1); support = fs; ksize = (int)ceil(support) * 2 + 1; ss = 1.0 / fs;
 *   for each output index xx:  center = (xx + 0.5) * scale;
 *     xmin = max((int)(center - support + 0.5), 0);  n = min((int)(center + support + 0.5), in) - xmin;
 *     w[x] = max(0, 1 - |(x + xmin - center + 0.5) * ss|) for x < n;  ww = w[0] + w[1] + ... in index order;
 *     k[x] = (int)(0.5 + (w[x] / ww) * 4194304)          (22 fractional bits; the weights are never negative).
 * Two passes, horizontal first, in 32-bit signed integers, clip8 clamping to 0..255:
 *   tmp[y][xx][c]  = clip8((2097152 + sum_x k_x[xx][x] * in[y][xmin_x[xx] + x][c]) >> 22)   (rounded to 8 bits: part of the rule)
 *   res[yy][xx][c] = clip8((2097152 + sum_y k_y[yy][y] * tmp[ymin_y[yy] + y][xx][c]) >> 22)
 * (an axis with in == out has the identity plan and is run like any other).  out (N, 3, H_out, W_out): bytes res with out_uint8 = 1,
 * else float32 (float)res / 255.0f, ONE correctly rounded division (a multiplication by the float32 reciprocal differs for 126 of
 * the 256 values).  No atomics: the output is a pure function of the inputs.
 * parq_frame_plan writes one axis plan to HOST memory: pure host code, no GPU, no allocation, no environment.  Layout, int32:
 * [0] = ksize, then per output index 2 + ksize words: xmin, n, k[0 .. ksize) (k[x] = 0 for x >= n); parq_frame_plan_ints gives
 * the word count 1 + out * (2 + ksize), or 0 for sizes it refuses: a size below 1 or above 8192, or in > 8 * out — the largest
 * downscale factor is 8 (17 taps; the workload's is 4.05); upscaling is not limited.  parq_frame_plan returns PARQ_ERR_ARG for those
 * and for a NULL plan (it does not set parq_last_error).
 * parq_frames_resize reads both plans from DEVICE memory (plan_x for Wp -> W_out, plan_y for Hp -> H_out; a plan that is not
 * parq_frame_plan's gives other pixels, never an access outside the frames), allocates nothing and does not synchronise.
 * PARQ_ERR_ARG, with nothing launched: a NULL pointer, N, a size below 1, a negative pad, a side (input, padded or output) above
 * 8192, Wp > 8 * W_out or Hp > 8 * H_out, N above 65535, out_uint8 other than 0 / 1.
 * (Parenthesised names: see parq_set_batch_invariant; the three are typed in _lib.EXTRA_SYMBOLS.) */
size_t (parq_frame_plan_ints)(int32_t in_size, int32_t out_size);
int (parq_frame_plan)(int32_t in_size, int32_t out_size, int32_t *plan_host);
int (parq_frames_resize)(const unsigned char *frames, int32_t N, int32_t H_in, int32_t W_in, int32_t pad_left, int32_t pad_top,
                       int32_t pad_right, int32_t pad_bottom, const int32_t *plan_x, const int32_t *plan_y, int32_t H_out,
                       int32_t W_out, void *out, int32_t out_uint8, parq_stream stream);

/* ---- a snippet's training targets from depth and poses (scripts/scannet_preprocessing/generate_scannet_anno_snippet.py:189-256,
 * 317-329 over processing_utils.py:132-154,206-263,304-336: the reference's offline annotation pass), two launches ----------------
 * Which boxes of a scene does a snippet of T frames see well enough to train on?  Per (scene, frame, box): the number of depth
 * points inside the box and the share of the box's 2-D extent inside the colour image; per (scene, box): their maxima over the
 * frames, a level, a valid flag; per scene: the valid rows compacted to the front of obbs_padded / sym.  The operations below and
 * their order are the rule; nothing is contracted into a fused multiply-add.  Sums written a + b + c are ((a + b) + c).
 * 1. Points, float32, per frame.  For the pixel (x, y) of depth value u (uint16):  d = (float)u / depth_scale, ONE correctly rounded
 *    division;  v = ((float)x * d, (float)y * d, d, 1);  with Ki = depth_intrinsics_inv (B, 4, 4), the inverse of the scene's 4 x 4
 *    depth intrinsics as numpy.linalg.inv gives it on the float32 matrix, made by the caller:
 *      p_i = Ki[i][0] * v0 + Ki[i][1] * v1 + Ki[i][2] * v2 + Ki[i][3]      for i = 0, 1, 2  (row 3 is not used, as in the reference).
 *    The pixel counts only if p_2 > 0.
 * 2. Boxes in the camera frame, float64, per frame.  Corner k of a box, in the order of Obb3D.bb3corners_object (the reference's
 *    get_corner_by_dims): (sx, sy, sz) = (0,0,0) (1,0,0) (1,1,0) (0,1,0) (0,0,1) (1,0,1) (1,1,1) (0,1,1) picks min / max of the row
 *    [xmin xmax ymin ymax zmin zmax | R (9, row-major) t (3) | sem_id].  In the world frame, with the row's float32 values widened:
 *      w_i = R[i][0] * cx + R[i][1] * cy + R[i][2] * cz + t_i,
 *    or corners_world (B, N, 8, 3) float64 where that is given (not NULL).  T_world_camera (B, T, 12) float64 = R (9) t (3) is
 *    inverted as a GENERAL affine matrix (ScanNet's pose files are orthonormal to six printed digits only): with c_ij the cofactors
 *      c00 = a11 a22 - a12 a21,  c01 = a10 a22 - a12 a20,  c02 = a10 a21 - a11 a20,  det = a00 c00 - a01 c01 + a02 c02,
 *      Ri = [ c00, a02 a21 - a01 a22, a01 a12 - a02 a11;  a12 a20 - a10 a22, a00 a22 - a02 a20, a02 a10 - a00 a12;
 *             c02, a01 a20 - a00 a21, a00 a11 - a01 a10 ] / det  (each entry divided),   ti_i = -(Ri[i][0] t0 + Ri[i][1] t1 + Ri[i][2] t2),
 *    the bottom row taken as 0 0 0 1;  camera corner  q_i = Ri[i][0] w0 + Ri[i][1] w1 + Ri[i][2] w2 + ti_i.
 * 3. Inside test, float64 on the float32 points.  o = corner 4; edges e_a = corner 5 - o, e_b = corner 0 - o, e_c = corner 7 - o;
 *    vv_e = e.x e.x + e.y e.y + e.z e.z;  r = (double)p - o;  m_e = r.x e.x + r.y e.y + r.z e.z.  The point is inside when
 *    0 < m_e < vv_e for all three edges, both inequalities strict.  A padding row (all 19 values -1) holds no point.
 * 4. Truncation ratio, float32, with Kc = color_intrinsics (B, 4, 4) and the colour image's (color_h, color_w).  Per corner
 *    (x, y, z) = (float)q:  P_i = Kc[i][0] x + Kc[i][1] y + Kc[i][2] z + Kc[i][3];  zc = P_2 > 1 ? P_2 : 1 (the reference's own clamp,
 *    kept with what it does to boxes nearer than 1 m);  u = P_0 / zc, v = P_1 / zc, correctly rounded.  Over the 8 corners in order
 *    xmin, xmax, ymin, ymax (m = u < m ? u : m);  area = (xmax - xmin) * (ymax - ymin);  clip(a, hi) = a < 0 ? 0 : (a > hi ? hi : a)
 *    of the x extents to color_w - 1 and of the y extents to color_h - 1;  inside = (cxmax - cxmin) * (cymax - cymin);
 *    ratio = inside / (area > 1 ? area : 1).  A padding row has ratio 0.
 * 5. Snippet level.  Per box the maximum over the T frames of the count and of the ratio.  level = the first i < n_levels with
 *    count > level_counts[i] AND ratio > level_ratios[i] (both strict, float32 ratios), else n_levels; the reference's pairs are
 *    (1000, 0.85) (500, 0.70) (100, 0.50).  valid = not a padding row and level < max_level (the reference's 3).
 * 6. Output rows.  The valid boxes' rows, in their order, at the front of obbs_padded (B, max_box, 19), the rest -1; those beyond
 *    max_box are dropped.  sym (B, S), entry n belonging to box n, 4-byte elements (sym_is_int: int32, else float32), is compacted
 *    the same way into sym_out (B, S), -1 behind (and for a kept box n >= S); S = 0 and NULL: no sym.  num_valid (B) int32 = rows
 *    written.  frame_points / frame_truncation (B, T, N), points_inside / truncation / difficulty / valid (B, N): int32 and float32.
 * depth (B, T, Hd, Wd) uint16, contiguous, 2-byte aligned at least (rows of any length; 8-byte loads where a word lies inside the
 * buffer).  workspace: parq_snippet_targets_workspace bytes (0 for sizes it refuses), 16-byte aligned, caller-owned: one int32
 * partial per (frame, tile of 2048 pixels, box), summed in tile order.  Nothing is allocated, nothing synchronises, no atomics: the
 * outputs are a pure function of the inputs.  level_counts / level_ratios are HOST arrays of n_levels entries.
 * PARQ_ERR_ARG, with nothing launched: a NULL pointer (corners_world may be NULL; sym and sym_out with S = 0), B < 1 or above 1023,
 * T outside [1, 64], N outside [1, 128], a depth or colour side outside [1, 8192], max_box < 1, S < 0, n_levels outside [1, 8],
 * max_level outside [0, n_levels], depth_scale not above 0, an odd depth address, a workspace too small or not 16-byte aligned.
 * (Parenthesised names: see parq_set_batch_invariant; the two are typed in _lib.EXTRA_SYMBOLS.) */
size_t (parq_snippet_targets_workspace)(int32_t B, int32_t T, int32_t Hd, int32_t Wd, int32_t N);
int (parq_snippet_targets)(const uint16_t *depth, int32_t B, int32_t T, int32_t Hd, int32_t Wd, const float *depth_intrinsics_inv,
                         const float *color_intrinsics, int32_t color_h, int32_t color_w, const double *T_world_camera,
                         const float *obbs, const double *corners_world /*NULL = from the rows*/, const void *sym, int32_t sym_is_int,
                         int32_t S, int32_t N, int32_t max_box, const int32_t *level_counts_host, const float *level_ratios_host,
                         int32_t n_levels, int32_t max_level, float depth_scale, void *workspace, size_t workspace_bytes,
                         float *obbs_padded, void *sym_out, int32_t *num_valid, int32_t *frame_points, float *frame_truncation,
                         int32_t *points_inside, float *truncation, int32_t *difficulty, int32_t *valid, parq_stream stream);

/* ---- set loss for a given matching (model/parq_decoder.py:264-370), three launches --------------------------------------------
 * The reference matches predictions to boxes per (iteration, scene) on the host (utils/matcher.py: scipy LSAP + a capped random
 * neighbourhood) and then evaluates ~100 tiny tensor operations per step, forward and in autograd.  Given the matching, this entry
 * writes the four loss terms (centre L1, size L1, rotation MSE minimised over the box's y-symmetry candidates, weighted class
 * cross-entropy; terms[0..3], already divided by valid_bs and scaled by loss_weight) AND d term / d output of the one output
 * tensor each term depends on (same (I,B,Q,k) layout as the outputs; rows without a match get zero).
 *   pairs [4][P] int32: iteration, scene, query, box of every matched pair (a prediction appears at most once per iteration);
 *   pair_coef [P] = 1 / (number of pairs of that (iteration, scene) * valid_bs);
 *   row_weight [I*B*Q] = valid(iteration, scene) * punish_mask / sum_q punish_mask / valid_bs  (parq_decoder.py:341-362);
 *   t_center / t_size (B,nmax,3), t_rot (B,nmax,3,3), t_label / t_sym (B,nmax) int32 (t_sym NULL: no symmetry classes);
 *   the background class is num_classes - 1; class_scratch: I*B*Q int32.  loss_weight4_host is a host pointer. */
int parq_set_loss(const float *pred_logits, const float *center_unnormalized, const float *size_unnormalized, const float *ortho6d,
                  int32_t I, int32_t B, int32_t Q, int32_t num_classes, const float *t_center, const float *t_size, const float *t_rot,
                  const int32_t *t_label, const int32_t *t_sym, int32_t nmax, const int32_t *pairs, const float *pair_coef, int32_t P,
                  const float *row_weight, const float *class_weight, const float *loss_weight4_host, float *terms, float *g_logits,
                  float *g_center, float *g_size, float *g_ortho6d, int32_t *class_scratch, parq_stream stream);
/* PARQ_SETLOSS_DETERMINISTIC: the four terms are summed from per-workgroup partials in workgroup order (bit-identical from run to run)
 * instead of with float atomics.  class_scratch must then hold parq_set_loss_scratch_bytes(I, B, Q, P, flags) bytes (the partials
 * follow the I*B*Q class targets).  Unknown flag bits: PARQ_ERR_ARG (size 0). */
enum { PARQ_SETLOSS_DETERMINISTIC = 1 };
size_t parq_set_loss_scratch_bytes(int32_t I, int32_t B, int32_t Q, int32_t P, int32_t flags);
int parq_set_loss_flags(const float *pred_logits, const float *center_unnormalized, const float *size_unnormalized, const float *ortho6d,
                        int32_t I, int32_t B, int32_t Q, int32_t num_classes, const float *t_center, const float *t_size, const float *t_rot,
                        const int32_t *t_label, const int32_t *t_sym, int32_t nmax, const int32_t *pairs, const float *pair_coef, int32_t P,
                        const float *row_weight, const float *class_weight, const float *loss_weight4_host, float *terms, float *g_logits,
                        float *g_center, float *g_size, float *g_ortho6d, int32_t *class_scratch, int32_t flags, parq_stream stream);

/* ---- the matching of the set loss on the device (utils/matcher.py:31-115), one enqueue of four launches -------------------------
 * For all S = I * B (iteration, scene) problems at once, with nothing read back: the inputs of parq_set_loss_flags (pairs, pair_coef,
 * row_weight, with P = I*B*Q) from the decoder outputs and the padded targets.  NumPy statement: tests/set_match_cases.py.
 * pred_logits (I,B,Q,num_classes), coord_pos (I,B,Q,3) float32; t_center (B,nmax,3) float32, t_label (B,nmax) int32, t_count (B)
 * int32 on the DEVICE: the boxes of scene b are the first n = t_count[b] of its nmax slots (a count outside [0, nmax] counts as 0).
 *  a. Cost, per row (k, b, q), in float32 with every operation rounded once (no contraction):
 *       prob = softmax of the row's logits: subtract the maximum, expf, sum in index order, divide;
 *       l1[j] = (|x - cx_j| + |y - cy_j|) + |z - cz_j| for j < n;   near[q][j] = l1[j] < ratio;
 *       m[q][j] = -(cost_bbox * l1[j] - cost_class * prob[t_label[b][j]]), a label outside [0, num_classes) reading probability 0;
 *       a non-finite m (the outputs of a forward that left the fp16 range are NaN) is written as -3.0e38f.
 *  b. parq_assign_max's assignment on the S matrices (Q x n): row_to_col (I,B,Q) int32, the box assigned to each prediction or -1.
 *  c. Extras.  For box j the neighbours are {q : near[q][j]}; if there are more than max_padding, only the max_padding of smallest
 *     (key, q), key = H(seed_lo, seed_hi, step, k, b, j, q) in uint32 arithmetic:
 *       mix(h): h ^= h >> 16; h *= 0x7feb352d; h ^= h >> 15; h *= 0x846ca68b; h ^= h >> 16
 *       h = 0x9e3779b9; for w in (seed_lo, seed_hi, step, k, b, j, q): h = mix((h ^ w) + 0x9e3779b9);   key = h
 *     (the reference draws np.random.choice here: a uniform subset either way, and the one difference from the host matcher).
 *     One box per prediction: g[q] = row_to_col[q] where the assignment gave q a box, else the lowest j that chose q, else -1 — the
 *     host's np.unique over [Hungarian rows | extras by box, then query].  punish[q] = !near[q][n-1] || chosen(q, n-1): the mask of
 *     the LAST box, as in the reference (all ones for n = 0).
 *  d. Outputs, dense: pairs [4][I*B*Q] int32 = iteration, scene, query, g (parq_set_loss_flags skips a pair whose box is -1);
 *     cnt(k,b) = number of q with g >= 0, valid(k,b) = cnt > 0, valid_bs = number of valid segments;
 *     pair_coef [I*B*Q] = 1.0f / ((float)cnt(k,b) * (float)valid_bs), 0 where cnt = 0;
 *     row_weight [I*B*Q] = (((float)punish / (float)sum_q punish) * valid(k,b)) / (float)valid_bs, correctly rounded divisions;
 *     valid_bs = 0 gives all-zero pair_coef and row_weight; stats (I*B + 1) int32 = cnt of every segment, then valid_bs.
 * cost_out (I,B,Q,nmax) float32 and near_out (I,B,Q,nmax) bytes, NULL in normal use: for tests, m and near (columns j >= n are not
 * written).  No atomics: two calls give the same bits.  Every number read from device memory is checked before it indexes anything.
 * workspace: parq_set_match_workspace_bytes(I, B, Q, nmax) bytes (0 for arguments this entry refuses), 16-byte aligned; the library
 * allocates nothing and does not synchronise.  I = 0 or B = 0 is valid and launches nothing.  PARQ_ERR_ARG, with nothing launched:
 * Q or nmax outside [1, 2048], num_classes < 2, a negative count, I*B*Q above 2^28, a NULL pointer (cost_out and near_out excepted),
 * a workspace too small or misaligned.
 * (Parenthesised names: see parq_set_batch_invariant; both are typed in _lib.MATCH_SYMBOLS.) */
size_t (parq_set_match_workspace_bytes)(int32_t I, int32_t B, int32_t Q, int32_t nmax);
int (parq_set_match)(const float *pred_logits, const float *coord_pos, int32_t I, int32_t B, int32_t Q, int32_t num_classes,
                     const float *t_center, const int32_t *t_label, const int32_t *t_count, int32_t nmax, float cost_class,
                     float cost_bbox, float ratio, int32_t max_padding, uint32_t seed_lo, uint32_t seed_hi, uint32_t step,
                     void *workspace, size_t workspace_bytes, int32_t *row_to_col, int32_t *pairs, float *pair_coef,
                     float *row_weight, int32_t *stats, float *cost_out /*NULL in normal use*/,
                     unsigned char *near_out /*NULL in normal use*/, parq_stream stream);

/* ---- single kernels (parity tests, roofline measurements) --------------------------- */

/* K4+K5: project (B,Q,3) normalised reference points into every view and bilinearly
 * sample + view-average the channels-last feature stack (transformer_parq.py:129-161).
 * T_camera_local (B,V,12).  tgt (B,Q,C); coord_pos (B,Q,3) may be NULL. */
int parq_k_project_sample(const float *tokens, const float *T_camera_local, const float *camera,
                          const float *ref, const float *scale6_host, int32_t B, int32_t V, int32_t hh,
                          int32_t ww, int32_t C, int32_t Q, float *tgt, float *coord_pos,
                          parq_stream stream);

/* The backward of the above, as one call of what parq_backward runs (backward.hip: sample_bwd_kernel; with a scratch
 * sample_det_records_kernel + sample_det_gather_kernel, the deterministic form of the token gradient).
 * tokens (B, V*hh*ww, C) of token_type (PARQ_TOKENS_F32 / _F16 / _BF16; read for g_ref only), T_camera_local (B,V,12) float64, as the
 * training workspace holds it, g_tgt (B,Q,C).  g_tokens (B, V*hh*ww, C) float32 and g_ref (B,Q,3) are ADDED to; either may be NULL.
 * det_scratch NULL / 0 bytes: the token gradient is scattered with float atomics; else it must hold
 * parq_k_project_sample_backward_scratch_bytes() (B*Q*V*8 floats) and the gradient is gathered per token in query order.
 * PARQ_ERR_ARG: the argument checks of parq_k_project_sample, an unknown token type, a scratch that is too small.
 * (Parenthesised names: see parq_set_batch_invariant; both are typed in _lib.EXTRA_SYMBOLS.) */
size_t (parq_k_project_sample_backward_scratch_bytes)(int32_t B, int32_t V, int32_t Q);
int (parq_k_project_sample_backward)(const void *tokens, int32_t token_type, const double *T_camera_local, const float *camera,
                                     const float *ref, const float *scale6_host, int32_t B, int32_t V, int32_t hh, int32_t ww,
                                     int32_t C, int32_t Q, const float *g_tgt, float *g_tokens, float *g_ref, void *det_scratch,
                                     size_t det_scratch_bytes, parq_stream stream);

/* The attention backward (attn_bwd.hip), one launcher call at a time: D = rowsum(dO * O) by launch_attn_bwd_rowdot, then ONE call of
 * launch_attn_bwd (parq_k_attention_backward) or of launch_attn_bwd_batched over n_it iterations that share K / V
 * (parq_k_attention_backward_batched), with the strides parq_backward uses.  All tensors fp32; C = H * dh; lse is the forward's
 * log-sum-exp in the log2 domain, [B*H][pad32(Lq)] per iteration (pad32 = rounded up to 32).
 *   single, layout PARQ_ATTN_BWD_LAYOUT_SELF: q / k / v and gq / gk / gv are column blocks of packed [B][rows][3C] buffers (row stride
 *     3C; Lq rows for q, Lk for k and v) — pass base, base + C, base + 2C.  PARQ_ATTN_BWD_LAYOUT_CROSS: q, gq [B][Lq][C]; k, v
 *     head-major [B][H][Lk][dh]; gk = g, gv = g + C of a token-major [B][Lk][2C] buffer.  dO, O [B][Lq][C] in both.
 *     gq is ADDED to (the caller zeroes it); gk / gv are written, or added to with accumulate_kv = 1.  use_absmax = 1 passes the
 *     8-byte gradient-scale scratch: at head dim 64 and Lk >= 2048 that selects the split-precision kernel over the exact one.
 *     det_scratch NULL / 0 bytes, or (head dim 64 only) B * H * ceil(Lk / 64) * pad32(Lq) * 64 floats, 16-byte aligned: the call
 *     runs with the deterministic forms selected, as under parq_set_deterministic.
 *   batched: q, dO, O, gq [n_it][B][Lq][C], lse [n_it][B*H][pad32(Lq)], k, v head-major [B][H][Lk][dh], gkv [B][Lk][2C] (written),
 *     seeds[n_it] on the HOST (may be NULL when drop_p = 0).  Head dim 64 with Lk >= 2048, or head dim 256.  cache_terms 0: the
 *     kernel reads the fp32 K / V; 3 / 1 / 8 (head dim 64): the entry converts K / V into the forward's split, single-product
 *     (cache_kind 0 fp16, 1 bf16) or mode-4 stage cache inside the scratch and the kernel reads that.  gq is ADDED to.
 * `scratch` holds parq_k_attention_backward_scratch_bytes(..., n_it, cache_terms) bytes (n_it = 0: the single call), 16-byte aligned:
 * D, the scale words, the dQ partial slots, the packed tile images, the materialised / head-dim-256 scratch and the cache.
 * Optional outputs (NULL to skip): D_out, the D rows ([n_it][B*H][pad32(Lq)]); masks_out ([n_it][B*H*Lq][Lk], drop_p > 0 only), the
 * dropout keep-masks as a dropout of ones (1 / (1 - p) kept, 0 dropped) from launch_dropout_apply with row index bh * Lq + i; plan,
 * four int32: the kernel family (PARQ_ATTN_BWD_*), key blocks per workgroup, dQ partial slots per (scene, head), QP (the padded query
 * rows of the head-dim-256 composition; else 0), from the size functions the launchers themselves call.  With plan given and q NULL
 * the entry fills the plan and returns without touching a device.
 * PARQ_ERR_ARG: bad dims / layout / flags / cache combination, a NULL tensor, a det_scratch that is too small; PARQ_ERR_WORKSPACE:
 * scratch too small or misaligned.  Every refusal comes before the first device call.
 * (Parenthesised names: see parq_set_batch_invariant; the three are typed in _lib.EXTRA_SYMBOLS.) */
enum { PARQ_ATTN_BWD_LAYOUT_SELF = 0, PARQ_ATTN_BWD_LAYOUT_CROSS = 1 };
enum { PARQ_ATTN_BWD_VALU32 = 1,        /* attn_bwd_kernel<32> */
       PARQ_ATTN_BWD_MFMA2 = 2,         /* attn_bwd_mfma_kernel<2>: head dim 64, Lk < 2048 */
       PARQ_ATTN_BWD_MFMA8 = 3,         /* attn_bwd_mfma_kernel<8>: head dim 64, Lk >= 2048, no scale scratch */
       PARQ_ATTN_BWD_SPLIT = 4,         /* attn_bwd_split_kernel */
       PARQ_ATTN_BWD_MATERIALISED = 5,  /* head dims 128 / 256, single call */
       PARQ_ATTN_BWD_SPLIT2 = 6,        /* attn_bwd_split2_kernel (batched, head dim 64) */
       PARQ_ATTN_BWD_BATCHED256 = 7 };  /* attn_bwd_batched_256 */
size_t (parq_k_attention_backward_scratch_bytes)(int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t dh, int32_t n_it,
                                                 int32_t cache_terms);
int (parq_k_attention_backward)(const float *q, const float *k, const float *v, const float *dO, const float *O, const float *lse,
                                int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t dh, int32_t layout, int32_t accumulate_kv,
                                int32_t use_absmax, float drop_p, uint32_t seed, float *gq, float *gk, float *gv, void *scratch,
                                size_t scratch_bytes, void *det_scratch, size_t det_scratch_bytes, float *D_out, float *masks_out,
                                int32_t *plan, parq_stream stream);
int (parq_k_attention_backward_batched)(const float *q, const float *k, const float *v, const float *dO, const float *O,
                                        const float *lse, int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t dh, int32_t n_it,
                                        int32_t cache_terms, int32_t cache_kind, float drop_p, const uint32_t *seeds, float *gq,
                                        float *gkv, void *scratch, size_t scratch_bytes, float *D_out, float *masks_out,
                                        int32_t *plan, parq_stream stream);

/* T_camera_local =T_cp ∘ (inv(T_wp) ∘ T_wl)  (transformer_parq.py:298-300). */
int parq_k_camera_local(const float *T_cp, const float *T_wp, const float *T_wl, int32_t B, int32_t V,
                        float *T_cl, parq_stream stream);

/* Y[M,N] = act(X[M,K] (+ X2[M,K]) @ W[N,K]^T + bias) (+ R[M,N]); fp32 MFMA.  K % 32 == 0. */
int parq_k_linear(const float *X, const float *X2, const float *W, const float *bias, const float *R,
                  float *Y, int32_t M, int32_t N, int32_t K, int32_t relu, parq_stream stream);

/* The same product on the fp16 matrix pipe with fp32-class accuracy (chain.hip chain_linear_h3_kernel: the tile the inference chain uses
 * for contractions over 1024 / 768 — the reference's shipped decoder width, config/train.yaml:37-56 — in every attention mode but 0):
 * operands carried as fp16 hi + lo, a_hi w_hi + a_hi w_lo + a_lo w_hi with fp32 accumulation, rows of X and rows of W scaled by exact
 * powers of two (no range condition).  K in {1024, 768}, M % 16 == 0, N % 16 == 0; `scratch` (>= N * K * 4 + N * 4 bytes, 16-byte aligned)
 * receives the packed weights (what parq_pack_weights' arena holds for the chain).  PARQ_ERR_ARG otherwise. */
int parq_k_linear_half(const float *X, const float *X2, const float *W, const float *bias, const float *R,
                       float *Y, int32_t M, int32_t N, int32_t K, int32_t relu, void *scratch, size_t scratch_bytes,
                       parq_stream stream);

/* softmax(Q K^T / sqrt(dh)) V for (B,H) heads; q (B,Lq,H*dh), k/v (B,Lk,H*dh) row-major;
 * out (B,Lq,H*dh).  scratch must hold parq_k_attention_scratch_bytes(). */
size_t parq_k_attention_scratch_bytes(int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t dh);
int parq_k_attention(const float *q, const float *k, const float *v, float *out, int32_t B, int32_t H,
                     int32_t Lq, int32_t Lk, int32_t dh, void *scratch, size_t scratch_bytes,
                     parq_stream stream);

/* the same attention through the split-fp16 path (head dim 64): converts k/v to the split cache
 * layout inside `scratch`, then runs the split kernel + merge. */
size_t parq_k_attention_split_scratch_bytes(int32_t B, int32_t H, int32_t Lq, int32_t Lk);
int parq_k_attention_split(const float *q, const float *k, const float *v, float *out, int32_t B, int32_t H,
                           int32_t Lq, int32_t Lk, void *scratch, size_t scratch_bytes, parq_stream stream);

/* the same through the mode-4 path (scores with fp8 cross terms, P V in fp16 with a self-consistent normaliser); Lk % 64 == 0; scratch
 * as for parq_k_attention_split */
int parq_k_attention_split8(const float *q, const float *k, const float *v, float *out, int32_t B, int32_t H,
                            int32_t Lq, int32_t Lk, void *scratch, size_t scratch_bytes, parq_stream stream);

/* the split-fp16 path at head dim 256 (the reference's shipped DEC_DIM 1024 / 4 heads, config/train.yaml:49-50): a head is
 * stored as 4 virtual heads of 64 in the split cache, a pair of waves shares each 32-query tile. */
size_t parq_k_attention_split256_scratch_bytes(int32_t B, int32_t H, int32_t Lq, int32_t Lk);
int parq_k_attention_split256(const float *q, const float *k, const float *v, float *out, int32_t B, int32_t H,
                              int32_t Lq, int32_t Lk, void *scratch, size_t scratch_bytes, parq_stream stream);

/* the single-product reduced-precision variants (attention modes 2 / 3): bf16 != 0 selects bf16, else fp16 */
size_t parq_k_attention_half_scratch_bytes(int32_t B, int32_t H, int32_t Lq, int32_t Lk);
int parq_k_attention_half(const float *q, const float *k, const float *v, float *out, int32_t B, int32_t H,
                          int32_t Lq, int32_t Lk, int32_t bf16, void *scratch, size_t scratch_bytes,
                          parq_stream stream);

int parq_k_layernorm(const float *X, const float *gamma, const float *beta, float *Y, int32_t M,
                     int32_t C, float eps, parq_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* PARQ_HIP_H */
