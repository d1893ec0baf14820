/*
 * ezdit.h -- C ABI of libezaudio_hip.so: the MI355X (gfx950) EzAudio denoising path.
 *
 * The reference (haidog-yaqub/EzAudio) is pure Python/PyTorch and has no FFI layer; its hot path
 * sits behind plain Python callables.  This header is therefore the boundary a maintainer would
 * bind (ctypes stub in INTEGRATION.md); each entry point names the reference interface it stands
 * in for (paths relative to the reference tree).
 *
 * Conventions (surface B3):
 *   - every pointer marked `dev` is a DEVICE pointer owned by the caller; the library never
 *     allocates or frees persistent device memory.  Weights live in one caller-owned blob laid out
 *     by ezdit_param_info(); all activations / tables live in one caller-owned workspace.
 *   - the PER-STEP entry points (ezdit_forward, ezdit_controlnet_forward, ezdit_sampler_run, ezdit_set_step,
 *     ezdit_cfg_ddim_step, ezdit_cfg_ddim_step_per_sample, ezdit_cfg_multistep_step, ezdit_cfg_apg_step, ezdit_add_noise, ezdit_canvas_blend, ezdit_canvas_blend_loop, the ezvae_* ops) are ASYNCHRONOUS on their stream: no device sync, no host read of
 *     device data (a sampler step is hipGraph-capturable).  The once-per-call SET-UP entry points synchronise the
 *     stream and must not be called inside a stream capture: ezdit_bind_workspace (diagnostic builds only),
 *     ezdit_prepare_context (reads the context mask back to find single-key batch elements when `xkey1` is on),
 *     ezdit_prepare_timesteps, ezdit_sampler_begin, ezdit_sampler_set_sample_params, ezdit_sampler_set_multistep, ezdit_sampler_set_start, ezdit_sampler_set_apg, ezdit_sampler_set_canvas and ezdit_sampler_set_canvas_loop (host staging
 *     buffers of the timestep / coefficient tables), ezdit_set_lengths, ezdit_sampler_set_pair_lengths and ezdit_sampler_set_cn_scales
 *     (host mirrors of the length / scale tables), ezdit_set_context_weights (host mirror of the prompt timeline; reads the context mask back).
 *   - return 0 = OK, negative = error; ezdit_last_error() gives a thread-local message.  No C++
 *     exception crosses the ABI.
 *   - a handle is bound to the device that was current at ezdit_create() and is NOT thread-safe:
 *     one handle per device/stream; multi-GPU = one process + one handle per GPU.
 *   - layouts: latents channel-major fp32 [rows, C, L] exactly as the reference passes them
 *     (src/inference.py:67,75); context fp32 [B, Lc, Cctx]; masks uint8 (0/1).
 */
#ifndef EZDIT_H
#define EZDIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EZDIT_ABI_VERSION 4   /* 4 (round 6): ezdit_test_attention takes V row-major [B][H][Lkp][DV] (was V^T [B][H][DV][Lkp]); the internal buffers "vt" / "vct" are "v" / "vc" */

typedef struct ezdit_handle ezdit_handle;
typedef void* ezdit_stream; /* hipStream_t */

/* Mirrors the `model:` section of ckpts/ezaudio-{l,xl}.yml (the keys UDiT.__init__ consumes,
 * src/models/udit.py:11-30).  Only the shipped combination is implemented; ezdit_create returns
 * EZDIT_E_UNSUPPORTED for anything else, mirroring the NotImplementedError sites udit.py:83,113,127. */
typedef struct {
    int32_t embed_dim;     /* D */
    int32_t num_heads;     /* H, head_dim = D / H, must be 64 or 72 */
    int32_t depth;         /* depth//2 in-blocks + mid + depth//2 out-blocks */
    int32_t in_chans;      /* 257 = 2*out_chans + 1 (MaskDiT concat, conditioners.py:161-176) */
    int32_t out_chans;     /* C = 128 latent channels */
    int32_t context_dim;   /* T5 width */
    int32_t ada_sola_rank; /* r */
    float   ada_sola_alpha;
    float   mlp_ratio;     /* 4.0 */
    int32_t max_len;       /* longest latent sequence the RoPE table covers */
    /* ControlNet variant (src/models/controlnet.py:87-315): the first depth/2 blocks of the backbone + condition embed +
     * one zero-initialised Linear per skip; no mid/out blocks, no final block.  0 = plain UDiT. */
    int32_t controlnet;
    int32_t cond_in;       /* channels of the control signal (1 for energy) */
    int32_t cond_c0;       /* cond_blocks[0] = 64 (+1 mask channel when cond_mask) */
    int32_t cond_c1;       /* cond_blocks[1] = 128 */
    int32_t cond_mask;     /* DiTControlNetEmbed cond_mask: append the (all-zero at inference) mask channel */
} ezdit_config;

enum {
    EZDIT_OK = 0,
    EZDIT_E_INVALID = -1,      /* bad argument / shape (reference: AssertionError class) */
    EZDIT_E_UNSUPPORTED = -2,  /* config value outside the implemented set (NotImplementedError) */
    EZDIT_E_STATE = -3,        /* call order: weights/workspace/context/timesteps not prepared */
    EZDIT_E_HIP = -4           /* a HIP runtime call failed */
};

/* ---- parameter blob layout (replaces MaskDiT.load_state_dict, api/ezaudio.py:83-85) ---------- */
enum { EZDIT_P_F32 = 0, EZDIT_P_BF16 = 1 };
enum {
    EZDIT_T_NONE = 0,
    EZDIT_T_GEGLU8 = 1, /* rows re-ordered so each 16-row group = 8 value rows then their 8 gate rows */
    /* fused to_q | to_k | to_v weight [3D][D] of an even head count (round 6): within the q rows [0, D) and the k rows [D, 2D), the rows of every PAIR of
     * heads (2 dh rows) are re-ordered so that stored row c = 16 j + 4 g + 2 e + s of the pair holds channel f + (dh / 2) s of head hh, with the RoPE pair
     * index f = 8 (j mod dh/16) + 2 g + e for the dh/16 full 16-row groups of a head (hh = 0 for the first dh/16 groups, 1 for the last), and -- head_dim 72:
     * 4.5 groups per head -- the middle group split by g: g < 2 -> head 0, g >= 2 -> head 1, f = 32 + 2 (g & 1) + e (csrc/gemm_pp.h qkrope_col).  A
     * channel and its rotate-half partner then sit side by side, two pairs per lane of the 16x16 MFMA output: per-head LayerNorm + RoPE run on the
     * accumulators.  The v rows [2D, 3D) keep their order.  q and k are stored in this channel order; q . k^T is invariant under it. */
    EZDIT_T_QKROPE = 2
};
typedef struct {
    char    name[64];      /* our slot name, e.g. "blk3.wqkv" */
    char    src[3][96];    /* state-dict keys concatenated along dim 0 (nsrc of them) */
    int32_t nsrc;
    int32_t dtype;         /* EZDIT_P_* */
    int32_t transform;     /* EZDIT_T_* */
    int64_t rows, cols;    /* logical shape after concatenation (trailing dims flattened) */
    int64_t rows_pad, ld;  /* stored shape: zero padded to [rows_pad][ld] */
    int64_t offset;        /* byte offset in the blob, 256-byte aligned */
} ezdit_param_info_t;

int         ezdit_abi_version(void);
const char* ezdit_last_error(void);

int    ezdit_create(const ezdit_config* cfg, ezdit_handle** out);
int    ezdit_destroy(ezdit_handle* h);

int    ezdit_param_count(const ezdit_handle* h);
int    ezdit_param_info(const ezdit_handle* h, int index, ezdit_param_info_t* out);
size_t ezdit_param_bytes(const ezdit_handle* h);
int    ezdit_bind_weights(ezdit_handle* h, const void* dev_blob, size_t bytes);

/* ---- workspace ------------------------------------------------------------------------------- */
/* B = denoiser batch rows (2 x prompts with CFG), L = latent frames, Lc = context tokens,
 * n_slots = number of distinct timesteps whose modulation tables are resident (sampler: n_steps). */
size_t ezdit_workspace_bytes(const ezdit_handle* h, int B, int L, int Lc, int n_slots);
int    ezdit_bind_workspace(ezdit_handle* h, void* dev_ws, size_t bytes, int B, int L, int Lc, int n_slots,
                            ezdit_stream stream);

/* ---- Run-time tables of the step -------------------------------------------------------------- */
/* The setters below hand the step a RUN-TIME TABLE: a small array in the workspace that the kernels of the step read at run time.  One
 * contract holds for all of them; their own comments say only what is specific to each.
 *   - A set-up entry point: the values are a HOST array, the call uploads them and waits for `stream`.  EZDIT_E_STATE inside a stream
 *     capture and before the state the table lives in exists: a bound workspace, or, for a call-scoped table, a sampler call begun on
 *     it ("ezdit_sampler_begin first").  NULL or a count of 0 switches the table off: bit for bit the call that never set it.
 *   - A captured step graph serves every set of values: new values into a table that is on keep the graph.  Switching a table on or
 *     off changes kernel arguments and drops it, and so does a kernel argument that rides with the table.
 *   - A refused call changes nothing and launches nothing.
 *   - Scope, and what else switches a table off:
 *       table (setter)                            graph dropped when                  also cleared by
 *       lengths (ezdit_set_lengths)               off <-> on                          ezdit_bind_workspace, ezdit_sampler_set_pair_lengths(NULL)
 *       the ControlNet's half of pair lengths     off <-> on: the graph of every      ezdit_bind_workspace, detach, ezdit_destroy of the backbone,
 *         (ezdit_sampler_set_pair_lengths)          backbone it is attached to; a       ezdit_set_lengths(NULL) on the ControlNet
 *                                                   changed table also invalidates
 *                                                   the condition embed
 *       ControlNet scales (.._set_cn_scales)      off <-> on                          ezdit_bind_workspace, ezdit_sampler_attach_controlnet,
 *                                                                                       ezdit_destroy of the ControlNet
 *       context weights (ezdit_set_context_weights) off <-> on                        ezdit_bind_workspace, ezdit_prepare_context
 *       token weights                             off <-> on (a table of equal        ezdit_bind_workspace, ezdit_prepare_context
 *         (ezdit_set_context_token_weights)         weights per row is off)
 *       sample settings (.._set_sample_params)    off <-> on                          ezdit_bind_workspace, ezdit_sampler_begin
 *       multistep (.._set_multistep)              off <-> on, another history buffer  ezdit_bind_workspace, ezdit_sampler_begin
 *       start (.._set_start)                      off <-> on (also moves the step     ezdit_bind_workspace, ezdit_sampler_begin
 *                                                   counter: on, min(start_steps);
 *                                                   off after on, 0)
 *       canvas (.._set_canvas, .._set_canvas_loop:  off <-> on, another T or ramp,    ezdit_bind_workspace, ezdit_sampler_begin, either setter
 *         one table, a line or a ring)              line <-> ring                       with NULL
 *       compose weights (.._begin_composed         off <-> on, another K: only a      ezdit_bind_workspace, ezdit_sampler_begin,
 *         switches it on, .._set_compose_weights     begin does either                  ezdit_sampler_begin_composed (which sets its own)
 *         replaces the values)
 *       projected guidance (.._set_apg)           off <-> on, another momentum buffer ezdit_bind_workspace, ezdit_sampler_begin,
 *                                                                                       ezdit_sampler_begin_composed
 * ezdit_bind_workspace ends the sampler call as well: ezdit_sampler_run and the call-scoped setters (the last six) return EZDIT_E_STATE
 * until the next ezdit_sampler_begin, whatever shape was bound. */

/* ---- step-invariant work, hoisted (reference recomputes it every step) ----------------------- */
/* context_embed + per-block norm_context + cross to_k/to_v + head LayerNorm(k):
 * src/models/udit.py:94-97,295-296; blocks.py:84-85,150; utils/attention.py:128-142.
 * ctx fp32 [B,Lc,Cctx]; mask uint8 [B,Lc], 1 = attend (T5 attention_mask, src/inference.py:42,47). */
int ezdit_prepare_context(ezdit_handle* h, const float* dev_ctx, const uint8_t* dev_mask, ezdit_stream stream);

/* timestep embedding, TimestepEmbedder, time_act, time_ada(_final), per-block AdaLN-SOLA:
 * utils/modules.py:19-61; udit.py:305-316; blocks.py:39-45,132-133.  `timesteps` is a HOST array.
 * per_row = 0: every batch row uses slot `cur_step` (see ezdit_set_step); sampler usage.
 * per_row = 1: n must equal B and row b uses slot b (MaskDiT.forward with a [B] timesteps tensor). */
int ezdit_prepare_timesteps(ezdit_handle* h, const int32_t* timesteps, int n, int per_row, ezdit_stream stream);
int ezdit_set_step(ezdit_handle* h, int step, ezdit_stream stream);

/* ---- mixed-length batches: per-sample valid lengths of a PADDED batch -------------------------- */
/* The batch is stored padded to L frames (x / gt / gt_mask / noise / latents [.., C, L], token rows B * L); batch row b is valid on
 * the frames [0, lengths[b % n]) -- the rule by which row b reads latent row b % x_rows, so n = P serves a CFG batch of 2 P rows.
 * `lengths` is a HOST array, 1 <= lengths[i] <= L, n divides B; NULL or n = 0 clears (every row has L frames again, bit for bit the
 * behaviour without this call; all lengths equal to L give those bits as well).  With lengths set, the valid frames of a row are what
 * a call with that row alone at its own length computes (up to rounding): self-attention sees the keys [0, len) only (the
 * reference's `x_mask`, src/models/blocks.py:143), the FinalBlock's Conv1d sees a zero at frame len (which `x_mask` does NOT give),
 * `rescale_noise_cfg` takes mean / std over the C * len valid elements, and the input assembly substitutes zeros for padded frames:
 * what the caller leaves there -- NaN included -- is ignored.  Frames >= len of ezdit_forward's output and of the sampler's latents
 * are written as exactly 0.  Padded token rows are still computed (and discarded) by the per-row kernels.
 * A run-time table of the step (contract above), bind-scoped.
 * EZDIT_E_INVALID: a length outside [1, L], n not dividing B.  EZDIT_E_UNSUPPORTED: a ControlNet handle, a backbone with a ControlNet
 * attached (this call can set one of the two tables that must agree: the pair has ezdit_sampler_set_pair_lengths below; clearing with
 * NULL is allowed on either handle); ezdit_forward with cn_skips refuses likewise while lengths are set (the caller's residuals come
 * from a condition embed whose convolutions have a boundary of their own).  ezdit_sampler_begin checks that both rows of a CFG pair
 * have the same length. */
int ezdit_set_lengths(ezdit_handle* h, const int32_t* lengths, int n, ezdit_stream stream);

/* ---- the denoiser operator: MaskDiT.forward / UDiT.forward ----------------------------------- */
/* src/models/conditioners.py:156-183 (in_ch = C: x [x_rows,C,L], optional gt/gt_mask [x_rows,C,L];
 * batch row b reads latent row b % x_rows, which is how the CFG pair shares one latent,
 * src/inference.py:75) or src/models/udit.py:281-362 directly (in_ch = 2C+1: x is the assembled
 * [B,257,L] input, as src/inference_controlnet.py:97-99 calls unet.model).
 * cn_skips: optional n_cn device pointers to fp32 [B,L,D] ControlNet residuals in the reference's
 * list order (popped from the end, udit.py:345-348), each already multiplied by conditioning_scale.
 * out: fp32 [B,C,L]. */
int ezdit_forward(ezdit_handle* h, const float* dev_x, int in_ch, int x_rows,
                  const float* dev_gt, const uint8_t* dev_gt_mask,
                  const float* const* cn_skips, int n_cn,
                  float* dev_out, ezdit_stream stream);

/* ---- ControlNet (handle created with cfg.controlnet = 1) ------------------------------------------------ */
/* DiTControlNetEmbed (controlnet.py:65-84) on the control signal, hoisted out of the step loop (it depends on the
 * condition only): cond fp32 [B, cond_in, Lcond] with Lcond = 2 L (the embed has one stride-2 conv).  With the lengths of an attached
 * pair set (ezdit_sampler_set_pair_lengths) Lcond is still 2 L, the padded form, and each sample's boundary sits at 2 len_b. */
int ezdit_prepare_condition(ezdit_handle* cn, const float* dev_cond, int Lcond, ezdit_stream stream);
/* DiTControlNet.forward (controlnet.py:252-315): x as in ezdit_forward (in_ch = C needs `dev_mask_embed`, the [C] fp32
 * mask_embed of the MaskDiT that assembles the input, conditioners.py:161-176); the depth/2 residuals
 * zero_linear_i(skip_i) land in the ControlNet workspace.  They are NOT yet multiplied by conditioning_scale. */
int ezdit_controlnet_forward(ezdit_handle* cn, const float* dev_x, int in_ch, int x_rows, const float* dev_gt,
                             const uint8_t* dev_gt_mask, const float* dev_mask_embed, ezdit_stream stream);
/* pointers to the residuals of the last ezdit_controlnet_forward, in the reference's list order (out[i] <-> skip i) */
int ezdit_controlnet_residuals(ezdit_handle* cn, const float** out, int n);
/* the backbone's sampler then runs ControlNet + backbone per step (src/inference_controlnet.py:89-99) */
int ezdit_sampler_attach_controlnet(ezdit_handle* h, ezdit_handle* cn, float conditioning_scale);
/* scale applied to cn_skips inside ezdit_forward (default 1.0: residuals already scaled by the caller, as DiTControlNet.forward
 * returns them).  Independent of the conditioning_scale of a ControlNet attached to the fused sampler. */
int ezdit_set_cn_scale(ezdit_handle* h, float scale);

/* ---- batched ControlNet: per-sample lengths and conditioning scales of an ATTACHED pair ------------------------------------- */
/* ezdit_set_lengths for a backbone `h` with a ControlNet attached, both bound to the same (B, L): the same validation (HOST array,
 * 1 <= lengths[i] <= L, n divides B, batch row b reads lengths[b % n]), the table uploaded to BOTH handles; NULL or n = 0 clears both.
 * With the table on, ezdit_prepare_condition still takes the padded [B, cond_in, 2 L] condition, but batch element b is its own
 * [cond_in, 2 len_b] signal: every layer of the embed reads zero at and beyond its valid input length (2 len_b; len_b behind the
 * stride-2 layer) whatever the buffer holds -- NaN included -- and writes zero at and beyond its valid output length, so rows
 * [0, len_b) of the embed are what that sample's own condition gives and the rows beyond are exactly 0.  ezdit_controlnet_forward
 * and the fused sampler's ControlNet branch then run on the table as the backbone does (input assembly, self-attention keys); the
 * residuals of padded rows are finite and read by nobody.
 * The embed is computed from the table: setting another table, or clearing one, invalidates it -- ezdit_controlnet_forward and
 * ezdit_sampler_run return EZDIT_E_STATE until ezdit_prepare_condition has run again.  ezdit_sampler_run also returns EZDIT_E_STATE,
 * naming the mismatch, when the two handles' tables differ (one of them cleared or re-bound behind the pair's back).
 * Detaching (ezdit_sampler_attach_controlnet(h, NULL, ..)) or destroying the backbone clears the ControlNet's table and leaves the
 * backbone's; destroying either handle leaves the other usable.
 * Two run-time tables of the step (contract above), bind-scoped.  EZDIT_E_STATE also without an attached ControlNet, or when the two
 * handles are bound to different (B, L).  EZDIT_E_INVALID as ezdit_set_lengths. */
int ezdit_sampler_set_pair_lengths(ezdit_handle* h, const int32_t* lengths, int n, ezdit_stream stream);
/* conditioning_scale per sample of the fused sampler: `scales` is a HOST array of n floats, n divides B, batch row b multiplies the
 * attached ControlNet's residuals by scales[b % n] (the rule of the lengths: the CFG pair of a sample shares its scale) instead of the
 * scalar of ezdit_sampler_attach_controlnet; NULL or n = 0 goes back to that scalar.  The table lives at the end of the workspace
 * (ezdit_workspace_bytes grows by 1 KB) and is read by the row kernel once per token row.  ezdit_forward with caller-provided residuals
 * never reads it (ezdit_set_cn_scale is its scale).
 * A run-time table of the step (contract above), bind-scoped.  EZDIT_E_STATE also without an attached ControlNet.
 * EZDIT_E_INVALID: n not dividing B, a non-finite value. */
int ezdit_sampler_set_cn_scales(ezdit_handle* h, const float* scales, int n, ezdit_stream stream);

/* ---- sampler: CFG + rescale + DDIM, src/inference.py:70-100 + diffusers DDIMScheduler.step ---- */
typedef struct {
    float sa, sb;      /* sqrt(alpha_bar_t), sqrt(1 - alpha_bar_t) */
    float c_x0, c_dir; /* sqrt(alpha_bar_prev), sqrt(1 - alpha_bar_prev - sigma^2) */
    float sigma;       /* eta * sqrt(variance) */
} ezdit_ddim_coef;

/* ONE stand-alone CFG + guidance-rescale + DDIM update (src/inference.py:88-100 `rescale_noise_cfg` + `scheduler.step`), for
 * callers that keep their own Python loop: dev_pred fp32 [2P][n] (rows [0,P) conditional, [P,2P) unconditional; [P][n] when
 * guidance_scale <= 0), dev_latents fp32 [P][n] updated in place, dev_noise fp32 [P][n] for THIS step or NULL, coef by value
 * (host), n = C*L elements per sample, dev_scratch >= P*256 floats (needed when guidance_rescale > 0).  No handle needed. */
int ezdit_cfg_ddim_step(const float* dev_pred, float* dev_latents, const float* dev_noise, const ezdit_ddim_coef* coef,
                        float guidance_scale, float guidance_rescale, int P, int n, float* dev_scratch, ezdit_stream stream);

/* dev_latents fp32 [P,C,L] is updated in place each step; dev_noise fp32 [n_steps,P,C,L] or NULL
 * (eta == 0); coefs is a HOST array of n_steps entries (copied into the workspace);
 * guidance_scale <= 0 disables CFG (B = P, src/inference.py:94-96), otherwise B = 2P with rows
 * [0,P) conditional and [P,2P) unconditional.  gt/gt_mask as in ezdit_forward (editing). */
int ezdit_sampler_begin(ezdit_handle* h, float* dev_latents, int P, const float* dev_noise,
                        const ezdit_ddim_coef* coefs, int n_steps,
                        float guidance_scale, float guidance_rescale,
                        const float* dev_gt, const uint8_t* dev_gt_mask, ezdit_stream stream);
/* run `n` consecutive steps from the current step counter; use_graph != 0 captures one step into a
 * hipGraph on first use and replays it (no host work between kernels).  Running past the prepared steps (n_steps of
 * ezdit_sampler_begin / n of ezdit_prepare_timesteps) is refused with EZDIT_E_STATE; ezdit_set_step rewinds. */
int ezdit_sampler_run(ezdit_handle* h, int n, int use_graph, ezdit_stream stream);

/* ---- per-sample sampler settings: guidance_scale, guidance_rescale and eta per prompt of ONE batched call ------------------- */
/* After ezdit_sampler_begin, sample p of the call takes guidance_scale[p], guidance_rescale[p] and, at step i, the coefficients
 * coefs[i * P + p] (step-major, n_steps * P entries: each sample's own eta enters through its c_dir and sigma) instead of the call's
 * scalars.  All three are HOST arrays; all three NULL (or P = 0) clears the table: the scalars of ezdit_sampler_begin hold again, bit
 * for bit.  Every sample comes out as the call with that sample alone and its settings would give it (the forward of a row depends
 * on that row only); a table in which every sample holds the call's scalars gives bitwise the latents of the scalar path.
 *   guidance_scale[p] <= 0   sample p has no guidance: v = pred[p], no rescale; its unconditional row pred[P + p] is computed by the
 *                            denoiser (the batch keeps its 2 P rows) but not read by the update -- the reference's `guidance_scale=None`
 *                            run (src/inference.py:94-96) inside a CFG batch
 *   guidance_rescale[p] <= 0 no rescale statistics for sample p
 *   sigma == 0 at a step     sample p draws no noise at that step: its slice of dev_noise is not read (it may hold NaN).  dev_noise of
 *                            ezdit_sampler_begin is NULL only when every sample has eta <= 0
 * Per-sample lengths (ezdit_set_lengths) work together with the table.  The table lives at the END of the workspace and is read by the
 * last two kernels of the step; with the table on both kernels are launched whatever the values are.  A backbone with a ControlNet
 * attached accepts the table.  ezdit_workspace_bytes is at most n_slots * (B / 2 + 1) * 32 + 2048 bytes larger for it: room for
 * B / 2 + 1 samples, the B / 2 of a CFG batch.
 * A run-time table of the step (contract above), call-scoped.
 * EZDIT_E_INVALID: P is not the P of ezdit_sampler_begin; only some of the arrays given; a non-finite value; guidance_scale[p] > 0 on a
 * sampler begun without CFG rows (B == P); sigma != 0 on a sampler begun without noise.  EZDIT_E_UNSUPPORTED: P > B / 2 + 1 (a batch
 * begun without CFG rows of more than two samples). */
int ezdit_sampler_set_sample_params(ezdit_handle* h, const float* guidance_scale, const float* guidance_rescale,
                                    const ezdit_ddim_coef* coefs, int P, ezdit_stream stream);

/* The per-sample form of ezdit_cfg_ddim_step, for callers that keep their own loop: dev_params fp32 [P][8] ON THE DEVICE holds
 * (guidance_scale, guidance_rescale, sa, sb, c_x0, c_dir, sigma, 0) of each sample, with the rules above.  dev_pred is fp32 [2P][n]
 * always, dev_noise fp32 [P][n] for this step or NULL, dev_scratch >= P*256 floats (always needed).  dev_lens (nullable, device,
 * int32 [P]): sample p is valid on frames [0, dev_lens[p]) of its L (L divides n), as ezdit_set_lengths; 1 <= dev_lens[p] <= L is
 * the caller's to guarantee (no value makes the kernels touch memory outside the P * n elements).  Asynchronous, no handle needed. */
int ezdit_cfg_ddim_step_per_sample(const float* dev_pred, float* dev_latents, const float* dev_noise, const float* dev_params,
                                   const int32_t* dev_lens, int L, int P, int n, float* dev_scratch, ezdit_stream stream);

/* ---- multistep solver: DPM-Solver++(2M) in the fused sampler step ------------------------------------------------------------- */
/* For v-prediction the DDIM update at eta = 0 is first-order DPM-Solver++; the 2M solver adds one term in the data prediction of the
 * step before:   x0_i = sa x - sb v,  eps_i = sa v + sb x  (as ezdit_ddim_coef),   x_next = c_x0 x0_i + c_dir eps_i + c_hist_i (x0_i - x0_{i-1}).
 * After ezdit_sampler_begin, c_hist is a HOST array of n_steps values (the n_steps of
 * ezdit_sampler_begin; ezaudio_amd/scheduler.py multistep_coefficients) and dev_x0_hist a caller-owned fp32 [P][C][L] device buffer that
 * must live as long as the sampler runs: the last kernel of every step reads x0_{i-1} from it and writes x0_i back (0 on the padded
 * frames of ezdit_set_lengths).  c_hist NULL switches it off: the DDIM step again, bit for bit.
 *   c_hist_i == 0     step i is first-order and does NOT read the history: the buffer may hold anything (NaN included) when the run
 *                     starts, c_hist_0 being 0 by construction.  The history is still written.
 * The values go into a spare slot of the coefficient rows already in the workspace (ezdit_workspace_bytes is unchanged); the history
 * buffer is a kernel argument.  c_hist
 * depends on the schedule only, so with a per-sample table (ezdit_sampler_set_sample_params) every sample takes the call's c_hist_i;
 * per-sample lengths, per-sample guidance and rescale, editing (gt / gt_mask) and an attached ControlNet work unchanged.
 * A run-time table of the step (contract above), call-scoped.  While it is on, ezdit_set_step(k) with k != 0 is refused with EZDIT_E_STATE (the
 * history would not be step k - 1's; k = 0 is fine, c_hist_0 = 0).  With a start table (ezdit_sampler_set_start) the one accepted k is min(start_steps)
 * instead: that step is first-order for every sample active at it.
 * EZDIT_E_INVALID: n_steps is not the sampler's; a non-finite value; c_hist without dev_x0_hist; a sampler begun with noise, or a
 * per-sample table with any sigma != 0 (the solver is deterministic; ezdit_sampler_set_sample_params in turn refuses sigma != 0 while
 * the solver is on). */
int ezdit_sampler_set_multistep(ezdit_handle* h, const float* c_hist, int n_steps, float* dev_x0_hist, ezdit_stream stream);

/* The multistep form of ezdit_cfg_ddim_step_per_sample, for callers that keep their own loop: dev_params[p][7], the spare zero of that
 * operator, is c_hist of sample p; dev_x0_hist fp32 [P][n] holds x0 of the step before and is rewritten with this step's (0 on padded
 * frames; not read for a sample whose c_hist is 0).  Guidance, rescale and dev_lens as there; no noise (sigma, dev_params[p][6], is
 * not applied).  dev_scratch >= P*256 floats.  Asynchronous, no handle needed. */
int ezdit_cfg_multistep_step(const float* dev_pred, float* dev_latents, float* dev_x0_hist, const float* dev_params,
                             const int32_t* dev_lens, int L, int P, int n, float* dev_scratch, ezdit_stream stream);

/* ---- composed guidance: K weighted prompts per sample in the fused step ---------------------------------------------------------- */
/* Several conditions per sample, each guided with its own weight against ONE shared unconditional row (the AND of "Compositional Visual Generation with
 * Composable Diffusion Models", Liu et al. 2022).  Sample p of P carries K conditions (1 <= K <= EZDIT_COMPOSE_MAX) with the weights w[p][0 .. K-1]:
 *   batch rows   [c_0 (P rows) | c_1 (P rows) | ... | c_{K-1} (P rows) | u (P rows)], B = (K + 1) P: row k P + p is condition k of sample p, row K P + p its
 *                unconditional row.  K = 1 is the layout of ezdit_sampler_begin.  Batch row b reads latent row b % P and length b % P, as always.
 *   combination  in fp32, k ascending:  d = w_0 (c_0 - u);  d += w_k (c_k - u) for k = 1 .. K-1;  v = u + g_p d, g_p the sample's guidance_scale (the call's
 *                scalar or its row of ezdit_sampler_set_sample_params).  Everything behind v is the step as it is without composition: rescale, x0 / eps,
 *                the DDIM or 2M update, noise, history, padded frames, held samples.
 *   rescale      the reference is the PRIMARY condition: ratio = std(c_0) / std(v), unbiased, over the sample's valid elements
 *   weights      w[p][0] finite and > 0; the others any finite value.  A negative weight steers away from its prompt and keeps the empty-prompt baseline.
 *                A weight of exactly 0: row k P + p is computed by the denoiser (the batch keeps its shape) but NOT read by the update -- how a sample
 *                with fewer prompts than K sits in a batch.  A sample with g_p <= 0 reads c_0 alone.
 *   identity     K = 1 with w = 1 gives the bits of the call without composition.
 * ezdit_sampler_begin_composed takes the arguments of ezdit_sampler_begin plus K and the HOST array weights [P][K].  The weights are a run-time table of
 * the step (contract above), call-scoped, in a workspace region of their own (B floats; ezdit_workspace_bytes grows by 256 .. 1024 bytes): one captured step
 * serves every set of values, which ezdit_sampler_set_compose_weights replaces (same P and K, the same rules for the values; it cannot switch composition on
 * or change K -- that is another batch layout, so another begin).  With NULL (or P = 0) it switches composition off: a call of K = 1 goes on as the plain call,
 * one of K > 1 ENDS there (its batch has no plain reading: ezdit_sampler_run returns EZDIT_E_STATE until the next begin) -- what a caller does before it
 * attaches a ControlNet or sets context weights on a handle whose last call was composed.  ezdit_sampler_begin itself is unchanged and begins a call
 * without composition.
 * Per-sample lengths, per-sample settings, the multistep solver, a start table, gt / gt_mask and an attention window work unchanged.
 * EZDIT_E_INVALID: guidance_scale <= 0 (composition is guidance); K outside [1, EZDIT_COMPOSE_MAX]; B != (K + 1) P; a non-finite weight; w[p][0] <= 0;
 * lengths that differ between the K + 1 rows of a sample; P or K of the setter that are not the call's.  EZDIT_E_UNSUPPORTED: an attached ControlNet,
 * context weights that are on; ezdit_sampler_attach_controlnet, ezdit_set_context_weights and the canvas setters refuse likewise while composition is on.
 * EZDIT_E_STATE: ezdit_sampler_set_compose_weights on a call that was not begun composed. */
#define EZDIT_COMPOSE_MAX 8
int ezdit_sampler_begin_composed(ezdit_handle* h, float* dev_latents, int P, const float* dev_noise,
                                 const ezdit_ddim_coef* coefs, int n_steps,
                                 float guidance_scale, float guidance_rescale,
                                 const float* dev_gt, const uint8_t* dev_gt_mask, int K, const float* weights, ezdit_stream stream);
int ezdit_sampler_set_compose_weights(ezdit_handle* h, const float* weights, int P, int K, ezdit_stream stream);

/* The composed form of ezdit_cfg_ddim_step_per_sample / ezdit_cfg_multistep_step, for callers that keep their own loop: dev_pred fp32 [(K + 1) P][n] in
 * the row order above, dev_weights fp32 [P][K] ON THE DEVICE (the caller guarantees the rules for the values; no value makes the kernels touch memory
 * outside the (K + 1) P n elements), dev_params [P][8] = (guidance_scale, guidance_rescale, sa, sb, c_x0, c_dir, sigma, c_hist) as there.  dev_x0_hist NULL:
 * the DDIM form (dev_noise [P][n] of this step, or NULL); given: the multistep form (dev_noise must be NULL).  dev_lens, L, dev_scratch (>= P*256 floats,
 * always needed) as there.  Asynchronous, no handle needed.  EZDIT_E_INVALID: a NULL pointer among pred, latents, params, weights, scratch; K outside
 * [1, EZDIT_COMPOSE_MAX]; P < 1, n < 2; L not dividing n with dev_lens; noise together with a history. */
int ezdit_cfg_compose_step(const float* dev_pred, float* dev_latents, const float* dev_noise, float* dev_x0_hist, const float* dev_params,
                           const float* dev_weights, int K, const int32_t* dev_lens, int L, int P, int n, float* dev_scratch, ezdit_stream stream);

/* ---- adaptive projected guidance (APG) in the fused step ------------------------------------------------------------------------- */
/* Sadat et al., "Eliminating Oversaturation and Artifacts of High Guidance Scales in Diffusion Models": guidance on the DATA prediction with a capped norm, a
 * momentum across steps and the component parallel to the conditional prediction removed (or scaled by eta_apg).  Per sample, over its valid elements only,
 * with w the sample's guidance_scale (the call's scalar or its row of ezdit_sampler_set_sample_params) and (sa, sb, ...) its ezdit_ddim_coef of the step:
 *   x0c = sa x - sb c ;  d = sb (u - c) + beta_eff m ;  m <- d   (stored before the cap)
 *   s = min(1, r / |d|) if r > 0 and |d| > 0, else 1 ;  a = s <d, x0c> / |x0c|^2   (0 when |x0c|^2 = 0)
 *   U = s d - (1 - eta_apg) a x0c ;  x0 = x0c + (w - 1) U ;  v = c - (w - 1) U / sb ;  eps = sa v + sb x
 *   x_next = c_x0 x0 + c_dir eps (+ sigma z) (+ c_hist (x0 - x0_hist), x0_hist <- x0 with the multistep solver)
 * The element-wise arithmetic is fp32; the three sums are 64 chunked fp32 partial sums per sample added up in double, s and a are formed in double.
 * beta_eff is the sample's momentum, and 0 at the sample's own first step (step 0, or start_steps[p] with a start table): there the momentum buffer is not
 * read and may hold anything, NaN included.  eta_apg = 1, r = 0, momentum = 0 is plain classifier-free guidance (to rounding).
 * ezdit_sampler_set_apg takes HOST arrays of P values -- eta_apg, norm_threshold (r; 0 = no cap), momentum, on -- and dev_momentum, a caller-owned fp32
 * [P][C][L] device buffer that must live as long as the sampler runs: the last kernel of every step rewrites the rows of the APG samples with d (0 on the
 * padded frames of ezdit_set_lengths).  A sample with on = 0 takes classifier-free guidance and guidance_rescale exactly as without the table; a sample with
 * guidance_scale <= 0 takes its conditional prediction alone; the momentum rows of either are neither read nor written, nor are those of a sample the start
 * table holds.  guidance_rescale is NOT applied to an APG sample.
 * A run-time table of the step (contract above), call-scoped, in a workspace region of its own: ezdit_workspace_bytes grows by 16 B bytes, rounded up to a
 * multiple of 256.  All four arrays NULL (or P = 0) switches it off: the plain step again, bit for bit.  While it is on both tail kernels of the step are launched
 * (the plain step at guidance_rescale 0 launches one).  ezdit_set_step(k) follows the multistep rule while it is on: only k = 0, or min(start_steps) with a start
 * table, else EZDIT_E_STATE (the momentum would not be step k - 1's).
 * Per-sample lengths, the per-sample settings table, the multistep solver, a start table, step noise, gt / gt_mask, an attached ControlNet, an attention
 * window, context weights and token weights work unchanged; none of them is touched.
 * EZDIT_E_UNSUPPORTED: a call begun composed (ezdit_sampler_begin_composed; a begin ends the table, so the other direction cannot arise), a canvas or a ring
 * that is on -- and the canvas setters refuse likewise while the table is on.  EZDIT_E_INVALID: P is not the sampler's; only some of the arrays, or no
 * dev_momentum; a non-finite value; norm_threshold < 0; on != 0 on a sampler begun without CFG rows (B = P). */
int ezdit_sampler_set_apg(ezdit_handle* h, const float* eta_apg, const float* norm_threshold, const float* momentum, const int32_t* on, int P,
                          float* dev_momentum, ezdit_stream stream);

/* The APG form of ezdit_cfg_ddim_step_per_sample / ezdit_cfg_multistep_step, for callers that keep their own loop: dev_pred fp32 [2 P][n], dev_params fp32
 * [P][12] ON THE DEVICE = (guidance_scale, guidance_rescale, sa, sb, c_x0, c_dir, sigma, c_hist, eta_apg, norm_threshold, beta_eff, on) -- beta_eff is the
 * momentum this step applies (the caller passes 0 at a sample's first step; dev_momentum is not read then) --, dev_momentum fp32 [P][n] rewritten as above.
 * dev_x0_hist NULL: the DDIM form (dev_noise [P][n] of this step, or NULL; c_hist is not applied); given: the multistep form (dev_noise must be NULL).
 * dev_lens, L, dev_scratch (>= P*256 floats, always needed) as there.  Asynchronous, no handle needed.  EZDIT_E_INVALID: a NULL pointer among pred, latents,
 * momentum, params, scratch; P < 1, n < 2; L not dividing n with dev_lens; noise together with a history. */
int ezdit_cfg_apg_step(const float* dev_pred, float* dev_latents, const float* dev_noise, float* dev_x0_hist, float* dev_momentum, const float* dev_params,
                       const int32_t* dev_lens, int L, int P, int n, float* dev_scratch, ezdit_stream stream);

/* ---- audio-to-audio: start the sampler from a noised clip, per sample ------------------------------------------------------------ */
/* Noise a clean VAE latent into the model's space at each sample's start step, in place of the init noise:
 *   dev_latents[p][i] = sa_p * ((dev_clean[p][i] + shift) * scale) + sb_p * dev_latents[p][i]
 * dev_latents fp32 [P][n] holds the init noise on entry; dev_clean fp32 [P][n] is the encoder's output, `(x + shift) * scale` the
 * reference's `scale_shift` (src/utils/utils.py:20-21) in that order; dev_params fp32 [P][2] ON THE DEVICE holds (sa, sb) =
 * (sqrt(alpha_bar), sqrt(1 - alpha_bar)) of sample p's start step (the first two slots of its ezdit_ddim_coef row).  dev_lens
 * (nullable, device, int32 [P]) as in ezdit_cfg_ddim_step_per_sample: frames >= dev_lens[p] of the L (n = C L) are written as exactly
 * 0 whatever dev_clean and dev_latents hold there, NaN included.
 *   (sa_p, sb_p) exactly (0, 1)   sample p is not touched and its dev_clean row is not read: start step 0 of a zero-terminal-SNR
 *                                 schedule, the plain text-to-audio call bit for bit
 * Asynchronous, no handle needed.  EZDIT_E_INVALID: dev_clean, dev_latents or dev_params NULL; P or n < 1; L < 1 or L not dividing n
 * (with or without dev_lens). */
int ezdit_add_noise(const float* dev_clean, float* dev_latents, const float* dev_params, float scale, float shift,
                    const int32_t* dev_lens, int L, int P, int n, ezdit_stream stream);

/* After ezdit_sampler_begin, sample p's first step is start_steps[p] (HOST array of P values in [0, n_steps)) instead of 0; the device
 * step counter and the host's count of steps done are set to min(start_steps), so ezdit_sampler_run(n) is bounded by n_steps minus
 * that.  While the step counter is below start_steps[p] sample p is HELD: the denoiser computes its rows (the batch keeps its shape,
 * as padded frames are computed) and the last two kernels of the step skip it -- no read of its prediction, noise slice or history,
 * no write of its latents or history: the latents keep their bits.  From start_steps[p] on it is updated as in a run that begins
 * there alone; with the multistep solver on, step start_steps[p] is first-order for it (c_hist = 0, the history is written, not read).
 * NULL or P = 0 clears the table (and, if it was on, puts the step counter back to 0).
 * The table lives at the END of the workspace (ezdit_workspace_bytes grows by 1 KB).  Per-sample lengths (plain and pair), the per-sample settings table, the
 * multistep solver (set in either order with it), gt / gt_mask and an attached ControlNet work unchanged; none of them is touched.
 * While the table is on, ezdit_set_step(k) is accepted only for k == min(start_steps) -- a rewind to the run's own beginning, also with
 * the multistep solver on (that step is first-order for every sample active at it); any other k is EZDIT_E_STATE.  With it off
 * ezdit_set_step keeps its rules.
 * A run-time table of the step (contract above), call-scoped.  EZDIT_E_INVALID: P is not the P of ezdit_sampler_begin; a value outside
 * [0, n_steps). */
int ezdit_sampler_set_start(ezdit_handle* h, const int32_t* start_steps, int P, ezdit_stream stream);

/* ---- long-form canvas: the P samples of one call are overlapping windows of one long latent, blended inside the step ------------------- */
/* MultiDiffusion-style sampling of a clip longer than the trained length: a canvas of T frames is covered by P windows of L frames, window p
 * holding the canvas frames [dev_offsets[p], dev_offsets[p] + L).  The operator averages, in place, every canvas frame that two or more
 * windows hold:   v = sum_p w_p x_p / sum_p w_p,   w_p = min(r + 1, L - r, ramp) at window p's local frame r = j - dev_offsets[p],
 * in fp32 over the holders in ascending p, and stores the same v into every holder: the aliases are bit-identical afterwards and the result
 * does not depend on scheduling.  ramp 1 is the plain mean, ramp = the overlap a linear cross-fade.  An element held by ONE window is neither
 * read nor written (it may hold NaN); a table without overlap leaves the buffer bitwise untouched.
 * dev_latents fp32 [P][C][L], dev_offsets int32 [P] ON THE DEVICE (ascending, first 0, no gap, last + L == T: the caller's to guarantee -- no
 * value makes the kernel touch memory outside the P * C * L elements).  Asynchronous, no handle needed.
 * EZDIT_E_INVALID: a NULL pointer; P, C or L < 1; ramp < 1; T outside [L, P * L] (what no table can give). */
int ezdit_canvas_blend(float* dev_latents, const int32_t* dev_offsets, int P, int C, int L, int T, int ramp, ezdit_stream stream);

/* After ezdit_sampler_begin, the P samples of the call are the windows of a canvas of T frames: `offsets` is a HOST array of P first frames.
 * While the table is on, every step ends with ezdit_canvas_blend on the updated latents (one more kernel behind the update, on the same
 * stream: one more node of the captured step), so the windows agree on their shared frames after every step and the canvas can be read off
 * the windows when the run ends.  While off the step issues exactly the launches it issues without this call.  The table lives at the
 * END of the workspace (ezdit_workspace_bytes grows by 1 KB); T and the ramp are kernel arguments.
 * The per-sample settings table and the multistep solver work with it (the blend acts on the updated latents; the history of data
 * predictions stays per window and is not blended).
 * A run-time table of the step (contract above), call-scoped.  EZDIT_E_INVALID unless P is the P of ezdit_sampler_begin, offsets[0] == 0, the offsets ascend strictly,
 * offsets[i + 1] <= offsets[i] + L (no uncovered frame), offsets[P - 1] + L == T and ramp >= 1.  EZDIT_E_UNSUPPORTED with a length table
 * (ezdit_set_lengths), a start table, gt / gt_mask or an attached ControlNet -- long edits, long audio-to-audio and long ControlNet runs
 * are not implemented; while the canvas is on, ezdit_set_lengths, ezdit_sampler_set_start and ezdit_sampler_attach_controlnet (with a
 * ControlNet) are refused the same way. */
int ezdit_sampler_set_canvas(ezdit_handle* h, const int32_t* offsets, int P, int T, int ramp, ezdit_stream stream);

/* ---- seamless loops: the canvas as a ring ------------------------------------------------------------------------------------------------ */
/* The canvas above is a line: its first and last frame know nothing of each other.  Here the T frames are a RING: window p holds the ring
 * frames (dev_offsets[p] + r) mod T for r in [0, L), so the last window runs into the first and every window has both its edges inside a
 * neighbour; a clip decoded from the ring (with wrapped context: ezaudio_amd.sampler.decode_circular) ends where it begins.  L <= T, so a
 * window holds a ring frame at most once.  Everything else is ezdit_canvas_blend: the same weights min(r + 1, L - r, ramp), the fp32 sum over
 * the holders in ascending p, the same v into every holder (bit-identical aliases, across the wrap too), one thread per (c, j), an element
 * with one holder neither read nor written, and no value of the device table makes the kernel touch memory outside the P * C * L elements.
 * With a table whose last window ends exactly at T (no window wraps) the result is ezdit_canvas_blend's bit for bit.
 * Asynchronous, no handle needed.  EZDIT_E_INVALID: a NULL pointer; P, C or L < 1; ramp < 1; L > T; T > P * L (what no table can cover). */
int ezdit_canvas_blend_loop(float* dev_latents, const int32_t* dev_offsets, int P, int C, int L, int T, int ramp, ezdit_stream stream);

/* ezdit_sampler_set_canvas for the ring: while on, every step ends with ezdit_canvas_blend_loop on the updated latents -- one more node of
 * the captured step than the plain step, the same count as the line.  It is the SAME run-time table as ezdit_sampler_set_canvas (the same
 * slot of the workspace: ezdit_workspace_bytes does not grow): the two setters replace each other (line <-> ring is another kernel and
 * drops the graph), NULL or P = 0 on either switches the table off, ezdit_sampler_begin clears it.  The per-sample settings table and the
 * multistep solver work with it; the multistep history stays per window.
 * EZDIT_E_INVALID unless P is the P of ezdit_sampler_begin, L <= T, offsets[0] == 0, the offsets ascend strictly, offsets[i + 1] <=
 * offsets[i] + L, offsets[P - 1] < T, offsets[P - 1] + L >= T (no gap at the wrap) and ramp >= 1.  EZDIT_E_STATE and EZDIT_E_UNSUPPORTED
 * as ezdit_sampler_set_canvas: not with a length table, a start table, gt / gt_mask or an attached ControlNet, and those four are refused
 * while the ring is on.  Audio quality on the real checkpoints (whether the seam is audible, the choice of overlap and ramp) is unmeasured. */
int ezdit_sampler_set_canvas_loop(ezdit_handle* h, const int32_t* offsets, int P, int T, int ramp, ezdit_stream stream);

/* ---- Oobleck VAE decoder building blocks (src/modules/stable_vae/models/autoencoders.py:38-61,82-113,149-190) --------
 * Stateless ops on caller-owned device buffers; the layer sequence is host code (ezaudio_amd/vae.py), run once per call.
 * Activations are token-major [L][C] with zero halo rows so that convolutions are GEMMs over shifted rows. */
/* out fp32 [M][ldo] = A[M][K] . W[N][K]^T (+ bias[N]) (+ resid[M][ldr]); K tile t (64 wide) of A is read at byte offset
 * (t / conv_cpb) * conv_tap_bytes + (t % conv_cpb) * 128 (conv_cpb = 0: plain GEMM).  A, W bf16.  `tile` is a configuration id of csrc/gemm.hip.
 * Refused before anything is read or launched (the message of ezdit_last_error names the argument):
 *   EZDIT_E_UNSUPPORTED  a tile id that is no configuration; conv_cpb != 0 on a tile other than 6, 9, 13, 25 (only the lockstep kernel implements the
 *                        conv addressing: 60, 61, 62, 66, 70, 72, 73 would run a plain GEMM over K * 2 bytes of each row); dev_resid on tile 70, 72, 73
 *                        (the K-split kernel's fp32 epilogue adds none; 6, 9, 13, 25, 60, 61, 62, 66 do)
 *   EZDIT_E_INVALID      M or N <= 0; K not a positive multiple of 64; N not a multiple of 4; lda, ldw or conv_cpb < 0; wrows <= 0; conv_tap_bytes not a
 *                        multiple of 16; (M - 1) lda plus the furthest tap's reach (conv_cpb = 0: plus K), or (wrows - 1) ldw + K, at or above 2^31
 *                        elements -- the kernels stage A and W through 32-bit offsets
 * The other four ops return EZDIT_E_INVALID for L, T, C or latent_dim <= 0 (and C not a multiple of 4; 8 for ezvae_conv_out1). */
int ezvae_gemm(const void* dev_a, int lda, const void* dev_w, int ldw, int wrows, const float* dev_bias, const float* dev_resid,
               int ldr, float* dev_out, int ldo, int M, int N, int K, int conv_cpb, long conv_tap_bytes, int tile,
               ezdit_stream stream);
/* SnakeBeta (models/blocks.py:317-358) fused with the fp32 -> bf16 cast: out = x + inv_beta * sin(alpha x)^2; alpha NULL = cast only */
int ezvae_snake_bf16(const float* dev_x, int ldx, const float* dev_alpha, const float* dev_inv_beta, void* dev_out, int ldo,
                     long L, int C, ezdit_stream stream);
/* final WNConv1d(C -> 1, k 7, pad 3, no bias): xb bf16 haloed (row 0 = position -3), w fp32 [7][C] -> out fp32 [L] */
int ezvae_conv_out1(const void* dev_xb, int ldx, const float* dev_w, float* dev_out, long L, int C, ezdit_stream stream);

/* encoder input WNConv1d(1 -> C, k 7, pad 3) (autoencoders.py:130-132): wav fp32 [T], w fp32 [7][C], bias [C] -> out fp32 [T][C] */
int ezvae_conv_in1(const float* dev_wav, const float* dev_w, const float* dev_bias, float* dev_out, long T, int C, ezdit_stream stream);
/* VAEBottleneck.encode (models/bottleneck.py:67-71,77-87): enc fp32 [L][2*latent] token-major (mean | scale), noise fp32
 * [latent][L] (caller's randn; NULL = return the mean) -> z fp32 [latent][L] = noise * (softplus(scale) + 1e-4) + mean */
int ezvae_sample(const float* dev_enc, const float* dev_noise, float* dev_z, int L, int latent_dim, ezdit_stream stream);

/* ---- segment forms of the four ops: B samples stacked along the token axis, zero rows between them, so that every conv of a ragged batch stays ONE ezvae_gemm ------
 * Sample b lies on rows [b * stride, b * stride + len_b) of a level; len_b = dev_lens[b] * mul / div (integer division; dev_lens: one int32 [B] device table per call --
 * the decoder multiplies by its strides so far, the encoder divides, and a chain of floors equals one floor by the product).  Values outside an interior (padding,
 * the rows a GEMM computed inside a gap) are never read, so they may be NaN.  EZDIT_E_INVALID for rows, W, Lmax, C, B, mul, div or a stride <= 0, a NULL table, C not a
 * multiple of 4 (8 for conv_out1), or more blocks than one launch holds. */
/* every row r < rows of the launch is written: bf16(snake(x[b * stride_in + l])) with b = r / stride_out, l = r % stride_out where b < B and l < len_b, ZERO elsewhere
 * (the gap rows are written, not assumed: a cached buffer may hold an earlier call's interiors there).  stride_in != stride_out: the first layer reads the un-gapped input. */
int ezvae_snake_bf16_seg(const float* dev_x, int ldx, const float* dev_alpha, const float* dev_inv_beta, void* dev_out, int ldo, long rows, int C,
                         const int32_t* dev_lens, int B, long mul, long div, long stride_in, long stride_out, ezdit_stream stream);
/* ezvae_conv_out1 on the stacked haloed sequence (row b * stride_in = sample b's position -3): out fp32 [B][W], out[b][l] for l < len_b, zero up to W */
int ezvae_conv_out1_seg(const void* dev_xb, int ldx, const float* dev_w, float* dev_out, long W, int C, const int32_t* dev_lens, int B, long mul, long div,
                        long stride_in, ezdit_stream stream);
/* ezvae_conv_in1 on wav fp32 [B][Tmax] with sample b's own bound dev_lens[b]: out fp32 [rows][C] stacked with stride_out rows per sample, zero rows in the gaps */
int ezvae_conv_in1_seg(const float* dev_wav, const float* dev_w, const float* dev_bias, float* dev_out, long rows, int C, const int32_t* dev_lens, int B,
                       long Tmax, long stride_out, ezdit_stream stream);
/* ezvae_sample on enc stacked (frame l of sample b = row b * stride_enc + l), noise (or NULL) and z fp32 [B][latent][Lmax]; z is zero beyond len_b */
int ezvae_sample_seg(const float* dev_enc, const float* dev_noise, float* dev_z, int Lmax, int latent_dim, const int32_t* dev_lens, int B, long mul, long div,
                     long stride_enc, ezdit_stream stream);

/* ---- unit-test hooks: one kernel family each, same code the forward uses ---------------------- */
int ezdit_test_gemm(ezdit_handle* h, int variant, const void* dev_a_bf16, int lda, const void* dev_w_bf16, int ldw,
                    const float* dev_bias, void* dev_out, int ldo, int M, int N, int K, int splitk,
                    ezdit_stream stream);
/* unit-test hook of the un-split residual projection (LayerNorm algebra, producer side; csrc/gemm_ks.h): h_out = h_in + gate * (A . W^T + bias)
 * (fp32 [M][N]; gate NULL = 1, h_in NULL = 0), zu = bf16(h_out * zg) ([M][ld_zu]) and zstat ([ceil(N / cw)][M] float pairs, part-major: sum and
 * sum of squares of each cw-column tile, cw = the kernel's tile width: 96 for tile 70, see csrc/gemm.hip). */
int ezdit_test_resid(int tile, const void* dev_a_bf16, int lda, const void* dev_w_bf16, int ldw, const float* dev_bias, const float* dev_h_in,
                     const float* dev_gate, const float* dev_zg, float* dev_h_out, void* dev_zu_bf16, int ld_zu, void* dev_zstat,
                     int M, int N, int K, ezdit_stream stream);
/* ... and of its two skip-path forms (csrc/common.h GemmArgs COPY2 / ZIN; DESIGN.md "The skip path"): dev_zu2 != NULL -- additionally zu2 = bf16(h_out * zg2) ([M][ld_zu2]; gate and
 * h_in required); dev_zstat_in2 != NULL -- the launch first finishes a LayerNorm over zD columns whose partial statistics come in two part-major sets of zparts parts
 * (dev_zstat_in, dev_zstat_in2: [zparts][M] float pairs): acc := r (acc - mu zG[col]) + bias[col], no gate, no h_in.  dev_h_out NULL = the fp32 stream is not stored. */
int ezdit_test_resid_skip(int tile, const void* dev_a_bf16, int lda, const void* dev_w_bf16, int ldw, const float* dev_bias, const float* dev_h_in,
                          const float* dev_gate, const float* dev_zg, float* dev_h_out, void* dev_zu_bf16, int ld_zu, void* dev_zstat,
                          int M, int N, int K, const float* dev_zg2, void* dev_zu2_bf16, int ld_zu2, const void* dev_zstat_in, const void* dev_zstat_in2,
                          int zparts, int zD, const float* dev_zG, ezdit_stream stream);
/* ... and of its DUAL form (csrc/common.h GemmArgs.zd; tiles 70 and 61; gate and h_in required): the rows OUTSIDE [act_row0, act_row1) additionally get
 * dev_zd[row / rows_per_b] (fp32 [batch elements][zd_stride]) in h_out and the gain dev_zg2 instead of dev_zg in zu; zstat covers h_out as stored. */
int ezdit_test_resid_dual(int tile, const void* dev_a_bf16, int lda, const void* dev_w_bf16, int ldw, const float* dev_bias, const float* dev_h_in,
                          const float* dev_gate, const float* dev_zg, float* dev_h_out, void* dev_zu_bf16, int ld_zu, void* dev_zstat,
                          int M, int N, int K, const float* dev_zd, long zd_stride, const float* dev_zg2, int act_row0, int act_row1, int rows_per_b,
                          ezdit_stream stream);
/* unit-test hook of the LayerNorm algebra's CONSUMER side (csrc/common.h GemmArgs.z*; tiles 60, 61, 66, 67): epi 2 (GEGLU: dev_out bf16 [M][ldo], ldo >= N / 2, W rows and the
 * tables in the interleaved 8 value / 8 gate order) or epi 3 (fused QKV: dev_out unused).  The operand is A' = bf16(x g); the epilogue applies
 * acc := r (acc - mu zG[slot][col]) + zC[slot][col] with (mu, r) of row m merged from dev_zstat_in -- float pairs (sum, sum of squares) [zparts][zs_stride], PART-MAJOR,
 * part p = the columns [p zw, min((p + 1) zw, zD)) of x -- and slot = *dev_cur_step + dev_row_slot[m / rows_per_b] (either NULL = 0); zG, zC fp32 [slots][zt_slot_stride].
 * dev_bias is what the forward passes along (C' already holds it: the consumer form must not add it again).  epi 3: M = B L token rows; q, k bf16 [B][H][Lp][DQK], v bf16
 * [B][H][Lp][DV] (DQK / DV = 64 / 64 or 80 / 96 for head_dim 64 / 72; only rows < L and columns < dh are written); qn / kn: the per-head LayerNorm affine [dh]; rope
 * cos / sin fp32 [>= L][dh / 2] or NULL.  perm 1: N = 3 H dh, W rows packed by EZDIT_T_QKROPE, q and k leave in that column order (two heads per tile); perm 0 with
 * dev_k = dev_v = NULL and no tables: the q-only projection of batched prompts (tile 61, N = H dh, natural order).  epi 3 with dev_zstat_in = NULL: the plain projection
 * (no LayerNorm algebra: the operand is a finished LayerNorm), as the step launches it with zfuse off. */
int ezdit_test_consumer(int tile, int epi, int epi_lds, const void* dev_a_bf16, int lda, const void* dev_w_bf16, int ldw, int w_rows, const float* dev_bias,
                        void* dev_out, int ldo, int M, int N, int K,
                        const void* dev_zstat_in, long zs_stride, int zparts, int zD, int zw, const float* dev_zG, const float* dev_zC, long zt_slot_stride, float zeps,
                        const int* dev_cur_step, const int* dev_row_slot, int rows_per_b,
                        const float* dev_qn_w, const float* dev_qn_b, const float* dev_kn_w, const float* dev_kn_b, const float* dev_rope_cos, const float* dev_rope_sin,
                        void* dev_q, void* dev_k, void* dev_v, int B, int H, int L, int Lp, int dh, int perm, ezdit_stream stream);
/* the RoPE tables of the fused QKV epilogue as ezdit_bind_workspace fills them: cos / sin fp32 [max_len][dh / 2] */
int ezdit_test_rope_table(float* dev_cos, float* dev_sin, int max_len, int dh, ezdit_stream stream);
/* unit-test hook of cross-attention with its own q projection (csrc/attn.hip k_attn<.., ZQ, 32 | 64>; Lkp % 128 == 0): q = LN_head(r (xu . xw_h^T - mu zG) + zC) per head
 * (xu bf16 [batch elements x Lq][ldu] = bf16(x g), xw bf16 [xw_rows][ldw] in nn.Linear layout, xK % 64 == 0, qn affine [dh], zG / zC fp32 [H dh], statistics as above with
 * row = b Lq + query), then softmax(q k^T / sqrt(dh) + mask) v -> dev_out bf16 [batch elements x Lq][ldo].  k bf16 [.][H][Lkp][DQK], v bf16 [.][H][Lkp][DV], kmask [.][Lk].
 * The launch covers the batch elements [b0, b0 + B); every pointer is given for batch element 0.  qtile 32 | 64 | 0 (auto), xk2 0 / 1, xcd_map 0 / 1 as the options. */
int ezdit_test_cross_attention(const void* dev_xu, int ldu, const void* dev_xw, int ldw, int xw_rows, int xK, const float* dev_qn_w, const float* dev_qn_b,
                               const void* dev_k, const void* dev_v, const uint8_t* dev_kmask, void* dev_out, int ldo, int B, int b0, int H, int dh,
                               int Lq, int Lk, int Lqp, int Lkp,
                               const void* dev_zstat_in, long zs_stride, int zparts, int zD, int zw, const float* dev_zG, const float* dev_zC, float zeps,
                               int xk2, int qtile, int xcd_map, ezdit_stream stream);
/* test hook: launches of k_gemm_pp / k_gemm_ks / k_attn record, per workgroup, eight 64-bit shader-clock stamps (kernel start, K-loop
 * start, K-loop end, kernel end, then epilogue internals) into dev_buf ([capacity_workgroups][8] uint64; NULL switches it off).  A launch
 * whose grid exceeds capacity_workgroups writes no stamps.  Un-register (NULL) before freeing the buffer. */
int ezdit_debug_gemm_timestamps(void* dev_buf, long capacity_workgroups);
/* q, k bf16 [B][H][L*p][DQK], v bf16 [B][H][Lkp][DV] (DQK / DV = 64 / 64 or 80 / 96 for head_dim 64 / 72; q and k channels [dh, DQK) zero; rows beyond Lq / Lk and v channels
 * [dh, DV) may hold anything finite), dev_kmask uint8 [B][Lk] or NULL, out bf16 [B*Lq][ldD] (columns [D, ldD) are not written).  Refused with EZDIT_E_INVALID before the
 * first HIP call: a null q, k, v or out, B, Lq or Lk <= 0, Lqp < Lq, Lkp < Lk, Lqp or Lkp no multiple of 64 (the kernel reads whole 64-row query tiles and 32-key sub-tiles
 * unchecked), then a null handle.  With dev_kmask the hook waits for `stream`, reads the mask back and refuses a batch element without a valid key (its softmax is 0 / 0). */
int ezdit_test_attention(ezdit_handle* h, const void* dev_q, const void* dev_k, const void* dev_v,
                         const uint8_t* dev_kmask, void* dev_out, int B, int Lq, int Lk, int Lqp, int Lkp,
                         ezdit_stream stream);
/* ezdit_test_attention over a padded batch (csrc/common.h AttnArgs.klen; Lq == Lk): dev_klen int32 [B] on the DEVICE, 1 <= klen[b] <= Lk (checked: the hook
 * waits for `stream` and reads it back), NULL = ezdit_test_attention.  Batch element b attends to the keys [0, klen[b]); its query rows >= klen[b] come back as zeros. */
int ezdit_test_attention_varlen(ezdit_handle* h, const void* dev_q, const void* dev_k, const void* dev_v,
                                const uint8_t* dev_kmask, void* dev_out, int B, int Lq, int Lk, int Lqp, int Lkp,
                                const int32_t* dev_klen, ezdit_stream stream);
/* unit-test hook of the FinalBlock's Conv1d(C, C, 3, pad 1) (k_final_conv; C % 8 == 0): y fp32 [B * L][ldy] token-major, w fp32 [C][C][3], b fp32 [C] -> out fp32 [B][C][L].
 * dev_lens int32 [B] on the DEVICE or NULL: inputs at frames >= lens[b] read as zero, outputs at frames >= lens[b] are written as zero (checked as above). */
int ezdit_test_final_conv(const float* dev_y, int ldy, const float* dev_w, const float* dev_b, float* dev_out, int B, int C, int L,
                          const int32_t* dev_lens, ezdit_stream stream);
/* unit-test hook of the row operator (csrc/rowops.hip k_row, csrc/rowbody.h k_row_w; the fields are those of csrc/common.h RowArgs, one for one):
 *   h_new = h_in (mode 0) | h_in + gate[slot] * (sum of nsplit slabs + bias) (mode 1) | sum of nsplit slabs + bias (mode 2)        fp32 [M][D] -> h_out (NULL: not stored)
 *   u = LN(h_new) ln_g[slot] + ln_c[slot], or with skip: LN over [h_new | skip + s cn] (width 2 D, ln_g / ln_c of length 2 D)      bf16 [M][ld_u], zero up to ld_u
 * slot = *cur_step + row_slot[row / L] (either NULL = 0), s = cn_tab[row / L] or cn_scale.  Slabs: fp32 or bf16 (part_bf16) [nsplit][part_stride] with rows of ld_part.
 * variant 1 asks for the wave-per-row form (taken up to D = 1280, 4 bf16 slabs or 1 fp32 slab; otherwise the workgroup-per-row form runs), affine its XCD row map.
 * n_slots = the slots the gate / LayerNorm tables hold.  Checked before anything is launched -- EZDIT_E_UNSUPPORTED: D % 4, D > 2048, nsplit > 8; EZDIT_E_INVALID: nsplit < 0,
 * a pointer the mode needs is NULL, ld_u below the written width, ld_u or a stride not a multiple of 4, M / D / L <= 0, cn without skip, skip without u, u without ln_g / ln_c,
 * a misaligned pointer, and (the hook waits for `stream` and reads cur_step / row_slot back) a slot outside [0, n_slots). */
typedef struct ezdit_test_row_args {
    const float* h_in; float* h_out;
    const void* part; int32_t nsplit; int32_t ld_part; int64_t part_stride; int32_t part_bf16; int32_t mode;
    const float* bias; const float* gate; int64_t gate_slot_stride;
    const float* ln_g; const float* ln_c; int64_t ln_slot_stride;
    const float* skip; const float* cn; const float* cn_tab; float cn_scale; int32_t ld_u;
    void* u;
    int32_t M, D, L, n_slots;
    const int32_t* cur_step; const int32_t* row_slot;
    int32_t wt, variant, affine, reserved;
} ezdit_test_row_args;
int ezdit_test_row(const ezdit_test_row_args* args, ezdit_stream stream);
/* unit-test hook of k_headnorm (csrc/rowops.hip): x fp32 [B L][ldx] holds the parts at the columns q_col / k_col / v_col + head * dh (-1 = absent); q, k = per-head
 * LayerNorm with the q / k affine [dh], then the half-split RoPE at position row % L (rope_cos / rope_sin fp32 [>= L][dh / 2], both NULL = no RoPE) -> bf16 [B][H][Lp][DQK];
 * v = bf16(x) -> [B][H][Lp][DV] (DQK / DV = 64 / 64 or 80 / 96).  Only rows < L and channels < dh are written.  EZDIT_E_UNSUPPORTED: dh other than 64 / 72;
 * EZDIT_E_INVALID: Lp < L, ldx or a column offset that breaks the 8-byte (q / k) or 16-byte (v) loads or does not hold H dh columns, a present part whose pointers are NULL. */
int ezdit_test_headnorm(const float* dev_x, int ldx, int q_col, int k_col, int v_col, const float* dev_qn_w, const float* dev_qn_b, const float* dev_kn_w,
                        const float* dev_kn_b, const float* dev_rope_cos, const float* dev_rope_sin, void* dev_q, void* dev_k, void* dev_v,
                        int B, int H, int L, int Lp, int dh, ezdit_stream stream);
/* unit-test hook of k_assemble (csrc/rowops.hip): in_ch = C: out bf16 [B L][ldo] = [x[b % x_rows] | gt where gt_mask == 0, else mask_embed | gt_mask channel 0, or 1 without
 * gt | zeros] from x fp32 [x_rows][C][L], gt fp32 / gt_mask uint8 [x_rows][C][L] (both or neither), mask_embed fp32 [C]; in_ch = 2 C + 1: x fp32 [B][in_ch][L] is already
 * assembled (transpose + cast).  dev_lens int32 [B] on the DEVICE or NULL: frames >= lens[b] become zero rows.  EZDIT_E_INVALID: another in_ch, x_rows that does not divide
 * B, gt without gt_mask or the reverse, ldo < 2 C + 1, lens outside [1, L] (read back as above). */
int ezdit_test_assemble(const float* dev_x, int x_rows, int in_ch, const float* dev_gt, const uint8_t* dev_gt_mask, const float* dev_mask_embed, void* dev_out, int ldo,
                        int B, int C, int L, const int32_t* dev_lens, ezdit_stream stream);
/* copy an internal fp32/bf16 buffer (by name, e.g. "h", "u", "q", "k", "v", "mod") for debugging. */
int ezdit_debug_buffer(ezdit_handle* h, const char* name, void** dev_ptr, size_t* bytes);
/* number of kernel launches issued by the last ezdit_forward (host counter). */
int ezdit_last_launch_count(const ezdit_handle* h);
/* n > 0: ezdit_forward returns after n kernel launches so a test can inspect intermediates; 0 = off. */
int ezdit_debug_stop_after(ezdit_handle* h, int n_launches);
/* A/B knobs (a captured graph is dropped and re-captured; set them BEFORE ezdit_prepare_timesteps when they select the LayerNorm-algebra path).
 * Defaults are the measured best on MI355X; none changes results beyond fp rounding.  Unknown names return EZDIT_E_INVALID.  Every name below is set
 * by a test (tests/test_host.py: all of them on a handle; tests/test_gpu.py, tests/test_controlnet.py: each non-default value against the reference
 * goldens or bitwise against the default).  Round 5 removed 30 names that only the experiments which settled them ever set (tile / split-K ids per
 * shape, zbig*, ztile, zmlp, zskip, pp_max_m, prefetch, gemm_debug, fuse_resid, fuse_qkv, fuse_qnorm, qkv_waves9, xcd_map, slab_bf16, geglu_tile ...).
 *   zfuse 0/1, default 1 (LayerNorm algebra: attention-out / cross-attention-out / skip_linear / in-block MLP-out projections UN-SPLIT with the
 *     residual, per-column-tile LayerNorm statistics and the next GEMM's operand in their epilogue -- k_gemm_ks (csrc/gemm_ks.h) up to 2048 rows,
 *     the ping-pong kernel's 128 x 144 tile above -- the consumer GEMM finishing the LayerNorm in its epilogue: no split-K slabs, no row
 *     kernel on those edges; needs gemm_pp = 3 and a LayerNorm-algebra q projection (fuse_q2 at small grids, q2_pp above); 0 = split-K slabs + row kernel)
 *   xkey1 0/1, default 1 (single-key cross-attention shortcut, needs zfuse: a batch element whose context mask has ONE valid key -- every unconditional
 *     row of classifier-free guidance -- gets the constant W_o v_key + b_o from the attention-out projection instead of a cross-attention launch;
 *     cross-attention and its out-projection then run over the other batch elements only.  Exact (softmax over one key is 1); 0 = every row through k_attn)
 *   skip_z 0/1, default 1 (needs zfuse; M <= 2048 token rows, no ControlNet residuals: the out-blocks' LayerNorm over [x | skip] in front of skip_linear by the same algebra --
 *     the in-block that produces a skip keeps its statistics and writes its half of the out-block's operand, the MLP-out projection in front of the out-block runs un-split,
 *     skip_linear finishes the LayerNorm in its epilogue: one launch less per out-block; 0 = split-K slabs + the row kernel on that edge)
 *   geglu_co / qkv_co 0/1/2 (GEGLU GEMM / fused QKV GEMM on the co-resident kernel k_gemm_co (csrc/gemm_co.h): 4-wave workgroups, 128 x 144 tiles, TWO per CU, so that one
 *     workgroup's prologue / epilogue runs under the other's K loop; 1 = above 2048 token rows (batched prompts), 2 = always, 0 = the ping-pong kernel's 128 x 288 tile.
 *     Defaults: geglu_co 0, qkv_co 1 -- four prompts per GPU -1.5 % per step, one prompt untouched.
 *     qkv_form: the fused QKV GEMM's form on the ping-pong kernel up to 2048 token rows.  1 (default) = tile 67, the un-split 8-wave form: every wave walks every K tile of
 *     16 rows x two heads, nothing is exchanged behind the loop; 0 = tile 61, the k-split schedule with the partial-tile exchange (results differ in the fp32 summation order
 *     over K only).  The option list is closed, so the form rides on this knob: qkv_co + 4 selects qkv_form = 0.  Above 2048 rows qkv_co decides as before)
 *   gemm_pp (ping-pong kernel k_gemm_pp: bit 0 GEGLU GEMM; 0 = the round-1 lockstep kernel for it and no LayerNorm algebra.  Bit 1 -- the fused QKV GEMM -- is
 *     retired: since round 6 that GEMM always runs on the ping-pong kernel, its weights are packed for it, EZDIT_T_QKROPE)
 *   tile_partial (tile id of the split-K residual GEMMs at M <= 2048 rows: 9 = lockstep 128 x 128, 62 = the same tile on the ping-pong kernel; csrc/gemm.hip table)
 *   wt 0/1/2 (write-through (sc1) output stores; 2 = default: on while B L <= 2048)
 *   fuse_q2 0/1/2 (cross-attention computes its own q projection; 2 = also for large grids), q2_pp 0/1 (cross-attention q projection at grids too large
 *     for fuse_q2: ping-pong GEMM with the per-head LayerNorm in its epilogue; 0 = fp32 GEMM + normalisation inside k_attn)
 *   attn_nkh 0/2/4 (attention key sub-blocks per tile, 0 = by grid size), attn_xk2 0/1 (cross-attention q projection: two K tiles per ring slot and barrier)
 *   attn_qtile 0/32/64 (fused cross-attention: query rows per workgroup; 0 = 32 when the 64-row grid has <= 128 workgroups -- one prompt with the single-key shortcut)
 *   attn_xcd 0/1 (attention: all query tiles of a (batch, head) pair on one XCD), gemm_panel (bit mask over 1 D x D projections, 2 skip_linear, 4 MLP-out; M <= 1024: the split-K GEMM puts all workgroups of
 *     an M tile on XCD tm % 8) and row_affine 0/1 (the row kernel processes row panel p on XCD p % 8).  Placement only: bitwise identical results.
 *   row_variant 0/1 (row kernel: one workgroup / one wave per row), epi_lds 0/1 (bf16 GEMM epilogues staged through LDS and written as 16-byte row chunks)
 *   cn_overlap 0/1 (fused sampler: ControlNet branch on a side stream next to the backbone's in-blocks)
 *   stamp_launch i / trace_launches 0/1 (diagnostics, eager launches only: launch i of a forward writes its in-kernel cycle stamps to the buffer
 *     registered with ezdit_debug_gemm_timestamps; every launch of a forward is named on stderr -- tools/diag_stamps.py)
 * A library built with -DEZ_DIAG (EZAUDIO_DIAG=1 python -m ezaudio_amd.build) also knows zfake 0/1: the LayerNorm-algebra consumers run on a finished
 * LayerNorm with neutral tables (what the consumer side costs by itself; results change by the factor rsqrt(1 + 1e-5)). */
int ezdit_set_option(ezdit_handle* h, const char* name, int value);

/* ---- Sliding-window self-attention ------------------------------------------------------------------------------------------------------------------------
 * radius >= 1: in every block's SELF-attention frame i attends to the frames j with |i - j| <= radius (and j below the sample's length, ezdit_set_lengths) --
 * 2 radius + 1 keys, so a row of any length stays inside the range of relative RoPE positions the model was trained on (radius 250 = the 501 keys of the
 * trained 10 s row).  radius 0 = off (default).  Cross-attention, the single-key shortcut and everything else in the block are untouched: nothing else looks
 * along the time axis.  Handle-scoped: it survives ezdit_bind_workspace and ezdit_sampler_begin.  With radius >= L - 1 of the bound row nothing is masked and the
 * step launches exactly the kernels of radius 0 (same bits, same launch count); otherwise the self-attention launch of each block is the band form of k_attn
 * (csrc/attn.hip BAND: it walks only the key tiles its queries can see), one launch as before.  A change drops the captured step, like ezdit_set_option.
 * Accepted on backbone and ControlNet handles; ezdit_sampler_attach_controlnet refuses (EZDIT_E_INVALID) a pair whose radii differ -- set both before attaching.
 * EZDIT_E_INVALID: radius < 0.  EZDIT_E_STATE: the handle's stream (that of its latest bind / sampler run) is being captured.
 * Audio quality of windowed sampling on the released checkpoints is unmeasured. */
int ezdit_set_attention_window(ezdit_handle* h, int radius);
/* unit-test hook of the band form: self-attention (Lq = Lk = L, padded to Lp) with key j valid for query i iff |i - j| <= radius and j < klen[b] (L where dev_klen is
 * NULL).  Buffer layouts, refusals and the klen read-back are those of ezdit_test_attention_varlen (no key mask); radius >= 1 is required (EZDIT_E_INVALID).  It ALWAYS
 * launches the band instantiation, also for radius >= L - 1 where nothing is masked: that launch must equal ezdit_test_attention bit for bit. */
int ezdit_test_attention_band(ezdit_handle* h, const void* dev_q, const void* dev_k, const void* dev_v, void* dev_out, int B, int L, int Lp,
                              const int32_t* dev_klen, int radius, ezdit_stream stream);

/* ---- Prompt timeline: time-varying prompts in one row's cross-attention -----------------------------------------------------------------------------------
 * The bound context holds S prompts of 128 tokens each (Lc = 128 S: prompt s occupies the context rows [128 s, 128 s + 128) of ezdit_prepare_context, its unused rows
 * zero with mask 0) and every latent frame i of batch row b weights them, weights[b][s][i] >= 0 (HOST, [B][S][L], natural weights):
 *     out_i = sum_s sum_{j in K_s} w_si exp(q_i k_j / sqrt(dh)) v_j  /  sum_s sum_{j in K_s} w_si exp(q_i k_j / sqrt(dh))          (K_s: the valid keys of prompt s)
 * -- attention over all prompts' tokens with the bias ln w_si on the scores of prompt s.  A weight of 0 removes the prompt for that frame; only the ratios of a
 * frame's weights matter (the table stores log2(w / max_s w)); a frame that weights one prompt gets that prompt's plain cross-attention.  Applied inside the
 * cross-attention launch of every block (csrc/attn.hip TL: a workgroup walks only the prompts its frames weight): the launch count of a step does not change.
 * Self-attention, the MLP, AdaLN and RoPE are untouched.  A row that needs no timeline carries weight 1 on prompt 0 and 0 elsewhere.
 * A run-time table of the step (contract above), bind-scoped; it serves ezdit_forward and the sampler step alike.  Call it after ezdit_prepare_context (the weights
 * are checked against its key mask; a new ezdit_prepare_context switches the table off) and after ezdit_set_lengths (frames beyond a row's length are neither checked nor
 * read: they take the last frame's weights, so padding rows stay finite; ezdit_set_lengths with OTHER lengths returns EZDIT_E_STATE while the table is on).  S = 1 with every weight 1 gives the bits of the call without the table.
 * EZDIT_E_INVALID: S outside [1, 16]; Lc != 128 S; a negative or non-finite weight; a frame that weights no prompt with a valid key (which covers a single-key row
 * -- the unconditional row of classifier-free guidance -- whose key's prompt is weighted 0 at some frame).  EZDIT_E_UNSUPPORTED: a ControlNet handle, a backbone with
 * a ControlNet attached, a canvas that is on; ezdit_sampler_attach_controlnet and the canvas setters refuse likewise while the table is on.  EZDIT_E_STATE: no
 * prepared context.  Audio quality on the released checkpoints is unmeasured: whether a cross-fade of the softmax prior sounds like one, and which fade length to use. */
int ezdit_set_context_weights(ezdit_handle* h, const float* weights, int S, ezdit_stream stream);
/* unit-test hooks of the timeline form.  ezdit_test_attention_timeline: the layouts and refusals of ezdit_test_attention plus weights (HOST, [B][S][Lq]) and
 * Lk = Lkp = 128 S; the weights are checked as the setter checks them.  It ALWAYS launches the TL instantiation of the plain 8-wave kernel, and waits for it.
 * ezdit_test_cross_attention_timeline: the arguments of ezdit_test_cross_attention, then weights (HOST, [B][S][Lq], for the launched batch elements) and S;
 * qtile 32 or 64 (EZDIT_E_INVALID otherwise). */
int ezdit_test_attention_timeline(ezdit_handle* h, const void* dev_q, const void* dev_k, const void* dev_v, const uint8_t* dev_kmask, void* dev_out, int B,
                                  int Lq, int Lk, int Lqp, int Lkp, const float* weights, int S, ezdit_stream stream);
int ezdit_test_cross_attention_timeline(const void* dev_xu, int ldu, const void* dev_xw, int ldw, int xw_rows, int xK, const float* dev_qn_w, const float* dev_qn_b,
                                        const void* dev_k, const void* dev_v, const uint8_t* dev_kmask, void* dev_out, int ldo, int B, int b0, int H, int dh, int Lq, int Lk,
                                        int Lqp, int Lkp, const void* dev_zstat_in, long zs_stride, int zparts, int zD, int zw, const float* dev_zG, const float* dev_zC,
                                        float zeps, int xk2, int qtile, int xcd_map, const float* weights, int S, ezdit_stream stream);

/* ---- Prompt emphasis: per-token weights as a key bias in cross-attention ------------------------------------------------------------------------------------
 * Every context token j of batch row b carries a weight w_bj > 0 (HOST, [B][Lc], natural weights; n = B rows) and, with V_b the valid keys of the row's mask,
 *     out_i = sum_{j in V_b} w_bj exp(q_i k_j / sqrt(dh)) v_j  /  sum_{j in V_b} w_bj exp(q_i k_j / sqrt(dh))
 * -- attention with the bias ln w_bj on the scores of key j, the same in every block and head.  An integer weight n is exactly that token's context row repeated n
 * times.  V is untouched, and so are K / V of ezdit_prepare_context: the table costs nothing per call.  Only the ratios within a row matter: the table stores
 * fp32(log2(w_bj / max_{j in V_b} w_bj)) (computed in fp64; [B][Lcp], 0 at masked and padding keys).  The mask alone decides validity: the values of `weights` at masked keys
 * are not read, and dropping a token is the mask's business (a weight of 0 is refused).  Applied inside the cross-attention launch of every block (csrc/attn.hip KW):
 * the launch count of a step does not change.  A single-key row (the unconditional row of classifier-free guidance) stays exact: softmax over one key is 1 whatever its weight.
 * A run-time table of the step (contract above), bind-scoped; it serves ezdit_forward and the sampler step alike, with composed guidance, the canvas and the ring, length
 * tables, the start table and the multistep solver.  Call it after ezdit_prepare_context (the weights are checked against its key mask; a new ezdit_prepare_context switches
 * the table off).  A table in which every row's valid weights are equal ("all weights 1" included) is OFF: the step runs the plain kernels, bit for bit the call that
 * never set it.  weights == NULL switches it off.
 * EZDIT_E_INVALID: n != B; a valid key's weight that is not finite or <= 0; a row whose largest and smallest valid weights differ by more than 2^20.
 * EZDIT_E_UNSUPPORTED: a ControlNet handle or a backbone with a ControlNet attached (its blocks have cross-attention of their own; ezdit_sampler_attach_controlnet refuses
 * likewise while the table is on); the prompt timeline being on (ezdit_set_context_weights refuses likewise while this table is on); a bound shape whose cross-attention
 * does not run an 8-wave form of the kernel (Lc padded to a multiple of 128 and at most 512 workgroups of 64 queries): that one is reported by ezdit_forward /
 * ezdit_sampler_run, from the launcher's own check, while the table is on.  EZDIT_E_STATE: no prepared context.
 * Audio quality on the released checkpoints is unmeasured: how strongly a weight of 1.6 is heard.
 * ABI: additive (version unchanged): one setter and the two hooks below; AttnArgs is internal. */
int ezdit_set_context_token_weights(ezdit_handle* h, const float* weights, int n, ezdit_stream stream);
/* unit-test hooks of the emphasis form: the arguments of their ..._timeline twins with natural weights (HOST, [B][Lk], for the launched batch elements) instead of the
 * timeline's, checked as the setter checks them against the launched rows of dev_kmask, and keep_on: 0 = a table of zeros launches the plain instantiation (as the
 * setter would), 1 = the KW instantiation whatever the table holds -- that launch must equal the hook without weights bit for bit.  Lkp % 128 == 0 (EZDIT_E_UNSUPPORTED
 * otherwise); they wait for the launch. */
int ezdit_test_attention_keyweights(ezdit_handle* h, const void* dev_q, const void* dev_k, const void* dev_v, const uint8_t* dev_kmask, void* dev_out, int B,
                                    int Lq, int Lk, int Lqp, int Lkp, const float* weights, int keep_on, ezdit_stream stream);
int ezdit_test_cross_attention_keyweights(const void* dev_xu, int ldu, const void* dev_xw, int ldw, int xw_rows, int xK, const float* dev_qn_w, const float* dev_qn_b,
                                          const void* dev_k, const void* dev_v, const uint8_t* dev_kmask, void* dev_out, int ldo, int B, int b0, int H, int dh, int Lq, int Lk,
                                          int Lqp, int Lkp, const void* dev_zstat_in, long zs_stride, int zparts, int zD, int zw, const float* dev_zG, const float* dev_zC,
                                          float zeps, int xk2, int qtile, int xcd_map, const float* weights, int keep_on, ezdit_stream stream);

/* ---- T5 text encoder (csrc/t5.hip): stands in for transformers' T5EncoderModel in the `text_encoder` slot (api/ezaudio.py:80-82, src/inference.py:42-50) --------
 * Encoder stacks of the flan-t5 / T5 v1.1 family only: gated gelu_new feed-forward, head dim 64, no biases, T5LayerNorm (RMS), the bidirectional
 * relative-position bias of block 0 shared by all layers.  Same conventions as above: caller-owned device memory (one weight blob, one workspace per
 * (B, L)), errors through ezdit_last_error(), ezt5_encode asynchronous on its stream (capturable).  The tokenizer stays outside.
 * Nothing below touches an ezdit_handle; the ABI version is unchanged (additive). */
typedef struct ezt5_handle ezt5_handle;
enum { EZT5_FF_GATED_GELU_NEW = 0, EZT5_FF_RELU = 1, EZT5_FF_GATED_GELU = 2, EZT5_FF_OTHER = 3 };   /* only the first is built */
typedef struct {
    int32_t vocab;         /* rows of the token embedding (shared.weight) */
    int32_t d_model;       /* multiple of 64 */
    int32_t d_kv;          /* head dim: 64 */
    int32_t num_heads;     /* inner width = num_heads * d_kv (need not equal d_model) */
    int32_t d_ff;          /* multiple of 64 */
    int32_t num_layers;
    int32_t num_buckets;   /* relative_attention_num_buckets (32) */
    int32_t max_distance;  /* relative_attention_max_distance (128) */
    float   eps;           /* layer_norm_epsilon */
    int32_t max_len;       /* longest token sequence (<= 512): the expanded bias table covers the distances -(max_len - 1) .. max_len - 1 */
    int32_t ff_act;        /* EZT5_FF_*: feed_forward_proj of the checkpoint; anything but gated gelu_new is EZDIT_E_UNSUPPORTED */
} ezt5_config;
/* one tensor of the weight blob.  Names / shapes / sources (Hugging Face T5EncoderModel keys, N = layer):
 *   embed        f32  [vocab][d_model]             shared.weight (= encoder.embed_tokens.weight)
 *   bias_table   f32  [num_heads][2 max_len - 1]   entry [h][(key - query) + max_len - 1] = encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight
 *                                                  [bucket(key - query)][h], bucket() = T5Attention._relative_position_bucket, bidirectional (expanded once, by the packer)
 *   blkN.ln0     f32  [d_model]                    encoder.block.N.layer.0.layer_norm.weight
 *   blkN.wqkv    bf16 [3 inner][d_model]           ...layer.0.SelfAttention.{q, k, v}.weight stacked along dim 0
 *   blkN.wo      bf16 [d_model][inner]             ...layer.0.SelfAttention.o.weight
 *   blkN.ln1     f32  [d_model]                    encoder.block.N.layer.1.layer_norm.weight
 *   blkN.wi      bf16 [2 d_ff][d_model]            ...layer.1.DenseReluDense.{wi_0, wi_1}.weight stacked along dim 0
 *   blkN.wff     bf16 [d_model][d_ff]              ...layer.1.DenseReluDense.wo.weight
 *   final_ln     f32  [d_model]                    encoder.final_layer_norm.weight
 * Every matrix is stored row-major and unpadded ([rows][cols]); offsets are 256-byte aligned. */
typedef struct {
    char    name[32];
    int32_t dtype;         /* EZDIT_P_* */
    int32_t reserved;
    int64_t rows, cols;
    int64_t offset;        /* byte offset in the blob */
} ezt5_tensor_info_t;

/* EZDIT_E_UNSUPPORTED (nothing allocated): d_kv != 64; d_model, d_ff or num_heads * d_kv not a multiple of 64; ff_act != EZT5_FF_GATED_GELU_NEW; max_len > 512 */
int    ezt5_create(const ezt5_config* cfg, ezt5_handle** out);
int    ezt5_destroy(ezt5_handle* h);
int    ezt5_tensor_count(const ezt5_handle* h);
/* bytes of the weight blob; `table` (nullable) receives the first `capacity` entries of the tensor table, in blob order */
size_t ezt5_blob_bytes(const ezt5_handle* h, ezt5_tensor_info_t* table, int capacity);
int    ezt5_bind_weights(ezt5_handle* h, const void* dev_blob, size_t bytes);
/* activations of one encode of B sequences of L tokens (0 + error message: L > max_len, or rows x widest activation >= 2^31 elements) */
size_t ezt5_workspace_bytes(const ezt5_handle* h, int B, int L);
/* also decides the four GEMM shapes of a layer at B * L rows: EZDIT_E_UNSUPPORTED for one the GEMM refuses, so that ezt5_encode meets none */
int    ezt5_bind_workspace(ezt5_handle* h, void* dev_ws, size_t bytes, int B, int L);
/* last_hidden_state: ids int32 [B][L], mask uint8 [B][L] (1 = attend; HF attention_mask) -> out fp32 [B][L][d_model].  Masked keys contribute exactly 0; rows at masked
 * positions are computed like any other (finite).  (B, L) must be the bound workspace's: EZDIT_E_STATE otherwise, and without weights; L > max_len: EZDIT_E_UNSUPPORTED.
 * A device index beyond the GEMM's 32 per-device slots: EZDIT_E_UNSUPPORTED.  Nothing is launched when an error other than EZDIT_E_HIP is returned
 * (EZDIT_E_HIP: a launch failed, or the runtime refused a GEMM's LDS attribute, possibly after earlier launches of the same encode). */
int    ezt5_encode(ezt5_handle* h, const int32_t* dev_ids, const uint8_t* dev_mask, float* dev_out, int B, int L, ezdit_stream stream);
/* unit-test hooks (same kernels; two, one per new kernel that a test must reach below ezt5_encode): k_t5_attn on q, k, v bf16 [B L][64 H] (head h in columns [64 h, 64 h + 64)), bias fp32 [H][2 L - 1] (entry (key - query) + L - 1),
 * mask uint8 [B][L] -> out bf16 [B L][64 H] = softmax(q k^T + bias + mask) v, no 1 / sqrt(d) scale, L <= 512 ... */
int    ezt5_test_attention(const void* dev_q, const void* dev_k, const void* dev_v, const float* dev_bias, const uint8_t* dev_mask, void* dev_out,
                           int B, int H, int L, ezdit_stream stream);
/* ... and k_t5_embed_rms on x fp32 [M][D] (D % 4 == 0), w fp32 [D] -> out bf16 [M][D] = bf16(x rsqrt(mean(x^2) + eps) w) */
int    ezt5_test_rms(const float* dev_x, const float* dev_w, float eps, void* dev_out, int M, int D, ezdit_stream stream);
/* The encoder's launchers with their full argument lists, one hook per launch of ezt5_encode (tests/test_t5_kernels_gpu.py chains them into a layer, bit for bit).
 * Everything that bounds an address is refused (EZDIT_E_INVALID / EZDIT_E_UNSUPPORTED) before the first HIP call.
 * k_t5_attn in either operand form: f32_in = 0 bf16 operands, 1 fp32 operands rounded in the loader (ezt5_encode: one interleaved buffer, k = q + inner, v = q + 2 inner,
 * ld = 3 inner).  q, k, v rows [B L][ld] (ld >= 64 H, a multiple of 8), bias fp32 [H][bias_ld] with entry (key - query) + bias_half (bias_half >= L - 1,
 * bias_ld >= bias_half + L), out bf16 rows [B L][ldo] (ldo >= 64 H, a multiple of 4; columns >= 64 H are not written). */
int    ezt5_test_attention_ex(const void* dev_q, const void* dev_k, const void* dev_v, int f32_in, int ld, const float* dev_bias, int bias_ld, int bias_half,
                              const uint8_t* dev_mask, void* dev_out, int ldo, int B, int H, int L, ezdit_stream stream);
/* k_t5_embed_rms: exactly one of ids (int32 [M], clamped to [0, vocab); needs emb fp32 [vocab][D] and x_out fp32 [M][D], which receives the gathered rows) / x_in fp32 [M][D]
 * (x_out is then not touched and may alias x_in), exactly one of u_bf16 [M][D] / out_f32 [M][D]; D a positive multiple of 4 */
int    ezt5_test_embed_rms(const int32_t* dev_ids, const float* dev_emb, int vocab, const float* dev_x_in, float* dev_x_out, const float* dev_w, float eps,
                           void* dev_u_bf16, float* dev_out_f32, int M, int D, ezdit_stream stream);
/* k_t5_gated_gelu: h fp32 [M][2 F] -> g bf16 [M][F] = gelu_new(h[:, :F]) h[:, F:]; F a positive multiple of 4 */
int    ezt5_test_gated_gelu(const float* dev_h, void* dev_g, int M, int F, ezdit_stream stream);
/* the encoder's GEMM call: out fp32 [M][N] = A bf16 [M][K] . W bf16 [N][K]^T (+ resid fp32 [M][N], nullable), after the shape check ezt5_bind_workspace makes */
int    ezt5_test_gemm(const void* dev_A, int K, const void* dev_W, int N, const float* dev_resid, float* dev_out, int M, ezdit_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* EZDIT_H */
