// C ABI of libezaudio_hip.so (include/ezdit.h): parameter layout, workspace carving, and the host-side
// sequencing of the denoising step.  The sequencing restates UDiT.forward (src/models/udit.py:281-362),
// DiTBlock._forward (src/models/blocks.py:120-160) and the sampler loop body (src/inference.py:70-100)
// as a fixed chain of asynchronous kernel launches on one stream (hipGraph-capturable: no allocation, no
// sync, no host read-back anywhere below ezdit_forward / ezdit_sampler_run).
#include "../../include/ezdit.h"
#include "common.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

static thread_local std::string g_err;

// sets the thread-local message behind ezdit_last_error() and returns `code` (shared with vae.hip through common.h)
int ez_fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define fail ez_fail
// the reason a launcher gave for refusing a configuration (ez_refuse), until the caller that reports the refusal takes it
static thread_local std::string g_refusal;
int ez_refuse(const char* fmt, ...) {
    char buf[384];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_refusal = buf;
    return 1;
}
static std::string take_refusal() {
    std::string r;
    if (!g_refusal.empty()) r = " (" + g_refusal + ")";
    g_refusal.clear();
    return r;
}

namespace {

#define HIPCHK(expr)                                                                            \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) return fail(EZDIT_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

inline long rup(long x, long a) { return (x + a - 1) / a * a; }

struct Buf {  // one carved workspace region
    size_t off = 0, bytes = 0;
};

}  // namespace

struct WRef {   // one bf16 weight matrix of the blob, resolved once at ezdit_bind_weights
    const bf16_t* W = nullptr; int ld = 0; int rows = 0;
};
struct BlkW {   // per-block parameters used on the per-step path (no string / map work inside ezdit_forward)
    const float *bskip, *aqnw, *aqnb, *aknw, *aknb, *bo, *n2w, *n2b, *cqnw, *cqnb, *bo2, *b1, *b2, *snw, *snb, *zb;
    WRef wskip, wqkv, wo, wq2, wo2, w1, w2, zw;
};
struct WsPtrs {  // workspace regions used on the per-step path, resolved once at ezdit_bind_workspace
    int* ints; float *rope_cos, *rope_sin, *coef, *cfgpart;
    bf16_t* ape; float *h, *skips; bf16_t *u, *ucat; float* qkv; bf16_t *q, *k, *v, *ao, *act; float *part, *y, *pred;
    uint8_t* kmask; bf16_t *kc, *vc; float *mod, *modf;
    float *cembed, *cnres; bf16_t* skipbf;   // ControlNet only
    float2* zstat; float *zt_qkv, *zt_geglu, *zt_q2;   // LayerNorm algebra: partial row statistics, G' / C' tables
    float2* zstat_skip; float* zt_skip; bf16_t* ucat_z;              // ... of the out-blocks' LN_2D([x | skip]) -> skip_linear: the skips' statistics (kept from the in-block to its out-block), static tables
    float* spc;  // [n_steps][P][8] DDIM coefficients per sample: the second device array of the table ezdit_handle::sp
    float* zd;   // [nblk][B][D] constant cross-attention-out vectors of the single-key batch elements (opt_xkey1)
};

static void drop_graph(ezdit_handle* h);

// A run-time table of the step (include/ezdit.h, "Run-time tables of the step"): a small device array that the kernels of the captured step read at run time, so
// one captured step serves every set of values.  Only switching a table on or off changes kernel arguments (null <-> table, or another kernel) and drops the
// graph; so does a kernel argument that rides with the table (`rearm`: the multistep history pointer, the canvas' T and ramp).  The kernels are given read().
template <typename T>
struct Table {
    bool on = false;
    std::vector<T> host;   // host mirror: the source of the asynchronous upload, which it must outlive (upload_table)
    T* dev = nullptr;      // workspace region (resolve_workspace)
    const T* read() const { return on ? dev : nullptr; }
    void set(ezdit_handle* owner, bool to, bool rearm = false) {
        if (to != on || (to && rearm)) drop_graph(owner);
        on = to;
    }
};

static unsigned long long* g_gemm_ts = nullptr;   // ezdit_debug_gemm_timestamps: device buffer for in-kernel cycle stamps (gemm_pp.h, gemm_ks.h, attn.hip)
static long g_gemm_ts_cap = 0;                    // ... and the workgroups it has room for ([workgroup][8] uint64): a launch with a larger grid gets no stamps

struct ezdit_handle {
    ezdit_config cfg;
    int D, H, dh, nblk, nhalf, I, C, Cin, Cctx, r6;
    int DQK, DV;       // padded head dims used by the attention layouts
    int ldD, ld2D, ldI, ldPE, ldCtx;  // bf16 leading dimensions (multiples of 64)
    float scaling;

    std::vector<ezdit_param_info_t> params;
    std::map<std::string, int> pidx;
    size_t param_bytes = 0;
    const char* wblob = nullptr;

    // workspace
    char* ws = nullptr;
    size_t ws_bytes = 0;
    int B = 0, L = 0, Lc = 0, n_slots = 0, M = 0, Mp = 0, Lp = 0, Lcp = 0, Mc = 0;
    std::map<std::string, Buf> bufs;
    bool ctx_ready = false, ts_ready = false, cond_ready = false;
    bool z_tables_ready = false;   // the LayerNorm-algebra tables of the prepared timesteps exist (opt_zfuse was on at ezdit_prepare_timesteps)
    bool skip_tables_ready = false;   // ... and the static tables of the skip path (opt_skip_z was on as well): a forward never reads tables that were not built
    int n_ts = 0, per_row = 0;

    // sampler
    float* latents = nullptr;
    const float* noise = nullptr;
    const float* s_gt = nullptr;
    const uint8_t* s_gt_mask = nullptr;
    int P = 0, n_steps = 0;
    float gscale = 0.f, grescale = 0.f;
    hipGraphExec_t graph_exec = nullptr;
    hipGraph_t graph = nullptr;

    // ---- run-time tables of the step (struct Table).  Bind-scoped: cleared by reset_bind_state ----
    Table<int> lens;     // [B] padded batch (ezdit_set_lengths, ezdit_sampler_set_pair_lengths): batch element b is valid on frames [0, lens[b])
    const int* lens_dev() const { return lens.read(); }
    Table<float> cns;    // [B] conditioning_scale per batch element of the attached ControlNet (ezdit_sampler_set_cn_scales), read by the row kernel
    // prompt timeline (ezdit_set_context_weights): the context is tl_S prompts of 128 keys and every frame weights them.  The mirror is [B][S][L] score biases (k_attn TL,
    // AttnArgs.tlb), which go to `dev`, then [B][S] frame supports as int pairs (bit copies in the float mirror), which go to tlsup.  Read by the cross-attention launch only
    Table<float> tl;
    int2* tlsup = nullptr;
    int tl_S = 0;
    // prompt emphasis (ezdit_set_context_token_weights): [B][Lcp] score biases log2(w_j / max w) of the context keys (k_attn KW, AttnArgs.kbias), zero at masked and padding
    // keys.  On only while some bias is non-zero: a uniform row is the plain kernel.  Read by the cross-attention launch only
    Table<float> tw;
    // ---- call-scoped: they belong to one sampler call and are cleared by reset_call_state ----
    // per-sample sampler settings (ezdit_sampler_set_sample_params), read by k_cfg_stats / k_cfg_apply: the mirror is [P][2] (guidance_scale, guidance_rescale),
    // which goes to `dev`, then [n_steps][P][8] DDIM coefficients, which go to p.spc.  Room for sp_cap(B) samples: the B / 2 of a CFG batch
    Table<float> sp;
    static int sp_cap(int B) { return B / 2 + 1; }
    // the call's coefficient rows [n_steps][8] (ezdit_sampler_begin uploads them; the step always reads them).  `on` is the multistep solver
    // (ezdit_sampler_set_multistep): c_hist lives in slot 5 of the rows, the history of data predictions ms_hist is the caller's and a kernel argument
    Table<float> coef;
    float* ms_hist = nullptr;
    Table<int> start;    // [P] first step of each sample (ezdit_sampler_set_start), read by the last two kernels of the step.  start_min is the step the run begins at
    int start_min = 0;
    // [P] first canvas frame of each window (ezdit_sampler_set_canvas): the P windows of the call overlap on a canvas of canvas_T frames and k_canvas_blend, one more
    // launch behind the update, averages the shared frames (T and the ramp are its arguments).  Off: the step issues the launches it has always issued
    // canvas_loop (ezdit_sampler_set_canvas_loop): the same table read as a ring of canvas_T frames, blended by k_canvas_blend_loop -- another kernel, so the
    // two setters replacing each other drop the graph
    Table<int> canvas;
    int canvas_T = 0, canvas_ramp = 1;
    bool canvas_loop = false;
    // [P][cw_K] weights of composed guidance (ezdit_sampler_begin_composed switches it on, ezdit_sampler_set_compose_weights replaces the values): the batch is
    // [c_0 | .. | c_{K-1} | u], B = (cw_K + 1) P, and the last two kernels of the step run their composed instantiations (launch_cfg_compose).  K is a kernel argument
    Table<float> cw;
    int cw_K = 1;
    // [P][4] (eta_apg, norm_threshold, momentum, on) of adaptive projected guidance (ezdit_sampler_set_apg): the last two kernels of the step run their APG
    // instantiations (launch_cfg_apg), always both.  The momentum buffer apg_mom is the caller's and a kernel argument, like ms_hist
    Table<float> apg;
    float* apg_mom = nullptr;

    int launches = 0;
    bool is_cn = false;          // ControlNet variant (cfg.controlnet)
    int c0 = 0, c0m = 0, c1 = 0; // condition-embed channel counts
    ezdit_handle* cn = nullptr;  // ControlNet attached to this backbone's sampler
    float cn_scale = 1.0f;       // conditioning_scale of the ATTACHED ControlNet (fused sampler only)
    float fwd_cn_scale = 1.0f;   // scale ezdit_forward applies to caller-provided residuals (ezdit_set_cn_scale; default 1)
    std::vector<ezdit_handle*> cn_users;  // backbones whose sampler has this ControlNet attached (cleared on destroy)
    const float* ext_mask_embed = nullptr;
    // ---- fixed tile / split-K choices (measured on MI355X in rounds 1-4; the per-shape override options they used to be
    // were deleted in round 5: nothing but the experiments that settled them ever set a non-default value) ----
    // M <= 2048 rows: 128 x 128 8-wave tiles with a 3-deep ring and split-K 3 (216 workgroups, 3 bf16 slabs) for the residual GEMMs that still run
    // split-K, 128 x 64 8-wave ring 4 for the small fp32 ones; patch embed and final Linear on the K-split kernel (k_gemm_ks: 252 / 42 workgroups)
    static constexpr int kSplitK = 3, kTileF32 = 25, kTilePE = 70, kTileFin = 73;
    // M > 2048 rows (batched prompts): the split-K residual GEMMs that remain on the ping-pong kernel's 128 x 288 tile with split-K 2 (32 x 4 x 2 =
    // 256 workgroups at M = 4000, no N padding); the un-split LayerNorm-algebra producer is the ping-pong kernel's 128 x 144 tile above kZBigM rows
    // (one round of 256 workgroups at M = 4000) and k_gemm_ks's 48 x 96 tile (id 70) up to there
    static constexpr int kTilePartialBig = 60, kSplitBig = 2, kZTile = 70, kZBigM = 2048;
    int opt_tile_partial = 9;   // split-K residual GEMMs at M <= 2048: 9 = lockstep 128 x 128 (k_gemm), 62 = the same tile on the ping-pong kernel
    int opt_gemm_pp = 3;   // ping-pong kernel (k_gemm_pp): bit 0 GEGLU GEMM (128x288; 0 = the round-1 lockstep kernel and no LayerNorm algebra); bit 1 retired in round 6 (the fused QKV GEMM always runs on it)
    // LayerNorm algebra (common.h, GemmArgs.z*): the attention-out, cross-attention-out, skip_linear and (in front of an in / mid block) MLP-out
    // projections run UN-SPLIT (k_gemm_ks, gemm_ks.h: 48 x 96 tiles, 252 workgroups at M = 1000; the ping-pong kernel's 128 x 144 tile above 2048 rows) with
    // the gated residual, per-column-tile LayerNorm statistics and the next GEMM's operand bf16(h g) in their epilogue; the consumer (fused QKV
    // GEMM, cross-attention q projection, GEGLU GEMM) finishes the LayerNorm in ITS epilogue as r (acc - mu G') + C': no split-K slabs and 86
    // of the 102 row-kernel launches of an XL step less (239 launches instead of 325), the same algebra as the reference (goldens pass at the
    // same gates).  Needs gemm_pp bits 0 and 1 and a LayerNorm-algebra q projection; otherwise the step falls back to split-K slabs + the row kernel.
    int opt_zfuse = 1;
    // ... and the out-blocks' LN_2D([x | skip]) -> skip_linear (blocks.py:124-128) the same way (round 6, k_gemm_ks forms COPY2 / ZIN, gemm_ks.h): the statistics of the concatenation
    // are the sums of the halves'; the in-block that produces `skip` keeps them and writes bf16(skip g[D:]) into the right half of ITS out-block's operand (one operand buffer per
    // out-block), the MLP-out projection in front of the out-block runs un-split and writes bf16(x g[:D]) + statistics, skip_linear finishes the LayerNorm in its epilogue:
    // 14 split-K GEMMs + 14 row-kernel launches of an XL step become 14 un-split launches (225 launches instead of 239).  The ping-pong producer (M > kZBigM rows) has the same forms.
    // ControlNet residuals change the skips (skip + scale * residual) and take the row-kernel path.
    int opt_skip_z = 1;
    bool skip_z_usable() const { return opt_skip_z && !is_cn && nhalf > 0 && zparts() <= (ztile() == kZTile ? 16 : 8); }   // (statistics parts a lane group of the consumer covers)
    // GEGLU GEMM on the co-resident kernel (k_gemm_co, gemm_co.h: 4-wave workgroups with a 128 x 144 tile, TWO per CU, so that a workgroup's prologue and
    // epilogue run under its neighbour's K loop): 0 = never, 1 = above kCoM rows (batched prompts: the ping-pong kernel runs 4 rounds of workgroups there), 2 = always
    int opt_geglu_co = 0;
    int opt_qkv_co = 1;   // the same choice for the fused QKV GEMM (no k-split exchange in the 4-wave form).  Default 1 since round 6: four prompts per GPU 10.25 -> 10.07 ... 10.11 ms per step (-1.5 %),
                          // 768 workgroups = three per CU, two of them resident; at one prompt (192 workgroups, one per CU: nothing to overlap with) the 4-wave form loses 1.3 %
    // qkv_form: the form of the fused QKV GEMM on the ping-pong kernel, up to kCoM rows.  1 (default) = tile 67, the un-split 8-wave form (every wave walks every K tile of its
    // 16 rows x two heads: no exchange behind the loop, twice the fragment reads per K tile); 0 = tile 61, the k-split schedule (each wave group takes every other K tile, the
    // two partial tiles meet through the LDS behind the loop).  The option list is closed, so the form rides on `qkv_co`: adding 4 to its value selects form 0.
    // Default 1: at one prompt both the K loop and the epilogue of the launch are shorter in this form (stamps and the step-time comparison: DESIGN.md section 4)
    int opt_qkv_form = 1;
    int qkv_tile() const { return (opt_qkv_co == 2 || (opt_qkv_co == 1 && M > kCoM)) ? 66 : (opt_qkv_form == 1 && M <= kCoM) ? 67 : 61; }
    static constexpr int kCoM = 2048;
    int geglu_tile() const { return !(opt_gemm_pp & 1) ? 13 : (opt_geglu_co == 2 || (opt_geglu_co == 1 && M > kCoM)) ? 66 : 60; }
    // Single-key cross-attention shortcut (needs the LayerNorm-algebra path).  Softmax over ONE valid key is exactly 1, so for a batch element whose
    // context mask has a single valid key -- every unconditional row of classifier-free guidance: the T5 encoding of "" is one EOS token
    // (src/inference.py:44-50, attention.py:131-135) -- cross-attention returns v_key for every query and the cross-attention block adds the
    // step-invariant vector  d = W_o v_key + b_o  (blocks.py:147-151).  ezdit_prepare_context finds those batch elements and computes d per block
    // (zd); the attention-out projection adds it for their rows and emits the GEGLU GEMM's operand for them (k_gemm_ks DUAL / the ping-pong
    // producer), and cross-attention + its out-projection run over the remaining batch elements only -- which must be one contiguous range
    // [act_b0, act_b1), as in the CFG layout [cond.. | uncond..]; otherwise the general path runs.  Exact; the FLOP count of the bench line is NOT reduced for it.
    int opt_xkey1 = 1;
    bool xkey1 = false;          // set by ezdit_prepare_context: the bound context qualifies
    int act_b0 = 0, act_b1 = 0;  // batch elements that still run cross-attention
#ifdef EZ_DIAG
    int opt_zfake = 0;   // DIAGNOSTIC build only: the consumers run their LayerNorm-algebra variant on a FINISHED LayerNorm with neutral statistics (mean 0, variance 1, G' = 0, C' = bias): what the consumer side costs by itself
#endif
    // fused QKV GEMM (per-head LayerNorm + RoPE + the attention layouts in the epilogue, all in registers): 2 = ping-pong kernel (tiles of two whole heads),
    // 0 = no (odd head counts: fp32 projection + k_headnorm).  Static since round 6: the q / k rows of `wqkv` are PACKED in the RoPE-pair order the
    // register epilogue needs (EZDIT_T_QKROPE) whenever two heads tile the projection, so no option can route such a model to the unfused path.
    bool qk_perm() const { return D % (2 * dh) == 0; }
    int qkv_mode() const { return qk_perm() ? 2 : 0; }
    // the cross-attention kernel computes its own q projection (8-wave form: small grids, or forced by fuse_q2 = 2)
    // (nb = batch elements the cross-attention launch covers: with the single-key shortcut only the multi-key ones)
    bool q2_fused(int nb) const { return opt_fuse_q2 && ((long)nb * H * ((L + 63) / 64) <= 512 || opt_fuse_q2 == 2) && Lcp % 128 == 0; }
    // the LayerNorm-algebra path can run for the bound shape under the current options (its tables are built by ezdit_prepare_timesteps only then)
    bool zfuse_usable() const {
        // the cross-attention q projection must be one of the two LayerNorm-algebra consumers: fused into k_attn (small grids) or the ping-pong GEMM with the q epilogue
        return opt_zfuse && zparts() <= Z_MAXP && (opt_gemm_pp & 1) && qkv_mode() == 2 && (q2_fused(B) || opt_q2_pp);
    }
    int ztile() const { return (M > kZBigM && !per_row) ? 61 : kZTile; }   // producer of the LayerNorm algebra for the bound shape (the ping-pong producer shares one modulation slot per launch)
    int zwidth() const { return ztile() == 61 ? 144 : 96; }   // statistics part = the producer's tile width
    int zparts() const { return (D + zwidth() - 1) / zwidth(); }   // statistics parts of a D-wide producer
    // ---- layouts of the LayerNorm-algebra buffers.  carve (sizes), ezdit_prepare_timesteps (fill), forward_impl (use) and the EZ_DIAG blocks all go through these ----
    // G' / C' tables of one consumer: [slot][item][G' | C'][N] floats, item = block (out-block for zt_skip); the static tables (norm2 -> to_q, skip_norm -> skip_linear) have one slot
    struct ZTab { float *G, *C; long slot_stride; };
    static long ztab_floats(int items, long N) { return (long)items * 2 * N; }
    static ZTab ztab(float* base, int item, long N, long slot_stride) { float* G = base + ztab_floats(item, N); return {G, G + N, slot_stride}; }
    ZTab zt_qkv_of(int b) const { return ztab(p.zt_qkv, b, 3L * D, ztab_floats(nblk, 3L * D)); }
    ZTab zt_geglu_of(int b) const { return ztab(p.zt_geglu, b, 2L * I, ztab_floats(nblk, 2L * I)); }
    ZTab zt_q2_of(int b) const { return ztab(p.zt_q2, b, D, 0); }
    ZTab zt_skip_of(int j) const { return ztab(p.zt_skip, j, D, 0); }
    // partial statistics are part-major [part][Mp] float pairs in ranges of Z_MAXP parts: `zstat` holds two ranges (the second one: the x half in front of an
    // out-block, written by the MLP-out projection and read by skip_linear), `zstat_skip` one range per skip (kept from the in-block to its out-block)
    static size_t zrange(long Mp_) { return (size_t)Z_MAXP * Mp_; }
    float2* zstat_xhalf() const { return p.zstat + zrange(Mp); }
    float2* zstat_skip_of(int i) const { return p.zstat_skip + (size_t)i * zrange(Mp); }
    size_t ucat_elems(long Mp_) const { return (size_t)Mp_ * ld2D; }
    bf16_t* ucat_of(int j) const { return p.ucat_z + (size_t)j * ucat_elems(Mp); }   // operand [x | skip] of out-block j
    int opt_wt = 2;   // write-through (sc1) output stores: 0 off, 1 on, 2 = on while B L <= 2048.  The end-of-kernel write-back then has nothing left to flush: -3.5 % step time
                      // for one prompt (4.19 -> 4.04 ms), +1.4 % for four (the step is throughput-bound there and the stores compete with the loads)
    int wt() const { return opt_wt == 2 ? (B * L <= 2048) : opt_wt; }
    int opt_fuse_q2 = 1;                                                                  // cross-attn q projection inside k_attn (one prompt); 2 = at every grid size
    int opt_attn_nkh = 0;                                                                 // attention key sub-blocks per tile (0 = auto)
    int opt_q2_pp = 1;                                                                    // cross-attn q projection at large grids: ping-pong GEMM with the per-head LayerNorm in its epilogue (0: fp32 GEMM + normalisation inside k_attn)
    int opt_attn_xcd = 1;                                                                 // attention: all query tiles of a (batch, head) on one XCD
    // sliding-window self-attention (ezdit_set_attention_window): radius in frames, 0 = off.  Handle-scoped: neither ezdit_bind_workspace nor ezdit_sampler_begin
    // clears it.  A radius that covers the bound row (>= L - 1) masks nothing and launches the plain kernel: attn_band() is what the self-attention launch is given
    int attn_window = 0;
    int attn_band() const { return attn_window > 0 && attn_window < L - 1 ? attn_window : 0; }
    hipStream_t last_stream = nullptr;   // the stream of the latest forward / sampler call on this handle: what a setter without a stream argument asks about a capture
    // XCD affinity of the residual path at M <= 1024 (placement only, results bit-identical): gemm_panel = shapes (1 D x D, 2 skip, 4 MLP-out)
    // whose split-K GEMM puts ALL workgroups of an M tile on XCD tm % 8; row_affine = the row kernel processes row panel p on XCD p % 8, so
    // a panel's slabs, residual stream and LayerNorm output stay in one XCD's L2 (the L2 keeps its lines across kernel boundaries: a
    // same-XCD consumer of 4 MB is 2 us faster than a cross-XCD one, tools/microbench/xcd_bench.hip).  In situ on MI355X: XL 4.497 ->
    // 4.442 ms/step (+1.2 %, three boxes +0.9 ... +1.5 %), L 3.611 -> 3.518 (+2.7 %); the MLP-out shape gains nothing more and re-reads W
    // 8x (94 vs 66 MB fetched per launch), so it keeps the box placement.
    int opt_gemm_panel = 3, opt_row_affine = 1;
    // bf16 GEMM epilogues (GEGLU output, split-K slabs, q / k heads of the fused QKV GEMM) staged through LDS and written as whole 16-byte
    // chunks: in the MFMA C layout a lane owns one row, so a direct store instruction scatters 4-8 bytes into 32-64 different lines.
    // Bit-identical; XL 4.384 -> 4.281 ms/step (+2.4 %), L +1.8 % for the GEGLU / slab part alone.
    int opt_epi_lds = 1;
    // cross-attention q projection: two K tiles per ring slot, barrier and counted wait (a wave's work per K tile is 3 MFMAs: the loop is its
    // fixed cost per iteration).  Bit-identical; XL 4.319 -> 4.285 ms/step (+0.8 %), L +1.1 %.
    int opt_attn_xk2 = 1;
    // fused cross-attention with the LayerNorm algebra: query rows per workgroup (attn.hip k_attn QT): 0 = 32 when the 64-row grid is <= 128 workgroups (one prompt with the
    // single-key shortcut: 256 workgroups of 32 rows instead of 128 of 64), 64 / 32 = always
    int opt_attn_qtile = 0;
    int opt_cn_overlap = 1;                                                               // fused sampler: ControlNet branch on a side stream, concurrent with the backbone's in-blocks
    hipStream_t cn_stream = nullptr; hipEvent_t cn_fork = nullptr, cn_join = nullptr;
    int opt_row_variant = 1;                                                              // row kernel: 0 = one workgroup per row, 1 = one wave per row
    int debug_stop = 0;  // > 0: ezdit_forward returns after this many launches (unit-test hook)
    int opt_stamp_launch = -1;   // in-situ cycle stamps: the launch with this index of a forward writes them (ezdit_debug_gemm_timestamps buffer; eager launches only)
    int opt_trace_launches = 0;  // print 'index name' of every launch of a forward to stderr
    int steps_done = 0;  // host mirror of the device step counter (ezdit_sampler_run bounds check)
    int device = -1;     // device that was current at ezdit_create
    std::vector<BlkW> blk;
    WRef w_pe, w_fin;
    const float *b_pe = nullptr, *b_fin = nullptr, *w_mask_embed = nullptr, *w_fin_cw = nullptr, *w_fin_cb = nullptr;
    WsPtrs p;
    WRef wref(const std::string& name) const {
        const ezdit_param_info_t& pi = params[pidx.at(name)];
        WRef r; r.W = reinterpret_cast<const bf16_t*>(wblob + pi.offset); r.ld = (int)pi.ld; r.rows = (int)pi.rows_pad;
        return r;
    }

    template <typename T>
    const T* w(const std::string& name) const {
        auto it = pidx.find(name);
        if (it == pidx.end()) {
            fprintf(stderr, "ezdit: unknown parameter slot %s\n", name.c_str());
            abort();
        }
        return reinterpret_cast<const T*>(wblob + params[it->second].offset);
    }
    int pld(const std::string& name) const { return (int)params[pidx.at(name)].ld; }
    template <typename T>
    T* buf(const std::string& name) const {
        return reinterpret_cast<T*>(ws + bufs.at(name).off);
    }
};

// the captured step of `h` goes, and that of every backbone that has `h` attached as its ControlNet: their step embeds its kernels, arguments and buffers
static void drop_graph(ezdit_handle* h) {
    if (h->graph_exec) { (void)hipGraphExecDestroy(h->graph_exec); h->graph_exec = nullptr; }
    if (h->graph) { (void)hipGraphDestroy(h->graph); h->graph = nullptr; }
    for (ezdit_handle* u : h->cn_users) drop_graph(u);
}

namespace {

// ------------------------------------------------------------------------------------------------------
// parameter layout
// ------------------------------------------------------------------------------------------------------
void add_param(ezdit_handle* h, const std::string& name, std::vector<std::string> srcs, int dtype, long rows, long cols,
               int transform = EZDIT_T_NONE) {
    ezdit_param_info_t p;
    memset(&p, 0, sizeof p);
    snprintf(p.name, sizeof p.name, "%s", name.c_str());
    p.nsrc = (int)srcs.size();
    for (int i = 0; i < p.nsrc; ++i) snprintf(p.src[i], sizeof p.src[i], "%s", srcs[i].c_str());
    p.dtype = dtype;
    p.transform = transform;
    p.rows = rows;
    p.cols = cols;
    if (dtype == EZDIT_P_BF16) {
        p.rows_pad = rup(rows, 128);
        p.ld = rup(cols, 64);
    } else {
        p.rows_pad = rows;
        p.ld = cols;
    }
    p.offset = (int64_t)h->param_bytes;
    const size_t bytes = (size_t)p.rows_pad * p.ld * (dtype == EZDIT_P_BF16 ? 2 : 4);
    h->param_bytes += rup((long)bytes, 256);
    h->pidx[name] = (int)h->params.size();
    h->params.push_back(p);
}

std::string blk_prefix(const ezdit_handle* h, int b) {
    char s[64];
    if (h->is_cn) snprintf(s, sizeof s, "in_blocks.%d", b);  // DiTControlNet is not wrapped: no "model." prefix
    else if (b < h->nhalf) snprintf(s, sizeof s, "model.in_blocks.%d", b);
    else if (b == h->nhalf) snprintf(s, sizeof s, "model.mid_block");
    else snprintf(s, sizeof s, "model.out_blocks.%d", b - h->nhalf - 1);
    return s;
}
std::string bn(int b, const char* k) {
    char s[64];
    snprintf(s, sizeof s, "blk%d.%s", b, k);
    return s;
}

void build_params(ezdit_handle* h) {
    const long D = h->D, C = h->C, I = h->I, dh = h->dh, r6 = h->r6;
    const int F = EZDIT_P_F32, Bf = EZDIT_P_BF16;
    const std::string m = h->is_cn ? "" : "model.";
    if (!h->is_cn) add_param(h, "mask_embed", {"mask_embed"}, F, 1, C);
    add_param(h, "pe.w", {m + "patch_embed.proj.weight"}, Bf, D, h->Cin);
    add_param(h, "pe.b", {m + "patch_embed.proj.bias"}, F, 1, D);
    add_param(h, "te.w1", {m + "time_embed.mlp.0.weight"}, F, D, 256);
    add_param(h, "te.b1", {m + "time_embed.mlp.0.bias"}, F, 1, D);
    add_param(h, "te.w2", {m + "time_embed.mlp.2.weight"}, F, D, D);
    add_param(h, "te.b2", {m + "time_embed.mlp.2.bias"}, F, 1, D);
    add_param(h, "ada.w", {m + "time_ada.weight"}, F, 6 * D, D);
    add_param(h, "ada.b", {m + "time_ada.bias"}, F, 1, 6 * D);
    add_param(h, "ce.w1", {m + "context_embed.0.weight"}, Bf, D, h->Cctx);
    add_param(h, "ce.b1", {m + "context_embed.0.bias"}, F, 1, D);
    add_param(h, "ce.w2", {m + "context_embed.2.weight"}, Bf, D, D);
    add_param(h, "ce.b2", {m + "context_embed.2.bias"}, F, 1, D);
    if (!h->is_cn) {
        add_param(h, "adaf.w", {"model.time_ada_final.weight"}, F, 2 * D, D);
        add_param(h, "adaf.b", {"model.time_ada_final.bias"}, F, 1, 2 * D);
        add_param(h, "fin.nw", {"model.final_block.norm.weight"}, F, 1, D);
        add_param(h, "fin.nb", {"model.final_block.norm.bias"}, F, 1, D);
        add_param(h, "fin.w", {"model.final_block.linear.weight"}, Bf, C, D);
        add_param(h, "fin.b", {"model.final_block.linear.bias"}, F, 1, C);
        add_param(h, "fin.cw", {"model.final_block.final_layer.weight"}, F, C, C * 3);
        add_param(h, "fin.cb", {"model.final_block.final_layer.bias"}, F, 1, C);
    } else {
        // DiTControlNetEmbed (controlnet.py:10-39) and the zero-initialised output Linears (:228-234)
        const long c0 = h->c0, c0m = h->c0m, c1 = h->c1, ci = h->cfg.cond_in;
        add_param(h, "cn.cin.w", {"controlnet_pre.conv_in.weight"}, F, c0, ci);
        add_param(h, "cn.cin.b", {"controlnet_pre.conv_in.bias"}, F, 1, c0);
        if (h->cfg.cond_mask) add_param(h, "cn.mask_embed", {"controlnet_pre.mask_embed"}, F, 1, c0);
        add_param(h, "cn.c0.w", {"controlnet_pre.blocks.0.0.weight"}, F, c0m, c0m * 3);
        add_param(h, "cn.c0.b", {"controlnet_pre.blocks.0.0.bias"}, F, 1, c0m);
        add_param(h, "cn.c1.w", {"controlnet_pre.blocks.0.2.weight"}, F, c1, c0m * 3);
        add_param(h, "cn.c1.b", {"controlnet_pre.blocks.0.2.bias"}, F, 1, c1);
        add_param(h, "cn.cout.w", {"controlnet_pre.conv_out.weight"}, F, D, c1);
        add_param(h, "cn.cout.b", {"controlnet_pre.conv_out.bias"}, F, 1, D);
        for (int b = 0; b < h->nblk; ++b) {
            char k[64];
            snprintf(k, sizeof k, "controlnet_zero_blocks.%d", b);
            add_param(h, bn(b, "zw"), {std::string(k) + ".weight"}, Bf, D, D);
            add_param(h, bn(b, "zb"), {std::string(k) + ".bias"}, F, 1, D);
        }
    }
    // per-block parameters, kind-major so that one kind is a constant-stride array over blocks
    struct V { const char* name; const char* key; long n; };
    const V vecs[] = {
        {"n1w", "norm1.weight", D}, {"n1b", "norm1.bias", D}, {"n2w", "norm2.weight", D}, {"n2b", "norm2.bias", D},
        {"n3w", "norm3.weight", D}, {"n3b", "norm3.bias", D}, {"ncw", "norm_context.weight", D},
        {"ncb", "norm_context.bias", D},
        {"a.qnw", "attn.norm_q.weight", dh}, {"a.qnb", "attn.norm_q.bias", dh}, {"a.knw", "attn.norm_k.weight", dh},
        {"a.knb", "attn.norm_k.bias", dh}, {"c.qnw", "cross_attn.norm_q.weight", dh},
        {"c.qnb", "cross_attn.norm_q.bias", dh}, {"c.knw", "cross_attn.norm_k.weight", dh},
        {"c.knb", "cross_attn.norm_k.bias", dh},
        {"bo", "attn.proj.bias", D}, {"bo2", "cross_attn.proj.bias", D}, {"b2", "mlp.net.2.bias", D},
        {"table", "adaln.scale_shift_table", 6 * D},
    };
    for (const V& v : vecs)
        for (int b = 0; b < h->nblk; ++b) add_param(h, bn(b, v.name), {blk_prefix(h, b) + "." + v.key}, F, 1, v.n);
    // per-STEP matrices of one block are contiguous
    for (int b = 0; b < h->nblk; ++b) {
        const std::string p = blk_prefix(h, b);
        add_param(h, bn(b, "b1"), {p + ".mlp.net.0.proj.bias"}, F, 1, 2 * I, EZDIT_T_GEGLU8);
        if (b > h->nhalf) {
            add_param(h, bn(b, "snw"), {p + ".skip_norm.weight"}, F, 1, 2 * D);
            add_param(h, bn(b, "snb"), {p + ".skip_norm.bias"}, F, 1, 2 * D);
            add_param(h, bn(b, "wskip"), {p + ".skip_linear.weight"}, Bf, D, 2 * D);
            add_param(h, bn(b, "bskip"), {p + ".skip_linear.bias"}, F, 1, D);
        }
        add_param(h, bn(b, "wqkv"), {p + ".attn.to_q.weight", p + ".attn.to_k.weight", p + ".attn.to_v.weight"}, Bf, 3 * D, D, h->qk_perm() ? EZDIT_T_QKROPE : EZDIT_T_NONE);
        add_param(h, bn(b, "wo"), {p + ".attn.proj.weight"}, Bf, D, D);
        add_param(h, bn(b, "wq2"), {p + ".cross_attn.to_q.weight"}, Bf, D, D);
        add_param(h, bn(b, "wo2"), {p + ".cross_attn.proj.weight"}, Bf, D, D);
        add_param(h, bn(b, "w1"), {p + ".mlp.net.0.proj.weight"}, Bf, 2 * I, D, EZDIT_T_GEGLU8);
        add_param(h, bn(b, "w2"), {p + ".mlp.net.2.weight"}, Bf, D, I);
    }
    // used once per CALL only (context K/V projection, AdaLN-SOLA low-rank factors)
    for (int b = 0; b < h->nblk; ++b) {
        const std::string p = blk_prefix(h, b);
        add_param(h, bn(b, "wkv2"), {p + ".cross_attn.to_k.weight", p + ".cross_attn.to_v.weight"}, Bf, 2 * D, D);
        add_param(h, bn(b, "lora_a"), {p + ".adaln.lora_a.weight"}, F, r6, D);
        add_param(h, bn(b, "lora_b"), {p + ".adaln.lora_b.weight"}, F, 6 * D, r6);
    }
}

// ------------------------------------------------------------------------------------------------------
// workspace carving
// ------------------------------------------------------------------------------------------------------
size_t carve(const ezdit_handle* h, int B, int L, int Lc, int n_slots, std::map<std::string, Buf>* out) {
    size_t off = 0;
    auto add = [&](const char* name, size_t bytes) {
        Buf b;
        b.off = off;
        b.bytes = bytes;
        if (out) (*out)[name] = b;
        off += (size_t)rup((long)bytes, 256);
    };
    const long D = h->D, C = h->C, H = h->H;
    const long M = (long)B * L, Mp = rup(M, 128), Lp = rup(L, 128), Lcp = rup(Lc, 128);  // attention stages 64- or 128-key tiles
    const long Mc = (long)B * Lc, Mcp = rup(Mc, 128);
    const int nblk = h->nblk;
    add("ints", 256 * sizeof(int));                       // [0] cur_step, [8] CFG arrival counter, [16..] row_slot (<= 240 rows)
    add("rope_cos", (size_t)h->cfg.max_len * (h->dh / 2) * 4);
    add("rope_sin", (size_t)h->cfg.max_len * (h->dh / 2) * 4);
    add("coef", (size_t)(n_slots > 0 ? n_slots : 1) * 8 * 4);
    add("cfgpart", (size_t)B * 64 * 4 * 4);
    add("sink", 256);
    if (h->is_cn) {
        const long Lc2 = 2L * L;
        add("cn_e0", (size_t)B * h->c0 * Lc2 * 4);
        add("cn_e1", (size_t)B * h->c0m * Lc2 * 4);
        add("cn_e2", (size_t)B * h->c1 * L * 4);
        add("cembed", (size_t)rup((long)B * L, 128) * h->D * 4);
        add("cnres", (size_t)h->nhalf * rup((long)B * L, 128) * h->D * 4);
        add("skipbf", (size_t)rup((long)B * L, 128) * h->ldD * 2);
    }
    add("ape", Mp * h->ldPE * 2);
    add("h", Mp * D * 4);
    add("skips", (size_t)h->nhalf * Mp * D * 4);
    add("u", Mp * h->ldD * 2);
    add("ucat", Mp * h->ld2D * 2);                        // LN_2D([x | skip]) of the out-blocks: its own buffer, because the skip GEMM that reads it
                                                          // writes `u` from inside the same launch (fused row operator)
    add("qkv", Mp * 3 * D * 4);
    add("q", (size_t)B * H * Lp * h->DQK * 2);
    add("k", (size_t)B * H * Lp * h->DQK * 2);
    add("v", (size_t)B * H * Lp * h->DV * 2);
    add("ao", Mp * h->ldD * 2);
    add("act", Mp * h->ldI * 2);
    add("part", (size_t)8 * Mp * D * 4);
    add("y", Mp * C * 4);
    add("pred", (size_t)B * C * L * 4);
    // context (step invariant)
    add("kmask", rup(Mc, 256));
    add("ctx_bf", Mcp * h->ldCtx * 2);
    add("c1", Mcp * D * 4);
    add("c1b", Mcp * h->ldD * 2);
    add("c2", Mcp * D * 4);
    add("cu", Mcp * h->ldD * 2);
    add("ckv", Mcp * 2 * D * 4);
    add("kc", (size_t)nblk * B * H * Lcp * h->DQK * 2);
    add("vc", (size_t)nblk * B * H * Lcp * h->DV * 2);
    // time path
    const long ns = n_slots > 0 ? n_slots : 1;
    add("ts", ns * 4);
    add("t1", ns * D * 4);
    add("tt", ns * D * 4);
    add("ada", ns * 6 * D * 4);
    add("adaf", ns * 2 * D * 4);
    add("la", ns * h->r6 * 4);
    add("lora", ns * nblk * 6 * D * 4);
    add("mod", ns * nblk * 6 * D * 4);
    add("modf", ns * 2 * D * 4);
    // LayerNorm algebra: partial row statistics (chunks of 64 columns, up to the 2D-wide concat), G' / C' tables per modulation slot
    {
        const long I2 = 2L * h->I, N3 = 3L * D, nmax = I2 > N3 ? I2 : N3;
        const size_t zr = ezdit_handle::zrange(Mp), z64 = (size_t)Mp * ((2 * D + 63) / 64), nskip = h->nhalf > 0 ? h->nhalf : 1;
        add("zstat", (z64 > 2 * zr ? z64 : 2 * zr) * 8);   // two part ranges of Z_MAXP: the second one holds the statistics of the x half in front of an out-block (skip_z)
        add("zt_qkv", (size_t)ns * ezdit_handle::ztab_floats(nblk, N3) * 4);
        add("zt_geglu", (size_t)ns * ezdit_handle::ztab_floats(nblk, I2) * 4);
        add("zt_q2", (size_t)ezdit_handle::ztab_floats(nblk, D) * 4);
        add("zd", (size_t)nblk * B * D * 4);
        add("zA", (size_t)rup(4 * ns, 128) * h->ldD * 2);
        add("ztmp", (size_t)rup(4 * ns, 128) * nmax * 4);
#ifdef EZ_DIAG
        add("zneutral", zr * 8);
        add("zzeros", (size_t)nmax * 4);
#endif
        // skip path by the LayerNorm algebra (opt_skip_z), BEHIND everything else: the buffers above keep the offsets -- the relative placement in the HBM channels -- the
        // round's measurements were made with.  One [x | skip] operand per out-block (the in-block fills the right half long before the out-block runs), the skips' statistics, static tables
        add("ucat_z", (h->is_cn ? 1 : nskip) * h->ucat_elems(Mp) * 2);
        add("zstat_skip", nskip * zr * 8);
        add("zt_skip", (size_t)ezdit_handle::ztab_floats((int)nskip, D) * 4);
        add("lens", 256 * sizeof(int));   // per-batch-element valid frames of a padded batch (B <= 240), behind everything else for the same reason
        add("spg", (size_t)ezdit_handle::sp_cap(B) * 2 * 4);        // per-sample sampler settings, at the very end (no existing buffer moves): at most
        add("spc", (size_t)ns * ezdit_handle::sp_cap(B) * 8 * 4);   // n_slots * (B / 2 + 1) * 32 bytes + 2 KB more workspace than without them
        add("cns", 256 * sizeof(float));   // per-batch-element conditioning_scale (B <= 240), behind `lens` and the sample tables for the same reason: no existing buffer moves
        add("start", 256 * sizeof(int));   // per-sample first step (ezdit_sampler_set_start; P <= B <= 240), at the very end for the same reason: 1 KB
        add("canvas", 256 * sizeof(int));  // per-window first canvas frame (ezdit_sampler_set_canvas; P <= B <= 240), behind `start` for the same reason: 1 KB
        add("tlb", (size_t)B * (Lcp / 128) * L * 4);     // prompt timeline (ezdit_set_context_weights): one score bias per (batch element, prompt, frame) and the prompts' frame
        add("tlsup", (size_t)B * (Lcp / 128) * 8);       // supports, behind `canvas` for the same reason: B L 4 bytes at one prompt
        add("cw", (size_t)B * sizeof(float));            // weights of composed guidance [P][K], P K < B = (K + 1) P; at the very end for the same reason
        add("kbias", (size_t)B * Lcp * 4);               // prompt emphasis (ezdit_set_context_token_weights): one score bias per context key, behind `cw` for the same reason
        add("apg", (size_t)B * 4 * sizeof(float));       // adaptive projected guidance (ezdit_sampler_set_apg): [P][4], P <= B; at the very end for the same reason: 16 B bytes
    }
    return off;
}

// ------------------------------------------------------------------------------------------------------
// launch helpers
// ------------------------------------------------------------------------------------------------------
struct Ctx {
    ezdit_handle* h;
    hipStream_t st;
    const int* cur = nullptr; const int* row_slot = nullptr;   // modulation slot of this forward (a ControlNet attached to the fused sampler reads the BACKBONE's step counter)
    // first launch failure of this call (hipGetLastError after EVERY launch: a rejected launch -- LDS limit, bad grid,
    // unsupported fused configuration -- must surface as an error code, never as stale numbers)
    hipError_t err = hipSuccess;
    int rc = EZDIT_OK;
    const char* where = nullptr;
    std::string why;   // the reason the refusing launcher gave (ez_refuse), for the message
    // cycle-stamp buffer for the launch about to be issued (nullptr unless the 'stamp_launch' option selects it)
    unsigned long long* stamps() const { return (g_gemm_ts && h->launches == h->opt_stamp_launch) ? g_gemm_ts : nullptr; }
    void launched(const char* what, int launch_rc = 0) {
        if (h->opt_trace_launches) fprintf(stderr, "launch %d %s\n", h->launches, what);
        h->launches++;
        if (launch_rc != 0 && rc == EZDIT_OK) { rc = launch_rc; where = what; why = take_refusal(); }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess && err == hipSuccess) { err = e; where = what; }
    }
    bool bad() const { return err != hipSuccess || rc != EZDIT_OK; }
    int result() const {
        if (rc != EZDIT_OK) return fail(rc, "%s: configuration not supported by the HIP kernels%s", where ? where : "?", why.c_str());
        if (err != hipSuccess) return fail(EZDIT_E_HIP, "launch of %s failed: %s", where ? where : "?", hipGetErrorString(err));
        return EZDIT_OK;
    }
};

// LayerNorm-algebra input of a consumer GEMM (EPI_QKV, EPI_GEGLU): the operand is A' = bf16(x g) and the epilogue finishes the LayerNorm from the tables `t` and the
// partial statistics `stat` (null = plain GEMM on a finished LayerNorm).  A launch over a row sub-range starts at row row0 = batch element b0 (statistics / per-row slot offsets)
struct ZIn {
    ezdit_handle::ZTab t{};
    const float2* stat = nullptr;
    int row0 = 0, b0 = 0;
};

// hn: EPI_QKV epilogue arguments; panel: panel placement of a split-K GEMM (GemmArgs.xcd_panel)
void gemm(Ctx& c, const bf16_t* A, int lda, const WRef& w, const float* bias, void* out, int ldo, int M, int N,
          int epi, int tile, const HeadNormArgs* hn = nullptr, const ZIn& z = ZIn{}, int splitk = 1, long slab = 0, bool panel = false) {
    ezdit_handle* h = c.h;
    GemmArgs g;
    memset(&g, 0, sizeof g);
    g.A = A;
    g.lda = lda;
    g.W = w.W;
    g.ldw = w.ld;
    g.wrows = w.rows;
    g.bias = bias;
    g.out = out;
    g.ldo = ldo;
    g.slab_stride = slab;
    g.M = M;
    g.N = N;
    g.K = w.ld;
    g.splitk = splitk;
    g.epi = epi;
    g.tile = tile;
    g.xcd_map = 1;
    g.part_bf16 = (epi == EPI_PARTIAL) ? 1 : 0;   // split-K slabs in bf16
    g.wt = h->wt();
    g.epi_lds = h->opt_epi_lds;
    g.rows_per_b = 1;
    if (hn) g.hn = *hn;
    g.xcd_panel = panel ? 1 : 0;
#ifdef EZ_DIAG
    if (!z.stat && h->opt_zfake && (epi == EPI_QKV || epi == EPI_GEGLU) && (tile == 60 || tile == 61 || tile == 66) && h->zparts() <= Z_MAXP) {
        g.zw = h->zwidth(); g.zstat_in = h->buf<float2>("zneutral"); g.zs_stride = h->Mp; g.zparts = h->zparts(); g.zD = h->D;
        g.zG = h->buf<float>("zzeros"); g.zC = bias ? bias : g.zG; g.zt_slot_stride = 0; g.zeps = 1e-5f; g.rows_per_b = h->L;
    }
#endif
    if (z.stat) {
        g.zw = h->zwidth(); g.zstat_in = z.stat + z.row0; g.zs_stride = h->Mp; g.zparts = h->zparts(); g.zD = h->D; g.zG = z.t.G; g.zC = z.t.C; g.zt_slot_stride = z.t.slot_stride; g.zeps = 1e-5f;
        g.cur_step = c.cur ? c.cur : h->p.ints; g.row_slot = c.cur ? c.row_slot : (h->per_row ? h->p.ints + 16 : nullptr); g.rows_per_b = h->L;
        if (g.row_slot) g.row_slot += z.b0;
    }
    g.ts = c.stamps(); g.ts_cap = g_gemm_ts_cap;
    c.launched(epi == EPI_GEGLU ? "k_gemm (GEGLU)" : epi == EPI_QKV ? "k_gemm (QKV)" : epi == EPI_PARTIAL ? "k_gemm (split-K slabs)" : "k_gemm", launch_gemm(g, c.st));
}

// Tile / split-K choices: measured in situ on MI355X (DESIGN.md section 4 has the numbers); fixed since round 5 except tile_partial.
int tile_for(const ezdit_handle* h, int M, bool partial) {
    if (M <= 2048) return partial ? h->opt_tile_partial : ezdit_handle::kTileF32;
    return partial ? ezdit_handle::kTilePartialBig : ezdit_handle::kTileF32;
}

int pick_splitk(const ezdit_handle* h, int M, int N, int K) {
    const int tiles = ((M + 127) / 128) * ((N + 63) / 64);
    const int nk = K / 64;
    if (M > 2048) return ezdit_handle::kSplitBig < nk ? ezdit_handle::kSplitBig : nk;
    if (tiles >= 256) return 1;
    return ezdit_handle::kSplitK < nk ? ezdit_handle::kSplitK : nk;  // fewer slabs = less row-kernel traffic
}

// residual GEMM: part = A . W^T as split-K slabs (reduced by the row kernel that follows)
int gemm_partial(Ctx& c, const bf16_t* A, int lda, const WRef& w, int M, int N) {
    ezdit_handle* h = c.h;
    const int K = w.ld;
    const int s = pick_splitk(h, M, N, K);
    const int shape_bit = K >= 4 * N ? 4 : K >= 2 * N ? 2 : 1;
    const bool panel = (h->opt_gemm_panel & shape_bit) && M <= 1024;
    gemm(c, A, lda, w, nullptr, h->p.part, h->D, M, N, EPI_PARTIAL, tile_for(h, M, true), nullptr, ZIn{}, s, (long)h->Mp * h->D, panel);
    return s;
}

// Base arguments of an un-split residual launch (EPI_RESID):  h_out = h_in + gate * (A . W^T + bias),  zu = bf16(h_out * zg),  zstat_out [N tiles][zs_stride] = the partial
// LayerNorm statistics of h_out.  The step's edges (forward_impl) and the stand-alone hooks (ezdit_test_resid*) all start from this one and add only what their form needs
GemmArgs resid_args(int tile, const bf16_t* A, int lda, const bf16_t* W, int ldw, int wrows, const float* bias, const float* h_in, const float* gate, const float* zg,
                    float* h_out, bf16_t* zu, int ld_zu, float2* zstat_out, long zs_stride, int M, int N, int K) {
    GemmArgs g;
    memset(&g, 0, sizeof g);
    g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.wrows = wrows; g.bias = bias;
    g.out = h_out; g.ldo = N; g.M = M; g.N = N; g.K = K; g.splitk = 1; g.epi = EPI_RESID; g.tile = tile; g.xcd_map = 1;
    g.resid = h_in; g.ldr = N; g.gate = gate; g.rows_per_b = 1;
    g.zu = zu; g.ld_zu = ld_zu; g.zg = zg; g.zstat_out = zstat_out; g.zs_stride = zs_stride;
    return g;
}

// One residual edge of the step:  h_out = h_in + gate * (A . W^T + bias),  then the LayerNorm (gain ln_g, shift ln_c) in front of the GEMM that reads the result.
// A site of forward_impl fills it once; forward_impl's edge() picks the form and the launches.  Lives on the stack; `name` is a literal.
struct Edge {
    const char* name = nullptr;   // launch name of the un-split form
    // the reader finishes the LayerNorm in its own epilogue (LayerNorm algebra): ONE un-split launch that also emits A' = bf16(h_out ln_g) and partial statistics.
    // Otherwise split-K slabs + the row kernel, which writes the finished LayerNorm
    bool algebra = false;
    const bf16_t* A = nullptr; int lda = 0; const WRef* w = nullptr; const float* bias = nullptr;
    const float* h_in = nullptr; float* h_out = nullptr;   // h_in null: no residual; h_out null: the fp32 stream is not stored
    const float* gate = nullptr; long gate_stride = 0;     // null = 1; per modulation slot when the stride is non-zero
    const float *ln_g = nullptr, *ln_c = nullptr; long ln_stride = 0;   // null ln_g: no LayerNorm follows
    // ---- the un-split forms' extras (GemmArgs: DUAL / COPY2 / ZIN) ----
    int b0 = 0, nb = -1;     // the launch covers the batch elements [b0, b0 + nb) only (nb < 0: all)
    int dual_blk = -1;       // >= 0: DUAL form with the constant cross-attention-out vectors of this block (GemmArgs.zd)
    bf16_t* zu = nullptr; int ld_zu = 0;   // operand buffer instead of `u` ...
    float2* zstat_out = nullptr;           // ... and statistics instead of the shared buffer (whole-batch launches only)
    bf16_t* zu2 = nullptr; int ld_zu2 = 0; const float* zg2 = nullptr;          // COPY2: a second operand bf16(h_out zg2)
    const float2 *zin = nullptr, *zin2 = nullptr; const float* zG = nullptr;    // ZIN: A = bf16([x | skip] g) with the halves' statistics; G' (C' goes in `bias`)
    // ---- the row-kernel form's extras: LayerNorm over [h_out | skip + cn_scale cn] (long skip connection, ControlNet residual) ----
    const float *skip = nullptr, *cn = nullptr;
};

void resolve_weights(ezdit_handle* h) {
    h->blk.assign(h->nblk, BlkW{});
    for (int b = 0; b < h->nblk; ++b) {
        BlkW& k = h->blk[b];
        k.aqnw = h->w<float>(bn(b, "a.qnw")); k.aqnb = h->w<float>(bn(b, "a.qnb"));
        k.aknw = h->w<float>(bn(b, "a.knw")); k.aknb = h->w<float>(bn(b, "a.knb"));
        k.cqnw = h->w<float>(bn(b, "c.qnw")); k.cqnb = h->w<float>(bn(b, "c.qnb"));
        k.bo = h->w<float>(bn(b, "bo")); k.bo2 = h->w<float>(bn(b, "bo2")); k.b2 = h->w<float>(bn(b, "b2"));
        k.n2w = h->w<float>(bn(b, "n2w")); k.n2b = h->w<float>(bn(b, "n2b"));
        k.b1 = h->w<float>(bn(b, "b1"));
        k.wqkv = h->wref(bn(b, "wqkv")); k.wo = h->wref(bn(b, "wo")); k.wq2 = h->wref(bn(b, "wq2"));
        k.wo2 = h->wref(bn(b, "wo2")); k.w1 = h->wref(bn(b, "w1")); k.w2 = h->wref(bn(b, "w2"));
        if (!h->is_cn && b > h->nhalf) {
            k.snw = h->w<float>(bn(b, "snw")); k.snb = h->w<float>(bn(b, "snb"));
            k.wskip = h->wref(bn(b, "wskip")); k.bskip = h->w<float>(bn(b, "bskip"));
        }
        if (h->is_cn) { k.zw = h->wref(bn(b, "zw")); k.zb = h->w<float>(bn(b, "zb")); }
    }
    h->w_pe = h->wref("pe.w"); h->b_pe = h->w<float>("pe.b");
    if (!h->is_cn) {
        h->w_fin = h->wref("fin.w"); h->b_fin = h->w<float>("fin.b");
        h->w_fin_cw = h->w<float>("fin.cw"); h->w_fin_cb = h->w<float>("fin.cb");
        h->w_mask_embed = h->w<float>("mask_embed");
    }
}

void resolve_workspace(ezdit_handle* h) {
    WsPtrs& p = h->p;
    memset(&p, 0, sizeof p);
    p.ints = h->buf<int>("ints"); p.rope_cos = h->buf<float>("rope_cos"); p.rope_sin = h->buf<float>("rope_sin");
    p.coef = h->buf<float>("coef"); p.cfgpart = h->buf<float>("cfgpart");
    p.ape = h->buf<bf16_t>("ape"); p.h = h->buf<float>("h"); p.skips = h->buf<float>("skips"); p.u = h->buf<bf16_t>("u"); p.ucat = h->buf<bf16_t>("ucat");
    p.qkv = h->buf<float>("qkv"); p.q = h->buf<bf16_t>("q"); p.k = h->buf<bf16_t>("k"); p.v = h->buf<bf16_t>("v");
    p.ao = h->buf<bf16_t>("ao"); p.act = h->buf<bf16_t>("act"); p.part = h->buf<float>("part"); p.y = h->buf<float>("y");
    p.pred = h->buf<float>("pred"); p.kmask = h->buf<uint8_t>("kmask"); p.kc = h->buf<bf16_t>("kc"); p.vc = h->buf<bf16_t>("vc");
    p.mod = h->buf<float>("mod"); p.modf = h->buf<float>("modf");
    p.zd = h->buf<float>("zd"); p.spc = h->buf<float>("spc");
    h->lens.dev = h->buf<int>("lens"); h->cns.dev = h->buf<float>("cns"); h->sp.dev = h->buf<float>("spg"); h->coef.dev = p.coef;
    h->start.dev = h->buf<int>("start"); h->canvas.dev = h->buf<int>("canvas");
    h->tl.dev = h->buf<float>("tlb"); h->tlsup = h->buf<int2>("tlsup");
    h->cw.dev = h->buf<float>("cw");
    h->tw.dev = h->buf<float>("kbias");
    h->apg.dev = h->buf<float>("apg");
    p.zstat = h->buf<float2>("zstat"); p.zt_qkv = h->buf<float>("zt_qkv"); p.zt_geglu = h->buf<float>("zt_geglu"); p.zt_q2 = h->buf<float>("zt_q2");
    p.zstat_skip = h->buf<float2>("zstat_skip"); p.zt_skip = h->buf<float>("zt_skip"); p.ucat_z = h->buf<bf16_t>("ucat_z");
    if (h->is_cn) { p.cembed = h->buf<float>("cembed"); p.cnres = h->buf<float>("cnres"); p.skipbf = h->buf<bf16_t>("skipbf"); }
}

// the launch of a stand-alone hook: a stale error of an earlier call is not this one's; a configuration the launcher refuses (non-zero return) and a failed launch are reported
template <typename Launch>
int hook_launch(const char* kernel, const char* config, Launch launch) {
    (void)hipGetLastError();
    g_refusal.clear();
    if (launch()) return fail(EZDIT_E_UNSUPPORTED, "%s not supported%s", config, take_refusal().c_str());
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(EZDIT_E_HIP, "launch of %s failed: %s", kernel, hipGetErrorString(e));
    return EZDIT_OK;
}

// what the three stand-alone forms of the update share: one step on the caller's tensors, no device step counter, the whole row when there are no lengths
CfgDdimArgs standalone_step(const float* pred, float* latents, const float* noise, int P, int n, const int32_t* lens = nullptr, int L = 0) {
    CfgDdimArgs a;
    a.pred = pred; a.latents = latents; a.noise = noise;
    a.P = P; a.n = n;
    a.lens = lens; a.L = lens ? L : n;
    return a;
}

// ------------------------------------------------------------------------------------------------------
// run-time tables of the step: what every setter shares
// ------------------------------------------------------------------------------------------------------
enum class Needs { Bound, BoundBackbone, Begun };   // a bound workspace (on a backbone handle), or a sampler call begun on it

// The checks every table setter `fn` begins with: a handle, the state the table lives in and a stream that is not being captured
int setter_checks(const ezdit_handle* h, const char* fn, Needs needs, hipStream_t st) {
    if (!h) return fail(EZDIT_E_INVALID, "null handle");
    if (needs == Needs::BoundBackbone && h->is_cn) return fail(EZDIT_E_INVALID, "first argument must be a backbone handle");
    if (needs == Needs::Begun ? !h->latents : !h->ws) return fail(EZDIT_E_STATE, needs == Needs::Begun ? "ezdit_sampler_begin first" : "bind workspace first");
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
    if (cs != hipStreamCaptureStatusNone) return fail(EZDIT_E_STATE, "%s inside a stream capture (it uploads from host memory and waits)", fn);
    return EZDIT_OK;
}

// New values `v` of a table: they become its host mirror and go to the device.  The copy is asynchronous and reads the mirror, so the stream is drained on both
// sides: an earlier upload may still be reading the mirror that is replaced, and the next one may replace it right after this call.  With `tail` given the
// first `head` elements go to t.dev and the rest to `tail` (the sample table's two device arrays)
template <typename T>
int upload_table(Table<T>& t, std::vector<T> v, hipStream_t st, size_t head = 0, T* tail = nullptr) {
    HIPCHK(hipStreamSynchronize(st));
    t.host.swap(v);
    if (!tail) head = t.host.size();
    HIPCHK(hipMemcpyAsync(t.dev, t.host.data(), head * sizeof(T), hipMemcpyHostToDevice, st));
    if (tail) HIPCHK(hipMemcpyAsync(tail, t.host.data() + head, (t.host.size() - head) * sizeof(T), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    return EZDIT_OK;
}

// n values for B batch rows: row b takes src[b % n], the rule by which batch row b reads latent row b % x_rows (a CFG pair shares its value)
template <typename T>
std::vector<T> per_row(const T* src, int n, int B) {
    std::vector<T> v((size_t)B);
    for (int b = 0; b < B; ++b) v[b] = src[b % n];
    return v;
}

// the per-sample lengths of a call expanded to the B rows of the bound batch, or the refusal of a table that does not fit it
int expand_lengths(const ezdit_handle* h, const int32_t* lengths, int n, std::vector<int>* v) {
    if (n < 0 || n > h->B || h->B % n) return fail(EZDIT_E_INVALID, "%d lengths do not divide B = %d", n, h->B);
    for (int i = 0; i < n; ++i)
        if (lengths[i] < 1 || lengths[i] > h->L) return fail(EZDIT_E_INVALID, "lengths[%d] = %d outside [1, L = %d]", i, (int)lengths[i], h->L);
    *v = per_row<int>(lengths, n, h->B);
    return EZDIT_OK;
}

// The prompt timeline of B batch elements (include/ezdit.h, ezdit_set_context_weights): natural weights w [B][S][L] -> the table the TL form of k_attn reads,
// [B][S][L] biases log2(w / max_s w) (TL_OFF for a weight of 0; the dominant prompt of a frame has exactly 0) followed by [B][S] supports (first, last + 1 frame of
// weight > 0) as bit copies.  lens (nullable, [B]): the frames that exist; a frame beyond takes the last existing frame's column, whatever the caller left there, and
// stands in the supports with it: a workgroup whose queries are all padding then walks the prompts of the last frame and its rows stay FINITE (a padding row that meets no
// weighted key would end as 0 / 0, and the next block's self-attention passes masked keys through P . V with P = 0: 0 * NaN = NaN).  The range of a workgroup that holds
// the last existing frame is not widened by this.  mask (nullable = every key valid, [B][128 S]): every existing frame needs a weight > 0 on a prompt that has a valid key -- its softmax has no
// term otherwise -- which covers the single-key batch elements of the shortcut as well (their constant output is their prompt at every frame)
int timeline_table(const float* w, int B, int S, int L, const int* lens, const uint8_t* mask, std::vector<float>* out) {
    const size_t nb = (size_t)B * S * L;
    out->assign(nb + (size_t)B * S * 2, 0.f);
    std::vector<int> sup((size_t)B * S * 2, 0);
    for (int b = 0; b < B; ++b) {
        const int len = lens ? lens[b] : L;
        bool has_key[TL_MAXS];
        for (int s = 0; s < S; ++s) {
            has_key[s] = !mask;
            for (int j = 0; mask && j < 128 && !has_key[s]; ++j) has_key[s] = mask[((size_t)b * S + s) * 128 + j] != 0;
        }
        for (int i = 0; i < L; ++i) {
            const int f = i < len ? i : len - 1;   // (a frame beyond the length: the last one that exists)
            double mx = 0.0;
            bool seen = false;
            for (int s = 0; s < S; ++s) {
                const float x = w[((size_t)b * S + s) * L + f];
                if (!std::isfinite(x) || x < 0.f) return fail(EZDIT_E_INVALID, "weights[%d][%d][%d] = %g: a weight is finite and >= 0", b, s, f, (double)x);
                mx = x > mx ? x : mx;
                seen = seen || (x > 0.f && has_key[s]);
            }
            if (!seen) return fail(EZDIT_E_INVALID, "frame %d of batch element %d weights no prompt that has a valid key", f, b);
            for (int s = 0; s < S; ++s) {
                const float x = w[((size_t)b * S + s) * L + f];
                (*out)[((size_t)b * S + s) * L + i] = x > 0.f ? (float)std::log2((double)x / mx) : TL_OFF;
                if (x > 0.f) {
                    int* fs = &sup[((size_t)b * S + s) * 2];
                    if (fs[1] == 0) fs[0] = i;
                    fs[1] = i + 1;
                }
            }
        }
    }
    memcpy(out->data() + nb, sup.data(), sup.size() * sizeof(int));
    return EZDIT_OK;
}

// Prompt emphasis of B batch elements (include/ezdit.h, ezdit_set_context_token_weights): natural weights w [B][Lk] -> the table the KW form of k_attn reads, [B][Lkp]
// biases fp32(log2(w_j / max over the valid keys)), computed in fp64: every bias is <= 0, the heaviest valid key has exactly 0, and masked and padding keys hold 0.
// mask (nullable = every key valid, [B][Lk]): w is not read at a masked key.  *any: some bias is non-zero (a table of zeros is the plain kernel)
int keyweight_table(const float* w, int B, int Lk, int Lkp, const uint8_t* mask, std::vector<float>* out, bool* any) {
    out->assign((size_t)B * Lkp, 0.f);
    *any = false;
    for (int b = 0; b < B; ++b) {
        double mx = 0.0, mn = 0.0;
        bool seen = false;
        for (int j = 0; j < Lk; ++j) {
            if (mask && !mask[(size_t)b * Lk + j]) continue;
            const float x = w[(size_t)b * Lk + j];
            if (!std::isfinite(x) || !(x > 0.f)) return fail(EZDIT_E_INVALID, "weights[%d][%d] = %g: the weight of a valid key is finite and above 0 (the mask drops a token)", b, j, (double)x);
            mx = seen ? (x > mx ? x : mx) : x;
            mn = seen ? (x < mn ? x : mn) : x;
            seen = true;
        }
        if (!seen) continue;   // (a row without a valid key has no weights to check; its biases stay 0)
        if (mx > mn * 1048576.0) return fail(EZDIT_E_INVALID, "weights of batch element %d span %g .. %g: more than 2^20 apart", b, mn, mx);
        for (int j = 0; j < Lk; ++j) {
            if (mask && !mask[(size_t)b * Lk + j]) continue;
            const float bias = (float)std::log2((double)w[(size_t)b * Lk + j] / mx);
            (*out)[(size_t)b * Lkp + j] = bias;
            *any = *any || bias != 0.f;
        }
    }
    return EZDIT_OK;
}

// A ControlNet handle carries a length table only as half of an attached pair (ezdit_sampler_set_pair_lengths): when the pair ends -- detach, or the
// backbone is destroyed -- the table goes, and with it the condition embed that was computed from it.  The backbone keeps its own table.
void clear_cn_lengths(ezdit_handle* cn) {
    if (cn->lens.on) cn->cond_ready = false;
    cn->lens.set(cn, false);
    cn->lens.host.clear();
}

// ---- the lifetime of the tables.  Call-scoped ones belong to one sampler call: ezdit_sampler_begin starts without them
void reset_call_state(ezdit_handle* h) {
    h->sp.set(h, false);
    h->coef.set(h, false); h->ms_hist = nullptr;
    h->start.set(h, false); h->start_min = 0;
    h->canvas.set(h, false); h->canvas_loop = false;
    h->cw.set(h, false); h->cw_K = 1;
    h->apg.set(h, false); h->apg_mom = nullptr;
}

// the values of a composed call's weight table [P][K]: finite, the primary condition's above 0
int check_compose_weights(const float* w, int P, int K) {
    for (int p = 0; p < P; ++p)
        for (int k = 0; k < K; ++k) {
            const float x = w[(size_t)p * K + k];
            if (!std::isfinite(x)) return fail(EZDIT_E_INVALID, "weights[%d][%d] is not finite", p, k);
            if (k == 0 && !(x > 0.f)) return fail(EZDIT_E_INVALID, "weights[%d][0] = %g: the primary condition's weight is above 0", p, (double)x);
        }
    return EZDIT_OK;
}

// ... bind-scoped ones, and the sampler call itself, belong to one binding of the workspace: a new one zeroes the device arrays and may have another shape, so
// nothing that was set or begun on the old one holds ("ezdit_sampler_begin first" rests on `latents`)
void reset_bind_state(ezdit_handle* h) {
    h->lens.set(h, false); h->lens.host.clear();
    h->cns.set(h, false);
    h->tl.set(h, false); h->tl.host.clear(); h->tl_S = 0;
    h->tw.set(h, false); h->tw.host.clear();
    h->coef.host.clear();
    h->latents = nullptr; h->noise = nullptr; h->s_gt = nullptr; h->s_gt_mask = nullptr;
    h->P = 0; h->n_steps = 0;
    drop_graph(h);   // (whatever the tables were: the captured step points at the old buffers)
}

}  // namespace

// ======================================================================================================
extern "C" {

int ezdit_abi_version(void) { return EZDIT_ABI_VERSION; }
const char* ezdit_last_error(void) { return g_err.c_str(); }

int ezdit_create(const ezdit_config* cfg, ezdit_handle** out) {
    if (!cfg || !out) return fail(EZDIT_E_INVALID, "null argument");
    if (cfg->embed_dim <= 0 || cfg->num_heads <= 0 || cfg->embed_dim % cfg->num_heads)
        return fail(EZDIT_E_INVALID, "embed_dim %d not divisible by num_heads %d", cfg->embed_dim, cfg->num_heads);
    const int dh = cfg->embed_dim / cfg->num_heads;
    if (dh != 64 && dh != 72) return fail(EZDIT_E_UNSUPPORTED, "head_dim %d: only 64 and 72 are implemented", dh);
    if (cfg->embed_dim > 1280 || cfg->embed_dim % 4) return fail(EZDIT_E_UNSUPPORTED, "embed_dim %d > 1280", cfg->embed_dim);
    if (cfg->in_chans != 2 * cfg->out_chans + 1)
        return fail(EZDIT_E_UNSUPPORTED, "in_chans %d != 2*out_chans+1 (MaskDiT concat)", cfg->in_chans);
    if (cfg->depth < 2 || cfg->depth % 2) return fail(EZDIT_E_UNSUPPORTED, "depth %d must be even", cfg->depth);
    if (cfg->mlp_ratio != 4.0f) return fail(EZDIT_E_UNSUPPORTED, "mlp_ratio %g", (double)cfg->mlp_ratio);
    ezdit_handle* h = new ezdit_handle();
    h->cfg = *cfg;
    if (h->cfg.max_len <= 0) h->cfg.max_len = 2048;
    h->D = cfg->embed_dim;
    h->H = cfg->num_heads;
    h->dh = dh;
    h->nhalf = cfg->depth / 2;
    h->is_cn = cfg->controlnet != 0;
    h->nblk = h->is_cn ? cfg->depth / 2 : cfg->depth + 1;
    if (h->is_cn) {
        if (cfg->cond_in <= 0 || cfg->cond_c0 <= 0 || cfg->cond_c1 <= 0) {
            delete h;
            return fail(EZDIT_E_INVALID, "controlnet needs cond_in / cond_blocks");
        }
        h->c0 = cfg->cond_c0;
        h->c0m = cfg->cond_c0 + (cfg->cond_mask ? 1 : 0);
        h->c1 = cfg->cond_c1;
    }
    h->I = (int)(cfg->embed_dim * cfg->mlp_ratio);
    h->C = cfg->out_chans;
    h->Cin = cfg->in_chans;
    h->Cctx = cfg->context_dim;
    h->r6 = 6 * cfg->ada_sola_rank;
    h->scaling = cfg->ada_sola_alpha / (float)cfg->ada_sola_rank;
    h->DQK = dh == 64 ? 64 : 80;
    h->DV = dh == 64 ? 64 : 96;
    h->ldD = (int)rup(h->D, 64);
    h->ld2D = (int)rup(2 * h->D, 64);
    h->ldI = (int)rup(h->I, 64);
    h->ldPE = (int)rup(h->Cin, 64);
    h->ldCtx = (int)rup(h->Cctx, 64);
    build_params(h);
    (void)hipGetDevice(&h->device);
    *out = h;
    return EZDIT_OK;
}

int ezdit_destroy(ezdit_handle* h) {
    if (!h) return EZDIT_OK;
    drop_graph(h);
    for (ezdit_handle* u : h->cn_users)   // a backbone must not keep a dangling pointer to this ControlNet
        if (u->cn == h) { u->cn = nullptr; u->cn_scale = 1.0f; u->cns.set(u, false); }
    if (h->cn) {
        auto& v = h->cn->cn_users;
        for (size_t i = 0; i < v.size(); ++i) if (v[i] == h) { v.erase(v.begin() + i); break; }
        clear_cn_lengths(h->cn);
    }
    if (h->cn_fork) (void)hipEventDestroy(h->cn_fork);
    if (h->cn_join) (void)hipEventDestroy(h->cn_join);
    if (h->cn_stream) (void)hipStreamDestroy(h->cn_stream);
    delete h;
    return EZDIT_OK;
}

int ezdit_param_count(const ezdit_handle* h) { return h ? (int)h->params.size() : 0; }
int ezdit_param_info(const ezdit_handle* h, int i, ezdit_param_info_t* out) {
    if (!h || !out || i < 0 || i >= (int)h->params.size()) return fail(EZDIT_E_INVALID, "bad parameter index %d", i);
    *out = h->params[i];
    return EZDIT_OK;
}
size_t ezdit_param_bytes(const ezdit_handle* h) { return h ? h->param_bytes : 0; }

int ezdit_bind_weights(ezdit_handle* h, const void* blob, size_t bytes) {
    if (!h || !blob) return fail(EZDIT_E_INVALID, "null argument");
    if (bytes < h->param_bytes) return fail(EZDIT_E_INVALID, "weight blob %zu < required %zu bytes", bytes, h->param_bytes);
    h->wblob = reinterpret_cast<const char*>(blob);
    h->ctx_ready = h->ts_ready = false;
    resolve_weights(h);
    return EZDIT_OK;
}

size_t ezdit_workspace_bytes(const ezdit_handle* h, int B, int L, int Lc, int n_slots) {
    if (!h || B <= 0 || L <= 0 || Lc <= 0) return 0;
    return carve(h, B, L, Lc, n_slots, nullptr);
}

int ezdit_bind_workspace(ezdit_handle* h, void* ws, size_t bytes, int B, int L, int Lc, int n_slots, ezdit_stream stream) {
    if (!h || !ws) return fail(EZDIT_E_INVALID, "null argument");
    if (B <= 0 || B > 240 || L <= 0 || Lc <= 0) return fail(EZDIT_E_INVALID, "bad shape B=%d L=%d Lc=%d", B, L, Lc);
    if (L > h->cfg.max_len) return fail(EZDIT_E_INVALID, "L=%d exceeds max_len=%d", L, h->cfg.max_len);
    std::map<std::string, Buf> bufs;
    const size_t need = carve(h, B, L, Lc, n_slots, &bufs);
    if (bytes < need) return fail(EZDIT_E_INVALID, "workspace %zu < required %zu bytes", bytes, need);
    hipStream_t st = (hipStream_t)stream;
    h->last_stream = st;
    h->ws = reinterpret_cast<char*>(ws);
    h->ws_bytes = bytes;
    h->bufs = bufs;
    h->B = B; h->L = L; h->Lc = Lc; h->n_slots = n_slots > 0 ? n_slots : 1;
    h->M = B * L; h->Mp = (int)rup(h->M, 128); h->Lp = (int)rup(L, 128); h->Lcp = (int)rup(Lc, 128);
    h->Mc = B * Lc;
    resolve_workspace(h);
    h->steps_done = 0;
    h->ctx_ready = h->ts_ready = h->cond_ready = false;
    reset_call_state(h);
    reset_bind_state(h);
    // zero everything once: all padding rows / columns / keys stay zero for the lifetime of the binding
    HIPCHK(hipMemsetAsync(ws, 0, need, st));
    launch_rope_table(h->buf<float>("rope_cos"), h->buf<float>("rope_sin"), h->cfg.max_len, h->dh, st);
#ifdef EZ_DIAG
    {   // zfake diagnostic: statistics of a zero-mean, unit-variance row in parts of zwidth() columns
        const int zw = h->zwidth(), parts = h->zparts();
        if (parts <= Z_MAXP) {
            std::vector<float2> hst(ezdit_handle::zrange(h->Mp), make_float2(0.f, 0.f));
            for (int k = 0; k < parts; ++k)
                for (int r = 0; r < h->Mp; ++r) hst[(size_t)k * h->Mp + r] = make_float2(0.f, (float)(k == parts - 1 ? h->D - zw * (parts - 1) : zw));
            HIPCHK(hipMemcpyAsync(h->buf<float2>("zneutral"), hst.data(), hst.size() * sizeof(float2), hipMemcpyHostToDevice, st));
            HIPCHK(hipStreamSynchronize(st));
        }
    }
#endif
    return EZDIT_OK;
}

// ------------------------------------------------------------------------------------------------------
int ezdit_prepare_context(ezdit_handle* h, const float* ctx, const uint8_t* mask, ezdit_stream stream) {
    if (!h || !ctx) return fail(EZDIT_E_INVALID, "null argument");
    if (!h->wblob || !h->ws) return fail(EZDIT_E_STATE, "bind weights and workspace first");
    Ctx c{h, (hipStream_t)stream};
    const int Mc = h->Mc, D = h->D;
    uint8_t* km = h->buf<uint8_t>("kmask");
    if (mask) HIPCHK(hipMemcpyAsync(km, mask, Mc, hipMemcpyDeviceToDevice, c.st));
    else HIPCHK(hipMemsetAsync(km, 1, Mc, c.st));
    // (the context weights were checked against the old mask: a new context starts without them.  Behind the first copy: a call refused above changes nothing)
    h->tl.set(h, false); h->tl.host.clear(); h->tl_S = 0;
    h->tw.set(h, false); h->tw.host.clear();   // (the token weights likewise)
    // single-key batch elements (opt_xkey1): their cross-attention output is a constant.  The mask is read back once per call (B Lc bytes)
    std::vector<int> key1(h->B, -1);   // the valid key of a single-key batch element, -1 otherwise
    const bool old_x1 = h->xkey1; const int old_b0 = h->act_b0, old_b1 = h->act_b1;
    h->xkey1 = false; h->act_b0 = 0; h->act_b1 = h->B;
    // (the read-back below synchronises the stream: ezdit_prepare_context is not a per-step entry point and must not be called inside a stream capture;
    // it is skipped when its result could not be used -- the option must be set BEFORE this call)
    if (mask && h->opt_xkey1 && h->zfuse_usable()) {
        std::vector<uint8_t> hm((size_t)Mc);
        HIPCHK(hipMemcpyAsync(hm.data(), mask, Mc, hipMemcpyDeviceToHost, c.st));
        HIPCHK(hipStreamSynchronize(c.st));
        int first = -1, last = -1, n1 = 0;
        for (int b = 0; b < h->B; ++b) {
            int cnt = 0, at = -1;
            for (int j = 0; j < h->Lc; ++j) if (hm[(size_t)b * h->Lc + j]) { ++cnt; at = j; }
            if (cnt == 1) { key1[b] = at; ++n1; }
            else { if (first < 0) first = b; last = b; }
        }
        bool contiguous = true;
        for (int b = first; first >= 0 && b <= last; ++b) if (key1[b] >= 0) contiguous = false;
        if (n1 > 0 && contiguous) {
            h->xkey1 = true;
            h->act_b0 = first < 0 ? 0 : first;
            h->act_b1 = first < 0 ? 0 : last + 1;
        }
    }
    // the captured step bakes (xkey1, act_b0, act_b1) into its launch structure (DUAL attention-out, cross-attention over a batch sub-range):
    // a context with another single-key pattern must not replay the old graph -- nor may a backbone that captured this ControlNet's kernels
    if (h->xkey1 != old_x1 || h->act_b0 != old_b0 || h->act_b1 != old_b1) drop_graph(h);
    // context_embed: Linear -> SiLU -> Linear  (udit.py:94-97)
    launch_cast_bf16(ctx, h->Cctx, h->buf<bf16_t>("ctx_bf"), h->ldCtx, Mc, h->Cctx, 0, c.st);
    gemm(c, h->buf<bf16_t>("ctx_bf"), h->ldCtx, h->wref("ce.w1"), h->w<float>("ce.b1"), h->buf<float>("c1"), D, Mc, D, EPI_F32, tile_for(h, Mc, false));
    launch_cast_bf16(h->buf<float>("c1"), D, h->buf<bf16_t>("c1b"), h->ldD, Mc, D, 1, c.st);
    gemm(c, h->buf<bf16_t>("c1b"), h->ldD, h->wref("ce.w2"), h->w<float>("ce.b2"), h->buf<float>("c2"), D, Mc, D, EPI_F32, tile_for(h, Mc, false));
    for (int b = 0; b < h->nblk; ++b) {
        // norm_context (blocks.py:150) -> to_k / to_v -> head LayerNorm on k (attention.py:128-142)
        RowArgs r;
        memset(&r, 0, sizeof r);
        r.h_in = h->buf<float>("c2");
        r.mode = 0;
        r.ln_g = h->w<float>(bn(b, "ncw"));
        r.ln_c = h->w<float>(bn(b, "ncb"));
        r.u = h->buf<bf16_t>("cu");
        r.ld_u = h->ldD;
        r.M = Mc; r.D = D; r.L = h->Lc;
        launch_row(r, c.st);
        gemm(c, h->buf<bf16_t>("cu"), h->ldD, h->wref(bn(b, "wkv2")), nullptr, h->buf<float>("ckv"), 2 * D, Mc, 2 * D, EPI_F32, tile_for(h, Mc, false));
        HeadNormArgs hn;
        memset(&hn, 0, sizeof hn);
        hn.x = h->buf<float>("ckv"); hn.ldx = 2 * D;
        hn.q_col = -1; hn.k_col = 0; hn.v_col = D;
        hn.kn_w = h->w<float>(bn(b, "c.knw")); hn.kn_b = h->w<float>(bn(b, "c.knb"));
        hn.k = h->buf<bf16_t>("kc") + (size_t)b * h->B * h->H * h->Lcp * h->DQK;
        hn.v = h->buf<bf16_t>("vc") + (size_t)b * h->B * h->H * h->Lcp * h->DV;
        hn.B = h->B; hn.H = h->H; hn.L = h->Lc; hn.Lp = h->Lcp; hn.dh = h->dh;
        launch_headnorm(hn, c.st);
        c.launched("k_headnorm");
        if (h->xkey1) {
            // d[b] = W_o v_key + b_o for the single-key batch elements: v_key is row (b Lc + key) of the fp32 value projection above, rounded to bf16
            // as the attention kernel's V^T operand and output would be (P = 1 exactly), W_o the bf16 out-projection the step uses
            const WRef wo2 = h->wref(bn(b, "wo2"));
            GemvBatch gb;
            gb.x = h->buf<float>("ckv"); gb.y = h->p.zd + (size_t)b * h->B * D; gb.n = 0;
            for (int e = 0; e <= h->B; ++e) {   // one launch per GEMV_MAXB single-key batch elements (one launch per block for every CFG batch up to 32 prompts)
                if (e < h->B && key1[e] >= 0) {
                    gb.xoff[gb.n] = ((long)e * h->Lc + key1[e]) * 2 * D + D;
                    gb.yoff[gb.n] = (long)e * D;
                    gb.n++;
                }
                if (gb.n == GEMV_MAXB || (e == h->B && gb.n > 0)) {
                    launch_gemv_bf16w(gb, 1, wo2.W, wo2.ld, h->w<float>(bn(b, "bo2")), D, D, c.st);
                    c.launched("k_gemv_bf16w");
                    gb.n = 0;
                }
            }
        }
    }
    if (c.bad()) return c.result();
    h->ctx_ready = true;
    return EZDIT_OK;
}

int ezdit_prepare_timesteps(ezdit_handle* h, const int32_t* ts, int n, int per_row, ezdit_stream stream) {
    if (!h || !ts) return fail(EZDIT_E_INVALID, "null argument");
    if (!h->wblob || !h->ws) return fail(EZDIT_E_STATE, "bind weights and workspace first");
    if (n <= 0 || n > h->n_slots) return fail(EZDIT_E_INVALID, "n=%d timesteps but workspace holds %d slots", n, h->n_slots);
    if (per_row && n != h->B) return fail(EZDIT_E_INVALID, "per_row needs n == B (%d != %d)", n, h->B);
    hipStream_t st = (hipStream_t)stream;
    const int D = h->D, nblk = h->nblk;
    h->per_row = per_row;   // (the producer choice of the LayerNorm algebra depends on it: ztile())
    int* ints = h->buf<int>("ints");
    HIPCHK(hipMemcpyAsync(h->buf<int>("ts"), ts, (size_t)n * 4, hipMemcpyHostToDevice, st));
    std::vector<int> rs(240, 0);
    if (per_row) for (int b = 0; b < h->B; ++b) rs[b] = b;
    HIPCHK(hipMemcpyAsync(ints + 16, rs.data(), 240 * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));  // rs is a stack/heap temporary; prepare is not on the per-step path
    launch_set_int(ints, 0, 0, st);
    // TimestepEmbedder + time_act (modules.py:50-60, udit.py:313)
    launch_linear_f32(nullptr, h->buf<int>("ts"), 1, h->w<float>("te.w1"), h->w<float>("te.b1"), h->buf<float>("t1"), n, D, 256, 1, D, st);
    launch_linear_f32(h->buf<float>("t1"), nullptr, 0, h->w<float>("te.w2"), h->w<float>("te.b2"), h->buf<float>("tt"), n, D, D, 1, D, st);
    launch_linear_f32(h->buf<float>("tt"), nullptr, 0, h->w<float>("ada.w"), h->w<float>("ada.b"), h->buf<float>("ada"), n, 6 * D, D, 0, 6 * D, st);
    if (!h->is_cn)
        launch_linear_f32(h->buf<float>("tt"), nullptr, 0, h->w<float>("adaf.w"), h->w<float>("adaf.b"), h->buf<float>("adaf"), n, 2 * D, D, 0, 2 * D, st);
    for (int b = 0; b < nblk; ++b) {
        launch_linear_f32(h->buf<float>("tt"), nullptr, 0, h->w<float>(bn(b, "lora_a")), nullptr, h->buf<float>("la"), n, h->r6, D, 0, h->r6, st);
        launch_linear_f32(h->buf<float>("la"), nullptr, 0, h->w<float>(bn(b, "lora_b")), nullptr,
                          h->buf<float>("lora") + (size_t)b * 6 * D, n, 6 * D, h->r6, 0, (long)nblk * 6 * D, st);
    }
    ModFinalizeArgs m;
    memset(&m, 0, sizeof m);
    m.ada = h->buf<float>("ada");
    m.lora = h->buf<float>("lora");
    m.scaling = h->scaling;
    m.table = h->w<float>(bn(0, "table"));
    m.table_stride = nblk > 1 ? (h->w<float>(bn(1, "table")) - h->w<float>(bn(0, "table"))) : 0;
    m.n1w = h->w<float>(bn(0, "n1w")); m.n1b = h->w<float>(bn(0, "n1b"));
    m.n3w = h->w<float>(bn(0, "n3w")); m.n3b = h->w<float>(bn(0, "n3b"));
    m.norm_stride = nblk > 1 ? (h->w<float>(bn(1, "n1w")) - h->w<float>(bn(0, "n1w"))) : 0;
    m.mod = h->buf<float>("mod");
    m.has_final = h->is_cn ? 0 : 1;
    if (!h->is_cn) {
        m.ada_final = h->buf<float>("adaf");
        m.nfw = h->w<float>("fin.nw"); m.nfb = h->w<float>("fin.nb");
        m.mod_final = h->buf<float>("modf");
    }
    m.n = n; m.nblk = nblk; m.D = D;
    launch_mod_finalize(m, st);
    {
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(EZDIT_E_HIP, "time-path launch failed: %s", hipGetErrorString(e));
    }
    if (h->zfuse_usable()) {
        // LayerNorm algebra tables (GemmArgs.z*): G' = g W^T, C' = c W^T (+ bias) of the LayerNorm in front of the fused QKV GEMM (norm1,
        // modulated: per slot), of the GEGLU GEMM (norm3, modulated; C' carries mlp.net.0.proj.bias) and of cross-attention's to_q (norm2,
        // static).  Small bf16 GEMMs on exact hi + lo splits of the fp32 vectors; once per call.
        Ctx c{h, st};
        const long mod_slot = (long)nblk * 6 * D;
        bf16_t* zA = h->buf<bf16_t>("zA");
        float* ztmp = h->buf<float>("ztmp");
        const int I2 = 2 * h->I, N3 = 3 * D;
        for (int b = 0; b < nblk; ++b) {
            const BlkW& w = h->blk[b];
            const float* modb = h->p.mod + (long)b * 6 * D;
            launch_z_hilo(modb + 0 * D, modb + 1 * D, mod_slot, zA, h->ldD, n, D, st);
            gemm(c, zA, h->ldD, w.wqkv, nullptr, ztmp, N3, 4 * n, N3, EPI_F32, 25);
            const ezdit_handle::ZTab tq = h->zt_qkv_of(b), tg = h->zt_geglu_of(b), t2 = h->zt_q2_of(b);
            launch_z_combine(ztmp, N3, nullptr, tq.G, tq.C, tq.slot_stride, n, N3, st);
            launch_z_hilo(modb + 3 * D, modb + 4 * D, mod_slot, zA, h->ldD, n, D, st);
            gemm(c, zA, h->ldD, w.w1, nullptr, ztmp, I2, 4 * n, I2, EPI_F32, 25);
            launch_z_combine(ztmp, I2, w.b1, tg.G, tg.C, tg.slot_stride, n, I2, st);
            launch_z_hilo(w.n2w, w.n2b, 0, zA, h->ldD, 1, D, st);
            gemm(c, zA, h->ldD, w.wq2, nullptr, ztmp, D, 4, D, EPI_F32, 25);
            launch_z_combine(ztmp, D, nullptr, t2.G, t2.C, t2.slot_stride, 1, D, st);
            if (b > h->nhalf && h->skip_z_usable()) {   // skip_norm (static, over the 2 D columns of [x | skip]) in front of skip_linear; C' carries skip_linear.bias
                const ezdit_handle::ZTab tk = h->zt_skip_of(b - h->nhalf - 1);
                launch_z_hilo(w.snw, w.snb, 0, zA, h->ld2D, 1, 2 * D, st);
                gemm(c, zA, h->ld2D, w.wskip, nullptr, ztmp, D, 4, D, EPI_F32, 25);
                launch_z_combine(ztmp, D, w.bskip, tk.G, tk.C, tk.slot_stride, 1, D, st);
            }
        }
        const hipError_t e = hipGetLastError();
        if (c.bad() || e != hipSuccess) return fail(EZDIT_E_HIP, "LayerNorm-algebra table launch failed: %s", hipGetErrorString(e));
    }
    h->steps_done = 0;
    h->ts_ready = true;
    h->z_tables_ready = h->zfuse_usable();
    h->skip_tables_ready = h->z_tables_ready && h->skip_z_usable();
    h->n_ts = n;
    h->per_row = per_row;
    return EZDIT_OK;
}

int ezdit_set_step(ezdit_handle* h, int step, ezdit_stream stream) {
    if (!h || !h->ws) return fail(EZDIT_E_STATE, "bind workspace first");
    if (step < 0 || step >= h->n_slots) return fail(EZDIT_E_INVALID, "step %d out of range", step);
    // start table: only a rewind to the run's own beginning (first-order for every sample active at it, so also with the multistep solver on)
    if (h->start.on && step != h->start_min)
        return fail(EZDIT_E_STATE, "start table: step %d is not the run's first step %d (only a rewind to it keeps every sample's trajectory)", step, h->start_min);
    if (h->coef.on && !h->start.on && step != 0) return fail(EZDIT_E_STATE, "multistep solver: the history is not step %d's (only a rewind to step 0 keeps it right)", step - 1);
    if (h->apg.on && !h->start.on && step != 0) return fail(EZDIT_E_STATE, "projected guidance: the momentum is not step %d's (only a rewind to step 0 keeps it right)", step - 1);
    launch_set_int(h->p.ints, step, 0, (hipStream_t)stream);
    h->steps_done = step;
    return EZDIT_OK;
}

int ezdit_set_lengths(ezdit_handle* h, const int32_t* lengths, int n, ezdit_stream stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = setter_checks(h, "ezdit_set_lengths", Needs::Bound, st)) return rc;
    // (the timeline's table was built for the frames that existed when it was set: padding frames carry the last frame's weights and stand in no support)
    if (h->tl.on) {   // (a call that leaves the lengths as they are is let through)
        bool same = (!lengths || n == 0) ? !h->lens.on : false;
        if (lengths && n > 0 && h->lens.on && n <= h->B && h->B % n == 0) {
            same = true;
            for (int b = 0; b < h->B; ++b) same = same && h->lens.host[b] == lengths[b % n];
        }
        if (!same) return fail(EZDIT_E_STATE, "new lengths while the context weights are on: ezdit_set_context_weights(NULL), the lengths, then the weights again");
    }
    if (!lengths || n == 0) {
        if (h->is_cn) clear_cn_lengths(h);   // (a table the pair call left on a ControlNet: its embed goes with it)
        else { h->lens.set(h, false); h->lens.host.clear(); }
        return EZDIT_OK;
    }
    // one handle's call can set only one of the two tables of an attached pair, and they must agree: the pair has its own call
    if (h->is_cn) return fail(EZDIT_E_UNSUPPORTED, "per-sample lengths on a ControlNet handle (its condition embed is computed from the table: ezdit_sampler_set_pair_lengths on the backbone it is attached to)");
    if (h->cn) return fail(EZDIT_E_UNSUPPORTED, "per-sample lengths with a ControlNet attached: ezdit_sampler_set_pair_lengths sets both tables");
    if (h->canvas.on) return fail(EZDIT_E_UNSUPPORTED, "per-sample lengths while the canvas is on (ezdit_sampler_set_canvas): its windows have one length");
    std::vector<int> v;
    if (int rc = expand_lengths(h, lengths, n, &v)) return rc;
    if (int rc = upload_table(h->lens, std::move(v), st)) return rc;
    h->lens.set(h, true);
    return EZDIT_OK;
}

// Prompt timeline: per-frame weights of the S prompts of the bound context (Lc = 128 S; prompt s = context rows [128 s, 128 s + 128)).  The table is checked against the
// key mask of the latest ezdit_prepare_context and the lengths that are set, then read by the cross-attention launch of every block (k_attn TL)
int ezdit_set_context_weights(ezdit_handle* h, const float* weights, int S, ezdit_stream stream) {
    hipStream_t st = (hipStream_t)stream;
    if (h && weights && h->is_cn) return fail(EZDIT_E_UNSUPPORTED, "context weights on a ControlNet handle");   // (whatever its state: the ControlNet has no timeline)
    if (int rc = setter_checks(h, "ezdit_set_context_weights", Needs::Bound, st)) return rc;
    if (!weights) {
        h->tl.set(h, false); h->tl.host.clear(); h->tl_S = 0;
        return EZDIT_OK;
    }
    if (h->cn) return fail(EZDIT_E_UNSUPPORTED, "context weights with a ControlNet attached");
    if (h->canvas.on) return fail(EZDIT_E_UNSUPPORTED, "context weights while the canvas is on (ezdit_sampler_set_canvas): a window has one prompt");
    if (h->cw.on) return fail(EZDIT_E_UNSUPPORTED, "context weights while composed guidance is on (ezdit_sampler_begin_composed)");
    if (h->tw.on) return fail(EZDIT_E_UNSUPPORTED, "context weights while the token weights are on (ezdit_set_context_token_weights)");
    if (S < 1 || S > TL_MAXS) return fail(EZDIT_E_INVALID, "S = %d outside [1, %d]", S, TL_MAXS);
    if (h->Lc != 128 * S) return fail(EZDIT_E_INVALID, "S = %d prompts need a context of %d tokens (128 each), the workspace is bound to Lc = %d", S, 128 * S, h->Lc);
    if (!h->ctx_ready) return fail(EZDIT_E_STATE, "ezdit_prepare_context first: the weights are checked against its key mask");
    std::vector<uint8_t> km((size_t)h->Mc);
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemcpy(km.data(), h->p.kmask, km.size(), hipMemcpyDeviceToHost));
    std::vector<float> v;
    if (int rc = timeline_table(weights, h->B, S, h->L, h->lens.on ? h->lens.host.data() : nullptr, km.data(), &v)) return rc;
    if (int rc = upload_table(h->tl, std::move(v), st, (size_t)h->B * S * h->L, reinterpret_cast<float*>(h->tlsup))) return rc;
    h->tl.set(h, true);
    h->tl_S = S;
    return EZDIT_OK;
}

// Prompt emphasis: one weight per context token of every batch row.  The table is checked against the key mask of the latest ezdit_prepare_context, then read by the
// cross-attention launch of every block (k_attn KW).  A table of zeros (every row uniform) is OFF: the plain instantiations run
int ezdit_set_context_token_weights(ezdit_handle* h, const float* weights, int n, ezdit_stream stream) {
    hipStream_t st = (hipStream_t)stream;
    if (h && weights && h->is_cn) return fail(EZDIT_E_UNSUPPORTED, "token weights on a ControlNet handle (its blocks have cross-attention of their own)");
    if (int rc = setter_checks(h, "ezdit_set_context_token_weights", Needs::Bound, st)) return rc;
    if (!weights) {
        h->tw.set(h, false); h->tw.host.clear();
        return EZDIT_OK;
    }
    if (h->cn) return fail(EZDIT_E_UNSUPPORTED, "token weights with a ControlNet attached (its blocks have cross-attention of their own)");
    if (h->tl.on) return fail(EZDIT_E_UNSUPPORTED, "token weights while the context weights are on (ezdit_set_context_weights)");
    if (n != h->B) return fail(EZDIT_E_INVALID, "n = %d rows of weights, the workspace is bound to B = %d", n, h->B);
    if (!h->ctx_ready) return fail(EZDIT_E_STATE, "ezdit_prepare_context first: the weights are checked against its key mask");
    std::vector<uint8_t> km((size_t)h->Mc);
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemcpy(km.data(), h->p.kmask, km.size(), hipMemcpyDeviceToHost));
    std::vector<float> v;
    bool any = false;
    if (int rc = keyweight_table(weights, h->B, h->Lc, h->Lcp, km.data(), &v, &any)) return rc;
    if (!any) {   // every row uniform: the plain kernel, bit for bit the call that never set the table
        h->tw.set(h, false); h->tw.host.clear();
        return EZDIT_OK;
    }
    // (a shape whose cross-attention does not run an 8-wave form is refused by launch_attention itself: the forward or the step reports its return code as EZDIT_E_UNSUPPORTED)
    if (int rc = upload_table(h->tw, std::move(v), st)) return rc;
    h->tw.set(h, true);
    return EZDIT_OK;
}

// The lengths of an attached pair: one table, uploaded to the backbone AND its ControlNet.  The ControlNet's condition embed is computed from the table
// (ezdit_prepare_condition moves the convolution boundary to 2 len_b), so a new table invalidates it.
int ezdit_sampler_set_pair_lengths(ezdit_handle* h, const int32_t* lengths, int n, ezdit_stream stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = setter_checks(h, "ezdit_sampler_set_pair_lengths", Needs::BoundBackbone, st)) return rc;
    ezdit_handle* cn = h->cn;
    if (!cn) return fail(EZDIT_E_STATE, "no ControlNet attached (ezdit_sampler_attach_controlnet first; a backbone alone takes ezdit_set_lengths)");
    if (!cn->ws || cn->B != h->B || cn->L != h->L)
        return fail(EZDIT_E_STATE, "the attached ControlNet is bound to (B, L) = (%d, %d), the backbone to (%d, %d)", cn->ws ? cn->B : 0, cn->ws ? cn->L : 0, h->B, h->L);
    if (!lengths || n == 0) {
        h->lens.set(h, false); h->lens.host.clear();
        clear_cn_lengths(cn);
        return EZDIT_OK;
    }
    std::vector<int> v;
    if (int rc = expand_lengths(h, lengths, n, &v)) return rc;
    if (!cn->lens.on || cn->lens.host != v) cn->cond_ready = false;   // the embed of the old table: ezdit_prepare_condition again
    if (int rc = upload_table(h->lens, v, st)) return rc;
    if (int rc = upload_table(cn->lens, std::move(v), st)) return rc;
    h->lens.set(h, true);
    cn->lens.set(cn, true);   // (null <-> table in the ControlNet's kernels, which the backbone's step captured: drop_graph reaches its users)
    return EZDIT_OK;
}

// conditioning_scale per batch element of the fused sampler's ControlNet residuals (row b: scales[b % n], the rule of the lengths: a CFG pair shares its scale)
int ezdit_sampler_set_cn_scales(ezdit_handle* h, const float* scales, int n, ezdit_stream stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = setter_checks(h, "ezdit_sampler_set_cn_scales", Needs::BoundBackbone, st)) return rc;
    if (!h->cn) return fail(EZDIT_E_STATE, "no ControlNet attached (ezdit_sampler_attach_controlnet first)");
    if (!scales || n == 0) {
        h->cns.set(h, false);
        return EZDIT_OK;
    }
    if (n < 0 || n > h->B || h->B % n) return fail(EZDIT_E_INVALID, "%d scales do not divide B = %d", n, h->B);
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(scales[i])) return fail(EZDIT_E_INVALID, "non-finite conditioning scale of sample %d", i);
    if (int rc = upload_table(h->cns, per_row<float>(scales, n, h->B), st)) return rc;
    h->cns.set(h, true);
    return EZDIT_OK;
}

// ------------------------------------------------------------------------------------------------------
// cn_scale multiplies the ControlNet residuals `cn` (conditioning_scale, controlnet.py:313): the fused sampler passes the
// attached ControlNet's scale, ezdit_forward passes 1 (the caller's residuals are already scaled, as DiTControlNet.forward returns them)
// cn_ready (nullable): event the residuals `cn` become valid at; waited for right before their first consumer, so a ControlNet
// forward on another stream overlaps the backbone's in-blocks and mid block (the two chains are independent until then,
// src/inference_controlnet.py:89-99 + udit.py:345-348).
static int forward_impl(ezdit_handle* h, const float* x, int in_ch, int x_rows, const float* gt, const uint8_t* gt_mask,
                        const float* const* cn, int n_cn, float cn_scale, float* out, hipStream_t st, hipEvent_t cn_ready = nullptr,
                        const int* cur_override = nullptr, const float* cn_tab = nullptr) {
    const bool cn_mode = h->is_cn;  // ControlNet: in-blocks only, then one zero-Linear per skip (controlnet.py:303-315)
    Ctx c{h, st};
    const WsPtrs& p = h->p;
    const int D = h->D, M = h->M, nblk = h->nblk, nhalf = h->nhalf, Mp = h->Mp;
    // device step counter that selects the modulation slot.  A ControlNet attached to the fused sampler reads the BACKBONE's counter
    // (cur_override): only that one is advanced by the CFG / DDIM kernel, and the reference evaluates the ControlNet at the current t
    // every step (src/inference_controlnet.py:92-96)
    const int* cur = cur_override ? cur_override : p.ints;
    const int* row_slot = h->per_row ? p.ints + 16 : nullptr;
    c.cur = cur; c.row_slot = row_slot;
    float* hA = p.h;
    float* skips = p.skips;
    bf16_t* u = p.u;
    float* part = p.part;
    const float* mod = p.mod;
    const long mod_slot = (long)nblk * 6 * D;
    h->launches = 0;
    (void)hipGetLastError();   // a stale error of an earlier, unrelated call must not be blamed on this one
#define STOPCHK() do { if (c.bad()) return c.result(); if (h->debug_stop > 0 && h->launches >= h->debug_stop) return EZDIT_OK; } while (0)

    // A4 + A5: input assembly and patch embed (Conv1d k=1 == per-token Linear)
    AssembleArgs as;
    as.x = x; as.x_rows = x_rows; as.in_ch = in_ch;
    as.gt = gt; as.gt_mask = gt_mask; as.mask_embed = cn_mode ? h->ext_mask_embed : h->w_mask_embed;
    as.out = p.ape; as.ldo = h->ldPE;
    as.B = h->B; as.C = h->C; as.L = h->L; as.lens = h->lens_dev();
    STOPCHK();
    launch_assemble(as, st);
    c.launched("k_assemble");
    // What `u` holds: null = a finished LayerNorm (written by the row kernel); otherwise A' = bf16(h g) of the LayerNorm algebra, and the pointer is where its producer
    // put the partial statistics.  row() and edge() set it, the consumer sites read it
    const float2* u_stat = nullptr;
    // the row kernel of an edge: h_out = h_in + gate * (the sum of `nsplit` slabs + bias)  (mode 1; 2: no h_in, 0: h_in alone), then u = LN(h_out) ln_g + ln_c
    auto row = [&](const Edge& e, int mode, const float* slabs, int nsplit) {
        RowArgs r;
        memset(&r, 0, sizeof r);
        r.h_in = e.h_in; r.h_out = e.h_out;
        r.part = slabs; r.nsplit = nsplit; r.part_stride = (long)Mp * D; r.ld_part = D;
        r.part_bf16 = (slabs == part) ? 1 : 0;   // the split-K slabs are bf16
        r.cn_scale = cn_scale; r.cn_tab = cn_tab;   // (cn_tab: the fused sampler's per-sample scales; ezdit_forward never passes one)
        r.bias = e.bias; r.gate = e.gate; r.gate_slot_stride = e.gate_stride; r.mode = mode;
        r.ln_g = e.ln_g; r.ln_c = e.ln_c; r.ln_slot_stride = e.ln_stride;
        r.skip = e.skip; r.cn = e.cn;
        r.u = e.ln_g ? (e.skip ? p.ucat : u) : nullptr; r.ld_u = e.skip ? h->ld2D : h->ldD;
        r.M = M; r.D = D; r.L = h->L;
        r.cur_step = cur; r.row_slot = row_slot; r.wt = h->wt();
        r.variant = h->opt_row_variant;
        r.affine = h->opt_row_affine && M <= 1024;
        launch_row(r, st);
        c.launched("k_row");
        if (e.ln_g && !e.skip) u_stat = nullptr;   // `u` now holds a finished LayerNorm
    };
    auto modv = [&](int blk, int which) { return mod + ((long)blk * 6 + which) * D; };
    const int qkv_mode = h->qkv_mode();   // 2: fused QKV GEMM (ping-pong kernel), 0: fp32 projection + k_headnorm
    const bool zf = h->z_tables_ready && h->zfuse_usable();
    // The launches of one residual edge.  Not the LayerNorm algebra: the projection as split-K slabs + the row kernel that reduces them -- two launches (the one-launch
    // form with an in-launch hand-off measured slower in round 2 and was removed), with the debug_stop / error check of STOPCHK between them.
    // LayerNorm algebra (opt_zfuse): ONE un-split projection whose epilogue produces h_out, its partial LayerNorm statistics and A' = bf16(h_out ln_g) for the next
    // GEMM, which finishes the LayerNorm
    auto edge = [&](const Edge& e) {
        if (!e.algebra) {
            const int s2 = gemm_partial(c, e.A, e.lda, *e.w, M, D);
            if (c.bad() || (h->debug_stop > 0 && h->launches >= h->debug_stop)) return;
            row(e, e.h_in ? 1 : 2, part, s2);
            return;
        }
        const long r0 = (long)e.b0 * h->L;
        const int Ms = e.nb < 0 ? M : e.nb * h->L, K = e.w->ld;
        int tile = h->ztile();
        // few rows (the cross-attention-out projection over one prompt's conditional rows, M = 500): 48-row tiles leave 11 x 12 = 132 workgroups for 256 CUs;
        // 32 x 96 tiles (id 72) give 16 x 12 = 192 with 11 % fewer operand bytes each: 3.968 -> 3.951 ms per step, bit-identical (profiles/r05_experiments.txt)
        if (tile == ezdit_handle::kZTile && e.dual_blk < 0 && !e.zu2 && !e.zin2 && Ms <= 672 && K <= 2 * D) tile = 72;
        GemmArgs g = resid_args(tile, e.A + r0 * e.lda, e.lda, e.w->W, e.w->ld, e.w->rows, e.bias, e.h_in ? e.h_in + r0 * D : nullptr, e.gate, e.ln_g,
                                e.h_out ? e.h_out + r0 * D : nullptr, e.zu ? e.zu : u + r0 * h->ldD, e.zu ? e.ld_zu : h->ldD,
                                e.zstat_out ? e.zstat_out : p.zstat + r0, h->Mp, Ms, D, K);
        g.wt = h->wt(); g.gate_slot_stride = e.gate_stride; g.zg_slot_stride = e.ln_stride;
        g.cur_step = cur; g.row_slot = row_slot ? row_slot + e.b0 : nullptr; g.rows_per_b = h->L;
        if (e.dual_blk >= 0) {
            g.zd = p.zd + (size_t)e.dual_blk * h->B * D; g.zd_stride = D;
            g.zg2 = modv(e.dual_blk, 3); g.zg2_slot_stride = mod_slot;
            g.act_row0 = h->act_b0 * h->L; g.act_row1 = h->act_b1 * h->L;
        }
        if (e.zu2) { g.zu2 = e.zu2; g.ld_zu2 = e.ld_zu2; g.zg2 = e.zg2; g.zg2_slot_stride = 0; }
        if (e.zin2) { g.zstat_in = e.zin; g.zstat_in2 = e.zin2; g.zG = e.zG; g.zparts = h->zparts(); g.zD = 2 * D; g.zeps = 1e-5f; }
        g.ts = c.stamps(); g.ts_cap = g_gemm_ts_cap;
        c.launched(e.name, launch_gemm(g, st));
        if (!e.zu) u_stat = e.zstat_out ? e.zstat_out : p.zstat;   // `u` now holds A'
    };
    // LN_2D([x | skip]) -> skip_linear by the LayerNorm algebra (opt_skip_z): not with ControlNet residuals (they change the skips)
    const bool skipz = zf && h->skip_tables_ready && h->skip_z_usable() && !(cn && n_cn > 0);
    // single-key shortcut (opt_xkey1): cross-attention + its out-projection cover the batch elements [xb0, xb0 + xnb) only
    const bool x1 = zf && h->opt_xkey1 && h->xkey1;
    const int xb0 = x1 ? h->act_b0 : 0, xnb = x1 ? h->act_b1 - h->act_b0 : h->B;

    // LN1 of block 0 on the patch embedding (ControlNet: x = patch_embed(x) + controlnet_pre(condition) first, :263-266)
    STOPCHK();
    {
        Edge e;
        e.name = "k_gemm (un-split residual: patch embed)"; e.algebra = zf && !cn_mode;
        e.A = p.ape; e.lda = h->ldPE; e.w = &h->w_pe; e.bias = h->b_pe; e.h_out = hA;
        e.ln_g = modv(0, 0); e.ln_c = modv(0, 1); e.ln_stride = mod_slot;
        if (e.algebra) {
            // the patch embed itself is the producer for block 0's norm1 (no gate, no residual: h = acc + bias, statistics, bf16(h g)) -- no row-kernel launch
            edge(e);
        } else {
            // not a split-K edge: the K-split fp32 GEMM applies the bias itself, the row kernel adds the condition embed (ControlNet: one fp32 "slab") and normalises
            gemm(c, e.A, e.lda, *e.w, e.bias, hA, D, M, D, EPI_F32, M <= 2048 ? ezdit_handle::kTilePE : tile_for(h, M, false));
            STOPCHK();
            e.bias = nullptr; e.h_in = hA;
            if (cn_mode) row(e, 1, p.cembed, 1);
            else { e.h_out = nullptr; row(e, 0, part, 0); }
        }
    }
    const float* hcur = hA;

    for (int b = 0; b < nblk; ++b) {
        const BlkW& w = h->blk[b];
        const bool is_in = b < nhalf, is_out = b > nhalf;
        if (is_out) {
            // u holds LN_2D([x | skip]) -> skip_linear (blocks.py:124-128)
            STOPCHK();
            const int j = b - nhalf - 1;
            Edge e;
            e.name = skipz ? "k_gemm (un-split residual: skip_linear ZIN)" : "k_gemm (un-split residual: skip_linear)"; e.algebra = zf;
            e.A = skipz ? h->ucat_of(j) : p.ucat; e.lda = h->ld2D; e.w = &w.wskip; e.bias = w.bskip; e.h_out = hA;
            e.ln_g = modv(b, 0); e.ln_c = modv(b, 1); e.ln_stride = mod_slot;
            if (skipz) {   // the operand is bf16([x | skip] g): finish ITS LayerNorm from the halves' statistics and G'; C' (it carries skip_linear.bias) takes the bias' place
                const ezdit_handle::ZTab t = h->zt_skip_of(j);
                e.zin = h->zstat_xhalf(); e.zin2 = h->zstat_skip_of(nhalf - 1 - j); e.zG = t.G; e.bias = t.C;
            }
            edge(e);
            hcur = hA;
        }
        // ---- self attention (blocks.py:136-141) ----
        STOPCHK();
        HeadNormArgs hn;
        memset(&hn, 0, sizeof hn);
        hn.x = p.qkv; hn.ldx = 3 * D;
        hn.q_col = 0; hn.k_col = D; hn.v_col = 2 * D;
        hn.qn_w = w.aqnw; hn.qn_b = w.aqnb;
        hn.kn_w = w.aknw; hn.kn_b = w.aknb;
        hn.rope_cos = p.rope_cos; hn.rope_sin = p.rope_sin;
        hn.q = p.q; hn.k = p.k; hn.v = p.v;
        hn.B = h->B; hn.H = h->H; hn.L = h->L; hn.Lp = h->Lp; hn.dh = h->dh;
        if (qkv_mode) {
            // head-norm + RoPE + the attention layouts inside the projection GEMM (128 x two-head tiles): no fp32 q|k|v round trip, one launch less
            hn.perm = 1;   // (qkv_mode == 2 <=> the weights were packed with EZDIT_T_QKROPE)
            gemm(c, u, h->ldD, w.wqkv, nullptr, nullptr, 0, M, 3 * D, EPI_QKV, h->qkv_tile(), &hn, ZIn{h->zt_qkv_of(b), u_stat});
        } else {
            gemm(c, u, h->ldD, w.wqkv, nullptr, p.qkv, 3 * D, M, 3 * D, EPI_F32, tile_for(h, M, false));
            STOPCHK();
            launch_headnorm(hn, st);
            c.launched("k_headnorm");
        }
        AttnArgs at;
        memset(&at, 0, sizeof at);
        at.q = hn.q; at.k = hn.k; at.v = hn.v; at.kmask = nullptr;
        at.nkh = h->opt_attn_nkh; at.xcd_map = h->opt_attn_xcd; at.wt = h->wt();
        at.out = p.ao; at.ldo = h->ldD;
        at.B = h->B; at.H = h->H; at.Lq = h->L; at.Lk = h->L; at.Lqp = h->Lp; at.Lkp = h->Lp; at.dh = h->dh;
        at.klen = h->lens_dev();   // the reference's x_mask: keys beyond a sample's length do not exist
        at.band = h->attn_band();  // sliding window (0: the plain kernel, today's launch); the same single launch either way
        STOPCHK();
        at.ts = c.stamps(); at.ts_cap = g_gemm_ts_cap;
        c.launched("k_attn (self)", launch_attention(at, st));
        STOPCHK();
        {   // x += (1 - gate_msa) * (proj + bias); then norm2 (plain affine LN) for cross-attention q
            Edge e;
            e.name = x1 ? "k_gemm (un-split residual: attention-out DUAL)" : "k_gemm (un-split residual: attention-out)"; e.algebra = zf;
            e.A = at.out; e.lda = h->ldD; e.w = &w.wo; e.bias = w.bo; e.h_in = hcur; e.h_out = hA;
            e.gate = modv(b, 2); e.gate_stride = mod_slot;
            e.ln_g = w.n2w; e.ln_c = w.n2b;
            if (x1) e.dual_blk = b;
            edge(e);
        }
        hcur = hA;
        // ---- cross attention (blocks.py:147-151) ----
        STOPCHK();
        // one prompt: the cross-attention kernel also computes its own q = LN_head(u . Wq^T) (8-wave form, Lcp % 128 == 0)
        // (x1: over the batch elements [xb0, xb0 + xnb) only -- the others are single-key rows served by the attention-out projection above)
        const bool fuse_q2 = h->q2_fused(xnb);   // four prompts per GPU with the shortcut: 4 x 16 x 8 = 512 workgroups -> fused (10.38 -> 10.22 ms per step of 4)
        const long xr0 = (long)xb0 * h->L;          // first row of the sub-range
        const int xM = xnb * h->L;
        if (xnb > 0) {
            memset(&hn, 0, sizeof hn);
            hn.x = p.qkv; hn.ldx = D;
            hn.q_col = 0; hn.k_col = -1; hn.v_col = -1;
            hn.qn_w = w.cqnw; hn.qn_b = w.cqnb;
            hn.q = p.q + (size_t)xb0 * h->H * h->Lp * h->DQK;
            hn.B = xnb; hn.H = h->H; hn.L = h->L; hn.Lp = h->Lp; hn.dh = h->dh;
            at.xu = nullptr; at.nkh = h->opt_attn_nkh;
            at.B = xnb; at.b0 = xb0;
            const ZIn zq{h->zt_q2_of(b), u_stat, (int)xr0, xb0};   // norm2 -> to_q by the LayerNorm algebra (static tables)
            if (fuse_q2) {
                at.xu = u; at.ldu = h->ldD; at.xw = w.wq2.W; at.ldw = w.wq2.ld;
                at.xw_rows = w.wq2.rows; at.xK = at.ldw;
                at.qn_w = hn.qn_w; at.qn_b = hn.qn_b; at.nkh = 4; at.xk2 = h->opt_attn_xk2; at.qtile = h->opt_attn_qtile;
#ifdef EZ_DIAG
                if (!u_stat && h->opt_zfake && h->zparts() <= Z_MAXP) {
                    at.zw = h->zwidth(); at.zstat_in = h->buf<float2>("zneutral"); at.zs_stride = h->Mp; at.zparts = h->zparts(); at.zD = D; at.zeps = 1e-5f;
                    at.zG = h->buf<float>("zzeros"); at.zC = at.zG;
                }
#endif
                if (u_stat) {
                    at.zw = h->zwidth(); at.zstat_in = u_stat; at.zs_stride = h->Mp; at.zparts = h->zparts(); at.zD = D; at.zeps = 1e-5f;
                    at.zG = zq.t.G; at.zC = zq.t.C;
                }
            } else if (qkv_mode == 2 && h->opt_q2_pp) {
                // batched prompts: the q projection on the ping-pong kernel with the fused-QKV epilogue restricted to its q part (N = D, no RoPE):
                // per-head LayerNorm and the bf16 attention layout straight out of the GEMM -- no fp32 q round trip, no 128 x 64 tile at M = 4000
                // (k_gemm<128,64> + normalisation inside k_attn: 30 us; this: one round of 256 workgroups).  LayerNorm-algebra capable (zt_q2 is static)
                gemm(c, u + xr0 * h->ldD, h->ldD, w.wq2, nullptr, nullptr, 0, xM, D, EPI_QKV, 61, &hn, zq);
                at.q = p.q;   // (launch_attention advances it by b0)
            } else {
                gemm(c, u + xr0 * h->ldD, h->ldD, w.wq2, nullptr, p.qkv + xr0 * D, D, xM, D, EPI_F32, tile_for(h, xM, false));
                at.q_raw = p.qkv; at.ld_qraw = D; at.qn_w = hn.qn_w; at.qn_b = hn.qn_b;   // the cross-attention kernel normalises q itself
            }
            at.q = p.q;
            at.k = p.kc + (size_t)b * h->B * h->H * h->Lcp * h->DQK;
            at.v = p.vc + (size_t)b * h->B * h->H * h->Lcp * h->DV;
            at.kmask = p.kmask; at.klen = nullptr; at.band = 0;   // (the key lengths and the band are self-attention's: context keys have their own mask and no time axis)
            at.tlb = h->tl.read(); at.tlsup = h->tl.on ? h->tlsup : nullptr;   // ... unless the prompt timeline gives them one (ezdit_set_context_weights): the TL form, the same single launch
            at.kbias = h->tw.read();   // prompt emphasis (ezdit_set_context_token_weights): the KW form, the same single launch; [B][Lcp], advanced by b0 like the mask
            at.Lk = h->Lc; at.Lkp = h->Lcp;
            STOPCHK();
            at.ts = c.stamps(); at.ts_cap = g_gemm_ts_cap;
            const int arc = launch_attention(at, st);
            c.launched("k_attn (cross)", arc && at.kbias ? EZDIT_E_UNSUPPORTED : arc);   // (a shape without an 8-wave form while the token weights are on: ezdit_set_context_token_weights)
            STOPCHK();
            Edge e;
            e.name = "k_gemm (un-split residual: cross-out)"; e.algebra = zf;
            e.A = at.out; e.lda = h->ldD; e.w = &w.wo2; e.bias = w.bo2; e.h_in = hA; e.h_out = hA;
            e.ln_g = modv(b, 3); e.ln_c = modv(b, 4); e.ln_stride = mod_slot;
            e.b0 = xb0; if (x1) e.nb = xnb;
            edge(e);
        }
        // ---- GEGLU MLP (blocks.py:154-156) ----
        STOPCHK();
        gemm(c, u, h->ldD, w.w1, w.b1, p.act, h->ldI, M, 2 * h->I, EPI_GEGLU, h->geglu_tile(), nullptr, ZIn{h->zt_geglu_of(b), u_stat});   // 128 x 288 ping-pong kernel / 128 x 144 co-resident kernel / round-1 lockstep kernel
        STOPCHK();
        // x += (1 - gate_mlp) * (mlp + bias); the LN that follows belongs to the NEXT consumer
        Edge e;
        e.A = p.act; e.lda = h->ldI; e.w = &w.w2; e.bias = w.b2; e.h_in = hA;
        e.gate = modv(b, 5); e.gate_stride = mod_slot;
        if (cn_mode && b == nblk - 1) {
            e.h_out = skips + (size_t)b * Mp * D;   // the ControlNet's last skip: no LayerNorm follows
        } else if (b == nblk - 1) {
            e.ln_g = p.modf; e.ln_c = p.modf + D; e.ln_stride = 2L * D;   // the final block's norm; its Linear is no LayerNorm-algebra consumer
        } else if (b + 1 > nhalf) {
            const int j = b + 1 - nhalf - 1;  // out block index of the consumer
            const float* cnp = (cn && n_cn > 0) ? cn[n_cn - 1 - j] : nullptr;
            if (cnp && cn_ready) { (void)hipStreamWaitEvent(st, cn_ready, 0); cn_ready = nullptr; }   // join the ControlNet stream
            e.ln_g = h->blk[b + 1].snw; e.ln_c = h->blk[b + 1].snb;
            e.algebra = skipz;
            if (skipz) {   // un-split: x_new only lives on as bf16(x_new g[:D]) in the left half of the out-block's operand, statistics in the second part range of the shared buffer
                e.name = "k_gemm (un-split residual: MLP-out -> [x | skip])";
                e.zu = h->ucat_of(j); e.ld_zu = h->ld2D; e.zstat_out = h->zstat_xhalf();
            } else {
                e.skip = skips + (size_t)(nhalf - 1 - j) * Mp * D; e.cn = cnp;
            }
        } else {
            e.h_out = is_in ? skips + (size_t)b * Mp * D : hA;
            e.ln_g = modv(b + 1, 0); e.ln_c = modv(b + 1, 1); e.ln_stride = mod_slot;
            e.name = "k_gemm (un-split residual: MLP-out)"; e.algebra = zf;
            if (skipz && is_in) {   // COPY2: + the skip half of the matching out-block's operand, statistics kept until that out-block
                const int j = nhalf - 1 - b;
                e.name = "k_gemm (un-split residual: MLP-out COPY2)";
                e.zstat_out = h->zstat_skip_of(b); e.zu2 = h->ucat_of(j) + D; e.ld_zu2 = h->ld2D; e.zg2 = h->blk[nhalf + 1 + j].snw + D;
            }
            hcur = e.h_out;
        }
        edge(e);
    }
    if (cn_mode) {
        // controlnet_skips[i] = zero_Linear_i(skip_i) (* conditioning_scale, applied by the consumer)  controlnet.py:311-313
        for (int i = 0; i < nblk; ++i) {
            launch_cast_bf16(skips + (size_t)i * Mp * D, D, p.skipbf, h->ldD, M, D, 0, st);
            c.launched("k_cast_bf16");
            gemm(c, p.skipbf, h->ldD, h->blk[i].zw, h->blk[i].zb, p.cnres + (size_t)i * Mp * D, D, M, D, EPI_F32, tile_for(h, M, false));
        }
        return c.result();
    }
    // A18 FinalBlock: u = LN(x)*(1+scale)+shift -> Linear(D->C) -> transpose -> Conv1d(C,C,3,pad 1)
    STOPCHK();
    gemm(c, u, h->ldD, h->w_fin, h->b_fin, p.y, h->C, M, h->C, EPI_F32, M <= 2048 ? ezdit_handle::kTileFin : tile_for(h, M, false));
    FinalConvArgs fc;
    fc.y = p.y; fc.ldy = h->C;
    fc.w = h->w_fin_cw; fc.b = h->w_fin_cb;
    fc.out = out; fc.B = h->B; fc.C = h->C; fc.L = h->L; fc.lens = h->lens_dev();
    STOPCHK();
    launch_final_conv(fc, st);
    c.launched("k_final_conv");
    return c.result();
}

int ezdit_forward(ezdit_handle* h, const float* x, int in_ch, int x_rows, const float* gt, const uint8_t* gt_mask,
                  const float* const* cn_skips, int n_cn, float* out, ezdit_stream stream) {
    if (!h || !x || !out) return fail(EZDIT_E_INVALID, "null argument");
    if (h->is_cn) return fail(EZDIT_E_INVALID, "this handle is a ControlNet: use ezdit_controlnet_forward");
    if (!h->wblob || !h->ws) return fail(EZDIT_E_STATE, "bind weights and workspace first");
    if (!h->ctx_ready) return fail(EZDIT_E_STATE, "ezdit_prepare_context has not run for this workspace");
    if (!h->ts_ready) return fail(EZDIT_E_STATE, "ezdit_prepare_timesteps has not run for this workspace");
    if (in_ch != h->C && in_ch != h->Cin) return fail(EZDIT_E_INVALID, "in_ch %d: expected %d or %d", in_ch, h->C, h->Cin);
    if (in_ch == h->C && (x_rows <= 0 || h->B % x_rows)) return fail(EZDIT_E_INVALID, "x_rows %d does not divide B %d", x_rows, h->B);
    if ((gt == nullptr) != (gt_mask == nullptr)) return fail(EZDIT_E_INVALID, "gt and gt_mask must be given together");
    if (n_cn != 0 && n_cn != h->nhalf) return fail(EZDIT_E_INVALID, "n_cn %d: expected 0 or %d", n_cn, h->nhalf);
    if (n_cn != 0 && h->lens.on) return fail(EZDIT_E_UNSUPPORTED, "ControlNet residuals with per-sample lengths (ezdit_set_lengths)");
    // the caller's residuals are already multiplied by conditioning_scale (DiTControlNet.forward returns them scaled,
    // controlnet.py:313); a scale left on the handle by the fused sampler must not be applied a second time
    return forward_impl(h, x, in_ch, x_rows, gt, gt_mask, cn_skips, n_cn, h->fwd_cn_scale, out, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------------
int ezdit_prepare_condition(ezdit_handle* h, const float* cond, int Lcond, ezdit_stream stream) {
    if (!h || !cond) return fail(EZDIT_E_INVALID, "null argument");
    if (!h->is_cn) return fail(EZDIT_E_INVALID, "not a ControlNet handle");
    if (!h->wblob || !h->ws) return fail(EZDIT_E_STATE, "bind weights and workspace first");
    if (Lcond != 2 * h->L) return fail(EZDIT_E_INVALID, "condition length %d != 2 * L (%d): the embed has one stride-2 conv", Lcond, 2 * h->L);
    hipStream_t st = (hipStream_t)stream;
    Conv1dArgs a;
    memset(&a, 0, sizeof a);
    // conv_in: Conv1d(cond_in, c0, 1)                                               controlnet.py:15,66
    a.x = cond; a.w = h->w<float>("cn.cin.w"); a.b = h->w<float>("cn.cin.b"); a.out = h->buf<float>("cn_e0");
    a.B = h->B; a.Cin = h->cfg.cond_in; a.cin_valid = a.Cin; a.Cout = h->c0; a.Lin = Lcond; a.Lout = Lcond; a.ksize = 1; a.stride = 1; a.pad = 0;
    // padded batch (the pair call's table): batch element b is its own [cond_in, 2 len_b] condition -- every layer's zero padding sits at ITS end, not at
    // 2 L (after the 1 x 1 conv_in a padded frame would hold the bias, which the k = 3 layer behind it reads at frame 2 len_b)
    a.lens = h->lens_dev(); a.lin_mul = 2; a.lout_mul = 2;
    launch_conv1d(a, st);
    // eval: no position is masked, the appended mask channel is all zeros (:68-74) -> channel c0 is an implicit zero input
    a.x = h->buf<float>("cn_e0"); a.w = h->w<float>("cn.c0.w"); a.b = h->w<float>("cn.c0.b"); a.out = h->buf<float>("cn_e1");
    a.Cin = h->c0m; a.cin_valid = h->c0; a.Cout = h->c0m; a.ksize = 3; a.pad = 1; a.act = 1;
    launch_conv1d(a, st);
    a.x = h->buf<float>("cn_e1"); a.w = h->w<float>("cn.c1.w"); a.b = h->w<float>("cn.c1.b"); a.out = h->buf<float>("cn_e2");
    a.Cin = h->c0m; a.cin_valid = h->c0m; a.Cout = h->c1; a.Lout = h->L; a.stride = 2; a.lout_mul = 1;
    launch_conv1d(a, st);
    // conv_out: Conv1d(c1, D, 1) then transpose to [B, L, D]                         :37,79-82
    a.x = h->buf<float>("cn_e2"); a.w = h->w<float>("cn.cout.w"); a.b = h->w<float>("cn.cout.b"); a.out = h->buf<float>("cembed");
    a.Cin = h->c1; a.cin_valid = h->c1; a.Cout = h->D; a.Lin = h->L; a.Lout = h->L; a.ksize = 1; a.stride = 1; a.pad = 0; a.act = 0;
    a.out_token_major = 1; a.lin_mul = 1;
    launch_conv1d(a, st);
    {
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(EZDIT_E_HIP, "condition-embed launch failed: %s", hipGetErrorString(e));
    }
    h->cond_ready = true;
    return EZDIT_OK;
}

int ezdit_controlnet_forward(ezdit_handle* h, const float* x, int in_ch, int x_rows, const float* gt, const uint8_t* gt_mask,
                             const float* mask_embed, ezdit_stream stream) {
    if (!h || !x) return fail(EZDIT_E_INVALID, "null argument");
    if (!h->is_cn) return fail(EZDIT_E_INVALID, "not a ControlNet handle");
    if (!h->wblob || !h->ws) return fail(EZDIT_E_STATE, "bind weights and workspace first");
    if (!h->ctx_ready || !h->ts_ready || !h->cond_ready) return fail(EZDIT_E_STATE, "prepare context, timesteps and condition first");
    if (in_ch != h->C && in_ch != h->Cin) return fail(EZDIT_E_INVALID, "in_ch %d: expected %d or %d", in_ch, h->C, h->Cin);
    if (in_ch == h->C && !mask_embed) return fail(EZDIT_E_INVALID, "in_ch = C needs the backbone's mask_embed");
    if (in_ch == h->C && (x_rows <= 0 || h->B % x_rows)) return fail(EZDIT_E_INVALID, "x_rows %d does not divide B %d", x_rows, h->B);
    h->ext_mask_embed = mask_embed;
    return forward_impl(h, x, in_ch, x_rows, gt, gt_mask, nullptr, 0, 1.0f, nullptr, (hipStream_t)stream);
}

int ezdit_controlnet_residuals(ezdit_handle* h, const float** out, int n) {
    if (!h || !out || !h->is_cn || !h->ws) return fail(EZDIT_E_INVALID, "need a bound ControlNet handle");
    if (n != h->nhalf) return fail(EZDIT_E_INVALID, "n %d != depth/2 %d", n, h->nhalf);
    for (int i = 0; i < n; ++i) out[i] = h->buf<float>("cnres") + (size_t)i * h->Mp * h->D;
    return EZDIT_OK;
}

int ezdit_sampler_attach_controlnet(ezdit_handle* h, ezdit_handle* cn, float conditioning_scale) {
    if (!h || h->is_cn) return fail(EZDIT_E_INVALID, "first argument must be a backbone handle");
    if (cn && !cn->is_cn) return fail(EZDIT_E_INVALID, "second argument must be a ControlNet handle");
    if (cn && h->canvas.on) return fail(EZDIT_E_UNSUPPORTED, "a ControlNet while the canvas is on (ezdit_sampler_set_canvas)");
    if (cn && h->tl.on) return fail(EZDIT_E_UNSUPPORTED, "a ControlNet while the context weights are on (ezdit_set_context_weights)");
    if (cn && h->cw.on) return fail(EZDIT_E_UNSUPPORTED, "a ControlNet while composed guidance is on (ezdit_sampler_begin_composed)");
    if (cn && h->tw.on) return fail(EZDIT_E_UNSUPPORTED, "a ControlNet while the token weights are on (ezdit_set_context_token_weights)");
    if (cn && cn->attn_window != h->attn_window)
        return fail(EZDIT_E_INVALID, "attention windows differ: backbone %d, ControlNet %d frames (ezdit_set_attention_window on both)", h->attn_window, cn->attn_window);
    if (h->cn && h->cn != cn) {
        auto& v = h->cn->cn_users;
        for (size_t i = 0; i < v.size(); ++i) if (v[i] == h) { v.erase(v.begin() + i); break; }
        clear_cn_lengths(h->cn);   // the pair ends: the ControlNet's half of its table goes, the backbone keeps its own
    }
    if (cn && h->cn != cn) cn->cn_users.push_back(h);
    h->cn = cn;
    h->cn_scale = cn ? conditioning_scale : 1.0f;
    h->cns.set(h, false);   // an attach gives every sample this scalar; ezdit_sampler_set_cn_scales comes after it
    if (cn && !h->cn_stream) {   // side stream + fork / join events of the overlapped ControlNet branch: created here, never inside a stream capture
        HIPCHK(hipStreamCreateWithFlags(&h->cn_stream, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&h->cn_fork, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&h->cn_join, hipEventDisableTiming));
    }
    drop_graph(h);
    return EZDIT_OK;
}

int ezdit_set_cn_scale(ezdit_handle* h, float scale) {
    if (!h) return fail(EZDIT_E_INVALID, "null handle");
    h->fwd_cn_scale = scale;
    return EZDIT_OK;
}

// ------------------------------------------------------------------------------------------------------
// what ezdit_sampler_begin and ezdit_sampler_begin_composed do once their arguments are accepted: the call's coefficient rows, step 0, no call-scoped table
static int begin_call(ezdit_handle* h, float* latents, int P, const float* noise, const ezdit_ddim_coef* coefs, int n_steps, float guidance_scale,
                      float guidance_rescale, const float* gt, const uint8_t* gt_mask, hipStream_t st) {
    h->last_stream = st;
    std::vector<float> cf((size_t)n_steps * 8, 0.f);
    for (int i = 0; i < n_steps; ++i) {
        cf[i * 8 + 0] = coefs[i].sa; cf[i * 8 + 1] = coefs[i].sb; cf[i * 8 + 2] = coefs[i].c_x0;
        cf[i * 8 + 3] = coefs[i].c_dir; cf[i * 8 + 4] = coefs[i].sigma;
    }
    if (int rc = upload_table(h->coef, std::move(cf), st)) return rc;
    launch_set_int(h->p.ints, 0, 0, st);
    h->steps_done = 0;
    h->latents = latents; h->noise = noise; h->P = P; h->n_steps = n_steps;
    h->gscale = guidance_scale; h->grescale = guidance_rescale;
    h->s_gt = gt; h->s_gt_mask = gt_mask;
    reset_call_state(h);
    drop_graph(h);   // (another latents pointer, other scalars: whatever the tables were)
    return EZDIT_OK;
}

int ezdit_sampler_begin(ezdit_handle* h, float* latents, int P, const float* noise, const ezdit_ddim_coef* coefs, int n_steps,
                        float guidance_scale, float guidance_rescale, const float* gt, const uint8_t* gt_mask,
                        ezdit_stream stream) {
    if (!h || !latents || !coefs) return fail(EZDIT_E_INVALID, "null argument");
    if (!h->ws || !h->wblob) return fail(EZDIT_E_STATE, "bind weights and workspace first");
    if (n_steps <= 0 || n_steps > h->n_slots) return fail(EZDIT_E_INVALID, "n_steps %d > workspace slots %d", n_steps, h->n_slots);
    const int needB = guidance_scale > 0.f ? 2 * P : P;
    if (P <= 0 || needB != h->B) return fail(EZDIT_E_INVALID, "P=%d with guidance %g needs B=%d, workspace has B=%d", P, (double)guidance_scale, needB, h->B);
    if ((gt == nullptr) != (gt_mask == nullptr)) return fail(EZDIT_E_INVALID, "gt and gt_mask must be given together");
    if (h->lens.on && needB == 2 * P)
        for (int p = 0; p < P; ++p)
            if (h->lens.host[p] != h->lens.host[P + p])
                return fail(EZDIT_E_INVALID, "lengths of the CFG pair of sample %d differ (%d, %d)", p, h->lens.host[p], h->lens.host[P + p]);
    return begin_call(h, latents, P, noise, coefs, n_steps, guidance_scale, guidance_rescale, gt, gt_mask, (hipStream_t)stream);
}

// The composed call (include/ezdit.h, "composed guidance"): K conditions per sample, B = (K + 1) P.  Every check comes before the first change of state
int ezdit_sampler_begin_composed(ezdit_handle* h, float* latents, int P, const float* noise, const ezdit_ddim_coef* coefs, int n_steps,
                                 float guidance_scale, float guidance_rescale, const float* gt, const uint8_t* gt_mask, int K, const float* weights,
                                 ezdit_stream stream) {
    if (!h || !latents || !coefs || !weights) return fail(EZDIT_E_INVALID, "null argument");
    if (!h->ws || !h->wblob) return fail(EZDIT_E_STATE, "bind weights and workspace first");
    if (n_steps <= 0 || n_steps > h->n_slots) return fail(EZDIT_E_INVALID, "n_steps %d > workspace slots %d", n_steps, h->n_slots);
    if (!(guidance_scale > 0.f)) return fail(EZDIT_E_INVALID, "guidance_scale = %g: composed guidance needs guidance", (double)guidance_scale);
    if (K < 1 || K > CFG_KMAX) return fail(EZDIT_E_INVALID, "K = %d outside [1, %d]", K, CFG_KMAX);
    if (P <= 0 || (long)(K + 1) * P != h->B) return fail(EZDIT_E_INVALID, "P=%d with K=%d conditions needs B=%ld, workspace has B=%d", P, K, (long)(K + 1) * P, h->B);
    if ((gt == nullptr) != (gt_mask == nullptr)) return fail(EZDIT_E_INVALID, "gt and gt_mask must be given together");
    if (int rc = check_compose_weights(weights, P, K)) return rc;
    if (h->lens.on)
        for (int b = P; b < h->B; ++b)
            if (h->lens.host[b] != h->lens.host[b % P])
                return fail(EZDIT_E_INVALID, "lengths of the rows of sample %d differ (%d, %d at batch row %d)", b % P, h->lens.host[b % P], h->lens.host[b], b);
    if (h->cn) return fail(EZDIT_E_UNSUPPORTED, "composed guidance with a ControlNet attached");
    if (h->tl.on) return fail(EZDIT_E_UNSUPPORTED, "composed guidance with context weights (ezdit_set_context_weights)");
    hipStream_t st = (hipStream_t)stream;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
    if (cs != hipStreamCaptureStatusNone) return fail(EZDIT_E_STATE, "ezdit_sampler_begin_composed inside a stream capture (it uploads from host memory and waits)");
    if (int rc = begin_call(h, latents, P, noise, coefs, n_steps, guidance_scale, guidance_rescale, gt, gt_mask, st)) return rc;
    if (int rc = upload_table(h->cw, std::vector<float>(weights, weights + (size_t)P * K), st)) return rc;
    h->cw.set(h, true); h->cw_K = K;
    return EZDIT_OK;
}

int ezdit_sampler_set_compose_weights(ezdit_handle* h, const float* weights, int P, int K, ezdit_stream stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = setter_checks(h, "ezdit_sampler_set_compose_weights", Needs::Begun, st)) return rc;
    if (!weights || P == 0) {   // off.  K = 1 is the layout of the plain call, which goes on; with K > 1 the batch has no plain reading and the call ends here
        if (h->cw.on && h->cw_K > 1) { h->latents = nullptr; h->noise = nullptr; h->s_gt = nullptr; h->s_gt_mask = nullptr; }
        h->cw.set(h, false); h->cw_K = 1;
        return EZDIT_OK;
    }
    if (!h->cw.on) return fail(EZDIT_E_STATE, "the call was not begun composed (ezdit_sampler_begin_composed): composition is another batch layout");
    if (P != h->P || K != h->cw_K) return fail(EZDIT_E_INVALID, "P = %d, K = %d: the call was begun with P = %d, K = %d", P, K, h->P, h->cw_K);
    if (int rc = check_compose_weights(weights, P, K)) return rc;
    return upload_table(h->cw, std::vector<float>(weights, weights + (size_t)P * K), st);
}

static int sampler_step(ezdit_handle* h, hipStream_t st) {
    float* pred = h->p.pred;
    const float* cnp[64];
    int n_cn = 0;
    hipEvent_t cn_ready = nullptr;
    if (h->cn) {  // src/inference_controlnet.py:89-99: ControlNet on the same assembled input, then the backbone with its skips
        ezdit_handle* cn = h->cn;
        if (cn->B != h->B || cn->L != h->L || cn->nhalf != h->nhalf || cn->D != h->D || !cn->ctx_ready || !cn->ts_ready || !cn->cond_ready)
            return fail(EZDIT_E_STATE, "attached ControlNet is not prepared for this shape (bind/context/timesteps/condition)");
        // the ControlNet indexes ITS modulation tables with the backbone's device step counter: its prepared schedule must cover the backbone's
        if (cn->n_ts < h->n_steps || cn->n_slots < h->n_steps || cn->per_row != h->per_row)
            return fail(EZDIT_E_STATE, "attached ControlNet was prepared for %d timesteps (per_row %d), the sampler runs %d (per_row %d)", cn->n_ts, cn->per_row, h->n_steps, h->per_row);
        cn->ext_mask_embed = h->w_mask_embed;
        hipStream_t cst = st;
        if (h->opt_cn_overlap && h->debug_stop == 0) {   // fork: the ControlNet chain runs next to the backbone's first half
            if (!h->cn_stream) return fail(EZDIT_E_STATE, "side stream missing: attach the ControlNet through ezdit_sampler_attach_controlnet");
            HIPCHK(hipEventRecord(h->cn_fork, st));
            HIPCHK(hipStreamWaitEvent(h->cn_stream, h->cn_fork, 0));
            cst = h->cn_stream;
        }
        int rc0 = forward_impl(cn, h->latents, h->C, h->P, h->s_gt, h->s_gt_mask, nullptr, 0, 1.0f, nullptr, cst, nullptr, h->p.ints);
        if (cst != st) {
            HIPCHK(hipEventRecord(h->cn_join, cst));
            cn_ready = h->cn_join;
            if (rc0) (void)hipStreamWaitEvent(st, cn_ready, 0);   // never leave the side stream unjoined (capture)
        }
        if (rc0) return rc0;
        n_cn = cn->nhalf;
        for (int i = 0; i < n_cn; ++i) cnp[i] = cn->p.cnres + (size_t)i * cn->Mp * cn->D;
    }
    int rc = forward_impl(h, h->latents, h->C, h->P, h->s_gt, h->s_gt_mask, n_cn ? cnp : nullptr, n_cn, h->cn_scale, pred, st, cn_ready, nullptr,
                          n_cn ? h->cns.read() : nullptr);
    if (rc && cn_ready) (void)hipStreamWaitEvent(st, cn_ready, 0);
    if (rc) return rc;
    CfgDdimArgs a;
    a.pred = pred; a.latents = h->latents; a.noise = h->noise;
    a.coef = h->p.coef; a.cur_step = h->p.ints;
    a.guidance_scale = h->gscale; a.guidance_rescale = h->grescale;
    a.P = h->P; a.n = h->C * h->L;
    a.step_inc = h->p.ints; a.done = reinterpret_cast<unsigned*>(h->p.ints + 8);
    a.lens = h->lens_dev(); a.L = h->L;
    a.sp_g = h->sp.read(); a.sp_c = h->sp.on ? h->p.spc : nullptr; a.sp_g_stride = 2;
    a.x0_hist = h->coef.on ? h->ms_hist : nullptr;
    a.start = h->start.read();
    if (h->cw.on) {   // composed guidance: the same arguments plus the weight table, the composed instantiations
        a.K = h->cw_K; a.cw = h->cw.dev;
        if (launch_cfg_compose(a, h->p.cfgpart, st)) return fail(EZDIT_E_STATE, "composed guidance with K = %d", h->cw_K);
    } else if (h->apg.on) {   // projected guidance: the same arguments plus the table and the momentum, the APG instantiations, always both launches
        a.apg = h->apg.dev; a.apg_m = h->apg_mom;
        if (launch_cfg_apg(a, h->p.cfgpart, st)) return fail(EZDIT_E_STATE, "projected guidance without its momentum buffer");
    } else
    launch_cfg_ddim(a, h->p.cfgpart, st);   // its last kernel also advances the device step counter
    h->launches += (h->apg.on || h->sp.on || (h->gscale > 0.f && h->grescale > 0.f)) ? 2 : 1;
    if (h->canvas.on) {   // long-form canvas: the windows' shared frames are averaged on the updated latents (x0_hist stays per window)
        CanvasBlendArgs cb;
        cb.latents = h->latents; cb.off = h->canvas.dev; cb.P = h->P; cb.C = h->C; cb.L = h->L; cb.T = h->canvas_T; cb.ramp = h->canvas_ramp;
        if (h->canvas_loop) launch_canvas_blend_loop(cb, st); else launch_canvas_blend(cb, st);
        h->launches += 1;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(EZDIT_E_HIP, "launch of k_cfg_* failed: %s", hipGetErrorString(e));
    return EZDIT_OK;
}

// A2 + A3 + S of SURVEY.md section 8a as ONE stand-alone operator (src/inference.py:88-100): what a caller that keeps the
// reference's Python loop binds in place of `rescale_noise_cfg` + `scheduler.step`.
int ezdit_cfg_ddim_step(const float* pred, float* latents, const float* noise, const ezdit_ddim_coef* coef, float guidance_scale,
                        float guidance_rescale, int P, int n, float* scratch, ezdit_stream stream) {
    if (!pred || !latents || !coef || P < 1 || n < 2) return fail(EZDIT_E_INVALID, "bad argument");
    if (guidance_scale > 0.f && guidance_rescale > 0.f && !scratch) return fail(EZDIT_E_INVALID, "guidance_rescale needs %d scratch floats", P * 256);
    CfgDdimArgs a = standalone_step(pred, latents, noise, P, n);
    a.hc[0] = coef->sa; a.hc[1] = coef->sb; a.hc[2] = coef->c_x0; a.hc[3] = coef->c_dir; a.hc[4] = coef->sigma;
    a.guidance_scale = guidance_scale; a.guidance_rescale = guidance_rescale;
    launch_cfg_ddim(a, scratch, (hipStream_t)stream);
    return EZDIT_OK;
}

// The per-sample form of the operator above: params fp32 [P][8] ON THE DEVICE = (guidance_scale, guidance_rescale, sa, sb, c_x0, c_dir, sigma, 0) of each
// sample; pred is [2 P][n] always (the unconditional row of a sample with guidance_scale <= 0 is not read), lens (nullable, device) as ezdit_set_lengths.
int ezdit_cfg_ddim_step_per_sample(const float* pred, float* latents, const float* noise, const float* params, const int32_t* lens, int L, int P, int n,
                                   float* scratch, ezdit_stream stream) {
    if (!pred || !latents || !params || P < 1 || n < 2) return fail(EZDIT_E_INVALID, "bad argument");
    if (!scratch) return fail(EZDIT_E_INVALID, "the per-sample step needs %d scratch floats", P * 256);
    if (lens && (L < 1 || n % L)) return fail(EZDIT_E_INVALID, "lens given: L = %d must divide n = %d", L, n);
    CfgDdimArgs a = standalone_step(pred, latents, noise, P, n, lens, L);
    a.sp_g = params; a.sp_c = params + 2; a.sp_g_stride = 8;
    return hook_launch("k_cfg_*", "", [&] { launch_cfg_ddim(a, scratch, (hipStream_t)stream); return 0; });
}

// The multistep form of the per-sample operator: params[p][7] is c_hist of sample p (slot 5 of the row sp_c = params + 2 points at), x0_hist the data
// prediction of the step before, rewritten with this step's.
int ezdit_cfg_multistep_step(const float* pred, float* latents, float* x0_hist, const float* params, const int32_t* lens, int L, int P, int n,
                             float* scratch, ezdit_stream stream) {
    if (!pred || !latents || !x0_hist || !params || P < 1 || n < 2) return fail(EZDIT_E_INVALID, "bad argument");
    if (!scratch) return fail(EZDIT_E_INVALID, "the multistep step needs %d scratch floats", P * 256);
    if (lens && (L < 1 || n % L)) return fail(EZDIT_E_INVALID, "lens given: L = %d must divide n = %d", L, n);
    CfgDdimArgs a = standalone_step(pred, latents, nullptr, P, n, lens, L);
    a.sp_g = params; a.sp_c = params + 2; a.sp_g_stride = 8;
    a.x0_hist = x0_hist;
    return hook_launch("k_cfg_*", "", [&] { launch_cfg_ddim(a, scratch, (hipStream_t)stream); return 0; });
}

// The composed form of the two operators above (include/ezdit.h, "composed guidance"): pred [(K + 1) P][n], weights [P][K] on the device
int ezdit_cfg_compose_step(const float* pred, float* latents, const float* noise, float* x0_hist, const float* params, const float* weights, int K,
                           const int32_t* lens, int L, int P, int n, float* scratch, ezdit_stream stream) {
    if (!pred || !latents || !params || !weights || P < 1 || n < 2) return fail(EZDIT_E_INVALID, "bad argument");
    if (K < 1 || K > CFG_KMAX) return fail(EZDIT_E_INVALID, "K = %d outside [1, %d]", K, CFG_KMAX);
    if (!scratch) return fail(EZDIT_E_INVALID, "the composed step needs %d scratch floats", P * 256);
    if (lens && (L < 1 || n % L)) return fail(EZDIT_E_INVALID, "lens given: L = %d must divide n = %d", L, n);
    if (noise && x0_hist) return fail(EZDIT_E_INVALID, "noise together with a history: the multistep form is deterministic");
    CfgDdimArgs a = standalone_step(pred, latents, noise, P, n, lens, L);
    a.sp_g = params; a.sp_c = params + 2; a.sp_g_stride = 8;
    a.x0_hist = x0_hist;
    a.K = K; a.cw = weights;
    return hook_launch("k_cfg_*", "composed guidance", [&] { return launch_cfg_compose(a, scratch, (hipStream_t)stream); });
}

// Adaptive projected guidance (include/ezdit.h, "adaptive projected guidance"): the table [P][4] and the caller's momentum buffer.  Every check comes before the first change of state
int ezdit_sampler_set_apg(ezdit_handle* h, const float* eta_apg, const float* norm_threshold, const float* momentum, const int32_t* on, int P, float* momentum_buf,
                          ezdit_stream stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = setter_checks(h, "ezdit_sampler_set_apg", Needs::Begun, st)) return rc;
    if ((!eta_apg && !norm_threshold && !momentum && !on) || P == 0) {   // off: the plain step again
        h->apg.set(h, false); h->apg_mom = nullptr;
        return EZDIT_OK;
    }
    if (!eta_apg || !norm_threshold || !momentum || !on) return fail(EZDIT_E_INVALID, "eta_apg, norm_threshold, momentum and on must be given together");
    if (!momentum_buf) return fail(EZDIT_E_INVALID, "a table without a momentum buffer");
    if (P != h->P) return fail(EZDIT_E_INVALID, "P = %d, the sampler was begun with P = %d", P, h->P);
    std::vector<float> v((size_t)P * 4);
    for (int p = 0; p < P; ++p) {
        if (!std::isfinite(eta_apg[p]) || !std::isfinite(norm_threshold[p]) || !std::isfinite(momentum[p])) return fail(EZDIT_E_INVALID, "non-finite value of sample %d", p);
        if (norm_threshold[p] < 0.f) return fail(EZDIT_E_INVALID, "norm_threshold[%d] = %g: a norm is >= 0 (0 = no cap)", p, (double)norm_threshold[p]);
        if (on[p] && h->B != 2 * P) return fail(EZDIT_E_INVALID, "on[%d] on a sampler begun without CFG rows (B = %d, P = %d)", p, h->B, P);
        v[p * 4 + 0] = eta_apg[p]; v[p * 4 + 1] = norm_threshold[p]; v[p * 4 + 2] = momentum[p]; v[p * 4 + 3] = on[p] ? 1.f : 0.f;
    }
    if (h->cw.on) return fail(EZDIT_E_UNSUPPORTED, "projected guidance with composed guidance (ezdit_sampler_begin_composed)");
    if (h->canvas.on) return fail(EZDIT_E_UNSUPPORTED, "projected guidance with a canvas (ezdit_sampler_set_canvas, ezdit_sampler_set_canvas_loop)");
    if (int rc = upload_table(h->apg, std::move(v), st)) return rc;
    h->apg.set(h, true, momentum_buf != h->apg_mom);   // (another momentum buffer is another kernel argument)
    h->apg_mom = momentum_buf;
    return EZDIT_OK;
}

// The APG form of the per-sample operators (include/ezdit.h): params [P][12] on the device, the momentum rewritten in place
int ezdit_cfg_apg_step(const float* pred, float* latents, const float* noise, float* x0_hist, float* momentum, const float* params, const int32_t* lens, int L,
                       int P, int n, float* scratch, ezdit_stream stream) {
    if (!pred || !latents || !momentum || !params || P < 1 || n < 2) return fail(EZDIT_E_INVALID, "bad argument");
    if (!scratch) return fail(EZDIT_E_INVALID, "the APG step needs %d scratch floats", P * 256);
    if (lens && (L < 1 || n % L)) return fail(EZDIT_E_INVALID, "lens given: L = %d must divide n = %d", L, n);
    if (noise && x0_hist) return fail(EZDIT_E_INVALID, "noise together with a history: the multistep form is deterministic");
    CfgDdimArgs a = standalone_step(pred, latents, noise, P, n, lens, L);
    a.sp_g = params; a.sp_g_stride = 12;
    a.sp_c = params + 2; a.sp_c_stride = 12;
    a.apg = params + 8; a.apg_stride = 12;
    a.apg_m = momentum;
    a.x0_hist = x0_hist;
    return hook_launch("k_cfg_*", "projected guidance", [&] { return launch_cfg_apg(a, scratch, (hipStream_t)stream); });
}

int ezdit_sampler_set_multistep(ezdit_handle* h, const float* c_hist, int n_steps, float* x0_hist, ezdit_stream stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = setter_checks(h, "ezdit_sampler_set_multistep", Needs::Begun, st)) return rc;
    const int ns = h->n_steps;
    if (c_hist) {
        if (n_steps != ns) return fail(EZDIT_E_INVALID, "n_steps = %d, the sampler was begun with %d", n_steps, ns);
        if (!x0_hist) return fail(EZDIT_E_INVALID, "c_hist given without a history buffer");
        for (int i = 0; i < ns; ++i)
            if (!std::isfinite(c_hist[i])) return fail(EZDIT_E_INVALID, "non-finite c_hist of step %d", i);
        if (h->noise) return fail(EZDIT_E_INVALID, "the multistep solver is deterministic: the sampler was begun with noise");
        if (h->sp.on) {
            const float* c = h->sp.host.data() + (size_t)h->P * 2;
            for (long i = 0; i < (long)ns * h->P; ++i)
                if (c[i * 8 + 4] != 0.f) return fail(EZDIT_E_INVALID, "the multistep solver is deterministic: sigma != 0 in the sample table (step %ld, sample %ld)", i / h->P, i % h->P);
        }
    }
    std::vector<float> rows = h->coef.host;
    for (int i = 0; i < ns; ++i) rows[(size_t)i * 8 + 5] = c_hist ? c_hist[i] : 0.f;
    if (int rc = upload_table(h->coef, std::move(rows), st)) return rc;
    const bool on = c_hist != nullptr;
    h->coef.set(h, on, x0_hist != h->ms_hist);   // (another history buffer is another kernel argument)
    h->ms_hist = on ? x0_hist : nullptr;
    return EZDIT_OK;
}

int ezdit_add_noise(const float* clean, float* latents, const float* params, float scale, float shift, const int32_t* lens, int L, int P, int n,
                    ezdit_stream stream) {
    if (!clean || !latents || !params || P < 1 || n < 1) return fail(EZDIT_E_INVALID, "bad argument");
    if (L < 1 || n % L) return fail(EZDIT_E_INVALID, "L = %d must divide n = %d", L, n);
    AddNoiseArgs a;
    a.clean = clean; a.latents = latents; a.params = params; a.scale = scale; a.shift = shift;
    a.lens = lens; a.L = L; a.P = P; a.n = n;
    return hook_launch("k_add_noise", "", [&] { launch_add_noise(a, (hipStream_t)stream); return 0; });
}

int ezdit_sampler_set_start(ezdit_handle* h, const int32_t* start_steps, int P, ezdit_stream stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = setter_checks(h, "ezdit_sampler_set_start", Needs::Begun, st)) return rc;
    if (!start_steps || P == 0) {   // off: every sample runs from step 0 again
        if (h->start.on) {   // (the run it belonged to began at start_min: the plain run begins at 0)
            launch_set_int(h->p.ints, 0, 0, st);
            h->steps_done = 0;
        }
        h->start.set(h, false); h->start_min = 0;
        return EZDIT_OK;
    }
    if (h->canvas.on) return fail(EZDIT_E_UNSUPPORTED, "a start table while the canvas is on (ezdit_sampler_set_canvas): its windows run every step together");
    if (P != h->P) return fail(EZDIT_E_INVALID, "P = %d, the sampler was begun with P = %d", P, h->P);
    int lo = h->n_steps;
    for (int p = 0; p < P; ++p) {
        if (start_steps[p] < 0 || start_steps[p] >= h->n_steps) return fail(EZDIT_E_INVALID, "start_steps[%d] = %d outside [0, n_steps = %d)", p, (int)start_steps[p], h->n_steps);
        if (start_steps[p] < lo) lo = start_steps[p];
    }
    if (int rc = upload_table(h->start, std::vector<int>(start_steps, start_steps + P), st)) return rc;
    launch_set_int(h->p.ints, lo, 0, st);
    h->steps_done = lo;
    h->start.set(h, true); h->start_min = lo;
    return EZDIT_OK;
}

int ezdit_canvas_blend(float* latents, const int32_t* offsets, int P, int C, int L, int T, int ramp, ezdit_stream stream) {
    if (!latents || !offsets) return fail(EZDIT_E_INVALID, "null argument");
    if (P < 1 || C < 1 || L < 1 || C > 65535) return fail(EZDIT_E_INVALID, "P = %d, C = %d, L = %d", P, C, L);
    if (ramp < 1) return fail(EZDIT_E_INVALID, "ramp = %d: at least 1 (the plain mean)", ramp);
    // the table is on the device and this call does not wait for it: T is checked against what any valid table gives
    if (T < L || (long)T > (long)P * L) return fail(EZDIT_E_INVALID, "T = %d: %d windows of %d frames cover between %d and %ld frames", T, P, L, L, (long)P * L);
    CanvasBlendArgs a;
    a.latents = latents; a.off = offsets; a.P = P; a.C = C; a.L = L; a.T = T; a.ramp = ramp;
    return hook_launch("k_canvas_blend", "", [&] { launch_canvas_blend(a, (hipStream_t)stream); return 0; });
}

// The canvas table has two setters: the line (ezdit_sampler_set_canvas: the last window ends the canvas) and the ring (ezdit_sampler_set_canvas_loop: the last
// window starts inside the ring and reaches or passes its end, L <= T).  One slot, one lifetime; the form picks the kernel, so line <-> ring drops the graph.
static int set_canvas_table(ezdit_handle* h, const char* who, const int32_t* offsets, int P, int T, int ramp, bool loop, hipStream_t st) {
    if (int rc = setter_checks(h, who, Needs::Begun, st)) return rc;
    if (!offsets || P == 0) {   // off: independent windows again (whichever setter switched the table on)
        h->canvas.set(h, false); h->canvas_loop = false;
        return EZDIT_OK;
    }
    const int L = h->L;
    if (P != h->P) return fail(EZDIT_E_INVALID, "P = %d, the sampler was begun with P = %d", P, h->P);
    if (ramp < 1) return fail(EZDIT_E_INVALID, "ramp = %d: at least 1 (the plain mean)", ramp);
    if (loop && L > T) return fail(EZDIT_E_INVALID, "T = %d below the window length %d: a window holds a ring frame at most once", T, L);
    if (offsets[0] != 0) return fail(EZDIT_E_INVALID, "offsets[0] = %d: the first window starts the %s", (int)offsets[0], loop ? "ring" : "canvas");
    for (int i = 0; i + 1 < P; ++i) {
        if (offsets[i + 1] <= offsets[i]) return fail(EZDIT_E_INVALID, "offsets[%d] = %d is not above offsets[%d] = %d", i + 1, (int)offsets[i + 1], i, (int)offsets[i]);
        if ((long)offsets[i + 1] > (long)offsets[i] + L)
            return fail(EZDIT_E_INVALID, "offsets[%d] = %d leaves a gap behind window %d, which ends at frame %ld", i + 1, (int)offsets[i + 1], i, (long)offsets[i] + L);
    }
    const long end = (long)offsets[P - 1] + L;
    if (!loop && end != (long)T) return fail(EZDIT_E_INVALID, "T = %d, the last window ends at frame %ld", T, end);
    if (loop && offsets[P - 1] >= T) return fail(EZDIT_E_INVALID, "offsets[%d] = %d: the last window starts inside the ring of T = %d frames", P - 1, (int)offsets[P - 1], T);
    if (loop && end < (long)T) return fail(EZDIT_E_INVALID, "T = %d: the last window ends at frame %ld and leaves a gap at the wrap", T, end);
    if (h->lens.on) return fail(EZDIT_E_UNSUPPORTED, "a canvas with per-sample lengths (ezdit_set_lengths): its windows have one length");
    if (h->start.on) return fail(EZDIT_E_UNSUPPORTED, "a canvas with a start table (ezdit_sampler_set_start)");
    if (h->s_gt) return fail(EZDIT_E_UNSUPPORTED, "a canvas with gt / gt_mask: long edits are not implemented");
    if (h->cn) return fail(EZDIT_E_UNSUPPORTED, "a canvas with a ControlNet attached");
    if (h->tl.on) return fail(EZDIT_E_UNSUPPORTED, "a canvas with context weights (ezdit_set_context_weights): a window has one prompt");
    if (h->cw.on) return fail(EZDIT_E_UNSUPPORTED, "a canvas with composed guidance (ezdit_sampler_begin_composed)");
    if (h->apg.on) return fail(EZDIT_E_UNSUPPORTED, "a canvas with projected guidance (ezdit_sampler_set_apg): the momentum is not blended across windows");
    if (int rc = upload_table(h->canvas, std::vector<int>(offsets, offsets + P), st)) return rc;
    h->canvas.set(h, true, T != h->canvas_T || ramp != h->canvas_ramp || loop != h->canvas_loop);   // (T and the ramp are kernel arguments; the other form is another kernel)
    h->canvas_T = T; h->canvas_ramp = ramp; h->canvas_loop = loop;
    return EZDIT_OK;
}

int ezdit_sampler_set_canvas(ezdit_handle* h, const int32_t* offsets, int P, int T, int ramp, ezdit_stream stream) {
    return set_canvas_table(h, "ezdit_sampler_set_canvas", offsets, P, T, ramp, false, (hipStream_t)stream);
}

int ezdit_canvas_blend_loop(float* latents, const int32_t* offsets, int P, int C, int L, int T, int ramp, ezdit_stream stream) {
    if (!latents || !offsets) return fail(EZDIT_E_INVALID, "null argument");
    if (P < 1 || C < 1 || L < 1 || C > 65535) return fail(EZDIT_E_INVALID, "P = %d, C = %d, L = %d", P, C, L);
    if (ramp < 1) return fail(EZDIT_E_INVALID, "ramp = %d: at least 1 (the plain mean)", ramp);
    // the table is on the device and this call does not wait for it: T is checked against what any valid table gives
    if (L > T) return fail(EZDIT_E_INVALID, "L = %d above T = %d: a window holds a ring frame at most once", L, T);
    if ((long)T > (long)P * L) return fail(EZDIT_E_INVALID, "T = %d: %d windows of %d frames cover at most %ld frames", T, P, L, (long)P * L);
    CanvasBlendArgs a;
    a.latents = latents; a.off = offsets; a.P = P; a.C = C; a.L = L; a.T = T; a.ramp = ramp;
    return hook_launch("k_canvas_blend_loop", "", [&] { launch_canvas_blend_loop(a, (hipStream_t)stream); return 0; });
}

int ezdit_sampler_set_canvas_loop(ezdit_handle* h, const int32_t* offsets, int P, int T, int ramp, ezdit_stream stream) {
    return set_canvas_table(h, "ezdit_sampler_set_canvas_loop", offsets, P, T, ramp, true, (hipStream_t)stream);
}

int ezdit_sampler_set_sample_params(ezdit_handle* h, const float* guidance_scale, const float* guidance_rescale, const ezdit_ddim_coef* coefs, int P,
                                    ezdit_stream stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = setter_checks(h, "ezdit_sampler_set_sample_params", Needs::Begun, st)) return rc;
    if ((!guidance_scale && !guidance_rescale && !coefs) || P == 0) {
        h->sp.set(h, false);
        return EZDIT_OK;
    }
    if (!guidance_scale || !guidance_rescale || !coefs) return fail(EZDIT_E_INVALID, "guidance_scale, guidance_rescale and coefs must be given together");
    if (P != h->P) return fail(EZDIT_E_INVALID, "P = %d, the sampler was begun with P = %d", P, h->P);
    if (P > ezdit_handle::sp_cap(h->B)) return fail(EZDIT_E_UNSUPPORTED, "per-sample settings for %d samples: a workspace of B = %d has room for %d", P, h->B, ezdit_handle::sp_cap(h->B));
    const int ns = h->n_steps;
    std::vector<float> v((size_t)P * 2 + (size_t)ns * P * 8, 0.f);
    for (int p = 0; p < P; ++p) {
        if (!std::isfinite(guidance_scale[p]) || !std::isfinite(guidance_rescale[p])) return fail(EZDIT_E_INVALID, "non-finite guidance of sample %d", p);
        if (guidance_scale[p] > 0.f && h->B != (h->cw.on ? h->cw_K + 1 : 2) * P)
            return fail(EZDIT_E_INVALID, "guidance_scale[%d] = %g on a sampler begun without CFG rows (B = P = %d)", p, (double)guidance_scale[p], P);
        v[p * 2 + 0] = guidance_scale[p]; v[p * 2 + 1] = guidance_rescale[p];
    }
    float* c = v.data() + (size_t)P * 2;
    for (long i = 0; i < (long)ns * P; ++i) {   // step-major: coefs[step * P + p]
        const ezdit_ddim_coef& k = coefs[i];
        if (!std::isfinite(k.sa) || !std::isfinite(k.sb) || !std::isfinite(k.c_x0) || !std::isfinite(k.c_dir) || !std::isfinite(k.sigma))
            return fail(EZDIT_E_INVALID, "non-finite coefficient of step %ld, sample %ld", i / P, i % P);
        if (k.sigma != 0.f && !h->noise) return fail(EZDIT_E_INVALID, "sigma != 0 (step %ld, sample %ld) on a sampler begun without noise", i / P, i % P);
        if (k.sigma != 0.f && h->coef.on) return fail(EZDIT_E_INVALID, "sigma != 0 (step %ld, sample %ld) while the multistep solver is on (it is deterministic)", i / P, i % P);
        c[i * 8 + 0] = k.sa; c[i * 8 + 1] = k.sb; c[i * 8 + 2] = k.c_x0; c[i * 8 + 3] = k.c_dir; c[i * 8 + 4] = k.sigma;
    }
    if (int rc = upload_table(h->sp, std::move(v), st, (size_t)P * 2, h->p.spc)) return rc;
    h->sp.set(h, true);
    return EZDIT_OK;
}

int ezdit_sampler_run(ezdit_handle* h, int n, int use_graph, ezdit_stream stream) {
    if (!h || !h->latents) return fail(EZDIT_E_STATE, "ezdit_sampler_begin first");
    if (!h->ctx_ready || !h->ts_ready) return fail(EZDIT_E_STATE, "prepare context and timesteps first");
    if (h->per_row) return fail(EZDIT_E_STATE, "sampler needs ezdit_prepare_timesteps(per_row = 0)");
    // the device-side step counter selects the modulation slot, the DDIM coefficients and the noise slice: running past the
    // prepared steps would index all three out of bounds
    if (n < 0 || h->steps_done + n > h->n_steps || h->steps_done + n > h->n_ts)
        return fail(EZDIT_E_STATE, "run of %d steps from step %d exceeds the %d prepared steps (ezdit_set_step rewinds)", n,
                    h->steps_done, h->n_steps < h->n_ts ? h->n_steps : h->n_ts);
    if (h->cn) {
        // an attached pair runs on ONE length table held twice (ezdit_sampler_set_pair_lengths) and on the condition embed computed from it.  Checked here, not in the
        // step: a replay of the captured graph reads the tables too
        const ezdit_handle* cn = h->cn;
        const std::vector<int>&hl = h->lens.host, &cl = cn->lens.host;
        if (h->lens.on != cn->lens.on)
            return fail(EZDIT_E_STATE, "per-sample lengths are set on the %s only: an attached pair takes them through ezdit_sampler_set_pair_lengths", h->lens.on ? "backbone" : "ControlNet");
        if (h->lens.on && hl != cl) {
            size_t b = 0;
            while (b < hl.size() && b < cl.size() && hl[b] == cl[b]) ++b;
            return fail(EZDIT_E_STATE, "the length tables of the backbone and the attached ControlNet differ at batch row %zu (%d, %d)", b,
                        b < hl.size() ? hl[b] : -1, b < cl.size() ? cl[b] : -1);
        }
        if (!cn->cond_ready) return fail(EZDIT_E_STATE, "the attached ControlNet has no condition embed for its current lengths: ezdit_prepare_condition first");
        if (cn->attn_window != h->attn_window)
            return fail(EZDIT_E_STATE, "attention windows of the backbone (%d) and the attached ControlNet (%d) differ", h->attn_window, cn->attn_window);
    }
    hipStream_t st = (hipStream_t)stream;
    h->last_stream = st;
    if (!use_graph) {
        for (int i = 0; i < n; ++i) {
            int rc = sampler_step(h, st);
            if (rc) return rc;
            h->steps_done++;
        }
        return EZDIT_OK;
    }
    if (!h->graph_exec) {
        if (st == nullptr) return fail(EZDIT_E_INVALID, "graph capture needs a non-default stream");
        HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        int rc = sampler_step(h, st);
        hipGraph_t g = nullptr;
        hipError_t e = hipStreamEndCapture(st, &g);
        if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
        if (e != hipSuccess) return fail(EZDIT_E_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
        h->graph = g;
        HIPCHK(hipGraphInstantiate(&h->graph_exec, g, nullptr, nullptr, 0));
    }
    for (int i = 0; i < n; ++i) { HIPCHK(hipGraphLaunch(h->graph_exec, st)); h->steps_done++; }
    return EZDIT_OK;
}

// ------------------------------------------------------------------------------------------------------
int ezdit_debug_gemm_timestamps(void* dev_buf, long capacity_workgroups) {
    g_gemm_ts = static_cast<unsigned long long*>(dev_buf);
    g_gemm_ts_cap = dev_buf ? capacity_workgroups : 0;
    return EZDIT_OK;
}

int ezdit_test_gemm(ezdit_handle* h, int variant, const void* A, int lda, const void* W, int ldw, const float* bias, void* out,
                    int ldo, int M, int N, int K, int splitk, ezdit_stream stream) {
    if (K % 64) return fail(EZDIT_E_INVALID, "K=%d must be a multiple of 64", K);
    GemmArgs g;
    memset(&g, 0, sizeof g);
    g.A = (const bf16_t*)A; g.lda = lda; g.W = (const bf16_t*)W; g.ldw = ldw; g.wrows = (int)rup(N, 128); g.bias = bias; g.out = out; g.ldo = ldo;
    g.M = M; g.N = N; g.K = K; g.splitk = splitk < 1 ? 1 : splitk;
    g.slab_stride = (long)rup(M, 128) * ldo;
    g.conv_cpb = 0; g.conv_tap_bytes = 0; g.resid = nullptr; g.ldr = 0; g.xcd_map = 1; g.part_bf16 = 0; g.wt = h ? h->wt() : 0; memset(&g.hn, 0, sizeof g.hn);
    g.gate = nullptr; g.gate_slot_stride = 0; g.cur_step = nullptr; g.row_slot = nullptr; g.rows_per_b = 1;
    g.debug = variant / 1000; variant %= 1000;   // 1000 * bits + v: bit 3 LDS-staged bf16 epilogue, bit 4 bf16 slabs, bit 6 LayerNorm-algebra consumer on neutral tables, bits 8.. k_gemm_pp ablation variant (EZ_ABLATE builds)
    if (g.debug & 8) g.epi_lds = 1;
    if (g.debug & 16) g.part_bf16 = 1;   // 16000 + v: bf16 split-K slabs
    g.ts = g_gemm_ts; g.ts_cap = g_gemm_ts_cap;
    g.epi = variant % 4; g.tile = variant / 4;   // variant = tile_config * 4 + epilogue
    if (g.debug & 64) {
        // 64000 + v: run the consumer side of the LayerNorm algebra on neutral tables (statistics of a zero-mean, unit-variance row, G' = 0,
        // C' = bias): same results as the plain epilogue up to the factor rsqrt(1 + 1e-5), same code path and memory traffic as the real thing
        static float2* zs = nullptr; static float* zg0 = nullptr; static float* zc = nullptr; static size_t cap_rows = 0, cap_n = 0;
        const size_t rows = (size_t)rup(M, 128), nn = (size_t)rup(N, 128);
        if (rows > cap_rows) { if (zs) (void)hipFree(zs); HIPCHK(hipMalloc(&zs, rows * 12 * sizeof(float2))); cap_rows = rows;
            std::vector<float2> hst(rows * 12, make_float2(0.f, 96.f)); HIPCHK(hipMemcpy(zs, hst.data(), hst.size() * sizeof(float2), hipMemcpyHostToDevice)); }
        if (nn > cap_n) { if (zg0) (void)hipFree(zg0); if (zc) (void)hipFree(zc); HIPCHK(hipMalloc(&zg0, nn * 4)); HIPCHK(hipMalloc(&zc, nn * 4)); cap_n = nn; HIPCHK(hipMemset(zg0, 0, nn * 4)); HIPCHK(hipMemset(zc, 0, nn * 4)); }
        // C' = the bias itself: no copy in the timed path
        g.zstat_in = zs; g.zs_stride = (long)cap_rows; g.zparts = 12; g.zD = 1152; g.zw = 96; g.zG = zg0; g.zC = bias ? bias : zc;
        g.zt_slot_stride = 0; g.zeps = 1e-5f;
        g.debug &= ~64;
    }
    if (g.epi > EPI_GEGLU || g.tile > 127) return fail(EZDIT_E_INVALID, "bad gemm variant %d", variant);
    if (g.epi != EPI_PARTIAL) g.splitk = 1;
    char config[32];
    snprintf(config, sizeof config, "gemm variant %d", variant);
    return hook_launch("k_gemm", config, [&] { return launch_gemm(g, (hipStream_t)stream); });
}

// EPI_RESID (un-split residual projection + partial LayerNorm statistics + next operand), stand-alone:
// h_out = h_in + gate * (A . W^T + bias); zu = bf16(h_out * zg); zstat[N / tile-width chunks][row] = (sum, sum of squares) over the chunk's columns (part-major)
int ezdit_test_resid(int tile, const void* A, int lda, const void* W, int ldw, const float* bias, const float* h_in, const float* gate, const float* zg,
                     float* h_out, void* zu, int ld_zu, void* zstat, int M, int N, int K, ezdit_stream stream) {
    if (K % 64) return fail(EZDIT_E_INVALID, "K=%d must be a multiple of 64", K);
    GemmArgs g = resid_args(tile, (const bf16_t*)A, lda, (const bf16_t*)W, ldw, (int)rup(N, 128), bias, h_in, gate, zg, h_out, (bf16_t*)zu, ld_zu, (float2*)zstat, M, M, N, K);   // zstat [N tiles][M]
    g.ts = g_gemm_ts; g.ts_cap = g_gemm_ts_cap;
    return hook_launch("the residual GEMM", "residual GEMM configuration", [&] { return launch_gemm(g, (hipStream_t)stream); });
}

// the skip path's forms of the same launch (GemmArgs COPY2 / ZIN), stand-alone:
//   zu2 != NULL (COPY2; gate and h_in required): additionally zu2 = bf16(h_out * zg2)
//   zstat_in2 != NULL (ZIN; no gate, no h_in): the operand A is bf16(x * g) of rows whose (sum, sum of squares) over zD columns come in two part-major sets of zparts parts
//   (zstat_in, zstat_in2: [zparts][M] float pairs); acc := r (acc - mu zG[col]) + bias[col] (bias = C'), then the epilogue as above.  h_out NULL = the fp32 stream is not stored
int ezdit_test_resid_skip(int tile, const void* A, int lda, const void* W, int ldw, const float* bias, const float* h_in, const float* gate, const float* zg,
                          float* h_out, void* zu, int ld_zu, void* zstat, int M, int N, int K,
                          const float* zg2, void* zu2, int ld_zu2, const void* zstat_in, const void* zstat_in2, int zparts, int zD, const float* zG, ezdit_stream stream) {
    if (K % 64) return fail(EZDIT_E_INVALID, "K=%d must be a multiple of 64", K);
    GemmArgs g = resid_args(tile, (const bf16_t*)A, lda, (const bf16_t*)W, ldw, (int)rup(N, 128), bias, h_in, gate, zg, h_out, (bf16_t*)zu, ld_zu, (float2*)zstat, M, M, N, K);   // zstat [N tiles][M]
    g.zu2 = (bf16_t*)zu2; g.ld_zu2 = ld_zu2; g.zg2 = zg2;
    g.zstat_in = (const float2*)zstat_in; g.zstat_in2 = (const float2*)zstat_in2; g.zparts = zparts; g.zD = zD; g.zG = zG; g.zeps = 1e-5f;
    return hook_launch("the residual GEMM", "residual GEMM configuration", [&] { return launch_gemm(g, (hipStream_t)stream); });
}

// the DUAL form of the same launch (GemmArgs.zd; the attention-out projection when single-key batch elements skip cross-attention), stand-alone: the rows OUTSIDE
// [act_row0, act_row1) get  h_out = h_in + gate * (A . W^T + bias) + zd[row / rows_per_b]  and  zu = bf16(h_out * zg2); the rows inside it no zd and the gain zg
int ezdit_test_resid_dual(int tile, const void* A, int lda, const void* W, int ldw, const float* bias, const float* h_in, const float* gate, const float* zg,
                          float* h_out, void* zu, int ld_zu, void* zstat, int M, int N, int K,
                          const float* zd, long zd_stride, const float* zg2, int act_row0, int act_row1, int rows_per_b, ezdit_stream stream) {
    if (K % 64) return fail(EZDIT_E_INVALID, "K=%d must be a multiple of 64", K);
    if (!zd || rows_per_b <= 0) return fail(EZDIT_E_INVALID, "the DUAL form needs zd and rows_per_b");
    GemmArgs g = resid_args(tile, (const bf16_t*)A, lda, (const bf16_t*)W, ldw, (int)rup(N, 128), bias, h_in, gate, zg, h_out, (bf16_t*)zu, ld_zu, (float2*)zstat, M, M, N, K);   // zstat [N tiles][M]
    g.rows_per_b = rows_per_b;
    g.zd = zd; g.zd_stride = zd_stride; g.zg2 = zg2; g.act_row0 = act_row0; g.act_row1 = act_row1;
    return hook_launch("the residual GEMM", "residual GEMM configuration", [&] { return launch_gemm(g, (hipStream_t)stream); });
}

// consumer side of the LayerNorm algebra, stand-alone (GemmArgs.z*: what gemm() above fills from its ZIn): epi = EPI_GEGLU (out bf16 [M][ldo]) or EPI_QKV
// (nothing goes to `out`; q / k / v in the attention layouts, HeadNormArgs) with  acc := r (acc - mu zG[slot][col]) + zC[slot][col]  in the epilogue, (mu, r) merged from the
// part-major partial statistics zstat_in [zparts][zs_stride], slot = *cur_step + row_slot[row / rows_per_b] (NULL = 0 each).  EPI_QKV: perm = 1 with RoPE tables is the fused
// q | k | v projection (N = 3 H dh, W rows packed by EZDIT_T_QKROPE), perm = 0 with k = v = NULL and no tables the q-only projection of batched prompts (N = H dh)
int ezdit_test_consumer(int tile, int epi, int epi_lds, const void* A, int lda, const void* W, int ldw, int wrows, const float* bias, void* out, int ldo, int M, int N, int K,
                        const void* zstat_in, long zs_stride, int zparts, int zD, int zw, const float* zG, const float* zC, long zt_slot_stride, float zeps,
                        const int* cur_step, const int* row_slot, int rows_per_b,
                        const float* qn_w, const float* qn_b, const float* kn_w, const float* kn_b, const float* rope_cos, const float* rope_sin,
                        void* q, void* k, void* v, int B, int H, int L, int Lp, int dh, int perm, ezdit_stream stream) {
    if (K % 64) return fail(EZDIT_E_INVALID, "K=%d must be a multiple of 64", K);
    if (epi != EPI_GEGLU && epi != EPI_QKV) return fail(EZDIT_E_INVALID, "epi %d is no LayerNorm-algebra consumer", epi);
    // (EPI_QKV without statistics: the plain projection of a finished operand -- the instantiation the step launches with the LayerNorm algebra off)
    if ((!zstat_in && epi != EPI_QKV) || rows_per_b <= 0) return fail(EZDIT_E_INVALID, "the consumer form needs zstat_in and rows_per_b");
    GemmArgs g;
    memset(&g, 0, sizeof g);
    g.A = (const bf16_t*)A; g.lda = lda; g.W = (const bf16_t*)W; g.ldw = ldw; g.wrows = wrows; g.bias = bias; g.out = out; g.ldo = ldo;
    g.M = M; g.N = N; g.K = K; g.splitk = 1; g.epi = epi; g.tile = tile; g.xcd_map = 1; g.epi_lds = epi_lds;
    g.zstat_in = (const float2*)zstat_in; g.zs_stride = zs_stride; g.zparts = zparts; g.zD = zD; g.zw = zw; g.zG = zG; g.zC = zC; g.zt_slot_stride = zt_slot_stride; g.zeps = zeps;
    g.cur_step = cur_step; g.row_slot = row_slot; g.rows_per_b = rows_per_b;
    if (epi == EPI_QKV) {
        if (M != B * L) return fail(EZDIT_E_INVALID, "M=%d != B L = %d", M, B * L);
        HeadNormArgs& hn = g.hn;
        hn.q_col = 0; hn.k_col = k ? H * dh : -1; hn.v_col = v ? 2 * H * dh : -1;
        hn.qn_w = qn_w; hn.qn_b = qn_b; hn.kn_w = kn_w; hn.kn_b = kn_b; hn.rope_cos = rope_cos; hn.rope_sin = rope_sin;
        hn.q = (bf16_t*)q; hn.k = (bf16_t*)k; hn.v = (bf16_t*)v;
        hn.B = B; hn.H = H; hn.L = L; hn.Lp = Lp; hn.dh = dh; hn.perm = perm;
    }
    return hook_launch("the consumer GEMM", "consumer GEMM configuration", [&] { return launch_gemm(g, (hipStream_t)stream); });
}

// the RoPE tables as ezdit_bind_workspace fills them: cos / sin fp32 [max_len][dh / 2]
int ezdit_test_rope_table(float* cosT, float* sinT, int max_len, int dh, ezdit_stream stream) {
    if (!cosT || !sinT || max_len <= 0 || dh <= 0 || dh % 2) return fail(EZDIT_E_INVALID, "bad RoPE table request");
    return hook_launch("k_rope_table", "", [&] { launch_rope_table(cosT, sinT, max_len, dh, (hipStream_t)stream); return 0; });
}

// cross-attention with its own q projection and the LayerNorm algebra, stand-alone (the AttnArgs forward_impl builds for fuse_q2): q = LN_head(r (xu . xw_h^T - mu zG) + zC),
// then softmax(q k^T / sqrt(dh) + mask) v over the batch elements [b0, b0 + B) of the buffers (all pointers are given for batch element 0)
int ezdit_test_cross_attention(const void* xu, int ldu, const void* xw, int ldw, int xw_rows, int xK, const float* qn_w, const float* qn_b,
                               const void* k, const void* v, const uint8_t* kmask, void* out, int ldo, int B, int b0, int H, int dh, int Lq, int Lk, int Lqp, int Lkp,
                               const void* zstat_in, long zs_stride, int zparts, int zD, int zw, const float* zG, const float* zC, float zeps,
                               int xk2, int qtile, int xcd_map, ezdit_stream stream) {
    if (!xu || !xw || xK <= 0 || xK % 64) return fail(EZDIT_E_INVALID, "the fused projection needs xu, xw and xK a multiple of 64");
    AttnArgs a;
    memset(&a, 0, sizeof a);
    a.k = (const bf16_t*)k; a.v = (const bf16_t*)v; a.kmask = kmask;
    a.out = (bf16_t*)out; a.ldo = ldo;
    a.B = B; a.b0 = b0; a.H = H; a.Lq = Lq; a.Lk = Lk; a.Lqp = Lqp; a.Lkp = Lkp; a.dh = dh;
    a.xu = (const bf16_t*)xu; a.ldu = ldu; a.xw = (const bf16_t*)xw; a.ldw = ldw; a.xw_rows = xw_rows; a.xK = xK;
    a.qn_w = qn_w; a.qn_b = qn_b; a.nkh = 4; a.xk2 = xk2; a.qtile = qtile; a.xcd_map = xcd_map;
    a.zstat_in = (const float2*)zstat_in; a.zs_stride = zs_stride; a.zparts = zparts; a.zD = zD; a.zw = zw; a.zG = zG; a.zC = zC; a.zeps = zeps;
    return hook_launch("k_attn", "attention configuration", [&] { return launch_attention(a, (hipStream_t)stream); });
}

// what both plain-attention hooks refuse.  Everything that bounds an address comes before the first HIP call and before the handle is looked at (k_attn itself checks
// nothing: it reads Lkp / 32 sub-tiles of whole 64-row query tiles); a fine description with no handle is refused last.  With a key mask the hook then waits for `stream`
// and reads the mask back, as the varlen hook does for its lengths: a batch element without a valid key has no softmax (0 / 0), which is the caller's mistake and no
// property of the kernel
static int attn_hook_refusals(const ezdit_handle* h, const void* q, const void* k, const void* v, const uint8_t* kmask, const void* out, int B, int Lq, int Lk,
                              int Lqp, int Lkp, hipStream_t stream) {
    if (!q || !k || !v || !out) return fail(EZDIT_E_INVALID, "null q, k, v or out");
    if (B <= 0 || Lq <= 0 || Lk <= 0) return fail(EZDIT_E_INVALID, "bad shape B=%d Lq=%d Lk=%d", B, Lq, Lk);
    if (Lqp < Lq || Lkp < Lk) return fail(EZDIT_E_INVALID, "padded lengths Lqp=%d Lkp=%d below Lq=%d Lk=%d", Lqp, Lkp, Lq, Lk);
    if (Lqp % 64 || Lkp % 64) return fail(EZDIT_E_INVALID, "padded lengths Lqp=%d Lkp=%d must be multiples of 64", Lqp, Lkp);
    if (!h) return fail(EZDIT_E_INVALID, "null handle");
    if (kmask) {
        std::vector<uint8_t> km((size_t)B * Lk);
        HIPCHK(hipStreamSynchronize(stream));
        HIPCHK(hipMemcpy(km.data(), kmask, km.size(), hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b) {
            bool any = false;
            for (int j = 0; j < Lk && !any; ++j) any = km[(size_t)b * Lk + j] != 0;
            if (!any) return fail(EZDIT_E_INVALID, "kmask leaves batch element %d without a valid key", b);
        }
    }
    return 0;
}

int ezdit_test_attention(ezdit_handle* h, const void* q, const void* k, const void* v, const uint8_t* kmask, void* out, int B,
                         int Lq, int Lk, int Lqp, int Lkp, ezdit_stream stream) {
    if (int rc = attn_hook_refusals(h, q, k, v, kmask, out, B, Lq, Lk, Lqp, Lkp, (hipStream_t)stream)) return rc;
    AttnArgs a;
    memset(&a, 0, sizeof a);
    a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.v = (const bf16_t*)v; a.kmask = kmask;
    a.nkh = h->opt_attn_nkh; a.xcd_map = h->opt_attn_xcd;
    a.out = (bf16_t*)out; a.ldo = h->ldD;
    a.B = B; a.H = h->H; a.Lq = Lq; a.Lk = Lk; a.Lqp = Lqp; a.Lkp = Lkp; a.dh = h->dh;
    a.ts = g_gemm_ts; a.ts_cap = g_gemm_ts_cap;
    return hook_launch("k_attn", "attention configuration", [&] { return launch_attention(a, (hipStream_t)stream); });
}

int ezdit_test_attention_varlen(ezdit_handle* h, const void* q, const void* k, const void* v, const uint8_t* kmask, void* out, int B,
                                int Lq, int Lk, int Lqp, int Lkp, const int32_t* dev_klen, ezdit_stream stream) {
    if (dev_klen && Lq != Lk) return fail(EZDIT_E_INVALID, "per-batch-element lengths are a self-attention form: Lq %d != Lk %d", Lq, Lk);
    if (int rc = attn_hook_refusals(h, q, k, v, kmask, out, B, Lq, Lk, Lqp, Lkp, (hipStream_t)stream)) return rc;
    if (dev_klen) {   // a test hook may wait: the lengths bound what the kernel reads and which rows it zeroes
        std::vector<int> kl((size_t)B);
        HIPCHK(hipStreamSynchronize((hipStream_t)stream));
        HIPCHK(hipMemcpy(kl.data(), dev_klen, (size_t)B * sizeof(int), hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b)
            if (kl[b] < 1 || kl[b] > Lk) return fail(EZDIT_E_INVALID, "klen[%d] = %d outside [1, Lk = %d]", b, kl[b], Lk);
    }
    AttnArgs a;
    memset(&a, 0, sizeof a);
    a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.v = (const bf16_t*)v; a.kmask = kmask;
    a.nkh = h->opt_attn_nkh; a.xcd_map = h->opt_attn_xcd;
    a.out = (bf16_t*)out; a.ldo = h->ldD;
    a.B = B; a.H = h->H; a.Lq = Lq; a.Lk = Lk; a.Lqp = Lqp; a.Lkp = Lkp; a.dh = h->dh;
    a.klen = dev_klen;
    return hook_launch("k_attn", "attention configuration", [&] { return launch_attention(a, (hipStream_t)stream); });
}

// the band form of plain self-attention, stand-alone.  ALWAYS the band instantiation, also for a radius that masks nothing (>= L - 1): that run is what compares the
// band code with the plain kernel on equal masks
int ezdit_test_attention_band(ezdit_handle* h, const void* q, const void* k, const void* v, void* out, int B, int L, int Lp, const int32_t* dev_klen, int radius,
                              ezdit_stream stream) {
    if (radius < 1) return fail(EZDIT_E_INVALID, "radius = %d: the band form needs a radius >= 1", radius);
    if (int rc = attn_hook_refusals(h, q, k, v, nullptr, out, B, L, L, Lp, Lp, (hipStream_t)stream)) return rc;
    if (dev_klen) {   // a test hook may wait: the lengths bound what the kernel reads and which rows it zeroes
        std::vector<int> kl((size_t)B);
        HIPCHK(hipStreamSynchronize((hipStream_t)stream));
        HIPCHK(hipMemcpy(kl.data(), dev_klen, (size_t)B * sizeof(int), hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b)
            if (kl[b] < 1 || kl[b] > L) return fail(EZDIT_E_INVALID, "klen[%d] = %d outside [1, L = %d]", b, kl[b], L);
    }
    AttnArgs a;
    memset(&a, 0, sizeof a);
    a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.v = (const bf16_t*)v;
    a.nkh = h->opt_attn_nkh; a.xcd_map = h->opt_attn_xcd;
    a.out = (bf16_t*)out; a.ldo = h->ldD;
    a.B = B; a.H = h->H; a.Lq = L; a.Lk = L; a.Lqp = Lp; a.Lkp = Lp; a.dh = h->dh;
    a.klen = dev_klen;
    a.band = radius;
    return hook_launch("k_attn", "attention configuration", [&] { return launch_attention(a, (hipStream_t)stream); });
}

// the timeline form, stand-alone: what both hooks share.  The key mask is read back (a test hook may wait), the table is built and checked as the setter does it
// (lens none), lives in device memory of the hook's own for the launch of the batch elements [b0, b0 + B), and goes when the launch is done
static int timeline_hook(AttnArgs& a, const float* weights, int S, hipStream_t st) {
    if (!weights) return fail(EZDIT_E_INVALID, "null weights");
    if (S < 1 || S > TL_MAXS) return fail(EZDIT_E_INVALID, "S = %d outside [1, %d]", S, TL_MAXS);
    if (a.Lk != 128 * S || a.Lkp != a.Lk) return fail(EZDIT_E_INVALID, "S = %d prompts are Lk = Lkp = %d keys, not Lk = %d, Lkp = %d", S, 128 * S, a.Lk, a.Lkp);
    if (a.B <= 0 || a.b0 < 0 || a.Lq <= 0) return fail(EZDIT_E_INVALID, "bad shape B=%d b0=%d Lq=%d", a.B, a.b0, a.Lq);
    std::vector<uint8_t> km;
    HIPCHK(hipStreamSynchronize(st));
    if (a.kmask) {
        km.resize((size_t)a.B * a.Lk);
        HIPCHK(hipMemcpy(km.data(), a.kmask + (size_t)a.b0 * a.Lk, km.size(), hipMemcpyDeviceToHost));
    }
    std::vector<float> v;
    if (int rc = timeline_table(weights, a.B, S, a.Lq, nullptr, a.kmask ? km.data() : nullptr, &v)) return rc;
    const size_t nb = (size_t)a.B * S * a.Lq, ns = (size_t)a.B * S * 2, skip_b = (size_t)a.b0 * S * a.Lq, skip_s = (size_t)a.b0 * S * 2;
    float* dev = nullptr;   // [b0 + B][S][Lq] biases | [b0 + B][S] supports: launch_attention advances both by b0 batch elements
    const size_t sup_at = (skip_b + nb + 1) & ~(size_t)1;   // (the supports are read as 8-byte pairs)
    HIPCHK(hipMalloc(&dev, (sup_at + skip_s + ns) * sizeof(float)));
    float* dsup = dev + sup_at;
    hipError_t e = hipMemcpy(dev + skip_b, v.data(), nb * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dsup + skip_s, v.data() + nb, ns * sizeof(float), hipMemcpyHostToDevice);
    int rc = e == hipSuccess ? EZDIT_OK : fail(EZDIT_E_HIP, "upload of the timeline table failed: %s", hipGetErrorString(e));
    if (!rc) {
        a.tlb = dev; a.tlsup = reinterpret_cast<const int2*>(dsup);
        rc = hook_launch("k_attn (timeline)", "attention configuration", [&] { return launch_attention(a, st); });
    }
    const hipError_t es = hipStreamSynchronize(st);
    (void)hipFree(dev);
    if (!rc && es != hipSuccess) rc = fail(EZDIT_E_HIP, "k_attn (timeline) failed: %s", hipGetErrorString(es));
    return rc;
}

// the timeline form of the plain 8-wave kernel (the q2_pp / q_raw paths of cross-attention).  ALWAYS the TL instantiation, also for S = 1 with every weight 1: that run
// is what compares it with ezdit_test_attention on equal inputs
int ezdit_test_attention_timeline(ezdit_handle* h, const void* q, const void* k, const void* v, const uint8_t* kmask, void* out, int B,
                                  int Lq, int Lk, int Lqp, int Lkp, const float* weights, int S, ezdit_stream stream) {
    if (int rc = attn_hook_refusals(h, q, k, v, kmask, out, B, Lq, Lk, Lqp, Lkp, (hipStream_t)stream)) return rc;
    AttnArgs a;
    memset(&a, 0, sizeof a);
    a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.v = (const bf16_t*)v; a.kmask = kmask;
    a.nkh = 4; a.xcd_map = h->opt_attn_xcd;
    a.out = (bf16_t*)out; a.ldo = h->ldD;
    a.B = B; a.H = h->H; a.Lq = Lq; a.Lk = Lk; a.Lqp = Lqp; a.Lkp = Lkp; a.dh = h->dh;
    return timeline_hook(a, weights, S, (hipStream_t)stream);
}

// ... and of the fused-projection forms with the LayerNorm algebra: the arguments of ezdit_test_cross_attention, then weights [B][S][Lq] (HOST) of the launched batch elements
int ezdit_test_cross_attention_timeline(const void* xu, int ldu, const void* xw, int ldw, int xw_rows, int xK, const float* qn_w, const float* qn_b,
                                        const void* k, const void* v, const uint8_t* kmask, void* out, int ldo, int B, int b0, int H, int dh, int Lq, int Lk, int Lqp, int Lkp,
                                        const void* zstat_in, long zs_stride, int zparts, int zD, int zw, const float* zG, const float* zC, float zeps,
                                        int xk2, int qtile, int xcd_map, const float* weights, int S, ezdit_stream stream) {
    if (!xu || !xw || xK <= 0 || xK % 64) return fail(EZDIT_E_INVALID, "the fused projection needs xu, xw and xK a multiple of 64");
    if (!k || !v || !out || !zstat_in) return fail(EZDIT_E_INVALID, "null k, v, out or statistics");
    if (qtile != 32 && qtile != 64) return fail(EZDIT_E_INVALID, "qtile = %d: 32 or 64", qtile);
    if (qtile == 32 && (!xcd_map || (xK / 64) % 2)) return fail(EZDIT_E_INVALID, "qtile = 32 needs the XCD map and an even number of K tiles");
    AttnArgs a;
    memset(&a, 0, sizeof a);
    a.k = (const bf16_t*)k; a.v = (const bf16_t*)v; a.kmask = kmask;
    a.out = (bf16_t*)out; a.ldo = ldo;
    a.B = B; a.b0 = b0; a.H = H; a.Lq = Lq; a.Lk = Lk; a.Lqp = Lqp; a.Lkp = Lkp; a.dh = dh;
    a.xu = (const bf16_t*)xu; a.ldu = ldu; a.xw = (const bf16_t*)xw; a.ldw = ldw; a.xw_rows = xw_rows; a.xK = xK;
    a.qn_w = qn_w; a.qn_b = qn_b; a.nkh = 4; a.xk2 = xk2; a.qtile = qtile; a.xcd_map = xcd_map;
    a.zstat_in = (const float2*)zstat_in; a.zs_stride = zs_stride; a.zparts = zparts; a.zD = zD; a.zw = zw; a.zG = zG; a.zC = zC; a.zeps = zeps;
    return timeline_hook(a, weights, S, (hipStream_t)stream);
}

// the emphasis form, stand-alone: what both hooks share.  The key mask is read back (a test hook may wait), the table is built and checked as the setter does it, lives
// in device memory of the hook's own for the launch of the batch elements [b0, b0 + B), and goes when the launch is done.  keep_on = 0: a table of zeros launches the
// plain instantiation, as the setter would; 1: the KW instantiation whatever the table holds
static int keyweight_hook(AttnArgs& a, const float* weights, int keep_on, hipStream_t st) {
    if (!weights) return fail(EZDIT_E_INVALID, "null weights");
    if (a.B <= 0 || a.b0 < 0 || a.Lq <= 0 || a.Lk <= 0 || a.Lkp < a.Lk) return fail(EZDIT_E_INVALID, "bad shape B=%d b0=%d Lq=%d Lk=%d Lkp=%d", a.B, a.b0, a.Lq, a.Lk, a.Lkp);
    std::vector<uint8_t> km;
    HIPCHK(hipStreamSynchronize(st));
    if (a.kmask) {
        km.resize((size_t)a.B * a.Lk);
        HIPCHK(hipMemcpy(km.data(), a.kmask + (size_t)a.b0 * a.Lk, km.size(), hipMemcpyDeviceToHost));
    }
    std::vector<float> v;
    bool any = false;
    if (int rc = keyweight_table(weights, a.B, a.Lk, a.Lkp, a.kmask ? km.data() : nullptr, &v, &any)) return rc;
    if (!any && !keep_on) return hook_launch("k_attn", "attention configuration", [&] { return launch_attention(a, st); });
    const size_t nb = (size_t)a.B * a.Lkp, skip_b = (size_t)a.b0 * a.Lkp;
    float* dev = nullptr;   // [b0 + B][Lkp]: launch_attention advances it by b0 batch elements
    HIPCHK(hipMalloc(&dev, (skip_b + nb) * sizeof(float)));
    const hipError_t e = hipMemcpy(dev + skip_b, v.data(), nb * sizeof(float), hipMemcpyHostToDevice);
    int rc = e == hipSuccess ? EZDIT_OK : fail(EZDIT_E_HIP, "upload of the key-bias table failed: %s", hipGetErrorString(e));
    if (!rc) {
        a.kbias = dev;
        rc = hook_launch("k_attn (emphasis)", "attention configuration", [&] { return launch_attention(a, st); });
    }
    const hipError_t es = hipStreamSynchronize(st);
    (void)hipFree(dev);
    if (!rc && es != hipSuccess) rc = fail(EZDIT_E_HIP, "k_attn (emphasis) failed: %s", hipGetErrorString(es));
    return rc;
}

// the emphasis form of the plain 8-wave kernel (the q2_pp / q_raw paths of cross-attention): the arguments of ezdit_test_attention_timeline with natural weights [B][Lk] (HOST)
int ezdit_test_attention_keyweights(ezdit_handle* h, const void* q, const void* k, const void* v, const uint8_t* kmask, void* out, int B,
                                    int Lq, int Lk, int Lqp, int Lkp, const float* weights, int keep_on, ezdit_stream stream) {
    if (int rc = attn_hook_refusals(h, q, k, v, kmask, out, B, Lq, Lk, Lqp, Lkp, (hipStream_t)stream)) return rc;
    AttnArgs a;
    memset(&a, 0, sizeof a);
    a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.v = (const bf16_t*)v; a.kmask = kmask;
    a.nkh = 4; a.xcd_map = h->opt_attn_xcd;
    a.out = (bf16_t*)out; a.ldo = h->ldD;
    a.B = B; a.H = h->H; a.Lq = Lq; a.Lk = Lk; a.Lqp = Lqp; a.Lkp = Lkp; a.dh = h->dh;
    return keyweight_hook(a, weights, keep_on, (hipStream_t)stream);
}

// ... and of the fused-projection forms with the LayerNorm algebra: the arguments of ezdit_test_cross_attention, then weights [B][Lk] (HOST) of the launched batch elements
int ezdit_test_cross_attention_keyweights(const void* xu, int ldu, const void* xw, int ldw, int xw_rows, int xK, const float* qn_w, const float* qn_b,
                                          const void* k, const void* v, const uint8_t* kmask, void* out, int ldo, int B, int b0, int H, int dh, int Lq, int Lk, int Lqp, int Lkp,
                                          const void* zstat_in, long zs_stride, int zparts, int zD, int zw, const float* zG, const float* zC, float zeps,
                                          int xk2, int qtile, int xcd_map, const float* weights, int keep_on, ezdit_stream stream) {
    if (!xu || !xw || xK <= 0 || xK % 64) return fail(EZDIT_E_INVALID, "the fused projection needs xu, xw and xK a multiple of 64");
    if (!k || !v || !out || !zstat_in) return fail(EZDIT_E_INVALID, "null k, v, out or statistics");
    if (qtile != 32 && qtile != 64) return fail(EZDIT_E_INVALID, "qtile = %d: 32 or 64", qtile);
    if (qtile == 32 && (!xcd_map || (xK / 64) % 2)) return fail(EZDIT_E_INVALID, "qtile = 32 needs the XCD map and an even number of K tiles");
    if (H <= 0 || (dh != 64 && dh != 72) || Lkp % 128 || Lqp < Lq) return fail(EZDIT_E_INVALID, "bad shape H=%d dh=%d Lq=%d Lqp=%d Lkp=%d", H, dh, Lq, Lqp, Lkp);
    AttnArgs a;
    memset(&a, 0, sizeof a);
    a.k = (const bf16_t*)k; a.v = (const bf16_t*)v; a.kmask = kmask;
    a.out = (bf16_t*)out; a.ldo = ldo;
    a.B = B; a.b0 = b0; a.H = H; a.Lq = Lq; a.Lk = Lk; a.Lqp = Lqp; a.Lkp = Lkp; a.dh = dh;
    a.xu = (const bf16_t*)xu; a.ldu = ldu; a.xw = (const bf16_t*)xw; a.ldw = ldw; a.xw_rows = xw_rows; a.xK = xK;
    a.qn_w = qn_w; a.qn_b = qn_b; a.nkh = 4; a.xk2 = xk2; a.qtile = qtile; a.xcd_map = xcd_map;
    a.zstat_in = (const float2*)zstat_in; a.zs_stride = zs_stride; a.zparts = zparts; a.zD = zD; a.zw = zw; a.zG = zG; a.zC = zC; a.zeps = zeps;
    return keyweight_hook(a, weights, keep_on, (hipStream_t)stream);
}

int ezdit_test_final_conv(const float* y, int ldy, const float* w, const float* b, float* out, int B, int C, int L, const int32_t* dev_lens,
                          ezdit_stream stream) {
    if (!y || !w || !b || !out) return fail(EZDIT_E_INVALID, "null argument");
    if (B <= 0 || L <= 0 || C <= 0 || ldy < C) return fail(EZDIT_E_INVALID, "bad shape B=%d C=%d L=%d ldy=%d", B, C, L, ldy);
    // (the kernel's two-halves walk of a weight row needs C % 8 == 0; every shipped model has C = 128)
    if (C % 8) return fail(EZDIT_E_UNSUPPORTED, "C = %d is not a multiple of 8", C);
    if (dev_lens) {
        std::vector<int> ln((size_t)B);
        HIPCHK(hipStreamSynchronize((hipStream_t)stream));
        HIPCHK(hipMemcpy(ln.data(), dev_lens, (size_t)B * sizeof(int), hipMemcpyDeviceToHost));
        for (int i = 0; i < B; ++i)
            if (ln[i] < 1 || ln[i] > L) return fail(EZDIT_E_INVALID, "lens[%d] = %d outside [1, L = %d]", i, ln[i], L);
    }
    FinalConvArgs fc;
    fc.y = y; fc.ldy = ldy; fc.w = w; fc.b = b; fc.out = out; fc.B = B; fc.C = C; fc.L = L; fc.lens = dev_lens;
    return hook_launch("k_final_conv", "", [&] { launch_final_conv(fc, (hipStream_t)stream); return 0; });
}

// the row operator (launch_row: k_row / k_row_w) on a caller-described RowArgs.  Everything that bounds an address is checked here, before the first HIP call: the kernels
// themselves check nothing (k_row would drop the columns beyond 2048 and the slabs beyond 8 without a word)
int ezdit_test_row(const ezdit_test_row_args* t, ezdit_stream stream) {
    if (!t) return fail(EZDIT_E_INVALID, "null argument");
    if (t->M <= 0 || t->D <= 0 || t->L <= 0) return fail(EZDIT_E_INVALID, "bad shape M=%d D=%d L=%d", t->M, t->D, t->L);
    if (t->nsplit < 0) return fail(EZDIT_E_INVALID, "nsplit = %d", t->nsplit);
    if (t->mode < 0 || t->mode > 2) return fail(EZDIT_E_INVALID, "mode = %d (0 COPY, 1 RES, 2 SET)", t->mode);
    if ((t->wt | t->variant | t->affine | t->part_bf16) & ~1) return fail(EZDIT_E_INVALID, "wt, variant, affine and part_bf16 are 0 or 1");
    if (t->D % 4) return fail(EZDIT_E_UNSUPPORTED, "D = %d is not a multiple of 4 (16-byte chunks)", t->D);
    if (t->D > 2048) return fail(EZDIT_E_UNSUPPORTED, "D = %d is beyond the 2048 columns of the workgroup-per-row form", t->D);
    if (t->nsplit > 8) return fail(EZDIT_E_UNSUPPORTED, "nsplit = %d is beyond the 8 slabs of the workgroup-per-row form", t->nsplit);
    auto misaligned = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
    const int width = t->skip ? 2 * t->D : t->D;
    if (t->mode != 2 && !t->h_in) return fail(EZDIT_E_INVALID, "mode %d reads h_in", t->mode);
    if (t->mode != 0 && t->nsplit > 0) {
        if (!t->part) return fail(EZDIT_E_INVALID, "mode %d with %d slabs reads part", t->mode, t->nsplit);
        if (t->ld_part < t->D || t->ld_part % 4 || t->part_stride % 4 || (t->nsplit > 1 && t->part_stride <= 0))
            return fail(EZDIT_E_INVALID, "bad slab layout ld_part=%d part_stride=%ld", t->ld_part, (long)t->part_stride);
    }
    if (t->gate && (t->gate_slot_stride < 0 || t->gate_slot_stride % 4)) return fail(EZDIT_E_INVALID, "gate_slot_stride = %ld", (long)t->gate_slot_stride);
    if (t->cn && !t->skip) return fail(EZDIT_E_INVALID, "cn without skip");
    if (t->skip && !t->u) return fail(EZDIT_E_INVALID, "skip without u: the concatenation exists for the LayerNorm only");
    if (t->u) {
        if (!t->ln_g || !t->ln_c) return fail(EZDIT_E_INVALID, "u without ln_g / ln_c");
        if (t->ln_slot_stride < 0 || t->ln_slot_stride % 4) return fail(EZDIT_E_INVALID, "ln_slot_stride = %ld", (long)t->ln_slot_stride);
        if (t->ld_u < width || t->ld_u % 4) return fail(EZDIT_E_INVALID, "ld_u = %d: below the written width %d or not a multiple of 4", t->ld_u, width);
    }
    if (misaligned(t->h_in, 16) || misaligned(t->h_out, 16) || misaligned(t->part, t->part_bf16 ? 8 : 16) || misaligned(t->bias, 16) || misaligned(t->gate, 16) ||
        misaligned(t->ln_g, 16) || misaligned(t->ln_c, 16) || misaligned(t->skip, 16) || misaligned(t->cn, 16) || misaligned(t->u, 8))
        return fail(EZDIT_E_INVALID, "a pointer breaks the alignment of the 16-byte (bf16: 8-byte) accesses");
    const bool slotted = (t->gate && t->mode != 0) || t->u;
    if (slotted) {
        if (t->n_slots < 1) return fail(EZDIT_E_INVALID, "n_slots = %d", t->n_slots);
        // a test hook may wait: the slots bound what the kernel reads of the gate / LayerNorm tables
        const int B = (t->M + t->L - 1) / t->L;
        int cur = 0;
        std::vector<int> rs((size_t)B, 0);
        if (t->cur_step || t->row_slot) HIPCHK(hipStreamSynchronize((hipStream_t)stream));
        if (t->cur_step) HIPCHK(hipMemcpy(&cur, t->cur_step, sizeof(int), hipMemcpyDeviceToHost));
        if (t->row_slot) HIPCHK(hipMemcpy(rs.data(), t->row_slot, (size_t)B * sizeof(int), hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b)
            if (cur + rs[b] < 0 || cur + rs[b] >= t->n_slots)
                return fail(EZDIT_E_INVALID, "slot %d + %d of batch element %d outside [0, n_slots = %d)", cur, rs[b], b, t->n_slots);
    }
    RowArgs r;
    memset(&r, 0, sizeof r);
    r.h_in = t->h_in; r.h_out = t->h_out;
    r.part = (const float*)t->part; r.nsplit = t->nsplit; r.part_stride = (long)t->part_stride; r.ld_part = t->ld_part; r.part_bf16 = t->part_bf16;
    r.bias = t->bias; r.gate = t->gate; r.gate_slot_stride = (long)t->gate_slot_stride; r.mode = t->mode;
    r.ln_g = t->ln_g; r.ln_c = t->ln_c; r.ln_slot_stride = (long)t->ln_slot_stride;
    r.cn_scale = t->cn_scale; r.cn_tab = t->cn_tab; r.skip = t->skip; r.cn = t->cn;
    r.u = (bf16_t*)t->u; r.ld_u = t->ld_u;
    r.M = t->M; r.D = t->D; r.L = t->L;
    r.cur_step = t->cur_step; r.row_slot = t->row_slot;
    r.wt = t->wt; r.variant = t->variant; r.affine = t->affine;
    return hook_launch("k_row", "", [&] { launch_row(r, (hipStream_t)stream); return 0; });
}

// per-head LayerNorm (+ RoPE) of q / k and the cast of v into the attention layouts (launch_headnorm: k_headnorm), the un-fused form of the fused QKV epilogue
int ezdit_test_headnorm(const float* x, int ldx, int q_col, int k_col, int v_col, const float* qn_w, const float* qn_b, const float* kn_w, const float* kn_b,
                        const float* rope_cos, const float* rope_sin, void* q, void* k, void* v, int B, int H, int L, int Lp, int dh, ezdit_stream stream) {
    if (B <= 0 || H <= 0 || L <= 0 || Lp < L) return fail(EZDIT_E_INVALID, "bad shape B=%d H=%d L=%d Lp=%d", B, H, L, Lp);
    if (dh != 64 && dh != 72) return fail(EZDIT_E_UNSUPPORTED, "head_dim %d (64 and 72 are built)", dh);
    if (q_col < -1 || k_col < -1 || v_col < -1 || (q_col < 0 && k_col < 0 && v_col < 0)) return fail(EZDIT_E_INVALID, "no part to build");
    const int cols[3] = {q_col, k_col, v_col};
    for (int i = 0; i < 3; ++i)
        if (cols[i] >= 0 && (long)cols[i] + (long)H * dh > ldx) return fail(EZDIT_E_INVALID, "columns [%d, %d + H dh) do not fit ldx = %d", cols[i], cols[i], ldx);
    // q / k rows are read with 8-byte loads, v rows with 16-byte loads
    if (ldx % 2 || (q_col >= 0 && q_col % 2) || (k_col >= 0 && k_col % 2)) return fail(EZDIT_E_INVALID, "ldx = %d or a q / k column offset breaks the 8-byte loads", ldx);
    if (v_col >= 0 && (ldx % 4 || v_col % 4)) return fail(EZDIT_E_INVALID, "ldx = %d or v_col = %d breaks the 16-byte loads", ldx, v_col);
    if (!x) return fail(EZDIT_E_INVALID, "null x");
    if (q_col >= 0 && (!q || !qn_w || !qn_b)) return fail(EZDIT_E_INVALID, "q is present: q, qn_w and qn_b are needed");
    if (k_col >= 0 && (!k || !kn_w || !kn_b)) return fail(EZDIT_E_INVALID, "k is present: k, kn_w and kn_b are needed");
    if (v_col >= 0 && !v) return fail(EZDIT_E_INVALID, "v is present: v is needed");
    if (!rope_cos != !rope_sin) return fail(EZDIT_E_INVALID, "rope_cos and rope_sin come together");
    auto misaligned = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
    if (misaligned(x, v_col >= 0 ? 16 : 8) || misaligned(q, 4) || misaligned(k, 4) || misaligned(v, 16))
        return fail(EZDIT_E_INVALID, "a pointer breaks the alignment of the vector accesses");
    HeadNormArgs hn;
    memset(&hn, 0, sizeof hn);
    hn.x = x; hn.ldx = ldx; hn.q_col = q_col; hn.k_col = k_col; hn.v_col = v_col;
    hn.qn_w = qn_w; hn.qn_b = qn_b; hn.kn_w = kn_w; hn.kn_b = kn_b; hn.rope_cos = rope_cos; hn.rope_sin = rope_sin;
    hn.q = (bf16_t*)q; hn.k = (bf16_t*)k; hn.v = (bf16_t*)v;
    hn.B = B; hn.H = H; hn.L = L; hn.Lp = Lp; hn.dh = dh;
    return hook_launch("k_headnorm", "", [&] { launch_headnorm(hn, (hipStream_t)stream); return 0; });
}

// the input assembly of a forward (launch_assemble: k_assemble)
int ezdit_test_assemble(const float* x, int x_rows, int in_ch, const float* gt, const uint8_t* gt_mask, const float* mask_embed, void* out, int ldo,
                        int B, int C, int L, const int32_t* dev_lens, ezdit_stream stream) {
    if (B <= 0 || C <= 0 || L <= 0) return fail(EZDIT_E_INVALID, "bad shape B=%d C=%d L=%d", B, C, L);
    if (in_ch != C && in_ch != 2 * C + 1) return fail(EZDIT_E_INVALID, "in_ch = %d is neither C = %d nor 2 C + 1", in_ch, C);
    if (x_rows <= 0 || B % x_rows) return fail(EZDIT_E_INVALID, "x_rows %d does not divide B %d", x_rows, B);
    if (!gt != !gt_mask) return fail(EZDIT_E_INVALID, "gt and gt_mask come together");
    if (ldo < 2 * C + 1) return fail(EZDIT_E_INVALID, "ldo = %d is below the 2 C + 1 = %d assembled channels", ldo, 2 * C + 1);
    if (!x || !out || (in_ch == C && !mask_embed)) return fail(EZDIT_E_INVALID, "null argument");
    if (dev_lens) {
        std::vector<int> ln((size_t)B);
        HIPCHK(hipStreamSynchronize((hipStream_t)stream));
        HIPCHK(hipMemcpy(ln.data(), dev_lens, (size_t)B * sizeof(int), hipMemcpyDeviceToHost));
        for (int i = 0; i < B; ++i)
            if (ln[i] < 1 || ln[i] > L) return fail(EZDIT_E_INVALID, "lens[%d] = %d outside [1, L = %d]", i, ln[i], L);
    }
    AssembleArgs as;
    as.x = x; as.x_rows = x_rows; as.in_ch = in_ch; as.gt = gt; as.gt_mask = gt_mask; as.mask_embed = mask_embed;
    as.out = (bf16_t*)out; as.ldo = ldo; as.B = B; as.C = C; as.L = L; as.lens = dev_lens;
    return hook_launch("k_assemble", "", [&] { launch_assemble(as, (hipStream_t)stream); return 0; });
}

int ezdit_debug_buffer(ezdit_handle* h, const char* name, void** ptr, size_t* bytes) {
    if (!h || !h->ws || !name) return fail(EZDIT_E_STATE, "bind workspace first");
    auto it = h->bufs.find(name);
    if (it == h->bufs.end()) return fail(EZDIT_E_INVALID, "no workspace buffer named %s", name);
    if (ptr) *ptr = h->ws + it->second.off;
    if (bytes) *bytes = it->second.bytes;
    return EZDIT_OK;
}

int ezdit_last_launch_count(const ezdit_handle* h) { return h ? h->launches : 0; }
int ezdit_debug_stop_after(ezdit_handle* h, int n) {
    if (!h) return fail(EZDIT_E_INVALID, "null handle");
    h->debug_stop = n;
    return EZDIT_OK;
}
// radius of the sliding-window self-attention (include/ezdit.h).  The radius is a kernel argument and chooses the kernel: a change drops the captured step
int ezdit_set_attention_window(ezdit_handle* h, int radius) {
    if (!h) return fail(EZDIT_E_INVALID, "null handle");
    if (radius < 0) return fail(EZDIT_E_INVALID, "radius = %d (0 = off, >= 1 = frames on either side)", radius);
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(h->last_stream, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
    if (cs != hipStreamCaptureStatusNone) return fail(EZDIT_E_STATE, "ezdit_set_attention_window inside a stream capture (it changes the kernels of the step)");
    if (radius != h->attn_window) drop_graph(h);
    h->attn_window = radius;
    return EZDIT_OK;
}

int ezdit_set_option(ezdit_handle* h, const char* name, int value) {
    if (!h || !name) return fail(EZDIT_E_INVALID, "null argument");
    if (!strcmp(name, "zfuse")) h->opt_zfuse = value;
    else if (!strcmp(name, "xkey1")) h->opt_xkey1 = value;
    else if (!strcmp(name, "skip_z")) h->opt_skip_z = value;
    else if (!strcmp(name, "geglu_co")) h->opt_geglu_co = value;
    else if (!strcmp(name, "qkv_co")) { h->opt_qkv_co = value & 3; h->opt_qkv_form = (value & 4) ? 0 : 1; }   // (+ 4: qkv_form = 0, the k-split form up to kCoM rows)
    else if (!strcmp(name, "wt")) h->opt_wt = value;
    else if (!strcmp(name, "gemm_pp")) h->opt_gemm_pp = value;
    else if (!strcmp(name, "tile_partial")) h->opt_tile_partial = value;
    else if (!strcmp(name, "attn_xcd")) h->opt_attn_xcd = value;
    else if (!strcmp(name, "row_variant")) h->opt_row_variant = value;
    else if (!strcmp(name, "gemm_panel")) h->opt_gemm_panel = value;
    else if (!strcmp(name, "row_affine")) h->opt_row_affine = value;
    else if (!strcmp(name, "epi_lds")) h->opt_epi_lds = value;
    else if (!strcmp(name, "attn_xk2")) h->opt_attn_xk2 = value;
    else if (!strcmp(name, "attn_nkh")) h->opt_attn_nkh = value;
    else if (!strcmp(name, "attn_qtile")) h->opt_attn_qtile = value;
    else if (!strcmp(name, "cn_overlap")) h->opt_cn_overlap = value;
    else if (!strcmp(name, "fuse_q2")) h->opt_fuse_q2 = value;
    else if (!strcmp(name, "q2_pp")) h->opt_q2_pp = value;
    else if (!strcmp(name, "stamp_launch")) h->opt_stamp_launch = value;
    else if (!strcmp(name, "trace_launches")) h->opt_trace_launches = value;
#ifdef EZ_DIAG
    else if (!strcmp(name, "zfake")) h->opt_zfake = value;
#endif
    else return fail(EZDIT_E_INVALID, "unknown option %s", name);
    drop_graph(h);
    return EZDIT_OK;
}

}  // extern "C"
