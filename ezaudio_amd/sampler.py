"""Sampler driver: the reference's ``inference()`` (/root/reference/src/inference.py:26-107) with the
whole per-step loop body -- CFG batch, denoiser, CFG combine, guidance rescale, DDIM update -- resident on
the GPU: one hipGraph replayed ``ddim_steps`` times, no host synchronisation inside the loop
(the reference syncs every step through the CPU-side scheduler).

Beyond the reference: ``P`` independent prompts per call (the reference hard-codes one noise row,
src/inference.py:67); each prompt's cond/uncond pair stays on one GPU.
"""
import ctypes as C
import math

import torch

from . import _lib
from .denoiser import _ptr


def scale_shift_re(x, scale, shift):
    """src/utils/utils.py:24-25."""
    return (x / scale) - shift


def _is_seq(v):
    """A per-prompt form of a setting (list, tuple, or a tensor with a dimension), not one value for the call."""
    return isinstance(v, (list, tuple)) or (torch.is_tensor(v) and v.dim() > 0)


def _per_prompt(value, n_prompts, name):
    """A per-request setting as one value per prompt (list), or None for the scalar form."""
    if _is_seq(value):
        vals = [v.item() if torch.is_tensor(v) else v for v in value]
        if len(vals) != n_prompts:
            raise ValueError(f'{len(vals)} values of {name} for {n_prompts} prompts')
        return vals
    return None


def _collapse(value, n_prompts, name):
    """(scalar, None) when `value` is a scalar or a list of equal values -- the scalar call, the same bits -- else (None, list of floats);
    None / 0 = the setting is off for that sample."""
    vals = _per_prompt(value, n_prompts, name)
    if vals is None:
        return value, None
    vals = [float(v or 0.0) for v in vals]
    if len(set(vals)) == 1:
        return vals[0], None
    return None, vals


APG_DEFAULTS = dict(eta=0.0, norm_threshold=0.0, momentum=-0.5)   # what apg=True means: no parallel part, momentum -0.5, NO norm cap (which cap suits the EzAudio latent is unmeasured)


def apg_entries(apg, n_prompts):
    """``apg`` of prepare() / inference() / generate_audio() as a list of n_prompts rows (eta_apg, norm_threshold, momentum, on), or None when nobody asks for
    it (the plain call).  ``apg`` is True or a dict with keys among eta, norm_threshold, momentum (APG_DEFAULTS fill the rest) -- for every prompt -- or a list
    with one such entry, or None / False, per prompt.  ValueError: a list of another size, an unknown key, a non-finite value, a negative norm_threshold."""
    if apg is None or apg is False:
        return None
    entries = list(apg) if isinstance(apg, (list, tuple)) else [apg] * n_prompts
    if len(entries) != n_prompts:
        raise ValueError(f'apg: True, a dict, or one entry (or None) per prompt; got {len(entries)} entries for {n_prompts} prompts')
    rows = []
    for i, e in enumerate(entries):
        if e is None or e is False:
            rows.append((0.0, 0.0, 0.0, 0))
            continue
        if e is True:
            e = {}
        if not isinstance(e, dict) or set(e) - set(APG_DEFAULTS):
            raise ValueError(f'apg of prompt {i}: expected True or a dict with keys among {sorted(APG_DEFAULTS)}, got {e!r}')
        v = {k: float(e.get(k, d)) for k, d in APG_DEFAULTS.items()}
        if not all(math.isfinite(x) for x in v.values()):
            raise ValueError(f'apg of prompt {i}: {e!r} is not finite')
        if v['norm_threshold'] < 0:
            raise ValueError(f'apg of prompt {i}: norm_threshold {v["norm_threshold"]} is negative (0 = no cap)')
        rows.append((v['eta'], v['norm_threshold'], v['momentum'], 1))
    return rows if any(r[3] for r in rows) else None


def check_apg(rows, guidance_scale, guidance_rescale, compose=False, canvas=False):
    """What APG does not combine with, on the host: ``rows`` of apg_entries(), the guidance settings as scalars or per-prompt lists."""
    if rows is None:
        return
    if compose:
        raise ValueError('apg does not combine with composed guidance (compose)')
    if canvas:
        raise ValueError('apg does not combine with a canvas or a loop: the momentum is not blended across windows')
    n = len(rows)
    per = lambda v, k: [float(x or 0.0) for x in (_per_prompt(v, n, k) or [v] * n)]   # noqa: E731
    gs, gr = per(guidance_scale, 'guidance_scale'), per(guidance_rescale, 'guidance_rescale')
    for i, r in enumerate(rows):
        if r[3] and not gs[i] > 0:
            raise ValueError(f'apg of prompt {i} without guidance: projected guidance needs a guidance_scale above 0')
        if r[3] and gr[i] > 0:
            raise ValueError(f'apg of prompt {i} with guidance_rescale {gr[i]}: the rescale is not applied to projected guidance, ask for one of the two')


TIMELINE_SEG = 128     # context rows of one prompt of a timeline: one key tile of the cross-attention kernel (csrc/attn.hip TL)
TIMELINE_MAX = 16      # prompts of one timeline
COMPOSE_MAX = 8        # conditions per sample of composed guidance (include/ezdit.h EZDIT_COMPOSE_MAX)


def scene_weights(scene, frames, latent_sr, crossfade):
    """The prompt timeline of a scene: ``scene`` is a list of (text, start_s, end_s[, weight]) entries, which may overlap; the clip has ``frames`` latent frames at
    ``latent_sr`` frames per second.  Each entry gets a trapezoid envelope of height ``weight`` (default 1) whose edges rise and fall linearly over ``crossfade``
    seconds, centred on start_s and end_s -- so two entries that meet cross-fade with a constant sum -- except an edge that sits on the clip's own edge, which is
    not ramped.  Envelopes are sampled at the frame centres (i + 0.5) / latent_sr; a frame's weights are the envelopes divided by their sum.
    Returns (prompts, W): the S texts and a float32 tensor [S, frames] whose columns sum to 1.  ValueError: a frame that no entry covers, an entry outside the
    clip (or empty, or of weight <= 0), more than TIMELINE_MAX entries.  Whether a cross-fade of the softmax prior sounds like one is unmeasured."""
    frames, sr, cf = int(frames), float(latent_sr), float(crossfade)
    if frames < 1 or sr <= 0 or cf < 0:
        raise ValueError(f'frames={frames}, latent_sr={latent_sr}, crossfade={crossfade}: a clip has frames, a rate above 0 and a crossfade of at least 0')
    if not scene or len(scene) > TIMELINE_MAX:
        raise ValueError(f'a scene has between 1 and {TIMELINE_MAX} entries, got {len(scene) if scene else 0}')
    dur = frames / sr
    eps = 0.5 / sr      # an edge within half a frame of the clip's edge sits on it
    t = (torch.arange(frames, dtype=torch.float64) + 0.5) / sr
    prompts, env = [], []
    for n, e in enumerate(scene):
        if len(e) not in (3, 4):
            raise ValueError(f'scene entry {n}: (text, start_s, end_s[, weight]), got {e!r}')
        text, a, b, wt = e[0], float(e[1]), float(e[2]), float(e[3]) if len(e) == 4 else 1.0
        if a < -eps or b > dur + eps or b <= a:
            raise ValueError(f'scene entry {n} [{a:g} s, {b:g} s) lies outside the clip of {dur:g} s or is empty')
        if not wt > 0 or wt == float('inf'):
            raise ValueError(f'scene entry {n}: weight {wt!r} must be positive and finite')
        if cf > 0:
            rise = torch.ones_like(t) if a <= eps else ((t - a) / cf + 0.5).clamp(0, 1)
            fall = torch.ones_like(t) if b >= dur - eps else ((b - t) / cf + 0.5).clamp(0, 1)
        else:
            rise, fall = (t >= a - 1e-9).double(), (t < b - 1e-9).double() if b < dur - eps else torch.ones_like(t)
        prompts.append(text)
        env.append(wt * torch.minimum(rise, fall))
    env = torch.stack(env)
    tot = env.sum(0)
    if bool((tot <= 0).any()):
        i = int((tot <= 0).nonzero()[0])
        raise ValueError(f'no scene entry covers frame {i} ({(i + 0.5) / sr:g} s)')
    return prompts, (env / tot).float()


def timeline_context(text, text_mask):
    """The 128-aligned context of a timeline: text [.., S, Lt, Cctx] and its mask [.., S, Lt] (Lt <= TIMELINE_SEG tokens per prompt) -> ([.., 128 S, Cctx],
    [.., 128 S]): prompt s occupies the rows [128 s, 128 s + Lt), the rows behind are zeros with mask 0."""
    S, Lt = text.shape[-3], text.shape[-2]
    if Lt > TIMELINE_SEG:
        raise ValueError(f'{Lt} tokens per prompt: a timeline holds at most {TIMELINE_SEG}')
    if S > TIMELINE_MAX or tuple(text_mask.shape) != tuple(text.shape[:-1]):
        raise ValueError(f'text {tuple(text.shape)} / mask {tuple(text_mask.shape)}: at most {TIMELINE_MAX} prompts, one mask entry per token')
    lead = tuple(text.shape[:-3])
    ctx = torch.zeros(lead + (S, TIMELINE_SEG, text.shape[-1]), dtype=text.dtype, device=text.device)
    msk = torch.zeros(lead + (S, TIMELINE_SEG), dtype=torch.bool, device=text.device)
    ctx[..., :Lt, :] = text
    msk[..., :Lt] = text_mask.bool()
    return ctx.reshape(lead + (S * TIMELINE_SEG, text.shape[-1])), msk.reshape(lead + (S * TIMELINE_SEG,))


SOLVERS = ('ddim', 'dpmpp_2m')


def check_solver(solver, eta):
    """'ddim' (the default: the reference's scheduler) or 'dpmpp_2m' (DPM-Solver++(2M), deterministic: eta must be 0, every entry of a list)."""
    if solver not in SOLVERS:
        raise ValueError(f'solver={solver!r}: expected one of {SOLVERS}')
    if solver == 'dpmpp_2m':
        etas = eta if _is_seq(eta) else [eta]
        if any(float(e or 0.0) != 0.0 for e in etas):
            raise ValueError(f"solver='dpmpp_2m' is deterministic and takes no step noise: pass eta=0 (got eta={eta!r})")


class LatentSampler:
    """prepare() once per call, then run(n) advances n steps (DDIM, or DPM-Solver++(2M) with solver='dpmpp_2m') on the device."""

    def __init__(self, unet, scheduler):
        self.unet = unet
        self.scheduler = scheduler
        self.stream = torch.cuda.Stream(device=unet.device)
        self.latents = None

    def prepare(self, text, text_mask, uncond_text, uncond_mask, init_noise, step_noises, guidance_scale,
                guidance_rescale, ddim_steps, eta, gt=None, gt_mask=None, controlnet=None, condition=None,
                conditioning_scale=1.0, lengths=None, init_latents=None, start_steps=None, latent_scale=1.0, latent_shift=0.0, context_weights=None, compose_text=None, compose_mask=None,
                compose_weights=None, token_weights=None, uncond_token_weights=None, compose_token_weights=None, apg=None, canvas=None, canvas_loop=None, solver='ddim'):
        """``lengths`` (list of P ints): init_noise / step_noises / gt / gt_mask are padded to L = max(lengths) frames and sample p is valid on
        [0, lengths[p]) -- its final latent is what a call with that sample alone at its own length gives, zero beyond (include/ezdit.h
        ezdit_set_lengths).  With a ControlNet the table goes to the attached pair (ezdit_sampler_set_pair_lengths) and ``condition`` is
        [P, cond_in, 2 * max(lengths)], padded: sample p's control signal is its first 2 * lengths[p] frames, whatever lies behind is ignored.

        ``condition`` may be one shared [1, cond_in, 2 L] row (broadcast over the prompts, as gt is).  ``conditioning_scale`` may be a list of P
        values: equal values are the scalar call (the same bits, no table), otherwise every sample's residuals take its own scale
        (ezdit_sampler_set_cn_scales; set_cn_scales() replaces the values of a prepared call).

        ``guidance_scale``, ``guidance_rescale`` and ``eta`` may each be a list of P values (None / 0 = no guidance for that sample; scalars
        broadcast): every sample then comes out as the call with that sample alone and its own settings gives it (include/ezdit.h
        ezdit_sampler_set_sample_params).  Lists of equal values are the scalar call: the same bits, no table.

        ``solver='dpmpp_2m'``: the second-order multistep update (scheduler.multistep_coefficients, include/ezdit.h ezdit_sampler_set_multistep)
        in place of DDIM's; eta must be 0.  The history of data predictions is allocated here and lives on the sampler, so run() may be
        called in pieces.  'ddim' calls nothing new.

        ``init_latents`` with ``start_steps`` (audio-to-audio): init_latents is fp32 [P or 1, C, L] in VAE space (what the encoder returns; one row is
        broadcast like gt), start_steps an int or a list of P steps in [0, ddim_steps).  Sample p then starts at step start_steps[p] from
        sa (init_latents + latent_shift) latent_scale + sb init_noise with (sa, sb) of that step (ezdit_add_noise) and is held until the run reaches it
        (ezdit_sampler_set_start); run() without n runs the ddim_steps - min(start_steps) steps that are left.  Every sample comes out as the call with
        it alone, started there, gives it.  All starts 0 calls nothing new: the same bits as without the two arguments.

        ``canvas=(offsets, T, ramp)`` (long-form generation): the P samples are windows of one canvas of T latent frames, window p holding the frames
        [offsets[p], offsets[p] + L) (canvas_windows() chooses such offsets; draw_noises(canvas_offsets=) slices one canvas noise for them).  Every step then
        ends by averaging the frames that windows share, with the weights min(r + 1, L - r, ramp) of the local frame r (ezdit_sampler_set_canvas), and
        canvas_latents() reads the [1, C, T] canvas off the windows after finish().  Not with lengths, gt / gt_mask, a ControlNet or init_latents.  A canvas of
        one window, or one whose windows do not overlap, calls nothing new: the same bits as without the argument.

        ``canvas_loop=(offsets, T, ramp)`` (seamless loops; not together with ``canvas``): the canvas is a RING of T >= L frames, window p holding the frames
        (offsets[p] + r) mod T for r in [0, L), so the last window runs into the first (loop_windows() chooses such offsets; draw_noises(canvas_loop=) cuts
        one ring noise for them).  The step ends with the wrap blend (ezdit_sampler_set_canvas_loop: the same table as ``canvas``, the same refusals), and
        canvas_latents() reads the [1, C, T] ring, whose last frame continues into its first.

        ``context_weights`` [P, S, L] (prompt timeline, include/ezdit.h ezdit_set_context_weights): ``text`` is then [P, S, Lt, Cctx] and ``text_mask`` [P, S, Lt],
        S prompts per sample, and frame i of sample p weights prompt s by context_weights[p, s, i] in every block's cross-attention (scene_weights() makes such
        weights).  The 128-aligned context is built here; the unconditional rows keep their tokens in prompt 0 and weight it alone.  Not with a canvas, a loop or a
        ControlNet.

        ``compose_weights`` [P, K] with ``compose_text`` [P, K-1, Lt, Cctx] and ``compose_mask`` [P, K-1, Lt] (composed guidance, include/ezdit.h
        ezdit_sampler_begin_composed): sample p carries K conditions -- ``text`` is condition 0, the primary one -- and is guided by
        v = u + guidance_scale sum_k w[p, k] (c_k - u) against its one unconditional row; the guidance rescale takes the primary condition as its reference.
        w[p, 0] > 0; the others are any finite value, negative ones steer away from their prompt, and a weight of exactly 0 drops its condition (its row is
        computed and not read).  The batch is built here as [text | compose_text[:, 0] | ... | uncond_text]; set_compose_weights() replaces the values of a
        prepared call without a re-capture.  It combines with lengths, per-sample settings, ``solver``, gt / gt_mask, init_latents and an attention window; not with
        a ControlNet, a canvas, a loop or a timeline, and it needs guidance.  One condition with weight 1 is the plain call: nothing new is called, the same bits.

        ``token_weights`` [P, Lt] (prompt emphasis, include/ezdit.h ezdit_set_context_token_weights): token j of sample p's prompt weighs token_weights[p, j] > 0 in every
        block's cross-attention, as if it stood there that many times (parse_emphasis() / emphasis_weights() make such weights from '(words:1.6)' markup).
        ``uncond_token_weights`` [P, Lt] does the same for the unconditional rows (default: 1) and ``compose_token_weights`` [P, K-1, Lt] for the extra conditions of
        ``compose_text``.  The [B, Lc] table is built here in the layout of the batch; values at masked tokens are not read.  It combines with composed guidance, a canvas
        or loop, lengths, init_latents and ``solver``; not with a ControlNet or a timeline.  Weights that are equal within every row call nothing new: the same bits.

        ``apg`` (adaptive projected guidance, include/ezdit.h ezdit_sampler_set_apg): True, a dict(eta=, norm_threshold=, momentum=) or a list with one such
        entry (or None) per sample (apg_entries()).  A sample with an entry is guided on its data prediction -- the guidance direction keeps a momentum across
        steps, is capped at norm_threshold (0: no cap) and loses its part parallel to the conditional prediction (eta: the share that stays) -- in place of
        v = u + w (c - u); the others are guided as always.  The momentum buffer is allocated here and lives on the sampler, next to the multistep history;
        set_apg() replaces the values of a prepared call without a re-capture.  It combines with lengths, per-sample settings, ``solver``, step noise,
        init_latents, gt / gt_mask, a ControlNet, a timeline and token weights; not with composed guidance, a canvas or a loop, and a sample that asks for it
        needs guidance and no guidance_rescale.  Nobody asking calls nothing new: the same bits."""
        check_solver(solver, eta)
        apg = apg_entries(apg, init_noise.shape[0])
        if token_weights is not None or uncond_token_weights is not None or compose_token_weights is not None:
            if controlnet is not None or context_weights is not None:
                raise ValueError('token weights do not combine with a ControlNet or a prompt timeline')
            if text.dim() != 3:
                raise ValueError(f'token weights with text {tuple(text.shape)}: expected [P, Lt, Cctx]')
        compose = None
        if compose_weights is not None or compose_text is not None or compose_mask is not None:
            if compose_weights is None:
                raise ValueError('compose_text / compose_mask without compose_weights')
            cw = torch.as_tensor(compose_weights, dtype=torch.float32).cpu()
            n_cond = cw.shape[1] if cw.dim() == 2 else 0
            if cw.dim() != 2 or cw.shape[0] != init_noise.shape[0] or not 1 <= n_cond <= COMPOSE_MAX:
                raise ValueError(f'compose_weights {tuple(cw.shape)}: expected [P={init_noise.shape[0]}, K] with 1 <= K <= {COMPOSE_MAX}')
            if not bool(torch.isfinite(cw).all()) or not bool((cw[:, 0] > 0).all()):
                raise ValueError('compose_weights must be finite, and the primary condition (column 0) weighted above 0')
            if n_cond > 1:
                if (compose_text is None or compose_mask is None or text.dim() != 3 or compose_text.dim() != 4
                        or tuple(compose_text.shape) != (text.shape[0], n_cond - 1) + tuple(text.shape[1:])
                        or tuple(compose_mask.shape) != tuple(compose_text.shape[:3])):
                    raise ValueError(f'compose_text / compose_mask with text {tuple(text.shape)} and K = {n_cond}: expected [P, K-1, Lt, Cctx] and [P, K-1, Lt]')
            elif compose_text is not None and compose_text.shape[1] != 0:
                raise ValueError('compose_weights [P, 1] takes no compose_text')
            if not (n_cond == 1 and bool((cw == 1).all())):   # (one condition with weight 1: the plain call)
                if controlnet is not None or canvas is not None or canvas_loop is not None or context_weights is not None:
                    raise ValueError('composed guidance does not combine with a ControlNet, a canvas, a loop or a prompt timeline')
                compose = cw.contiguous()
        check_apg(apg, guidance_scale, guidance_rescale, compose=compose is not None, canvas=canvas is not None or canvas_loop is not None)
        if context_weights is not None:
            if canvas is not None or canvas_loop is not None or controlnet is not None:
                raise ValueError('a prompt timeline does not combine with a canvas, a loop or a ControlNet')
            context_weights = torch.as_tensor(context_weights, dtype=torch.float32).cpu()
            if text.dim() != 4 or context_weights.dim() != 3 or tuple(context_weights.shape) != (text.shape[0], text.shape[1], init_noise.shape[2]):
                raise ValueError(f'context_weights {tuple(context_weights.shape)} with text {tuple(text.shape)}: expected [P, S, L] and [P, S, Lt, Cctx]')
            n_seg = text.shape[1]
            text, text_mask = timeline_context(text, text_mask)
            # the unconditional rows: their tokens in prompt 0, nothing behind (the encoding of '' keeps its single valid key, and with it the single-key shortcut)
            pad = (n_seg - 1) * TIMELINE_SEG
            uncond_text, uncond_mask = timeline_context(uncond_text[:, None], uncond_mask[:, None])
            uncond_text = torch.nn.functional.pad(uncond_text, (0, 0, 0, pad))
            uncond_mask = torch.nn.functional.pad(uncond_mask, (0, pad))
        if (init_latents is None) != (start_steps is None):
            raise ValueError('init_latents and start_steps must be given together')
        u = self.unet
        dev = u.device
        P, Cc, L = init_noise.shape
        if isinstance(ddim_steps, (list, tuple)):
            raise ValueError('ddim_steps must be one value per call: per-prompt step counts are not supported')
        (guidance_scale, gs_l), (guidance_rescale, gr_l), (eta, eta_l) = (_collapse(v, P, k) for v, k in (
            (guidance_scale, 'guidance_scale'), (guidance_rescale, 'guidance_rescale'), (eta, 'eta')))
        table = None
        if gs_l is not None or gr_l is not None or eta_l is not None:
            table = tuple(l if l is not None else [float(v or 0.0)] * P for l, v in ((gs_l, guidance_scale), (gr_l, guidance_rescale), (eta_l, eta)))
            # what ezdit_sampler_begin sees: CFG rows when any sample has guidance; the table set right after it holds every sample's values
            guidance_scale, guidance_rescale, eta = max(table[0]), table[1][0], max(table[2])
        if lengths is not None:
            lengths = [int(v) for v in lengths]
            if len(lengths) != P:
                raise ValueError(f'{len(lengths)} lengths for P={P} samples')
        cn_scales = None
        if controlnet is not None:
            conditioning_scale, cn_scales = _collapse(conditioning_scale, P, 'conditioning_scale')
            if cn_scales is not None:
                conditioning_scale = max(cn_scales)   # what ezdit_sampler_attach_controlnet sees; the table set behind it holds every sample's value
            if condition is None or condition.dim() != 3 or condition.shape[0] not in (1, P) or condition.shape[2] != 2 * L:
                raise ValueError(f'condition must be [1 or P={P}, cond_in, 2 L = {2 * L}], got {None if condition is None else tuple(condition.shape)}')
        starts = None
        if start_steps is not None:
            starts = [int(v) for v in start_steps] if isinstance(start_steps, (list, tuple)) else [int(start_steps)] * P
            if len(starts) != P:
                raise ValueError(f'{len(starts)} start steps for P={P} samples')
            if min(starts) < 0 or max(starts) >= ddim_steps:
                raise ValueError(f'start_steps {starts} outside [0, ddim_steps = {ddim_steps})')
            if init_latents.dim() != 3 or init_latents.shape[0] not in (1, P) or tuple(init_latents.shape[1:]) != (Cc, L):
                raise ValueError(f'init_latents must be [1 or P={P}, {Cc}, {L}], got {tuple(init_latents.shape)}')
            if max(starts) == 0:
                starts = None   # every sample from pure noise: the plain call
        self.canvas = None
        if canvas is not None:
            offs, T, ramp = [int(v) for v in canvas[0]], int(canvas[1]), int(canvas[2])
            check_canvas(offs, L, T, ramp)
            if len(offs) != P:
                raise ValueError(f'{len(offs)} canvas offsets for P={P} windows')
            if lengths is not None or gt is not None or controlnet is not None or init_latents is not None:
                raise ValueError('a canvas does not combine with lengths, gt / gt_mask, a ControlNet or init_latents')
            self.canvas = (offs, T, ramp)
        self.loop = False
        if canvas_loop is not None:
            if canvas is not None:
                raise ValueError('canvas and canvas_loop are two forms of one table: give one')
            offs, T, ramp = [int(v) for v in canvas_loop[0]], int(canvas_loop[1]), int(canvas_loop[2])
            check_canvas_loop(offs, L, T, ramp)
            if len(offs) != P:
                raise ValueError(f'{len(offs)} loop offsets for P={P} windows')
            if lengths is not None or gt is not None or controlnet is not None or init_latents is not None:
                raise ValueError('a loop does not combine with lengths, gt / gt_mask, a ControlNet or init_latents')
            self.canvas, self.loop = (offs, T, ramp), True
        self.scheduler.set_timesteps(ddim_steps)
        ts = [int(t) for t in self.scheduler.timesteps]
        coefs = self.scheduler.ddim_coefficients(eta)
        use_cfg = bool(guidance_scale)
        if compose is not None:   # [c_0 (P rows) | c_1 | ... | c_{K-1} | u]: row k P + p is condition k of sample p
            if not use_cfg or float(guidance_scale) <= 0:
                raise ValueError('composed guidance needs a guidance_scale above 0')
            extra = [compose_text[:, k] for k in range(compose.shape[1] - 1)]
            ctx = torch.cat([text] + extra + [uncond_text], dim=0)
            msk = torch.cat([text_mask] + [compose_mask[:, k].to(text_mask.dtype) for k in range(compose.shape[1] - 1)] + [uncond_mask], dim=0)
        elif use_cfg:
            ctx = torch.cat([text, uncond_text], dim=0)          # src/inference.py:76-77
            msk = torch.cat([text_mask, uncond_mask], dim=0)
        else:
            ctx, msk = text, text_mask
        B = ctx.shape[0]
        tok_w = None
        if token_weights is not None or uncond_token_weights is not None or compose_token_weights is not None:
            # one row of weights per batch row, in the order the context was built in above; a part that was not given weighs 1
            def _part(wt, shape, name):
                if wt is None:
                    return torch.ones(shape, dtype=torch.float32)
                wt = torch.as_tensor(wt, dtype=torch.float32).cpu()
                if tuple(wt.shape) != tuple(shape):
                    raise ValueError(f'{name} {tuple(wt.shape)}: expected {tuple(shape)}')
                return wt
            Pt, Lt = text.shape[0], text.shape[1]
            parts = [_part(token_weights, (Pt, Lt), 'token_weights')]
            if compose is not None:
                cwt = _part(compose_token_weights, (Pt, compose.shape[1] - 1, Lt), 'compose_token_weights')
                parts += [cwt[:, k] for k in range(compose.shape[1] - 1)]
            elif compose_token_weights is not None:
                raise ValueError('compose_token_weights without composed guidance')
            if compose is not None or use_cfg:
                parts.append(_part(uncond_token_weights, (uncond_text.shape[0], Lt), 'uncond_token_weights'))
            elif uncond_token_weights is not None:
                raise ValueError('uncond_token_weights without guidance: there is no unconditional row')
            tok_w = torch.cat(parts, dim=0).contiguous()
        self.latents = init_noise.to(dev, torch.float32).contiguous().clone()
        self.noise = None if (eta <= 0 or step_noises is None) else step_noises.to(dev, torch.float32).contiguous()
        if eta > 0 and self.noise is None:
            raise ValueError('eta > 0 needs step_noises [n_steps, P, C, L]')
        if (gt is None) != (gt_mask is None):
            raise ValueError('gt and gt_mask must be given together')
        # the kernels index gt / gt_mask per latent row ([P, C, L]): a shared [1, C, L] reference (one clip edited under P prompts,
        # which is also what the sharded driver forwards un-sliced) is broadcast here
        for name, t in (('gt', gt), ('gt_mask', gt_mask)):
            if t is not None and t.shape[0] not in (1, P):
                raise ValueError(f'{name} has {t.shape[0]} rows; expected 1 or P={P}')
        self.gt = None if gt is None else gt.to(dev, torch.float32).expand(P, Cc, L).contiguous()
        self.gt_mask = None if gt_mask is None else gt_mask.to(dev).expand(P, Cc, L).to(torch.uint8).contiguous()
        cur = torch.cuda.current_stream(dev)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            if getattr(u, '_canvas_on', False):   # the handle outlives the call: an earlier call's canvas goes before this call's tables are set
                # (-3, EZDIT_E_STATE: the workspace was bound again since, which cleared the table and ended the call it belonged to)
                self._table_call(u.lib.ezdit_sampler_set_canvas, None, 0, 0, 1, ok=(-3,))
                u._canvas_on = False
            if getattr(u, '_compose_on', False):   # ... and so does an earlier call's composition, which the attach and the context weights below refuse to meet
                self._table_call(u.lib.ezdit_sampler_set_compose_weights, None, 0, 0, ok=(-3,))
                u._compose_on = False
            u.bind(B, L, ctx.shape[1], ddim_steps)
            u.prepare_context(ctx, msk)
            u.prepare_timesteps(ts, per_row=False)
            st = C.c_void_p(self.stream.cuda_stream)
            if controlnet is not None:
                controlnet.bind(B, L, ctx.shape[1], ddim_steps)
                controlnet.prepare_context(ctx, msk)
                controlnet.prepare_timesteps(ts, per_row=False)
            _lib.check(u.lib.ezdit_sampler_attach_controlnet(u._h, controlnet._h if controlnet is not None else None,
                                                             float(conditioning_scale)))
            self.controlnet = controlnet
            # (always: the bindings are cached, None clears an earlier call's)
            if controlnet is None:
                u.set_lengths(lengths, st)
            else:  # the pair's table first, then the condition embed that is computed from it
                arr = None if lengths is None else (C.c_int32 * P)(*lengths)
                self._table_call(u.lib.ezdit_sampler_set_pair_lengths, arr, 0 if lengths is None else P)
                cond = condition.to(dev, torch.float32).expand(P, -1, -1)
                cond = torch.cat([cond, cond], dim=0) if use_cfg else cond   # src/inference_controlnet.py:78-99: duplicated for the CFG pair
                controlnet.prepare_condition(cond)
            if context_weights is not None:   # behind the context and the lengths, which the table is checked against (prepare_context switched an earlier call's off)
                wt = context_weights
                if use_cfg:
                    one = torch.zeros_like(wt)
                    one[:, 0] = 1.0
                    wt = torch.cat([wt, one], dim=0)
                u.set_context_weights(wt, st)
            if tok_w is not None:   # behind the context, whose mask the table is checked against (prepare_context switched an earlier call's off)
                u.set_context_token_weights(tok_w, st)
            arr = (_lib.EzditDdimCoef * ddim_steps)(*[_lib.EzditDdimCoef(*c) for c in coefs])
            if compose is not None:
                n_cond = compose.shape[1]
                _lib.check(u.lib.ezdit_sampler_begin_composed(u._h, _ptr(self.latents), P, _ptr(self.noise), arr, ddim_steps,
                                                              float(guidance_scale), float(guidance_rescale or 0.0), _ptr(self.gt), _ptr(self.gt_mask),
                                                              n_cond, (C.c_float * (P * n_cond))(*compose.flatten().tolist()),
                                                              C.c_void_p(self.stream.cuda_stream)))
            else:
                _lib.check(u.lib.ezdit_sampler_begin(u._h, _ptr(self.latents), P, _ptr(self.noise), arr, ddim_steps,
                                                     float(guidance_scale or 0.0), float(guidance_rescale or 0.0),
                                                     _ptr(self.gt), _ptr(self.gt_mask),
                                                     C.c_void_p(self.stream.cuda_stream)))
        self.compose_K = None if compose is None else compose.shape[1]
        u._compose_on = compose is not None
        self.n_steps = ddim_steps
        self.P = P
        self.x0_hist = None
        self.apg_m = None
        self.first_step = 0
        if starts is not None:
            with torch.cuda.stream(self.stream):
                st = C.c_void_p(self.stream.cuda_stream)
                # (sa, sb) do not depend on eta: the call's rows serve every sample
                self._start_params = torch.tensor([[coefs[k][0], coefs[k][1]] for k in starts], dtype=torch.float32).to(dev)
                self._start_clean = init_latents.to(dev, torch.float32).expand(P, Cc, L).contiguous()
                self._start_lens = None if lengths is None else torch.tensor(lengths, dtype=torch.int32).to(dev)
                _lib.check(u.lib.ezdit_add_noise(_ptr(self._start_clean), _ptr(self.latents), _ptr(self._start_params), float(latent_scale),
                                                 float(latent_shift), _ptr(self._start_lens), L, P, Cc * L, st))
            self._table_call(u.lib.ezdit_sampler_set_start, (C.c_int32 * P)(*starts), P)
            self.first_step = min(starts)
        if self.loop:
            if P > 1:   # (one window that is the whole ring shares no frame with anybody)
                self.set_canvas_loop(*self.canvas)
        elif self.canvas is not None and any(b < a + L for a, b in zip(self.canvas[0], self.canvas[0][1:])):   # windows that share frames
            self.set_canvas(*self.canvas)
        if table is not None:
            self.set_sample_params(*table)
        if cn_scales is not None:
            self.set_cn_scales(cn_scales)
        if solver == 'dpmpp_2m':   # after the sample table: the library checks the two against each other
            self.x0_hist = torch.zeros_like(self.latents)
            ch = self.scheduler.multistep_coefficients()
            self._table_call(u.lib.ezdit_sampler_set_multistep, (C.c_float * ddim_steps)(*ch), ddim_steps, _ptr(self.x0_hist))
        if apg is not None:   # after the sample table (a sample's guidance comes from it) and the multistep setter
            self._set_apg_rows(apg)

    def set_apg(self, apg=None):
        """Adaptive projected guidance of the call prepare() began: what prepare(apg=) takes -- True, a dict, or one entry (or None) per sample -- or no
        argument to switch it off (classifier-free guidance again, the plain call's bits).  The captured step reads the table at run time: new values need no
        re-capture.  The momentum buffer is the sampler's and is kept across calls of this method; a run that is rewound starts without momentum anyway."""
        self._set_apg_rows(apg_entries(apg, self.P))

    def _set_apg_rows(self, rows):
        setter = self.unet.lib.ezdit_sampler_set_apg
        if rows is None:
            self._table_call(setter, None, None, None, None, 0, None)
            return
        if self.apg_m is None:
            self.apg_m = torch.zeros_like(self.latents)
        P = self.P
        cols = [(C.c_float * P)(*[r[k] for r in rows]) for k in range(3)]
        self._table_call(setter, *cols, (C.c_int32 * P)(*[r[3] for r in rows]), P, _ptr(self.apg_m))

    def _table_call(self, setter, *args, ok=()):
        """One call of a table setter of the library (include/ezdit.h, "Run-time tables of the step") for this sampler's handle, on the sampler stream.  Its
        code is checked; one listed in `ok` is handed back instead."""
        with torch.cuda.stream(self.stream):
            rc = setter(self.unet._h, *args, C.c_void_p(self.stream.cuda_stream))
        if rc not in ok:
            _lib.check(rc)
        return rc

    def set_sample_params(self, guidance_scale=None, guidance_rescale=None, eta=None):
        """Per-sample settings of the call prepare() began: three lists of P values (eta enters as each sample's own DDIM coefficient rows),
        or no argument to go back to the call's scalars.  The captured step reads the table at run time: new values need no re-capture."""
        setter = self.unet.lib.ezdit_sampler_set_sample_params
        if guidance_scale is None and guidance_rescale is None and eta is None:
            self._table_call(setter, None, None, None, 0)
            return
        P, n = self.P, self.n_steps
        vals = [[float(v or 0.0) for v in l] for l in (guidance_scale, guidance_rescale, eta)]
        if any(len(l) != P for l in vals):
            raise ValueError(f'per-sample settings need {P} values each')
        rows = sample_coefficients(self.scheduler, vals[2])
        gs, gr = (C.c_float * P)(*vals[0]), (C.c_float * P)(*vals[1])
        arr = (_lib.EzditDdimCoef * (n * P))(*[_lib.EzditDdimCoef(*rows[p][i]) for i in range(n) for p in range(P)])
        self._table_call(setter, gs, gr, arr, P)

    def set_canvas(self, offsets=None, T=0, ramp=1):
        """The canvas table of the call prepare() began: P window offsets, the canvas length and the ramp, or no argument to switch the blend off (independent
        windows).  The captured step reads the offsets at run time: new offsets of the same T and ramp need no re-capture."""
        u = self.unet
        if offsets is None:
            self._table_call(u.lib.ezdit_sampler_set_canvas, None, 0, 0, 1)
            u._canvas_on = False
            return
        offs = [int(v) for v in offsets]
        self._table_call(u.lib.ezdit_sampler_set_canvas, (C.c_int32 * len(offs))(*offs), len(offs), int(T), int(ramp))
        u._canvas_on = True
        self.canvas, self.loop = (offs, int(T), int(ramp)), False

    def set_canvas_loop(self, offsets=None, T=0, ramp=1):
        """set_canvas for the ring (ezdit_sampler_set_canvas_loop): the two replace each other, no argument on either switches the blend off."""
        u = self.unet
        if offsets is None:
            self._table_call(u.lib.ezdit_sampler_set_canvas_loop, None, 0, 0, 1)
            u._canvas_on = False
            return
        offs = [int(v) for v in offsets]
        self._table_call(u.lib.ezdit_sampler_set_canvas_loop, (C.c_int32 * len(offs))(*offs), len(offs), int(T), int(ramp))
        u._canvas_on = True
        self.canvas, self.loop = (offs, int(T), int(ramp)), True

    def canvas_latents(self):
        """The [1, C, T] canvas of a call prepared with ``canvas=`` or ``canvas_loop=``, assembled from the windows after finish().  With the blend on the
        windows agree bit for bit on the frames they share; the lowest window is the one copied.  A ring is cut at the first window's first frame."""
        if self.canvas is None:
            raise ValueError('prepare(canvas=...) or prepare(canvas_loop=...) first')
        offs, T, _ = self.canvas
        P, Cc, L = self.latents.shape
        out = torch.empty((1, Cc, T), dtype=self.latents.dtype, device=self.latents.device)
        if self.loop:
            for p in reversed(range(P)):
                out[0, :, _ring(offs[p], L, T, out.device)] = self.latents[p]
            return out
        for p in reversed(range(P)):
            out[0, :, offs[p]:offs[p] + L] = self.latents[p]
        return out

    def set_compose_weights(self, weights):
        """The weights [P, K] of the composed call prepare() began (``compose_weights``): same P and K, w[p, 0] > 0, finite.  The captured step reads them at
        run time: new values need no re-capture.  Switching composition on or off, or another K, is another batch: prepare() again."""
        if getattr(self, 'compose_K', None) is None:
            raise ValueError('set_compose_weights: prepare(compose_weights=...) first')
        w = torch.as_tensor(weights, dtype=torch.float32).cpu()
        if tuple(w.shape) != (self.P, self.compose_K):
            raise ValueError(f'compose weights {tuple(w.shape)}: the call was prepared with [P={self.P}, K={self.compose_K}]')
        self._table_call(self.unet.lib.ezdit_sampler_set_compose_weights, (C.c_float * w.numel())(*w.flatten().tolist()), self.P, self.compose_K)

    def set_cn_scales(self, scales=None):
        """conditioning_scale per sample of the call prepare() began with a ControlNet: a list of P values, or None to go back to the call's scalar.
        The captured step reads the table at run time: new values need no re-capture."""
        setter = self.unet.lib.ezdit_sampler_set_cn_scales
        if scales is None:
            self._table_call(setter, None, 0)
            return
        vals = [float(v) for v in scales]
        if len(vals) != self.P:
            raise ValueError(f'{len(vals)} conditioning scales for P={self.P} samples')
        self._table_call(setter, (C.c_float * self.P)(*vals), self.P)

    def run(self, n=None, use_graph=True):
        n = self.n_steps - self.first_step if n is None else n
        with torch.cuda.stream(self.stream):
            _lib.check(self.unet.lib.ezdit_sampler_run(self.unet._h, n, 1 if use_graph else 0,
                                                       C.c_void_p(self.stream.cuda_stream)))
        return self.latents

    def finish(self, block=True):
        """Hand back the latents.  BLOCKS THE HOST by default (`stream.synchronize()` on the sampler stream), so the caller's stream needs no
        ordering afterwards and the returned tensor is final.

        The host wait is deliberate: queueing a cross-stream wait (`current_stream.wait_stream(self.stream)`) while the step graphs are
        still executing makes the graphs themselves run 5-6 % slower on MI355X / ROCm 7.2 (4.01 vs 4.24 ms per step over a 20-step
        loop, HIP events on the sampler stream, alternating in one process: profiles/r04_experiments.txt) -- a second hardware queue
        parked on a barrier packet next to the running one.

        block=False keeps the round-3 contract for callers that pipeline host work: no host synchronisation, the CURRENT stream is made to wait
        for the sampler stream (stream-ordered; costs the running graphs the 5-6 % above)."""
        if block:
            self.stream.synchronize()
        else:
            torch.cuda.current_stream(self.latents.device).wait_stream(self.stream)
        return self.latents


def check_canvas(offsets, L, T, ramp):
    """The rules of ezdit_sampler_set_canvas, on the host: first offset 0, strictly ascending, no uncovered frame, the last window ends the canvas."""
    if not offsets or offsets[0] != 0:
        raise ValueError(f'canvas offsets {offsets}: the first window starts at frame 0')
    for a, b in zip(offsets, offsets[1:]):
        if b <= a or b > a + L:
            raise ValueError(f'canvas offsets {offsets}: each window starts behind the one before and no later than its end (window length {L})')
    if offsets[-1] + L != T:
        raise ValueError(f'canvas of {T} frames: the last window ends at frame {offsets[-1] + L}')
    if ramp < 1:
        raise ValueError(f'canvas ramp {ramp}: at least 1')


def _ring(offset, L, T, device):
    """The ring frames (offset + r) mod T, r in [0, L), as an index tensor."""
    return (torch.arange(L, device=device) + int(offset)) % int(T)


def loop_overlaps(offsets, L, T):
    """Frames that each window's tail shares with the head of its cyclic successor, the last window's with the first window's: L minus the step to it."""
    return [a + L - b for a, b in zip(offsets, list(offsets[1:]) + [offsets[0] + T])]


def check_canvas_loop(offsets, L, T, ramp):
    """The rules of ezdit_sampler_set_canvas_loop, on the host: a window no longer than the ring, first offset 0, strictly ascending, no uncovered frame
    between neighbours or at the wrap, the last window starts inside the ring."""
    if L < 1 or L > T:
        raise ValueError(f'a ring of {T} frames in windows of {L}: a window holds a ring frame at most once')
    if not offsets or offsets[0] != 0:
        raise ValueError(f'loop offsets {offsets}: the first window starts at frame 0')
    for a, b in zip(offsets, offsets[1:]):
        if b <= a or b > a + L:
            raise ValueError(f'loop offsets {offsets}: each window starts behind the one before and no later than its end (window length {L})')
    if offsets[-1] >= T:
        raise ValueError(f'ring of {T} frames: the last window starts at frame {offsets[-1]}')
    if offsets[-1] + L < T:
        raise ValueError(f'ring of {T} frames: the last window ends at frame {offsets[-1] + L} and leaves a gap at the wrap')
    if ramp < 1:
        raise ValueError(f'loop ramp {ramp}: at least 1')


def loop_windows(total_frames, window_frames, min_overlap):
    """(offsets, L) for a ring of total_frames: windows of L = min(window_frames, total_frames) frames at the offsets i T // P, with the fewest P >= 2 for
    which every window shares at least min_overlap frames with its cyclic successor (loop_overlaps).  The largest step between such offsets is
    ceil(T / P), so P = max(2, ceil(T / (L - min_overlap))).  A ring no longer than one window is two windows of L = T half a turn apart: a single window
    would have nobody to agree with at its own seam."""
    T, O = int(total_frames), int(min_overlap)
    if T < 2 or int(window_frames) < 1:
        raise ValueError(f'total_frames={total_frames}, window_frames={window_frames}: a ring has at least 2 frames, a window at least 1')
    L = min(int(window_frames), T)
    if O < 0 or O >= L:
        raise ValueError(f'min_overlap={min_overlap} outside [0, window length {L})')
    P = max(2, -(-T // (L - O)))
    if P > T:
        raise ValueError(f'min_overlap={min_overlap}: no {T} or fewer windows of {L} frames on a ring of {T} share that much')
    return [i * T // P for i in range(P)], L


def canvas_windows(total_frames, window_frames, min_overlap):
    """(offsets, L): the fewest windows of L <= window_frames latent frames that cover total_frames with at least min_overlap frames shared between
    neighbours, spread evenly (integer arithmetic).  A canvas that fits one window is ([0], total_frames): the plain call."""
    T, L, O = int(total_frames), int(window_frames), int(min_overlap)
    if T < 1 or L < 1:
        raise ValueError(f'total_frames={total_frames}, window_frames={window_frames}: both must be positive')
    if O < 0 or 2 * O > L:
        raise ValueError(f'min_overlap={min_overlap} outside [0, window_frames / 2 = {L / 2:g}]')
    if T <= L:
        return [0], T
    n = -(-(T - O) // (L - O))
    return [(i * (T - L) + (n - 1) // 2) // (n - 1) for i in range(n)], L


def decode_circular(autoencoder, latents, context=None):
    """Decode a ring of latents [N, C, T] as a ring: the VAE's convolutions pad with zeros, so the ring is extended by `context` wrapped frames on either side
    (tiled when context > T), decoded in ONE call, and context * (out_len // in_len) samples are cut from each end.  Once `context` covers the decoder's
    receptive field (``autoencoder.decoder_context_frames()``, what None asks for) no kept sample has seen a zero halo and the result is what a decoder with
    circular convolutions gives: its last sample continues into its first.  An injected autoencoder without that method needs an explicit `context`."""
    if context is None:
        ask = getattr(autoencoder, 'decoder_context_frames', None)
        if ask is None:
            raise ValueError('decode_circular: this autoencoder does not tell its receptive field (decoder_context_frames): pass context=')
        context = ask()
    context = int(context)
    if context < 0:
        raise ValueError(f'context={context}: at least 0')
    T = latents.shape[-1]
    ext = latents[..., torch.arange(-context, T + context, device=latents.device) % T]
    wav = autoencoder(embedding=ext)
    cut = context * (wav.shape[-1] // ext.shape[-1])
    return wav[..., cut:wav.shape[-1] - cut]


def sample_coefficients(scheduler, etas):
    """rows[p][i] = (sa, sb, c_x0, c_dir, sigma) of sample p at step i of the scheduler's current timesteps: `ddim_coefficients(eta_p)` per
    sample, what a call with that sample alone uploads."""
    by_eta = {}
    for e in etas:
        if e not in by_eta:
            by_eta[e] = scheduler.ddim_coefficients(e)
    return [by_eta[e] for e in etas]


def _frames_list(audio_frames, n_prompts):
    """audio_frames as one length per prompt, or None for the scalar form."""
    if _is_seq(audio_frames):
        lens = [int(v) for v in audio_frames]
        if len(lens) != n_prompts:
            raise ValueError(f'{len(lens)} lengths for {n_prompts} prompts')
        if min(lens) < 1:
            raise ValueError(f'lengths must be positive: {lens}')
        return lens
    return None


def pad_conditions(condition, frames, n_prompts):
    """The control signal of a call as ONE tensor [n_prompts or 1, cond_in, 2 * max(frames)]: a list of per-prompt tensors [1, cond_in, 2 * frames[i]]
    (or [cond_in, 2 * frames[i]]) is zero-padded behind each prompt's own frames; a tensor is checked and passed on."""
    lmax = max(frames) if isinstance(frames, (list, tuple)) else int(frames)
    if isinstance(condition, (list, tuple)):
        if len(condition) != n_prompts:
            raise ValueError(f'{len(condition)} conditions for {n_prompts} prompts')
        rows = [c if c.dim() == 3 else c.unsqueeze(0) for c in condition]
        for i, c in enumerate(rows):
            want = 2 * (frames[i] if isinstance(frames, (list, tuple)) else lmax)
            if c.shape[0] != 1 or c.shape[-1] != want:
                raise ValueError(f'condition {i} has shape {tuple(c.shape)}; expected [1, cond_in, {want}]')
        out = torch.zeros(n_prompts, rows[0].shape[1], 2 * lmax, dtype=rows[0].dtype, device=rows[0].device)
        for i, c in enumerate(rows):
            out[i:i + 1, :, :c.shape[-1]] = c
        return out
    if condition is None or condition.dim() != 3 or condition.shape[0] not in (1, n_prompts) or condition.shape[-1] != 2 * lmax:
        raise ValueError(f'condition must be [1 or {n_prompts}, cond_in, {2 * lmax}] or a list of per-prompt tensors, '
                         f'got {None if condition is None else tuple(condition.shape)}')
    return condition


def draw_noises(codec_dim, audio_frames, ddim_steps, eta, random_seed, device, n_prompts=1, first_index=0, start_steps=None, canvas_offsets=None, canvas_loop=None):
    """Init noise + per-step DDIM noise in the order the reference draws them from ONE generator
    (src/inference.py:58-67 then one randn per scheduler.step, diffusers `randn_tensor`).  For several
    prompts each sample gets its own generator seeded seed + index, so results do not depend on how
    prompts are sharded over GPUs.

    ``audio_frames`` may be a list with one length per prompt: sample i then draws (1, C, len_i) tensors -- the numbers a call with
    that sample alone draws -- which are placed into zero-padded [.., max(lengths)] tensors.

    ``eta`` may be a list with one value per prompt: sample i draws what a call with it alone draws -- nothing per step when eta_i <= 0; its
    slice of the step noise is then zero, and the whole tensor is None when no sample draws.  ``random_seed`` may be a list of seeds: sample
    i seeds its generator with random_seed[i], as a single-prompt call with that seed does (a scalar seed keeps seed + first_index + i).

    ``start_steps`` (audio-to-audio, one step per prompt): sample i draws its init noise, then ddim_steps - start_steps[i] step noises when its eta > 0 --
    the numbers a call with that sample alone draws -- placed at the step indices start_steps[i] .. ddim_steps - 1 of the [K, P, C, L] tensor, which is
    indexed by absolute step; the slices before are zero and never read.

    ``canvas_offsets`` (long-form canvas, one offset per window; ``audio_frames`` is the window length L): ONE generator, seeded like the single prompt's,
    draws the init noise (1, C, T) of the canvas of T = canvas_offsets[-1] + L frames and then, when eta > 0, one (1, C, T) per step; window i receives the
    slice [canvas_offsets[i], canvas_offsets[i] + L), so the windows share their noise where they share frames.  One window draws what the plain call draws.

    ``canvas_loop=T`` with ``canvas_offsets`` (seamless loops): the canvas draws are (1, C, T) -- the numbers the plain call of T frames draws -- and window i
    receives the ring frames (canvas_offsets[i] + r) mod T, r in [0, L): the cut wraps."""
    if canvas_loop is not None and canvas_offsets is None:
        raise ValueError('canvas_loop is the length of the ring that canvas_offsets lie on')
    if canvas_offsets is not None:
        offs = [int(v) for v in canvas_offsets]
        if _is_seq(audio_frames) or _is_seq(eta) or _is_seq(random_seed) or start_steps is not None:
            raise ValueError('a canvas takes one window length, one eta and one seed, and no start steps')
        L = int(audio_frames)
        T = offs[-1] + L if canvas_loop is None else int(canvas_loop)
        g = torch.Generator(device=device)
        if random_seed is not None:
            g.manual_seed(random_seed + first_index)
        else:
            g.seed()
        cut = lambda t: torch.cat([t[:, :, o:o + L] for o in offs], dim=0)   # noqa: E731
        if canvas_loop is not None:
            if L > T:
                raise ValueError(f'windows of {L} frames on a ring of {T}')
            cut = lambda t: torch.cat([t[:, :, _ring(o, L, T, t.device)] for o in offs], dim=0)   # noqa: E731
        init = cut(torch.randn((1, codec_dim, T), generator=g, device=device))
        if not (eta or 0) > 0:
            return init, None
        return init, torch.stack([cut(torch.randn((1, codec_dim, T), generator=g, device=device)) for _ in range(ddim_steps)])
    if start_steps is not None and len(start_steps) != n_prompts:
        raise ValueError(f'{len(start_steps)} start steps for {n_prompts} prompts')
    lens = _frames_list(audio_frames, n_prompts)
    etas = _per_prompt(eta, n_prompts, 'eta') or [eta] * n_prompts
    etas = [e or 0 for e in etas]
    seeds = _per_prompt(random_seed, n_prompts, 'random_seed')
    Lmax = max(lens) if lens is not None else audio_frames
    init = torch.zeros((n_prompts, codec_dim, Lmax), device=device)
    step = torch.zeros((ddim_steps, n_prompts, codec_dim, Lmax), device=device) if max(etas) > 0 else None
    for i in range(n_prompts):
        li = lens[i] if lens is not None else audio_frames
        g = torch.Generator(device=device)
        if seeds is not None and seeds[i] is not None:
            g.manual_seed(int(seeds[i]))
        elif seeds is None and random_seed is not None:
            g.manual_seed(random_seed + first_index + i)
        else:
            g.seed()
        init[i:i + 1, :, :li] = torch.randn((1, codec_dim, li), generator=g, device=device)
        if etas[i] > 0:
            for k in range(int(start_steps[i]) if start_steps is not None else 0, ddim_steps):
                step[k, i:i + 1, :, :li] = torch.randn((1, codec_dim, li), generator=g, device=device)
    return init, step


def _timeline_entries(text_raw, prompt_weights, frames):
    """(entries, W): every entry of text_raw as its list of prompts, and the weights of the call [N, S, max(frames)] with S the largest number of prompts of an
    entry: entry i's own [S_i, frames_i] array in the corner, zeros behind (prompts it does not have, frames beyond its length).  A plain entry (one prompt,
    weights None) weights its prompt 1 at every frame."""
    n = len(text_raw)
    entries = [list(t) if isinstance(t, (list, tuple)) else [t] for t in text_raw]
    if prompt_weights is None:
        prompt_weights = [None] * n
    if len(prompt_weights) != n:
        raise ValueError(f'{len(prompt_weights)} entries of prompt_weights for {n} entries of text_raw')
    n_seg = max(len(e) for e in entries)
    if min(len(e) for e in entries) < 1 or n_seg > TIMELINE_MAX:
        raise ValueError(f'an entry of text_raw holds between 1 and {TIMELINE_MAX} prompts')
    W = torch.zeros(n, n_seg, max(frames))
    for i, (e, w) in enumerate(zip(entries, prompt_weights)):
        if w is None:
            if len(e) != 1:
                raise ValueError(f'entry {i} of text_raw has {len(e)} prompts and no prompt_weights')
            W[i, 0, :frames[i]] = 1.0
            continue
        w = torch.as_tensor(w, dtype=torch.float32)
        if tuple(w.shape) != (len(e), frames[i]):
            raise ValueError(f'prompt_weights[{i}] has shape {tuple(w.shape)}; expected [{len(e)} prompts, {frames[i]} frames]')
        W[i, :len(e), :frames[i]] = w
    return entries, W


def compose_entries(compose, n_prompts):
    """``compose`` of inference() as (extras, W): extras[k][i] is the text of extra condition k of prompt i and W [n_prompts, K] the weights, column 0 the
    primary prompt's 1.  One prompt takes a list of (text, weight) pairs; several take one such list (or None) per prompt.  Lists shorter than the longest
    are padded with the prompt's own text at weight 0 (a dropped condition: its row is not read).  (None, None) when no prompt composes anything: the plain call."""
    if n_prompts == 1 and compose and all(isinstance(e, (list, tuple)) and len(e) == 2 and isinstance(e[0], str) for e in compose):
        compose = [compose]
    if not isinstance(compose, (list, tuple)) or len(compose) != n_prompts:
        raise ValueError(f'compose: a list of (text, weight) pairs for one prompt, or one such list (or None) per prompt; got {len(compose) if isinstance(compose, (list, tuple)) else compose!r} entries for {n_prompts} prompts')
    lists = []
    for i, c in enumerate(compose):
        c = list(c or [])
        for e in c:
            if not (isinstance(e, (list, tuple)) and len(e) == 2 and isinstance(e[0], str)):
                raise ValueError(f'compose of prompt {i}: expected (text, weight) pairs, got {e!r}')
            w = float(e[1])
            if w != w or w in (float('inf'), float('-inf')):
                raise ValueError(f'compose of prompt {i}: weight {e[1]!r} is not finite')
        lists.append(c)
    n_extra = max(len(c) for c in lists)
    if n_extra == 0:
        return None, None
    if n_extra + 1 > COMPOSE_MAX:
        raise ValueError(f'{n_extra} composed prompts: at most {COMPOSE_MAX - 1} next to the primary one')
    W = torch.zeros(n_prompts, n_extra + 1)
    W[:, 0] = 1.0
    for i, c in enumerate(lists):
        for k, e in enumerate(c):
            W[i, k + 1] = float(e[1])
    return lists, W


EMPHASIS_MIN, EMPHASIS_MAX = 2.0 ** -10, 2.0 ** 10      # a span's weight, products of nested groups included


def parse_emphasis(text):
    """Prompt emphasis markup -> (clean_text, spans).  A group is ``(words:1.6)``: a parenthesis group that ends in ``:number``.  Groups nest and their weights
    multiply; ``\\(`` and ``\\)`` are literal parentheses; parentheses without ``:number`` are ordinary text and stay; ``(words:0)`` removes the words from the text.
    spans is a list of (start, end, weight) over characters of clean_text, one per group that is left, inner groups carrying the product.  ValueError: a group that
    is not closed (an opening parenthesis that a later ``:number)`` would have to close), or a weight outside [2^-10, 2^10] (0 aside).  ``:number)`` is markup wherever
    it stands: ordinary text that holds it outside a group, such as 'at 3:30)', raises as unbalanced -- write the parenthesis as ``\\)``."""
    import re
    num = re.compile(r':\s*([0-9]*\.?[0-9]+(?:[eE][-+]?[0-9]+)?)\s*\)')
    out = []           # characters of the clean text
    stack = []         # open parentheses: index into `out` of the '(' that was emitted
    spans = []         # (start, end, weight, depth-independent): closed groups, in clean-text coordinates
    i, n = 0, len(text)
    squeeze = False
    while i < n:
        ch = text[i]
        if ch == '\\' and i + 1 < n and text[i + 1] in '()':
            out.append(text[i + 1]); i += 2
            continue
        if ch == '(':
            stack.append(len(out)); out.append('('); i += 1
            continue
        m = num.match(text, i) if ch == ':' else None
        if m is not None and stack:
            w = float(m.group(1))
            start = stack.pop()
            del out[start]      # the group's parentheses are markup
            spans = [(a - (a > start), b - (b > start), ww) for a, b, ww in spans]
            end = len(out)
            if w == 0.0:       # the group leaves the text, and the spans inside it with it
                del out[start:end]
                spans = [(a, b, ww) for a, b, ww in spans if not (a >= start and b <= end and a < end)]
                squeeze = True      # (the space behind the group goes when one stands in front of it, or nothing does)
            else:
                spans = [(a, b, ww * w) if (a >= start and b <= end) else (a, b, ww) for a, b, ww in spans]
                spans.append((start, end, w))
            i = m.end()
            continue
        if m is not None and not stack:
            raise ValueError(f'unbalanced emphasis markup in {text!r}: ":{m.group(1)})" closes no group')
        if ch == ')':
            if stack:
                stack.pop()      # a plain parenthesis pair: ordinary text
            out.append(')'); i += 1
            continue
        if ch == ' ' and squeeze and (not out or out[-1] == ' '):
            i += 1
            continue
        squeeze = False
        out.append(ch); i += 1
    clean = ''.join(out).rstrip()      # (an opening parenthesis that no ':number)' closes is ordinary text)
    res = []
    for a, b, w in spans:
        # nested groups: the inner span carries the product already; an outer span covers the whole group, so per-token weights take the innermost span's weight
        if not (EMPHASIS_MIN <= w <= EMPHASIS_MAX):
            raise ValueError(f'emphasis weight {w:g} in {text!r} outside [2^-10, 2^10]')
        b = min(b, len(clean))
        if b > a:
            res.append((a, b, w))
    return clean, sorted(res, key=lambda t: (t[0], -t[1]))


def emphasis_weights(tokenizer, clean_text, spans, max_length):
    """Per-token weights [Lt] (a list of max_length floats) of ``clean_text`` under ``spans`` of parse_emphasis().  The tokenizer need not give offsets: a span boundary at
    character p maps to token index len(tokenizer(clean_text[:p], add_special_tokens=False).input_ids), and those ids must be a prefix of the ids of the whole text
    (spans cover whole words), otherwise ValueError naming the span.  A token takes the weight of the innermost span that holds it; tokens outside every span, EOS
    and the padding weigh 1.  Truncation at max_length truncates the weights."""
    ids = list(tokenizer(clean_text, add_special_tokens=False).input_ids)
    w = [1.0] * len(ids)

    def at(p, span):
        pre = list(tokenizer(clean_text[:p], add_special_tokens=False).input_ids)
        if pre != ids[:len(pre)]:
            raise ValueError(f'emphasis span {clean_text[span[0]:span[1]]!r} (characters {span[0]}:{span[1]}) does not fall on token boundaries of {clean_text!r}: spans cover whole words')
        return len(pre)
    for sp in sorted(spans, key=lambda t: t[1] - t[0], reverse=True):      # outer spans first: inner ones overwrite with their product
        a, b = at(sp[0], sp), at(sp[1], sp)
        for j in range(a, b):
            w[j] = float(sp[2])
    w = (w + [1.0])[:max_length]      # EOS
    return w + [1.0] * (max_length - len(w))


@torch.no_grad()
def inference_controlnet(autoencoder, unet, controlnet, gt, gt_mask, condition, tokenizer, text_encoder, params,
                         noise_scheduler, text_raw, neg_text=None, audio_frames=500, guidance_scale=3,
                         guidance_rescale=0.0, ddim_steps=50, eta=1, random_seed=2024, conditioning_scale=1.0,
                         device='cuda', use_graph=True, init_latents=None, strength=None, solver='ddim'):
    """Same signature and semantics as the reference's ControlNet ``inference`` (src/inference_controlnet.py:27-129); ``solver``, ``init_latents`` and
    ``strength`` as in ``inference``."""
    return inference(autoencoder, unet, gt, gt_mask, tokenizer, text_encoder, params, noise_scheduler, text_raw, neg_text,
                     audio_frames, guidance_scale, guidance_rescale, ddim_steps, eta, random_seed, device, use_graph,
                     controlnet=controlnet, condition=condition, conditioning_scale=conditioning_scale, solver=solver,
                     init_latents=init_latents, strength=strength)


@torch.no_grad()
def inference(autoencoder, unet, gt, gt_mask, tokenizer, text_encoder, params, noise_scheduler, text_raw,
              neg_text=None, audio_frames=500, guidance_scale=3, guidance_rescale=0.0, ddim_steps=50, eta=1,
              random_seed=2024, device='cuda', use_graph=True, controlnet=None, condition=None, conditioning_scale=1.0,
              first_index=None, init_latents=None, strength=None, attention_window=None, prompt_weights=None, compose=None, emphasis=False, token_weights=None, apg=None, canvas_loop=None, decode_context=None, canvas_offsets=None, canvas_ramp=None,
              solver='ddim'):
    """Same signature and semantics as the reference's ``inference`` (src/inference.py:26-107).

    Extension (adaptive projected guidance, Sadat et al.): ``apg`` is True, a dict(eta=, norm_threshold=, momentum=) or a list with one such entry (or None) per
    prompt (apg_entries()): a prompt with an entry is guided on its data prediction -- the guidance direction carries a (negative) momentum across steps, is capped
    at norm_threshold and loses its component parallel to the conditional prediction (eta: the share of it that stays) -- which is what keeps a high guidance_scale
    from over-driving the latent; the other prompts are guided as always.  True means eta 0, momentum -0.5 and NO cap: which norm_threshold suits the EzAudio latent
    is unmeasured, so none is invented.  It combines with ``audio_frames`` lists, per-prompt settings, ``solver``, gt / gt_mask, ``init_latents``, a ControlNet, a
    timeline, emphasis and ``attention_window``, and is sliced with the prompts on a call sharded over ranks; ValueError with ``compose``, a canvas or loop, for a
    prompt that asks for it without guidance or together with a guidance_rescale above 0 (the rescale is not applied to projected guidance).  No entry for any
    prompt is the plain call, bit for bit.  Audio quality on the real checkpoints -- which cap, eta and momentum sound best -- is unmeasured.

    Extension (prompt emphasis): ``emphasis=True`` parses '(words:1.6)' markup (parse_emphasis) in every prompt of the call -- ``text_raw``, the extra prompts of
    ``compose`` and ``neg_text`` -- the text encoder sees the clean text, and token j of a prompt weighs its group's weight in every block's cross-attention
    (include/ezdit.h ezdit_set_context_token_weights); the table is passed on only if some weight is not 1.  ``token_weights`` [N, max_length] gives the primary
    prompts' weights directly.  ValueError with a prompt timeline or a ControlNet.  On a call sharded over ranks each rank parses its own prompts.  The default
    leaves every prompt verbatim.  Audio quality on the real checkpoints is unmeasured.

    Extension (composed guidance): ``compose`` gives a prompt further prompts with weights: for one prompt a list of (text, weight) pairs, for several one such
    list (or None) per prompt.  Every prompt is guided against the shared negative prompt with its own weight, v = u + guidance_scale ((c_0 - u) + sum_k w_k (c_k - u));
    the primary prompt has weight 1 and is the reference of the guidance rescale.  A negative weight is a negative prompt that keeps the empty-prompt baseline (``neg_text``
    replaces it).  Shorter lists are padded with the prompt's own text at weight 0; all prompts of the call are encoded in one text-encoder batch.  The batch grows to
    (K + 1) rows per prompt.  It combines with ``audio_frames`` lists, per-prompt settings, ``solver``, gt / gt_mask, ``init_latents`` and ``attention_window``;
    ValueError with a ControlNet, a canvas or loop, a timeline, without guidance, or for a call that would be sharded over ranks.  No entry for any prompt is the
    plain call, bit for bit.  Audio quality on the real checkpoints is unmeasured.

    Extension (sliding-window self-attention): ``attention_window`` is a radius in latent frames: in every block's self-attention a frame attends to the frames
    within that many frames of it, so a row longer than the trained length stays inside the trained range of relative positions.  It is set on ``unet`` (and on
    ``controlnet``) before anything is prepared and the previous value is put back when the call ends, also when it raises; the shards of a distributed call run
    on the same models and so under the same window.  It combines with everything below; a canvas' windows are short, so there it changes nothing.  Audio quality
    on the real checkpoints is unmeasured.

    Extension: ``solver='dpmpp_2m'`` samples with DPM-Solver++(2M) instead of DDIM (deterministic: eta must be 0, the signature's
    default eta=1 is refused, not ignored).  How few steps give the quality of a longer DDIM run on the real checkpoints is unmeasured.

    Extension: with ``torch.distributed`` initialised and several prompts, every rank samples AND
    VAE-decodes its own contiguous shard of the prompts and the waveforms are all-gathered once (RCCL).

    Extension: ``guidance_scale``, ``guidance_rescale``, ``eta`` and ``random_seed`` may each be a list with one entry per prompt (a guidance of
    None / 0 = that prompt runs without guidance): every prompt comes out as the call with it alone gives it.  ``ddim_steps`` stays one value.

    Extension: ``audio_frames`` may be a list with one latent length per prompt (mixed-length batch).  gt / gt_mask are then padded to
    max(audio_frames) frames; a prompt WITHOUT a reference clip in a batch that has some carries gt_mask all ones (that is the
    reference's no-gt input, src/models/conditioners.py:173-176).  The VAE decodes every sample at its own length (its convolutions have
    boundaries too) -- in one ragged call when the autoencoder is this package's ``Autoencoder``, one by one through an injected callable; the
    result is [N, 1, Tmax], zero beyond each sample's own duration.

    Extension: all of this with a ControlNet too.  ``condition`` is then [N or 1, cond_in, 2 * max(audio_frames)], padded (what lies behind a
    sample's own 2 * audio_frames[i] frames is ignored), or a list of N tensors [1, cond_in, 2 * audio_frames[i]], which is padded here;
    ``conditioning_scale`` may be a list with one value per prompt.

    Extension (audio-to-audio): ``init_latents`` [N or 1, C, max(audio_frames)] in VAE space (the encoder's output, padded when ``audio_frames`` is a
    list) with ``strength`` in (0, 1], one value or one per prompt: prompt i starts at step ``noise_scheduler.start_step(strength_i)`` from its clip
    noised to that step instead of from pure noise, and runs the steps that are left.  strength 1 is the plain call, bit for bit.  The latent's
    scale and shift come from ``params['autoencoder']``.  Audio quality versus strength on the real checkpoints is unmeasured.

    Extension (long-form generation): ``canvas_offsets`` (canvas_windows() chooses them) makes the call ONE clip of canvas_offsets[-1] + audio_frames latent
    frames, sampled as overlapping windows of ``audio_frames`` frames whose shared frames are averaged inside every step with the ramp ``canvas_ramp``
    (None: the smallest overlap between neighbours, a linear cross-fade; 1: the plain mean).  ``text_raw`` is one prompt for every window or a list with one
    prompt per window (a scene that changes over time); the settings are scalars; no gt, ControlNet or init_latents.  The canvas is decoded in one call:
    the result is [1, 1, T * ratio].  The windows are coupled, so the call is never sharded over ranks.  One window is the plain call.  Audio quality on the
    real checkpoints -- seam audibility, the choice of overlap and ramp, the comparison with one long row -- is unmeasured.

    Extension (seamless loops): ``canvas_loop=T`` with ``canvas_offsets`` (loop_windows() chooses them) makes the canvas a RING of T >= audio_frames latent
    frames: window p holds the frames (canvas_offsets[p] + r) mod T, the last window runs into the first, and the default ramp is the smallest cyclic overlap.
    The ring is decoded as a ring (decode_circular, with ``decode_context`` wrapped frames on either side; None asks the autoencoder): the result is
    [1, 1, T * ratio], and its end continues into its beginning.  Everything else as with the line; audio quality on the real checkpoints is unmeasured.

    Extension (prompt timeline): an entry of ``text_raw`` may be a LIST of prompts, and ``prompt_weights`` a list with one [S_i, frames_i] array (or None for a plain
    entry) per entry of ``text_raw``: frame j of sample i weights its prompt s by prompt_weights[i][s][j] in every block's cross-attention (scene_weights() makes
    such weights from a scene with times), so prompts switch, cross-fade or mix inside ONE sample.  Entries with fewer prompts than the largest are padded with
    prompts of weight 0.  It combines with ``audio_frames`` lists, per-prompt settings, ``solver``, gt / gt_mask, ``init_latents`` and ``attention_window``;
    ValueError with a canvas, a ControlNet, or a call that would be sharded over ranks.  Audio quality on the real checkpoints is unmeasured."""
    if attention_window is not None:
        if isinstance(attention_window, bool) or int(attention_window) != attention_window or int(attention_window) < 1:
            raise ValueError(f'attention_window is a radius in latent frames, a whole number >= 1: got {attention_window!r}')
        models = [unet] + ([controlnet] if controlnet is not None else [])
        previous = [getattr(m, 'attention_window', None) for m in models]
        try:
            for m in models:
                m.set_attention_window(int(attention_window))
            return inference(autoencoder, unet, gt, gt_mask, tokenizer, text_encoder, params, noise_scheduler, text_raw, neg_text, audio_frames, guidance_scale,
                             guidance_rescale, ddim_steps, eta, random_seed, device, use_graph, controlnet, condition, conditioning_scale, first_index=first_index,
                             init_latents=init_latents, strength=strength, canvas_loop=canvas_loop, decode_context=decode_context, canvas_offsets=canvas_offsets,
                             canvas_ramp=canvas_ramp, solver=solver, prompt_weights=prompt_weights, compose=compose, emphasis=emphasis, token_weights=token_weights, apg=apg)
        finally:
            for m, prev in zip(models, previous):
                m.set_attention_window(prev)
    if (init_latents is None) != (strength is None):
        raise ValueError('init_latents and strength must be given together')
    if neg_text is None:
        neg_text = [""]
    if canvas_offsets is not None:
        canvas_offsets = [int(v) for v in canvas_offsets]
        n_win = len(canvas_offsets)
        if isinstance(text_raw, str):
            text_raw = [text_raw] * n_win
        elif len(text_raw) == 1:
            text_raw = list(text_raw) * n_win
        if len(text_raw) != n_win:
            raise ValueError(f'{len(text_raw)} prompts for a canvas of {n_win} windows: one prompt, or one per window')
        if _is_seq(audio_frames):
            raise ValueError('a canvas takes one window length (audio_frames)')
        for name, v in (('guidance_scale', guidance_scale), ('guidance_rescale', guidance_rescale), ('eta', eta), ('random_seed', random_seed)):
            if _is_seq(v):
                raise ValueError(f'a canvas takes one {name}, not one per window')
        if gt is not None or gt_mask is not None or controlnet is not None or init_latents is not None:
            raise ValueError('a canvas does not combine with gt / gt_mask, a ControlNet or init_latents')
        if canvas_loop is not None:
            canvas_loop = int(canvas_loop)
            if canvas_ramp is None:
                canvas_ramp = max(1, min(loop_overlaps(canvas_offsets, audio_frames, canvas_loop))) if n_win else 1
            check_canvas_loop(canvas_offsets, audio_frames, canvas_loop, canvas_ramp)
        else:
            overlaps = [a + audio_frames - b for a, b in zip(canvas_offsets, canvas_offsets[1:])]
            if canvas_ramp is None:
                canvas_ramp = max(1, min(overlaps)) if overlaps else 1
            check_canvas(canvas_offsets, audio_frames, canvas_offsets[-1] + audio_frames, canvas_ramp)
    elif canvas_ramp is not None or canvas_loop is not None:
        raise ValueError('canvas_ramp / canvas_loop without canvas_offsets')
    if decode_context is not None and canvas_loop is None:
        raise ValueError('decode_context belongs to canvas_loop: only a ring is decoded with wrapped context')
    if isinstance(text_raw, str):
        text_raw = [text_raw]
    if isinstance(ddim_steps, (list, tuple)):
        raise ValueError('ddim_steps must be one value per call: per-prompt step counts are not supported (the prompts of a call share its timesteps)')
    for name, v in (('guidance_scale', guidance_scale), ('guidance_rescale', guidance_rescale), ('eta', eta), ('random_seed', random_seed),
                    ('conditioning_scale', conditioning_scale), ('strength', strength)):
        _per_prompt(v, len(text_raw), name)   # a list has one entry per prompt
    check_solver(solver, eta)
    # one entry per prompt of the call (an entry of a timeline is one prompt here), in the form prepare() takes; None when nobody asks
    apg_rows = apg_entries(apg, len(text_raw))
    check_apg(apg_rows, guidance_scale, guidance_rescale, canvas=canvas_offsets is not None)
    apg = None if apg_rows is None else [dict(eta=r[0], norm_threshold=r[1], momentum=r[2]) if r[3] else None for r in apg_rows]
    import torch.distributed as dist
    frames = _frames_list(audio_frames, len(text_raw))
    timeline = None
    if prompt_weights is not None or any(isinstance(t, (list, tuple)) for t in text_raw):
        if canvas_offsets is not None or controlnet is not None:
            raise ValueError('a prompt timeline does not combine with a canvas or a ControlNet')
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1 and len(text_raw) > 1 and first_index is None:
            raise ValueError('a prompt timeline is not sharded over ranks: call it with one rank\'s prompts')
        timeline = _timeline_entries(text_raw, prompt_weights, frames if frames is not None else [int(audio_frames)] * len(text_raw))
        text_raw = [p for entry in timeline[0] for p in entry]      # every prompt of every entry, encoded in one batch below
    composed = None
    if compose is not None:
        if controlnet is not None or canvas_offsets is not None or timeline is not None:
            raise ValueError('composed guidance does not combine with a ControlNet, a canvas or loop, or a prompt timeline')
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1 and len(text_raw) > 1 and first_index is None:
            raise ValueError('composed guidance is not sharded over ranks: call it with one rank\'s prompts')
        lists, cw = compose_entries(compose, len(text_raw))
        if lists is not None:
            check_apg(apg_rows, guidance_scale, guidance_rescale, compose=True)
            composed = (len(text_raw), cw)
            # every prompt of the call in ONE text-encoder batch: the primaries, then extra condition k of every prompt (a missing one: the prompt's own text, weight 0)
            text_raw = list(text_raw) + [lists[i][k][0] if k < len(lists[i]) else text_raw[i] for k in range(cw.shape[1] - 1) for i in range(len(text_raw))]
    if controlnet is not None:
        condition = pad_conditions(condition, frames if frames is not None else audio_frames, len(text_raw))
    if canvas_offsets is None and composed is None and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1 and len(text_raw) > 1 and first_index is None:
        from .dist import sample_sharded, slice_per_prompt
        n_all = len(text_raw)
        ratio_ = params['autoencoder']['sr'] // params['autoencoder']['latent_sr']
        t_all = (max(frames) if frames is not None else audio_frames) * ratio_   # every shard is gathered at the GLOBAL duration
        neg_all = list(neg_text) * n_all if len(neg_text) == 1 else list(neg_text)

        def local(s, e):
            if e == s:   # more ranks than prompts: contribute an empty shard of the common shape
                return torch.zeros(0, 1, t_all, device=device)
            sl = lambda t: t if t is None or t.shape[0] == 1 else t[s:e]   # noqa: E731  per-prompt tensors are sliced
            pp = lambda v: list(v[s:e]) if _per_prompt(v, n_all, 'setting') is not None else v   # noqa: E731  ... and so are per-prompt settings
            # mixed lengths: the lengths are sliced with the prompts, per-prompt tensors additionally cut to the shard's own padded length (the control
            # signal has two frames per latent frame).  One length for all: nothing to cut, and the shard comes out at the global duration by itself
            lmax = None if frames is None else max(frames[s:e])
            cut = lambda t, per_frame=1: t if t is None else sl(t)[..., :None if lmax is None else per_frame * lmax]   # noqa: E731
            wav = inference(autoencoder, unet, cut(gt), cut(gt_mask), tokenizer, text_encoder, params, noise_scheduler,
                            list(text_raw[s:e]), neg_all[s:e], audio_frames if frames is None else frames[s:e], pp(guidance_scale), pp(guidance_rescale),
                            ddim_steps, pp(eta), pp(random_seed), device, use_graph, controlnet, cut(condition, 2), pp(conditioning_scale), first_index=s,
                            solver=solver, init_latents=cut(init_latents), strength=pp(strength), emphasis=emphasis,
                            token_weights=None if token_weights is None else torch.as_tensor(token_weights)[s:e], apg=slice_per_prompt(apg, s, e, n_all))
            if frames is None:
                return wav
            out = torch.zeros(wav.shape[0], wav.shape[1], t_all, dtype=wav.dtype, device=wav.device)
            out[..., :wav.shape[-1]] = wav
            return out
        return sample_sharded(local, n_all)
    first_index = first_index or 0
    n_prompts = len(text_raw)
    if (emphasis or token_weights is not None) and (timeline is not None or controlnet is not None):
        raise ValueError('prompt emphasis does not combine with a prompt timeline or a ControlNet')
    if emphasis and token_weights is not None:
        raise ValueError('emphasis=True and token_weights: give one')
    emph = None
    if tokenizer is not None:
        max_len = params['text_encoder']['max_length']
        if emphasis:      # every prompt of the call: the primaries and the extra conditions (text_raw holds both by now), and the negative prompts
            parsed = [parse_emphasis(t) for t in text_raw]
            text_raw = [c for c, _ in parsed]
            w_text = torch.tensor([emphasis_weights(tokenizer, c, sp, max_len) for c, sp in parsed], dtype=torch.float32)
            neg_parsed = [parse_emphasis(t) for t in neg_text]
            neg_text = [c for c, _ in neg_parsed]
            w_neg = torch.tensor([emphasis_weights(tokenizer, c, sp, max_len) for c, sp in neg_parsed], dtype=torch.float32)
            emph = (w_text, w_neg)
        elif token_weights is not None:
            w_text = torch.as_tensor(token_weights, dtype=torch.float32).cpu()
            n_primary = composed[0] if composed is not None else n_prompts
            if tuple(w_text.shape) != (n_primary, max_len):
                raise ValueError(f'token_weights {tuple(w_text.shape)}: expected [{n_primary}, {max_len}]')
            emph = (torch.cat([w_text, torch.ones(n_prompts - n_primary, max_len)]), torch.ones(len(neg_text), max_len))
        tb = tokenizer(text_raw, max_length=max_len, padding="max_length", truncation=True, return_tensors="pt")
        text, text_mask = tb.input_ids.to(device), tb.attention_mask.to(device).bool()
        text = text_encoder(input_ids=text, attention_mask=text_mask).last_hidden_state
        if timeline is not None:      # [N, S, Lt, Cctx]: entry i's prompts in its first S_i places, the places behind empty (all masked, weight 0)
            entries, tl_w = timeline
            n_prompts, n_seg = len(entries), tl_w.shape[1]
            t4 = torch.zeros((n_prompts, n_seg) + tuple(text.shape[1:]), dtype=text.dtype, device=text.device)
            m4 = torch.zeros((n_prompts, n_seg, text.shape[1]), dtype=torch.bool, device=text.device)
            at = 0
            for i, entry in enumerate(entries):
                t4[i, :len(entry)], m4[i, :len(entry)] = text[at:at + len(entry)], text_mask[at:at + len(entry)]
                at += len(entry)
            text, text_mask = t4, m4
        if composed is not None:      # [N, K-1, Lt, Cctx]: the batch was primaries, then condition 1 of every prompt, condition 2 of every prompt, ...
            n_prompts, cw = composed
            comp_text = text[n_prompts:].reshape((cw.shape[1] - 1, n_prompts) + tuple(text.shape[1:])).transpose(0, 1).contiguous()
            comp_mask = text_mask[n_prompts:].reshape(cw.shape[1] - 1, n_prompts, text.shape[1]).transpose(0, 1).contiguous()
            text, text_mask = text[:n_prompts], text_mask[:n_prompts]
        ub = tokenizer(neg_text * n_prompts if len(neg_text) == 1 else neg_text, max_length=max_len,
                       padding="max_length", truncation=True, return_tensors="pt")
        uncond_text, uncond_mask = ub.input_ids.to(device), ub.attention_mask.to(device).bool()
        uncond_text = text_encoder(input_ids=uncond_text, attention_mask=uncond_mask).last_hidden_state
    else:
        raise NotImplementedError('tokenizer=None (unconditional model) is not a shipped configuration')
    codec_dim = params['model']['out_chans']
    unet.eval()
    a2a = {}
    if init_latents is not None:
        noise_scheduler.set_timesteps(ddim_steps)
        starts = [noise_scheduler.start_step(v) for v in (_per_prompt(strength, n_prompts, 'strength') or [strength] * n_prompts)]
        lmax = max(frames) if frames is not None else audio_frames
        if init_latents.dim() != 3 or init_latents.shape[0] not in (1, n_prompts) or tuple(init_latents.shape[1:]) != (codec_dim, lmax):
            raise ValueError(f'init_latents must be [1 or {n_prompts}, {codec_dim}, {lmax}], got {tuple(init_latents.shape)}')
        a2a = dict(init_latents=init_latents, start_steps=starts, latent_scale=params['autoencoder']['scale'], latent_shift=params['autoencoder']['shift'])
    long_form = canvas_offsets is not None and (len(canvas_offsets) > 1 or canvas_loop is not None)   # (one window of a line is the plain call, through the plain code)
    init, step_noises = draw_noises(codec_dim, audio_frames, ddim_steps, eta, random_seed, device, n_prompts, first_index,
                                    **(dict(start_steps=a2a['start_steps']) if a2a else {}), **(dict(canvas_offsets=canvas_offsets) if long_form else {}),
                                    **(dict(canvas_loop=canvas_loop) if canvas_loop is not None else {}))
    smp = LatentSampler(unet, noise_scheduler)
    # equal lengths are the unpadded batch (the same bits; include/ezdit.h ezdit_set_lengths): the length table is for ragged batches only
    ragged = frames is not None and len(set(frames)) > 1
    kw = dict(lengths=frames) if ragged else {}
    if solver != 'ddim':
        kw['solver'] = solver
    if timeline is not None:
        kw['context_weights'] = timeline[1]
    if emph is not None and (bool((emph[0] != 1).any()) or bool((emph[1] != 1).any())):      # (all weights 1: the plain call, no table)
        w_text, w_neg = emph
        n_primary = composed[0] if composed is not None else n_prompts
        kw['token_weights'] = w_text[:n_primary]
        if composed is not None:
            kw['compose_token_weights'] = w_text[n_primary:].reshape(composed[1].shape[1] - 1, n_primary, -1).transpose(0, 1).contiguous()
        if bool((w_neg != 1).any()):
            kw['uncond_token_weights'] = w_neg.expand(n_primary, -1) if w_neg.shape[0] == 1 else w_neg
    if composed is not None:
        kw.update(compose_text=comp_text.float(), compose_mask=comp_mask, compose_weights=composed[1])
    if apg is not None:
        kw['apg'] = apg
    if canvas_loop is not None:
        kw['canvas_loop'] = (canvas_offsets, canvas_loop, canvas_ramp)
    elif long_form:
        kw['canvas'] = (canvas_offsets, canvas_offsets[-1] + audio_frames, canvas_ramp)
    smp.prepare(text.float(), text_mask, uncond_text.float(), uncond_mask, init, step_noises, guidance_scale,
                guidance_rescale, ddim_steps, eta, gt=gt, gt_mask=gt_mask, controlnet=controlnet, condition=condition,
                conditioning_scale=conditioning_scale, **kw, **a2a)
    smp.run(use_graph=use_graph)
    latents = smp.finish()
    if canvas_loop is not None:   # one decode of the ring, with wrapped context
        return decode_circular(autoencoder, scale_shift_re(smp.canvas_latents(), params['autoencoder']['scale'], params['autoencoder']['shift']), decode_context)
    if long_form:   # one decode of the whole canvas
        return autoencoder(embedding=scale_shift_re(smp.canvas_latents(), params['autoencoder']['scale'], params['autoencoder']['shift']))
    pred = scale_shift_re(latents, params['autoencoder']['scale'], params['autoencoder']['shift'])
    if gt is not None:   # src/inference.py:103-104, with a shared [1, C, L] reference broadcast over the prompts
        keep = ~gt_mask.to(pred.device).expand_as(pred)
        pred = torch.where(keep, gt.to(pred.device, pred.dtype).expand_as(pred), pred)
    if not ragged:
        return autoencoder(embedding=pred)
    from .vae import Autoencoder
    if isinstance(autoencoder, Autoencoder):   # one ragged decode: every sample at its own length, stacked with zero gaps (ezaudio_amd/vae.py)
        return autoencoder(embedding=pred, lengths=frames)
    wavs = [autoencoder(embedding=pred[i:i + 1, :, :li]) for i, li in enumerate(frames)]   # an injected callable with the reference's surface: one by one
    out = torch.zeros(n_prompts, wavs[0].shape[1], max(w.shape[-1] for w in wavs), dtype=wavs[0].dtype, device=wavs[0].device)
    for i, w in enumerate(wavs):
        out[i:i + 1, :, :w.shape[-1]] = w
    return out
