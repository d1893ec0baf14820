"""Composed guidance (the AND of Liu et al., "Compositional Visual Generation with Composable Diffusion Models") as the tail of the sampler step: the definition
in float64, an fp32 emulation in the order of operations of k_cfg_stats / k_cfg_apply (element-wise expressions in fp32 with k ascending, 64 chunked partial
sums in fp32, their reduction and the ratio in double), eight deliberate mistakes built into copies of that emulation, the operator inputs that the CPU and
the GPU tests share, and the checking code of the GPU operator tests.  numpy only.

    batch rows   [c_0 (P rows) | c_1 (P rows) | ... | c_{K-1} (P rows) | u (P rows)]: row k P + p is condition k of sample p, row K P + p its unconditional row
    d  = w_0 (c_0 - u);  d += w_k (c_k - u), k = 1 .. K-1          (a weight of exactly 0: the row is not read)
    v  = u + g d                                                      (g <= 0: v = c_0, nothing else is read)
    v  = phi (v std(c_0) / std(v)) + (1 - phi) v   when phi > 0       (unbiased, over the sample's valid elements: the reference is the PRIMARY condition)
    x0 = sa x - sb v;  eps = sa v + sb x;  x_next = c_x0 x0 + c_dir eps (+ sigma z) (+ c_hist (x0 - x0_hist), x0_hist <- x0 with the multistep solver)

A row of `params`: (g, phi, sa, sb, c_x0, c_dir, sigma, c_hist), the layout of ezdit_cfg_compose_step; `weights` is [P][K].
"""
import functools

import numpy as np

NB, WG = 64, 256      # the statistics pass: 64 workgroups of 256 threads per sample, element i belongs to workgroup (i // 256) % 64
K_MAX = 8             # include/ezdit.h EZDIT_COMPOSE_MAX

MISTAKES = ('rescale_ref_weighted_mean', 'stats_over_padding', 'weight0_row_read', 'row_index_pK', 'uncond_at_P', 'weights_kP', 'g_twice', 'hist_from_c0')


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        return float('inf')
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def combine_fp64(conds, u, w, g, phi):
    """v of one sample on its valid elements: conds a list of K arrays, u one array, w K weights; float64."""
    conds = [np.asarray(c, np.float64) for c in conds]
    if not g > 0:
        return conds[0]
    u = np.asarray(u, np.float64)
    d = float(w[0]) * (conds[0] - u)
    for k in range(1, len(conds)):
        if float(w[k]) != 0.0:
            d = d + float(w[k]) * (conds[k] - u)
    v = u + g * d
    if phi > 0:
        v = phi * (v * (conds[0].std(ddof=1) / v.std(ddof=1))) + (1 - phi) * v
    return v


def step_fp64(pred, lat, hist, noise, params, weights, lens):
    """One call of the operator in float64: (latents, x0_hist) [P, C, L], zero on padded frames.  hist None: the DDIM form (noise [P, C, L] or None);
    given: the multistep form."""
    P, K = weights.shape
    out, hout = np.zeros(lat.shape, np.float64), np.zeros(lat.shape, np.float64)
    for p in range(P):
        g, phi, sa, sb, cx0, cdir, sigma, ch = (float(t) for t in params[p])
        n = lens[p]
        x = lat[p, :, :n].astype(np.float64)
        v = combine_fp64([pred[k * P + p, :, :n] for k in range(K)], pred[K * P + p, :, :n], weights[p], g, phi)
        x0, eps = sa * x - sb * v, sa * v + sb * x
        prev = cx0 * x0 + cdir * eps
        if hist is None and noise is not None and sigma != 0:
            prev = prev + sigma * noise[p, :, :n].astype(np.float64)
        if hist is not None and ch != 0:
            prev = prev + ch * (x0 - hist[p, :, :n].astype(np.float64))
        out[p, :, :n], hout[p, :, :n] = prev, x0
    return out, hout


def _partials(vals, idx):
    """The 64 fp32 partial sums of the statistics pass (vals fp32 over the flat elements idx of the sample), then their sum in double in the fixed order."""
    blk = (idx // WG) % NB
    tot = 0.0
    for b in range(NB):
        tot += float(np.sum(vals[blk == b], dtype=np.float32))
    return tot


def step_emul(pred, lat, hist, noise, params, weights, lens, mistake=None):
    """The operator as the kernels compute it.  `mistake` (one of MISTAKES) builds that error in.  'stats_over_padding' reads the padded frames and
    'weight0_row_read' the rows of weight 0: what they read shows in the result (NaN there makes it NaN)."""
    assert mistake is None or mistake in MISTAKES
    f = np.float32
    P, K = weights.shape
    Cc, L = lat.shape[1:]
    wflat = np.asarray(weights, f).ravel()
    out, hout = np.zeros(lat.shape, f), np.zeros(lat.shape, f)
    flat = np.arange(Cc * L).reshape(Cc, L)
    for p in range(P):
        g, phi, sa, sb, cx0, cdir, sigma, ch = (f(t) for t in params[p])
        n = lens[p]
        w = [wflat[k * P + p] if mistake == 'weights_kP' else wflat[p * K + k] for k in range(K)]
        row = (lambda k: p * K + k) if mistake == 'row_index_pK' else (lambda k: k * P + p)
        urow = P + p if mistake == 'uncond_at_P' else K * P + p

        def guided(ns):
            """(c_0, v before the rescale) on the first ns frames."""
            c0 = pred[row(0), :, :ns].astype(f)
            if not g > 0:
                return c0, c0
            u = pred[urow, :, :ns].astype(f)
            gk = g if mistake == 'g_twice' else f(1)
            d = (gk * w[0]) * (c0 - u)
            for k in range(1, K):
                if w[k] != 0 or mistake == 'weight0_row_read':
                    d = d + (gk * w[k]) * (pred[row(k), :, :ns].astype(f) - u)
            return c0, u + g * d
        c0, v = guided(n)
        if g > 0 and phi > 0:
            ns = L if mistake == 'stats_over_padding' else n
            cs, vs = guided(ns)
            if mistake == 'rescale_ref_weighted_mean':
                cs = sum(w[k] * pred[row(k), :, :ns].astype(f) for k in range(K)) / f(sum(w))
            idx = flat[:, :ns].ravel()
            s1, q1 = _partials(cs.ravel(), idx), _partials((cs * cs).ravel(), idx)
            s2, q2 = _partials(vs.ravel(), idx), _partials((vs * vs).ravel(), idx)
            nv = Cc * ns
            v1, v2 = (q1 - s1 * s1 / nv) / (nv - 1), (q2 - s2 * s2 / nv) / (nv - 1)
            ratio = f(np.sqrt(v1) / np.sqrt(v2))
            v = phi * (v * ratio) + (f(1) - phi) * v
        x = lat[p, :, :n].astype(f)
        x0, eps = sa * x - sb * v, sa * v + sb * x
        prev = cx0 * x0 + cdir * eps
        if hist is None and noise is not None and sigma != 0:
            prev = prev + sigma * noise[p, :, :n].astype(f)
        if hist is not None and ch != 0:
            prev = prev + ch * (x0 - hist[p, :, :n].astype(f))
        out[p, :, :n] = prev
        hout[p, :, :n] = sa * x - sb * c0 if mistake == 'hist_from_c0' else x0
    return out, hout


def distance(got, ref, lens, with_hist=True):
    """The largest rel-L2 over the outputs (latents, and x0_hist when the form has one) and the samples, each on the sample's valid frames; inf when a value is
    not finite."""
    worst = 0.0
    for g, r in list(zip(got, ref))[:2 if with_hist else 1]:
        for p, n in enumerate(lens):
            worst = max(worst, rel_l2(g[p, :, :n], r[p, :, :n]))
    return worst


# ---------------------------------------------------------------------------------------------------
# the operator cases of tests/test_compose_host.py and tests/test_compose_gpu.py
# ---------------------------------------------------------------------------------------------------
L_OP, C_OP = 150, 128                  # n = 128 x 150 = 19200: the grid-stride loop of 64 x 256 threads takes a second, partial trip
LENS_OP = (None, (131, 77, 1))
W3 = ((1.0, 0.8, -0.5), (0.7, 0.0, 1.3), (1.0, 0.5, 0.5))      # sample 1 has its second slot at weight 0; sample 2 runs without guidance


def mid_schedule_coef(eta=0.0):
    """(sa, sb, c_x0, c_dir, sigma) of step 7 of 50."""
    from ezaudio_amd.scheduler import DDIMScheduler
    from tests.util import DIFF
    sch = DDIMScheduler(**DIFF)
    sch.set_timesteps(50)
    co = sch._coef(int(sch.timesteps[7]), eta)
    assert 0.05 < co[0] < 0.95
    return co


@functools.lru_cache(maxsize=None)
def operator_case(K, lens, ms, P=3):
    """Inputs of one operator case, all finite everywhere (poisoned() marks what must not be read).  P = 3: sample 0 guidance 5 with rescale 0.75, sample 1
    guidance 2 without rescale, sample 2 no guidance (g = 0).  ms: the multistep form, c_hist (0.05, 0.4, 0) and no noise; otherwise the DDIM form with
    noise, sample 1 at sigma 0 (eta 0).  P = 1 (the K = 8 case): sample 0 alone, with alternating weights.
    Returns dict(pred [(K+1)P, C, L], lat, hist or None, noise or None, params [P, 8], weights [P, K], lens)."""
    rng = np.random.default_rng(9100 + 10 * K + (1 if ms else 0) + (100 if lens else 0) + 1000 * P)
    L, Cc = L_OP, C_OP
    base = (rng.standard_normal((P, Cc, L)) * 1.3).astype(np.float32)
    pred = np.empty(((K + 1) * P, Cc, L), np.float32)
    for k in range(K + 1):          # conditions and the unconditional prediction are correlated, as a denoiser's are
        pred[k * P:(k + 1) * P] = (0.6 * base + 0.8 * rng.standard_normal((P, Cc, L)) * 1.3).astype(np.float32)
    lat = rng.standard_normal((P, Cc, L)).astype(np.float32)
    hist = rng.standard_normal((P, Cc, L)).astype(np.float32) if ms else None
    noise = None if ms else rng.standard_normal((P, Cc, L)).astype(np.float32)
    co1, co0 = mid_schedule_coef(1.0), mid_schedule_coef(0.0)
    params = np.zeros((P, 8), np.float32)
    settings = ((5.0, 0.75, co1, 0.05), (2.0, 0.0, co0, 0.4), (0.0, 0.4, co1, 0.0))
    for p in range(P):
        g, phi, co, ch = settings[p]
        params[p] = (g, phi) + tuple(co0 if ms else co) + (ch if ms else 0.0,)
    if P == 3:
        weights = np.array([w[:K] for w in W3], np.float32)
    else:
        weights = np.array([[1.0, 0.8, -0.5, 0.0, 0.3, -0.2, 0.0, 0.6][:K]], np.float32)
    assert ms or (params[0, 6] > 0 and (P < 2 or params[1, 6] == 0))
    return dict(pred=pred, lat=lat, hist=hist, noise=noise, params=params, weights=weights, lens=list(lens) if lens else [L] * P, K=K, ms=ms)


def poisoned(case):
    """A copy of the inputs with NaN wherever the operator must not read: rows of weight 0, padded frames of every input, the noise slice of a sigma = 0
    sample, the history of a c_hist = 0 sample, every row but c_0 of a sample without guidance."""
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    P, K = c['weights'].shape
    nan = np.float32(np.nan)
    for p in range(P):
        n = c['lens'][p]
        for k in range(K + 1):
            c['pred'][k * P + p, :, n:] = nan
        for t in ('lat', 'hist', 'noise'):
            if c[t] is not None:
                c[t][p, :, n:] = nan
        for k in range(1, K):
            if c['weights'][p, k] == 0:
                c['pred'][k * P + p] = nan
        if not c['params'][p, 0] > 0:
            for k in range(1, K + 1):
                c['pred'][k * P + p] = nan
        if c['noise'] is not None and c['params'][p, 6] == 0:
            c['noise'][p] = nan
        if c['hist'] is not None and c['params'][p, 7] == 0:
            c['hist'][p] = nan
    return c


def run_fp64(case):
    return step_fp64(case['pred'], case['lat'], case['hist'], case['noise'], case['params'], case['weights'], case['lens'])


def run_emul(case, mistake=None):
    return step_emul(case['pred'], case['lat'], case['hist'], case['noise'], case['params'], case['weights'], case['lens'], mistake=mistake)


OPERATOR_CASES = tuple((K, lens, ms) for K in (1, 2, 3) for lens in LENS_OP for ms in (False, True))
K8_CASES = ((8, None, False, 1), (8, (131,), True, 1))       # (K, lens, ms, P): every slot of the weight registers, two of them at weight 0


@functools.lru_cache(maxsize=None)
def operator_floor():
    """The emulation's largest distance from float64 over the operator cases of the GPU test (K 1, 2, 3 at P = 3, both length sets, both forms; K = 8 at
    P = 1): the floor its gate is a multiple of."""
    floor = 0.0
    for K, lens, ms, P in tuple(c + (3,) for c in OPERATOR_CASES) + K8_CASES:
        case = operator_case(K, lens, ms, P)
        floor = max(floor, distance(run_emul(case), run_fp64(case), case['lens'], with_hist=ms))
    return floor


def second_context(cfg, Lc, seed_in):
    """The second condition of the loop goldens (tools/mint_compose_golden.py): a context row drawn as oracle.weights.make_inputs draws one, from another
    seed, nine valid tokens.  Returns (ctx [1, Lc, Cctx], mask [1, Lc])."""
    from oracle.weights import make_inputs
    inp = make_inputs(cfg, B=2, L=8, Lc=Lc, n_valid=(9, 1), seed=seed_in + 1000)
    return inp['ctx'][0:1], inp['ctx_mask'][0:1]


def oracle_loop(denoise, texts, masks, uncond_text, uncond_mask, init, coefs, c_hist, timesteps, guidance_scale, guidance_rescale, weights, gt=None, gt_mask=None):
    """The numpy oracle's sampler loop with the float64 combination: one sample, K = len(texts) conditions in the batch [c_0 | .. | c_{K-1} | u];
    denoise(x, t, ctx, mask, gt, gt_mask) -> pred.  c_hist all zero: DDIM; scheduler.multistep_coefficients(): DPM-Solver++(2M).  Returns the final latent."""
    K = len(texts)
    lat = np.asarray(init, np.float32)
    hist = None
    rep = lambda a: None if a is None else np.concatenate([a] * (K + 1), 0)   # noqa: E731
    ctx, msk = np.concatenate(list(texts) + [uncond_text], 0), np.concatenate(list(masks) + [uncond_mask], 0)
    for i, t in enumerate(timesteps):
        out = denoise(rep(lat), int(t), ctx, msk, rep(gt), rep(gt_mask))
        sa, sb, cx0, cdir, sigma = (float(c) for c in coefs[i])
        assert sigma == 0.0
        x = lat.astype(np.float64)
        v = combine_fp64([out[k:k + 1] for k in range(K)], out[K:K + 1], weights, float(guidance_scale), float(guidance_rescale))
        x0, eps = sa * x - sb * v, sa * v + sb * x
        nxt = cx0 * x0 + cdir * eps
        if c_hist[i] != 0.0:
            nxt = nxt + c_hist[i] * (x0 - hist)
        hist = x0
        lat = nxt.astype(np.float32)
    if gt is not None:
        lat = np.where(np.asarray(gt_mask, bool), lat, np.asarray(gt, np.float32))
    return lat


GATE_FLOORS = 4       # the GPU gate: this many floors (the multiple the adaptive-projected-guidance groundwork used)


def check_outputs(got, hgot, case, ref=None, gate=None):
    """What the GPU operator tests assert of the latents `got` and the history `hgot` (None for the DDIM form) that came back for `case`: every value
    finite, every sample within `gate` (default GATE_FLOORS floors) of float64 on its valid frames, padded frames exactly 0.  Returns the distances."""
    ref = ref or run_fp64(case)
    gate = GATE_FLOORS * operator_floor() if gate is None else gate
    outs = [(got, ref[0], 'latents')] + ([(hgot, ref[1], 'x0_hist')] if case['ms'] else [])
    dists = {}
    for g, r, name in outs:
        assert np.isfinite(g).all(), f'{name}: a value is not finite'
        for p, n in enumerate(case['lens']):
            e = rel_l2(g[p, :, :n], r[p, :, :n])
            dists[(name, p)] = e
            assert e < gate, (name, p, e, gate)
            assert not g[p, :, n:].any(), f'{name}: padded frames of sample {p} must be exactly 0'
    return dists
