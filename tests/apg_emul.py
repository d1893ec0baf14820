"""Adaptive projected guidance (Sadat et al., "Eliminating Oversaturation and Artifacts of High Guidance Scales in Diffusion Models") as a per-sample update
of the sampler step: the definition in float64, an fp32 emulation that follows the order of operations of a two-pass row kernel (k_cfg_stats / k_cfg_apply
style: 64 chunked partial sums in fp32, the final reduction in double), nine deliberate mistakes built into copies of that emulation, and operator inputs for
CPU and GPU tests to share.  numpy only; groundwork -- no kernel implements the update yet.

    x0c = sa x - sb c          x0u = sa x - sb u
    d   = (x0c - x0u) + beta_eff m          ; m <- d  (stored BEFORE the norm cap)
    s   = min(1, r / |d|)  if r > 0 and |d| > 0, else 1
    a   = s <d, x0c> / |x0c|^2              (0 when |x0c|^2 = 0)
    U   = s d - (1 - eta_apg) a x0c         (= orthogonal part + eta_apg * parallel part)
    x0  = x0c + (w - 1) U ;  v = c - (w - 1) U / sb ;  eps = sa v + sb x
    x_next = c_x0 x0 + c_dir eps (+ c_hist (x0 - x0_hist), x0_hist <- x0 with the multistep solver)

A row of `params`: (w, guidance_rescale, sa, sb, c_x0, c_dir, sigma, c_hist, eta_apg, norm_threshold, beta_eff, on).
"""
import numpy as np

NB, WG = 64, 256      # the statistics pass of the sampler tail: 64 workgroups of 256 threads per sample, element i belongs to workgroup (i // 256) % 64

MISTAKES = ('norm_over_padding', 'm_after_cap', 'project_on_x0u', 'project_on_c', 'w_not_w_minus_1', 'eta_on_orthogonal', 'cap_norm_squared',
            'm_read_first_step', 'sb_sign')


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def apg_fp64(c, u, x, m, sa, sb, w, eta, r, beta):
    """The definition, float64, on one sample's valid elements (any shape).  m may be None when beta == 0.  Returns (x0, v, d, info) with info = (|d|, s, a)."""
    c, u, x = (np.asarray(t, np.float64) for t in (c, u, x))
    x0c, x0u = sa * x - sb * c, sa * x - sb * u
    d = x0c - x0u
    if beta != 0:
        d = d + beta * np.asarray(m, np.float64)
    nd = float(np.sqrt((d * d).sum()))
    s = min(1.0, r / nd) if (r > 0 and nd > 0) else 1.0
    cc = float((x0c * x0c).sum())
    a = s * float((d * x0c).sum()) / cc if cc > 0 else 0.0
    U = s * d - (1.0 - eta) * a * x0c
    x0 = x0c + (w - 1.0) * U
    v = c - (w - 1.0) * U / sb
    return x0, v, d, (nd, s, a)


def step_fp64(pred, lat, hist, mom, params, lens):
    """One call of the operator in float64: (latents, x0_hist, momentum) [P, C, L], zero on padded frames; a sample without APG takes CFG + rescale, one
    without guidance its conditional prediction, and keeps its momentum rows as they were."""
    P = lat.shape[0]
    out, hout = np.zeros(lat.shape, np.float64), np.zeros(lat.shape, np.float64)
    mout = np.array(mom, np.float64)
    for p in range(P):
        w, phi, sa, sb, cx0, cdir, _, ch, eta, r, beta, on = (float(t) for t in params[p])
        n = lens[p]
        c, x = pred[p, :, :n].astype(np.float64), lat[p, :, :n].astype(np.float64)
        if w > 0 and on != 0:
            x0, v, d, _ = apg_fp64(c, pred[P + p, :, :n], x, mom[p, :, :n], sa, sb, w, eta, r, beta)
            mout[p] = 0.0
            mout[p, :, :n] = d
        else:
            v = c
            if w > 0:
                u = pred[P + p, :, :n].astype(np.float64)
                v = u + w * (c - u)
                if phi > 0:
                    v = phi * (v * (c.std(ddof=1) / v.std(ddof=1))) + (1 - phi) * v
            x0 = sa * x - sb * v
        eps = sa * v + sb * x
        prev = cx0 * x0 + cdir * eps
        if ch != 0:
            prev = prev + ch * (x0 - hist[p, :, :n].astype(np.float64))
        out[p, :, :n], hout[p, :, :n] = prev, x0
    return out, hout, mout


def _partials(vals, idx):
    """The 64 fp32 partial sums of the statistics pass (vals fp32 over the flat elements idx of the sample), then their sum in double in the fixed order."""
    blk = (idx // WG) % NB
    tot = 0.0
    for b in range(NB):
        tot += float(np.sum(vals[blk == b], dtype=np.float32))
    return tot


def step_emul(pred, lat, hist, mom, params, lens, mistake=None, first_momentum=-0.5):
    """The operator as the kernels compute it: every element-wise expression in fp32, 64 chunked partial sums in fp32, their reduction and s, a in double.
    `mistake` (one of MISTAKES) builds that error in.  'norm_over_padding' reads the padded frames, so they must hold finite numbers for it;
    'm_read_first_step' applies `first_momentum` where beta_eff is 0."""
    assert mistake is None or mistake in MISTAKES
    f = np.float32
    P, Cc, L = lat.shape
    out, hout = np.zeros(lat.shape, f), np.zeros(lat.shape, f)
    mout = np.array(mom, f)
    flat = np.arange(Cc * L).reshape(Cc, L)
    for p in range(P):
        w, phi, sa, sb, cx0, cdir, _, ch, eta, r, beta, on = (f(t) for t in params[p])
        n = lens[p]
        c, x = pred[p, :, :n].astype(f), lat[p, :, :n].astype(f)
        if w > 0 and on != 0:
            if mistake == 'm_read_first_step' and beta == 0:
                beta = f(first_momentum)
            ns = L if mistake == 'norm_over_padding' else n       # the frames the sums run over
            cs, us, xs = pred[p, :, :ns].astype(f), pred[P + p, :, :ns].astype(f), lat[p, :, :ns].astype(f)
            x0c_s = sa * xs - sb * cs
            d_s = sb * (us - cs)
            if beta != 0:
                d_s = d_s + beta * mom[p, :, :ns].astype(f)
            proj_s = {'project_on_x0u': sa * xs - sb * us, 'project_on_c': cs}.get(mistake, x0c_s)
            idx = flat[:, :ns].ravel()
            dd = _partials((d_s * d_s).ravel(), idx)
            dc = _partials((d_s * proj_s).ravel(), idx)
            cc = _partials((proj_s * proj_s).ravel(), idx)
            nrm = dd if mistake == 'cap_norm_squared' else np.sqrt(dd)
            s = min(1.0, float(r) / nrm) if (r > 0 and dd > 0) else 1.0
            a_s = f(s)
            a_k = f((1.0 - float(eta)) * s * dc / cc) if cc > 0 else f(0)
            x0c, d, proj = x0c_s[:, :n], d_s[:, :n], proj_s[:, :n]
            mout[p] = 0
            mout[p, :, :n] = a_s * d if mistake == 'm_after_cap' else d
            if mistake == 'eta_on_orthogonal':     # eta_apg on the orthogonal part, the parallel one kept whole
                par = f(s * dc / cc) * proj
                U = eta * (a_s * d - par) + par
            else:
                U = a_s * d - a_k * proj
            g = w if mistake == 'w_not_w_minus_1' else w - f(1)
            x0 = x0c + g * U
            v = c + (g / sb) * U if mistake == 'sb_sign' else c - (g / sb) * U
        else:
            v = c
            if w > 0:
                u = pred[P + p, :, :n].astype(f)
                v = u + w * (c - u)
                if phi > 0:
                    ratio = f(np.sqrt(np.float64(c.astype(np.float64).var(ddof=1))) / np.sqrt(np.float64(v.astype(np.float64).var(ddof=1))))
                    v = phi * (v * ratio) + (f(1) - phi) * v
            x0 = sa * x - sb * v
        eps = sa * v + sb * x
        prev = cx0 * x0 + cdir * eps
        if ch != 0:
            prev = prev + ch * (x0 - hist[p, :, :n].astype(f))
        out[p, :, :n], hout[p, :, :n] = prev, x0
    return out, hout, mout


def distance(got, ref, lens, samples=None):
    """The largest rel-L2 over the three outputs (latents, x0_hist, momentum) and the samples, each on the sample's valid frames."""
    worst = 0.0
    for g, r in zip(got, ref):
        for p, n in enumerate(lens):
            if samples is not None and p not in samples:
                continue
            if np.linalg.norm(np.asarray(r[p, :, :n], np.float64)) == 0:
                continue
            worst = max(worst, rel_l2(g[p, :, :n], r[p, :, :n]))
    return worst


def operator_case(L, lens, coef, seed=None):
    """The operator inputs of tests/test_apg_host.py (and of a GPU test of the operator, once there is one): P = 3, C = 128, n = 128 L.  `coef` is (sa, sb, c_x0, c_dir, sigma) of a
    mid-schedule step (at step 0 x0c = -c: projecting onto c would be no mistake).
      sample 0  APG, w 5, eta_apg 0, momentum -0.5 applied, the cap at half the measured |d| (it bites), c_hist 0.05
      sample 1  APG, w 2, eta_apg 1, no cap, beta_eff 0 (its momentum rows are not read), c_hist 0.4
      sample 2  no guidance, c_hist 0
    All inputs finite everywhere (a GPU test poisons what must not be read).  Returns (pred [6, C, L], lat, hist, mom [3, C, L], params [3, 12], lens)."""
    P, Cc = 3, 128
    rng = np.random.default_rng(7100 + L if seed is None else seed)
    pred = (rng.standard_normal((2 * P, Cc, L)) * 1.3).astype(np.float32)
    pred[P:] = (0.6 * pred[:P] + 0.8 * pred[P:]).astype(np.float32)          # conditional and unconditional predictions are correlated, as a denoiser's are
    lat = rng.standard_normal((P, Cc, L)).astype(np.float32)
    hist = rng.standard_normal((P, Cc, L)).astype(np.float32)
    mom = (0.5 * rng.standard_normal((P, Cc, L))).astype(np.float32)
    ln = list(lens) if lens else [L] * P
    sa, sb = float(coef[0]), float(coef[1])
    _, _, _, (nd, _, _) = apg_fp64(pred[0, :, :ln[0]], pred[P, :, :ln[0]], lat[0, :, :ln[0]], mom[0, :, :ln[0]], sa, sb, 5.0, 0.0, 0.0, -0.5)
    params = np.zeros((P, 12), np.float32)
    params[0] = (5.0, 0.0) + tuple(coef) + (0.05, 0.0, 0.5 * nd, -0.5, 1.0)
    params[1] = (2.0, 0.0) + tuple(coef) + (0.4, 1.0, 0.0, 0.0, 1.0)
    params[2] = (0.0, 0.4) + tuple(coef) + (0.0, 0.0, 0.0, 0.0, 0.0)
    assert params[0, 6] == 0.0
    return pred, lat, hist, mom, params, ln


def floor_and_mistakes(case):
    """(floor, {mistake: distance}) on the inputs `case` (operator_case): the emulation's largest distance from float64, and each mistake's.  A mistake
    that cannot show on these inputs is left out: norms over padded frames when no padded sample uses its sums (an APG sample with eta_apg 1 and no cap
    is independent of them)."""
    pred, lat, hist, mom, params, ln = case
    ref = step_fp64(pred, lat, hist, mom, params, ln)
    floor = distance(step_emul(pred, lat, hist, mom, params, ln), ref, ln)
    padded = any(n < lat.shape[2] and q[0] > 0 and q[11] != 0 and (q[8] != 1 or q[9] > 0) for n, q in zip(ln, params))
    far = {}
    for mk in MISTAKES:
        if mk == 'norm_over_padding' and not padded:
            continue
        far[mk] = distance(step_emul(pred, lat, hist, mom, params, ln, mistake=mk), ref, ln)
    return floor, far
