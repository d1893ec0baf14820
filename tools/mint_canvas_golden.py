"""Mint the golden of long-form canvas runs (tests/test_canvas_gpu.py): tests/golden/sampler_canvas_xs.npz.

    python tools/mint_canvas_golden.py [--out tests/golden]

The reference samples one row of the trained length, so this is NOT a run of the reference: it is the numpy oracle's denoiser (oracle.dit.DiTOracle, fp32)
inside the loop of tools/mint_multistep_golden.py -- oracle.sampler's cfg_combine and rescale_noise_cfg per window, the DDIM / 2M update in float64 -- over P
windows of one canvas, followed at every step by the blend in float64:

    canvas frame j held by the windows p with off[p] <= j < off[p] + L, local frame r = j - off[p], w(r) = min(r + 1, L - r, ramp)
    v = sum_p w_p x_p / sum_p w_p    written into every holder, where two or more windows hold j

Inputs, weights and settings are those of the eta = 0 fixture `sampler_smp_xs_e0` (xs, L 96, 20 steps, guidance 3.5) WITHOUT gt / gt_mask, every window under
the fixture's one prompt.  The canvas init noise is sqrt(3) uniform_pm1('canvas.init'), the step noise of the eta = 1 case sqrt(3) uniform_pm1('canvas.z<i>'),
each [1, C, T]; window p takes the slice [off[p], off[p] + L).  Stored are the final canvases [1, C, T] (the lowest window wins; the holders agree anyway).

Cases:  a  offsets [0, 52, 104], T 200, ramp 44 (the overlap: a linear cross-fade), DDIM eta 0
        b  the same with the 2M update (the history of data predictions stays per window, unblended)
        c  offsets [0, 30, 60], T 156, ramp 1 (the plain mean), DDIM eta 1; frames 60 .. 95 are held by all three windows

The tool first reproduces the base golden (one window, with the fixture's gt) through the same loop and prints the distance, then runs every case without
the blend as well and prints rel-L2 between the blended and the unblended canvas: what separates the feature from its absence, against the 2e-2 gate of the
GPU test.  The target was 10 x the gate (0.2).  It is NOT reached at this width: a 0.088, b 0.087, c 0.079 -- four times the gate, twenty times the 4.4e-3
the fused loop measures on this fixture -- and no placement of three windows under one prompt on shared noise gets there (tried at eta 0: [0, 30, 60] with
ramp 30 and 66: 0.098; [0, 48, 96] ramp 48: 0.087; [0, 24, 48] ramp 24: 0.091; [0, 52, 104] ramp 1: 0.075): the xs model with random weights moves a window's
frames by about 0.12 when its neighbours change, whatever the overlap.  The issue's offsets are therefore kept, the figures are stored in the file's meta, and
the tool ends with status 1 after writing to say that the target was missed.  CPU only.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BASE = 'smp_xs_e0'
CASES = (dict(key='a', offsets=[0, 52, 104], T=200, ramp=44, eta=0.0, solver='ddim'),
         dict(key='b', offsets=[0, 52, 104], T=200, ramp=44, eta=0.0, solver='dpmpp_2m'),
         dict(key='c', offsets=[0, 30, 60], T=156, ramp=1, eta=1.0, solver='ddim'))
GATE = 2e-2


def canvas_noise(key, C, T, seed):
    from oracle.weights import uniform_pm1
    return (uniform_pm1(key, C * T, seed) * np.float32(np.sqrt(3.0))).reshape(1, C, T)


def blend(wins, offsets, T, ramp):
    """wins float32 [P][1][C][L] -> the same after one blend (float64 arithmetic, holders in ascending p)."""
    P, L = len(wins), wins[0].shape[-1]
    r = np.arange(L)
    w = np.minimum(np.minimum(r + 1, L - r), ramp).astype(np.float64)
    num = np.zeros(wins[0].shape[:-1] + (T,), np.float64)
    den, cnt = np.zeros(T, np.float64), np.zeros(T, np.int64)
    for p in range(P):
        sl = slice(offsets[p], offsets[p] + L)
        num[..., sl] += w * wins[p].astype(np.float64)
        den[sl] += w
        cnt[sl] += 1
    v = (num / den).astype(np.float32)
    out = []
    for p in range(P):
        sl = slice(offsets[p], offsets[p] + L)
        out.append(np.where(cnt[sl] >= 2, v[..., sl], wins[p]))
    return out


def assemble(wins, offsets, T):
    L = wins[0].shape[-1]
    out = np.zeros(wins[0].shape[:-1] + (T,), np.float32)
    for p in reversed(range(len(wins))):
        out[..., offsets[p]:offsets[p] + L] = wins[p]
    return out


def canvas_loop(denoise, text, text_mask, uncond_text, uncond_mask, init_canvas, offsets, L, ramp, coefs, c_hist, timesteps, guidance_scale,
                guidance_rescale, step_noises=None, gt=None, gt_mask=None):
    """tools/mint_multistep_golden.py multistep_loop over the windows of a canvas; ramp None = no blend (independent windows on sliced noise)."""
    from oracle.sampler import cfg_combine, rescale_noise_cfg
    T = init_canvas.shape[-1]
    cut = lambda a: [np.asarray(a[..., o:o + L], np.float32) for o in offsets]   # noqa: E731
    wins = cut(init_canvas)
    hist = [None] * len(offsets)
    cat = lambda a: None if a is None else np.concatenate([a, a], 0)   # noqa: E731
    for i, t in enumerate(timesteps):
        sa, sb, cx0, cdir, sigma = (float(c) for c in coefs[i])
        z = None if sigma == 0.0 else cut(step_noises[i])
        for p, lat in enumerate(wins):
            out = denoise(cat(lat), int(t), np.concatenate([text, uncond_text], 0), np.concatenate([text_mask, uncond_mask], 0), cat(gt), cat(gt_mask))
            v = cfg_combine(out[:1], out[1:], guidance_scale)
            if guidance_rescale > 0.0:
                v = rescale_noise_cfg(v, out[:1], guidance_rescale)
            x, v = lat.astype(np.float64), v.astype(np.float64)
            x0, eps = sa * x - sb * v, sa * v + sb * x
            nxt = cx0 * x0 + cdir * eps
            if sigma != 0.0:
                nxt = nxt + sigma * z[p].astype(np.float64)
            if c_hist[i] != 0.0:
                nxt = nxt + c_hist[i] * (x0 - hist[p])
            hist[p] = x0
            wins[p] = nxt.astype(np.float32)
        if ramp is not None and len(offsets) > 1:
            wins = blend(wins, offsets, T, ramp)
    if gt is not None:
        wins = [np.where(np.asarray(gt_mask, bool), w, np.asarray(gt, np.float32)) for w in wins]
    return assemble(wins, offsets, T)


def main():
    from ezaudio_amd.scheduler import DDIMScheduler
    from oracle.dit import DiTOracle
    from tests.util import DIFF, sampler_case
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='tests/golden')
    a = ap.parse_args()
    cfg, sd, inp, init, noises, g, meta = sampler_case(BASE)
    assert meta['eta'] == 0.0
    o = DiTOracle(cfg, sd)

    def denoise(x, t, ctx, msk, gt, gm):
        return o.forward(x, t, ctx, msk, gt=gt, mae_mask_infer=gm)[0]
    sch = DDIMScheduler(**DIFF)
    K, L, C = meta['steps'], meta['L'], cfg['out_chans']
    sch.set_timesteps(K)
    ts = [int(t) for t in sch.timesteps]
    rel = lambda x, y: float(np.linalg.norm(x.astype(np.float64) - y) / np.linalg.norm(y.astype(np.float64)))   # noqa: E731
    prompt = (inp['ctx'][0:1], inp['ctx_mask'][0:1], inp['ctx'][1:2], inp['ctx_mask'][1:2])
    kw = dict(timesteps=ts, guidance_scale=meta['guidance_scale'], guidance_rescale=meta['guidance_rescale'])
    base = canvas_loop(denoise, *prompt, init, [0], L, 1, sch.ddim_coefficients(0), [0.0] * K, gt=inp['gt'][0:1], gt_mask=inp['gt_mask'][0:1], **kw)
    print(f'one window through this loop vs the reference golden {BASE}: rel-L2 {rel(base, g["latent"]):.3e}')
    assert rel(base, g['latent']) < 2e-4     # tests/test_oracle.py's gate
    out, cases, short = {}, [], False
    for c in CASES:
        T = c['T']
        assert c['offsets'][-1] + L == T
        noise0 = canvas_noise('canvas.init', C, T, meta['seed_in'])
        zs = [canvas_noise(f'canvas.z{i}', C, T, meta['seed_in']) for i in range(K)] if c['eta'] > 0 else None
        ch = sch.multistep_coefficients() if c['solver'] == 'dpmpp_2m' else [0.0] * K
        args = (denoise, *prompt, noise0, c['offsets'], L)
        rest = (sch.ddim_coefficients(c['eta']), ch)
        on = canvas_loop(*args, c['ramp'], *rest, step_noises=zs, **kw)
        off = canvas_loop(*args, None, *rest, step_noises=zs, **kw)
        d = rel(on, off)
        print(f"case {c['key']} offsets {c['offsets']} T {T} ramp {c['ramp']} eta {c['eta']} {c['solver']}: blended vs unblended canvas rel-L2 {d:.3e}")
        assert np.isfinite(on).all() and d > GATE
        short = short or d < 10 * GATE
        out['canvas_' + c['key']] = on.astype(np.float32)
        cases.append(dict(c, unblended_rel_l2=d))
    m = dict(base=BASE, cases=cases, size=meta['size'], L=L, Lc=meta['Lc'], steps=K, seed_w=meta['seed_w'], seed_in=meta['seed_in'],
             guidance_scale=meta['guidance_scale'], guidance_rescale=meta['guidance_rescale'], with_gt=False)
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, 'sampler_canvas_xs.npz')
    np.savez_compressed(path, meta=np.array(repr(m)), **out)
    print('wrote', path, os.path.getsize(path), 'bytes')
    if short:
        print(f'blended vs unblended below the target of 10 x the gate = {10 * GATE:g} (see the docstring)')
        sys.exit(1)


if __name__ == '__main__':
    main()
