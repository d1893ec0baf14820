"""Mint the golden of the DPM-Solver++(2M) sampler loop (tests/test_multistep_gpu.py): tests/golden/sampler_ms_xs.npz.

    python tools/mint_multistep_golden.py [--out tests/golden]

The reference has no such solver, so this is NOT a run of the reference: it is the numpy oracle's denoiser (oracle.dit.DiTOracle, fp32, itself gated
against the reference goldens) inside the loop of oracle/sampler.py -- cfg_combine, rescale_noise_cfg -- with the update

    x0 = sa x - sb v,  eps = sa v + sb x,  x_next = c_x0 x0 + c_dir eps + c_hist_i (x0 - x0 of the step before)

evaluated in float64 per step from ezaudio_amd.scheduler's `ddim_coefficients(0)` and `multistep_coefficients()`.  Inputs, weights and settings are those
of the existing eta = 0 fixture `sampler_smp_xs_e0` (xs, L 96, 20 steps, guidance 3.5, editing with gt / gt_mask).  CPU only, a few seconds.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BASE = 'smp_xs_e0'


def multistep_loop(denoise, text, text_mask, uncond_text, uncond_mask, init, coefs, c_hist, timesteps, guidance_scale, guidance_rescale, gt=None,
                   gt_mask=None):
    """One prompt, batch 1: oracle/sampler.py `sample` with the 2M update in place of the scheduler's step."""
    from oracle.sampler import cfg_combine, rescale_noise_cfg
    lat = np.asarray(init, np.float32)
    hist = None
    for i, t in enumerate(timesteps):
        if guidance_scale:
            cat = lambda a: None if a is None else np.concatenate([a, a], 0)   # noqa: E731
            out = denoise(cat(lat), int(t), np.concatenate([text, uncond_text], 0), np.concatenate([text_mask, uncond_mask], 0), cat(gt), cat(gt_mask))
            v = cfg_combine(out[:1], out[1:], guidance_scale)
            if guidance_rescale > 0.0:
                v = rescale_noise_cfg(v, out[:1], guidance_rescale)
        else:
            v = denoise(lat, int(t), text, text_mask, gt, gt_mask)
        sa, sb, cx0, cdir, sigma = (float(c) for c in coefs[i])
        assert sigma == 0.0
        x, v = lat.astype(np.float64), v.astype(np.float64)
        x0, eps = sa * x - sb * v, sa * v + sb * x
        nxt = cx0 * x0 + cdir * eps
        if c_hist[i] != 0.0:
            nxt = nxt + c_hist[i] * (x0 - hist)
        hist = x0
        lat = nxt.astype(np.float32)
    if gt is not None:
        lat = np.where(np.asarray(gt_mask, bool), lat, np.asarray(gt, np.float32))
    return lat


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
    sch.set_timesteps(meta['steps'])
    gt = inp['gt'][0:1] if meta['with_gt'] else None
    gm = inp['gt_mask'][0:1] if meta['with_gt'] else None
    ch = sch.multistep_coefficients()
    args = (denoise, inp['ctx'][0:1], inp['ctx_mask'][0:1], inp['ctx'][1:2], inp['ctx_mask'][1:2], init, sch.ddim_coefficients(0))
    kw = dict(timesteps=[int(t) for t in sch.timesteps], guidance_scale=meta['guidance_scale'], guidance_rescale=meta['guidance_rescale'], gt=gt, gt_mask=gm)
    lat = multistep_loop(*args, ch, **kw)
    ddim = multistep_loop(*args, [0.0] * len(ch), **kw)
    rel = lambda x, y: float(np.linalg.norm(x.astype(np.float64) - y) / np.linalg.norm(y.astype(np.float64)))   # noqa: E731
    print(f'c_hist = 0 through this loop vs the reference golden {BASE}: rel-L2 {rel(ddim, g["latent"]):.3e}')
    print(f'2M vs DDIM on the same inputs: rel-L2 {rel(lat, ddim):.3e}')
    assert rel(ddim, g['latent']) < 2e-4     # the loop itself is the reference's when the new term is off (tests/test_oracle.py's gate)
    m = dict(base=BASE, solver='dpmpp_2m', size=meta['size'], L=meta['L'], Lc=meta['Lc'], steps=meta['steps'], seed_w=meta['seed_w'], seed_in=meta['seed_in'],
             guidance_scale=meta['guidance_scale'], guidance_rescale=meta['guidance_rescale'], eta=0.0, with_gt=meta['with_gt'])
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, 'sampler_ms_xs.npz')
    np.savez_compressed(path, latent=lat.astype(np.float32), c_hist=np.asarray(ch, np.float64), meta=np.array(repr(m)))
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
