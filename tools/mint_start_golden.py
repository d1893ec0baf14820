"""Mint the golden of sampler runs that START AT STEP k from a noised clip (tests/test_start_gpu.py): tests/golden/sampler_start_xs.npz.

    python tools/mint_start_golden.py [--out tests/golden]

The reference never starts anywhere but pure noise, so this is NOT a run of the reference: it is the numpy oracle's denoiser (oracle.dit.DiTOracle, fp32)
inside the loop of tools/mint_multistep_golden.py -- oracle.sampler's cfg_combine and rescale_noise_cfg, the DDIM / 2M update in float64 -- run over
timesteps[k:] from

    x_k = sa_k ((clean + shift) scale) + sb_k init        (sa_k, sb_k) = sqrt(alpha_bar), sqrt(1 - alpha_bar) of step k

for k = 1, 7, 19, once with the DDIM update and once with the 2M update whose c_hist_k is 0 (the run's first step is first-order and has no history), the
later steps taking the call's c_hist.  Inputs, weights and settings are those of the eta = 0 fixture `sampler_smp_xs_e0` (xs, L 96, 20 steps, guidance 3.5,
editing with gt / gt_mask); `clean` is uniform_pm1('start.clean') in VAE space with scale 0.5 and shift -0.3.  k = 19 runs the last step only, where
a_prev = 1 and c_hist = 0.  The tool first reproduces the base golden with k = 0 through the same code and prints the distance.  CPU only.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BASE = 'smp_xs_e0'
STARTS = (1, 7, 19)
SCALE, SHIFT = 0.5, -0.3


def clean_latent(meta, C):
    from oracle.weights import uniform_pm1
    return (1.5 * uniform_pm1('start.clean', C * meta['L'], meta['seed_in'])).reshape(1, C, meta['L']).astype(np.float32)


def noised(clean, init, sa, sb, scale=SCALE, shift=SHIFT):
    return (sa * ((clean.astype(np.float64) + shift) * scale) + sb * init.astype(np.float64)).astype(np.float32)


def main():
    from ezaudio_amd.scheduler import DDIMScheduler
    from oracle.dit import DiTOracle
    from tests.util import DIFF, sampler_case
    from tools.mint_multistep_golden import multistep_loop
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='tests/golden')
    a = ap.parse_args()
    cfg, sd, inp, init, noises, g, meta = sampler_case(BASE)
    assert meta['eta'] == 0.0
    o = DiTOracle(cfg, sd)

    def denoise(x, t, ctx, msk, gt, gm):
        return o.forward(x, t, ctx, msk, gt=gt, mae_mask_infer=gm)[0]
    sch = DDIMScheduler(**DIFF)
    K = meta['steps']
    sch.set_timesteps(K)
    gt = inp['gt'][0:1] if meta['with_gt'] else None
    gm = inp['gt_mask'][0:1] if meta['with_gt'] else None
    ts = [int(t) for t in sch.timesteps]
    coefs, ch = sch.ddim_coefficients(0), sch.multistep_coefficients()
    rel = lambda x, y: float(np.linalg.norm(x.astype(np.float64) - y) / np.linalg.norm(y.astype(np.float64)))   # noqa: E731

    def run(k, x_k, c_hist):
        return multistep_loop(denoise, inp['ctx'][0:1], inp['ctx_mask'][0:1], inp['ctx'][1:2], inp['ctx_mask'][1:2], x_k, coefs[k:], c_hist[k:],
                              timesteps=ts[k:], guidance_scale=meta['guidance_scale'], guidance_rescale=meta['guidance_rescale'], gt=gt, gt_mask=gm)
    base = run(0, init, [0.0] * K)
    print(f'k = 0 through this loop vs the reference golden {BASE}: rel-L2 {rel(base, g["latent"]):.3e}')
    assert rel(base, g['latent']) < 2e-4     # tests/test_oracle.py's gate
    clean = clean_latent(meta, cfg['out_chans'])
    out = {}
    for k in STARTS:
        x_k = noised(clean, init, coefs[k][0], coefs[k][1])
        ms = list(ch)
        ms[k] = 0.0
        out[f'ddim_{k}'] = run(k, x_k, [0.0] * K).astype(np.float32)
        out[f'ms_{k}'] = run(k, x_k, ms).astype(np.float32)
        print(f'start {k}: (sa, sb) = ({coefs[k][0]:.6f}, {coefs[k][1]:.6f}); DDIM vs the k = 0 run {rel(out[f"ddim_{k}"], base):.3e}; '
              f'2M vs DDIM {rel(out[f"ms_{k}"], out[f"ddim_{k}"]):.3e}')
    m = dict(base=BASE, starts=list(STARTS), scale=SCALE, shift=SHIFT, size=meta['size'], L=meta['L'], Lc=meta['Lc'], steps=K, seed_w=meta['seed_w'],
             seed_in=meta['seed_in'], guidance_scale=meta['guidance_scale'], guidance_rescale=meta['guidance_rescale'], eta=0.0, with_gt=meta['with_gt'])
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, 'sampler_start_xs.npz')
    np.savez_compressed(path, meta=np.array(repr(m)), **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
