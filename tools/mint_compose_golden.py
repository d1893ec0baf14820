"""Mint the goldens of the composed-guidance sampler loop (tests/test_compose_host.py, tests/test_compose_gpu.py): tests/golden/sampler_compose_xs.npz.

    python tools/mint_compose_golden.py [--out tests/golden]

The reference has no composed guidance, so this is NOT a run of the reference: it is the numpy oracle's denoiser (oracle.dit.DiTOracle, fp32, itself gated
against the reference goldens) inside the loop of oracle/sampler.py (tests/compose_emul.py `oracle_loop`), with the combination `combine_fp64` ( d = sum_k w_k (c_k - u),
v = u + g d, the rescale against the primary condition) evaluated in float64 per step in place of cfg_combine + rescale_noise_cfg, then the DDIM expression
-- or, for the second golden, DPM-Solver++(2M)'s -- from ezaudio_amd.scheduler's coefficients.  Inputs, weights and settings are those of the eta = 0 fixture
`sampler_smp_xs_e0` (xs, L 96, 20 steps, guidance 3.5 with its rescale, editing with gt / gt_mask); K = 2, the second context drawn as make_inputs draws one
(tests/compose_emul.py second_context).

The second weight is chosen here: the smallest of 0.25, 0.5, 0.75, 1, 1.5, 2, 3 for which BOTH goldens lie at least 10 gates (10 x 2e-2, the loop gate of
tests/test_multistep_gpu.py) from the plain-CFG loop of the same inputs -- otherwise the test could not tell composition from CFG.  The distances go into the
metadata.  CPU only, seconds.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BASE = 'smp_xs_e0'
GATE = 2e-2
CANDIDATES = (0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0)


def main():
    from ezaudio_amd.scheduler import DDIMScheduler
    from oracle.dit import DiTOracle
    from tests.compose_emul import oracle_loop as compose_loop, second_context
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
    n = meta['steps']
    gt = inp['gt'][0:1] if meta['with_gt'] else None
    gm = inp['gt_mask'][0:1] if meta['with_gt'] else None
    ch = sch.multistep_coefficients()
    ctx2, msk2 = second_context(cfg, meta['Lc'], meta['seed_in'])
    one = ([inp['ctx'][0:1]], [inp['ctx_mask'][0:1]])
    two = ([inp['ctx'][0:1], ctx2], [inp['ctx_mask'][0:1], msk2])
    tail = (inp['ctx'][1:2], inp['ctx_mask'][1:2], init, sch.ddim_coefficients(0))
    kw = dict(timesteps=[int(t) for t in sch.timesteps], guidance_scale=meta['guidance_scale'], guidance_rescale=meta['guidance_rescale'], gt=gt, gt_mask=gm)
    rel = lambda x, y: float(np.linalg.norm(x.astype(np.float64) - y) / np.linalg.norm(y.astype(np.float64)))   # noqa: E731
    cfg_ddim = compose_loop(denoise, *one, *tail, [0.0] * n, weights=[1.0], **kw)
    cfg_2m = compose_loop(denoise, *one, *tail, ch, weights=[1.0], **kw)
    # K = 1 with weight 1 is the fixture's own loop: this loop adds nothing of its own (the fixture's golden is the oracle's fp32 loop)
    print(f'K = 1, w = 1 vs the golden of {BASE}: rel-L2 {rel(cfg_ddim, g["latent"]):.3e}')
    assert rel(cfg_ddim, g['latent']) < 1e-4      # (fp64 against fp32 combination through 20 steps; measured 5e-7)
    # ... and a second condition at weight 0 changes nothing
    assert np.array_equal(compose_loop(denoise, *two, *tail, [0.0] * n, weights=[1.0, 0.0], **kw), cfg_ddim)
    for w2 in CANDIDATES:
        lat_ddim = compose_loop(denoise, *two, *tail, [0.0] * n, weights=[1.0, w2], **kw)
        lat_2m = compose_loop(denoise, *two, *tail, ch, weights=[1.0, w2], **kw)
        d1, d2 = rel(lat_ddim, cfg_ddim), rel(lat_2m, cfg_2m)
        print(f'w_1 = {w2}: composed vs plain CFG rel-L2 DDIM {d1:.3e} = {d1 / GATE:.1f} gates, dpmpp_2m {d2:.3e} = {d2 / GATE:.1f} gates')
        if min(d1, d2) >= 10 * GATE:
            break
    else:
        raise SystemExit('no candidate weight separates composition from CFG by 10 gates')
    m = dict(base=BASE, size=meta['size'], L=meta['L'], Lc=meta['Lc'], steps=n, seed_w=meta['seed_w'], seed_in=meta['seed_in'],
             guidance_scale=meta['guidance_scale'], guidance_rescale=meta['guidance_rescale'], eta=0.0, with_gt=meta['with_gt'], K=2, weights=[1.0, w2],
             dist_ddim=d1, dist_2m=d2)
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, 'sampler_compose_xs.npz')
    np.savez_compressed(path, latent_ddim=lat_ddim.astype(np.float32), latent_2m=lat_2m.astype(np.float32), meta=np.array(repr(m)))
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
