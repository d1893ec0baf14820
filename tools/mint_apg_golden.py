"""Mint the goldens of the adaptive-projected-guidance sampler loop (tests/test_apg_host.py; groundwork for a GPU test of a fused APG step):
tests/golden/sampler_apg_xs.npz.

    python tools/mint_apg_golden.py [--out tests/golden]

The reference has no APG, so this is NOT a run of the reference: it is the numpy oracle's denoiser (oracle.dit.DiTOracle, fp32, itself gated against the
reference goldens) inside the loop of oracle/sampler.py, with the APG update of tests/apg_emul.py (`apg_fp64`)
evaluated in float64 per step in place of cfg_combine + rescale_noise_cfg, then the DDIM expression -- or, for the second golden, DPM-Solver++(2M)'s -- from
ezaudio_amd.scheduler's coefficients.  Inputs, weights and settings are those of the eta = 0 fixture `sampler_smp_xs_e0` (xs, L 96, 20 steps, guidance 3.5,
editing with gt / gt_mask) with the rescale set to 0; APG runs with eta_apg 0, momentum -0.5 and a norm cap r.

r is chosen here: the tool prints |d| of step 0 and takes the largest of |d_0| / 2, / 4, / 8, ... for which the APG golden lies at least 10 gates
(10 x 2e-2, the loop gate of tests/test_multistep_gpu.py) from the plain-CFG loop of the same inputs -- otherwise the test could not tell APG from CFG.
CPU only, well under a minute.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BASE = 'smp_xs_e0'
GATE = 2e-2
ETA_APG, MOMENTUM = 0.0, -0.5


def apg_loop(denoise, text, text_mask, uncond_text, uncond_mask, init, coefs, c_hist, timesteps, guidance_scale, apg, gt=None, gt_mask=None):
    """One prompt, batch 1.  apg = (eta_apg, r, momentum) or None for plain CFG without rescale.  Returns (final latent, |d| per step)."""
    from oracle.sampler import cfg_combine
    from tests.apg_emul import apg_fp64
    lat = np.asarray(init, np.float32)
    hist, mom, norms = None, None, []
    cat = lambda a: None if a is None else np.concatenate([a, a], 0)   # noqa: E731
    for i, t in enumerate(timesteps):
        out = denoise(cat(lat), int(t), np.concatenate([text, uncond_text], 0), np.concatenate([text_mask, uncond_mask], 0), cat(gt), cat(gt_mask))
        sa, sb, cx0, cdir, sigma = (float(c) for c in coefs[i])
        assert sigma == 0.0 and sb != 0.0
        x = lat.astype(np.float64)
        if apg is None:
            v = cfg_combine(out[:1], out[1:], guidance_scale).astype(np.float64)
            x0 = sa * x - sb * v
        else:
            eta_apg, r, momentum = apg
            x0, v, mom, (nd, _, _) = apg_fp64(out[:1], out[1:], x, mom, sa, sb, float(guidance_scale), eta_apg, r, momentum if i > 0 else 0.0)
            norms.append(nd)
        eps = sa * v + sb * x
        nxt = cx0 * x0 + cdir * eps
        if c_hist[i] != 0.0:
            nxt = nxt + c_hist[i] * (x0 - hist)
        hist = x0
        lat = nxt.astype(np.float32)
    if gt is not None:
        lat = np.where(np.asarray(gt_mask, bool), lat, np.asarray(gt, np.float32))
    return lat, norms


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
    K = meta['steps']
    gt = inp['gt'][0:1] if meta['with_gt'] else None
    gm = inp['gt_mask'][0:1] if meta['with_gt'] else None
    ch = sch.multistep_coefficients()
    args = (denoise, inp['ctx'][0:1], inp['ctx_mask'][0:1], inp['ctx'][1:2], inp['ctx_mask'][1:2], init, sch.ddim_coefficients(0))
    kw = dict(timesteps=[int(t) for t in sch.timesteps], guidance_scale=meta['guidance_scale'], gt=gt, gt_mask=gm)
    rel = lambda x, y: float(np.linalg.norm(x.astype(np.float64) - y) / np.linalg.norm(y.astype(np.float64)))   # noqa: E731
    cfg_ddim, _ = apg_loop(*args, [0.0] * K, apg=None, **kw)
    cfg_2m, _ = apg_loop(*args, ch, apg=None, **kw)
    # eta_apg 1, no cap, no momentum is plain CFG: the loop itself adds nothing
    same, norms = apg_loop(*args, [0.0] * K, apg=(1.0, 0.0, 0.0), **kw)
    print(f'APG with eta_apg 1, r 0, momentum 0 vs the plain-CFG loop: rel-L2 {rel(same, cfg_ddim):.3e}')
    assert rel(same, cfg_ddim) < 1e-5
    print('|d| per step without cap and momentum:', ' '.join(f'{v:.2f}' for v in norms))
    d0 = norms[0]
    for div in (2, 4, 8, 16, 32, 64):
        r = float(np.float32(d0 / div))
        lat_ddim, nd = apg_loop(*args, [0.0] * K, apg=(ETA_APG, r, MOMENTUM), **kw)
        dist = rel(lat_ddim, cfg_ddim)
        print(f'r = |d_0| / {div} = {r:.4f}: APG (DDIM) vs plain CFG rel-L2 {dist:.3e} = {dist / GATE:.1f} gates; the cap bites on {sum(v > r for v in nd)} of {K} steps')
        if dist >= 10 * GATE:
            break
    else:
        raise SystemExit('no r separates APG from CFG by 10 gates')
    lat_2m, _ = apg_loop(*args, ch, apg=(ETA_APG, r, MOMENTUM), **kw)
    print(f'APG (dpmpp_2m) vs plain CFG (dpmpp_2m): rel-L2 {rel(lat_2m, cfg_2m):.3e} = {rel(lat_2m, cfg_2m) / GATE:.1f} gates')
    assert rel(lat_2m, cfg_2m) >= 10 * GATE
    m = dict(base=BASE, size=meta['size'], L=meta['L'], Lc=meta['Lc'], steps=K, seed_w=meta['seed_w'], seed_in=meta['seed_in'],
             guidance_scale=meta['guidance_scale'], guidance_rescale=0.0, eta=0.0, with_gt=meta['with_gt'], eta_apg=ETA_APG, norm_threshold=r, momentum=MOMENTUM,
             d0=d0, dist_ddim=rel(lat_ddim, cfg_ddim), dist_2m=rel(lat_2m, cfg_2m))
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, 'sampler_apg_xs.npz')
    np.savez_compressed(path, latent_ddim=lat_ddim.astype(np.float32), latent_2m=lat_2m.astype(np.float32), meta=np.array(repr(m)))
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
