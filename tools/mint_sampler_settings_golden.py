"""Mint the reference goldens of the per-sample sampler settings (tests/test_sample_params_gpu.py).

    python tools/mint_sampler_settings_golden.py [--only NAME ...] [--out tests/golden]

Four runs of the reference's unmodified inference() through oracle.mint_golden.mint_sampler (CPU, needs the reference tree, a few
seconds each).  All share size xs, Lc 20, 50 steps and seed_w 1 with the existing `sampler_smp_xs` (guidance 5.0, rescale 0.75,
eta 1.0, seed_in 21, L 96), so the five can sit in one batch, each with its own guidance_scale / guidance_rescale / eta:

    smp_xs_b     another value of all three knobs (guidance alone wrong: rel-L2 0.77 off its golden, eta alone wrong: 0.76)
    smp_xs_d     guidance 7.0 WITHOUT rescale next to samples with it (rescale 0.75 instead of 0: 0.30 off)
    smp_xs_n     no guidance (guidance_scale=None: the reference's `text == ''` run) inside a CFG batch
    smp_xs_c60   60 frames, eta 0: the partner of smp_xs in a batch with per-sample lengths AND settings
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COMMON = dict(size='xs', Lc=20, steps=50, seed_w=1)
JOBS = {
    'smp_xs_b':   dict(L=96, seed_in=26, guidance_scale=2.0, guidance_rescale=0.3, eta=0.5),
    'smp_xs_d':   dict(L=96, seed_in=29, guidance_scale=7.0, guidance_rescale=0.0, eta=1.0),
    'smp_xs_n':   dict(L=96, seed_in=28, guidance_scale=None, guidance_rescale=0.0, eta=1.0),
    'smp_xs_c60': dict(L=60, seed_in=27, guidance_scale=3.5, guidance_rescale=0.0, eta=0.0),
}


def main():
    from oracle.mint_golden import mint_sampler
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', nargs='*')
    ap.add_argument('--out', default='tests/golden')
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    for name, kw in JOBS.items():
        if a.only and name not in a.only:
            continue
        mint_sampler(name, out_dir=a.out, **COMMON, **kw)


if __name__ == '__main__':
    main()
