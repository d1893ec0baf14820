"""Step time of the fused sampler with solver='dpmpp_2m' against solver='ddim' at eta = 0 -- diagnostic, GPU only.

    python tools/bench_solver_step.py [--steps 50] [--loops 7] [--prompts 1 4]

EzAudio-XL, 10 s latent (L = 500), random-init weights and random context, guidance 5 / rescale 0.75.  The two solvers ALTERNATE in one process; every
loop prepares the call, runs 2 steps (graph capture + warm-up) and times the remaining steps with HIP events on the sampler stream.  Prints the median
step time of each solver and their ratio per prompt count.  It measures the cost of a step only: how many steps either solver needs is not its subject.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ezaudio_amd import MaskDiT                                      # noqa: E402
from ezaudio_amd.config import configs, load_yaml_with_includes      # noqa: E402
from ezaudio_amd.sampler import LatentSampler                        # noqa: E402
from ezaudio_amd.scheduler import DDIMScheduler                      # noqa: E402
from ezaudio_amd.weights import random_state_dict                    # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--loops', type=int, default=7)
    ap.add_argument('--prompts', type=int, nargs='*', default=[1, 4])
    a = ap.parse_args()
    params = load_yaml_with_includes(configs['s3_xl']['config'])
    cfg = params['model']
    unet = MaskDiT(device='cuda:0', **cfg)
    unet.load_state_dict(random_state_dict(cfg, seed=0))
    sch = DDIMScheduler(**params['diff'])
    L, Lc, C = 500, 100, cfg['out_chans']
    g = torch.Generator().manual_seed(3)
    for P in a.prompts:
        text, un = torch.randn(P, Lc, cfg['context_dim'], generator=g).cuda(), torch.randn(P, Lc, cfg['context_dim'], generator=g).cuda()
        tm = torch.zeros(P, Lc, dtype=torch.bool).cuda()
        tm[:, :12] = True
        um = torch.zeros(P, Lc, dtype=torch.bool).cuda()
        um[:, :1] = True
        init = torch.randn(P, C, L, generator=g).cuda()
        times = {'ddim': [], 'dpmpp_2m': []}
        for loop in range(a.loops + 1):                                # loop 0 warms both up and is not counted
            for solver in ('ddim', 'dpmpp_2m') if loop % 2 == 0 else ('dpmpp_2m', 'ddim'):
                smp = LatentSampler(unet, sch)
                smp.prepare(text, tm, un, um, init, None, 5.0, 0.75, a.steps, 0.0, solver=solver)
                smp.run(2)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(smp.stream):
                    e0.record()
                smp.run(a.steps - 2)
                with torch.cuda.stream(smp.stream):
                    e1.record()
                lat = smp.finish()
                assert torch.isfinite(lat).all()
                if loop:
                    times[solver].append(e0.elapsed_time(e1) / (a.steps - 2))
        med = {k: statistics.median(v) for k, v in times.items()}
        print(json.dumps(dict(prompts=P, steps=a.steps, loops=a.loops, step_ms_ddim=round(med['ddim'], 4), step_ms_dpmpp_2m=round(med['dpmpp_2m'], 4),
                              ratio=round(med['dpmpp_2m'] / med['ddim'], 4),
                              ddim_all=[round(v, 4) for v in times['ddim']], dpmpp_2m_all=[round(v, 4) for v in times['dpmpp_2m']])), flush=True)


if __name__ == '__main__':
    main()
