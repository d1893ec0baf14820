"""Cost of adaptive projected guidance on the fused sampler -- diagnostic, GPU only.

    python tools/bench_apg.py [--parent-lib PATH/libezaudio_hip.so] [--steps 50] [--loops 7] [--prompts 1 4] [--out profiles/apg_bench_xl.json]

EzAudio-XL, random-init weights and random context, guidance 5, eta 0, DDIM.  The method of tools/bench_emphasis.py: the libraries are loaded into ONE process, each
with its own handle, weights and workspace, and ALTERNATE; every loop prepares the call, runs 2 steps (graph capture + warm-up) and times the remaining steps with
HIP events on the sampler stream.  Printed per side: the median step time and the spread (max - min) / median of its loops.

1. Table OFF against another build of the library (--parent-lib: the parent commit's, built from its own tree) at --prompts prompts of 10 s (L = 500), rescale 0.75:
   the off path launches the kernels it launched before, so the ratio is to be read against the parent's own loop-to-loop spread.
2. APG ON (eta_apg 0, momentum -0.5, a cap of 30) against OFF at the same shapes, both at rescale 0 (APG takes no rescale): on launches the statistics pass, which
   the plain step at rescale 0 does not, and both tail kernels stream the momentum, P C L floats each way.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ezaudio_amd.config import configs, load_yaml_with_includes      # noqa: E402
from ezaudio_amd.sampler import LatentSampler                        # noqa: E402
from ezaudio_amd.scheduler import DDIMScheduler                      # noqa: E402
from ezaudio_amd.weights import random_state_dict                    # noqa: E402
from tools.bench_start import model, other_library                   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--loops', type=int, default=7)
    ap.add_argument('--prompts', type=int, nargs='*', default=[1, 4])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    params = load_yaml_with_includes(configs['s3_xl']['config'])
    cfg = params['model']
    sd = random_state_dict(cfg, seed=0)
    models = {'this': model(cfg, sd)}
    if a.parent_lib:
        models['parent'] = model(cfg, sd, other_library(a.parent_lib))
    sch = DDIMScheduler(**params['diff'])
    Lc, Cc, K = 100, cfg['out_chans'], a.steps
    g = torch.Generator().manual_seed(3)
    results = []

    def inputs(P, L):
        """one prompt per sample, 12 valid tokens, one in the unconditional row"""
        text, un = torch.randn(P, Lc, cfg['context_dim'], generator=g).cuda(), torch.randn(P, Lc, cfg['context_dim'], generator=g).cuda()
        tm = torch.zeros(P, Lc, dtype=torch.bool).cuda()
        tm[:, :12] = True
        um = torch.zeros(P, Lc, dtype=torch.bool).cuda()
        um[:, :1] = True
        return text, tm, un, um, torch.randn(P, Cc, L, generator=g).cuda()

    def alternate(what, sides, **extra):
        """sides: name -> (model key, prepare arguments, guidance_rescale, prepare keywords); step ms of each, alternating."""
        times = {k: [] for k in sides}
        launches = {}
        order = list(sides)
        for loop in range(a.loops + 1):                                # loop 0 warms every side up and is not counted
            for k in order if loop % 2 == 0 else order[::-1]:
                key, inp, rescale, kw = sides[k]
                smp = LatentSampler(models[key], sch)
                smp.prepare(*inp[:5], None, 5.0, rescale, K, 0.0, **kw)
                smp.run(2)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(smp.stream):
                    e0.record()
                smp.run(K - 2)
                with torch.cuda.stream(smp.stream):
                    e1.record()
                assert torch.isfinite(smp.finish()).all()
                launches[k] = models[key].last_launch_count
                if loop:
                    times[k].append(e0.elapsed_time(e1) / (K - 2))
        med = {k: statistics.median(v) for k, v in times.items()}
        out = dict(what=what, steps=K, loops=a.loops, launches=launches, **extra)
        for k, v in times.items():
            out[k] = dict(median=round(med[k], 4), spread=round((max(v) - min(v)) / med[k], 5), all=[round(x, 4) for x in v])
        names = list(sides)
        for n in names[1:]:
            out[f'{n}_over_{names[0]}'] = round(med[n] / med[names[0]], 5)
        print(json.dumps(out), flush=True)
        results.append(out)
        return med

    apg = dict(eta=0.0, norm_threshold=30.0, momentum=-0.5)
    for P in a.prompts:
        inp = inputs(P, 500)
        if 'parent' in models:
            alternate('table off at rescale 0.75, step ms', {'parent': ('parent', inp, 0.75, {}), 'this': ('this', inp, 0.75, {})}, prompts=P)
        alternate('apg on against off at rescale 0, step ms', {'off': ('this', inp, 0.0, {}), 'on': ('this', inp, 0.0, dict(apg=apg))}, prompts=P)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(dict(tool='tools/bench_apg.py', device=torch.cuda.get_device_name(0), results=results), f, indent=1)


if __name__ == '__main__':
    main()
