"""Cost of the long-form canvas on the fused sampler -- diagnostic, GPU only.

    python tools/bench_canvas.py [--parent-lib PATH/libezaudio_hip.so] [--steps 50] [--loops 7] [--prompts 1 4] [--out FILE.json]

EzAudio-XL, random-init weights and random context, guidance 5 / rescale 0.75, eta 0, DDIM.  The method of tools/bench_start.py: the libraries are loaded into
ONE process, each with its own handle, weights and workspace, and ALTERNATE; every loop prepares the call, runs 2 steps (graph capture + warm-up) and times
the remaining steps with HIP events on the sampler stream.  Printed per side: the median step time and the spread (max - min) / median of its own loops.

1. Canvas OFF against another build of the library (--parent-lib: the parent commit's, built from its own tree) at --prompts prompts of 10 s (L = 500): the
   off path adds no launch and no kernel argument, so the ratio is to be read against the parent's own loop-to-loop spread.
2. Canvas ON, four windows of L = 500 over T = 1500 frames (30 s; canvas_windows(1500, 500, 125), ramp = the smallest overlap), against the plain
   four-prompt step of the parent (of this library without --parent-lib): the difference is k_canvas_blend.
3. The total for 30 s, for orientation: steps x the canvas step against steps x the step of ONE row of 1500 frames, which is what generate_audio(length=30)
   runs today (RoPE positions three times beyond the trained length).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ezaudio_amd.config import configs, load_yaml_with_includes      # noqa: E402
from ezaudio_amd.sampler import LatentSampler, canvas_windows        # noqa: E402
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
    base = 'parent' if a.parent_lib else 'this'
    sch = DDIMScheduler(**params['diff'])
    Lc, Cc, K = 100, cfg['out_chans'], a.steps
    g = torch.Generator().manual_seed(3)
    results = []

    def inputs(P, L):
        text, un = torch.randn(P, Lc, cfg['context_dim'], generator=g).cuda(), torch.randn(P, Lc, cfg['context_dim'], generator=g).cuda()
        tm = torch.zeros(P, Lc, dtype=torch.bool).cuda()
        tm[:, :12] = True
        um = torch.zeros(P, Lc, dtype=torch.bool).cuda()
        um[:, :1] = True
        return text, tm, un, um, torch.randn(P, Cc, L, generator=g).cuda()

    def alternate(what, sides, **extra):
        """sides: name -> (model key, prepare arguments, prepare keywords); step ms of each, alternating."""
        times = {k: [] for k in sides}
        order = list(sides)
        for loop in range(a.loops + 1):                                # loop 0 warms every side up and is not counted
            for k in order if loop % 2 == 0 else order[::-1]:
                key, inp, kw = sides[k]
                smp = LatentSampler(models[key], sch)
                smp.prepare(*inp[:5], None, 5.0, 0.75, K, 0.0, **kw)
                smp.run(2)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(smp.stream):
                    e0.record()
                smp.run(K - 2)
                with torch.cuda.stream(smp.stream):
                    e1.record()
                assert torch.isfinite(smp.finish()).all()
                if loop:
                    times[k].append(e0.elapsed_time(e1) / (K - 2))
        med = {k: statistics.median(v) for k, v in times.items()}
        out = dict(what=what, steps=K, loops=a.loops, **extra)
        for k, v in times.items():
            out[k] = dict(median=round(med[k], 4), spread=round((max(v) - min(v)) / med[k], 5), all=[round(x, 4) for x in v])
        names = list(sides)
        if len(names) == 2:
            out[f'{names[0]}_over_{names[1]}'] = round(med[names[0]] / med[names[1]], 5)
        print(json.dumps(out), flush=True)
        results.append(out)
        return med

    # 1. canvas off: this library against the parent's
    for P in a.prompts:
        inp = inputs(P, 500)
        alternate('canvas off, step ms', {k: (k, inp, {}) for k in models}, prompts=P)
    # 2. canvas on: four windows against the plain four-prompt step
    offs, L = canvas_windows(1500, 500, 125)
    ramp = min(x + L - y for x, y in zip(offs, offs[1:]))
    win = inputs(len(offs), L)
    med = alternate('canvas on (4 windows of 500 over 1500 frames) against the plain 4-prompt step, step ms',
                    {'canvas': ('this', win, dict(canvas=(offs, 1500, ramp))), 'plain': (base, win, {})}, offsets=offs, ramp=ramp, plain_side=base)
    # 3. 30 s in all: the canvas against one row of 1500 frames
    row = inputs(1, 1500)
    med1 = alternate('one row of 1500 frames, step ms', {'row': (base, row, {})}, side=base)
    out = dict(what='30 s in all (steps x step ms), canvas against one 1500-frame row', steps=K, canvas_ms=round(K * med['canvas'], 2),
               row_ms=round(K * med1['row'], 2), canvas_over_row=round(med['canvas'] / med1['row'], 4))
    print(json.dumps(out), flush=True)
    results.append(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(dict(tool='tools/bench_canvas.py', device=torch.cuda.get_device_name(0), results=results), f, indent=1)


if __name__ == '__main__':
    main()
