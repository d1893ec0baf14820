"""Cost of the prompt timeline on the fused sampler -- diagnostic, GPU only.

    python tools/bench_timeline.py [--parent-lib PATH/libezaudio_hip.so] [--steps 50] [--loops 7] [--prompts 1 4] [--out profiles/timeline_bench_xl.json]

EzAudio-XL, random-init weights and random context, guidance 5 / rescale 0.75, eta 0, DDIM.  The method of tools/bench_window.py: the libraries are loaded into ONE
process, each with its own handle, weights and workspace, and ALTERNATE; every loop prepares the call, runs 2 steps (graph capture + warm-up) and times the remaining
steps with HIP events on the sampler stream.  Printed per side: the median step time and the spread (max - min) / median of its loops.

1. Timeline OFF against another build of the library (--parent-lib: the parent commit's, built from its own tree) at --prompts prompts of 10 s (L = 500): the off path
   launches the kernels it launched before, so the ratio is to be read against the parent's own loop-to-loop spread.
2. One row of 1500 frames (30 s) under sliding-window radius 250, CFG on: a three-prompt scene (a switch and a cross-fade: every key tile is walked by some workgroup,
   most workgroups walk one) against the same row with one prompt (Lc = 100, no table).
3. One row of 500 frames with S = 3 against the same row with one prompt.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ezaudio_amd.config import configs, load_yaml_with_includes      # noqa: E402
from ezaudio_amd.sampler import LatentSampler, scene_weights         # noqa: E402
from ezaudio_amd.scheduler import DDIMScheduler                      # noqa: E402
from ezaudio_amd.weights import random_state_dict                    # noqa: E402
from tools.bench_start import model, other_library                   # noqa: E402

RADIUS, S = 250, 3


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

    def inputs(P, L, n_seg=None):
        """one prompt per sample (text [P, Lc, Cctx]) or n_seg prompts per sample (text [P, n_seg, Lc, Cctx]); 12 valid tokens per prompt, one in the unconditional row"""
        seg = () if n_seg is None else (n_seg,)
        text, un = torch.randn(P, *seg, Lc, cfg['context_dim'], generator=g).cuda(), torch.randn(P, Lc, cfg['context_dim'], generator=g).cuda()
        tm = torch.zeros(P, *seg, Lc, dtype=torch.bool).cuda()
        tm[..., :12] = True
        um = torch.zeros(P, Lc, dtype=torch.bool).cuda()
        um[:, :1] = True
        return text, tm, un, um, torch.randn(P, Cc, L, generator=g).cuda()

    def scene(L):
        """three prompts over L frames at 50 frames per second: a switch at one third, a two-second cross-fade at two thirds"""
        sec = L / 50.0
        _, hard = scene_weights([('a', 0, sec / 3), ('bc', sec / 3, sec)], L, 50.0, 0.0)
        _, fade = scene_weights([('ab', 0, 2 * sec / 3), ('c', 2 * sec / 3, sec)], L, 50.0, 2.0)
        return torch.stack([hard[0], hard[1] * fade[0], fade[1]])[None]      # [1, S, L]; the columns sum to 1

    def alternate(what, sides, **extra):
        """sides: name -> (model key, prepare arguments, prepare keywords, radius or None); step ms of each, alternating."""
        times = {k: [] for k in sides}
        order = list(sides)
        for loop in range(a.loops + 1):                                # loop 0 warms every side up and is not counted
            for k in order if loop % 2 == 0 else order[::-1]:
                key, inp, kw, radius = sides[k]
                if key == 'this':
                    models[key].set_attention_window(radius)
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
        for n in names[1:]:
            out[f'{n}_over_{names[0]}'] = round(med[n] / med[names[0]], 5)
        print(json.dumps(out), flush=True)
        results.append(out)
        return med

    # 1. timeline off: this library against the parent's
    if 'parent' in models:
        for P in a.prompts:
            inp = inputs(P, 500)
            alternate('timeline off, step ms', {'parent': ('parent', inp, {}, None), 'this': ('this', inp, {}, None)}, prompts=P)
    # 2. one row of 1500 frames at radius 250: one prompt against a three-prompt scene
    alternate('30 s: one row of 1500 frames at radius 250, one prompt / a three-prompt scene; step ms',
              {'one': ('this', inputs(1, 1500), {}, RADIUS), 'scene': ('this', inputs(1, 1500, S), dict(context_weights=scene(1500)), RADIUS)}, radius=RADIUS, S=S)
    # 3. one row of 500 frames: one prompt against S = 3
    alternate('10 s: one row of 500 frames, one prompt / a three-prompt scene; step ms',
              {'one': ('this', inputs(1, 500), {}, None), 'scene': ('this', inputs(1, 500, S), dict(context_weights=scene(500)), None)}, S=S)
    models['this'].set_attention_window(None)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(dict(tool='tools/bench_timeline.py', device=torch.cuda.get_device_name(0), results=results), f, indent=1)


if __name__ == '__main__':
    main()
