"""Cost of sliding-window self-attention on the fused sampler -- diagnostic, GPU only.

    python tools/bench_window.py [--parent-lib PATH/libezaudio_hip.so] [--steps 50] [--loops 7] [--prompts 1 4] [--out FILE.json]
    python tools/bench_window.py --trace full|window [--steps 10]          (the program of a kernel trace: see 3.)

EzAudio-XL, random-init weights and random context, guidance 5 / rescale 0.75, eta 0, DDIM.  The method of tools/bench_start.py and tools/bench_canvas.py: the
libraries are loaded into ONE process, each with its own handle, weights and workspace, and ALTERNATE; every loop prepares the call, runs 2 steps (graph capture +
warm-up) and times the remaining steps with HIP events on the sampler stream.  Printed per side: the median step time and the spread (max - min) / median of its loops.

1. Window OFF against another build of the library (--parent-lib: the parent commit's, built from its own tree) at --prompts prompts of 10 s (L = 500): the off
   path launches the kernels it launched before, so the ratio is to be read against the parent's own loop-to-loop spread.
2. One row of 1500 frames (30 s), CFG on: full attention against radius 250 (each frame sees the 501 keys of the trained row) against the four-window canvas of
   tools/bench_canvas.py, step ms and steps x step ms; and the row of 500 frames at radius 250 (frame 0 does not see frame 499: still the band form, 250 < L - 1)
   and at radius 499 (covers the row: the plain kernel, parity expected).
3. --trace runs a few eager steps of the 1500-frame row with full attention or with radius 250 and nothing else: the program for
   `rocprofv3 --kernel-trace --stats -- python tools/bench_window.py --trace ...`, whose per-kernel table gives the self-attention kernel's own time.
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

RADIUS = 250


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--loops', type=int, default=7)
    ap.add_argument('--prompts', type=int, nargs='*', default=[1, 4])
    ap.add_argument('--trace', choices=['full', 'window'], default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    params = load_yaml_with_includes(configs['s3_xl']['config'])
    cfg = params['model']
    sd = random_state_dict(cfg, seed=0)
    models = {'this': model(cfg, sd)}
    if a.parent_lib and not a.trace:
        models['parent'] = model(cfg, sd, other_library(a.parent_lib))
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

    if a.trace:
        models['this'].set_attention_window(RADIUS if a.trace == 'window' else None)
        smp = LatentSampler(models['this'], sch)
        smp.prepare(*inputs(1, 1500), None, 5.0, 0.75, K, 0.0)
        smp.run(K, use_graph=False)
        assert torch.isfinite(smp.finish()).all()
        torch.cuda.synchronize()
        print(json.dumps(dict(trace=a.trace, steps=K, launches_per_step=models['this'].last_launch_count)))
        return

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

    # 1. window off: this library against the parent's
    if 'parent' in models:
        for P in a.prompts:
            inp = inputs(P, 500)
            alternate('window off, step ms', {'parent': ('parent', inp, {}, None), 'this': ('this', inp, {}, None)}, prompts=P)
    # 2. one row of 1500 frames: full attention, radius 250, the four-window canvas
    row = inputs(1, 1500)
    offs, L = canvas_windows(1500, 500, 125)
    ramp = min(x + L - y for x, y in zip(offs, offs[1:]))
    med = alternate('30 s: one row of 1500 frames with full attention / with radius 250, and four windows of 500 on a canvas; step ms',
                    {'full': ('this', row, {}, None), 'window': ('this', row, {}, RADIUS), 'canvas': ('this', inputs(len(offs), L), dict(canvas=(offs, 1500, ramp)), None)},
                    radius=RADIUS, offsets=offs, ramp=ramp)
    out = dict(what='30 s in all (steps x step ms)', steps=K, **{k + '_ms': round(K * v, 2) for k, v in med.items()})
    print(json.dumps(out), flush=True)
    results.append(out)
    # the trained row at a radius that covers it: the plain kernel
    short = inputs(1, 500)
    alternate('10 s: one row of 500 frames, window off / radius 250 (>= L - 1 is not reached: 250 < 499, the band form) / radius 499 (the plain kernel); step ms',
              {'off': ('this', short, {}, None), 'r250': ('this', short, {}, RADIUS), 'r499': ('this', short, {}, 499)})
    models['this'].set_attention_window(None)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(dict(tool='tools/bench_window.py', device=torch.cuda.get_device_name(0), results=results), f, indent=1)


if __name__ == '__main__':
    main()
