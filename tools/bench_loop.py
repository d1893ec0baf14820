"""Cost of seamless loops (the canvas as a ring) on the fused sampler and end to end -- diagnostic, GPU only.

    python tools/bench_loop.py [--parent-lib PATH/libezaudio_hip.so] [--steps 50] [--loops 7] [--prompts 1 4] [--out FILE.json]

EzAudio-XL, random-init weights and random context, guidance 5 / rescale 0.75, eta 0, DDIM.  The method of tools/bench_canvas.py: the libraries are loaded into
ONE process, each with its own handle, weights and workspace, and ALTERNATE; every loop prepares the call, runs 2 steps (graph capture + warm-up) and times
the remaining steps with HIP events on the sampler stream.  Printed per side: the median step time and the spread (max - min) / median of its own loops.

1. Table OFF against another build of the library (--parent-lib: the parent commit's, built from its own tree) at --prompts prompts of 10 s (L = 500): the
   off path adds no launch and no kernel argument, so the ratio is to be read against the parent's own loop-to-loop spread.
2. Loop ON, four windows of L = 500 on a ring of 1500 frames (loop_windows(1500, 500, 125): [0, 375, 750, 1125], ramp 125), against the LINEAR canvas of
   four windows over 1500 frames (canvas_windows(1500, 500, 125), ramp 166), both on this library: k_canvas_blend_loop against k_canvas_blend.
3. End to end, wall time with a device synchronise: EzAudio.generate_loop(30 s) against EzAudio.generate_long_audio(30 s), synthetic VAE weights and a stand-in
   text encoder (tools/bench_e2e.py), alternated.  Both sample four windows; the loop decodes 2 x decoder_context_frames() more latent frames.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ezaudio_amd import api as A                                     # noqa: E402
from ezaudio_amd.config import configs, load_yaml_with_includes      # noqa: E402
from ezaudio_amd.sampler import LatentSampler, canvas_windows, loop_overlaps, loop_windows   # noqa: E402
from ezaudio_amd.scheduler import DDIMScheduler                      # noqa: E402
from ezaudio_amd.vae import Autoencoder                              # noqa: E402
from ezaudio_amd.weights import random_state_dict                    # noqa: E402
from oracle import vae as V                                          # noqa: E402  (synthetic VAE weights only)
from tools.bench_start import model, other_library                   # noqa: E402


class Tok:
    def __call__(self, texts, max_length, padding, truncation, return_tensors):
        ids = torch.zeros(len(texts), max_length, dtype=torch.long)
        mask = torch.zeros(len(texts), max_length, dtype=torch.long)
        for i, t in enumerate(texts):
            n = max(1, min(max_length, len(t.split()) + 1))
            ids[i, :n] = torch.arange(1, n + 1)
            mask[i, :n] = 1
        return type('B', (), dict(input_ids=ids, attention_mask=mask))()


class Enc:
    def __init__(self, dim):
        self.table = torch.randn(128, dim, generator=torch.Generator().manual_seed(7)).cuda()

    def __call__(self, input_ids, attention_mask):
        return type('O', (), dict(last_hidden_state=self.table[input_ids % 128]))()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--loops', type=int, default=7)
    ap.add_argument('--e2e-loops', type=int, default=3)
    ap.add_argument('--prompts', type=int, nargs='*', default=[1, 4])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    params = load_yaml_with_includes(configs['s3_xl']['config'])
    cfg = params['model']
    sd = random_state_dict(cfg, seed=0)
    vsd = {k: torch.from_numpy(v) for k, v in V.make_vae_state_dict(dict(V.VAE_DEFAULT), 6).items()}
    common = dict(channels=128, c_mults=[1, 2, 4, 8], strides=[2, 4, 6, 10], use_snake=True)
    vconf = {'model': {'decoder': {'type': 'oobleck', 'config': dict(out_channels=1, latent_dim=128, final_tanh=False, **common)}}}
    ez = A.EzAudio('s3_xl', autoencoder=Autoencoder(config=vconf, state_dict=vsd), tokenizer=Tok(), text_encoder=Enc(cfg['context_dim']), state_dict=sd)
    models = {'this': model(cfg, sd)}                                # (its own handle, made like the parent's: ez.unet serves part 3 only)
    if a.parent_lib:
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

    def emit(out):
        print(json.dumps(out), flush=True)
        results.append(out)

    def summary(what, times, **extra):
        med = {k: statistics.median(v) for k, v in times.items()}
        out = dict(what=what, **extra)
        for k, v in times.items():
            out[k] = dict(median=round(med[k], 4), spread=round((max(v) - min(v)) / med[k], 5), all=[round(x, 4) for x in v])
        names = list(times)
        if len(names) == 2:
            out[f'{names[0]}_over_{names[1]}'] = round(med[names[0]] / med[names[1]], 5)
        emit(out)

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
        summary(what, times, steps=K, loops=a.loops, **extra)

    # 1. table off: this library against the parent's
    if a.parent_lib:
        for P in a.prompts:
            inp = inputs(P, 500)
            alternate('table off, step ms', {k: (k, inp, {}) for k in models}, prompts=P)
    # 2. the ring against the line, four windows each
    loffs, L = loop_windows(1500, 500, 125)
    lramp = min(loop_overlaps(loffs, L, 1500))
    coffs, _ = canvas_windows(1500, 500, 125)
    cramp = min(x + L - y for x, y in zip(coffs, coffs[1:]))
    assert len(loffs) == len(coffs) == 4
    win = inputs(4, L)
    alternate('loop on (4 windows of 500 on a ring of 1500) against the linear canvas (4 windows over 1500), step ms',
              {'loop': ('this', win, dict(canvas_loop=(loffs, 1500, lramp))), 'line': ('this', win, dict(canvas=(coffs, 1500, cramp)))},
              loop_offsets=loffs, loop_ramp=lramp, line_offsets=coffs, line_ramp=cramp)
    # 3. end to end: generate_loop against generate_long_audio, 30 s
    calls = {'generate_loop': lambda: ez.generate_loop('rain on a tin roof', 30, ddim_steps=K, eta=0, random_seed=1),
             'generate_long_audio': lambda: ez.generate_long_audio('rain on a tin roof', 30, ddim_steps=K, eta=0, random_seed=1)}
    times = {k: [] for k in calls}
    order = list(calls)
    for loop in range(a.e2e_loops + 1):
        for k in order if loop % 2 == 0 else order[::-1]:
            torch.cuda.synchronize()
            t = time.perf_counter()
            sr, wav = calls[k]()
            torch.cuda.synchronize()
            dt = 1e3 * (time.perf_counter() - t)
            assert wav.shape == (30 * sr,)
            if loop:
                times[k].append(dt)
    summary('30 s end to end, wall ms (sampling, decode, copy to host)', times, steps=K, loops=a.e2e_loops,
            decode_context_frames=ez.autoencoder.decoder_context_frames())
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(dict(tool='tools/bench_loop.py', device=torch.cuda.get_device_name(0), results=results), f, indent=1)


if __name__ == '__main__':
    main()
