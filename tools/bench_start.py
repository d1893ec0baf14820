"""Cost of the start table (audio-to-audio) on the fused sampler -- diagnostic, GPU only.

    python tools/bench_start.py [--parent-lib PATH/libezaudio_hip.so] [--steps 50] [--loops 7] [--prompts 1 4]

EzAudio-XL, 10 s latent (L = 500), random-init weights and random context, guidance 5 / rescale 0.75, eta 0, DDIM.

1. Table OFF against another build of the library (--parent-lib: the parent commit's, built from its own tree): the two libraries are loaded into ONE
   process, each with its own handle, weights and workspace, and ALTERNATE; every loop prepares the call, runs 2 steps (graph capture + warm-up) and
   times the remaining steps with HIP events on the sampler stream (the method of tools/bench_solver_step.py).  Prints the median step time of each, their
   ratio, and the spread (max - min) / median of each side's own loops: the difference is to be read against that spread.
2. Table ON, this library alone: wall time of run() for a uniform start at steps / 2 against the full run, and a two-request call with starts
   [0, steps / 2] against the two single calls (full run + half run).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ezaudio_amd import MaskDiT, _lib                                # noqa: E402
from ezaudio_amd.config import configs, load_yaml_with_includes      # noqa: E402
from ezaudio_amd.sampler import LatentSampler                        # noqa: E402
from ezaudio_amd.scheduler import DDIMScheduler                      # noqa: E402
from ezaudio_amd.weights import random_state_dict                    # noqa: E402


def other_library(path):
    """Another build of the library, bound like _lib.load() binds this one (entry points it does not export are left out)."""
    lib = C.CDLL(path)
    for name, (res, args) in list(_lib.PROTOTYPES.items()) + list(_lib.T5_PROTOTYPES.items()):
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    assert lib.ezdit_abi_version() == _lib.ABI_VERSION
    return lib


def model(cfg, sd, lib=None):
    mine = _lib.load()
    if lib is not None:
        _lib._lib = lib                                               # MaskDiT keeps the library it was created with
    try:
        unet = MaskDiT(device='cuda:0', **cfg)
        unet.load_state_dict(sd)
    finally:
        _lib._lib = mine
    return unet


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--loops', type=int, default=7)
    ap.add_argument('--prompts', type=int, nargs='*', default=[1, 4])
    a = ap.parse_args()
    params = load_yaml_with_includes(configs['s3_xl']['config'])
    cfg = params['model']
    sd = random_state_dict(cfg, seed=0)
    models = {'this': model(cfg, sd)}
    if a.parent_lib:
        models['parent'] = model(cfg, sd, other_library(a.parent_lib))
    sch = DDIMScheduler(**params['diff'])
    L, Lc, Cc, K = 500, 100, cfg['out_chans'], a.steps
    g = torch.Generator().manual_seed(3)

    def inputs(P):
        text, un = torch.randn(P, Lc, cfg['context_dim'], generator=g).cuda(), torch.randn(P, Lc, cfg['context_dim'], generator=g).cuda()
        tm = torch.zeros(P, Lc, dtype=torch.bool).cuda()
        tm[:, :12] = True
        um = torch.zeros(P, Lc, dtype=torch.bool).cuda()
        um[:, :1] = True
        return text, tm, un, um, torch.randn(P, Cc, L, generator=g).cuda(), torch.randn(P, Cc, L, generator=g).cuda()

    # 1. table off: step time, this library against the parent's
    for P in a.prompts:
        text, tm, un, um, init, _ = inputs(P)
        times = {k: [] for k in models}
        order = list(models)
        for loop in range(a.loops + 1):                                # loop 0 warms both up and is not counted
            for k in order if loop % 2 == 0 else order[::-1]:
                smp = LatentSampler(models[k], sch)
                smp.prepare(text, tm, un, um, init, None, 5.0, 0.75, K, 0.0)
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
        out = dict(what='table off, step ms', prompts=P, steps=K, loops=a.loops)
        for k, v in times.items():
            out[k] = dict(median=round(med[k], 4), spread=round((max(v) - min(v)) / med[k], 5), all=[round(x, 4) for x in v])
        if 'parent' in med:
            out['this_over_parent'] = round(med['this'] / med['parent'], 5)
        print(json.dumps(out), flush=True)

    # 2. table on: wall time of run()
    unet = models['this']

    def wall(P, starts, inp):
        text, tm, un, um, init, clean = inp
        ts = []
        for loop in range(a.loops + 1):
            smp = LatentSampler(unet, sch)
            kw = {} if starts is None else dict(init_latents=clean, start_steps=starts, latent_scale=1.0, latent_shift=0.0)
            smp.prepare(text[:P], tm[:P], un[:P], um[:P], init[:P], None, 5.0, 0.75, K, 0.0, **kw)
            smp.run(1)                                                 # graph capture + warm-up; the step is undone below
            with torch.cuda.stream(smp.stream):
                _lib.check(unet.lib.ezdit_set_step(unet._h, smp.first_step, C.c_void_p(smp.stream.cuda_stream)))
            smp.stream.synchronize()
            t = time.perf_counter()
            smp.run()
            smp.finish()
            if loop:
                ts.append((time.perf_counter() - t) * 1e3)
        return statistics.median(ts)
    two = inputs(2)
    one = tuple(t[:1] for t in two)
    full, half = wall(1, None, one), wall(1, [K // 2], one)
    print(json.dumps(dict(what='uniform start, wall ms of run()', steps=K, start=K // 2, full=round(full, 3), started=round(half, 3),
                          ratio=round(half / full, 4))), flush=True)
    both = wall(2, [0, K // 2], two)
    print(json.dumps(dict(what='two requests, starts [0, K/2], wall ms of run()', steps=K, batched=round(both, 3), two_single_calls=round(full + half, 3),
                          ratio=round(both / (full + half), 4))), flush=True)


if __name__ == '__main__':
    main()
