"""GPU tests of audio-to-audio: a sampler run that starts at a per-sample step from a noised clip (ezdit_add_noise, ezdit_sampler_set_start,
LatentSampler.prepare(init_latents=, start_steps=), inference(init_latents=, strength=), EzAudio.audio_to_audio).

The reference never starts anywhere but pure noise.  The judges are the noising formula in float64 (kernel level), the numpy oracle's loop over
timesteps[k:] (tests/golden/sampler_start_xs.npz, tools/mint_start_golden.py), bit for bit the existing path (ezdit_set_step(k) on a run without the
table; the plain call where every start is 0) and, for held samples, each sample's own single run.  xs width throughout.
"""
import ctypes as C
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

from oracle import vae as V
from oracle.weights import uniform_pm1
from tests.test_sample_params_gpu import _row, get_model, t_
from tests.util import DIFF, load_golden, record, rel_l2, sampler_case

pytestmark = pytest.mark.gpu

SCALE, SHIFT = 0.5, -0.3


def _scheduler(steps):
    from ezaudio_amd.scheduler import DDIMScheduler
    sch = DDIMScheduler(**DIFF)
    sch.set_timesteps(steps)
    return sch


# ---------------------------------------------------------------------------------------------------
# 1. kernel level: ezdit_add_noise against float64
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L,lens', [(96, None), (150, None), (150, [150, 77, 1])])
def test_add_noise_operator_against_fp64(lib, L, lens):
    """P = 3, n = 128 L: 12288 elements are less than one sweep of the kernel's grid (16 x 256 threads x 4 elements), 19200 one sweep and a partial one.
    Sample 0 at step 7 of 50, sample 1 at step 30, sample 2 with the row (0, 1) and a NaN clean row: bitwise its input.  With lengths the padded frames of
    every input hold NaN and come out exactly 0.  Gate: rel-L2 5e-6, the operator gate of tests/test_gpu.py::test_cfg_ddim_step_operator_against_oracle."""
    P, Cc = 3, 128
    n = Cc * L
    g = torch.Generator().manual_seed(3000 + L)
    clean = (torch.randn(P, Cc, L, generator=g) * 1.7).numpy()
    lat = torch.randn(P, Cc, L, generator=g).numpy()
    co = _scheduler(50).ddim_coefficients(0.0)
    params = np.array([co[7][:2], co[30][:2], (0.0, 1.0)], np.float32)
    assert tuple(co[0][:2]) == (0.0, 1.0)                                # ... which is start step 0 of the shipped schedule
    ln = lens or [L] * P
    ref = (params[:, 0, None, None].astype(np.float64) * ((clean.astype(np.float64) + SHIFT) * SCALE)
           + params[:, 1, None, None].astype(np.float64) * lat.astype(np.float64))
    clean[2] = np.nan
    if lens:
        for p, k in enumerate(ln):
            clean[p, :, k:] = np.nan
            lat[p, :, k:] = np.nan
    cd, ld, pr = t_(clean), t_(lat), t_(params)
    kl = torch.tensor(ln, dtype=torch.int32, device='cuda:0') if lens else None
    klp = kl.data_ptr() if lens else None
    rc = lib.ezdit_add_noise(cd.data_ptr(), ld.data_ptr(), pr.data_ptr(), SCALE, SHIFT, klp, L, P, n, None)
    assert rc == 0, lib.ezdit_last_error()
    torch.cuda.synchronize()
    got = ld.cpu().numpy()
    for p, k in enumerate(ln[:2]):
        e = rel_l2(got[p, :, :k], ref[p, :, :k])
        record(f'add_noise operator L={L} lens={lens} sample {p} (sa {params[p, 0]:.4f}, sb {params[p, 1]:.4f}): rel-L2 vs fp64 {e:.3e}')
        assert np.isfinite(got[p]).all() and e < 5e-6, (p, e)
        assert np.array_equal(got[p, :, k:], np.zeros((Cc, L - k), np.float32)), 'padded frames must be exactly 0'
    # the (0, 1) sample is not touched at all: NaN padding included, its clean row is not read
    assert np.array_equal(got[2], lat[2], equal_nan=True) and np.isfinite(got[2, :, :ln[2]]).all()
    args = (cd.data_ptr(), ld.data_ptr(), pr.data_ptr(), SCALE, SHIFT, klp, L, P, n, None)
    for i in (0, 1, 2):                                                  # a null pointer of each required kind is refused
        assert lib.ezdit_add_noise(*(args[:i] + (None,) + args[i + 1:])) == -1, i
    assert lib.ezdit_add_noise(*(args[:6] + (L - 1,) + args[7:])) == -1 and b'divide' in lib.ezdit_last_error()
    assert lib.ezdit_add_noise(*(args[:6] + (0,) + args[7:])) == -1
    torch.cuda.synchronize()
    assert np.array_equal(ld.cpu().numpy(), got, equal_nan=True)         # a refused call launches nothing


# ---------------------------------------------------------------------------------------------------
# the fused loop on smp_xs_e0's inputs
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case():
    cfg, sd, inp, init, noises, g, meta = sampler_case('smp_xs_e0')
    assert (meta['size'], meta['seed_w'], meta['steps'], meta['eta'], meta['with_gt']) == ('xs', 1, 20, 0.0, True)
    clean = (1.5 * uniform_pm1('start.clean', 128 * meta['L'], meta['seed_in'])).reshape(1, 128, meta['L']).astype(np.float32)   # tools/mint_start_golden.py
    return inp, init, meta, clean


def _prepare(solver='ddim', P=1, starts=None, clean=None, with_gt=True, **kw):
    from ezaudio_amd.sampler import LatentSampler
    inp, init, meta, _ = _case()
    m = get_model('xs', 1)
    smp = LatentSampler(m, _scheduler(meta['steps']))
    text, tm = t_(inp['ctx'][0:1]).repeat(P, 1, 1), t_(inp['ctx_mask'][0:1]).repeat(P, 1)
    un, um = t_(inp['ctx'][1:2]).repeat(P, 1, 1), t_(inp['ctx_mask'][1:2]).repeat(P, 1)
    gt = t_(inp['gt'][0:1]) if with_gt else None
    gm = t_(inp['gt_mask'][0:1]) if with_gt else None
    args = dict(guidance_scale=meta['guidance_scale'], guidance_rescale=meta['guidance_rescale'], eta=0.0, step_noises=None)
    args.update(kw)
    a2a = {} if starts is None else dict(init_latents=clean, start_steps=starts, latent_scale=SCALE, latent_shift=SHIFT)
    smp.prepare(text, tm, un, um, t_(init).repeat(P, 1, 1), args['step_noises'], args['guidance_scale'], args['guidance_rescale'], meta['steps'],
                args['eta'], gt=gt, gt_mask=gm, solver=solver, **a2a)
    return smp


def _finish(smp, use_graph=True, pieces=None):
    for n in (pieces or [None]):
        smp.run(n, use_graph=use_graph)
    lat = smp.finish().clone()
    torch.cuda.synchronize()
    return lat


def _step_counter(m):
    torch.cuda.synchronize()
    return int(m.debug_buffer('ints', torch.int32)[0])


@functools.lru_cache(maxsize=None)
def _from_seven():
    """prepare(init_latents, start_steps=7) + run(), graph replay: computed once, shared, never modified."""
    _, _, _, clean = _case()
    return _finish(_prepare(starts=7, clean=t_(clean)))


def test_table_path_is_bitwise_the_existing_path_from_step_seven(lib):
    """Uniform start 7 through the start table against the same inputs through ezdit_add_noise, ezdit_sampler_begin, ezdit_set_step(7) and run(13) on a
    run WITHOUT the table (the kernels that have always run): identical bits, under graph replay and eager, and in pieces."""
    inp, init, meta, clean = _case()
    m = get_model('xs', 1)
    tab = _from_seven()
    assert torch.isfinite(tab).all()
    co = _scheduler(meta['steps']).ddim_coefficients(0.0)
    for use_graph in (True, False):
        smp = _prepare()
        st = C.c_void_p(smp.stream.cuda_stream)
        pr, cd = t_(np.array([co[7][:2]], np.float32)), t_(clean)
        with torch.cuda.stream(smp.stream):
            assert lib.ezdit_add_noise(cd.data_ptr(), smp.latents.data_ptr(), pr.data_ptr(), SCALE, SHIFT, None, meta['L'], 1, 128 * meta['L'], st) == 0
            assert lib.ezdit_set_step(m._h, 7, st) == 0
        old = _finish(smp, use_graph=use_graph, pieces=[13])
        assert torch.equal(old, tab), use_graph
    assert torch.equal(_finish(_prepare(starts=7, clean=t_(clean)), use_graph=False), tab)
    for use_graph in (True, False):
        assert torch.equal(_finish(_prepare(starts=7, clean=t_(clean)), use_graph=use_graph, pieces=[3, 10]), tab), use_graph
    smp = _prepare(starts=7, clean=t_(clean))
    assert smp.first_step == 7 and _step_counter(m) == 7
    assert lib.ezdit_sampler_run(m._h, 14, 1, C.c_void_p(smp.stream.cuda_stream)) == -3     # bounded by n_steps - current step


def test_started_runs_against_the_numpy_oracle(lib):
    """k = 1, 7, 19 (the last step alone: a_prev = 1, c_hist = 0), DDIM and the 2M update whose first step is first-order.  Gate: the project's fused-loop
    gate 2e-2 (tests/test_gpu.py::test_sampler_matches_reference_loop_golden); smp_xs_e0's own DDIM run from step 0 measures 4.4e-3."""
    inp, init, meta, clean = _case()
    g, gmeta = load_golden('sampler_start_xs')
    assert gmeta['base'] == 'smp_xs_e0' and gmeta['steps'] == meta['steps'] and (gmeta['scale'], gmeta['shift']) == (SCALE, SHIFT)
    gt, gm = t_(inp['gt'][0:1]), t_(inp['gt_mask'][0:1])
    fin = lambda lat: torch.where(gm, lat, gt).cpu().numpy()   # noqa: E731  src/inference.py:104-105
    for k in gmeta['starts']:
        got = {}
        for solver, key in (('ddim', 'ddim'), ('dpmpp_2m', 'ms')):
            lat = _finish(_prepare(solver, starts=k, clean=t_(clean)))
            got[key] = lat
            e = rel_l2(fin(lat), g[f'{key}_{k}'])
            record(f'sampler_start_xs start {k} of {meta["steps"]} ({solver}): final-latent rel-L2 vs the numpy oracle loop {e:.3e}')
            assert torch.isfinite(lat).all() and e < 2e-2, (k, solver, e)
        d = rel_l2(got['ms'].cpu().numpy(), got['ddim'].cpu().numpy())
        record(f'sampler_start_xs start {k}: 2M vs DDIM run {d:.3e}')
        assert (d == 0.0) if k == 19 else (d > 1e-3), (k, d)            # the history term is applied from step k + 1 on, and only there


# ---------------------------------------------------------------------------------------------------
# 4. held samples
# ---------------------------------------------------------------------------------------------------
def test_a_held_sample_keeps_its_bits_and_the_step_counter_advances(lib):
    """P = 2, starts [0, 7], eta 1, NaN in sample 1's step-noise slices 0 .. 6 and in sample 0's clean row (neither is read)."""
    inp, init, meta, clean = _case()
    m = get_model('xs', 1)
    K, L = meta['steps'], meta['L']
    noise = torch.randn(K, 2, 128, L, generator=torch.Generator().manual_seed(17)).cuda()
    held = noise.clone()
    held[:7, 1] = float('nan')
    cl2 = t_(clean).repeat(2, 1, 1)
    cl2[0] = float('nan')
    smp = _prepare(P=2, starts=[0, 7], clean=cl2, eta=1.0, step_noises=held)
    smp.stream.synchronize()
    noised = smp.latents.clone()
    co = _scheduler(K).ddim_coefficients(1.0)
    want = co[7][0] * ((clean.astype(np.float64) + SHIFT) * SCALE) + co[7][1] * init.astype(np.float64)
    assert torch.equal(noised[0:1], t_(init)) and rel_l2(noised[1:2].cpu().numpy(), want) < 5e-6
    assert smp.first_step == 0 and _step_counter(m) == 0
    smp.run(7)
    smp.stream.synchronize()
    assert torch.equal(smp.latents[1], noised[1]), 'a held sample keeps its bits'
    assert not torch.equal(smp.latents[0], noised[0]) and torch.isfinite(smp.latents).all()
    assert _step_counter(m) == 7, 'held workgroups still arrive at the counter'
    both = _finish(smp, pieces=[K - 7])
    assert torch.isfinite(both).all() and _step_counter(m) == K
    singles = (_finish(_prepare(eta=1.0, step_noises=noise[:, 0:1].contiguous())),
               _finish(_prepare(starts=[7], clean=t_(clean), eta=1.0, step_noises=noise[:, 1:2].contiguous())))
    for i, one in enumerate(singles):
        e = rel_l2(both[i:i + 1].cpu().numpy(), one.cpu().numpy())
        record(f'starts [0, 7] eta 1, sample {i}: rel-L2 vs its own single run {e:.3e} (bitwise: {torch.equal(both[i:i + 1], one)})')
        assert e < 2e-2, (i, e)


def test_held_samples_with_multistep_lengths_and_guidance(lib):
    """eta 0, dpmpp_2m, lengths [96, 77], guidance [5, 0], starts [0, 7]: each row against its own single run at its own length and start; padded frames
    exactly 0 in latents and history; the history of the held sample, NaN-filled on entry, is still NaN when its start step is reached."""
    from ezaudio_amd.sampler import LatentSampler
    m = get_model('xs', 1)
    rows = [_row('smp_xs'), _row('smp_xs_b')]
    lens, gs, starts, steps, nan = [96, 77], [5.0, 0.0], [0, 7], 20, np.float32(np.nan)
    cl = (1.5 * uniform_pm1('start.clean2', 2 * 128 * 96, 3)).reshape(2, 128, 96).astype(np.float32)

    def prep(sel, lengths, guidance):
        L = max(lengths)
        text, tm = t_(np.stack([rows[i]['ctx'][0] for i in sel])), t_(np.stack([rows[i]['mask'][0] for i in sel]))
        un, um = t_(np.stack([rows[i]['ctx'][1] for i in sel])), t_(np.stack([rows[i]['mask'][1] for i in sel]))
        init, clean = np.full((len(sel), 128, L), nan, np.float32), np.full((len(sel), 128, L), nan, np.float32)
        for j, (i, n) in enumerate(zip(sel, lengths)):
            init[j, :, :n] = rows[i]['init'][0, :, :n]
            clean[j, :, :n] = cl[i, :, :n]
        smp = LatentSampler(m, _scheduler(steps))
        smp.prepare(text, tm, un, um, t_(init), None, guidance, 0.75, steps, 0.0, solver='dpmpp_2m', init_latents=t_(clean),
                    start_steps=[starts[i] for i in sel], latent_scale=SCALE, latent_shift=SHIFT,
                    **(dict(lengths=lengths) if len(set(lengths)) > 1 else {}))
        return smp
    try:
        smp = prep([0, 1], lens, gs)
        with torch.cuda.stream(smp.stream):
            smp.x0_hist[1] = float('nan')
        smp.run(7)
        smp.stream.synchronize()
        assert torch.isnan(smp.x0_hist[1]).all(), 'the history of a held sample is not written'
        assert torch.isfinite(smp.x0_hist[0]).all() and torch.equal(smp.latents[1, :, 77:], torch.zeros_like(smp.latents[1, :, 77:]))
        both = _finish(smp, pieces=[steps - 7])
        hist = smp.x0_hist.clone()
        assert torch.isfinite(both).all() and torch.isfinite(hist).all()
        for i in range(2):
            one = _finish(prep([i], [lens[i]], gs[i] or None))
            e = rel_l2(both[i, :, :lens[i]].cpu().numpy(), one[0].cpu().numpy())
            record(f'dpmpp_2m lengths {lens} guidance {gs} starts {starts} row {i}: rel-L2 vs its own single run {e:.3e} '
                   f'(bitwise: {torch.equal(both[i, :, :lens[i]], one[0])})')
            assert e < 2e-2, (i, e)
            for what, t in (('latent', both), ('history', hist)):
                assert torch.equal(t[i, :, lens[i]:], torch.zeros_like(t[i, :, lens[i]:])), f'padded {what} frames must be exactly 0'
    finally:
        m.set_lengths(None)


# ---------------------------------------------------------------------------------------------------
# 5. strength 1
# ---------------------------------------------------------------------------------------------------
def test_every_start_zero_is_bitwise_the_plain_call(lib):
    inp, init, meta, clean = _case()
    plain = _finish(_prepare(P=2))
    smp = _prepare(P=2, starts=[0, 0], clean=torch.full((2, 128, meta['L']), float('nan'), device='cuda:0'))
    assert smp.first_step == 0
    assert torch.equal(_finish(smp), plain) and torch.isfinite(plain).all()
    with pytest.raises(ValueError, match='together'):
        smp.prepare(None, None, None, None, t_(init), None, 3.5, 0.0, 20, 0.0, start_steps=7)
    with pytest.raises(ValueError, match='together'):
        smp.prepare(None, None, None, None, t_(init), None, 3.5, 0.0, 20, 0.0, init_latents=t_(clean))
    for bad in (dict(start_steps=20), dict(start_steps=-1), dict(start_steps=[7, 7])):
        with pytest.raises(ValueError, match='start'):
            smp.prepare(None, None, None, None, t_(init), None, 3.5, 0.0, 20, 0.0, init_latents=t_(clean), **bad)
    with pytest.raises(ValueError, match='init_latents'):
        smp.prepare(None, None, None, None, t_(init), None, 3.5, 0.0, 20, 0.0, init_latents=t_(clean)[:, :, :50], start_steps=7)


# ---------------------------------------------------------------------------------------------------
# 6. refusals, off, ezdit_set_step
# ---------------------------------------------------------------------------------------------------
def test_set_start_refusals_off_and_set_step(lib):
    from ezaudio_amd import _lib
    from oracle.weights import model_config
    inp, init, meta, clean = _case()
    K = meta['steps']
    m = get_model('xs', 1)
    arr = lambda v: (C.c_int32 * len(v))(*v)   # noqa: E731
    # before ezdit_sampler_begin (a fresh handle)
    cfg = model_config('xs')
    c = _lib.EzditConfig(cfg['embed_dim'], cfg['num_heads'], cfg['depth'], cfg['in_chans'], cfg['out_chans'], cfg['context_dim'],
                         cfg['ada_sola_rank'], float(cfg['ada_sola_alpha']), float(cfg['mlp_ratio']), 2048)
    h = C.c_void_p()
    assert lib.ezdit_create(C.byref(c), C.byref(h)) == 0
    try:
        assert lib.ezdit_sampler_set_start(h, arr([0, 7]), 2, None) == -3 and b'ezdit_sampler_begin' in lib.ezdit_last_error()
    finally:
        lib.ezdit_destroy(h)

    plain = _finish(_prepare(P=2))
    cl2 = t_(clean).repeat(2, 1, 1)
    smp = _prepare(P=2, starts=[0, 7], clean=cl2)
    st = C.c_void_p(smp.stream.cuda_stream)
    smp.stream.synchronize()
    noised = smp.latents.clone()
    two = _finish(smp)
    assert not torch.equal(two[1], plain[1]) and torch.equal(two[0], plain[0])

    def rewind(k=0, lat=noised):
        with torch.cuda.stream(smp.stream):
            smp.latents.copy_(lat)
            return lib.ezdit_set_step(m._h, k, st)

    def in_capture():
        x = torch.zeros(8, device='cuda:0')
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=smp.stream):
            x.add_(1.0)
            rc = lib.ezdit_sampler_set_start(m._h, arr([3, 3]), 2, st)
        return rc
    for what, call, rc in (('wrong P', lambda: lib.ezdit_sampler_set_start(m._h, arr([0, 7, 7]), 3, st), -1),
                           ('negative', lambda: lib.ezdit_sampler_set_start(m._h, arr([0, -1]), 2, st), -1),
                           ('n_steps', lambda: lib.ezdit_sampler_set_start(m._h, arr([K, 7]), 2, st), -1),
                           ('capture', in_capture, -3),
                           ('set_step(7)', lambda: lib.ezdit_set_step(m._h, 7, st), -3),
                           ('set_step(3)', lambda: lib.ezdit_set_step(m._h, 3, st), -3)):
        assert call() == rc, what
        assert lib.ezdit_last_error()
        assert rewind() == 0                                            # a rewind to min(start_steps) is fine
        assert torch.equal(_finish(smp), two), what                     # the refused call left nothing behind
    # new values keep working on the same sampler: a uniform table is the run of test 2, and set_step follows min(start_steps)
    assert lib.ezdit_sampler_set_start(m._h, arr([7, 7]), 2, st) == 0
    assert _step_counter(m) == 7
    assert lib.ezdit_set_step(m._h, 0, st) == -3 and rewind(7, torch.cat([noised[1:2], noised[1:2]])) == 0
    with torch.cuda.stream(smp.stream):
        assert lib.ezdit_sampler_run(m._h, K - 7, 1, st) == 0
    smp.stream.synchronize()
    assert torch.equal(smp.latents[0:1], _from_seven()) and torch.equal(smp.latents[1:2], _from_seven())
    # the multistep solver in either order with the table; a rewind to the run's first step is accepted with it on
    hist = torch.full_like(smp.latents, float('nan'))
    ch = _scheduler(K).multistep_coefficients()
    assert lib.ezdit_sampler_set_multistep(m._h, (C.c_float * K)(*ch), K, hist.data_ptr(), st) == 0
    assert lib.ezdit_set_step(m._h, 0, st) == -3 and rewind(7, torch.cat([noised[1:2], noised[1:2]])) == 0
    with torch.cuda.stream(smp.stream):
        assert lib.ezdit_sampler_run(m._h, K - 7, 1, st) == 0
    smp.stream.synchronize()
    got = smp.latents.clone()
    ms7 = _finish(_prepare('dpmpp_2m', starts=7, clean=t_(clean)))
    assert torch.isfinite(hist).all() and torch.equal(got[0:1], ms7) and torch.equal(got[1:2], ms7)
    smp = _prepare(P=2, starts=[0, 7], clean=cl2)                        # (the line above re-prepared the model: begin again)
    st = C.c_void_p(smp.stream.cuda_stream)
    # NULL switches the table off: the plain run from step 0, bit for bit, and ezdit_set_step has its old rules again
    assert lib.ezdit_sampler_set_start(m._h, None, 0, st) == 0
    assert _step_counter(m) == 0
    with torch.cuda.stream(smp.stream):
        smp.latents.copy_(t_(init).expand_as(smp.latents))
        assert lib.ezdit_sampler_run(m._h, K, 1, st) == 0
    smp.stream.synchronize()
    assert torch.equal(smp.latents, plain)
    assert lib.ezdit_set_step(m._h, 3, st) == 0


# ---------------------------------------------------------------------------------------------------
# 7. end to end: inference(init_latents=, strength=) and EzAudio.audio_to_audio with the mini VAE and a stand-in text encoder
#    (the EzAudio('mini', ...) of tests/test_editing_batch_gpu.py; the helpers are copied, not imported from a test module)
# ---------------------------------------------------------------------------------------------------
MINI_VAE = dict(channels=64, c_mults=[1, 2], strides=[2, 4], latent_dim=128, out_channels=1)
SR = 24000


def _mini_autoencoder(device='cuda'):
    from ezaudio_amd.vae import Autoencoder
    cfg = MINI_VAE
    sd = {k: torch.from_numpy(v) for k, v in V.make_vae_state_dict(cfg, 5).items()}
    sd.update({k: torch.from_numpy(v) for k, v in V.make_vae_state_dict(cfg, 5, encoder=True).items()})
    common = dict(channels=cfg['channels'], c_mults=cfg['c_mults'], strides=cfg['strides'], use_snake=True)
    config = {'model': {'encoder': {'type': 'oobleck', 'config': dict(in_channels=1, latent_dim=2 * cfg['latent_dim'], **common)},
                        'decoder': {'type': 'oobleck', 'config': dict(out_channels=1, latent_dim=cfg['latent_dim'], final_tanh=False, **common)},
                        'bottleneck': {'type': 'vae'}}}
    return Autoencoder(model_type='stable_vae', quantization_first=True, config=config, state_dict=sd, device=device)


class _Tok:
    """Stand-in for T5Tokenizer (no checkpoints offline): deterministic ids, per-prompt valid length."""

    def __call__(self, texts, max_length, padding, truncation, return_tensors):
        ids = torch.zeros(len(texts), max_length, dtype=torch.long)
        mask = torch.zeros(len(texts), max_length, dtype=torch.long)
        for i, t in enumerate(texts):
            n = max(1, min(max_length, len(t.split()) + 1))
            ids[i, :n] = torch.tensor([(j % 97) + 1 for j in range(len(t), len(t) + n)])
            mask[i, :n] = 1
        return type('Batch', (), dict(input_ids=ids, attention_mask=mask))()


class _Enc:
    def __init__(self, dim):
        self.dim = dim

    def __call__(self, input_ids, attention_mask):
        g = torch.Generator().manual_seed(7)
        table = torch.randn(128, self.dim, generator=g).to(input_ids.device)
        return type('Out', (), dict(last_hidden_state=table[input_ids % 128]))()


WAV_A = (0.3 * uniform_pm1('a2a_a', 2400, 9)).astype(np.float32)        # 300 latent frames of the mini VAE (ratio 8)
WAV_B = (0.7 * uniform_pm1('a2a_b', 1203, 10)).astype(np.float32)       # 150 frames and a remainder of 3 samples


@pytest.fixture(scope='module')
def ez(tmp_path_factory):
    import yaml
    import ezaudio_amd
    from ezaudio_amd import api as A
    from ezaudio_amd.config import load_yaml_with_includes
    from oracle.weights import make_state_dict, model_config
    tmp = tmp_path_factory.mktemp('a2a')
    params = load_yaml_with_includes(os.path.join(os.path.dirname(ezaudio_amd.__file__), 'configs', 'ezaudio-xl.yml'))
    cfg = model_config('xs')
    params['model'] = dict(cfg)
    params['text_encoder']['dim'] = cfg['context_dim']
    yml = tmp / 'mini.yml'
    with open(yml, 'w') as f:
        yaml.safe_dump(params, f)
    sd = {k: torch.from_numpy(v) for k, v in make_state_dict(cfg, 1).items()}
    with pytest.MonkeyPatch.context() as mp:
        mp.setitem(A.configs, 'mini', {'path': str(tmp / 'none.pt'), 'url': '', 'config': str(yml)})
        mp.setitem(sys.modules, 'librosa', types.SimpleNamespace(load=lambda f, sr: (WAV_B.copy(), sr)))   # librosa is absent offline; the API uses load() only
        yield A.EzAudio('mini', autoencoder=_mini_autoencoder(), tokenizer=_Tok(), text_encoder=_Enc(cfg['context_dim']), state_dict=sd)


def test_inference_with_a_clip_and_per_prompt_strength(ez):
    from ezaudio_amd.sampler import inference
    L = 96
    torch.manual_seed(5)
    latent = ez.autoencoder(audio=torch.from_numpy(WAV_A[:L * 8]).reshape(1, 1, -1).cuda())
    assert latent.shape == (1, 128, L)
    args = (ez.autoencoder, ez.unet, None, None, ez.tokenizer, ez.text_encoder, ez.params, ez.noise_scheduler, ['rain on a roof', 'a dog barking twice'], None,
            L, 3.5, 0.5, 20, 1, [3, 8], 'cuda')
    plain = inference(*args)
    mixed = inference(*args, init_latents=latent, strength=[1.0, 0.5])
    assert mixed.shape == plain.shape == (2, 1, L * 8) and torch.isfinite(mixed).all()
    e = rel_l2(mixed[0].cpu().numpy(), plain[0].cpu().numpy())
    record(f'inference strength [1.0, 0.5]: sample 0 vs the plain batched call rel-L2 {e:.3e} (bitwise: {torch.equal(mixed[0], plain[0])})')
    assert e < 2e-2
    assert rel_l2(mixed[1].cpu().numpy(), plain[1].cpu().numpy()) > 1e-2      # sample 1 really started from the clip
    assert torch.equal(inference(*args, init_latents=latent, strength=1.0), plain)   # strength 1 for everybody: the plain call


def test_audio_to_audio_batch_and_single(ez):
    req = dict(ddim_steps=20, guidance_scale=[3.5, 2.0], guidance_rescale=[0.75, 0.0], eta=[1, 0], random_seed=[3, 8])
    torch.manual_seed(21)
    sr, outs = ez.audio_to_audio(['rain on a roof', 'a dog barking twice'], [WAV_A, 'b.wav'], strength=[0.5, 0.3], **req)
    assert sr == SR and isinstance(outs, list) and [o.shape for o in outs] == [(2400,), (1200,)]
    assert all(np.isfinite(o).all() and o.std() > 0 for o in outs)
    torch.manual_seed(21)
    one = {k: (v[0] if isinstance(v, list) else v) for k, v in req.items()}
    sr, single = ez.audio_to_audio('rain on a roof', WAV_A, strength=0.5, **one)
    assert single.shape == (2400,) and np.isfinite(single).all()
    e = rel_l2(outs[0], single)
    record(f'audio_to_audio request 0 of a batch of two (300 and 150 frames): rel_l2 {e:.3e} to its single call')
    assert e < 5e-2                                                      # the gate of tests/test_editing_batch_gpu.py for a request against its single call
    torch.manual_seed(21)
    sr, batch1 = ez.audio_to_audio(['rain on a roof'], [WAV_A], strength=[0.5], **{k: ([v[0]] if isinstance(v, list) else v) for k, v in req.items()})
    assert len(batch1) == 1 and np.array_equal(batch1[0], single)        # a batch of one is the single call, bit for bit
    with pytest.raises(ValueError, match='latent frame'):
        ez.audio_to_audio('rain', WAV_A[:7])
