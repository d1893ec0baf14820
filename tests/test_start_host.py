"""CPU tests of the host side of audio-to-audio (a sampler run that starts at a per-request step from a noised clip): DDIMScheduler.start_step, draw_noises with
start steps, EzAudio.audio_to_audio's validation and batched bookkeeping against a recording sampler and a stub VAE (the pattern of
tests/test_editing_batch_host.py; the stand-ins are copied, not imported from a test module), and the two new entry points of the C ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from ezaudio_amd.sampler import LatentSampler as _RealSampler
from ezaudio_amd.vae import Autoencoder
from tests.util import DIFF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {'text_encoder': {'max_length': 8}, 'model': {'out_chans': 4},
          'autoencoder': {'scale': 0.5, 'shift': -0.25, 'sr': 80, 'latent_sr': 10, 'dim': 4}}
SR, RATIO, DIM = 80, 8, 4


def _scheduler(steps=None):
    from ezaudio_amd.scheduler import DDIMScheduler
    sch = DDIMScheduler(**DIFF)
    if steps is not None:
        sch.set_timesteps(steps)
    return sch


# ---------------------------------------------------------------------------------------------------
# 1. strength -> start step
# ---------------------------------------------------------------------------------------------------
def test_start_step_maps_strength_to_the_first_step_rounded_half_up():
    sch = _scheduler(50)
    assert [sch.start_step(s) for s in (1, 0.75, 0.5, 0.3)] == [0, 12, 25, 35]
    sch.set_timesteps(100)
    assert 100 - sch.start_step(0.29) == 29 and int(100 * 0.29) == 28           # int() alone loses a step
    assert [sch.start_step(s) for s in (1.0, 0.5, 0.01, 0.005)] == [0, 50, 99, 99]
    sch.set_timesteps(20)
    assert [sch.start_step(s) for s in (1.0, 0.65, 0.5, 0.05, 0.025)] == [0, 7, 10, 19, 19]
    for K, bad in ((20, 0.0), (20, -0.1), (20, 1.01), (20, float('nan')), (20, 0.02), (50, 0.009), (100, 0.004)):
        sch.set_timesteps(K)
        with pytest.raises(ValueError):
            sch.start_step(bad)
    with pytest.raises(ValueError):
        _scheduler().start_step(0.5)                                            # no timesteps yet


def test_start_zero_of_the_shipped_schedule_is_exactly_noise():
    """What makes "strength 1" the plain call bit for bit: (sa, sb) of step 0 is exactly (0, 1), the row ezdit_add_noise leaves alone."""
    for K in (20, 50, 100):
        sch = _scheduler(K)
        assert float(sch.alphas_cumprod[999]) == 0.0
        assert sch.ddim_coefficients(1.0)[0][:2] == (0.0, 1.0) and sch.ddim_coefficients(0.0)[0][:2] == (0.0, 1.0)


# ---------------------------------------------------------------------------------------------------
# 2. the draws
# ---------------------------------------------------------------------------------------------------
def test_draw_noises_with_start_steps_draws_what_the_single_call_draws():
    from ezaudio_amd.sampler import draw_noises
    K = 20
    init, step = draw_noises(4, 6, K, [1, 1], [11, 12], 'cpu', n_prompts=2, start_steps=[0, 7])
    one_i, one_s = draw_noises(4, 6, K, 1, 12, 'cpu', n_prompts=1, start_steps=[7])
    assert step.shape == (K, 2, 4, 6) and one_s.shape == (K, 1, 4, 6)
    assert torch.equal(init[1:2], one_i)
    assert torch.equal(step[7:, 1:2], one_s[7:]) and not step[:7, 1].any() and not one_s[:7].any()
    # ... which are the first 13 step draws of that seed's generator after the init noise, at steps 7 .. 19
    g = torch.Generator().manual_seed(12)
    assert torch.equal(torch.randn((1, 4, 6), generator=g), one_i)
    for k in range(7, K):
        assert torch.equal(torch.randn((1, 4, 6), generator=g), step[k, 1:2]), k
    # sample 0 starts at 0: the draws of the call without start steps
    plain_i, plain_s = draw_noises(4, 6, K, 1, 11, 'cpu', n_prompts=1)
    assert torch.equal(init[0:1], plain_i) and torch.equal(step[:, 0:1], plain_s)
    # eta 0 draws nothing per step, lengths are honoured, a list of the wrong size is refused
    i3, s3 = draw_noises(4, [6, 3], K, [0, 1], [11, 12], 'cpu', n_prompts=2, start_steps=[3, 18])
    assert not s3[:, 0].any() and not s3[:18, 1].any() and s3[18:, 1, :, :3].abs().min() > 0 and not s3[:, 1, :, 3:].any()
    with pytest.raises(ValueError):
        draw_noises(4, 6, K, 1, 1, 'cpu', n_prompts=2, start_steps=[7])


# ---------------------------------------------------------------------------------------------------
# 3. EzAudio.audio_to_audio against stand-ins
# ---------------------------------------------------------------------------------------------------
class _RecordingSampler:
    """Honours the contract of the real one (each sample a function of its own valid frames, zero beyond) and keeps what prepare() was given."""
    seen = []

    def __init__(self, unet, scheduler):
        pass

    def prepare(self, text, text_mask, uncond, uncond_mask, init, step_noises, gs, gr, steps, eta, gt=None, gt_mask=None,
                controlnet=None, condition=None, conditioning_scale=1.0, **kw):
        P, _, L = init.shape
        lengths = kw.get('lengths') or [L] * P
        lat = init + text.mean(dim=(1, 2))[:, None, None]
        for i, n in enumerate(lengths):
            lat[i, :, n:] = 0
        self.lat = lat
        _RecordingSampler.seen.append(dict(P=P, L=L, init=init.clone(), step_noises=step_noises, gt=gt, kw=dict(kw), gs=gs, gr=gr, eta=eta, steps=steps))

    def run(self, use_graph=True):
        pass

    def finish(self):
        return self.lat


class _Tok:
    def __call__(self, texts, max_length, padding, truncation, return_tensors):
        ids = torch.tensor([[len(t) + 1, (sum(map(ord, t)) % 50) + 1] + [0] * (max_length - 2) for t in texts])
        return type('B', (), dict(input_ids=ids, attention_mask=(ids > 0).long()))()


def _enc(input_ids, attention_mask):
    return type('O', (), dict(last_hidden_state=torch.sin(input_ids.float())[:, :, None].repeat(1, 1, 6)))()


class _Unet:
    def eval(self):
        return self


class _StubVAE(Autoencoder):
    """ezaudio_amd.vae.Autoencoder on the CPU: frame means as the latent (no bottleneck noise: these tests compare what is passed on)."""

    def __init__(self):
        self.calls = []

    def latent_lengths(self, lengths):
        return [int(v) // RATIO for v in lengths]

    def __call__(self, audio=None, embedding=None, lengths=None):
        if audio is not None:
            self.calls.append(('encode', tuple(audio.shape), None if lengths is None else list(lengths)))
            N, _, T = audio.shape
            lens = self.latent_lengths(lengths if lengths is not None else [T] * N)
            L = max(lens)
            z = audio[:, 0, :L * RATIO].reshape(N, L, RATIO).mean(-1)[:, None, :].repeat(1, DIM, 1)
            for i, n in enumerate(lens):
                z[i, :, n:] = 0
            return z
        self.calls.append(('decode', tuple(embedding.shape), None if lengths is None else list(lengths)))
        return embedding.repeat_interleave(RATIO, dim=2)[:, :1].clone()


def _ez():
    from ezaudio_amd import api
    ez = api.EzAudio.__new__(api.EzAudio)
    ez.device = 'cpu'
    ez.autoencoder, ez.unet, ez.tokenizer, ez.text_encoder, ez.noise_scheduler, ez.params = _StubVAE(), _Unet(), _Tok(), _enc, _scheduler(), PARAMS
    return ez


def _wave(n, seed, amp):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


@pytest.fixture()
def seen(monkeypatch):
    from ezaudio_amd import sampler as S
    monkeypatch.setattr(S, 'LatentSampler', _RecordingSampler)
    _RecordingSampler.seen.clear()
    return _RecordingSampler.seen


PROMPTS = ['a dog barking', 'rain', '']
CLIPS = [_wave(203, 1, 0.9), _wave(120, 2, 0.1), _wave(165, 3, 0.5)]          # 25, 15 and 20 whole latent frames (two clips with a remainder)
SETTINGS = dict(strength=[0.5, 1.0, 0.3], guidance_scale=[5, 2.0, 4.0], guidance_rescale=[0.75, 0.5, 0.25], eta=[1, 0.5, 0], random_seed=[11, 12, 13])


def test_batched_audio_to_audio_is_one_call_of_each_kind_and_passes_what_the_single_calls_pass(seen):
    ez = _ez()
    sr, outs = ez.audio_to_audio(PROMPTS, CLIPS, ddim_steps=20, **SETTINGS)
    assert sr == SR and isinstance(outs, list) and len(seen) == 1
    assert [o.shape for o in outs] == [(200,), (120,), (160,)]                  # each trimmed to its own latent_frames * ratio
    assert ez.autoencoder.calls == [('encode', (3, 1, 203), [203, 120, 165]), ('decode', (3, 4, 25), [25, 15, 20])]
    b = seen[0]
    kw = b['kw']
    assert b['P'] == 3 and b['L'] == 25 and b['steps'] == 20 and b['gt'] is None
    assert kw['lengths'] == [25, 15, 20] and kw['start_steps'] == [10, 0, 14] and (kw['latent_scale'], kw['latent_shift']) == (0.5, -0.25)
    assert set(kw) == {'lengths', 'start_steps', 'init_latents', 'latent_scale', 'latent_shift'}
    assert b['gs'] == [5, 2.0, None] and b['gr'] == [0.75, 0.5, 0.25] and b['eta'] == [1, 0.5, 0]      # '' runs without guidance
    assert kw['init_latents'].shape == (3, 4, 25)
    sn = b['step_noises']
    assert not sn[:10, 0].any() and sn[10:, 0].abs().sum() > 0 and sn[:, 1, :, :15].abs().min() > 0 and not sn[:, 2].any()
    batch_outs = [o.copy() for o in outs]
    seen.clear()
    for i in range(3):
        ez1 = _ez()
        sr, one = ez1.audio_to_audio(PROMPTS[i], CLIPS[i], ddim_steps=20, **{k: v[i] for k, v in SETTINGS.items()})
        s, n = seen[i], [25, 15, 20][i]
        assert s['P'] == 1 and s['L'] == n and s['kw']['start_steps'] == [[10, 0, 14][i]] and 'lengths' not in s['kw']
        assert ez1.autoencoder.calls == [('encode', (1, 1, len(CLIPS[i])), None), ('decode', (1, 4, n), None)]
        assert torch.equal(kw['init_latents'][i:i + 1, :, :n], s['kw']['init_latents']) and not kw['init_latents'][i, :, n:].any()
        assert torch.equal(b['init'][i:i + 1, :, :n], s['init'])                                        # the request's own seed
        if SETTINGS['eta'][i]:
            assert torch.equal(sn[:, i:i + 1, :, :n], s['step_noises'])
        assert (s['gs'], s['gr'], s['eta']) == ([5, 2.0, None][i], SETTINGS['guidance_rescale'][i], SETTINGS['eta'][i])
        assert isinstance(one, np.ndarray) and one.shape == batch_outs[i].shape and np.array_equal(one, batch_outs[i])
    # the clip is peak-normalised before it is encoded: a scaled copy encodes to the same latent
    seen.clear()
    _ez().audio_to_audio('rain', 3.0 * CLIPS[1], ddim_steps=20, strength=0.5, random_seed=1)
    _ez().audio_to_audio('rain', CLIPS[1], ddim_steps=20, strength=0.5, random_seed=1)
    assert torch.allclose(seen[0]['kw']['init_latents'], seen[1]['kw']['init_latents'], rtol=0, atol=1e-6)


def test_one_shared_clip_and_scalar_settings_broadcast(seen):
    ez = _ez()
    sr, outs = ez.audio_to_audio(PROMPTS[:2], CLIPS[0], strength=0.5, ddim_steps=50, random_seed=[1, 2], eta=0, solver='dpmpp_2m')
    assert len(outs) == 2 and len(seen) == 1 and [o.shape for o in outs] == [(200,), (200,)]
    assert ez.autoencoder.calls == [('encode', (2, 1, 203), [203, 203]), ('decode', (2, 4, 25), None)]   # equal lengths: the unpadded batch
    kw = seen[0]['kw']
    assert kw['start_steps'] == [25, 25] and 'lengths' not in kw and kw['solver'] == 'dpmpp_2m' and seen[0]['step_noises'] is None
    assert torch.equal(kw['init_latents'][0], kw['init_latents'][1])
    import random
    random.seed(4)
    ez.audio_to_audio(PROMPTS[:2], CLIPS[0], ddim_steps=20, randomize_seed=True)
    assert not torch.equal(seen[1]['init'][0], seen[1]['init'][1])                                       # one seed per request
    sr, outs = ez.audio_to_audio(['rain'], [CLIPS[1]], ddim_steps=20, random_seed=5)
    sr, one = ez.audio_to_audio('rain', CLIPS[1], ddim_steps=20, random_seed=5)
    assert isinstance(outs, list) and len(outs) == 1 and np.array_equal(outs[0], one)


def test_audio_to_audio_refuses_bad_arguments_before_anything_runs(seen):
    ez = _ez()
    two = dict(text=PROMPTS[:2], audio=CLIPS[:2], ddim_steps=20)
    for kw in (dict(audio=CLIPS), dict(audio=CLIPS[:1]), dict(strength=[0.5]), dict(strength=[0.5, 0.5, 0.5]), dict(guidance_scale=[3.5]),
               dict(guidance_rescale=[0.5, 0.5, 0.5]), dict(eta=[1]), dict(random_seed=[1, 2, 3]), dict(ddim_steps=[20, 20]),
               dict(strength=[0.5, 0.0]), dict(strength=1.5), dict(strength=[0.5, 0.01]), dict(solver='dpmpp_2m'), dict(solver='unipc'),
               dict(audio=[np.zeros((2, 50), np.float32), CLIPS[1]]), dict(audio=[CLIPS[0], _wave(RATIO - 1, 4, 0.5)]), dict(text=[], audio=[])):
        with pytest.raises(ValueError):
            ez.audio_to_audio(**{**two, **kw})
    one = dict(text='rain', audio=CLIPS[0], ddim_steps=20)
    for kw in (dict(audio=CLIPS[:1]), dict(strength=[0.5]), dict(guidance_scale=[3.5]), dict(random_seed=[1]), dict(ddim_steps=[20]), dict(strength=0),
               dict(audio=_wave(RATIO - 1, 4, 0.5)), dict(audio=np.zeros((1, 80), np.float32))):
        with pytest.raises(ValueError):
            ez.audio_to_audio(**{**one, **kw})
    assert not seen and not ez.autoencoder.calls                            # refused before anything was encoded or sampled
    ez.autoencoder = lambda audio=None, embedding=None: None                # the reference's surface only: no ragged encode to batch on
    with pytest.raises(NotImplementedError):
        ez.audio_to_audio(**two)


def test_inference_and_prepare_want_the_clip_and_the_strength_together(seen):
    from ezaudio_amd.sampler import inference
    ez = _ez()
    args = (ez.autoencoder, ez.unet, None, None, ez.tokenizer, ez.text_encoder, PARAMS, ez.noise_scheduler, ['rain', 'wind'], None, 6, 3, 0.0, 20, 0, 1, 'cpu')
    lat = torch.zeros(2, 4, 6)
    for kw in (dict(init_latents=lat), dict(strength=0.5), dict(init_latents=lat, strength=[0.5]), dict(init_latents=torch.zeros(2, 4, 5), strength=0.5),
               dict(init_latents=torch.zeros(3, 4, 6), strength=0.5)):
        with pytest.raises(ValueError):
            inference(*args, **kw)
    assert not seen
    inference(*args, init_latents=lat[:1], strength=[1.0, 0.5])                # one shared row is passed on as it is
    assert seen[0]['kw']['start_steps'] == [0, 10] and seen[0]['kw']['init_latents'].shape == (1, 4, 6)
    import inspect
    sig = inspect.signature(_RealSampler.prepare).parameters
    assert [sig[k].default for k in ('init_latents', 'start_steps', 'latent_scale', 'latent_shift')] == [None, None, 1.0, 0.0]


# ---------------------------------------------------------------------------------------------------
# 4. ABI
# ---------------------------------------------------------------------------------------------------
def test_the_header_declares_and_the_binding_binds_the_start_entry_points(lib):
    from ezaudio_amd import _lib
    from oracle.weights import model_config
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ezdit.h')).read(), flags=re.S)
    for name, nargs in (('ezdit_add_noise', 10), ('ezdit_sampler_set_start', 4)):
        m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', hdr)
        assert m and len(m.group(1).split(',')) == nargs, name
        res, args = _lib.PROTOTYPES[name]
        assert res is C.c_int and len(args) == nargs
        assert getattr(lib, name).argtypes == args
    assert '#define EZDIT_ABI_VERSION 4' in hdr and lib.ezdit_abi_version() == 4 and _lib.ABI_VERSION == 4    # additive: the version stays
    cfg = model_config('xs')
    c = _lib.EzditConfig(cfg['embed_dim'], cfg['num_heads'], cfg['depth'], cfg['in_chans'], cfg['out_chans'], cfg['context_dim'],
                         cfg['ada_sola_rank'], float(cfg['ada_sola_alpha']), float(cfg['mlp_ratio']), 2048)
    h = C.c_void_p()
    assert lib.ezdit_create(C.byref(c), C.byref(h)) == 0
    try:
        st = (C.c_int32 * 2)(0, 7)
        assert lib.ezdit_sampler_set_start(h, st, 2, None) == -3 and b'ezdit_sampler_begin' in lib.ezdit_last_error()
        assert lib.ezdit_sampler_set_start(h, None, 0, None) == -3
        assert lib.ezdit_sampler_set_start(None, st, 2, None) == -1
        # the table costs at most 1 KB of workspace
        assert lib.ezdit_workspace_bytes(h, 2, 96, 20, 20) > 0
    finally:
        lib.ezdit_destroy(h)
    assert lib.ezdit_add_noise(None, None, None, 1.0, 0.0, None, 96, 1, 128 * 96, None) == -1
