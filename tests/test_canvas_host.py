"""CPU tests of the host side of long-form generation (overlapping windows of one canvas, blended inside the step): canvas_windows, draw_noises with canvas
offsets, EzAudio.generate_long_audio's bookkeeping against a recording sampler and a stub VAE (the pattern of tests/test_start_host.py; the stand-ins are
copied, not imported from a test module), the keyword order of inference() and the two new entry points of the C ABI."""
import ctypes as C
import inspect
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


def _scheduler():
    from ezaudio_amd.scheduler import DDIMScheduler
    return DDIMScheduler(**DIFF)


# ---------------------------------------------------------------------------------------------------
# 1. the windows
# ---------------------------------------------------------------------------------------------------
def test_canvas_windows_cover_the_canvas_with_the_minimum_overlap():
    from ezaudio_amd.sampler import canvas_windows, check_canvas
    assert canvas_windows(1500, 500, 125) == ([0, 333, 667, 1000], 500)
    assert canvas_windows(500, 500, 125) == ([0], 500) and canvas_windows(77, 500, 125) == ([0], 77)      # T <= L: the plain call
    assert canvas_windows(501, 500, 125) == ([0, 1], 500)
    assert canvas_windows(1000, 500, 0) == ([0, 500], 500)                                                # no overlap asked for, none made
    assert canvas_windows(200, 96, 44) == ([0, 52, 104], 96)
    for T, L, O in ((1500, 500, 125), (1501, 500, 125), (3000, 500, 250), (875, 500, 125), (876, 500, 125), (200, 96, 44), (157, 96, 1), (1000, 97, 48),
                    (12345, 500, 0), (2048, 500, 249)):
        offs, win = canvas_windows(T, L, O)
        assert win == L and offs[0] == 0 and offs[-1] + L == T, (T, L, O)
        steps = [b - a for a, b in zip(offs, offs[1:])]
        assert min(steps) >= 1 and max(steps) <= L - O, (T, L, O, offs)                                   # ascending; every neighbouring overlap >= O
        assert max(steps) - min(steps) <= 1                                                              # spread evenly
        assert len(offs) == -(-(T - O) // (L - O))                                                       # the fewest windows that can do it
        check_canvas(offs, L, T, max(1, O))
    for bad in ((1500, 500, -1), (1500, 500, 251), (0, 500, 125), (1500, 0, 0)):
        with pytest.raises(ValueError):
            canvas_windows(*bad)
    for offs, L, T, ramp in (([1, 50], 96, 146, 1), ([0, 97], 96, 193, 1), ([0, 50, 50], 96, 146, 1), ([0, 50], 96, 147, 1), ([0, 50], 96, 146, 0), ([], 96, 96, 1)):
        with pytest.raises(ValueError):
            check_canvas(offs, L, T, ramp)


# ---------------------------------------------------------------------------------------------------
# 2. the draws
# ---------------------------------------------------------------------------------------------------
def test_draw_noises_with_canvas_offsets_slices_one_canvas_draw():
    from ezaudio_amd.sampler import draw_noises
    K, offs, L = 5, [0, 4, 9], 6
    init, step = draw_noises(4, L, K, 1, 12, 'cpu', n_prompts=3, canvas_offsets=offs)
    assert init.shape == (3, 4, L) and step.shape == (K, 3, 4, L)
    g = torch.Generator().manual_seed(12)
    canvas = torch.randn((1, 4, 15), generator=g)
    for i, o in enumerate(offs):
        assert torch.equal(init[i:i + 1], canvas[:, :, o:o + L])
    assert torch.equal(init[0, :, 4:], init[1, :, :2])                      # the windows share their noise where they share frames
    for k in range(K):
        z = torch.randn((1, 4, 15), generator=g)
        for i, o in enumerate(offs):
            assert torch.equal(step[k, i:i + 1], z[:, :, o:o + L]), (k, i)
    i0, s0 = draw_noises(4, L, K, 0, 12, 'cpu', n_prompts=3, canvas_offsets=offs)
    assert torch.equal(i0, init) and s0 is None                             # eta 0 draws nothing per step
    # one window draws what the plain call draws
    one_i, one_s = draw_noises(4, L, K, 1, 12, 'cpu', n_prompts=1, canvas_offsets=[0])
    plain_i, plain_s = draw_noises(4, L, K, 1, 12, 'cpu', n_prompts=1)
    assert torch.equal(one_i, plain_i) and torch.equal(one_s, plain_s)
    for bad in (dict(eta=[1, 1, 1]), dict(random_seed=[1, 2, 3]), dict(audio_frames=[6, 6, 6]), dict(start_steps=[0, 0, 0])):
        kw = dict(codec_dim=4, audio_frames=L, ddim_steps=K, eta=1, random_seed=12, device='cpu', n_prompts=3, canvas_offsets=offs)
        kw.update(bad)
        with pytest.raises(ValueError):
            draw_noises(**kw)


# ---------------------------------------------------------------------------------------------------
# 3. EzAudio.generate_long_audio against stand-ins
# ---------------------------------------------------------------------------------------------------
class _RecordingSampler:
    """Keeps what prepare() was given; its windows are their init noise plus a per-window constant, its canvas the real assembly rule (lowest window wins)."""
    seen = []

    def __init__(self, unet, scheduler):
        pass

    def prepare(self, text, text_mask, uncond, uncond_mask, init, step_noises, gs, gr, steps, eta, gt=None, gt_mask=None,
                controlnet=None, condition=None, conditioning_scale=1.0, **kw):
        P, _, L = init.shape
        self.lat = init + text.mean(dim=(1, 2))[:, None, None]
        self.canvas = kw.get('canvas')
        _RecordingSampler.seen.append(dict(P=P, L=L, init=init.clone(), step_noises=step_noises, gt=gt, kw=dict(kw), gs=gs, gr=gr, eta=eta, steps=steps,
                                           text=text.clone()))

    def run(self, use_graph=True):
        pass

    def finish(self):
        return self.lat

    def canvas_latents(self):
        offs, T, _ = self.canvas
        out = torch.empty(1, self.lat.shape[1], T)
        for p in reversed(range(len(offs))):
            out[0, :, offs[p]:offs[p] + self.lat.shape[2]] = self.lat[p]
        return out


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
    def __init__(self):
        self.calls = []

    def __call__(self, audio=None, embedding=None, lengths=None):
        self.calls.append(('decode', tuple(embedding.shape), None if lengths is None else list(lengths)))
        return embedding.repeat_interleave(RATIO, dim=2)[:, :1].clone()


def _ez():
    from ezaudio_amd import api
    ez = api.EzAudio.__new__(api.EzAudio)
    ez.device = 'cpu'
    ez.autoencoder, ez.unet, ez.tokenizer, ez.text_encoder, ez.noise_scheduler, ez.params = _StubVAE(), _Unet(), _Tok(), _enc, _scheduler(), PARAMS
    return ez


@pytest.fixture()
def seen(monkeypatch):
    from ezaudio_amd import sampler as S
    monkeypatch.setattr(S, 'LatentSampler', _RecordingSampler)
    _RecordingSampler.seen.clear()
    return _RecordingSampler.seen


def test_generate_long_audio_is_one_sampler_call_and_one_decode(seen):
    from ezaudio_amd.sampler import canvas_windows, draw_noises
    ez = _ez()
    # 30 s at 10 latent frames per second in windows of 10 s that share 2.5 s: 300 frames in windows of 100 sharing >= 25
    offs, L = canvas_windows(300, 100, 25)
    assert offs == [0, 67, 133, 200] and L == 100
    sr, wav = ez.generate_long_audio('rain on a roof', 30, ddim_steps=20, random_seed=7)
    assert sr == SR and isinstance(wav, np.ndarray) and wav.shape == (300 * RATIO,)
    assert len(seen) == 1 and ez.autoencoder.calls == [('decode', (1, DIM, 300), None)]
    b = seen[0]
    assert b['P'] == 4 and b['L'] == 100 and b['steps'] == 20 and b['gt'] is None and (b['gs'], b['gr'], b['eta']) == (5, 0.75, 1)
    assert set(b['kw']) == {'canvas'} and b['kw']['canvas'] == (offs, 300, 33)         # the ramp: the smallest overlap, a cross-fade
    init, step = draw_noises(DIM, 100, 20, 1, 7, 'cpu', n_prompts=4, canvas_offsets=offs)
    assert torch.equal(b['init'], init) and torch.equal(b['step_noises'], step)
    assert torch.equal(b['text'][0], b['text'][3])                                      # one prompt under every window
    # the waveform is the decode of the canvas in VAE space
    canvas = torch.empty(1, DIM, 300)
    lat = init + b['text'].mean(dim=(1, 2))[:, None, None]
    for p in reversed(range(4)):
        canvas[0, :, offs[p]:offs[p] + 100] = lat[p]
    want = (canvas / 0.5 + 0.25).repeat_interleave(RATIO, dim=2)[0, 0].numpy()
    assert np.array_equal(wav, want)
    # one prompt per window, the 2M solver
    seen.clear()
    ez.generate_long_audio(['rain', 'thunder', 'rain', 'birds'], 30, ddim_steps=20, random_seed=7, eta=0, solver='dpmpp_2m')
    assert len(seen) == 1 and seen[0]['kw'] == dict(canvas=(offs, 300, 33), solver='dpmpp_2m') and seen[0]['step_noises'] is None
    assert not torch.equal(seen[0]['text'][0], seen[0]['text'][1]) and torch.equal(seen[0]['text'][0], seen[0]['text'][2])
    # other windows and overlaps reach the sampler as canvas_windows gives them
    seen.clear()
    ez.generate_long_audio('rain', 15, window=10, overlap=5, ddim_steps=20, random_seed=1)
    assert seen[0]['kw']['canvas'] == ([0, 50], 150, 50) and seen[0]['P'] == 2


def test_generate_long_audio_refusals_name_the_window_count(seen):
    ez = _ez()
    with pytest.raises(ValueError, match='4 windows'):
        ez.generate_long_audio(['rain', 'thunder'], 30, ddim_steps=20)
    with pytest.raises(ValueError, match='1 windows'):
        ez.generate_long_audio(['rain', 'thunder'], 10, ddim_steps=20)
    for kw in (dict(guidance_scale=[5] * 4), dict(eta=[1] * 4), dict(random_seed=[1] * 4), dict(guidance_rescale=[0.5] * 4), dict(ddim_steps=[20] * 4),
               dict(solver='dpmpp_2m'), dict(solver='unipc'), dict(overlap=6), dict(overlap=-1)):
        with pytest.raises(ValueError):
            ez.generate_long_audio('rain', 30, **{**dict(ddim_steps=20), **kw})
    with pytest.raises(ValueError):
        ez.generate_long_audio('rain', [30, 30])
    assert not seen and not ez.autoencoder.calls


def test_a_length_within_the_window_is_exactly_generate_audio(seen):
    for length in (10, 7):
        ez = _ez()
        sr, long = ez.generate_long_audio('rain', length, ddim_steps=20, random_seed=3)
        sr2, plain = ez.generate_audio('rain', length, ddim_steps=20, random_seed=3)
        a, b = seen[-2], seen[-1]
        assert sr == sr2 and np.array_equal(long, plain) and long.shape == (length * 10 * RATIO,)
        assert a['kw'] == b['kw'] == {} and (a['P'], a['L'], a['gs'], a['gr'], a['eta'], a['steps']) == (b['P'], b['L'], b['gs'], b['gr'], b['eta'], b['steps'])
        assert torch.equal(a['init'], b['init']) and torch.equal(a['step_noises'], b['step_noises'])
        assert ez.autoencoder.calls[0] == ez.autoencoder.calls[1]


def test_inference_canvas_keywords_and_refusals(seen):
    from ezaudio_amd.sampler import inference
    names = list(inspect.signature(inference).parameters)
    assert names[-3:] == ['canvas_offsets', 'canvas_ramp', 'solver']         # solver stays the last keyword
    sig = inspect.signature(_RealSampler.prepare).parameters
    assert sig['canvas'].default is None and list(sig)[-1] == 'solver'
    ez = _ez()
    args = (ez.autoencoder, ez.unet, None, None, ez.tokenizer, ez.text_encoder, PARAMS, ez.noise_scheduler)
    rest = (None, 6, 3, 0.0, 20, 0, 1, 'cpu')
    out = inference(*args, 'rain', *rest, canvas_offsets=[0, 4, 9], canvas_ramp=1)
    assert out.shape == (1, 1, 15 * RATIO) and seen[0]['kw'] == dict(canvas=([0, 4, 9], 15, 1)) and seen[0]['P'] == 3
    out = inference(*args, ['rain', 'wind', 'sea'], *rest, canvas_offsets=[0, 4, 9])
    assert seen[1]['kw']['canvas'] == ([0, 4, 9], 15, 1)                      # the smallest overlap (9 + ... : 4 + 6 - 9 = 1)
    # one window: the plain call, through the plain code
    one = inference(*args, 'rain', *rest, canvas_offsets=[0])
    plain = inference(*args, 'rain', *rest)
    assert torch.equal(one, plain) and seen[2]['kw'] == seen[3]['kw'] == {}
    n = len(seen)
    lat = torch.zeros(1, 4, 6)
    for text, kw in ((['rain', 'wind'], dict(canvas_offsets=[0, 4, 9])), ('rain', dict(canvas_offsets=[0, 7])), ('rain', dict(canvas_offsets=[1, 4])),
                     ('rain', dict(canvas_offsets=[0, 4, 4])), ('rain', dict(canvas_offsets=[0, 4], canvas_ramp=0)), ('rain', dict(canvas_ramp=2)),
                     ('rain', dict(canvas_offsets=[0, 4], init_latents=lat, strength=0.5))):
        with pytest.raises(ValueError):
            inference(*args, text, *rest, **kw)
    with pytest.raises(ValueError):
        inference(*args[:2], lat, lat.bool(), *args[4:], 'rain', *rest, canvas_offsets=[0, 4])
    with pytest.raises(ValueError):
        inference(*args, 'rain', None, 6, [3, 3], 0.0, 20, 0, 1, 'cpu', canvas_offsets=[0, 4])
    assert len(seen) == n


# ---------------------------------------------------------------------------------------------------
# 4. ABI
# ---------------------------------------------------------------------------------------------------
def test_the_header_declares_and_the_binding_binds_the_canvas_entry_points(lib):
    from ezaudio_amd import _lib
    from oracle.weights import model_config
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ezdit.h')).read(), flags=re.S)
    for name, nargs in (('ezdit_canvas_blend', 8), ('ezdit_sampler_set_canvas', 6)):
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
        off = (C.c_int32 * 2)(0, 50)
        assert lib.ezdit_sampler_set_canvas(h, off, 2, 146, 1, None) == -3 and b'ezdit_sampler_begin' in lib.ezdit_last_error()
        assert lib.ezdit_sampler_set_canvas(h, None, 0, 0, 1, None) == -3
        assert lib.ezdit_sampler_set_canvas(None, off, 2, 146, 1, None) == -1
    finally:
        lib.ezdit_destroy(h)
    # refused before anything is launched: null pointers, ramp 0, a T no table of P windows of L frames can give
    assert lib.ezdit_canvas_blend(None, None, 3, 128, 96, 200, 1, None) == -1
    assert lib.ezdit_canvas_blend(C.c_void_p(256), None, 3, 128, 96, 200, 1, None) == -1
    assert lib.ezdit_canvas_blend(None, C.c_void_p(256), 3, 128, 96, 200, 1, None) == -1
    for P, Cc, L, T, ramp in ((3, 128, 96, 200, 0), (3, 128, 96, 95, 1), (3, 128, 96, 289, 1), (0, 128, 96, 96, 1), (3, 0, 96, 200, 1), (3, 128, 0, 200, 1)):
        assert lib.ezdit_canvas_blend(C.c_void_p(256), C.c_void_p(256), P, Cc, L, T, ramp, None) == -1, (P, Cc, L, T, ramp)
