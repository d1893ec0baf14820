"""CPU side of sliding-window self-attention: the seconds -> radius rule of EzAudio's entry points and its refusals, inference() setting the window before anything is
prepared and putting the previous one back (also when the sampler raises), and the two new symbols of the C ABI.  The GPU side is tests/test_window_gpu.py."""
import inspect
import os
import re

import pytest
import torch

from tests.test_canvas_host import PARAMS, _RecordingSampler, _StubVAE, _Tok, _enc, _scheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Unet:
    """stands in for MaskDiT: keeps the window and the order in which it was set"""

    def __init__(self, window=None):
        self.attention_window = window
        self.log = []

    def eval(self):
        return self

    def set_attention_window(self, frames):
        self.attention_window = frames or None
        self.log.append(self.attention_window)


def _ez(window=None):
    from ezaudio_amd import api
    ez = api.EzAudio.__new__(api.EzAudio)
    ez.device = 'cpu'
    ez.autoencoder, ez.unet, ez.tokenizer, ez.text_encoder, ez.noise_scheduler, ez.params = _StubVAE(), _Unet(window), _Tok(), _enc, _scheduler(), PARAMS
    return ez


@pytest.fixture()
def seen(monkeypatch):
    from ezaudio_amd import sampler as S

    class Sampler(_RecordingSampler):
        def prepare(self, *a, **kw):
            Sampler.window_at_prepare.append(Sampler.unet.attention_window)
            if Sampler.fail:
                raise RuntimeError('the sampler fell over')
            super().prepare(*a, **kw)

        def __init__(self, unet, scheduler):
            Sampler.unet = unet
    Sampler.window_at_prepare, Sampler.fail = [], False
    monkeypatch.setattr(S, 'LatentSampler', Sampler)
    _RecordingSampler.seen.clear()
    return Sampler


def test_seconds_become_a_radius_in_latent_frames(seen):
    """latent_sr 10: a span of s seconds is round(10 s / 2) frames on either side"""
    ez = _ez()
    for seconds, radius in ((10, 50), (5, 25), (0.5, 2), (0.3, 2), (0.2, 1), (1.1, 6), (0.7, 4)):      # (round half to even, as Python's round)
        assert ez._window_radius(seconds) == radius == int(round(seconds * 10 / 2)), seconds
    assert ez._window_radius(None) is None
    ez.generate_audio('rain', length=30, ddim_steps=5, random_seed=3, attention_window=10)
    assert seen.window_at_prepare == [50] and ez.unet.log == [50, None] and ez.unet.attention_window is None
    assert _RecordingSampler.seen[0]['L'] == 300 and 'attention_window' not in _RecordingSampler.seen[0]['kw']
    # without the argument nothing is set at all
    ez.generate_audio('rain', length=30, ddim_steps=5, random_seed=3)
    assert seen.window_at_prepare == [50, None] and ez.unet.log == [50, None]


@pytest.mark.parametrize('bad', [[10, 10], (5,), 0, -1, 0.0, 0.04, 0.09, True])
def test_window_refusals(seen, bad):
    ez = _ez()
    with pytest.raises(ValueError, match='attention_window'):
        ez.generate_audio('rain', length=30, ddim_steps=5, attention_window=bad)
    with pytest.raises(ValueError, match='attention_window'):
        ez.audio_to_audio('rain', torch.zeros(800).numpy(), attention_window=bad, ddim_steps=5)
    with pytest.raises(ValueError, match='attention_window'):
        ez.editing_audio('rain', 2, torch.zeros(800).numpy(), 1, 1, attention_window=bad, ddim_steps=5)
    assert not seen.window_at_prepare and not ez.unet.log      # refused before anything ran


def test_every_entry_point_takes_the_window_and_says_quality_is_unmeasured():
    from ezaudio_amd import api, sampler
    for fn in (api.EzAudio.generate_audio, api.EzAudio.editing_audio, api.EzAudio.audio_to_audio, sampler.inference):
        assert inspect.signature(fn).parameters['attention_window'].default is None, fn
        assert 'unmeasured' in fn.__doc__
    assert 'attention_window' not in inspect.signature(api.EzAudio_ControlNet.generate_audio).parameters      # out of scope: the handle-level setter only


def test_inference_restores_the_previous_window_also_when_the_sampler_raises(seen):
    from ezaudio_amd.sampler import inference
    unet = _Unet(window=33)      # a window the caller set on the model itself

    def call(**kw):
        return inference(_StubVAE(), unet, None, None, _Tok(), _enc, PARAMS, _scheduler(), ['rain'], None, 120, 5, 0.75, 5, 1, 3, 'cpu', **kw)
    call(attention_window=20)
    assert seen.window_at_prepare == [20] and unet.attention_window == 33 and unet.log == [20, 33]
    seen.fail = True
    with pytest.raises(RuntimeError, match='fell over'):
        call(attention_window=7)
    assert seen.window_at_prepare == [20, 7] and unet.attention_window == 33 and unet.log == [20, 33, 7, 33]
    seen.fail = False
    call()      # no argument: the model's own window stays and nothing is set
    assert seen.window_at_prepare == [20, 7, 33] and unet.log == [20, 33, 7, 33]
    # lists of lengths, per-prompt settings, a solver: the window rides along
    inference(_StubVAE(), unet, None, None, _Tok(), _enc, PARAMS, _scheduler(), ['rain', 'wind'], None, [120, 90], [5, 3], 0.75, 5, 0, [3, 4], 'cpu',
              solver='dpmpp_2m', attention_window=12)
    assert seen.window_at_prepare[-1] == 12 and unet.attention_window == 33
    for bad in (0, -3, 2.5, True, [4]):
        with pytest.raises((ValueError, TypeError)):
            call(attention_window=bad)
    assert unet.attention_window == 33


def test_a_controlnet_of_the_call_gets_the_same_window_and_its_own_back(seen):
    from ezaudio_amd.sampler import inference
    unet, cn = _Unet(), _Unet(window=9)
    seen.fail = True      # (the stand-in sampler knows no ControlNet: what matters is what both hold when prepare is reached)
    held = []
    orig = seen.prepare

    def prepare(self, *a, **kw):
        held.append((unet.attention_window, cn.attention_window))
        return orig(self, *a, **kw)
    seen.prepare = prepare
    with pytest.raises(RuntimeError):
        inference(_StubVAE(), unet, None, None, _Tok(), _enc, PARAMS, _scheduler(), ['rain'], None, 120, 5, 0.75, 5, 1, 3, 'cpu', True, cn,
                  torch.zeros(1, 1, 240), 1.0, attention_window=20)
    assert held == [(20, 20)] and unet.attention_window is None and cn.attention_window == 9


def test_the_two_symbols_are_exported_bound_and_documented(lib):
    from ezaudio_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'ezdit.h')).read()
    assert '#define EZDIT_ABI_VERSION 4' in hdr and lib.ezdit_abi_version() == 4 and _lib.ABI_VERSION == 4      # additive: the version stays
    for name in ('ezdit_set_attention_window', 'ezdit_test_attention_band'):
        assert re.search(r'\bint %s\(' % name, hdr), name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is not None, name
    assert len(lib.ezdit_test_attention_band.argtypes) == 11 and len(lib.ezdit_set_attention_window.argtypes) == 2
    # the setter's refusals that need no GPU; the option table is left alone
    assert lib.ezdit_set_attention_window(None, 4) == -1 and b'null handle' in lib.ezdit_last_error()
    api = open(os.path.join(ROOT, 'ezaudio_amd', 'csrc', 'api.hip')).read()
    body = api[api.index('int ezdit_set_option('):]
    assert 'window' not in body
    from ezaudio_amd import DiTControlNet, MaskDiT
    assert callable(MaskDiT.set_attention_window) and callable(DiTControlNet.set_attention_window) and MaskDiT.attention_window is None
