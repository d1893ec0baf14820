"""CPU tests of the host side of the batched EzAudio.editing_audio: per-request crop / pad / mask bookkeeping, ONE ragged encode, ONE sampler call at per-request
latent lengths, ONE decode, and the order of the bottleneck-noise draws.  The HIP sampler is replaced by a recording stand-in and the VAE by a stub with the
surface of ezaudio_amd.vae.Autoencoder (lengths=, latent_lengths), the pattern of tests/test_controlnet_batch_host.py."""
import sys
import types

import numpy as np
import pytest
import torch

from ezaudio_amd.vae import Autoencoder

PARAMS = {'text_encoder': {'max_length': 8}, 'model': {'out_chans': 4},
          'autoencoder': {'scale': 1.0, 'shift': 0.0, 'sr': 80, 'latent_sr': 10, 'dim': 4}}
SR, LATENT_SR, RATIO, DIM = 80, 10, 8, 4


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
        _RecordingSampler.seen.append(dict(P=P, L=L, init=init.clone(), gt=gt.clone(), gt_mask=gt_mask.clone(), kw=dict(kw), gs=gs, gr=gr, eta=eta,
                                           steps=steps, text=text.clone()))

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
    """ezaudio_amd.vae.Autoencoder on the CPU (inference() batches the ragged decode for that class only): frame means as the latent mean, the bottleneck
    noise drawn as the real bottleneck draws it."""

    def __init__(self):
        self.calls = []

    def latent_lengths(self, lengths):
        return [int(v) // RATIO for v in lengths]

    def __call__(self, audio=None, embedding=None, lengths=None):
        from ezaudio_amd.vae import draw_bottleneck_noise
        if audio is not None:
            self.calls.append(('encode', tuple(audio.shape), None if lengths is None else list(lengths)))
            N, _, T = audio.shape
            lens = self.latent_lengths(lengths if lengths is not None else [T] * N)
            L = max(lens)
            mean = audio[:, 0, :L * RATIO].reshape(N, L, RATIO).mean(-1)[:, None, :].repeat(1, DIM, 1)
            noise = torch.randn(N, DIM, L) if lengths is None else draw_bottleneck_noise(DIM, lens, L, 'cpu')
            z = mean + 0.1 * noise
            for i, n in enumerate(lens):
                z[i, :, n:] = 0
            return z
        self.calls.append(('decode', tuple(embedding.shape), None if lengths is None else list(lengths)))
        return embedding.repeat_interleave(RATIO, dim=2)[:, :1].clone()


def _ez():
    from ezaudio_amd import api
    ez = api.EzAudio.__new__(api.EzAudio)
    ez.device = 'cpu'
    ez.autoencoder, ez.unet, ez.tokenizer, ez.text_encoder, ez.noise_scheduler, ez.params = _StubVAE(), _Unet(), _Tok(), _enc, None, PARAMS
    return ez


def _wave(n, seed, amp):
    g = np.random.default_rng(seed)
    return (amp * g.standard_normal(n)).astype(np.float32)


@pytest.fixture()
def seen(monkeypatch):
    from ezaudio_amd import sampler as S
    monkeypatch.setattr(S, 'LatentSampler', _RecordingSampler)
    _RecordingSampler.seen.clear()
    return _RecordingSampler.seen


PROMPTS = ['a dog barking', 'rain', '']
CLIPS = [_wave(200, 1, 0.9), _wave(120, 2, 0.1), _wave(160, 3, 0.5)]       # 2.5 s, 1.5 s, 2.0 s
# request 0: inside the clip; request 1: the mask runs past the end (out-padding mode); request 2: from the start, the boundary cut to half the mask
REQ = dict(boundary=[0.25, 1.0, 0.5], mask_start=[1.0, 1.2, 0.0], mask_length=[0.5, 0.6, 0.4])
SETTINGS = dict(guidance_scale=[3.5, 2.0, 4.0], guidance_rescale=[0.0, 0.5, 0.25], eta=[1, 0.5, 0], random_seed=[11, 12, 13])


def _single(ez, i, **over):
    kw = {k: v[i] for k, v in {**REQ, **SETTINGS}.items()}
    kw.update(over)
    return ez.editing_audio(PROMPTS[i], gt_file=CLIPS[i], ddim_steps=3, **kw)


def test_batched_edit_is_one_call_of_each_kind_and_passes_what_the_single_calls_pass(seen):
    ez = _ez()
    torch.manual_seed(0)
    sr, outs = ez.editing_audio(PROMPTS, gt_file=CLIPS, ddim_steps=3, **REQ, **SETTINGS)
    assert sr == SR and isinstance(outs, list) and len(outs) == 3 and len(seen) == 1
    # chunks: [0.75, 1.75) s = 80 samples; [0.9, 1.8) s of the clip padded to 1.8 s = 72 samples; [0, 0.6) s = 48 samples (all multiples of the VAE ratio, so the paste sizes agree)
    assert ez.autoencoder.calls == [('encode', (3, 1, 80), [80, 72, 48]), ('decode', (3, 4, 10), [10, 9, 6])]
    b = seen[0]
    assert b['P'] == 3 and b['L'] == 10 and b['kw'] == dict(lengths=[10, 9, 6]) and b['steps'] == 3
    assert b['gs'] == [3.5, 2.0, None] and b['gr'] == [0.0, 0.5, 0.25] and b['eta'] == [1, 0.5, 0]      # '' runs without guidance
    assert b['gt'].shape == (3, 4, 10) and b['gt_mask'].shape == (3, 4, 10) and b['gt_mask'].dtype == torch.bool
    spans = [(2, 8), (3, 9), (0, 4)]            # round(mask seconds * latent_sr) inside each chunk
    batch_outs = [o.copy() for o in outs]
    seen.clear()
    torch.manual_seed(0)                        # ... and the single calls in list order: the same bottleneck-noise draws, the same everything
    for i in range(3):
        ez1 = _ez()
        sr, one = _single(ez1, i)
        s = seen[i]
        n = [10, 9, 6][i]
        assert s['P'] == 1 and s['L'] == n and s['kw'] == {}
        assert ez1.autoencoder.calls == [('encode', (1, 1, [80, 72, 48][i]), None), ('decode', (1, 4, n), None)]
        assert torch.equal(b['gt'][i:i + 1, :, :n], s['gt']) and not b['gt'][i, :, n:].any()
        assert torch.equal(b['gt_mask'][i:i + 1, :, :n], s['gt_mask']) and not b['gt_mask'][i, :, n:].any()
        lo, hi = spans[i]
        want = torch.zeros(4, 10, dtype=torch.bool)
        want[:, lo:hi] = True
        assert torch.equal(b['gt_mask'][i], want)
        assert torch.equal(b['init'][i:i + 1, :, :n], s['init'])                                          # the request's own seed
        assert torch.equal(b['text'][i:i + 1], s['text'])
        assert (s['gs'], s['gr'], s['eta']) == ([3.5, 2.0, None][i], SETTINGS['guidance_rescale'][i], SETTINGS['eta'][i])
        assert one.shape == batch_outs[i].shape and np.array_equal(one, batch_outs[i])
    assert [o.shape for o in batch_outs] == [(200,), (144,), (160,)]                                      # request 1 came back padded to the mask's end


def test_single_edit_passes_what_it_always_passed(seen):
    ez = _ez()
    clip = CLIPS[0]
    torch.manual_seed(3)
    sr, out = ez.editing_audio('rain', boundary=0.25, gt_file=clip, mask_start=1.0, mask_length=0.5, ddim_steps=3, random_seed=5)
    s = seen[0]
    norm = clip / (np.max(np.abs(clip)) + 1e-9)
    assert sr == SR and isinstance(out, np.ndarray) and out.shape == (200,)
    assert s['P'] == 1 and s['L'] == 10 and s['kw'] == {} and (s['gs'], s['gr'], s['eta'], s['steps']) == (3.5, 0, 1, 3)
    assert ez.autoencoder.calls == [('encode', (1, 1, 80), None), ('decode', (1, 4, 10), None)]
    torch.manual_seed(3)
    want_gt = _StubVAE()(audio=torch.tensor(norm[60:140]).reshape(1, 1, -1))
    assert torch.equal(s['gt'], want_gt)
    want = torch.zeros(1, 4, 10, dtype=torch.bool)
    want[:, :, 2:8] = True
    assert torch.equal(s['gt_mask'], want)
    keep = np.ones(200, bool)
    keep[60:140] = False
    assert np.array_equal(out[keep], norm[keep]) and not np.array_equal(out[~keep], norm[~keep])
    # a path goes through librosa.load, as ever; a one-entry batch is that call
    mod = types.SimpleNamespace(load=lambda f, sr: (clip.copy(), sr))
    sys.modules['librosa'], old = mod, sys.modules.get('librosa')
    try:
        torch.manual_seed(3)
        sr, from_path = ez.editing_audio('rain', boundary=0.25, gt_file='clip.wav', mask_start=1.0, mask_length=0.5, ddim_steps=3, random_seed=5)
    finally:
        if old is None:
            del sys.modules['librosa']
        else:
            sys.modules['librosa'] = old
    assert np.array_equal(from_path, out)
    torch.manual_seed(3)
    sr, outs = ez.editing_audio(['rain'], boundary=0.25, gt_file=[clip], mask_start=1.0, mask_length=0.5, ddim_steps=3, random_seed=5)
    assert isinstance(outs, list) and len(outs) == 1 and np.array_equal(outs[0], out)
    assert torch.equal(seen[2]['gt'], s['gt']) and torch.equal(seen[2]['init'], s['init'])


def test_size_mismatches_and_a_list_of_step_counts_raise(seen):
    ez = _ez()
    two = dict(text=PROMPTS[:2], gt_file=CLIPS[:2], boundary=0.25, mask_start=0.5, mask_length=0.5, ddim_steps=3)
    for kw in (dict(boundary=[0.25]), dict(mask_start=[0.5, 0.5, 0.5]), dict(mask_length=[0.5]), dict(guidance_scale=[3.5]),
               dict(guidance_rescale=[0.5, 0.5, 0.5]), dict(eta=[1]), dict(random_seed=[1, 2, 3]), dict(gt_file=CLIPS), dict(gt_file=CLIPS[:1]),
               dict(ddim_steps=[3, 3]), dict(gt_file=[np.zeros((2, 50), np.float32), CLIPS[1]])):
        with pytest.raises(ValueError):
            ez.editing_audio(**{**two, **kw})
    one = dict(text='rain', gt_file=CLIPS[0], boundary=0.25, mask_start=0.5, mask_length=0.5, ddim_steps=3)
    for kw in (dict(gt_file=CLIPS[:1]), dict(boundary=[0.25]), dict(mask_start=[0.5]), dict(guidance_scale=[3.5]), dict(random_seed=[1]),
               dict(ddim_steps=[3])):
        with pytest.raises(ValueError):
            ez.editing_audio(**{**one, **kw})
    with pytest.raises(ValueError):
        ez.editing_audio(**{**two, 'solver': 'dpmpp_2m'})                   # the default eta = 1 with the deterministic solver, as elsewhere
    assert not seen and not ez.autoencoder.calls                            # refused before anything was encoded or sampled
    ez.autoencoder = lambda audio=None, embedding=None: None                # the reference's surface only: no ragged encode to batch on
    with pytest.raises(NotImplementedError):
        ez.editing_audio(**two)


def test_a_shared_recording_is_loaded_once_and_cropped_per_request(seen, monkeypatch):
    ez = _ez()
    loads = []

    def load(f, sr):
        loads.append(f)
        return CLIPS[0].copy(), sr
    monkeypatch.setitem(sys.modules, 'librosa', types.SimpleNamespace(load=load))
    sr, outs = ez.editing_audio(PROMPTS[:2], boundary=0.25, gt_file='shared.wav', mask_start=[1.0, 0.5], mask_length=0.5, ddim_steps=3,
                                random_seed=[1, 2], randomize_seed=False)
    assert loads == ['shared.wav'] and len(outs) == 2 and len(seen) == 1
    assert ez.autoencoder.calls[0] == ('encode', (2, 1, 80), [80, 80])
    assert seen[0]['kw'] == {}                                              # equal lengths: the unpadded batch, one equal-length decode
    assert ez.autoencoder.calls[1] == ('decode', (2, 4, 10), None)
    norm = CLIPS[0] / (np.max(np.abs(CLIPS[0])) + 1e-9)
    for out, (lo, hi) in zip(outs, ((60, 140), (20, 100))):
        keep = np.ones(200, bool)
        keep[lo:hi] = False
        assert np.array_equal(out[keep], norm[keep]) and not np.array_equal(out[~keep], norm[~keep])
    assert outs[0] is not outs[1]
    # randomize_seed: one seed per request
    import random
    random.seed(4)
    ez.editing_audio(PROMPTS[:2], boundary=0.25, gt_file='shared.wav', mask_start=[1.0, 0.5], mask_length=0.5, ddim_steps=3, randomize_seed=True)
    assert not torch.equal(seen[1]['init'][0], seen[1]['init'][1])


def test_bottleneck_noise_is_drawn_per_clip_in_list_order():
    from ezaudio_amd.vae import draw_bottleneck_noise
    lens = [7, 3, 5]
    torch.manual_seed(9)
    noise = draw_bottleneck_noise(4, lens, 8, 'cpu')
    torch.manual_seed(9)
    singles = [torch.randn(1, 4, n) for n in lens]
    assert noise.shape == (3, 4, 8)
    for b, (n, s) in enumerate(zip(lens, singles)):
        assert torch.equal(noise[b:b + 1, :, :n], s) and not noise[b, :, n:].any()
    torch.manual_seed(9)
    assert not torch.equal(torch.randn(3, 4, 8)[1, :, :3], singles[1][0])   # ONE padded draw would give other numbers
