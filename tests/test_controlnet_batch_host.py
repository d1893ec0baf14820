"""CPU tests of the host side of the batched ControlNet: EzAudio_ControlNet.generate_audio with lists (per-clip energy curves, padded
conditions, lengths, scales, trimming), inference() with a list of conditions, and the sharded driver's slicing.  The HIP sampler is replaced
by a recording stand-in, the pattern of tests/test_ragged_host.py."""
import ctypes as C

import numpy as np
import pytest
import torch

PARAMS = {'text_encoder': {'max_length': 8}, 'model': {'out_chans': 4},
          'autoencoder': {'scale': 1.0, 'shift': 0.0, 'sr': 80, 'latent_sr': 10, 'dim': 4}}
SR, LATENT_SR = 80, 10
HOP, WINDOW = 4, 8      # two control frames per latent frame: hop = sr / (2 latent_sr)


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
        if condition is not None:
            lat = lat + torch.stack([condition[i if condition.shape[0] > 1 else 0, :, :2 * n].mean() for i, n in enumerate(lengths)])[:, None, None]
        for i, n in enumerate(lengths):
            lat[i, :, n:] = 0
        self.lat = lat
        _RecordingSampler.seen.append(dict(P=P, L=L, condition=None if condition is None else condition.clone(), scale=conditioning_scale,
                                           controlnet=controlnet, kw=dict(kw), gs=gs, gr=gr, eta=eta, text=text.clone()))

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


def _vae(embedding):
    return embedding.repeat_interleave(SR // LATENT_SR, dim=2)[:, :1].clone()


def _ez():
    from ezaudio_amd import api
    from ezaudio_amd.conditions import Conditioner
    ez = api.EzAudio_ControlNet.__new__(api.EzAudio_ControlNet)
    ez.device = 'cpu'
    ez.autoencoder, ez.unet, ez.tokenizer, ez.text_encoder, ez.noise_scheduler, ez.params = _vae, _Unet(), _Tok(), _enc, None, PARAMS
    ez.controlnet = object()
    ez.conditioner = Conditioner('energy', hop_size=HOP, window_size=WINDOW, padding='reflect', min_db=-60, norm=True)
    return ez


def _wave(n, seed, amp):
    g = np.random.default_rng(seed)
    t = np.arange(n)
    return (amp * g.standard_normal(n) * (0.3 + 0.7 * np.sin(2 * np.pi * t / 97.0) ** 2)).astype(np.float32)


def _curve_alone(ez, wav, seconds, gate=0.0):
    """The control signal of one clip by itself: what the reference's single-clip code computes (api/controlnet.py:118-131)."""
    gt = wav / (np.max(np.abs(wav)) + 1e-9)
    if gate > 0:
        gt[np.abs(gt) <= gate] = 0
    n = int(round(seconds * SR))
    gt = np.pad(gt, (0, n - len(gt))) if len(gt) < n else gt[:n]
    return ez.conditioner(torch.tensor(gt).unsqueeze(0), (1, 4, n // 8))


PROMPTS = ['a dog barking', 'rain', 'applause']


@pytest.fixture()
def seen(monkeypatch):
    from ezaudio_amd import sampler as S
    monkeypatch.setattr(S, 'LatentSampler', _RecordingSampler)
    _RecordingSampler.seen.clear()
    return _RecordingSampler.seen


def test_generate_audio_with_lists_passes_per_clip_curves_lengths_and_scales(seen):
    ez = _ez()
    clips = [_wave(130, 1, 0.9), _wave(64, 2, 0.05), _wave(200, 3, 0.4)]      # 1.625 s, 0.8 s, 2.5 s; very different loudness
    secs = [1.6, 0.5, 1.2]
    sr, wavs = ez.generate_audio(PROMPTS, clips, length=secs, conditioning_scale=[1.0, 0.5, 0.25], surpass_noise=[0, 0.01, 0],
                                 guidance_scale=[3.5, 2.0, 3.5], ddim_steps=3, random_seed=[1, 2, 3])
    assert sr == SR and isinstance(wavs, list) and len(seen) == 1
    s = seen[0]
    frames = [16, 5, 12]
    assert s['P'] == 3 and s['L'] == 16 and s['kw'] == dict(lengths=frames) and s['scale'] == [1.0, 0.5, 0.25]
    assert s['controlnet'] is ez.controlnet and s['gs'] == [3.5, 2.0, 3.5]
    cond = s['condition']
    assert cond.shape == (3, 1, 32)                                            # 2 * Lmax control frames, padded
    for i, (w, sec, gate, f) in enumerate(zip(clips, secs, [0, 0.01, 0], frames)):
        alone = _curve_alone(ez, w.copy(), sec, gate)
        assert alone.shape == (1, 1, 2 * f)
        assert torch.equal(cond[i:i + 1, :, :2 * f], alone) and not cond[i, :, 2 * f:].any()
        assert abs(float(cond[i, :, :2 * f].max()) - 1.0) < 1e-6               # normalised by THIS clip's own maximum
    # each output trimmed to min(the recording's length, its duration)
    assert [w.shape for w in wavs] == [(128,), (40,), (96,)]
    sr, wavs = ez.generate_audio(PROMPTS[:2], [_wave(100, 4, 0.5), _wave(1000, 5, 0.5)], length=[2.0, 2.0], ddim_steps=3, random_seed=3)
    assert [w.shape for w in wavs] == [(100,), (160,)]                         # a short recording keeps its own length
    assert seen[1]['kw'] == {} and seen[1]['scale'] == 1 and seen[1]['condition'].shape == (2, 1, 40)   # equal lengths: the unpadded batch
    # length=None: the reference's fixed 10 s for every prompt
    sr, wavs = ez.generate_audio(PROMPTS[:2], [_wave(300, 6, 0.5), _wave(900, 7, 0.5)], ddim_steps=3, random_seed=3)
    assert [w.shape for w in wavs] == [(300,), (800,)] and seen[2]['L'] == 100 and seen[2]['condition'].shape == (2, 1, 200)


def test_generate_audio_single_prompt_passes_what_it_always_passed(seen):
    ez = _ez()
    wav = _wave(300, 8, 0.7)
    sr, out = ez.generate_audio('rain', wav, ddim_steps=3, random_seed=5, conditioning_scale=0.8)
    s = seen[0]
    assert sr == SR and isinstance(out, np.ndarray) and out.shape == (300,)    # 1-D, trimmed to the recording
    assert s['P'] == 1 and s['L'] == 100 and s['kw'] == {} and s['scale'] == 0.8 and s['eta'] == 1 and s['gs'] == 3.5 and s['gr'] == 0
    assert torch.equal(s['condition'], _curve_alone(ez, wav.copy(), 10)) and s['condition'].shape == (1, 1, 200)
    # ... and the one-entry batch is that call: same conditions, same seeds, same audio
    sr, outs = ez.generate_audio(['rain'], [wav], ddim_steps=3, random_seed=5, conditioning_scale=0.8)
    assert torch.equal(seen[1]['condition'], s['condition']) and np.array_equal(outs[0], out)
    # a duration for the single prompt
    sr, out = ez.generate_audio('rain', wav, ddim_steps=3, random_seed=5, length=1.5)
    assert out.shape == (120,) and seen[2]['L'] == 15 and seen[2]['condition'].shape == (1, 1, 30)


def test_generate_audio_list_size_mismatches_raise(seen):
    ez = _ez()
    clips = [_wave(100, 1, 0.5), _wave(100, 2, 0.5)]
    for kw in (dict(length=[1, 2, 3]), dict(conditioning_scale=[1.0]), dict(surpass_noise=[0, 0, 0]), dict(guidance_scale=[3.5]),
               dict(guidance_rescale=[0.5]), dict(eta=[1, 1, 1]), dict(random_seed=[1])):
        with pytest.raises(ValueError):
            ez.generate_audio(PROMPTS[:2], clips, ddim_steps=3, **kw)
    with pytest.raises(ValueError):
        ez.generate_audio(PROMPTS[:2], clips[:1], ddim_steps=3)
    with pytest.raises(ValueError):
        ez.generate_audio(PROMPTS[:2], clips[0], ddim_steps=3)
    with pytest.raises(ValueError):
        ez.generate_audio('rain', clips, ddim_steps=3)
    with pytest.raises(ValueError):
        ez.generate_audio('rain', clips[0], ddim_steps=3, conditioning_scale=[1.0])
    with pytest.raises(ValueError):
        ez.generate_audio(PROMPTS[:2], clips, ddim_steps=[3, 3])
    with pytest.raises(ValueError):
        ez.generate_audio(PROMPTS[:2], [np.zeros((2, 50), np.float32), clips[1]], ddim_steps=3)
    assert not seen                                                            # refused before anything was sampled


def _infer(conditions, frames, scales, **kw):
    from ezaudio_amd import sampler as S
    return S.inference(_vae, _Unet(), None, None, _Tok(), _enc, PARAMS, None, PROMPTS, None, audio_frames=frames, guidance_scale=3.5,
                       ddim_steps=3, eta=1, random_seed=11, device='cpu', controlnet=object(), condition=conditions, conditioning_scale=scales, **kw)


def test_inference_pads_a_list_of_conditions_and_checks_shapes(seen):
    from ezaudio_amd.sampler import pad_conditions
    frames = [16, 5, 12]
    conds = [torch.arange(2 * f, dtype=torch.float32).reshape(1, 1, 2 * f) + 1 for f in frames]
    out = _infer(conds, frames, [1.0, 0.5, 0.25])
    assert out.shape == (3, 1, 128) and len(seen) == 1
    c = seen[0]['condition']
    assert c.shape == (3, 1, 32) and seen[0]['kw'] == dict(lengths=frames) and seen[0]['scale'] == [1.0, 0.5, 0.25]
    for i, f in enumerate(frames):
        assert torch.equal(c[i:i + 1, :, :2 * f], conds[i]) and not c[i, :, 2 * f:].any()
    padded = pad_conditions(conds, frames, 3)
    again = _infer(padded, frames, [1.0, 0.5, 0.25])                           # the padded tensor form is the same call
    assert torch.equal(again, out) and torch.equal(seen[1]['condition'], c)
    for bad in (conds[:2], [conds[0], conds[1], conds[1]], padded[:, :, :30], padded[:2]):
        with pytest.raises(ValueError):
            _infer(bad, frames, 1.0)
    with pytest.raises(ValueError):
        _infer(conds, frames, [1.0, 0.5])


def test_sharded_driver_slices_scales_and_cuts_conditions_to_the_shards_length(seen, monkeypatch):
    """The sharded path of inference() (torch.distributed initialised, several prompts) calls inference() again per shard: the scale list is
    sliced with the prompts, the condition is cut to 2 * lmax of the SHARD.  The process group is faked: every shard is run here, in turn."""
    import torch.distributed as dist
    from ezaudio_amd import dist as ezdist
    frames = [5, 12, 16]                                                       # shard [0, 2) has lmax 12, shard [2, 3) has 16
    conds = [torch.arange(2 * f, dtype=torch.float32).reshape(1, 1, 2 * f) + 1 for f in frames]
    whole = _infer(conds, frames, [1.0, 0.5, 0.25])
    seen.clear()
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda group=None: 2)

    def fake_sharded(fn, n):
        assert n == 3
        return torch.cat([fn(*ezdist.shard_range(n, r, 2)) for r in range(2)], 0)
    monkeypatch.setattr(ezdist, 'sample_sharded', fake_sharded)
    out = _infer(conds, frames, [1.0, 0.5, 0.25])
    assert torch.equal(out, whole)
    assert len(seen) == 2
    a, b = seen
    assert a['P'] == 2 and a['L'] == 12 and a['kw'] == dict(lengths=[5, 12]) and a['scale'] == [1.0, 0.5] and a['condition'].shape == (2, 1, 24)
    assert torch.equal(a['condition'][0:1, :, :10], conds[0]) and torch.equal(a['condition'][1:2], conds[1])
    assert b['P'] == 1 and b['L'] == 16 and b['kw'] == {} and b['scale'] == [0.25] and torch.equal(b['condition'], conds[2])
    # equal lengths: the unpadded shards, scales still sliced
    seen.clear()
    eq = [torch.full((1, 1, 20), float(i + 1)) for i in range(3)]
    _infer(eq, 10, [1.0, 0.5, 0.25])
    assert [s['scale'] for s in seen] == [[1.0, 0.5], [0.25]] and [tuple(s['condition'].shape) for s in seen] == [(2, 1, 20), (1, 1, 20)]


def test_pair_entry_points_are_exported_and_refuse_without_workspace(lib):
    from ezaudio_amd import _lib
    from oracle.weights import model_config
    cfg = model_config('xs')
    c = _lib.EzditConfig(cfg['embed_dim'], cfg['num_heads'], cfg['depth'], cfg['in_chans'], cfg['out_chans'], cfg['context_dim'],
                         cfg['ada_sola_rank'], float(cfg['ada_sola_alpha']), float(cfg['mlp_ratio']), 2048)
    h = C.c_void_p()
    assert lib.ezdit_create(C.byref(c), C.byref(h)) == 0
    try:
        arr, sc = (C.c_int32 * 2)(5, 5), (C.c_float * 2)(1.0, 0.5)
        assert lib.ezdit_sampler_set_pair_lengths(h, arr, 2, None) == -3 and b'workspace' in lib.ezdit_last_error()
        assert lib.ezdit_sampler_set_cn_scales(h, sc, 2, None) == -3 and b'workspace' in lib.ezdit_last_error()
        assert lib.ezdit_sampler_set_pair_lengths(None, arr, 2, None) == -1 and lib.ezdit_sampler_set_cn_scales(None, sc, 2, None) == -1
        assert lib.ezdit_abi_version() == 4
    finally:
        lib.ezdit_destroy(h)


def test_prepare_refuses_a_bad_condition_before_touching_the_device():
    from ezaudio_amd.sampler import LatentSampler
    smp = LatentSampler.__new__(LatentSampler)
    smp.unet = type('U', (), dict(device='cpu'))()
    init = torch.zeros(2, 4, 8)
    for cond in (None, torch.zeros(3, 1, 16), torch.zeros(2, 1, 15), torch.zeros(2, 16)):
        with pytest.raises(ValueError, match='condition'):
            smp.prepare(None, None, None, None, init, None, 3.5, 0.0, 3, 0, controlnet=object(), condition=cond)
    with pytest.raises(ValueError, match='conditioning_scale'):
        smp.prepare(None, None, None, None, init, None, 3.5, 0.0, 3, 0, controlnet=object(), condition=torch.zeros(2, 1, 16),
                    conditioning_scale=[1.0, 0.5, 0.25])
