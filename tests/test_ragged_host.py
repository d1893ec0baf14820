"""CPU tests of the host side of mixed-length batches: noise drawing, prompt sharding with per-prompt lengths, the public API's trimming,
and the C ABI's refusals that need no GPU."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def test_draw_noises_with_a_list_of_lengths_equals_per_sample_calls():
    from ezaudio_amd.sampler import draw_noises
    lens = [7, 16, 1, 11]
    for eta in (1.0, 0.0):
        init, step = draw_noises(3, lens, 4, eta, 5, 'cpu', n_prompts=4, first_index=2)
        assert init.shape == (4, 3, 16) and (step is None) == (eta == 0.0)
        if step is not None:
            assert step.shape == (4, 4, 3, 16)
        for i, n in enumerate(lens):
            one, one_step = draw_noises(3, n, 4, eta, 5, 'cpu', n_prompts=1, first_index=2 + i)   # the sample alone at its own length
            assert torch.equal(init[i:i + 1, :, :n], one) and not init[i, :, n:].any()
            if step is not None:
                assert torch.equal(step[:, i:i + 1, :, :n], one_step) and not step[:, i, :, n:].any()
    same, _ = draw_noises(3, [5, 5], 2, 1.0, 9, 'cpu', n_prompts=2)
    ref, _ = draw_noises(3, 5, 2, 1.0, 9, 'cpu', n_prompts=2)
    assert torch.equal(same, ref)
    with pytest.raises(ValueError):
        draw_noises(3, [5, 5, 5], 2, 1.0, 9, 'cpu', n_prompts=2)
    with pytest.raises(ValueError):
        draw_noises(3, [5, 0], 2, 1.0, 9, 'cpu', n_prompts=2)


# ----------------------------------------------------------------------------------------------------------------------
# inference() with per-prompt lengths; the HIP sampler is replaced by a CPU stand-in (the pattern of tests/test_dist.py)
# that honours the contract: a function of each sample's OWN valid frames, zero beyond
# ----------------------------------------------------------------------------------------------------------------------
class _CpuSampler:
    def __init__(self, unet, scheduler):
        pass

    def prepare(self, text, text_mask, uncond, uncond_mask, init, step_noises, gs, gr, steps, eta, gt=None, gt_mask=None,
                controlnet=None, condition=None, conditioning_scale=1.0, lengths=None):
        P, _, L = init.shape
        lengths = [L] * P if lengths is None else lengths
        lat = init + 0.1 * step_noises.sum(dim=0) + text.mean(dim=(1, 2))[:, None, None] + 3 * uncond.mean(dim=(1, 2))[:, None, None]
        for i, n in enumerate(lengths):
            lat[i] = lat[i] + lat[i, :, :n].max()      # couples the frames of a sample, as attention does (max: exact in any order)
            lat[i, :, n:] = 0
        self.lat = lat

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
    """8 samples per frame, with a boundary effect like a convolution's: the last sample of a clip depends on where the clip ends."""
    w = embedding.repeat_interleave(8, dim=2)[:, :1].clone()
    w[..., -1] += 100.0
    return w


PROMPTS = ['a dog barking', 'rain', 'a car passing by on a wet road', 'birds', 'applause']
NEGS = ['noise', '', 'music', 'low quality', 'speech']
FRAMES = [16, 9, 12, 16, 5]
PARAMS = {'text_encoder': {'max_length': 8}, 'model': {'out_chans': 4}, 'autoencoder': {'scale': 1.0, 'shift': 0.0, 'sr': 80, 'latent_sr': 10}}


def _run_inference(prompts, negs, frames):
    from ezaudio_amd import sampler as S
    S.LatentSampler = _CpuSampler
    return S.inference(_vae, _Unet(), None, None, _Tok(), _enc, PARAMS, None, prompts, negs, audio_frames=frames, guidance_scale=5,
                       ddim_steps=3, eta=1, random_seed=11, device='cpu')


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, n, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        out = _run_inference(PROMPTS[:n], NEGS[:n], FRAMES[:n])
        q.put((rank, out.clone()))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_inference_with_mixed_lengths_decodes_each_sample_at_its_own_length():
    out = _run_inference(PROMPTS, NEGS, FRAMES)
    assert out.shape == (5, 1, 128)
    for i, n in enumerate(FRAMES):
        alone = _run_inference([PROMPTS[i]], [NEGS[i]], n) if i == 0 else None
        assert not out[i, :, 8 * n:].any() and out[i, 0, 8 * n - 1] > 50      # the VAE saw a clip of n frames, not of 16
        if alone is not None:
            assert torch.equal(out[i:i + 1, :, :8 * n], alone)               # (sample 0 has seed + 0: the one-prompt call)


@pytest.mark.parametrize('n', [5, 3, 2])   # odd prompt counts: unequal shards, whose own longest sample differs from the global one
def test_inference_with_mixed_lengths_shards_over_gloo_world2(n):
    world = 2
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    ref = _run_inference(PROMPTS[:n], NEGS[:n], FRAMES[:n])      # no process group here: the unsharded path
    assert ref.shape == (n, 1, 8 * max(FRAMES[:n]))
    for r in range(world):
        assert torch.equal(results[r], ref)


def test_generate_audio_with_a_list_of_lengths_returns_trimmed_arrays(monkeypatch):
    from ezaudio_amd import api, sampler as S
    monkeypatch.setattr(S, 'LatentSampler', _CpuSampler)
    ez = api.EzAudio.__new__(api.EzAudio)
    ez.device = 'cpu'
    ez.autoencoder, ez.unet, ez.tokenizer, ez.text_encoder, ez.noise_scheduler, ez.params = _vae, _Unet(), _Tok(), _enc, None, PARAMS
    sr, wavs = ez.generate_audio(PROMPTS[:3], length=[1.6, 0.5, 1.2], ddim_steps=3, random_seed=3)
    assert sr == 80 and isinstance(wavs, list) and [w.shape for w in wavs] == [(128,), (40,), (96,)]
    assert all(w[-1] > 50 for w in wavs)                                      # each decoded at its own length
    sr, batch = ez.generate_audio(PROMPTS[:3], length=1, ddim_steps=3, random_seed=3)   # the scalar keeps its meaning and return type
    assert isinstance(batch, np.ndarray) and batch.shape == (3, 80)
    with pytest.raises(ValueError):
        ez.generate_audio(PROMPTS[:3], length=[1, 2], ddim_steps=3)
    with pytest.raises(ValueError):
        ez.generate_audio('rain', length=[1], ddim_steps=3)


def test_set_lengths_is_exported_and_refuses_a_handle_without_workspace(lib):
    from ezaudio_amd import _lib
    from oracle.weights import model_config
    cfg = model_config('xs')
    c = _lib.EzditConfig(cfg['embed_dim'], cfg['num_heads'], cfg['depth'], cfg['in_chans'], cfg['out_chans'], cfg['context_dim'],
                         cfg['ada_sola_rank'], float(cfg['ada_sola_alpha']), float(cfg['mlp_ratio']), 2048)
    h = C.c_void_p()
    assert lib.ezdit_create(C.byref(c), C.byref(h)) == 0
    try:
        arr = (C.c_int32 * 2)(5, 5)
        assert lib.ezdit_set_lengths(h, arr, 2, None) == -3 and b'workspace' in lib.ezdit_last_error()
        assert lib.ezdit_set_lengths(None, arr, 2, None) == -1
        assert lib.ezdit_abi_version() == 4
    finally:
        lib.ezdit_destroy(h)
    assert lib.ezdit_test_final_conv(None, 0, None, None, None, 1, 128, 4, None, None) == -1
