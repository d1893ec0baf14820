"""Batched EzAudio.editing_audio end to end on the GPU: two edits of different recordings, lengths, masks, prompts and seeds in ONE ragged encode, ONE sampler
call and ONE ragged decode, against the two single calls.  The model is the EzAudio('mini', ...) of tests/test_vae.py (xs DiT, mini VAE with an 8x ratio, stand-in
tokenizer / text encoder); the helpers are copied, not imported from a test module."""
import os
import sys
import types

import numpy as np
import pytest

from oracle import vae as V
from oracle.weights import uniform_pm1
from tests.util import record, rel_l2

pytestmark = pytest.mark.gpu

MINI_VAE = dict(channels=64, c_mults=[1, 2], strides=[2, 4], latent_dim=128, out_channels=1)
SR = 24000


def _mini_autoencoder(device='cuda'):
    import torch
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
        import torch
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
        import torch
        g = torch.Generator().manual_seed(7)
        table = torch.randn(128, self.dim, generator=g).to(input_ids.device)
        return type('Out', (), dict(last_hidden_state=table[input_ids % 128]))()


# request A: a 1 s numpy waveform, chunk [0.30, 0.50) s = samples [7200, 12000) = 600 latent frames of the mini VAE; request B: a 0.5 s recording that goes through
# (a stubbed) librosa.load, chunk [0.18, 0.28) s = samples [4320, 6720) = 300 frames.  All four bounds are multiples of the VAE ratio 8, so the paste sizes agree.
SRC_A = (0.3 * uniform_pm1('editb_a', SR, 9)).astype(np.float32)
SRC_B = (0.7 * uniform_pm1('editb_b', SR // 2, 10)).astype(np.float32)
REQ_A = dict(text='rain on a roof', gt_file=SRC_A, boundary=0.05, mask_start=0.35, mask_length=0.1, guidance_scale=3.5, guidance_rescale=0.0, eta=1,
             random_seed=3)
REQ_B = dict(text='a dog barking twice', gt_file='b.wav', boundary=0.02, mask_start=0.2, mask_length=0.06, guidance_scale=2.0, guidance_rescale=0.5, eta=0.5,
             random_seed=8)
CHUNK = {'a': (7200, 12000), 'b': (4320, 6720)}
SRC = {'a': SRC_A, 'b': SRC_B}


def _batch(*reqs):
    return {k: [r[k] for r in reqs] for k in reqs[0]}


@pytest.fixture(scope='module')
def ez(tmp_path_factory):
    import yaml
    import torch
    import ezaudio_amd
    from ezaudio_amd import api as A
    from ezaudio_amd.config import load_yaml_with_includes
    from oracle.weights import make_state_dict, model_config
    tmp = tmp_path_factory.mktemp('edit_batch')
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
        mp.setitem(sys.modules, 'librosa', types.SimpleNamespace(load=lambda f, sr: (SRC_B.copy(), sr)))   # librosa is absent offline; the API uses load() only
        yield A.EzAudio('mini', autoencoder=_mini_autoencoder(), tokenizer=_Tok(), text_encoder=_Enc(cfg['context_dim']), state_dict=sd)


@pytest.fixture(scope='module')
def singles(ez):
    """The two single calls, in list order after one seeding of the global generator (the bottleneck noise comes from it)."""
    import torch
    torch.manual_seed(21)
    return {'a': ez.editing_audio(ddim_steps=20, **REQ_A)[1], 'b': ez.editing_audio(ddim_steps=20, **REQ_B)[1]}


def test_batched_edit_matches_the_single_calls(ez, singles):
    import torch
    torch.manual_seed(21)
    sr, outs = ez.editing_audio(ddim_steps=20, **_batch(REQ_A, REQ_B))
    assert sr == SR and isinstance(outs, list) and len(outs) == 2
    for name, out in zip('ab', outs):
        src, (lo, hi) = SRC[name], CHUNK[name]
        assert out.shape == src.shape == singles[name].shape and np.isfinite(out).all()
        keep = np.ones(len(src), bool)
        keep[lo:hi] = False
        assert np.array_equal(out[keep], (src / (np.abs(src).max() + 1e-9))[keep])           # outside the re-synthesised chunk: untouched
        assert np.array_equal(singles[name][keep], out[keep])
        r = rel_l2(out[lo:hi], singles[name][lo:hi])
        record(f'batched edit, request {name} ({(hi - lo) // 8} frames): rel_l2 {r:.3e} to its single call inside the chunk')
        assert out[lo:hi].std() > 0 and not np.array_equal(out[lo:hi], (src / (np.abs(src).max() + 1e-9))[lo:hi])
        assert r < 5e-2


def test_swapping_the_requests_swaps_the_results(ez, monkeypatch):
    """The bottleneck noise is drawn from the global generator in list order (the draws of the single calls), so a swapped list hands every clip OTHER noise by
    design; for this check the draw is pinned per clip (a generator seeded by the clip's latent length), and then nothing may depend on the position in the batch."""
    import torch
    from ezaudio_amd import vae as hipvae

    def pinned(latent, lengths, width, device):
        noise = torch.zeros(len(lengths), latent, width, device=device)
        for b, n in enumerate(lengths):
            noise[b, :, :n] = torch.randn(latent, n, generator=torch.Generator().manual_seed(1000 + n)).to(device)
        return noise
    monkeypatch.setattr(hipvae, 'draw_bottleneck_noise', pinned)
    sr, ab = ez.editing_audio(ddim_steps=20, **_batch(REQ_A, REQ_B))
    sr, ba = ez.editing_audio(ddim_steps=20, **_batch(REQ_B, REQ_A))
    assert np.array_equal(ab[0], ba[1]) and np.array_equal(ab[1], ba[0])
    assert not np.array_equal(ab[0][slice(*CHUNK['a'])], (SRC_A / (np.abs(SRC_A).max() + 1e-9))[slice(*CHUNK['a'])])


def test_a_batch_of_one_is_the_single_call(ez, singles):
    import torch
    torch.manual_seed(21)
    sr, outs = ez.editing_audio(ddim_steps=20, **_batch(REQ_A))
    assert len(outs) == 1 and np.array_equal(outs[0], singles['a'])
