"""CPU tests of the host side of per-sample sampler settings: noise drawing with per-prompt eta and seeds, the per-sample coefficient rows,
list validation in prepare / inference / generate_audio, and the C ABI's declarations and refusals that need no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests.test_ragged_host import PARAMS, PROMPTS, _Tok, _Unet, _enc, _vae
from tests.util import DIFF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_draw_noises_with_per_prompt_eta_and_seeds_equals_single_prompt_calls():
    from ezaudio_amd.sampler import draw_noises
    etas, seeds = [1.0, 0.0, 0.5, None], [7, 7, 123, 5]
    for frames in (6, [6, 3, 5, 1]):
        init, step = draw_noises(3, frames, 4, etas, seeds, 'cpu', n_prompts=4, first_index=9)
        L = frames if isinstance(frames, int) else max(frames)
        assert init.shape == (4, 3, L) and step.shape == (4, 4, 3, L)
        for i in range(4):
            n = frames if isinstance(frames, int) else frames[i]
            one, one_step = draw_noises(3, n, 4, etas[i], seeds[i], 'cpu')       # the single-prompt call with that seed and eta
            assert torch.equal(init[i:i + 1, :, :n], one) and not init[i, :, n:].any()
            if etas[i]:
                assert torch.equal(step[:, i:i + 1, :, :n], one_step) and not step[:, i, :, n:].any()
            else:
                assert one_step is None and not step[:, i].any()                   # nothing drawn per step: a zero slice
    a, _ = draw_noises(3, 6, 4, [1.0, 0.0], [7, 7], 'cpu', n_prompts=2)
    assert torch.equal(a[0], a[1])                                                 # the init noise does not depend on eta
    _, none = draw_noises(3, 6, 4, [0.0, 0], [1, 2], 'cpu', n_prompts=2)
    assert none is None                                                            # None only when every eta is <= 0
    _, some = draw_noises(3, 6, 4, [0.0, 1e-3], [1, 2], 'cpu', n_prompts=2)
    assert some is not None and not some[:, 0].any() and some[:, 1].any()
    # a scalar seed keeps seed + first_index + i, a scalar eta broadcasts
    b, bs = draw_noises(3, 6, 4, 1.0, 11, 'cpu', n_prompts=3, first_index=2)
    c, cs = draw_noises(3, 6, 4, [1.0] * 3, [13, 14, 15], 'cpu', n_prompts=3)
    assert torch.equal(b, c) and torch.equal(bs, cs)
    for bad in (dict(eta=[1.0, 0.0, 1.0]), dict(random_seed=[1])):
        with pytest.raises(ValueError):
            draw_noises(3, 6, 4, **dict(dict(eta=1.0, random_seed=3), **bad), device='cpu', n_prompts=2)


def test_per_sample_coefficient_rows_are_the_schedulers_rows_per_eta():
    from ezaudio_amd.sampler import sample_coefficients
    from ezaudio_amd.scheduler import DDIMScheduler
    sch = DDIMScheduler(**DIFF)
    sch.set_timesteps(10)
    etas = [1.0, 0.0, 0.5, 1.0]
    rows = sample_coefficients(sch, etas)
    assert len(rows) == 4 and all(len(r) == 10 for r in rows)
    for p, eta in enumerate(etas):
        for i, t in enumerate(sch.timesteps):
            assert rows[p][i] == sch._coef(t, eta)
    assert all(c[4] == 0.0 for c in rows[1]) and rows[0][3][4] > rows[2][3][4] > 0.0     # sigma scales with eta
    assert rows[0][-1][4] == 0.0                                                         # the last step draws nothing at any eta


class _RecordingSampler:
    """Stands in for LatentSampler (tests/test_ragged_host.py's pattern): keeps what prepare() was given."""
    seen = []

    def __init__(self, unet, scheduler):
        pass

    def prepare(self, text, text_mask, uncond, uncond_mask, init, step_noises, gs, gr, steps, eta, **kw):
        _RecordingSampler.seen.append(dict(gs=gs, gr=gr, eta=eta, init=init.clone(), noise=None if step_noises is None else step_noises.clone(),
                                           P=init.shape[0]))
        self.lat = init

    def run(self, use_graph=True):
        pass

    def finish(self):
        return self.lat


def _infer(prompts, **kw):
    from ezaudio_amd import sampler as S
    args = dict(audio_frames=8, guidance_scale=5, guidance_rescale=0.0, ddim_steps=3, eta=1, random_seed=11)
    args.update(kw)
    return S.inference(_vae, _Unet(), None, None, _Tok(), _enc, PARAMS, None, prompts, None, device='cpu', **args)


def test_inference_passes_per_prompt_lists_through_and_validates_them(monkeypatch):
    from ezaudio_amd import sampler as S
    monkeypatch.setattr(S, 'LatentSampler', _RecordingSampler)
    _RecordingSampler.seen.clear()
    out = _infer(PROMPTS[:3], guidance_scale=[5, None, 2.5], guidance_rescale=[0.75, 0, 0], eta=[1, 0, 0.5], random_seed=[4, 5, 6])
    assert out.shape == (3, 1, 64)
    seen = _RecordingSampler.seen[-1]
    assert seen['gs'] == [5, None, 2.5] and seen['gr'] == [0.75, 0, 0] and seen['eta'] == [1, 0, 0.5] and seen['P'] == 3
    assert not seen['noise'][:, 1].any() and seen['noise'][:, 0].any() and seen['noise'][:, 2].any()
    for i, (seed, eta) in enumerate(zip([4, 5, 6], [1, 0, 0.5])):                  # each prompt as its single-prompt call
        _infer([PROMPTS[i]], eta=eta, random_seed=seed)
        one = _RecordingSampler.seen[-1]
        assert torch.equal(one['init'], seen['init'][i:i + 1])
        if eta:
            assert torch.equal(one['noise'], seen['noise'][:, i:i + 1])
    for bad, word in ((dict(guidance_scale=[5, 5]), 'guidance_scale'), (dict(guidance_rescale=[0.1] * 4), 'guidance_rescale'),
                      (dict(eta=[1]), 'eta'), (dict(random_seed=[1, 2]), 'random_seed'), (dict(ddim_steps=[3, 3, 3]), 'ddim_steps')):
        with pytest.raises(ValueError, match=word):
            _infer(PROMPTS[:3], **bad)


class _SettingsSampler(_RecordingSampler):
    """A CPU stand-in whose result depends on each sample's own settings and noise only."""

    def prepare(self, text, text_mask, uncond, uncond_mask, init, step_noises, gs, gr, steps, eta, **kw):
        P = init.shape[0]
        col = lambda v: torch.tensor([float(x or 0) for x in (v if isinstance(v, list) else [v] * P)])[:, None, None]   # noqa: E731
        self.lat = init * col(gs) + 100 * col(gr) + (0 if step_noises is None else (step_noises * col(eta)).sum(dim=0))


SHARD = dict(guidance_scale=[5, None, 2.5], guidance_rescale=[0.75, 0, 0.5], eta=[1, 0, 0.5], random_seed=[4, 5, 6])


def _shard_worker(rank, world, port, q):
    import torch.distributed as dist
    from ezaudio_amd import sampler as S
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        S.LatentSampler = _SettingsSampler
        q.put((rank, _infer(PROMPTS[:3], **SHARD).clone()))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_the_sharded_path_slices_per_prompt_settings_with_the_prompts(monkeypatch):
    import torch.multiprocessing as mp
    from ezaudio_amd import sampler as S
    from tests.test_ragged_host import _free_port
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_shard_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    monkeypatch.setattr(S, 'LatentSampler', _SettingsSampler)
    ref = _infer(PROMPTS[:3], **SHARD)                                   # no process group here: the unsharded path
    for r in range(2):
        assert torch.equal(results[r], ref)
    for i in range(3):                                                   # and every prompt is its single-prompt call
        one = _infer([PROMPTS[i]], **{k: v[i] for k, v in SHARD.items()})
        assert torch.equal(one, ref[i:i + 1])


def test_prepare_validates_lists_and_collapses_equal_ones():
    from ezaudio_amd.sampler import _collapse
    assert _collapse(5.0, 3, 'g') == (5.0, None) and _collapse(None, 3, 'g') == (None, None)
    assert _collapse([5, 5.0, 5], 3, 'g') == (5.0, None)               # equal lists are the scalar call: no table
    assert _collapse([None, 0, 0.0], 3, 'g') == (0.0, None)
    assert _collapse([5, None, 2], 3, 'g') == (None, [5.0, 0.0, 2.0])
    assert _collapse(torch.tensor([1.0, 0.5]), 2, 'eta') == (None, [1.0, 0.5])
    with pytest.raises(ValueError, match='guidance_scale'):
        _collapse([5, 5], 3, 'guidance_scale')


def test_generate_audio_with_per_prompt_settings(monkeypatch):
    from ezaudio_amd import api, sampler as S
    monkeypatch.setattr(S, 'LatentSampler', _RecordingSampler)
    ez = api.EzAudio.__new__(api.EzAudio)
    ez.device = 'cpu'
    ez.autoencoder, ez.unet, ez.tokenizer, ez.text_encoder, ez.noise_scheduler, ez.params = _vae, _Unet(), _Tok(), _enc, None, PARAMS
    _RecordingSampler.seen.clear()
    sr, batch = ez.generate_audio(PROMPTS[:3], length=1, guidance_scale=[5, 3, 1], guidance_rescale=[0.75, 0, 0], eta=[1, 0, 1],
                                  ddim_steps=3, random_seed=[1, 2, 3])
    assert sr == 80 and isinstance(batch, np.ndarray) and batch.shape == (3, 80)    # return shapes unchanged
    assert _RecordingSampler.seen[-1]['gs'] == [5, 3, 1] and _RecordingSampler.seen[-1]['eta'] == [1, 0, 1]
    ez.generate_audio(['rain', '', 'birds'], length=1, guidance_scale=4, ddim_steps=3, random_seed=3)
    assert _RecordingSampler.seen[-1]['gs'] == [4, None, 4]                         # the "empty input" rule per prompt
    ez.generate_audio(['rain', ''], length=1, guidance_scale=[4, 6], ddim_steps=3, random_seed=3)
    assert _RecordingSampler.seen[-1]['gs'] == [4, None]
    ez.generate_audio('', length=1, ddim_steps=3, random_seed=3)
    assert _RecordingSampler.seen[-1]['gs'] is None                                 # the scalar rule is unchanged
    ez.generate_audio(PROMPTS[:2], length=1, ddim_steps=3, randomize_seed=True)
    a = _RecordingSampler.seen[-1]['init']
    ez.generate_audio(PROMPTS[:2], length=1, ddim_steps=3, randomize_seed=True)
    assert not torch.equal(a, _RecordingSampler.seen[-1]['init'])
    for kw, word in ((dict(guidance_scale=[5, 5]), 'guidance_scale'), (dict(eta=[1, 1, 1, 1]), 'eta'), (dict(random_seed=[1]), 'random_seed'),
                     (dict(guidance_rescale=[0.5]), 'guidance_rescale'), (dict(ddim_steps=[3, 3, 3]), 'ddim_steps')):
        with pytest.raises(ValueError, match=word):
            ez.generate_audio(PROMPTS[:3], length=1, **dict(dict(ddim_steps=3), **kw))
    with pytest.raises(ValueError, match='eta'):
        ez.generate_audio('rain', length=1, eta=[1], ddim_steps=3)


def test_the_header_declares_and_the_binding_binds_the_two_entry_points(lib):
    from ezaudio_amd import _lib
    from oracle.weights import model_config
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ezdit.h')).read(), flags=re.S)
    for name, nargs in (('ezdit_sampler_set_sample_params', 6), ('ezdit_cfg_ddim_step_per_sample', 10)):
        m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', hdr)
        assert m and len(m.group(1).split(',')) == nargs, name
        res, args = _lib.PROTOTYPES[name]
        assert res is C.c_int and len(args) == nargs
        assert getattr(lib, name).argtypes == args
    assert '#define EZDIT_ABI_VERSION 4' in hdr and lib.ezdit_abi_version() == 4    # additive: the version stays
    cfg = model_config('xs')
    c = _lib.EzditConfig(cfg['embed_dim'], cfg['num_heads'], cfg['depth'], cfg['in_chans'], cfg['out_chans'], cfg['context_dim'],
                         cfg['ada_sola_rank'], float(cfg['ada_sola_alpha']), float(cfg['mlp_ratio']), 2048)
    h = C.c_void_p()
    assert lib.ezdit_create(C.byref(c), C.byref(h)) == 0
    try:
        gs = (C.c_float * 2)(5.0, 5.0)
        co = (_lib.EzditDdimCoef * 2)()
        assert lib.ezdit_sampler_set_sample_params(h, gs, gs, co, 2, None) == -3 and b'ezdit_sampler_begin' in lib.ezdit_last_error()
        assert lib.ezdit_sampler_set_sample_params(None, gs, gs, co, 2, None) == -1
    finally:
        lib.ezdit_destroy(h)
    assert lib.ezdit_cfg_ddim_step_per_sample(None, None, None, None, None, 0, 1, 128, None, None) == -1
