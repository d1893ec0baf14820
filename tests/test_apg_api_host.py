"""CPU tests of the host side of adaptive projected guidance: the `apg` argument of LatentSampler.prepare / set_apg, inference() and EzAudio.generate_audio,
editing_audio and audio_to_audio -- parsing and defaults, the per-prompt lists, the ValueErrors, where prepare() sets the table, and slicing on a sharded call --
and the two new entry points of the C ABI as far as they go without a GPU.  The sampler is the recording stand-in of tests/test_canvas_host.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests.test_canvas_host import PARAMS, _enc, _ez, _RecordingSampler, _Tok, _Unet, seen  # noqa: F401  (`seen` is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROMPTS = ['a dog barking', 'rain', 'applause']


# ---------------------------------------------------------------------------------------------------
# 1. parsing and defaults
# ---------------------------------------------------------------------------------------------------
def test_apg_entries_defaults_lists_and_refusals():
    from ezaudio_amd.sampler import APG_DEFAULTS, apg_entries
    assert APG_DEFAULTS == dict(eta=0.0, norm_threshold=0.0, momentum=-0.5)      # apg=True: no parallel part, momentum -0.5, NO cap
    assert apg_entries(True, 2) == [(0.0, 0.0, -0.5, 1)] * 2
    assert apg_entries(dict(norm_threshold=7.5), 1) == [(0.0, 7.5, -0.5, 1)]
    assert apg_entries(dict(eta=0.25, momentum=0), 3) == [(0.25, 0.0, 0.0, 1)] * 3
    assert apg_entries([True, None, dict(eta=1, norm_threshold=2, momentum=0.5)], 3) == [(0.0, 0.0, -0.5, 1), (0.0, 0.0, 0.0, 0), (1.0, 2.0, 0.5, 1)]
    for nobody in (None, False, [None, None], [False, None]):
        assert apg_entries(nobody, 2) is None                                    # nobody asks: the plain call
    nan, inf = float('nan'), float('inf')
    for bad, n in (([True], 2), ([True, True, True], 2), (dict(cap=1.0), 1), ('on', 1), (1.0, 1), (dict(eta=nan), 1), (dict(norm_threshold=inf), 1),
                   (dict(norm_threshold=-1.0), 1), ([dict(momentum=nan), None], 2)):
        with pytest.raises(ValueError):
            apg_entries(bad, n)


def test_check_apg_refuses_what_apg_does_not_combine_with():
    from ezaudio_amd.sampler import apg_entries, check_apg
    rows = apg_entries([True, None], 2)
    check_apg(None, None, 0.75, compose=True, canvas=True)                       # nobody asks: nothing to refuse
    check_apg(rows, 5, 0.0)
    check_apg(rows, [5, None], [0.0, 0.75])                                      # the sample without APG may have no guidance, and a rescale
    check_apg(rows, torch.tensor([5.0, 0.0]), None)
    for kw, word in ((dict(guidance_scale=5, guidance_rescale=0.75), 'guidance_rescale'), (dict(guidance_scale=[5, 5], guidance_rescale=[0.5, 0.0]), 'guidance_rescale'),
                     (dict(guidance_scale=None, guidance_rescale=0.0), 'without guidance'), (dict(guidance_scale=[0, 5], guidance_rescale=0.0), 'without guidance'),
                     (dict(guidance_scale=5, guidance_rescale=0.0, compose=True), 'compose'), (dict(guidance_scale=5, guidance_rescale=0.0, canvas=True), 'canvas')):
        with pytest.raises(ValueError, match=word):
            check_apg(rows, **kw)


# ---------------------------------------------------------------------------------------------------
# 2. LatentSampler: prepare() refuses before it touches the device; where it sets the table; set_apg
# ---------------------------------------------------------------------------------------------------
def test_prepare_refuses_apg_with_what_it_does_not_combine_with():
    from ezaudio_amd.sampler import LatentSampler
    smp = LatentSampler.__new__(LatentSampler)                                   # (no stream, no model: the checks under test come first)
    P, Lt, Cc = 2, 4, 8
    text, tm = torch.zeros(P, Lt, Cc), torch.ones(P, Lt, dtype=torch.bool)
    init = torch.zeros(P, 3, 16)
    ct, cm = torch.zeros(P, 1, Lt, Cc), torch.ones(P, 1, Lt, dtype=torch.bool)
    for gs, gr, kw, word in ((3.5, 0.0, dict(apg=True, compose_weights=[[1.0, 0.5], [1.0, -0.5]], compose_text=ct, compose_mask=cm), 'composed guidance'),
                             (3.5, 0.0, dict(apg=True, canvas=([0, 8], 24, 1)), 'canvas'),
                             (3.5, 0.0, dict(apg=True, canvas_loop=([0, 8], 20, 1)), 'loop'),
                             (3.5, 0.75, dict(apg=True), 'guidance_rescale'),
                             ([3.5, 3.5], [0.0, 0.75], dict(apg=[None, True]), 'guidance_rescale'),
                             (None, 0.0, dict(apg=True), 'without guidance'),
                             ([3.5, None], 0.0, dict(apg=[None, dict(eta=1.0)]), 'without guidance'),
                             (3.5, 0.0, dict(apg=[True]), 'entries'),
                             (3.5, 0.0, dict(apg=dict(threshold=1.0)), 'keys')):
        with pytest.raises(ValueError, match=word):
            smp.prepare(text, tm, text, tm, init, None, gs, gr, 10, 0.0, **kw)


def test_prepare_sets_the_table_behind_the_sample_table_and_the_multistep_setter():
    from ezaudio_amd.sampler import LatentSampler
    p = inspect.signature(LatentSampler.prepare).parameters
    assert p['apg'].default is None and list(p)[-1] == 'solver'                  # a new keyword, the last one stays
    src = inspect.getsource(LatentSampler.prepare)
    order = [src.index(s) for s in ('ezdit_sampler_begin(', 'self.set_sample_params(*table)', 'u.lib.ezdit_sampler_set_multistep,', 'self._set_apg_rows(apg)')]
    assert order == sorted(order), order
    assert src.count('_set_apg_rows') == 1


class _FakeLib:
    def ezdit_sampler_set_apg(self, *a):                                          # (never called: _table_call is recorded)
        raise AssertionError


def _bare_sampler(P=2):
    from ezaudio_amd.sampler import LatentSampler
    smp = LatentSampler.__new__(LatentSampler)
    smp.P, smp.latents, smp.apg_m = P, torch.zeros(P, 4, 8), None
    smp.unet = type('U', (), dict(lib=_FakeLib()))()
    calls = []
    smp._table_call = lambda setter, *args, ok=(): calls.append((setter.__name__, args))
    return smp, calls


def test_set_apg_checks_shapes_and_hands_the_library_four_arrays_and_its_own_buffer():
    smp, calls = _bare_sampler()
    for bad in ([True], [True] * 3, dict(gamma=1), [dict(norm_threshold=-2.0), None]):
        with pytest.raises(ValueError):
            smp.set_apg(bad)
    assert not calls and smp.apg_m is None                                       # refused before anything was allocated or set
    smp.set_apg([dict(eta=0.25, norm_threshold=3.0), None])
    (name, args), = calls
    assert name == 'ezdit_sampler_set_apg' and len(args) == 6
    eta, thr, mom, on, P, buf = args
    assert (list(eta), list(thr), list(mom), list(on), P) == ([0.25, 0.0], [3.0, 0.0], [-0.5, 0.0], [1, 0], 2)
    assert smp.apg_m is not None and smp.apg_m.shape == smp.latents.shape and smp.apg_m.dtype == torch.float32 and not smp.apg_m.any()
    assert buf.value == smp.apg_m.data_ptr()
    kept = smp.apg_m
    smp.set_apg(True)                                                           # new values: the same buffer
    assert smp.apg_m is kept and calls[-1][1][5].value == kept.data_ptr() and list(calls[-1][1][3]) == [1, 1]
    for off in (None, [None, None]):
        smp.set_apg(off)
        assert calls[-1][1] == (None, None, None, None, 0, None)


# ---------------------------------------------------------------------------------------------------
# 3. inference() and the EzAudio methods
# ---------------------------------------------------------------------------------------------------
def _infer(prompts, **kw):
    from ezaudio_amd import sampler as S
    args = dict(audio_frames=8, guidance_scale=5, guidance_rescale=0.0, ddim_steps=3, eta=0, random_seed=11)
    args.update(kw)
    return S.inference(_ez().autoencoder, _Unet(), None, None, _Tok(), _enc, PARAMS, _ez().noise_scheduler, prompts, None, device='cpu', **args)


def test_the_signatures_take_apg_and_keep_their_last_keyword():
    from ezaudio_amd import api, sampler as S
    for fn, last in ((S.inference, 'solver'), (api.EzAudio.generate_audio, 'solver'), (api.EzAudio.editing_audio, 'solver'), (api.EzAudio.audio_to_audio, 'apg')):
        p = inspect.signature(fn).parameters
        assert p['apg'].default is None and list(p)[-1] == last, fn


def test_inference_passes_one_entry_per_prompt_and_nothing_when_nobody_asks(seen):
    _infer(PROMPTS, apg=True)
    assert seen[-1]['kw']['apg'] == [dict(eta=0.0, norm_threshold=0.0, momentum=-0.5)] * 3
    _infer(PROMPTS, apg=[dict(norm_threshold=4.0), None, dict(eta=0.5, momentum=0.0)], guidance_rescale=[0.0, 0.75, 0.0])
    assert seen[-1]['kw']['apg'] == [dict(eta=0.0, norm_threshold=4.0, momentum=-0.5), None, dict(eta=0.5, norm_threshold=0.0, momentum=0.0)]
    assert seen[-1]['gr'] == [0.0, 0.75, 0.0]
    _infer(PROMPTS[0], apg=dict(momentum=0.0))
    assert seen[-1]['kw']['apg'] == [dict(eta=0.0, norm_threshold=0.0, momentum=0.0)]
    for nobody in (None, False, [None] * 3):
        _infer(PROMPTS, apg=nobody)
        assert 'apg' not in seen[-1]['kw']                                       # the plain call: nothing new is passed
    n = len(seen)
    for kw, word in ((dict(apg=[True]), 'entries'), (dict(apg=True, guidance_rescale=0.75), 'guidance_rescale'), (dict(apg=True, guidance_scale=None), 'without guidance'),
                     (dict(apg=[None, True, None], guidance_scale=[5, None, 5]), 'without guidance'),
                     (dict(apg=True, compose=[[('wind', 1.0)], None, None]), 'compose'), (dict(apg=dict(cap=3)), 'keys')):
        with pytest.raises(ValueError, match=word):
            _infer(PROMPTS, **kw)
    with pytest.raises(ValueError, match='canvas'):
        _infer('rain', apg=True, canvas_offsets=[0, 4])
    with pytest.raises(ValueError, match='canvas'):
        _infer('rain', apg=True, canvas_offsets=[0, 4], canvas_loop=10)
    assert len(seen) == n                                                        # refused before anything was sampled
    # compose entries that compose nothing are the plain call, and APG goes with it
    _infer(PROMPTS, apg=True, compose=[None, [], None])
    assert len(seen[-1]['kw']['apg']) == 3 and not any(k.startswith('compose') for k in seen[-1]['kw'])


def test_generate_audio_editing_audio_and_audio_to_audio_take_apg(seen, monkeypatch):
    ez = _ez()
    ez.generate_audio('rain', 1, guidance_rescale=0, ddim_steps=20, eta=0, random_seed=3, apg=True)
    assert seen[-1]['kw']['apg'] == [dict(eta=0.0, norm_threshold=0.0, momentum=-0.5)] and seen[-1]['P'] == 1
    ez.generate_audio(PROMPTS[:2], 1, guidance_rescale=[0, 0.75], ddim_steps=20, eta=0, random_seed=3, apg=[dict(eta=0.0, norm_threshold=0.0, momentum=-0.5), None])
    assert seen[-1]['kw']['apg'] == [dict(eta=0.0, norm_threshold=0.0, momentum=-0.5), None] and seen[-1]['P'] == 2
    ez.generate_audio(PROMPTS[:2], 1, ddim_steps=20, random_seed=3)
    assert 'apg' not in seen[-1]['kw']
    n = len(seen)
    with pytest.raises(ValueError, match='guidance_rescale'):
        ez.generate_audio('rain', 1, ddim_steps=20, random_seed=3, apg=True)       # (the default rescale 0.75 is a rescale: ask for one of the two)
    with pytest.raises(ValueError, match='same size'):
        ez.generate_audio(PROMPTS[:2], 1, guidance_rescale=0, apg=[True])
    with pytest.raises(ValueError, match='list of prompts'):
        ez.generate_audio('rain', 1, guidance_rescale=0, apg=[True, None])
    with pytest.raises(ValueError, match='without guidance'):
        ez.generate_audio('', 1, guidance_rescale=0, apg=True)
    with pytest.raises(ValueError, match='compose'):
        ez.generate_audio('rain', 1, guidance_rescale=0, apg=True, compose=[('wind', 0.5)])
    assert len(seen) == n
    # audio_to_audio and editing_audio hand the argument on, and refuse before they encode anything (their own host work is covered by their own tests)
    from ezaudio_amd import api
    got, encodes = [], []
    monkeypatch.setattr(api, 'inference', lambda *a, **kw: got.append(kw) or torch.zeros(len(a[8]) if isinstance(a[8], list) else 1, 1, 160))

    def vae(audio=None, embedding=None, lengths=None):
        encodes.append(tuple(audio.shape))
        return torch.zeros(audio.shape[0], 4, 20)
    ez.autoencoder = vae
    clip = np.sin(np.arange(160, dtype=np.float32))
    ez.audio_to_audio('rain', clip, guidance_rescale=0, eta=0, apg=dict(norm_threshold=2.0))
    assert got[-1]['apg'] == dict(norm_threshold=2.0) and len(encodes) == 1
    ez.audio_to_audio('rain', clip, eta=0)
    assert 'apg' not in got[-1]
    ez.editing_audio('rain', 1, clip, 0.5, 0.5, eta=0, apg=True)                 # (editing_audio's default rescale is 0)
    assert got[-1]['apg'] is True and len(encodes) == 3
    for call in (lambda: ez.audio_to_audio('rain', clip, eta=0, apg=True), lambda: ez.audio_to_audio('', clip, guidance_rescale=0, eta=0, apg=True),
                 lambda: ez.editing_audio('rain', 1, clip, 0.5, 0.5, guidance_rescale=0.5, eta=0, apg=True),
                 lambda: ez.editing_audio('rain', 1, clip, 0.5, 0.5, eta=0, apg=[True, None])):
        with pytest.raises(ValueError):
            call()
    assert len(encodes) == 3 and len(got) == 3                                   # refused before anything was encoded


def test_a_sharded_call_slices_the_apg_entries_with_the_prompts(seen, monkeypatch):
    import torch.distributed as dist
    from ezaudio_amd import dist as ezdist
    entries = [dict(norm_threshold=4.0), None, True]
    whole = _infer(PROMPTS, apg=entries, guidance_rescale=[0.0, 0.75, 0.0])
    full = list(seen[-1]['kw']['apg'])
    seen.clear()
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda group=None: 2)

    def fake_sharded(fn, n):
        assert n == 3
        return torch.cat([fn(*ezdist.shard_range(n, r, 2)) for r in range(2)], 0)
    monkeypatch.setattr(ezdist, 'sample_sharded', fake_sharded)
    out = _infer(PROMPTS, apg=entries, guidance_rescale=[0.0, 0.75, 0.0])
    assert torch.equal(out, whole) and len(seen) == 2
    a, b = seen
    assert a['P'] == 2 and a['kw']['apg'] == full[:2] and a['gr'] == [0.0, 0.75]
    assert b['P'] == 1 and b['kw']['apg'] == full[2:] and ezdist.slice_per_prompt(entries, 2, 3, 3) == [True]
    # a shard whose prompts ask for nothing is the plain call; one value for the call goes to every shard
    seen.clear()
    _infer(PROMPTS, apg=[None, None, True])
    assert 'apg' not in seen[0]['kw'] and seen[1]['kw']['apg'] == full[2:]
    assert ezdist.slice_per_prompt(True, 0, 2, 3) is True and ezdist.slice_per_prompt(None, 0, 2, 3) is None
    with pytest.raises(ValueError):
        ezdist.slice_per_prompt([True, None], 0, 2, 3)


# ---------------------------------------------------------------------------------------------------
# 4. the C ABI, as far as it goes without a GPU
# ---------------------------------------------------------------------------------------------------
def test_the_header_declares_and_the_binding_binds_the_apg_entry_points(lib):
    from ezaudio_amd import _lib
    from oracle.weights import model_config
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ezdit.h')).read(), flags=re.S)
    for name, nargs in (('ezdit_sampler_set_apg', 8), ('ezdit_cfg_apg_step', 12)):
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
        f1, i1 = (C.c_float * 1)(0.0), (C.c_int32 * 1)(1)
        assert lib.ezdit_sampler_set_apg(h, f1, f1, f1, i1, 1, None, None) == -3 and b'ezdit_sampler_begin' in lib.ezdit_last_error()
        assert lib.ezdit_sampler_set_apg(h, None, None, None, None, 0, None, None) == -3
        assert lib.ezdit_sampler_set_apg(None, f1, f1, f1, i1, 1, None, None) == -1
        # the table has a workspace region of its own: 16 B bytes, rounded up to 256
        grow = lambda B: lib.ezdit_workspace_bytes(h, B, 96, 20, 20)   # noqa: E731
        assert grow(2) > 0
    finally:
        lib.ezdit_destroy(h)
    assert lib.ezdit_cfg_apg_step(None, None, None, None, None, None, None, 0, 1, 128, None, None) == -1
