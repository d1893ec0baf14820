"""CPU tests of composed guidance (tests/compose_emul.py): the definition in float64 and its identities, the fp32 emulation in the kernels' order and its
distance from float64 -- the floor the GPU gate of tests/test_compose_gpu.py is a multiple of -- eight deliberate mistakes that must each stand well clear of
it and be refused by the GPU test's own checking code, the oracle-loop goldens of tools/mint_compose_golden.py, and the new surface: the exports of the
header and the library, the ``compose`` argument of inference() and generate_audio()."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import compose_emul as E
from tests.util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ('ezdit_sampler_begin_composed', 'ezdit_sampler_set_compose_weights', 'ezdit_cfg_compose_step')


# ---------------------------------------------------------------------------------------------------
# 1. the definition: identities in float64
# ---------------------------------------------------------------------------------------------------
def _vectors(seed=3, n=(16, 37), K=3):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(n) * 1.3
    return [0.6 * base + 0.8 * rng.standard_normal(n) for _ in range(K)], 0.6 * base + 0.8 * rng.standard_normal(n)


def test_one_condition_with_weight_1_is_cfg_combine_and_rescale_noise_cfg():
    """oracle/sampler.py computes the statistics in float32 (as the reference does), so the agreement is that of a float32 standard deviation: 1e-6."""
    from oracle.sampler import cfg_combine, rescale_noise_cfg
    (c, *_), u = _vectors()
    for g, phi in ((1.0, 0.0), (3.5, 0.0), (5.0, 0.75), (2.0, 0.4)):
        want = cfg_combine(c[None], u[None], g)
        if phi > 0:
            want = rescale_noise_cfg(want, c[None], phi)
        got = E.combine_fp64([c], u, [1.0], g, phi)
        assert E.rel_l2(got, want[0]) < (1e-6 if phi > 0 else 1e-13), (g, phi)
    assert np.array_equal(E.combine_fp64([c], u, [1.0], 0.0, 0.75), c)          # no guidance: the conditional prediction alone


def test_two_equal_conditions_are_one_condition_at_the_summed_weight():
    (c, c1, _), u = _vectors(5)
    for a, b, g, phi in ((1.0, 0.5, 3.5, 0.0), (0.7, -0.2, 5.0, 0.75), (2.0, 1.0, 2.0, 0.4)):
        two = E.combine_fp64([c, c], u, [a, b], g, phi)
        one = E.combine_fp64([c], u, [1.0], g * (a + b), phi)
        assert E.rel_l2(two, one) < 1e-13, (a, b)
    # a weight of 0 drops its row: whatever it holds, NaN included
    bad = np.full_like(c1, np.nan)
    assert np.array_equal(E.combine_fp64([c, bad, c1], u, [1.0, 0.0, -0.5], 3.5, 0.75), E.combine_fp64([c, c1], u, [1.0, -0.5], 3.5, 0.75))
    # a negative weight keeps the unconditional baseline: v - u is the weighted sum of the directions
    v = E.combine_fp64([c, c1], u, [1.0, -0.5], 3.5, 0.0)
    assert E.rel_l2(v - u, 3.5 * ((c - u) - 0.5 * (c1 - u))) < 1e-13
    # the rescale reference is the primary condition: the guided prediction takes ITS standard deviation at phi = 1
    v = E.combine_fp64([c, c1], u, [1.0, 0.8], 5.0, 1.0)
    assert abs(v.std(ddof=1) / c.std(ddof=1) - 1) < 1e-13


def test_the_step_in_float64_drops_what_must_not_be_read():
    """The poisoned copy of a case -- NaN in the rows of weight 0, the padded frames, the noise slice of the sigma = 0 sample, the history of the c_hist = 0
    sample, every row but c_0 of the sample without guidance -- gives the result of the clean one, in the definition and in the emulation."""
    for K, lens, ms in ((3, (131, 77, 1), False), (3, (131, 77, 1), True), (2, None, False)):
        case = E.operator_case(K, lens, ms)
        bad = E.poisoned(case)
        assert np.isnan(bad['pred']).any()
        for run in (E.run_fp64, E.run_emul):
            a, b = run(case), run(bad)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.isfinite(b[0]).all()


# ---------------------------------------------------------------------------------------------------
# 2. the emulation's floor, the eight mistakes, the GPU test's checking code
# ---------------------------------------------------------------------------------------------------
def _mistake_case():
    """K = 3 with lengths (131, 77, 1), the multistep form (it has the history output): sample 0 rescales and has padded frames, sample 1 has a weight of 0."""
    return E.operator_case(3, (131, 77, 1), True)


def test_identity_k1_w1_in_the_emulation_is_the_plain_expression_bit_for_bit():
    """u + g (1 (c - u)) is u + g (c - u) in fp32: the composed kernels with K = 1, w = 1 can give the plain operator's bits."""
    case = dict(E.operator_case(1, None, True), weights=np.ones((3, 1), np.float32))
    got, hgot = E.run_emul(case)
    f, P = np.float32, 3
    for p in (1, 2):                                                   # (the samples without rescale: one expression to write down)
        g, _, sa, sb, cx0, cdir, _, ch = (f(t) for t in case['params'][p])
        c, u, x = case['pred'][p], case['pred'][P + p], case['lat'][p]
        v = u + g * (c - u) if g > 0 else c
        x0 = sa * x - sb * v
        prev = cx0 * x0 + cdir * (sa * v + sb * x)
        if ch != 0:
            prev = prev + ch * (x0 - case['hist'][p])
        assert np.array_equal(got[p], prev) and np.array_equal(hgot[p], x0), p


def test_every_deliberate_mistake_stands_ten_floors_clear_of_float64():
    """The floor is the emulation's largest distance from float64 over ALL operator cases of the GPU test (E.operator_floor); the mistakes are built into the
    K = 3 case with lengths.  'weight0_row_read' shows only when the row holds something that 0 x does not erase, so it runs on the poisoned inputs and comes
    out non-finite (distance inf); 'stats_over_padding' needs finite padded frames and runs on the clean ones.
    Measured: floor 8.7e-8; the nearest mistakes 'stats_over_padding' 3.2e-4 (3 600 floors) and 'rescale_ref_weighted_mean' 1.2e-2."""
    floor = E.operator_floor()
    case = _mistake_case()
    ref = E.run_fp64(case)
    far = {}
    for mk in E.MISTAKES:
        inputs = E.poisoned(case) if mk == 'weight0_row_read' else case
        far[mk] = E.distance(E.run_emul(inputs, mistake=mk), ref, case['lens'])
    print(f'composed-guidance emulation floor (largest rel-L2 vs fp64 over the operator cases, latents and x0_hist): {floor:.3e}')
    for mk in E.MISTAKES:
        print(f'  mistake {mk:28s}: {far[mk]:.3e} = {far[mk] / floor:.1f} floors')
    assert 0 < floor < 1e-6
    assert len(E.MISTAKES) == 8 and set(far) == set(E.MISTAKES)
    for mk, dist in far.items():
        assert dist >= 10 * floor, (mk, dist, floor)
    # no mistake: inside one floor by construction, padded frames exactly zero
    got = E.run_emul(case)
    assert E.distance(got, ref, case['lens']) <= floor
    for t in got:
        for p, n in enumerate(case['lens']):
            assert not t[p, :, n:].any()


def test_the_gpu_tests_checking_code_refuses_every_mistake():
    """E.check_outputs is what tests/test_compose_gpu.py asserts with: it passes the emulation (on clean and on poisoned inputs) and refuses each mistake."""
    case = _mistake_case()
    for inputs in (case, E.poisoned(case)):
        d = E.check_outputs(*E.run_emul(inputs), case)
        assert max(d.values()) < E.GATE_FLOORS * E.operator_floor()
    for mk in E.MISTAKES:
        inputs = E.poisoned(case) if mk == 'weight0_row_read' else case
        with pytest.raises(AssertionError):
            E.check_outputs(*E.run_emul(inputs, mistake=mk), case)
    # ... and values left behind on padded frames
    got, hgot = E.run_emul(case)
    got[0, :, 140] = 1e-30
    with pytest.raises(AssertionError, match='padded'):
        E.check_outputs(got, hgot, case)


# ---------------------------------------------------------------------------------------------------
# 3. the goldens of the fused loop (tools/mint_compose_golden.py)
# ---------------------------------------------------------------------------------------------------
def test_the_loop_goldens_tell_composition_from_plain_cfg():
    """tests/golden/sampler_compose_xs.npz: the numpy oracle's 20-step loop on smp_xs_e0's inputs with the float64 combination, K = 2, DDIM and dpmpp_2m.  The
    mint tool chose the second weight so that each golden lies at least 10 loop gates (10 x 2e-2) from the plain-CFG loop of the same inputs."""
    g, meta = load_golden('sampler_compose_xs')
    base = load_golden('sampler_smp_xs_e0')[1]
    assert meta['base'] == 'smp_xs_e0' and meta['steps'] == 20 and meta['K'] == 2
    for key in ('size', 'L', 'Lc', 'seed_w', 'seed_in', 'guidance_scale', 'guidance_rescale', 'with_gt'):
        assert meta[key] == base[key], key
    assert meta['weights'][0] == 1.0 and meta['weights'][1] != 0.0 and len(meta['weights']) == 2
    for key, dist in (('latent_ddim', meta['dist_ddim']), ('latent_2m', meta['dist_2m'])):
        assert g[key].shape == (1, 128, meta['L']) and g[key].dtype == np.float32 and np.isfinite(g[key]).all()
        assert dist >= 10 * 2e-2, (key, dist)
    assert E.rel_l2(g['latent_2m'], g['latent_ddim']) > 1e-3          # two solvers, two goldens


# ---------------------------------------------------------------------------------------------------
# 4. the new surface
# ---------------------------------------------------------------------------------------------------
def test_the_header_and_the_library_export_the_composed_entry_points(lib):
    header = open(os.path.join(ROOT, 'include', 'ezdit.h')).read()
    for name in NEW_EXPORTS:
        assert re.search(r'^int %s\(' % name, header, re.M), name
        assert hasattr(lib, name), name
    assert re.search(r'#define EZDIT_COMPOSE_MAX %d\b' % E.K_MAX, header)
    assert '#define EZDIT_ABI_VERSION 4 ' in header and lib.ezdit_abi_version() == 4      # additive: the version stays


def test_inference_and_generate_audio_accept_compose():
    from ezaudio_amd import api, sampler
    assert inspect.signature(sampler.inference).parameters['compose'].default is None
    assert inspect.signature(api.EzAudio.generate_audio).parameters['compose'].default is None
    p = inspect.signature(sampler.LatentSampler.prepare).parameters
    assert all(p[k].default is None for k in ('compose_text', 'compose_mask', 'compose_weights'))
    assert sampler.COMPOSE_MAX == E.K_MAX


def test_compose_entries_pads_with_weight_zero_and_refuses_bad_lists():
    from ezaudio_amd.sampler import compose_entries
    lists, W = compose_entries([('distant thunder', 0.8), ('wind', -0.5)], 1)
    assert lists == [[('distant thunder', 0.8), ('wind', -0.5)]] and np.allclose(W.numpy(), [[1.0, 0.8, -0.5]])
    lists, W = compose_entries([[('a', 0.8)], None, [('x', 1), ('y', 2)]], 3)
    assert [len(c) for c in lists] == [1, 0, 2]
    assert np.array_equal(W.numpy(), np.array([[1, 0.8, 0], [1, 0, 0], [1, 1, 2]], np.float32))
    assert compose_entries([None, []], 2) == (None, None)               # nobody composes anything: the plain call
    for bad, n in (([('a', 1.0)], 2), ([[('a', float('nan'))]], 1), ([[('a', float('inf'))]], 1), ([['a']], 1), ([[(1, 2)]], 1),
                   ([[('p%d' % i, 1.0) for i in range(8)]], 1)):
        with pytest.raises(ValueError):
            compose_entries(bad, n)


def test_prepare_refuses_composition_with_what_it_does_not_combine_with():
    """The refusals that need no GPU: they come before anything is bound."""
    from ezaudio_amd.sampler import LatentSampler
    smp = LatentSampler.__new__(LatentSampler)                          # (no stream, no model: the checks under test come first)
    P, Lt, Cc = 2, 4, 8
    text, tm = torch.zeros(P, Lt, Cc), torch.ones(P, Lt, dtype=torch.bool)
    init = torch.zeros(P, 3, 16)
    ct, cm = torch.zeros(P, 1, Lt, Cc), torch.ones(P, 1, Lt, dtype=torch.bool)
    args = (text, tm, text, tm, init, None, 3.5, 0.0, 10, 0.0)
    w = [[1.0, 0.5], [1.0, -0.5]]
    for kw, msg in ((dict(compose_weights=w, compose_text=ct, compose_mask=cm, controlnet=object()), 'ControlNet'),
                    (dict(compose_weights=w, compose_text=ct, compose_mask=cm, canvas=([0, 8], 24, 1)), 'canvas'),
                    (dict(compose_weights=w, compose_text=ct, compose_mask=cm, canvas_loop=([0, 8], 20, 1)), 'loop'),
                    (dict(compose_weights=[[0.0, 1.0], [1.0, 1.0]], compose_text=ct, compose_mask=cm), 'above 0'),
                    (dict(compose_weights=[[1.0, float('nan')], [1.0, 1.0]], compose_text=ct, compose_mask=cm), 'finite'),
                    (dict(compose_weights=w), 'compose_text'),
                    (dict(compose_text=ct, compose_mask=cm), 'without compose_weights'),
                    (dict(compose_weights=[[1.0] * 9] * 2), 'K'),
                    (dict(compose_weights=[[1.0, 0.5]], compose_text=ct, compose_mask=cm), r'\[P=2, K\]')):
        with pytest.raises(ValueError, match=msg):
            smp.prepare(*args, **kw)


def test_generate_audio_builds_the_composed_call_in_one_encoder_batch(monkeypatch):
    """generate_audio(compose=) against the stand-ins of tests/test_canvas_host.py: one text-encoder batch holds every prompt of the call; prepare() receives the
    primaries as `text`, the extras as compose_text [N, K-1, Lt, Cctx] in the prompts' order (a missing one: the prompt's own text) and the weights [N, K]."""
    from ezaudio_amd import sampler as S
    from tests.test_canvas_host import _RecordingSampler, _enc, _ez
    monkeypatch.setattr(S, 'LatentSampler', _RecordingSampler)
    _RecordingSampler.seen.clear()
    ez = _ez()
    batches = []

    def enc(input_ids, attention_mask):
        batches.append(input_ids.shape[0])
        return _enc(input_ids, attention_mask)
    ez.text_encoder = enc
    tok = lambda texts: ez.tokenizer(texts, 8, 'max_length', True, 'pt')   # noqa: E731
    hidden = lambda texts: _enc(tok(texts).input_ids, None).last_hidden_state   # noqa: E731
    ez.generate_audio('rain', 1, ddim_steps=20, eta=0, random_seed=3, compose=[('distant thunder', 0.8), ('wind', -0.5)])
    one = _RecordingSampler.seen[-1]
    assert batches == [3, 1]                                           # the three prompts together, then the negative prompt
    assert one['P'] == 1 and torch.equal(one['text'], hidden(['rain']))
    assert torch.equal(one['kw']['compose_text'], hidden(['distant thunder', 'wind'])[None])
    assert one['kw']['compose_mask'].shape == (1, 2, 8) and one['kw']['compose_mask'].dtype == torch.bool
    assert np.allclose(one['kw']['compose_weights'].numpy(), [[1.0, 0.8, -0.5]])
    del batches[:]
    ez.generate_audio(['rain', 'a dog', 'birds'], 1, ddim_steps=20, eta=0, random_seed=3, compose=[[('thunder', 0.8)], None, [('wind', 1.0), ('a car', -1.0)]])
    many = _RecordingSampler.seen[-1]
    assert batches == [9, 3] and many['P'] == 3
    want = torch.stack([hidden(['thunder', 'rain']), hidden(['a dog', 'a dog']), hidden(['wind', 'a car'])])
    assert torch.equal(many['kw']['compose_text'], want) and torch.equal(many['text'], hidden(['rain', 'a dog', 'birds']))
    assert np.array_equal(many['kw']['compose_weights'].numpy(), np.array([[1, 0.8, 0], [1, 0, 0], [1, 1, -1]], np.float32))
    # nobody composes anything: the plain call, nothing new is passed
    ez.generate_audio(['rain', 'a dog'], 1, ddim_steps=20, eta=0, random_seed=3, compose=[None, []])
    assert not any(k.startswith('compose') for k in _RecordingSampler.seen[-1]['kw'])
    # refusals of inference(): a list of another size, a canvas, a timeline
    with pytest.raises(ValueError, match='same size'):
        ez.generate_audio(['rain', 'a dog'], 1, compose=[[('wind', 1.0)]])
    args = (ez.autoencoder, ez.unet, None, None, ez.tokenizer, ez.text_encoder, ez.params, ez.noise_scheduler)
    rest = (None, 6, 3, 0.0, 20, 0, 1, 'cpu')
    with pytest.raises(ValueError, match='canvas'):
        S.inference(*args, 'rain', *rest, canvas_offsets=[0, 4], compose=[('wind', 1.0)])
    with pytest.raises(ValueError, match='timeline'):
        S.inference(*args, [['rain', 'wind']], *rest, prompt_weights=[np.ones((2, 6), np.float32)], compose=[[('wind', 1.0)]])
    with pytest.raises(ValueError, match='ControlNet'):
        S.inference(*args, 'rain', *rest, controlnet=object(), condition=torch.zeros(1, 1, 12), compose=[('wind', 1.0)])
