"""Prompt emphasis end to end (run with -m gpu on an MI355X): MaskDiT.forward and the fused sampler with per-token weights (include/ezdit.h
ezdit_set_context_token_weights).  The definition is checked on the GPU itself: integer weights against the same forward on the context with those rows repeated, at four
times the GPU's own reorder floor (the distance between two runs of the repeated context with its rows permuted).  A table of equal weights is the plain call bit for bit
with the same launch count; new values replay the captured step, on <-> off captures again, a refused call changes nothing.  The kernel's arithmetic against fp64 is
tests/test_attention_keyweight_gpu.py's."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.weights import make_inputs, make_state_dict, model_config
from tests.util import record, rel_l2

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
L, LC, NV = 96, 20, 20
_models = {}


def get_model(size):
    from ezaudio_amd import MaskDiT
    if size not in _models:
        cfg = model_config(size)
        m = MaskDiT(device=DEV, **cfg)
        m.load_state_dict(make_state_dict(cfg, 1))
        _models[size] = (m, cfg)
    return _models[size]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _fwd(m, inp, ctx=None, mask=None, w=None, t=499):
    ctx = inp['ctx'] if ctx is None else ctx
    mask = inp['ctx_mask'] if mask is None else mask
    kw = {} if w is None else dict(context_token_weights=torch.as_tensor(w))
    out, _ = m(_t(inp['x']), torch.tensor(t), _t(ctx), context_mask=_t(mask), **kw)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize('size', ['xs', 'xs64'])
def test_integer_weights_are_the_forward_on_the_repeated_context(lib, size):
    """3 of 20 tokens weighted 8: the forward with the table against the forward without one on the context in which those three rows stand eight times."""
    m, cfg = get_model(size)
    inp = make_inputs(cfg, B=1, L=L, Lc=LC, n_valid=(NV,), seed=11)
    w = np.ones((1, LC), dtype=np.float32)
    heavy = [2, 7, 13]
    w[0, heavy] = 8.0
    rep = np.concatenate([np.arange(LC)] + [np.full(7, j) for j in heavy])
    ctx_rep, mask_rep = inp['ctx'][:, rep], inp['ctx_mask'][:, rep]
    perm = np.random.RandomState(3).permutation(len(rep))
    plain = _fwd(m, inp)
    weighted = _fwd(m, inp, w=w)
    dup = _fwd(m, inp, ctx_rep, mask_rep)
    dup_perm = _fwd(m, inp, ctx_rep[:, perm], mask_rep[:, perm])
    floor = rel_l2(dup_perm.numpy(), dup.numpy())
    dist = rel_l2(weighted.numpy(), dup.numpy())
    away = rel_l2(weighted.numpy(), plain.numpy())
    record(f'emphasis {size}: weighted forward vs repeated context rel-L2 {dist:.3e}, reorder floor of the repeated context {floor:.3e}, weighted vs unweighted {away:.3e}')
    assert torch.isfinite(weighted).all()
    assert floor > 0 and dist <= 4 * floor and dist <= 2e-2, (dist, floor)
    assert away > 10 * max(dist, floor), (away, dist)      # the table does something, far above what it is compared at


@pytest.mark.parametrize('size', ['xs', 'xs64'])
def test_equal_weights_and_off_after_on_are_the_plain_call(lib, size):
    m, cfg = get_model(size)
    inp = make_inputs(cfg, B=2, L=L, Lc=LC, n_valid=(NV, 1), seed=12)
    plain = _fwd(m, inp)
    n_plain = m.last_launch_count
    nan = np.full((2, LC), np.nan, dtype=np.float32)      # values at masked keys are not read
    ones, three = nan.copy(), nan.copy()
    ones[inp['ctx_mask']] = 1.0
    three[inp['ctx_mask']] = 3.0
    three[1][inp['ctx_mask'][1]] = 0.25                   # (each row uniform, at its own value)
    for name, w in (('all weights 1', ones), ('uniform rows', three)):
        assert torch.equal(_fwd(m, inp, w=w), plain), name
        assert m.last_launch_count == n_plain, name
    w = ones.copy()
    w[0, 3] = 4.0
    on = _fwd(m, inp, w=w)
    assert m.last_launch_count == n_plain, 'the table changes the launch count'
    assert torch.isfinite(on).all() and not torch.equal(on, plain)
    assert torch.equal(on[1], plain[1]), 'the single-key row must not change'
    assert torch.equal(_fwd(m, inp), plain), 'off after on'
    assert m.last_launch_count == n_plain


def test_refusals_change_nothing(lib):
    m, cfg = get_model('xs')
    inp = make_inputs(cfg, B=2, L=L, Lc=LC, n_valid=(NV, 1), seed=13)
    w = np.ones((2, LC), dtype=np.float32)
    w[0, 5] = 2.0
    ref = _fwd(m, inp, w=w)

    def rerun():
        out = torch.empty(2, cfg['out_chans'], L, dtype=torch.float32, device=DEV)
        x = _t(inp['x'])
        from ezaudio_amd import _lib
        _lib.check(m.lib.ezdit_forward(m._h, x.data_ptr(), cfg['out_chans'], 2, None, None, None, 0, out.data_ptr(), None))
        torch.cuda.synchronize()
        return out.cpu()
    assert torch.equal(rerun(), ref)
    bad_nan, bad_zero, bad_ratio = w.copy(), w.copy(), w.copy()
    bad_nan[0, 1] = np.nan
    bad_zero[0, 1] = 0.0
    bad_ratio[0, 1] = 2.0 ** 21.5
    for bad in (bad_nan, bad_zero, bad_ratio):
        with pytest.raises(AssertionError):
            m.set_context_token_weights(bad)
        assert torch.equal(rerun(), ref), 'a refused call changed the table'
    with pytest.raises(AssertionError):      # n != B
        arr = (C.c_float * LC)(*([1.0] * LC))
        from ezaudio_amd import _lib
        _lib.check(m.lib.ezdit_set_context_token_weights(m._h, arr, 1, None))
    assert torch.equal(rerun(), ref)
    # the timeline and the token weights refuse each other, in both directions
    inp128 = make_inputs(cfg, B=1, L=L, Lc=128, n_valid=(NV,), seed=14)
    w128 = np.ones((1, 128), dtype=np.float32)
    w128[0, 2] = 3.0
    on = _fwd(m, inp128, w=w128)
    with pytest.raises(NotImplementedError):
        m.set_context_weights(torch.ones(1, 1, L))
    out = torch.empty(1, cfg['out_chans'], L, dtype=torch.float32, device=DEV)
    from ezaudio_amd import _lib
    x = _t(inp128['x'])
    _lib.check(m.lib.ezdit_forward(m._h, x.data_ptr(), cfg['out_chans'], 1, None, None, None, 0, out.data_ptr(), None))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), on)
    m.set_context_token_weights(None)
    m.set_context_weights(torch.ones(1, 1, L))
    with pytest.raises(NotImplementedError):
        m.set_context_token_weights(w128)
    m.set_context_weights(None)


def _scheduler():
    from ezaudio_amd.scheduler import DDIMScheduler
    return DDIMScheduler(num_train_timesteps=1000, beta_schedule='scaled_linear', beta_start=0.00085, beta_end=0.012, prediction_type='v_prediction',
                         rescale_betas_zero_snr=True, timestep_spacing='trailing', clip_sample=False)


def _sampler(m, cfg, text, mask, tw, seed, K=4, rows=None, **kw):
    from ezaudio_amd.sampler import LatentSampler
    P = text.shape[0]
    g = torch.Generator().manual_seed(seed)
    init = torch.randn(P, cfg['out_chans'], L, generator=g)
    if rows is not None:
        init = init[rows]
        text, mask, tw = text[rows], mask[rows], None if tw is None else tw[rows]
        kw = {k: v[rows] for k, v in kw.items()}
        P = len(rows)
    un = torch.randn(1, LC, cfg['context_dim'], generator=torch.Generator().manual_seed(77)).expand(P, -1, -1).contiguous()
    um = torch.zeros(P, LC, dtype=torch.bool); um[:, 0] = True      # the encoding of '': one valid key
    smp = LatentSampler(m, _scheduler())
    smp.prepare(text.to(DEV), mask.to(DEV), un.to(DEV), um.to(DEV), init.to(DEV), None, 3.0, 0.5, K, 0.0, token_weights=tw, **kw)
    return smp


def _prompts(cfg, P, seed):
    g = torch.Generator().manual_seed(seed)
    text = torch.randn(P, LC, cfg['context_dim'], generator=g)
    mask = torch.zeros(P, LC, dtype=torch.bool)
    for p in range(P):
        mask[p, :NV - 3 * p] = True
    tw = torch.ones(P, LC)
    tw[0, 2:5] = 1.6
    tw[1:, 7] = 0.5
    tw[~mask] = float('nan')
    return text, mask, tw


def test_cfg_batch_of_two_is_each_samples_single_call(lib):
    m, cfg = get_model('xs')
    text, mask, tw = _prompts(cfg, 2, 21)
    both = _sampler(m, cfg, text, mask, tw, 5)
    both.run(use_graph=True)
    got = both.finish().clone()
    plain = _sampler(m, cfg, text, mask, None, 5)
    plain.run(use_graph=True)
    base = plain.finish().clone()
    assert torch.isfinite(got).all()
    for p in range(2):
        one = _sampler(m, cfg, text, mask, tw, 5, rows=[p])
        one.run(use_graph=True)
        assert torch.equal(one.finish()[0], got[p]), f'sample {p} differs from its single call'
        assert not torch.equal(got[p], base[p]), f'sample {p}: the weights changed nothing'


def test_new_values_replay_the_graph_and_on_off_capture_again(lib, capfd):
    m, cfg = get_model('xs')
    text, mask, tw = _prompts(cfg, 1, 22)
    K = 6
    smp = _sampler(m, cfg, text, mask, tw, 6, K=K)
    st = C.c_void_p(smp.stream.cuda_stream)
    full = lambda w: torch.cat([torch.nan_to_num(w, nan=1.0), torch.ones(1, LC)], 0)      # noqa: E731  the CFG batch: the unconditional row weighs 1
    tw2 = tw.clone(); tw2[0, 9] = 3.0
    assert lib.ezdit_set_option(m._h, b'trace_launches', 1) == 0
    try:
        def captured():
            capfd.readouterr()
            smp.run(1, use_graph=True)
            smp.stream.synchronize()
            return 'launch ' in capfd.readouterr().err
        assert captured(), 'first run'
        assert not captured(), 'second run replays'
        with torch.cuda.stream(smp.stream):
            m.set_context_token_weights(full(tw2), st)
        assert not captured(), 'new values into a table that is on keep the graph'
        with torch.cuda.stream(smp.stream):
            m.set_context_token_weights(None, st)
        assert captured(), 'off drops the graph'
        with torch.cuda.stream(smp.stream):
            m.set_context_token_weights(full(tw), st)
        assert captured(), 'on drops the graph'
        assert torch.isfinite(smp.finish()).all()
    finally:
        assert lib.ezdit_set_option(m._h, b'trace_launches', 0) == 0
    # new values behind a replayed graph equal a fresh call with them: two steps under tw, then the rest under tw2, graph against eager
    outs = []
    for graph in (True, False):
        s2 = _sampler(m, cfg, text, mask, tw, 6, K=K)
        s2.run(2, use_graph=graph)
        with torch.cuda.stream(s2.stream):
            m.set_context_token_weights(full(tw2), C.c_void_p(s2.stream.cuda_stream))
        s2.run(K - 2, use_graph=graph)
        outs.append(s2.finish().clone())
    assert torch.equal(outs[0], outs[1])


def test_composed_rows_take_their_own_weights(lib):
    """K = 2 conditions per sample with different token weights: prepare() builds the [B][Lc] table in the batch layout [c_0 | c_1 | u]; the explicit per-row table through
    the setter gives the same bits, and so does neither differ from a finite result that the weights move."""
    m, cfg = get_model('xs')
    P = 2
    text, mask, tw = _prompts(cfg, P, 23)
    text2, mask2, _ = _prompts(cfg, P, 24)
    tw2 = torch.ones(P, 1, LC); tw2[:, 0, 1] = 2.5
    cw = torch.tensor([[1.0, 0.6], [1.0, -0.4]])
    kw = dict(compose_text=text2[:, None].to(DEV), compose_mask=mask2[:, None].to(DEV), compose_weights=cw)
    a = _sampler(m, cfg, text, mask, tw, 7, compose_token_weights=tw2, **kw)
    a.run(use_graph=True)
    got = a.finish().clone()
    b = _sampler(m, cfg, text, mask, None, 7, **kw)      # the plain composed call, then the explicit table [c_0 rows | c_1 rows | u rows]
    table = torch.cat([torch.nan_to_num(tw, nan=1.0), tw2[:, 0], torch.ones(P, LC)], 0)
    with torch.cuda.stream(b.stream):
        m.set_context_token_weights(table, C.c_void_p(b.stream.cuda_stream))
    b.run(use_graph=True)
    assert torch.equal(b.finish(), got)
    c = _sampler(m, cfg, text, mask, None, 7, **kw)
    c.run(use_graph=True)
    assert torch.isfinite(got).all() and not torch.equal(c.finish(), got)


# ---------------------------------------------------------------------------------------------------
# against the numpy oracle (tools/mint_emphasis_golden.py): the integer set from the UNMODIFIED oracle on the duplicated context, the fractional set from its subclass
# ---------------------------------------------------------------------------------------------------
REL_TOL, ABS_TOL, LOOP_GATE = 2e-2, 0.15, 2e-2      # tests/test_gpu.py; the loop gate of tests/test_timeline_gpu.py


@pytest.mark.parametrize('name', ['xs', 'xs64'])
def test_forward_matches_both_golden_sets(lib, name):
    from tests.util import golden_case, load_golden
    cfg, sd, inp, kw, g0, meta = golden_case(name)
    g, em = load_golden('forward_emphasis_' + name)
    assert em['base'] == 'dit_' + name and em['L'] == L and em['LT'] == LC and meta['seed_w'] == 1 and not kw
    m, _ = get_model(meta['size'])
    ctx = _t(g['ctx'])
    msk = torch.ones(ctx.shape[:2], dtype=torch.bool, device=DEV)
    for kind in ('int', 'frac'):
        for t in meta['timesteps']:
            pred = m.forward(_t(inp['x']), torch.tensor(t), ctx, context_mask=msk, context_token_weights=torch.from_numpy(g['w_' + kind]))[0].cpu().numpy()
            ref = g[f'pred_{kind}_t{t}']
            r, a = rel_l2(pred, ref), float(np.abs(pred - ref).max())
            record(f'forward_emphasis_{name} {kind} t={t}: rel-L2 {r:.3e} max-abs {a:.3e} vs the oracle; {rel_l2(pred, g[f"plain_t{t}"]):.3e} from the unweighted oracle result '
                   f'(the golden is {em[kind + "_vs_plain"]:.3e} from it at the first timestep)')
            assert np.isfinite(pred).all()
            assert r < REL_TOL and a < ABS_TOL * max(1.0, float(ref.std()) / 1.48), (name, kind, t, r, a)


def test_sampler_loop_matches_the_oracle_loop(lib):
    """The inputs of smp_xs_e0, 20 steps, DDIM and dpmpp_2m, the conditional row weighted, the unconditional row single-key: <= 2e-2 against the oracle loop."""
    from ezaudio_amd.sampler import LatentSampler
    from ezaudio_amd.scheduler import DDIMScheduler
    from tests.util import DIFF, load_golden, sampler_case
    cfg, sd, inp, init, noises, g1, meta = sampler_case('smp_xs_e0')
    g, em = load_golden('sampler_emphasis_xs')
    assert em['base'] == 'smp_xs_e0' and em['steps'] == meta['steps'] == 20 and meta['seed_w'] == 1
    m, _ = get_model('xs')
    gt, gm = _t(inp['gt'][0:1]), _t(inp['gt_mask'][0:1])
    for solver in ('ddim', 'dpmpp_2m'):
        smp = LatentSampler(m, DDIMScheduler(**DIFF))
        smp.prepare(_t(inp['ctx'][0:1]), _t(inp['ctx_mask'][0:1]), _t(inp['ctx'][1:2]), _t(inp['ctx_mask'][1:2]), _t(init), None, meta['guidance_scale'],
                    meta['guidance_rescale'], meta['steps'], 0.0, gt=gt, gt_mask=gm, solver=solver, token_weights=torch.from_numpy(g['weights']))
        smp.run(use_graph=True)
        lat = smp.finish()
        fin = torch.where(gm, lat, gt).cpu().numpy()      # src/inference.py:104-105
        e = rel_l2(fin, g['latent_' + solver])
        record(f'sampler_emphasis_xs {solver}, {meta["steps"]} steps: final-latent rel-L2 vs the numpy oracle loop with the weights {e:.3e}; '
               f'{rel_l2(fin, g1["latent"]):.3e} from the unweighted golden (oracle, DDIM: {em["weighted_vs_plain_ddim"]:.3e})')
        assert torch.isfinite(lat).all() and e < LOOP_GATE, (solver, e)


def test_refusals_with_a_controlnet(lib):
    """The setter on a ControlNet handle, the setter with a ControlNet attached, the attach with the table on, and prepare() with both: every one refused, and the run
    that follows is bitwise what it was."""
    from ezaudio_amd import DiTControlNet
    from oracle.controlnet import CN_DEFAULT
    m, cfg = get_model('xs')
    text, mask, tw = _prompts(cfg, 2, 31)
    K = 3
    ref = _sampler(m, cfg, text, mask, tw, 9, K=K)
    ref.run(use_graph=True)
    ref = ref.finish().clone()
    ccfg = dict(cfg)
    ccfg.update(CN_DEFAULT)
    cn = DiTControlNet(device=DEV, **ccfg)
    full = torch.cat([torch.nan_to_num(tw, nan=1.0), torch.ones(2, LC)], 0).contiguous()
    arr = (C.c_float * full.numel())(*full.reshape(-1).tolist())
    smp = _sampler(m, cfg, text, mask, tw, 9, K=K)
    st = C.c_void_p(smp.stream.cuda_stream)
    try:
        # the table is on (prepare set it)
        assert lib.ezdit_sampler_attach_controlnet(m._h, cn._h, 1.0) == -2 and b'token weights' in lib.ezdit_last_error()
        assert lib.ezdit_set_context_token_weights(cn._h, arr, 4, st) == -2 and b'ControlNet' in lib.ezdit_last_error()
        smp.run(use_graph=True)
        assert torch.equal(smp.finish(), ref), 'a refused call changed the run'
        # the other order: table off, a ControlNet attached, the setter refused; detached, the setter works again
        smp = _sampler(m, cfg, text, mask, tw, 9, K=K)
        st = C.c_void_p(smp.stream.cuda_stream)
        with torch.cuda.stream(smp.stream):
            m.set_context_token_weights(None, st)
        assert lib.ezdit_sampler_attach_controlnet(m._h, cn._h, 1.0) == 0
        assert lib.ezdit_set_context_token_weights(m._h, arr, 4, st) == -2 and b'ControlNet' in lib.ezdit_last_error()
        assert lib.ezdit_sampler_attach_controlnet(m._h, None, 1.0) == 0
        assert lib.ezdit_set_context_token_weights(m._h, arr, 4, st) == 0, lib.ezdit_last_error()
        smp.run(use_graph=True)
        assert torch.equal(smp.finish(), ref), 'off, refused, on again: the run from before'
    finally:
        assert lib.ezdit_sampler_attach_controlnet(m._h, None, 1.0) == 0
    from ezaudio_amd.sampler import LatentSampler
    with pytest.raises(ValueError, match='ControlNet'):
        LatentSampler(m, _scheduler()).prepare(text, mask, text, mask, torch.zeros(2, cfg['out_chans'], L), None, 3.0, 0.5, K, 0.0, token_weights=tw, controlnet=cn,
                                               condition=torch.zeros(1, 1, 2 * L))


# ---------------------------------------------------------------------------------------------------
# the public surface: EzAudio('mini', ...) with the mini VAE, a word tokenizer and a stand-in text encoder (the fixture of tests/test_start_gpu.py; helpers copied)
# ---------------------------------------------------------------------------------------------------
MINI_VAE = dict(channels=64, c_mults=[1, 2], strides=[2, 4], latent_dim=128, out_channels=1)


def _mini_autoencoder(device='cuda'):
    from ezaudio_amd.vae import Autoencoder
    from oracle import vae as V
    cfg = MINI_VAE
    sd = {k: torch.from_numpy(v) for k, v in V.make_vae_state_dict(cfg, 5).items()}
    sd.update({k: torch.from_numpy(v) for k, v in V.make_vae_state_dict(cfg, 5, encoder=True).items()})
    common = dict(channels=cfg['channels'], c_mults=cfg['c_mults'], strides=cfg['strides'], use_snake=True)
    config = {'model': {'encoder': {'type': 'oobleck', 'config': dict(in_channels=1, latent_dim=2 * cfg['latent_dim'], **common)},
                        'decoder': {'type': 'oobleck', 'config': dict(out_channels=1, latent_dim=cfg['latent_dim'], final_tanh=False, **common)},
                        'bottleneck': {'type': 'vae'}}}
    return Autoencoder(model_type='stable_vae', quantization_first=True, config=config, state_dict=sd, device=device)


class _WordTok:
    """one token per word, EOS behind; serves the batch call of inference() and the single-string call of emphasis_weights()"""

    def _ids(self, text, eos=True):
        return [2 + sum(map(ord, w)) % 120 for w in text.split()] + ([1] if eos else [])

    def __call__(self, texts, max_length=None, padding=None, truncation=None, return_tensors=None, add_special_tokens=True):
        if isinstance(texts, str):
            return type('Enc', (), dict(input_ids=self._ids(texts, add_special_tokens)))()
        rows = [self._ids(t)[:max_length] for t in texts]
        ids = torch.tensor([r + [0] * (max_length - len(r)) for r in rows], dtype=torch.long)
        return type('Batch', (), dict(input_ids=ids, attention_mask=(ids > 0).long()))()


class _Enc:
    def __init__(self, dim):
        self.dim = dim

    def __call__(self, input_ids, attention_mask):
        table = torch.randn(128, self.dim, generator=torch.Generator().manual_seed(7)).to(input_ids.device)
        return type('Out', (), dict(last_hidden_state=table[input_ids % 128]))()


@pytest.fixture(scope='module')
def ez(tmp_path_factory):
    import os
    import yaml
    import ezaudio_amd
    from ezaudio_amd import api as A
    from ezaudio_amd.config import load_yaml_with_includes
    tmp = tmp_path_factory.mktemp('emphasis')
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
        yield A.EzAudio('mini', autoencoder=_mini_autoencoder(), tokenizer=_WordTok(), text_encoder=_Enc(cfg['context_dim']), state_dict=sd)


def test_generate_audio_with_emphasis_is_inference_with_the_token_weights(ez):
    from ezaudio_amd.sampler import emphasis_weights, inference, parse_emphasis
    marked = '(x y:2) z'
    req = dict(length=2, ddim_steps=8, random_seed=3)
    sr, on = ez.generate_audio(marked, emphasis=True, **req)
    clean, spans = parse_emphasis(marked)
    max_len = ez.params['text_encoder']['max_length']
    W = torch.tensor([emphasis_weights(ez.tokenizer, clean, spans, max_len)])
    assert clean == 'x y z' and W[0, :4].tolist() == [2.0, 2.0, 1.0, 1.0]
    frames = 2 * ez.params['autoencoder']['latent_sr']
    direct = inference(ez.autoencoder, ez.unet, None, None, ez.tokenizer, ez.text_encoder, ez.params, ez.noise_scheduler, clean, None, frames, 5, 0.75, 8, 1, 3,
                       ez.device, token_weights=W)
    assert np.isfinite(on).all() and on.std() > 0
    assert np.array_equal(on, direct.cpu().numpy().squeeze(0).squeeze(0)), 'emphasis=True differs from inference(token_weights=)'
    sr, plain_clean = ez.generate_audio(clean, **req)
    assert not np.array_equal(on, plain_clean), 'the weights changed nothing'
    # emphasis=False (the default) leaves the prompt verbatim: today's call
    sr, off = ez.generate_audio(marked, emphasis=False, **req)
    sr, today = ez.generate_audio(marked, **req)
    verbatim = inference(ez.autoencoder, ez.unet, None, None, ez.tokenizer, ez.text_encoder, ez.params, ez.noise_scheduler, marked, None, frames, 5, 0.75, 8, 1, 3, ez.device)
    assert np.array_equal(off, today) and np.array_equal(off, verbatim.cpu().numpy().squeeze(0).squeeze(0))


def test_the_other_public_methods_pass_emphasis_on(ez):
    """audio_to_audio (single and batch), generate_long_audio and generate_loop with emphasis=True: the marked prompt gives what the clean prompt does not, and a group
    of weight 1 gives the clean prompt's bits (all weights 1: no table)."""
    from oracle.weights import uniform_pm1
    wav = (0.3 * uniform_pm1('emph_a', 1600, 9)).astype(np.float32)      # 200 latent frames of the mini VAE (ratio 8)
    calls = {
        'audio_to_audio': lambda text, **kw: ez.audio_to_audio(text, wav, strength=0.5, ddim_steps=8, random_seed=3, **kw)[1],
        'audio_to_audio batch': lambda text, **kw: ez.audio_to_audio([text, 'rain'], [wav, wav[:800]], strength=[0.5, 0.5], ddim_steps=8, random_seed=[3, 4], **kw)[1][0],
        'generate_long_audio': lambda text, **kw: ez.generate_long_audio(text, 3, window=2, overlap=0.5, ddim_steps=6, random_seed=3, **kw)[1],
        'generate_loop': lambda text, **kw: ez.generate_loop(text, 3, window=2, overlap=0.5, ddim_steps=6, random_seed=3, **kw)[1],
    }
    for name, f in calls.items():
        torch.manual_seed(21)
        clean = f('x y z')
        torch.manual_seed(21)
        on = f('(x y:2) z', emphasis=True)
        torch.manual_seed(21)
        unit = f('(x y:1) z', emphasis=True)
        assert np.isfinite(on).all() and on.shape == clean.shape, name
        assert not np.array_equal(on, clean), f'{name}: the weights changed nothing'
        assert np.array_equal(unit, clean), f'{name}: a group of weight 1 is the clean prompt'
