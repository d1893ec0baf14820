"""The prompt timeline through the public surface (run with -m gpu on an MI355X): ezdit_set_context_weights under MaskDiT.forward and under the fused sampler step.
What is checked here is exact: a timeline that weights ONE prompt at every frame is the plain call with that prompt alone, bit for bit, whichever place the prompt has
among the S of the context -- through the fused-projection cross-attention of ezdit_forward and, with classifier-free guidance, through the batch sub-range and the
single-key shortcut of the sampler step -- and the table obeys the contract of the run-time tables (off is the call that never set it, new values replay the captured step,
on <-> off captures again, the launch count does not change, a refused call changes nothing).  The kernel's arithmetic against fp64 is tests/test_attention_timeline_gpu.py's."""
import ctypes as C

import pytest
import torch

from oracle.weights import make_state_dict, model_config
from tests.test_start_gpu import _scheduler

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
L, LT, S = 96, 20, 3      # latent frames, tokens per prompt, prompts
_models = {}


def get_model(size):
    from ezaudio_amd import MaskDiT
    if size not in _models:
        cfg = model_config(size)
        m = MaskDiT(device=DEV, **cfg)
        m.load_state_dict(make_state_dict(cfg, 1))
        _models[size] = (m, cfg)
    return _models[size]


def _inputs(cfg, B, seed=0):
    g = torch.Generator().manual_seed(4200 + seed)
    x = torch.randn(B, cfg['out_chans'], L, generator=g)
    text = torch.randn(B, S, LT, cfg['context_dim'], generator=g)
    mask = torch.ones(B, S, LT, dtype=torch.bool)
    mask[:, 1, 12:] = False      # prompts of 20, 12 and 1 tokens
    mask[:, 2, 1:] = False
    return x, text, mask


def _hard(B, pick):
    """[B][S][L]: row b weights prompt pick[b] alone"""
    w = torch.zeros(B, S, L)
    for b, s in enumerate(pick):
        w[b, s] = 1.0
    return w


def _scene(B):
    """row b: a cross-fade 0 -> 1 over [30, 60), then a switch to prompt 2 at frame 80 (rolled by b prompts)"""
    i = torch.arange(L, dtype=torch.float32)
    a = ((i - 30) / 30).clamp(0, 1)
    w = torch.stack([(1 - a) * (i < 80), a * (i < 80), (i >= 80).float()])
    return torch.stack([torch.roll(w, b, 0) for b in range(B)])


@pytest.mark.parametrize('size', ['xs', 'xs64'])
def test_forward_with_one_prompt_weighted_is_the_plain_call_with_that_prompt(lib, size):
    from ezaudio_amd.sampler import timeline_context
    m, cfg = get_model(size)
    B = 2
    x, text, mask = _inputs(cfg, B)
    ctx3, msk3 = timeline_context(text, mask)
    before = m.last_launch_count
    for pick in ([0, 1], [1, 0], [1, 1]):      # (prompts with several keys: a single-key row takes the shortcut, whose constant is computed another way)
        ctx1 = torch.stack([timeline_context(text[b, s:s + 1], mask[b, s:s + 1])[0] for b, s in enumerate(pick)])
        msk1 = torch.stack([timeline_context(text[b, s:s + 1], mask[b, s:s + 1])[1] for b, s in enumerate(pick)])
        plain, _ = m.forward(x.to(DEV), torch.tensor([500, 20]), ctx1.to(DEV), context_mask=msk1.to(DEV))
        n_plain = m.last_launch_count
        one, _ = m.forward(x.to(DEV), torch.tensor([500, 20]), ctx1.to(DEV), context_mask=msk1.to(DEV), context_weights=torch.ones(B, 1, L))
        assert m.last_launch_count == n_plain, 'the table changes the launch count'
        again, _ = m.forward(x.to(DEV), torch.tensor([500, 20]), ctx1.to(DEV), context_mask=msk1.to(DEV))
        tl, _ = m.forward(x.to(DEV), torch.tensor([500, 20]), ctx3.to(DEV), context_mask=msk3.to(DEV), context_weights=_hard(B, pick))
        assert m.last_launch_count == n_plain
        torch.cuda.synchronize()
        assert torch.isfinite(plain).all()
        assert torch.equal(one, plain), 'S = 1 with weight 1 differs from the plain call'
        assert torch.equal(again, plain), 'off after on differs from the run before'
        assert torch.equal(tl, plain), f'prompts {pick} weighted alone differ from the plain calls with them'
    assert before is not None


@pytest.mark.parametrize('size', ['xs', 'xs64'])
def test_forward_with_a_scene_is_finite_and_differs_from_every_single_prompt(lib, size):
    """A cross-fade and a switch: no exact reference here (the kernel's arithmetic is checked against fp64 in tests/test_attention_timeline_gpu.py); the result is finite,
    and differs from each single-prompt result, as does a frame-constant mix."""
    from ezaudio_amd.sampler import timeline_context
    m, cfg = get_model(size)
    B = 2
    x, text, mask = _inputs(cfg, B, 1)
    ctx3, msk3 = timeline_context(text, mask)
    run = lambda w: m.forward(x.to(DEV), torch.tensor(300), ctx3.to(DEV), context_mask=msk3.to(DEV), context_weights=w)[0].float().cpu()      # noqa: E731
    singles = [run(_hard(B, [s] * B)) for s in range(S)]
    scene = run(_scene(B))
    mix = torch.zeros(B, S, L); mix[:, :2] = 0.5
    mixed = run(mix)
    assert torch.isfinite(scene).all() and torch.isfinite(mixed).all()
    d = lambda a, b: float((a - b).norm() / b.norm())      # noqa: E731
    assert all(d(scene, s_) > 1e-4 and d(mixed, s_) > 1e-4 for s_ in singles)


def _sampler(m, cfg, P, text, mask, weights, seed, solver='ddim', K=4):
    from ezaudio_amd.sampler import LatentSampler
    g = torch.Generator().manual_seed(seed)
    init = torch.randn(P, cfg['out_chans'], L, generator=g)
    un = torch.randn(1, LT, cfg['context_dim'], generator=torch.Generator().manual_seed(77)).expand(P, -1, -1).contiguous()
    um = torch.zeros(P, LT, dtype=torch.bool); um[:, 0] = True      # the encoding of '': one valid key
    smp = LatentSampler(m, _scheduler(K))
    kw = {} if weights is None else dict(context_weights=weights)
    if weights is None:      # the plain call: text [P][128][Cctx], the unconditional tokens padded to the same 128 under the mask
        from ezaudio_amd.sampler import timeline_context
        un, um = timeline_context(un[:, None], um[:, None])
    smp.prepare(text.to(DEV), mask.to(DEV), un.to(DEV), um.to(DEV), init.to(DEV), None, 3.0, 0.5, K, 0.0, solver=solver, **kw)
    return smp


@pytest.mark.parametrize('solver', ['ddim', 'dpmpp_2m'])
def test_sampler_loop_with_one_prompt_weighted_is_the_plain_loop_and_graph_is_eager_is_pieces(lib, solver):
    from ezaudio_amd.sampler import timeline_context
    m, cfg = get_model('xs')
    P, K = 2, 4
    _, text, mask = _inputs(cfg, P, 2)
    pick = [1, 0]
    t1 = torch.stack([text[b, s] for b, s in enumerate(pick)])      # [P][LT][Cctx]: the plain call's prompts ...
    m1 = torch.stack([mask[b, s] for b, s in enumerate(pick)])
    ctx1, msk1 = timeline_context(t1[:, None], m1[:, None])          # ... zero-padded to 128 under the mask
    plain = _sampler(m, cfg, P, ctx1, msk1, None, 5, solver, K)
    plain.run(use_graph=True)
    ref = plain.finish().clone()
    outs = {}
    for name, pieces, graph in (('graph', [K], True), ('eager', [K], False), ('pieces', [1, 2, 1], True)):
        smp = _sampler(m, cfg, P, text, mask, _hard(P, pick), 5, solver, K)
        for n in pieces:
            smp.run(n, use_graph=graph)
        outs[name] = smp.finish().clone()
    assert torch.isfinite(ref).all() and ctx1.shape[1] == 128 and bool(msk1.any())
    for name, o in outs.items():
        assert torch.equal(o, ref), f'{solver}, {name}: prompts {pick} weighted alone differ from the plain loop with them'
    scene = _sampler(m, cfg, P, text, mask, _scene(P), 5, solver, K)
    scene.run(use_graph=True)
    got = scene.finish()
    assert torch.isfinite(got).all() and not torch.equal(got, ref)


def test_new_weights_replay_the_graph_and_on_off_capture_again(lib, capfd):
    m, cfg = get_model('xs')
    P, K = 1, 6
    _, text, mask = _inputs(cfg, P, 3)
    smp = _sampler(m, cfg, P, text, mask, _scene(P), 6, 'ddim', K)
    st = C.c_void_p(smp.stream.cuda_stream)
    cfgw = lambda w: torch.cat([w, _hard(P, [0])], 0)      # noqa: E731  the CFG batch: the unconditional row weights prompt 0
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
            m.set_context_weights(cfgw(_hard(P, [2])), st)
        assert not captured(), 'new values into a table that is on keep the graph'
        with torch.cuda.stream(smp.stream):
            m.set_context_weights(None, st)
        assert captured(), 'off drops the graph'
        with torch.cuda.stream(smp.stream):
            m.set_context_weights(cfgw(_scene(P)), st)
        assert captured(), 'on drops the graph'
        assert torch.isfinite(smp.finish()).all()
    finally:
        assert lib.ezdit_set_option(m._h, b'trace_launches', 0) == 0


def test_refusals_change_nothing(lib):
    from ezaudio_amd import _lib
    from ezaudio_amd.sampler import timeline_context
    m, cfg = get_model('xs')
    B = 2
    x, text, mask = _inputs(cfg, B, 4)
    ctx3, msk3 = timeline_context(text, mask)
    good = _scene(B)
    ref, _ = m.forward(x.to(DEV), torch.tensor(300), ctx3.to(DEV), context_mask=msk3.to(DEV), context_weights=good)
    ref = ref.clone()

    def refused(w, code):
        arr = (C.c_float * w.numel())(*w.reshape(-1).tolist())
        assert lib.ezdit_set_context_weights(m._h, arr, int(w.shape[1]), None) == code, lib.ezdit_last_error()
        assert lib.ezdit_last_error()
    bad = good.clone(); bad[0, :, 17] = 0.0
    refused(bad, -1)                                   # a frame that weights nothing
    bad = good.clone(); bad[1, 2, 3] = -1.0
    refused(bad, -1)
    bad = good.clone(); bad[1, 0, 0] = float('inf')
    refused(bad, -1)
    refused(good[:, :2].contiguous(), -1)              # S 128 != Lc
    only2 = _hard(B, [2, 2]); msk_no2 = msk3.clone(); msk_no2[:, 256:] = False
    with pytest.raises(AssertionError, match='valid key'):      # the only weighted prompt has no valid key (EZDIT_E_INVALID)
        m.forward(x.to(DEV), torch.tensor(300), ctx3.to(DEV), context_mask=msk_no2.to(DEV), context_weights=only2)
    with pytest.raises(_lib.EzditError):               # lengths while the table is on
        m.prepare_context(ctx3.to(DEV), msk3.to(DEV)); m.set_context_weights(good); m.set_lengths([L, L - 7])
    m.set_context_weights(None)
    again, _ = m.forward(x.to(DEV), torch.tensor(300), ctx3.to(DEV), context_mask=msk3.to(DEV), context_weights=good)
    assert torch.equal(again, ref)


# ---------------------------------------------------------------------------------------------------
# against the numpy oracle with the timeline (tools/mint_timeline_golden.py)
# ---------------------------------------------------------------------------------------------------
REL_TOL, ABS_TOL, LOOP_GATE = 2e-2, 0.15, 2e-2      # tests/test_gpu.py


def _t(a):
    import numpy as np
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize('name', ['xs', 'xs64'])
def test_forward_with_a_scene_matches_the_oracle_with_the_timeline(lib, name):
    """A switch and a cross-fade through the whole network: rel-L2 <= 2e-2 against the oracle whose cross-attention carries the bias ln w.  The golden's own distance from
    each of the three single-prompt results is in its meta; the GPU's distance from the plain one-prompt golden is printed beside it."""
    import numpy as np
    from ezaudio_amd.sampler import timeline_context
    from tests.util import golden_case, load_golden, record, rel_l2
    cfg, sd, inp, kw, g0, meta = golden_case(name)
    g, tm = load_golden('forward_timeline_' + name)
    assert tm['base'] == 'dit_' + name and tm['L'] == L and tm['S'] == S and tm['LT'] == LT and meta['seed_w'] == 1 and not kw
    assert min(tm['scene_vs_single']) > 5 * REL_TOL, tm['scene_vs_single']      # the scene is far from every single prompt
    m, _ = get_model(meta['size'])
    ctx4 = _t(g['ctx'])
    ctx, msk = timeline_context(ctx4, torch.ones(ctx4.shape[:3], dtype=torch.bool))
    for t in meta['timesteps']:
        pred = m.forward(_t(inp['x']).to(DEV), torch.tensor(t), ctx.to(DEV), context_mask=msk.to(DEV), context_weights=_t(g['weights']))[0].cpu().numpy()
        ref = g[f'pred_t{t}']
        r, a = rel_l2(pred, ref), float(np.abs(pred - ref).max())
        record(f'forward_timeline_{name} t={t} scene {tm["scene"]}: rel-L2 {r:.3e} max-abs {a:.3e} vs the oracle with the timeline; {rel_l2(pred, g0[f"pred_t{t}"]):.3e} from the '
               f'one-prompt golden (the oracle is {min(tm["scene_vs_single"]):.3e} from its nearest single prompt)')
        assert np.isfinite(pred).all()
        assert r < REL_TOL and a < ABS_TOL * max(1.0, float(ref.std()) / 1.48), (name, t, r, a)


@pytest.mark.parametrize('radius', [None, 8])
def test_sampler_loop_with_a_scene_matches_the_oracle_loop(lib, radius):
    """The inputs of smp_xs_e0, 20 steps, DDIM and dpmpp_2m, the conditional row under the scene: <= 2e-2 against the oracle loop; again under attention_window radius 8."""
    from ezaudio_amd.sampler import LatentSampler
    from tests.util import load_golden, record, rel_l2, sampler_case
    cfg, sd, inp, init, noises, g1, meta = sampler_case('smp_xs_e0')
    g, tm = load_golden('sampler_timeline_xs')
    assert tm['base'] == 'smp_xs_e0' and tm['steps'] == meta['steps'] == 20 and tm['radius'] == 8 and meta['seed_w'] == 1
    m, _ = get_model('xs')
    ctx4 = _t(g['ctx'])
    gt, gm = _t(inp['gt'][0:1]).to(DEV), _t(inp['gt_mask'][0:1]).to(DEV)
    try:
        m.set_attention_window(radius)
        for solver in ('ddim', 'dpmpp_2m'):
            smp = LatentSampler(m, _scheduler(meta['steps']))
            smp.prepare(ctx4.to(DEV), torch.ones(ctx4.shape[:3], dtype=torch.bool, device=DEV), _t(inp['ctx'][1:2]).to(DEV), _t(inp['ctx_mask'][1:2]).to(DEV),
                        _t(init).to(DEV), None, meta['guidance_scale'], meta['guidance_rescale'], meta['steps'], 0.0, gt=gt, gt_mask=gm, solver=solver,
                        context_weights=_t(g['weights']))
            smp.run(use_graph=True)
            lat = smp.finish()
            fin = torch.where(gm, lat, gt).cpu().numpy()      # src/inference.py:104-105
            e = rel_l2(fin, g['latent_' + solver + ('' if radius is None else f'_r{radius}')])
            record(f'sampler_timeline_xs {solver} radius {radius}, {meta["steps"]} steps: final-latent rel-L2 vs the numpy oracle loop with the timeline {e:.3e}; '
                   f'{rel_l2(fin, g1["latent"]):.3e} from the one-prompt golden (oracle, DDIM, no window: {tm["scene_vs_plain_ddim"]:.3e})')
            assert torch.isfinite(lat).all() and e < LOOP_GATE, (solver, radius, e)
    finally:
        m.set_attention_window(None)


def _ragged_inputs(name):
    from tests.util import golden_case, load_golden
    cfg, sd, inp, kw, g0, meta = golden_case(name)
    g, tm = load_golden('forward_timeline_' + name)
    return cfg, _t(inp['x'])[0:1], _t(g['ctx'])[0:1], g, tm, meta['timesteps'][0]


def test_padded_batch_with_three_scenes_is_finite_everywhere_and_each_sample_is_its_single_call(lib):
    """[96, 80, 33] frames in one padded call, S = 3 for all, three different scenes.  Every output frame is finite and the frames beyond a length exactly 0 -- also after a
    SECOND block has read the padding rows of the first (a padding row that met no weighted key would be 0 / 0, and 0 * NaN = NaN in the next self-attention) -- and
    each sample is bitwise the call with it alone at its own length."""
    from ezaudio_amd.sampler import timeline_context
    from tests.util import record, rel_l2
    cfg, x0, ctx4, g, tm, t0 = _ragged_inputs('xs')
    m, _ = get_model('xs')
    lens = [96, 80, 33]
    ctx, msk = timeline_context(ctx4, torch.ones(ctx4.shape[:3], dtype=torch.bool))
    a, b, n = tm['scene']
    scenes = [_t(g['weights'])[0], torch.roll(_t(g['weights'])[0], 1, 0), _hard(1, [2])[0]]      # the golden's scene | the same with the prompts rolled | prompt 2 alone
    i = torch.arange(L)
    scenes[1] = torch.stack([(i >= 20).float(), (i < 20) * 0.5, (i < 20) * 0.5])                  # ... made to END on prompt 0 and begin on a mix of 1 and 2
    X = torch.full((3, x0.shape[1], L), float('nan'))
    W = torch.zeros(3, S, L)
    for p, ln in enumerate(lens):
        X[p, :, :ln] = x0[0, :, :ln]
        W[p, :, :ln] = scenes[p][:, :ln]
    out = m.forward(X.to(DEV), torch.tensor(t0), ctx.expand(3, -1, -1).to(DEV), context_mask=msk.expand(3, -1).to(DEV), x_lens=lens, context_weights=W)[0].cpu()
    assert torch.isfinite(out).all(), 'a padded batch under a timeline must stay finite'
    for p, ln in enumerate(lens):
        single = m.forward(x0[:, :, :ln].to(DEV), torch.tensor(t0), ctx.to(DEV), context_mask=msk.to(DEV), context_weights=scenes[p][None, :, :ln].contiguous())[0].cpu()
        e = rel_l2(out[p, :, :ln].numpy(), single[0].numpy())
        record(f'timeline ragged batch {lens}: sample {p} (L {ln}) vs its single call: rel-L2 {e:.3e}')
        assert bool((out[p, :, ln:] == 0).all()), p
        assert torch.equal(out[p, :, :ln], single[0]), (p, e)
    m.set_lengths(None)


def test_padded_batch_with_three_two_and_one_prompts_matches_each_samples_golden(lib):
    """S_i = (3, 1, 2) in one padded call of [96, 80, 33] frames (missing prompts: weight 0 and an all-masked context): each sample within 2e-2 of the oracle run of it
    alone at its own length; the distance to the GPU's own single call is printed."""
    import numpy as np
    from ezaudio_amd.sampler import timeline_context
    from tests.util import record, rel_l2
    cfg, x0, ctx4, g, tm, t0 = _ragged_inputs('xs')
    m, _ = get_model('xs')
    assert [tuple(r) for r in tm['ragged']] == [(96, 3), (80, 1), (33, 2)]
    lens, sps = [96, 80, 33], [3, 1, 2]
    c4 = ctx4.expand(3, -1, -1, -1).clone()
    m4 = torch.zeros(3, S, LT, dtype=torch.bool)
    X = torch.zeros(3, x0.shape[1], L)
    W = torch.zeros(3, S, L)
    for p, (ln, sp) in enumerate(zip(lens, sps)):
        m4[p, :sp] = True
        c4[p, sp:] = 0
        X[p, :, :ln] = x0[0, :, :ln]
        W[p, :sp, :ln] = _t(g[f'ragged_w{p}'])
    ctx, msk = timeline_context(c4, m4)
    out = m.forward(X.to(DEV), torch.tensor(t0), ctx.to(DEV), context_mask=msk.to(DEV), x_lens=lens, context_weights=W)[0].cpu()
    assert torch.isfinite(out).all()
    for p, (ln, sp) in enumerate(zip(lens, sps)):
        c1, k1 = timeline_context(ctx4[:, :sp], torch.ones(1, sp, LT, dtype=torch.bool))
        single = m.forward(x0[:, :, :ln].to(DEV), torch.tensor(t0), c1.to(DEV), context_mask=k1.to(DEV), context_weights=_t(g[f'ragged_w{p}'])[None])[0].cpu()
        ref = g[f'ragged_p{p}'][0]
        r, a = rel_l2(out[p, :, :ln].numpy(), ref), float(np.abs(out[p, :, :ln].numpy() - ref).max())
        record(f'timeline ragged batch S_i {sps}: sample {p} (L {ln}, {sp} prompts): rel-L2 {r:.3e} max-abs {a:.3e} vs its oracle golden; '
               f'{rel_l2(out[p, :, :ln].numpy(), single[0].numpy()):.3e} from its single call')
        assert r < REL_TOL and bool((out[p, :, ln:] == 0).all()), (p, r)
    m.set_lengths(None)


def test_refusals_with_a_controlnet_a_canvas_and_a_stream_capture(lib):
    """ControlNet: the attach with the table on, the setter with one attached, the setter on a ControlNet handle.  The canvas and ring setters against the table, in both
    orders.  The setter inside a stream capture.  Every refusal leaves the run that follows bitwise what it was."""
    from ezaudio_amd import DiTControlNet
    from ezaudio_amd.sampler import timeline_context
    from oracle.controlnet import CN_DEFAULT
    m, cfg = get_model('xs')
    P, K = 2, 3
    _, text, mask = _inputs(cfg, P, 5)
    w = torch.cat([_scene(P), _hard(P, [0, 0])], 0)      # the CFG batch's table
    arr = lambda t: (C.c_float * t.numel())(*t.reshape(-1).tolist())      # noqa: E731
    ref = _sampler(m, cfg, P, text, mask, _scene(P), 9, 'ddim', K)
    ref.run(use_graph=True)
    ref = ref.finish().clone()
    smp = _sampler(m, cfg, P, text, mask, _scene(P), 9, 'ddim', K)
    st = C.c_void_p(smp.stream.cuda_stream)
    ccfg = dict(cfg)
    ccfg.update(CN_DEFAULT)
    cn = DiTControlNet(device=DEV, **ccfg)
    offs = (C.c_int32 * P)(0, 48)
    try:
        # the table is on (prepare set it)
        assert lib.ezdit_sampler_attach_controlnet(m._h, cn._h, 1.0) == -2 and b'context weights' in lib.ezdit_last_error()
        assert lib.ezdit_set_context_weights(cn._h, arr(w), S, st) == -2 and b'ControlNet' in lib.ezdit_last_error()
        assert lib.ezdit_sampler_set_canvas(m._h, offs, P, 144, 1, st) == -2 and b'context weights' in lib.ezdit_last_error()
        assert lib.ezdit_sampler_set_canvas_loop(m._h, offs, P, 120, 1, st) == -2 and b'context weights' in lib.ezdit_last_error()

        def in_capture():
            x = torch.zeros(8, device=DEV)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=smp.stream):
                x.add_(1.0)
                rc = lib.ezdit_set_context_weights(m._h, arr(_hard(2 * P, [1, 1, 0, 0])), S, st)
            return rc
        assert in_capture() == -3 and b'capture' in lib.ezdit_last_error()
        smp.run(use_graph=True)
        assert torch.equal(smp.finish(), ref), 'a refused call changed the run'
        # the other order: table off, then a ControlNet attached / a canvas on refuse the table
        smp = _sampler(m, cfg, P, text, mask, _scene(P), 9, 'ddim', K)
        st = C.c_void_p(smp.stream.cuda_stream)
        with torch.cuda.stream(smp.stream):
            m.set_context_weights(None, st)
        assert lib.ezdit_sampler_attach_controlnet(m._h, cn._h, 1.0) == 0
        assert lib.ezdit_set_context_weights(m._h, arr(w), S, st) == -2 and b'ControlNet' in lib.ezdit_last_error()
        assert lib.ezdit_sampler_attach_controlnet(m._h, None, 1.0) == 0
        for setter, T in ((lib.ezdit_sampler_set_canvas, 144), (lib.ezdit_sampler_set_canvas_loop, 120)):
            assert setter(m._h, offs, P, T, 1, st) == 0, lib.ezdit_last_error()
            assert lib.ezdit_set_context_weights(m._h, arr(w), S, st) == -2 and b'canvas' in lib.ezdit_last_error()
            assert setter(m._h, None, 0, 0, 1, st) == 0
        assert lib.ezdit_set_context_weights(m._h, arr(w), S, st) == 0, lib.ezdit_last_error()
        smp.run(use_graph=True)
        assert torch.equal(smp.finish(), ref), 'off, refused, on again: the run from before'
    finally:
        assert lib.ezdit_sampler_attach_controlnet(m._h, None, 1.0) == 0
