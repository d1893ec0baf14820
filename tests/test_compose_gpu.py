"""GPU tests of composed guidance: K weighted prompts per sample in the fused sampler step (ezdit_cfg_compose_step, ezdit_sampler_begin_composed,
ezdit_sampler_set_compose_weights, LatentSampler.prepare(compose_text=, compose_mask=, compose_weights=)).

The reference has no composed guidance.  The judges are the definition in float64 (tests/compose_emul.py; the gate is 4 x the floor that the fp32 emulation
of the kernels' order keeps from it, measured on the CPU by tests/test_compose_host.py, and the checking code is the one that test feeds its eight deliberate
mistakes to), the numpy oracle's loop with that definition (tests/golden/sampler_compose_xs.npz, tools/mint_compose_golden.py) and, bit for bit, the plain
operator and the plain call where composition reduces to them.  xs width throughout.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import compose_emul as E
from tests.test_sample_params_gpu import get_model, t_
from tests.util import DIFF, load_golden, record, rel_l2, sampler_case

pytestmark = pytest.mark.gpu

N_OP = E.C_OP * E.L_OP


def _scheduler(steps):
    from ezaudio_amd.scheduler import DDIMScheduler
    sch = DDIMScheduler(**DIFF)
    sch.set_timesteps(steps)
    return sch


@pytest.fixture(autouse=True)
def _leave_the_shared_model_plain(lib):
    """The xs model is shared with the other test modules: no test here leaves composition, lengths or a ControlNet on its handle."""
    yield
    m = get_model('xs', 1)
    if m._ws_key is not None:
        assert lib.ezdit_sampler_set_compose_weights(m._h, None, 0, 0, None) in (0, -3)
        m._compose_on = False
        m.set_lengths(None)


# ---------------------------------------------------------------------------------------------------
# 1. - 4. kernel level: ezdit_cfg_compose_step
# ---------------------------------------------------------------------------------------------------
def _run_operator(lib, case):
    """One call on copies of the case's arrays; returns (latents, x0_hist or None) as numpy."""
    P, K = case['weights'].shape
    L = E.L_OP
    pd, ld, pr, wd = t_(case['pred']), t_(case['lat']), t_(case['params']), t_(case['weights'])
    hd = t_(case['hist']) if case['hist'] is not None else None
    nd = t_(case['noise']) if case['noise'] is not None else None
    scratch = torch.zeros(P * 256, device='cuda:0')
    kl = torch.tensor(case['lens'], dtype=torch.int32, device='cuda:0') if case['lens'] != [L] * P else None
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    rc = lib.ezdit_cfg_compose_step(pd.data_ptr(), ld.data_ptr(), ptr(nd), ptr(hd), pr.data_ptr(), wd.data_ptr(), K, ptr(kl), L, P, N_OP,
                                    scratch.data_ptr(), None)
    assert rc == 0, lib.ezdit_last_error()
    torch.cuda.synchronize()
    return ld.cpu().numpy(), None if hd is None else hd.cpu().numpy()


@pytest.mark.parametrize('K,lens,ms,P', [c + (3,) for c in E.OPERATOR_CASES] + list(E.K8_CASES))
def test_compose_step_operator_against_fp64_and_reads_nothing_it_must_not(lib, K, lens, ms, P):
    """n = 128 x 150 = 19200 (a second, partial trip of the grid-stride loop), step 7 of 50.  P = 3: guidance 5 with rescale 0.75, guidance 2 without
    rescale and a weight of 0 in its second slot, no guidance (g = 0); lengths None and (131, 77, 1); the DDIM form with noise (one sample at sigma 0) and the
    multistep form (one sample at c_hist 0).  K = 8 at P = 1 fills every weight register, two of them with 0.
    The call runs on the POISONED inputs -- NaN in the rows of weight 0, the padded frames of every input, the noise slice of the sigma = 0 sample, the history
    of the c_hist = 0 sample, every row but c_0 of the sample without guidance -- and must come out finite, within 4 floors of float64 per sample on latents and
    x0_hist (E.check_outputs), exactly 0 on padded frames, and bit for bit what the clean inputs give."""
    case = E.operator_case(K, lens, ms, P)
    got, hgot = _run_operator(lib, E.poisoned(case))
    floor = E.operator_floor()
    dists = E.check_outputs(got, hgot, case)
    for (name, p), e in sorted(dists.items()):
        record(f'compose step operator K={K} P={P} lens={lens} {"multistep" if ms else "ddim"} {name} sample {p}: rel-L2 vs fp64 {e:.3e} '
               f'= {e / floor:.2f} floors (floor {floor:.3e}, gate {E.GATE_FLOORS} floors)')
    clean, hclean = _run_operator(lib, case)
    assert np.array_equal(clean, got)
    assert hgot is None or np.array_equal(hclean, hgot)


@pytest.mark.parametrize('lens', E.LENS_OP)
def test_one_condition_with_weight_1_is_bitwise_the_plain_operators(lib, lens):
    P, L = 3, E.L_OP
    for ms in (False, True):
        case = dict(E.operator_case(1, lens, ms), weights=np.ones((P, 1), np.float32))
        got, hgot = _run_operator(lib, case)
        pd, ld, pr = t_(case['pred']), t_(case['lat']), t_(case['params'])
        scratch = torch.zeros(P * 256, device='cuda:0')
        kl = torch.tensor(case['lens'], dtype=torch.int32, device='cuda:0') if lens else None
        klp = kl.data_ptr() if lens else None
        if ms:
            hd = t_(case['hist'])
            assert lib.ezdit_cfg_multistep_step(pd.data_ptr(), ld.data_ptr(), hd.data_ptr(), pr.data_ptr(), klp, L, P, N_OP, scratch.data_ptr(), None) == 0
        else:
            nd = t_(case['noise'])
            assert lib.ezdit_cfg_ddim_step_per_sample(pd.data_ptr(), ld.data_ptr(), nd.data_ptr(), pr.data_ptr(), klp, L, P, N_OP, scratch.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert np.isfinite(got).all() and np.array_equal(ld.cpu().numpy(), got), ms
        if ms:
            assert np.array_equal(hd.cpu().numpy(), hgot)


def test_compose_step_operator_refusals(lib):
    case = E.operator_case(2, None, True)
    P, L = 3, E.L_OP
    pd, ld, hd, pr, wd = (t_(case[k]) for k in ('pred', 'lat', 'hist', 'params', 'weights'))
    scratch = torch.zeros(P * 256, device='cuda:0')
    before = ld.clone()
    args = [pd.data_ptr(), ld.data_ptr(), None, hd.data_ptr(), pr.data_ptr(), wd.data_ptr(), 2, None, L, P, N_OP, scratch.data_ptr(), None]
    for i in (0, 1, 4, 5, 11):                                         # a null pointer of each required kind
        assert lib.ezdit_cfg_compose_step(*(args[:i] + [None] + args[i + 1:])) == -1, i
    for i, v in ((6, 0), (6, 9), (9, 0), (10, 1), (2, pd.data_ptr())):  # K out of range, P, n, noise together with a history
        assert lib.ezdit_cfg_compose_step(*(args[:i] + [v] + args[i + 1:])) == -1, (i, v)
    kl = torch.tensor([150, 77, 1], dtype=torch.int32, device='cuda:0')
    assert lib.ezdit_cfg_compose_step(*(args[:7] + [kl.data_ptr(), 7] + args[9:])) == -1      # L does not divide n
    torch.cuda.synchronize()
    assert torch.equal(ld, before)                                     # nothing was launched


# ---------------------------------------------------------------------------------------------------
# 5. the fused loop
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case():
    cfg, sd, inp, init, noises, g, meta = sampler_case('smp_xs_e0')
    assert (meta['size'], meta['seed_w'], meta['steps'], meta['eta'], meta['with_gt']) == ('xs', 1, 20, 0.0, True)
    ctx2, msk2 = E.second_context(cfg, meta['Lc'], meta['seed_in'])
    return inp, init, meta, ctx2, msk2


def _prepare(solver='ddim', weights=None, P=1, with_gt=True, pad_to=None, **kw):
    """The fixture's sample P times; weights [P][K] (None: the plain call) with the second context as every extra condition."""
    from ezaudio_amd.sampler import LatentSampler
    inp, init, meta, ctx2, msk2 = _case()
    m = get_model('xs', 1)
    smp = LatentSampler(m, _scheduler(meta['steps']))

    def ctx(a, mask):
        a, mask = t_(a), t_(mask)
        if pad_to:                                                      # (a context of pad_to tokens, the added ones masked)
            a = torch.nn.functional.pad(a, (0, 0, 0, pad_to - a.shape[1]))
            mask = torch.nn.functional.pad(mask, (0, pad_to - mask.shape[1]))
        return a.repeat(P, 1, 1), mask.repeat(P, 1)
    text, tm = ctx(inp['ctx'][0:1], inp['ctx_mask'][0:1])
    un, um = ctx(inp['ctx'][1:2], inp['ctx_mask'][1:2])
    if weights is not None:
        K = len(weights[0])
        c2, m2 = ctx(ctx2, msk2)
        kw.update(compose_weights=weights, compose_text=c2[:, None].repeat(1, K - 1, 1, 1), compose_mask=m2[:, None].repeat(1, K - 1, 1))
    gt = t_(inp['gt'][0:1]) if with_gt else None
    gm = t_(inp['gt_mask'][0:1]) if with_gt else None
    smp.prepare(text, tm, un, um, t_(init).repeat(P, 1, 1), None, kw.pop('guidance_scale', meta['guidance_scale']), meta['guidance_rescale'], meta['steps'],
                0.0, gt=gt, gt_mask=gm, solver=solver, **kw)
    return smp


def _finish(smp, n=None, use_graph=True):
    smp.run(n, use_graph=use_graph)
    lat = smp.finish().clone()
    torch.cuda.synchronize()
    return lat


def _rewind(lib, smp):
    init = _case()[1]
    with torch.cuda.stream(smp.stream):
        smp.latents.copy_(t_(init).expand_as(smp.latents))
        return lib.ezdit_set_step(smp.unet._h, 0, C.c_void_p(smp.stream.cuda_stream))


@functools.lru_cache(maxsize=None)
def _golden_weights():
    g, gmeta = load_golden('sampler_compose_xs')
    assert gmeta['base'] == 'smp_xs_e0' and gmeta['K'] == 2 and gmeta['steps'] == _case()[2]['steps']
    return g, [[float(v) for v in gmeta['weights']]]


@functools.lru_cache(maxsize=None)
def _runs():
    """The composed DDIM and 2M runs of the golden's weights and the plain DDIM run, P = 1, graph replay: computed once, shared, never modified."""
    w = _golden_weights()[1]
    return _finish(_prepare('ddim', w)), _finish(_prepare('dpmpp_2m', w)), _finish(_prepare('ddim'))


def test_fused_composed_loop_against_the_numpy_oracle_graph_and_eager(lib):
    """Gate: the project's loop gate 2e-2 (tests/test_gpu.py::test_sampler_matches_reference_loop_golden) for DDIM and dpmpp_2m, graph replay and eager
    launches; the goldens lie 13 gates from plain CFG, and so must the runs."""
    inp, init, meta, _, _ = _case()
    g, w = _golden_weights()
    ddim, ms, plain = _runs()
    gt, gm = t_(inp['gt'][0:1]), t_(inp['gt_mask'][0:1])
    fin = lambda lat: torch.where(gm, lat, gt).cpu().numpy()   # noqa: E731  src/inference.py:104-105
    for solver, run, key in (('ddim', ddim, 'latent_ddim'), ('dpmpp_2m', ms, 'latent_2m')):
        eager = _finish(_prepare(solver, w), use_graph=False)
        for how, lat in (('graph', run), ('eager', eager)):
            e = rel_l2(fin(lat), g[key])
            record(f'sampler_compose_xs ({solver}, {how}, K = 2, weights {w[0]}): final-latent rel-L2 vs the numpy oracle loop {e:.3e}')
            assert torch.isfinite(lat).all() and e < 2e-2, (solver, how, e)
        assert torch.equal(eager, run), solver
    d = rel_l2(fin(ddim), fin(plain))
    record(f'sampler_compose_xs: composed vs plain run {d:.3e}')
    assert d > 10 * 2e-2 - 2 * 2e-2, d                                  # (the golden's 13 gates less the two runs' own gates)


def test_compose_reduced_to_one_prompt_is_bitwise_the_plain_call(lib):
    from ezaudio_amd import _lib
    inp, init, meta, _, _ = _case()
    _, _, plain = _runs()
    # through prepare(): one condition with weight 1 calls nothing new
    smp = _prepare('ddim', [[1.0]])
    assert smp.compose_K is None and torch.equal(_finish(smp), plain)
    # through the library: the composed kernels themselves with K = 1, w = 1, on the same binding (B = 2 = (1 + 1) P)
    steps = meta['steps']
    arr = (_lib.EzditDdimCoef * steps)(*[_lib.EzditDdimCoef(*c) for c in _scheduler(steps).ddim_coefficients(0.0)])
    with torch.cuda.stream(smp.stream):
        smp.latents.copy_(t_(init))
        rc = lib.ezdit_sampler_begin_composed(smp.unet._h, smp.latents.data_ptr(), 1, None, arr, steps, float(meta['guidance_scale']),
                                              float(meta['guidance_rescale']), smp.gt.data_ptr(), smp.gt_mask.data_ptr(), 1, (C.c_float * 1)(1.0),
                                              C.c_void_p(smp.stream.cuda_stream))
    assert rc == 0, lib.ezdit_last_error()
    assert torch.equal(_finish(smp), plain)
    # ... and K = 1 switched off goes on as the plain call
    assert lib.ezdit_sampler_set_compose_weights(smp.unet._h, None, 0, 0, C.c_void_p(smp.stream.cuda_stream)) == 0
    assert _rewind(lib, smp) == 0
    assert torch.equal(_finish(smp), plain)
    # a second prompt at weight 0 is the plain result as well: its row is computed and not read (another batch shape runs other kernel forms: the gate of
    # "each sample as the call with it alone", 2e-2; measured 0 on MI355X)
    zero = _finish(_prepare('ddim', [[1.0, 0.0]]))
    e = rel_l2(zero.cpu().numpy(), plain.cpu().numpy())
    record(f'composed with the second weight 0 vs the plain call: {e:.3e}')
    assert e < 2e-2


# ---------------------------------------------------------------------------------------------------
# 6. one batched call: P = 3, K = 2, lengths (96, 77, 50)
# ---------------------------------------------------------------------------------------------------
STEPS_B, GS_B, GR_B = 20, 3.5, 0.75
W_B = {96: (1.0, 0.5), 77: (1.0, 0.0), 50: (1.0, -0.5)}               # the sample of 77 frames has its second slot at weight 0


@functools.lru_cache(maxsize=None)
def _request(L):
    """One request at its OWN length: (text, negative text) contexts, a second condition, the initial latent."""
    from oracle.weights import make_inputs, model_config, uniform_pm1
    cfg = model_config('xs')
    inp = make_inputs(cfg, B=2, L=L, Lc=20, n_valid=(7, 1), seed=300 + L)
    ctx2, msk2 = E.second_context(cfg, 20, 300 + L)
    init = (uniform_pm1('cmp.init', cfg['out_chans'] * L, 300 + L) * np.float32(np.sqrt(3.0))).reshape(1, cfg['out_chans'], L)
    return dict(ctx=inp['ctx'], mask=inp['ctx_mask'], ctx2=ctx2, mask2=msk2, init=init, L=L)


@functools.lru_cache(maxsize=None)
def _judge(L):
    """The numpy oracle's loop with the float64 combination on the request alone, at its own length."""
    from oracle.dit import DiTOracle
    from oracle.weights import make_state_dict, model_config
    cfg = model_config('xs')
    o = DiTOracle(cfg, make_state_dict(cfg, 1))
    r, sch = _request(L), _scheduler(STEPS_B)
    return E.oracle_loop(lambda x, t, c, m, gt, gm: o.forward(x, t, c, m)[0], [r['ctx'][0:1], r['ctx2']], [r['mask'][0:1], r['mask2']], r['ctx'][1:2],
                         r['mask'][1:2], r['init'], sch.ddim_coefficients(0.0), [0.0] * STEPS_B, [int(t) for t in sch.timesteps], GS_B, GR_B, W_B[L])


def _batched(lengths):
    from ezaudio_amd.sampler import LatentSampler
    rows = [_request(L) for L in lengths]
    Lmax = max(lengths)
    init = np.full((len(rows), 128, Lmax), np.nan, np.float32)          # (padded frames of the init noise hold NaN: they are not read)
    for i, r in enumerate(rows):
        init[i, :, :r['L']] = r['init'][0]
    cat = lambda k, sl: t_(np.concatenate([r[k][sl] for r in rows], 0))   # noqa: E731
    smp = LatentSampler(get_model('xs', 1), _scheduler(STEPS_B))
    smp.prepare(cat('ctx', slice(0, 1)), cat('mask', slice(0, 1)), cat('ctx', slice(1, 2)), cat('mask', slice(1, 2)), t_(init), None, GS_B, GR_B, STEPS_B, 0.0,
                lengths=list(lengths), compose_text=cat('ctx2', slice(0, 1))[:, None], compose_mask=cat('mask2', slice(0, 1))[:, None],
                compose_weights=[W_B[L] for L in lengths])
    return _finish(smp)


def test_one_batched_composed_call_with_lengths_each_sample_against_the_oracle_alone(lib):
    lengths = (96, 77, 50)
    lat = _batched(lengths)
    assert torch.isfinite(lat).all()
    for i, L in enumerate(lengths):
        e = rel_l2(lat[i, :, :L].cpu().numpy(), _judge(L)[0])
        record(f'composed batch P = 3, K = 2, lengths {lengths}, sample {i} (weights {W_B[L]}): final-latent rel-L2 vs the oracle alone {e:.3e}')
        assert e < 2e-2, (i, e)
        assert not lat[i, :, L:].any(), 'padded latent frames must be exactly 0'
    # two samples with equal inputs come out bit for bit equal, wherever they sit in the batch
    two = _batched((77, 96, 77))
    assert torch.isfinite(two).all() and torch.equal(two[0], two[2])
    e = rel_l2(two[1].cpu().numpy(), lat[0].cpu().numpy())
    assert e < 2e-2, e


# ---------------------------------------------------------------------------------------------------
# 7. the captured step reads the weights at run time
# ---------------------------------------------------------------------------------------------------
def test_a_captured_step_reads_the_compose_weights_at_run_time(lib):
    """The SAME captured graph replayed after ezdit_sampler_set_compose_weights with other values equals, bit for bit, a fresh call with those values -- and
    differs from the run before."""
    first, _, _ = _runs()
    smp = _prepare('ddim', _golden_weights()[1])
    assert torch.equal(_finish(smp), first)
    other = [[1.5, -0.7]]
    smp.set_compose_weights(other)
    assert _rewind(lib, smp) == 0
    second = _finish(smp)
    assert torch.isfinite(second).all() and not torch.equal(second, first)
    assert torch.equal(second, _finish(_prepare('ddim', other)))


# ---------------------------------------------------------------------------------------------------
# 8. with a start table
# ---------------------------------------------------------------------------------------------------
def test_composed_call_with_a_start_table_holds_the_held_sample(lib):
    """P = 2 from a clean latent, start steps (0, 6): while the run is below step 6 the second sample's latents keep their bits; afterwards it moves.  Both
    samples as the same call without composition would start them (ezdit_add_noise is not touched by composition)."""
    inp, init, meta, _, _ = _case()
    clean = t_(inp['gt'][0:1]) * 0.5
    w = [[1.0, 0.5], [1.0, -0.5]]
    for solver in ('ddim', 'dpmpp_2m'):
        smp = _prepare(solver, w, P=2, with_gt=False, init_latents=clean, start_steps=[0, 6])
        smp.stream.synchronize()
        begun = smp.latents.clone()
        assert smp.first_step == 0
        held = _finish(smp, n=6)
        assert torch.equal(held[1], begun[1]) and not torch.equal(held[0], begun[0]), solver
        done = _finish(smp, n=meta['steps'] - 6)
        assert torch.isfinite(done).all() and not torch.equal(done[1], begun[1]), solver


def test_composed_call_with_per_sample_guidance(lib):
    """P = 2, K = 2 with guidance_scale (3.5, None) through the sample table: sample 0 is the composed call with it alone; sample 1 has no guidance, reads its
    primary condition alone and is the unguided plain call.  Other batch shapes run other kernel forms, so the gate is the 2e-2 of "each sample as the call
    with it alone" (tests/test_sample_params_gpu.py); measured 0 for both on MI355X."""
    meta = _case()[2]
    w0 = _golden_weights()[1][0]
    both = _finish(_prepare('ddim', [w0, [1.0, -0.5]], P=2, guidance_scale=[meta['guidance_scale'], None]))
    assert torch.isfinite(both).all()
    alone = (_runs()[0], _finish(_prepare('ddim', None, guidance_scale=None)))
    for i in range(2):
        e = rel_l2(both[i].cpu().numpy(), alone[i][0].cpu().numpy())
        record(f'composed P = 2 with guidance ({meta["guidance_scale"]}, None), sample {i}: rel-L2 vs the call with it alone {e:.3e}')
        assert e < 2e-2, (i, e)
    assert rel_l2(both[1].cpu().numpy(), both[0].cpu().numpy()) > 2e-2       # (two different samples)


# ---------------------------------------------------------------------------------------------------
# 9. refusals
# ---------------------------------------------------------------------------------------------------
_cns = []


def _controlnet():
    """A ControlNet handle of this module's own (the pair of tests/test_controlnet_batch_gpu.py is not touched)."""
    if not _cns:
        from ezaudio_amd import DiTControlNet
        from oracle.controlnet import CN_DEFAULT, make_controlnet_state_dict
        from oracle.weights import model_config
        cfg = model_config('xs')
        ccfg = dict(cfg)
        ccfg.update(CN_DEFAULT)
        cn = DiTControlNet(device='cuda:0', **ccfg)
        cn.load_state_dict(make_controlnet_state_dict(cfg, CN_DEFAULT, 1))
        _cns.append(cn)
    return _cns[0]


def _begin_composed(lib, smp, P, K, w, gs=None, plain=False):
    from ezaudio_amd import _lib
    meta = _case()[2]
    steps = meta['steps']
    arr = (_lib.EzditDdimCoef * steps)(*[_lib.EzditDdimCoef(*c) for c in _scheduler(steps).ddim_coefficients(0.0)])
    gs = float(meta['guidance_scale']) if gs is None else gs
    st = C.c_void_p(smp.stream.cuda_stream)
    with torch.cuda.stream(smp.stream):
        if plain:
            return lib.ezdit_sampler_begin(smp.unet._h, smp.latents.data_ptr(), P, None, arr, steps, gs, float(meta['guidance_rescale']), None, None, st)
        wa = None if w is None else (C.c_float * len(w))(*w)
        return lib.ezdit_sampler_begin_composed(smp.unet._h, smp.latents.data_ptr(), P, None, arr, steps, gs, float(meta['guidance_rescale']), None, None,
                                                K, wa, st)


def test_composed_refusals_leave_the_call_as_it_was(lib):
    """Every refusal with its code; none launches anything or changes the call: the run behind them is bit for bit the run before."""
    m = get_model('xs', 1)
    h = m._h
    w = [[1.0, 0.5]]
    smp = _prepare('ddim', w, with_gt=False)
    st = C.c_void_p(smp.stream.cuda_stream)
    first = _finish(smp)
    launches = lib.ezdit_last_launch_count(h)
    nan, inf = float('nan'), float('inf')
    fl = lambda v: (C.c_float * len(v))(*v)   # noqa: E731
    i32 = lambda v: (C.c_int32 * len(v))(*v)   # noqa: E731
    L = smp.latents.shape[2]
    ones = torch.ones(3, 1, L)
    wptr = C.cast(C.c_void_p(ones.data_ptr()), C.POINTER(C.c_float))
    cn = _controlnet()
    INVALID, UNSUPPORTED, STATE = -1, -2, -3
    for what, call, rc in (
            ('K = 0', lambda: _begin_composed(lib, smp, 1, 0, [1.0]), INVALID),
            ('K = 9', lambda: _begin_composed(lib, smp, 1, 9, [1.0] * 9), INVALID),
            ('K = 3 does not fit B = 3', lambda: _begin_composed(lib, smp, 1, 3, [1.0] * 3), INVALID),
            ('P = 2 does not fit B = 3', lambda: _begin_composed(lib, smp, 2, 2, [1.0] * 4), INVALID),
            ('NaN weight', lambda: _begin_composed(lib, smp, 1, 2, [1.0, nan]), INVALID),
            ('infinite weight', lambda: _begin_composed(lib, smp, 1, 2, [inf, 1.0]), INVALID),
            ('w_0 = 0', lambda: _begin_composed(lib, smp, 1, 2, [0.0, 1.0]), INVALID),
            ('w_0 < 0', lambda: _begin_composed(lib, smp, 1, 2, [-1.0, 1.0]), INVALID),
            ('no guidance', lambda: _begin_composed(lib, smp, 1, 2, [1.0, 0.5], gs=0.0), INVALID),
            ('null weights', lambda: _begin_composed(lib, smp, 1, 2, None), INVALID),
            ('setter: other P', lambda: lib.ezdit_sampler_set_compose_weights(h, fl([1.0] * 4), 2, 2, st), INVALID),
            ('setter: other K', lambda: lib.ezdit_sampler_set_compose_weights(h, fl([1.0] * 3), 1, 3, st), INVALID),
            ('setter: NaN', lambda: lib.ezdit_sampler_set_compose_weights(h, fl([1.0, nan]), 1, 2, st), INVALID),
            ('setter: w_0 = 0', lambda: lib.ezdit_sampler_set_compose_weights(h, fl([0.0, 1.0]), 1, 2, st), INVALID),
            ('a ControlNet while composed', lambda: lib.ezdit_sampler_attach_controlnet(h, cn._h, 1.0), UNSUPPORTED),
            ('a canvas while composed', lambda: lib.ezdit_sampler_set_canvas(h, i32([0]), 1, L, 1, st), UNSUPPORTED),
            ('a ring while composed', lambda: lib.ezdit_sampler_set_canvas_loop(h, i32([0]), 1, L, 1, st), UNSUPPORTED),
            ('context weights while composed', lambda: lib.ezdit_set_context_weights(h, wptr, 1, st), UNSUPPORTED)):
        assert call() == rc, what
        assert lib.ezdit_last_error(), what
        assert lib.ezdit_last_launch_count(h) == launches, what
        assert _rewind(lib, smp) == 0
        assert torch.equal(_finish(smp), first), what
    # the other way round: a ControlNet attached first.  A plain call without guidance on the same binding (B = P = 3) ends composition
    assert _begin_composed(lib, smp, 3, 0, None, gs=0.0, plain=True) == 0, lib.ezdit_last_error()
    assert lib.ezdit_sampler_set_compose_weights(h, fl([1.0, 0.5]), 1, 2, st) == STATE       # the call was not begun composed
    assert lib.ezdit_sampler_attach_controlnet(h, cn._h, 1.0) == 0, lib.ezdit_last_error()
    try:
        assert _begin_composed(lib, smp, 1, 2, [1.0, 0.5]) == UNSUPPORTED
        assert b'ControlNet' in lib.ezdit_last_error()
    finally:
        assert lib.ezdit_sampler_attach_controlnet(h, None, 1.0) == 0
    # detached: the composed call begins again and is the run it was
    with torch.cuda.stream(smp.stream):
        smp.latents.copy_(t_(_case()[1]))
    assert _begin_composed(lib, smp, 1, 2, [1.0, 0.5]) == 0, lib.ezdit_last_error()
    assert torch.equal(_finish(smp), first)
    # K = 2 switched off ends the call
    assert lib.ezdit_sampler_set_compose_weights(h, None, 0, 0, st) == 0
    assert lib.ezdit_sampler_run(h, 1, 1, st) == STATE
    # through prepare(): no guidance, and what composition does not combine with
    with pytest.raises(ValueError, match='guidance'):
        _prepare('ddim', w, guidance_scale=None)
    with pytest.raises(ValueError, match='ControlNet'):
        _prepare('ddim', w, controlnet=cn, condition=torch.zeros(1, 1, 2 * L))
    with pytest.raises(ValueError, match='prepare'):
        _prepare('ddim').set_compose_weights(w)


def test_composed_begin_refuses_context_weights_that_are_on(lib):
    """A binding with a context of 128 tokens (one prompt of a timeline): with the context weights on, the composed begin is refused; off, it begins."""
    m = get_model('xs', 1)
    smp = _prepare('ddim', [[1.0, 0.5]], with_gt=False, pad_to=128)
    first = _finish(smp)
    st = C.c_void_p(smp.stream.cuda_stream)
    assert _begin_composed(lib, smp, 3, 0, None, gs=0.0, plain=True) == 0, lib.ezdit_last_error()
    m.set_context_weights(torch.ones(3, 1, smp.latents.shape[2]), st)
    try:
        assert _begin_composed(lib, smp, 1, 2, [1.0, 0.5]) == -2
        assert b'context weights' in lib.ezdit_last_error()
    finally:
        m.set_context_weights(None, st)
    with torch.cuda.stream(smp.stream):
        smp.latents.copy_(t_(_case()[1]))
    assert _begin_composed(lib, smp, 1, 2, [1.0, 0.5]) == 0, lib.ezdit_last_error()
    assert torch.equal(_finish(smp), first)
