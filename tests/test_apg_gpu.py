"""GPU tests of adaptive projected guidance in the fused sampler step (ezdit_cfg_apg_step, ezdit_sampler_set_apg, LatentSampler.prepare(apg=) / set_apg), through
the C ABI (run with -m gpu on an MI355X).

The reference has no APG.  The judges are the definition in float64 (tests/apg_emul.py step_fp64; the gate is 4 x the floor that the fp32 emulation of the kernels'
order keeps from it, computed here on the inputs of each case), the numpy oracle's loop with that definition (tests/golden/sampler_apg_xs.npz,
tools/mint_apg_golden.py) and, bit for bit, the plain operators and the plain call where APG is off.  xs width throughout.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import apg_emul as E
from tests.compose_emul import GATE_FLOORS
from tests.test_apg_host import mid_schedule_coef
from tests.test_sample_params_gpu import get_model, t_
from tests.util import DIFF, load_golden, record, rel_l2, sampler_case

pytestmark = pytest.mark.gpu

P_OP, C_OP = 3, 128
SENTINEL = np.float32(1234.5)
INVALID, UNSUPPORTED, STATE = -1, -2, -3
LOOP_GATE = 2e-2


def _scheduler(steps):
    from ezaudio_amd.scheduler import DDIMScheduler
    sch = DDIMScheduler(**DIFF)
    sch.set_timesteps(steps)
    return sch


@pytest.fixture(autouse=True)
def _leave_the_shared_model_plain(lib):
    """The xs model is shared with the other test modules: no test here leaves a table of its own on the handle."""
    yield
    m = get_model('xs', 1)
    if m._ws_key is not None:
        assert lib.ezdit_sampler_set_apg(m._h, None, None, None, None, 0, None, None) in (0, STATE)
        assert lib.ezdit_sampler_set_compose_weights(m._h, None, 0, 0, None) in (0, STATE)
        assert lib.ezdit_sampler_set_canvas(m._h, None, 0, 0, 1, None) in (0, STATE)
        m._compose_on = m._canvas_on = False
        m.set_lengths(None)


# ---------------------------------------------------------------------------------------------------
# 1. - 2. kernel level: ezdit_cfg_apg_step
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _operator_case(L, lens, ms):
    """apg_emul.operator_case at step 7 of 50; the DDIM form applies no c_hist.  The momentum rows of the sample without guidance hold a sentinel (they are
    not read, so the reference sees the same rows).  Returned arrays are shared: nobody writes to them."""
    pred, lat, hist, mom, params, ln = E.operator_case(L, list(lens) if lens else None, mid_schedule_coef())
    if not ms:
        params[:, 7] = 0.0
    mom[2] = SENTINEL
    return pred, lat, hist, mom, params, ln


def _poisoned(case, ms):
    """NaN wherever the operator must not read: the padded frames of every input, the momentum rows of the sample whose beta_eff is 0, the history of the
    sample whose c_hist is 0, the unconditional row of the sample without guidance."""
    pred, lat, hist, mom, params, ln = tuple(np.array(a) for a in case[:5]) + (case[5],)
    nan = np.float32(np.nan)
    for p, n in enumerate(ln):
        pred[p, :, n:] = pred[P_OP + p, :, n:] = lat[p, :, n:] = hist[p, :, n:] = nan
        if p != 2:
            mom[p, :, n:] = nan
    assert params[1, 10] == 0 and params[1, 11] != 0 and params[2, 0] == 0 and params[2, 7] == 0
    mom[1] = nan
    hist[2] = nan
    pred[P_OP + 2] = nan
    return pred, lat, hist, mom, params, ln


def _run_operator(lib, case, ms, noise=None):
    """One call on copies of the case's arrays; returns (latents, x0_hist or None, momentum) as numpy."""
    pred, lat, hist, mom, params, ln = case
    L = lat.shape[2]
    pd, ld, md, pr = t_(pred), t_(lat), t_(mom), t_(params)
    hd = t_(hist) if ms else None
    scratch = torch.full((P_OP * 256,), float('nan'), device='cuda:0')      # (every slot that is read was written by the statistics pass)
    kl = torch.tensor(ln, dtype=torch.int32, device='cuda:0') if ln != [L] * P_OP else None
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    rc = lib.ezdit_cfg_apg_step(pd.data_ptr(), ld.data_ptr(), ptr(noise), ptr(hd), md.data_ptr(), pr.data_ptr(), ptr(kl), L, P_OP, C_OP * L,
                                scratch.data_ptr(), None)
    assert rc == 0, lib.ezdit_last_error()
    torch.cuda.synchronize()
    return ld.cpu().numpy(), None if hd is None else hd.cpu().numpy(), md.cpu().numpy()


def _outputs(got, ms):
    return (got[0], got[1], got[2]) if ms else (got[0], got[2])


@pytest.mark.parametrize('ms', [False, True], ids=['ddim', 'multistep'])
@pytest.mark.parametrize('L,lens', [(96, None), (150, None), (150, (150, 77, 1)), (150, (131, 77, 1))])
def test_apg_step_operator_against_fp64_and_reads_nothing_it_must_not(lib, L, lens, ms):
    """P = 3, C = 128: n = 12288 leaves statistics workgroups without an element, n = 19200 sends threads round the stride loop a second time, length 1 is the
    shortest sample.  Sample 0: APG with momentum and a cap that bites; sample 1: APG at its first step (beta_eff 0); sample 2: no guidance.  The call runs on
    the poisoned inputs and must come out finite, exactly 0 on padded frames, with the sentinel rows untouched, and within 4 emulated floors of float64."""
    case = _operator_case(L, lens, ms)
    pred, lat, hist, mom, params, ln = case
    got = _run_operator(lib, _poisoned(case, ms), ms)
    for t in _outputs(got, ms):
        assert np.isfinite(t).all()
    for p, n in enumerate(ln):
        assert not got[0][p, :, n:].any(), 'padded latent frames must be exactly 0'
        assert not ms or not got[1][p, :, n:].any(), 'padded history frames must be exactly 0'
        assert p == 2 or not got[2][p, :, n:].any(), 'padded momentum frames of an APG sample must be exactly 0'
    assert np.array_equal(got[2][2], np.full_like(mom[2], SENTINEL)), 'the momentum rows of the sample without guidance were touched'
    ref = E.step_fp64(pred, lat, hist, mom, params, ln)
    floor, far = E.floor_and_mistakes(case)
    dist = E.distance(_outputs(got, ms), _outputs(ref, ms), ln)
    record(f'apg step operator L={L} lens={lens} {"multistep" if ms else "ddim"}: rel-L2 vs fp64 {dist:.3e} = {dist / floor:.2f} floors '
           f'(floor {floor:.3e}, gate {GATE_FLOORS} floors, nearest mistake {min(far.values()) / floor:.0f} floors)')
    assert dist <= GATE_FLOORS * floor, (dist, floor)
    clean = _run_operator(lib, case, ms)                                # what is poisoned is not read: the clean inputs give the same bits
    for a, b in zip(_outputs(clean, ms), _outputs(got, ms)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize('lens', [None, (131, 77, 1)])
def test_a_table_that_is_off_for_every_sample_is_bitwise_the_plain_operators(lib, lens):
    """on = 0 everywhere: guidance 5 with rescale 0.75, guidance 2, no guidance -- against ezdit_cfg_ddim_step_per_sample (with noise) and
    ezdit_cfg_multistep_step on the first eight columns of the same rows.  The momentum is not touched."""
    L = 150
    for ms in (False, True):
        pred, lat, hist, mom, params, ln = _operator_case(L, lens, ms)
        params = np.array(params)
        params[:, 11] = 0.0
        params[0, 1] = 0.75
        params[0, 6] = 0.0 if ms else 0.3                               # sigma: step noise in the DDIM form
        noise = None if ms else t_(np.random.default_rng(5).standard_normal((P_OP, C_OP, L)).astype(np.float32))
        got = _run_operator(lib, (pred, lat, hist, mom, params, ln), ms, noise)
        assert np.array_equal(got[2], mom), 'momentum touched'
        pd, ld, pr = t_(pred), t_(lat), t_(np.ascontiguousarray(params[:, :8]))
        scratch = torch.zeros(P_OP * 256, device='cuda:0')
        kl = torch.tensor(ln, dtype=torch.int32, device='cuda:0') if lens else None
        klp = kl.data_ptr() if lens else None
        if ms:
            hd = t_(hist)
            assert lib.ezdit_cfg_multistep_step(pd.data_ptr(), ld.data_ptr(), hd.data_ptr(), pr.data_ptr(), klp, L, P_OP, C_OP * L, scratch.data_ptr(), None) == 0
        else:
            assert lib.ezdit_cfg_ddim_step_per_sample(pd.data_ptr(), ld.data_ptr(), noise.data_ptr(), pr.data_ptr(), klp, L, P_OP, C_OP * L,
                                                      scratch.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert np.isfinite(got[0]).all() and np.array_equal(ld.cpu().numpy(), got[0]), ms
        if ms:
            assert np.array_equal(hd.cpu().numpy(), got[1])


@pytest.mark.parametrize('lens', [None, (131, 77, 1)])
def test_eta_1_without_cap_and_momentum_is_plain_cfg_within_the_gate(lib, lens):
    L = 150
    for ms in (False, True):
        pred, lat, hist, mom, params, ln = _operator_case(L, lens, ms)
        params = np.array(params)
        params[:2, 8:] = (1.0, 0.0, 0.0, 1.0)
        case = (pred, lat, hist, mom, params, ln)
        got = _run_operator(lib, case, ms)
        plain = np.array(params)
        plain[:, 11] = 0.0
        assert not plain[:, 1][plain[:, 0] > 0].any()                   # (no rescale on the guided samples: plain CFG)
        ref = E.step_fp64(pred, lat, hist, mom, plain, ln)
        floor, _ = E.floor_and_mistakes(case)
        dist = E.distance(got[:2] if ms else got[:1], ref[:2] if ms else ref[:1], ln)
        record(f'apg step operator eta_apg=1 r=0 momentum=0 lens={lens} {"multistep" if ms else "ddim"}: rel-L2 vs plain CFG in fp64 {dist:.3e} '
               f'= {dist / floor:.2f} floors (floor {floor:.3e})')
        assert dist <= GATE_FLOORS * floor, (dist, floor)


def test_apg_step_operator_refusals(lib):
    pred, lat, hist, mom, params, ln = _operator_case(96, None, True)
    pd, ld, hd, md, pr = (t_(a) for a in (pred, lat, hist, mom, params))
    scratch = torch.zeros(P_OP * 256, device='cuda:0')
    args = [pd.data_ptr(), ld.data_ptr(), None, hd.data_ptr(), md.data_ptr(), pr.data_ptr(), None, 96, P_OP, C_OP * 96, scratch.data_ptr(), None]
    for i in (0, 1, 4, 5, 10):                                          # a null pointer of each required kind
        assert lib.ezdit_cfg_apg_step(*(args[:i] + [None] + args[i + 1:])) == INVALID, i
    for i, v in ((8, 0), (9, 1), (2, pd.data_ptr())):                   # P, n, noise together with a history
        assert lib.ezdit_cfg_apg_step(*(args[:i] + [v] + args[i + 1:])) == INVALID, (i, v)
    kl = torch.tensor([96, 77, 1], dtype=torch.int32, device='cuda:0')
    assert lib.ezdit_cfg_apg_step(*(args[:6] + [kl.data_ptr(), 7] + args[8:])) == INVALID      # L does not divide n
    torch.cuda.synchronize()
    assert np.array_equal(ld.cpu().numpy(), lat) and np.array_equal(md.cpu().numpy(), mom)      # nothing was launched


# ---------------------------------------------------------------------------------------------------
# 3. the fused loop
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case():
    cfg, sd, inp, init, noises, g, meta = sampler_case('smp_xs_e0')
    assert (meta['size'], meta['seed_w'], meta['steps'], meta['eta'], meta['with_gt']) == ('xs', 1, 20, 0.0, True)
    return inp, init, meta


@functools.lru_cache(maxsize=None)
def _golden():
    g, gm = load_golden('sampler_apg_xs')
    assert gm['base'] == 'smp_xs_e0' and gm['steps'] == _case()[2]['steps'] and gm['guidance_rescale'] == 0.0
    return g, dict(eta=gm['eta_apg'], norm_threshold=gm['norm_threshold'], momentum=gm['momentum'])


def _prepare(solver='ddim', apg=None, P=1, with_gt=True, **kw):
    """The fixture's sample P times at guidance_rescale 0 (the goldens' setting)."""
    from ezaudio_amd.sampler import LatentSampler
    inp, init, meta = _case()
    smp = LatentSampler(get_model('xs', 1), _scheduler(meta['steps']))
    rep = lambda a: t_(a).repeat(P, *([1] * (a.ndim - 1)))   # noqa: E731
    gt = t_(inp['gt'][0:1]) if with_gt else None
    gm = t_(inp['gt_mask'][0:1]) if with_gt else None
    smp.prepare(rep(inp['ctx'][0:1]), rep(inp['ctx_mask'][0:1]), rep(inp['ctx'][1:2]), rep(inp['ctx_mask'][1:2]), rep(init), None,
                kw.pop('guidance_scale', meta['guidance_scale']), 0.0, meta['steps'], 0.0, gt=gt, gt_mask=gm, solver=solver, apg=apg, **kw)
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
def _runs():
    """The APG DDIM and 2M runs of the golden's settings and the plain DDIM and 2M runs, P = 1, graph replay: computed once, shared, never modified."""
    a = _golden()[1]
    return {('ddim', True): _finish(_prepare('ddim', a)), ('dpmpp_2m', True): _finish(_prepare('dpmpp_2m', a)),
            ('ddim', False): _finish(_prepare('ddim')), ('dpmpp_2m', False): _finish(_prepare('dpmpp_2m'))}


def test_fused_apg_loop_against_the_numpy_oracle_graph_and_eager(lib):
    """Gate: the project's loop gate 2e-2 for DDIM and dpmpp_2m, graph replay and eager launches; the goldens lie at least 10 gates from plain CFG, and so must
    the runs, less the two runs' own gates."""
    inp, init, meta = _case()
    g, a = _golden()
    gt, gm = t_(inp['gt'][0:1]), t_(inp['gt_mask'][0:1])
    fin = lambda lat: torch.where(gm, lat, gt).cpu().numpy()   # noqa: E731
    for solver, key in (('ddim', 'latent_ddim'), ('dpmpp_2m', 'latent_2m')):
        run = _runs()[solver, True]
        eager = _finish(_prepare(solver, a), use_graph=False)
        for how, lat in (('graph', run), ('eager', eager)):
            e = rel_l2(fin(lat), g[key])
            record(f'sampler_apg_xs ({solver}, {how}, {a}): final-latent rel-L2 vs the numpy oracle loop {e:.3e}')
            assert torch.isfinite(lat).all() and e < LOOP_GATE, (solver, how, e)
            d = rel_l2(fin(lat), fin(_runs()[solver, False]))
            record(f'sampler_apg_xs ({solver}, {how}): APG vs plain CFG run {d:.3e}')
            assert d > (10 - 2) * LOOP_GATE, (solver, how, d)
        assert torch.equal(eager, run), solver


def test_apg_switched_off_is_bitwise_the_plain_call_and_no_entry_calls_nothing_new(lib):
    a = _golden()[1]
    plain = _runs()['ddim', False]
    smp = _prepare('ddim', [None])
    assert smp.apg_m is None and torch.equal(_finish(smp), plain)
    smp = _prepare('ddim', a)
    assert torch.equal(_finish(smp), _runs()['ddim', True])
    smp.set_apg(None)
    assert _rewind(lib, smp) == 0
    assert torch.equal(_finish(smp), plain)
    # on with on = 0 for the sample: the APG instantiations on the plain branch, the same bits
    h, st = smp.unet._h, C.c_void_p(smp.stream.cuda_stream)
    f1 = lambda v: (C.c_float * 1)(v)   # noqa: E731
    assert lib.ezdit_sampler_set_apg(h, f1(0.0), f1(1.0), f1(-0.5), (C.c_int32 * 1)(0), 1, smp.apg_m.data_ptr(), st) == 0, lib.ezdit_last_error()
    assert _rewind(lib, smp) == 0
    assert torch.equal(_finish(smp), plain)


# ---------------------------------------------------------------------------------------------------
# 4. one batched call: lengths (96, 77, 50), per-sample guidance, APG on samples 0 and 2
# ---------------------------------------------------------------------------------------------------
LENGTHS_B, GS_B, GR_B = (96, 77, 50), (3.5, 5.0, 2.0), (0.0, 0.75, 0.0)
APG_B = (dict(norm_threshold=8.0), None, dict(eta=0.5, momentum=0.0))


def _batched(idx, apg, solver='ddim'):
    """The requests `idx` of the batch in one call, padded to the longest of LENGTHS_B or, alone, at their own length."""
    from ezaudio_amd.sampler import LatentSampler
    from tests.test_compose_gpu import _request
    rows = [_request(LENGTHS_B[i]) for i in idx]
    Lmax = max(LENGTHS_B) if len(idx) > 1 else rows[0]['L']
    init = np.full((len(rows), 128, Lmax), np.nan, np.float32)          # (padded frames of the init noise hold NaN: they are not read)
    for i, r in enumerate(rows):
        init[i, :, :r['L']] = r['init'][0]
    cat = lambda k, sl: t_(np.concatenate([r[k][sl] for r in rows], 0))   # noqa: E731
    smp = LatentSampler(get_model('xs', 1), _scheduler(20))
    smp.prepare(cat('ctx', slice(0, 1)), cat('mask', slice(0, 1)), cat('ctx', slice(1, 2)), cat('mask', slice(1, 2)), t_(init), None,
                [GS_B[i] for i in idx], [GR_B[i] for i in idx], 20, 0.0, lengths=[LENGTHS_B[i] for i in idx] if len(idx) > 1 else None,
                apg=None if apg is None else [apg[i] for i in idx], solver=solver)
    return _finish(smp)


@pytest.mark.parametrize('solver', ['ddim', 'dpmpp_2m'])
def test_one_batched_call_with_lengths_guidance_and_a_mix_of_apg_and_cfg_samples(lib, solver):
    lat = _batched((0, 1, 2), APG_B, solver)
    assert torch.isfinite(lat).all()
    for i, L in enumerate(LENGTHS_B):
        alone = _batched((i,), APG_B, solver)
        e = rel_l2(lat[i, :, :L].cpu().numpy(), alone[0].cpu().numpy())
        record(f'apg batch P = 3 ({solver}), lengths {LENGTHS_B}, sample {i} (apg {APG_B[i]}): final-latent rel-L2 vs its single call {e:.3e}')
        assert e < LOOP_GATE, (i, e)
        assert not lat[i, :, L:].any(), 'padded latent frames must be exactly 0'
    plain = _batched((0, 1, 2), None, solver)
    assert torch.equal(lat[1], plain[1]), 'the sample without APG is not bitwise the sample of the plain call of the same batch'
    for i in (0, 2):
        assert rel_l2(lat[i].cpu().numpy(), plain[i].cpu().numpy()) > 1e-3, i    # (APG did something)


# ---------------------------------------------------------------------------------------------------
# 5. run-time values, the start table
# ---------------------------------------------------------------------------------------------------
def test_a_captured_step_reads_the_apg_table_at_run_time(lib, capfd):
    a = _golden()[1]
    other = dict(eta=0.3, norm_threshold=2.0 * a['norm_threshold'], momentum=-0.2)
    m = get_model('xs', 1)
    smp = _prepare('ddim', a)
    assert lib.ezdit_set_option(m._h, b'trace_launches', 1) == 0
    try:
        def captured(n):
            capfd.readouterr()
            smp.run(n, use_graph=True)
            smp.stream.synchronize()
            return 'launch ' in capfd.readouterr().err
        assert captured(1), 'first run'
        assert not captured(19), 'second run replays'
        first = smp.finish().clone()
        smp.set_apg(other)
        assert _rewind(lib, smp) == 0
        assert not captured(20), 'new values into a table that is on keep the graph'
        second = smp.finish().clone()
        smp.set_apg(None)
        assert _rewind(lib, smp) == 0
        assert captured(20), 'off drops the graph'
        third = smp.finish().clone()
        smp.set_apg(a)
        assert _rewind(lib, smp) == 0
        assert captured(20), 'on drops the graph'
        fourth = smp.finish().clone()
    finally:
        assert lib.ezdit_set_option(m._h, b'trace_launches', 0) == 0
    assert torch.equal(first, _runs()['ddim', True]) and torch.equal(fourth, first)
    assert torch.equal(third, _runs()['ddim', False])
    assert torch.isfinite(second).all() and not torch.equal(second, first)
    assert torch.equal(second, _finish(_prepare('ddim', other)))


@pytest.mark.parametrize('solver', ['ddim', 'dpmpp_2m'])
def test_a_start_table_holds_a_sample_and_its_momentum_and_first_steps_ignore_nan(lib, solver):
    """P = 2 from a clean latent, start steps (0, 6), the momentum buffer full of NaN when the run begins.  Below step 6 the second sample's latents and momentum
    rows keep their bits (NaN included); its first step does not read them; both samples end finite and as the call with the sample alone gives them."""
    inp, init, meta = _case()
    a = _golden()[1]
    clean = t_(inp['gt'][0:1]) * 0.5
    smp = _prepare(solver, a, P=2, with_gt=False, init_latents=clean, start_steps=[0, 6])
    with torch.cuda.stream(smp.stream):
        smp.apg_m.fill_(float('nan'))
    smp.stream.synchronize()
    begun = smp.latents.clone()
    held = _finish(smp, n=6)
    assert torch.equal(held[1], begun[1]) and not torch.equal(held[0], begun[0])
    assert torch.isnan(smp.apg_m[1]).all() and torch.isfinite(smp.apg_m[0]).all()
    assert lib.ezdit_set_step(smp.unet._h, 3, C.c_void_p(smp.stream.cuda_stream)) == STATE      # only the run's first step
    done = _finish(smp, n=meta['steps'] - 6)
    assert torch.isfinite(done).all() and torch.isfinite(smp.apg_m).all() and not torch.equal(done[1], begun[1])
    for p, s0 in enumerate((0, 6)):
        one = _finish(_prepare(solver, a, with_gt=False, init_latents=clean, start_steps=[s0]))
        e = rel_l2(done[p].cpu().numpy(), one[0].cpu().numpy())
        record(f'apg with a start table ({solver}), sample {p} started at step {s0}: rel-L2 vs the call with it alone {e:.3e}')
        assert e < LOOP_GATE, (p, e)


# ---------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------
def test_apg_refusals_leave_the_call_as_it_was(lib):
    """Every refusal with its code; none launches anything or changes the call: the run behind it is bit for bit the run before."""
    from ezaudio_amd import _lib
    a = _golden()[1]
    smp = _prepare('ddim', a, with_gt=False)
    h, st = smp.unet._h, C.c_void_p(smp.stream.cuda_stream)
    first = _finish(smp)
    launches = lib.ezdit_last_launch_count(h)
    nan, inf = float('nan'), float('inf')
    fl = lambda *v: (C.c_float * len(v))(*v)   # noqa: E731
    i32 = lambda *v: (C.c_int32 * len(v))(*v)   # noqa: E731
    L = smp.latents.shape[2]
    mp = smp.apg_m.data_ptr()
    two = torch.zeros(2, 128, L, device='cuda:0')
    for what, call, rc in (
            ('another P', lambda: lib.ezdit_sampler_set_apg(h, fl(0, 0), fl(0, 0), fl(0, 0), i32(1, 1), 2, two.data_ptr(), st), INVALID),
            ('only some arrays', lambda: lib.ezdit_sampler_set_apg(h, fl(0), None, fl(0), i32(1), 1, mp, st), INVALID),
            ('no on array', lambda: lib.ezdit_sampler_set_apg(h, fl(0), fl(0), fl(0), None, 1, mp, st), INVALID),
            ('no momentum buffer', lambda: lib.ezdit_sampler_set_apg(h, fl(0), fl(0), fl(0), i32(1), 1, None, st), INVALID),
            ('NaN eta', lambda: lib.ezdit_sampler_set_apg(h, fl(nan), fl(0), fl(0), i32(1), 1, mp, st), INVALID),
            ('infinite cap', lambda: lib.ezdit_sampler_set_apg(h, fl(0), fl(inf), fl(0), i32(1), 1, mp, st), INVALID),
            ('NaN momentum', lambda: lib.ezdit_sampler_set_apg(h, fl(0), fl(0), fl(nan), i32(0), 1, mp, st), INVALID),
            ('negative cap', lambda: lib.ezdit_sampler_set_apg(h, fl(0), fl(-1.0), fl(0), i32(1), 1, mp, st), INVALID),
            ('a canvas while APG is on', lambda: lib.ezdit_sampler_set_canvas(h, i32(0), 1, L, 1, st), UNSUPPORTED),
            ('a ring while APG is on', lambda: lib.ezdit_sampler_set_canvas_loop(h, i32(0), 1, L, 1, st), UNSUPPORTED),
            ('ezdit_set_step(3) while APG is on', lambda: lib.ezdit_set_step(h, 3, st), STATE)):
        assert call() == rc, what
        assert lib.ezdit_last_error(), what
        assert lib.ezdit_last_launch_count(h) == launches, what
        assert _rewind(lib, smp) == 0
        assert torch.equal(_finish(smp), first), what
    # the other way round: a canvas, a ring or composition first.  Each refuses the table and goes on as it was
    smp.set_apg(None)
    assert _rewind(lib, smp) == 0
    plain = _finish(smp)
    assert torch.equal(plain, _finish(_prepare('ddim', None, with_gt=False)))
    on = lambda: lib.ezdit_sampler_set_apg(h, fl(a['eta']), fl(a['norm_threshold']), fl(a['momentum']), i32(1), 1, mp, st)   # noqa: E731
    for setter in (lib.ezdit_sampler_set_canvas, lib.ezdit_sampler_set_canvas_loop):
        assert setter(h, i32(0), 1, L, 1, st) == 0, lib.ezdit_last_error()
        assert on() == UNSUPPORTED and b'canvas' in lib.ezdit_last_error()
        assert setter(h, None, 0, 0, 1, st) == 0
    steps = _case()[2]['steps']
    arr = (_lib.EzditDdimCoef * steps)(*[_lib.EzditDdimCoef(*c) for c in _scheduler(steps).ddim_coefficients(0.0)])
    gs = float(_case()[2]['guidance_scale'])
    with torch.cuda.stream(smp.stream):
        smp.latents.copy_(t_(_case()[1]))
        assert lib.ezdit_sampler_begin_composed(h, smp.latents.data_ptr(), 1, None, arr, steps, gs, 0.0, None, None, 1, fl(1.0), st) == 0, lib.ezdit_last_error()
    assert on() == UNSUPPORTED and b'composed' in lib.ezdit_last_error()
    assert torch.equal(_finish(smp), plain)                             # (K = 1, w = 1: the plain call's bits)
    # a sampler begun without CFG rows (B = P = 2 on the same binding): on != 0 is refused, a table that is off for both samples is not
    with torch.cuda.stream(smp.stream):
        assert lib.ezdit_sampler_begin(h, two.data_ptr(), 2, None, arr, steps, 0.0, 0.0, None, None, st) == 0, lib.ezdit_last_error()
    m2 = torch.zeros_like(two)
    assert lib.ezdit_sampler_set_apg(h, fl(0, 0), fl(0, 0), fl(0, 0), i32(0, 1), 2, m2.data_ptr(), st) == INVALID and b'CFG rows' in lib.ezdit_last_error()
    assert lib.ezdit_sampler_set_apg(h, fl(0, 0), fl(0, 0), fl(0, 0), i32(0, 0), 2, m2.data_ptr(), st) == 0, lib.ezdit_last_error()
    # a begin ends the table: the plain call again, and the APG call after it is the run it was
    with torch.cuda.stream(smp.stream):
        smp.latents.copy_(t_(_case()[1]))
        assert lib.ezdit_sampler_begin(h, smp.latents.data_ptr(), 1, None, arr, steps, gs, 0.0, None, None, st) == 0, lib.ezdit_last_error()
    assert torch.equal(_finish(smp), plain)
    assert on() == 0, lib.ezdit_last_error()
    assert _rewind(lib, smp) == 0
    assert torch.equal(_finish(smp), first)
    # through prepare(): what APG does not combine with
    for kw, word in ((dict(guidance_scale=None), 'guidance'), (dict(canvas=([0], L, 1)), 'canvas'), (dict(canvas_loop=([0], L, 1)), 'canvas'),
                     (dict(compose_weights=[[1.0, 0.5]], compose_text=torch.zeros(1, 1, 20, 8), compose_mask=torch.ones(1, 1, 20, dtype=torch.bool)), 'compose')):
        with pytest.raises(ValueError, match=word):
            _prepare('ddim', a, with_gt=False, **kw)
    with pytest.raises(ValueError, match='entries'):
        _prepare('ddim').set_apg([a, a])
