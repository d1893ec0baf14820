"""GPU tests of the DPM-Solver++(2M) multistep solver (ezdit_cfg_multistep_step, ezdit_sampler_set_multistep, LatentSampler.prepare(solver='dpmpp_2m')).

The reference has no such solver.  The judges are the update's formula in float64 (kernel level), the numpy oracle's loop with that update
(tests/golden/sampler_ms_xs.npz, tools/mint_multistep_golden.py) and, bit for bit, the DDIM path where the new term is off.  xs width throughout.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests.test_sample_params_gpu import _row, get_model, t_
from tests.util import DIFF, load_golden, record, rel_l2, sampler_case

pytestmark = pytest.mark.gpu


def _scheduler(steps):
    from ezaudio_amd.scheduler import DDIMScheduler
    sch = DDIMScheduler(**DIFF)
    sch.set_timesteps(steps)
    return sch


# ---------------------------------------------------------------------------------------------------
# 1. kernel level: ezdit_cfg_multistep_step against float64
# ---------------------------------------------------------------------------------------------------
def _fp64_step(pred, lat, hist, params, lens):
    """CFG combine + guidance rescale per sample over its valid frames, then x_next = c_x0 x0 + c_dir eps + c_hist (x0 - hist) and hist = x0, in float64."""
    P = lat.shape[0]
    out, hout = np.zeros(lat.shape, np.float64), np.zeros(lat.shape, np.float64)
    for p in range(P):
        gs, phi, sa, sb, cx0, cdir, _, ch = (float(v) for v in params[p])
        n = lens[p]
        c, x = pred[p, :, :n].astype(np.float64), lat[p, :, :n].astype(np.float64)
        v = c
        if gs > 0:
            u = pred[P + p, :, :n].astype(np.float64)
            v = u + gs * (c - u)
            if phi > 0:
                v = phi * (v * (c.std(ddof=1) / v.std(ddof=1))) + (1 - phi) * v
        x0, eps = sa * x - sb * v, sa * v + sb * x
        prev = cx0 * x0 + cdir * eps
        if ch != 0:
            prev = prev + ch * (x0 - hist[p, :, :n].astype(np.float64))
        out[p, :, :n], hout[p, :, :n] = prev, x0
    return out, hout


def _operator_case(L, lens, c_hist):
    """P = 3, n = 128 L (tests/test_sample_params_gpu.py's shapes: 12288 elements are less than one grid sweep of 64 x 256, 19200 one sweep and a partial
    one).  Sample 0 guidance + rescale, sample 1 guidance alone, sample 2 no guidance with NaN in its unconditional prediction."""
    P, Cc = 3, 128
    g = torch.Generator().manual_seed(2000 + L)
    pred = (torch.randn(2 * P, Cc, L, generator=g) * 1.3).numpy()
    lat = torch.randn(P, Cc, L, generator=g).numpy()
    hist = torch.randn(P, Cc, L, generator=g).numpy()
    t = int(_scheduler(50).timesteps[7])
    co = _scheduler(50)._coef(t, 0.0)
    params = np.zeros((P, 8), np.float32)
    for p, (gs, phi) in enumerate(((5.0, 0.75), (2.0, 0.0), (0.0, 0.4))):
        params[p] = (gs, phi) + co + (c_hist[p],)
    assert params[0, 6] == 0.0
    return P, Cc, pred, lat, hist, params, lens or [L] * P


@pytest.mark.parametrize('L,lens', [(96, None), (150, None), (150, [150, 77, 1])])
def test_multistep_step_operator_against_fp64(lib, L, lens):
    """c_hist (0.05, 0.4, 0) per sample; the history of the c_hist = 0 sample is NaN (it must not be read), and with lengths the padded frames of every
    input hold NaN.  Latents AND the written history within rel-L2 5e-6 of float64, the gate of tests/test_gpu.py::test_cfg_ddim_step_operator_against_oracle;
    padded frames exactly 0 in both."""
    P, Cc, pred, lat, hist, params, ln = _operator_case(L, lens, (0.05, 0.4, 0.0))
    n = Cc * L
    ref, href = _fp64_step(pred, lat, hist, params, ln)
    hist[2] = np.nan
    pred[P + 2] = np.nan
    for p, k in enumerate(ln):
        pred[p, :, k:] = np.nan
        pred[P + p, :, k:] = np.nan
        lat[p, :, k:] = np.nan
        hist[p, :, k:] = np.nan
    pd, ld, hd, pr = t_(pred), t_(lat), t_(hist), t_(params)
    scratch = torch.zeros(P * 256, device='cuda:0')
    kl = torch.tensor(ln, dtype=torch.int32, device='cuda:0') if lens else None
    rc = lib.ezdit_cfg_multistep_step(pd.data_ptr(), ld.data_ptr(), hd.data_ptr(), pr.data_ptr(), kl.data_ptr() if lens else None, L, P, n,
                                      scratch.data_ptr(), None)
    assert rc == 0, lib.ezdit_last_error()
    torch.cuda.synchronize()
    got, hgot = ld.cpu().numpy(), hd.cpu().numpy()
    assert np.isfinite(got).all() and np.isfinite(hgot).all()
    for p, k in enumerate(ln):
        e, eh = rel_l2(got[p, :, :k], ref[p, :, :k]), rel_l2(hgot[p, :, :k], href[p, :, :k])
        record(f'multistep step operator L={L} lens={lens} sample {p} (c_hist {params[p, 7]:g}): rel-L2 vs fp64 latents {e:.3e}, history {eh:.3e}')
        assert e < 5e-6 and eh < 5e-6, (p, e, eh)
        zeros = np.zeros((Cc, L - k), np.float32)
        assert np.array_equal(got[p, :, k:], zeros) and np.array_equal(hgot[p, :, k:], zeros), 'padded frames must be exactly 0'
    args = (pd.data_ptr(), ld.data_ptr(), hd.data_ptr(), pr.data_ptr(), None, L, P, n, scratch.data_ptr(), None)
    for i in (0, 1, 2, 3, 8):                                         # a null pointer of each kind is refused
        assert lib.ezdit_cfg_multistep_step(*(args[:i] + (None,) + args[i + 1:])) == -1, i


@pytest.mark.parametrize('L,lens', [(150, None), (150, [150, 77, 1])])
def test_multistep_step_with_c_hist_zero_is_bitwise_the_ddim_step(lib, L, lens):
    P, Cc, pred, lat, hist, params, ln = _operator_case(L, lens, (0.0, 0.0, 0.0))
    n = Cc * L
    hist[:] = np.nan
    pred[P + 2] = np.nan
    pd, pr = t_(pred), t_(params)
    scratch = torch.zeros(P * 256, device='cuda:0')
    kl = torch.tensor(ln, dtype=torch.int32, device='cuda:0') if lens else None
    klp = kl.data_ptr() if lens else None
    a, b, hd = t_(lat), t_(lat), t_(hist)
    assert lib.ezdit_cfg_ddim_step_per_sample(pd.data_ptr(), a.data_ptr(), None, pr.data_ptr(), klp, L, P, n, scratch.data_ptr(), None) == 0
    assert lib.ezdit_cfg_multistep_step(pd.data_ptr(), b.data_ptr(), hd.data_ptr(), pr.data_ptr(), klp, L, P, n, scratch.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert torch.isfinite(hd).all()                                    # the history is written all the same


# ---------------------------------------------------------------------------------------------------
# the fused loop
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case():
    cfg, sd, inp, init, noises, g, meta = sampler_case('smp_xs_e0')
    assert (meta['size'], meta['seed_w'], meta['steps'], meta['eta'], meta['with_gt']) == ('xs', 1, 20, 0.0, True)
    return inp, init, meta


def _prepare(solver, P=1, with_gt=True, **kw):
    from ezaudio_amd.sampler import LatentSampler
    inp, init, meta = _case()
    m = get_model('xs', 1)
    smp = LatentSampler(m, _scheduler(meta['steps']))
    text, tm = t_(inp['ctx'][0:1]).repeat(P, 1, 1), t_(inp['ctx_mask'][0:1]).repeat(P, 1)
    un, um = t_(inp['ctx'][1:2]).repeat(P, 1, 1), t_(inp['ctx_mask'][1:2]).repeat(P, 1)
    gt = t_(inp['gt'][0:1]) if with_gt else None
    gm = t_(inp['gt_mask'][0:1]) if with_gt else None
    args = dict(guidance_scale=meta['guidance_scale'], guidance_rescale=meta['guidance_rescale'], eta=0.0, step_noises=None)
    args.update(kw)
    smp.prepare(text, tm, un, um, t_(init).repeat(P, 1, 1), args['step_noises'], args['guidance_scale'], args['guidance_rescale'], meta['steps'],
                args['eta'], gt=gt, gt_mask=gm, solver=solver)
    return smp


def _finish(smp, use_graph=True, pieces=None):
    for n in (pieces or [None]):
        smp.run(n, use_graph=use_graph)
    lat = smp.finish().clone()
    torch.cuda.synchronize()
    return lat


def _rewind(lib, smp):
    inp, init, meta = _case()
    with torch.cuda.stream(smp.stream):
        smp.latents.copy_(t_(init).expand_as(smp.latents))
        return lib.ezdit_set_step(smp.unet._h, 0, C.c_void_p(smp.stream.cuda_stream))


@functools.lru_cache(maxsize=None)
def _runs():
    """The 2M and the DDIM run of the fixture's inputs, P = 1, graph replay: computed once, shared, never modified."""
    return _finish(_prepare('dpmpp_2m')), _finish(_prepare('ddim'))


def test_fused_multistep_loop_against_the_numpy_oracle(lib):
    """Gate: the project's loop gate 2e-2 (tests/test_gpu.py::test_sampler_matches_reference_loop_golden); the bf16 denoiser's error dominates, so the
    number belongs next to smp_xs_e0's own DDIM figure, which is recorded beside it."""
    inp, init, meta = _case()
    g, gmeta = load_golden('sampler_ms_xs')
    assert gmeta['base'] == 'smp_xs_e0' and gmeta['steps'] == meta['steps']
    # (the float32 alpha_bar table, and c_hist with it, differs in its last bits from host to host -- scheduler.py `_linspace_f32` -- so the fixture's c_hist is
    # compared in structure only; a schedule that drifted shows in the gate below)
    ch = _scheduler(meta['steps']).multistep_coefficients()
    assert len(ch) == len(g['c_hist']) and [c == 0.0 for c in ch] == [c == 0.0 for c in g['c_hist']]
    ms, ddim = _runs()
    gt, gm = t_(inp['gt'][0:1]), t_(inp['gt_mask'][0:1])
    fin = lambda lat: torch.where(gm, lat, gt).cpu().numpy()   # noqa: E731  src/inference.py:104-105
    e = rel_l2(fin(ms), g['latent'])
    e_ddim = rel_l2(fin(ddim), sampler_case('smp_xs_e0')[5]['latent'])
    d = rel_l2(ms.cpu().numpy(), ddim.cpu().numpy())
    record(f'sampler_ms_xs (dpmpp_2m, 20 steps): final-latent rel-L2 vs the numpy oracle loop {e:.3e} (smp_xs_e0 DDIM on the same tree: {e_ddim:.3e}); '
           f'2M vs DDIM run {d:.3e}')
    assert torch.isfinite(ms).all() and e < 2e-2, e
    assert d > 1e-3, d                                                  # the term is really applied


def test_multistep_graph_equals_eager_batch_equals_single_and_runs_in_pieces(lib):
    ms, _ = _runs()
    assert torch.equal(_finish(_prepare('dpmpp_2m'), use_graph=False), ms)
    three = _finish(_prepare('dpmpp_2m', P=3))
    for i in range(3):
        assert torch.equal(three[i:i + 1], ms), i                       # samples never interact
    inp, init, meta = _case()
    assert torch.equal(_finish(_prepare('dpmpp_2m'), pieces=[3, meta['steps'] - 3]), ms)    # the history survives between calls
    assert torch.equal(_finish(_prepare('dpmpp_2m'), use_graph=False, pieces=[3, meta['steps'] - 3]), ms)


def test_multistep_with_per_sample_lengths_and_guidance(lib):
    """lengths [96, 77] with guidance_scale [5, 0]: each sample against its own single run at its own length.  Another batch shape runs other kernel
    forms, so bitwise equality is not promised: the gate is the 2e-2 that tests/test_sample_params_gpu.py puts on "each sample as the call with it alone"
    (both sides carry the bf16 denoiser's trajectory error).  Measured on MI355X at these shapes: 0 for both rows."""
    from ezaudio_amd.sampler import LatentSampler
    m = get_model('xs', 1)
    rows = [_row('smp_xs'), _row('smp_xs_b')]
    lens, gs, steps, nan = [96, 77], [5.0, 0.0], 20, np.float32(np.nan)

    def run(sel, lengths, guidance):
        L = max(lengths)
        text, tm = t_(np.stack([rows[i]['ctx'][0] for i in sel])), t_(np.stack([rows[i]['mask'][0] for i in sel]))
        un, um = t_(np.stack([rows[i]['ctx'][1] for i in sel])), t_(np.stack([rows[i]['mask'][1] for i in sel]))
        init = np.full((len(sel), 128, L), nan, np.float32)
        for j, (i, n) in enumerate(zip(sel, lengths)):
            init[j, :, :n] = rows[i]['init'][0, :, :n]
        smp = LatentSampler(m, _scheduler(steps))
        smp.prepare(text, tm, un, um, t_(init), None, guidance, 0.75, steps, 0.0, solver='dpmpp_2m',
                    **(dict(lengths=lengths) if len(set(lengths)) > 1 else {}))
        return _finish(smp)
    try:
        both = run([0, 1], lens, gs)
        assert torch.isfinite(both).all()
        for i in range(2):
            one = run([i], [lens[i]], gs[i] or None)
            e = rel_l2(both[i, :, :lens[i]].cpu().numpy(), one[0].cpu().numpy())
            record(f'dpmpp_2m lengths {lens} guidance {gs} row {i}: rel-L2 vs its own single run {e:.3e}')
            assert e < 2e-2, (i, e)
            assert torch.equal(both[i, :, lens[i]:], torch.zeros_like(both[i, :, lens[i]:])), 'padded latent frames must be exactly 0'
    finally:
        m.set_lengths(None)


# ---------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------
def test_set_multistep_refusals_and_off(lib):
    from ezaudio_amd import _lib
    inp, init, meta = _case()
    steps = meta['steps']
    m = get_model('xs', 1)
    ms, ddim = _runs()
    ch = _scheduler(steps).multistep_coefficients()
    arr = lambda v: (C.c_float * len(v))(*v)   # noqa: E731

    # a sampler begun with noise takes no multistep solver
    noise = torch.randn(steps, 1, 128, 96, generator=torch.Generator().manual_seed(5)).cuda()
    smp = _prepare('ddim', eta=1.0, step_noises=noise)
    noisy = _finish(smp)
    hist = torch.zeros_like(smp.latents)
    assert lib.ezdit_sampler_set_multistep(m._h, arr(ch), steps, hist.data_ptr(), C.c_void_p(smp.stream.cuda_stream)) == -1
    assert b'noise' in lib.ezdit_last_error()
    assert _rewind(lib, smp) == 0                                       # (the solver is off: any rewind is allowed)
    assert torch.equal(_finish(smp), noisy)

    smp = _prepare('dpmpp_2m', P=2)
    st = C.c_void_p(smp.stream.cuda_stream)
    two = _finish(smp)
    assert torch.equal(two[0:1], ms) and torch.equal(two[1:2], ms)
    hp = smp.x0_hist.data_ptr()
    bad = list(ch)
    bad[7] = float('nan')
    co = (_lib.EzditDdimCoef * (steps * 2))(*[_lib.EzditDdimCoef(0.9, 0.4, 0.95, 0.3, 0.1) for _ in range(steps * 2)])
    g2 = arr([3.5, 3.5])
    for what, call, rc in (('wrong n_steps', lambda: lib.ezdit_sampler_set_multistep(m._h, arr(ch[:-1]), steps - 1, hp, st), -1),
                           ('NaN c_hist', lambda: lib.ezdit_sampler_set_multistep(m._h, arr(bad), steps, hp, st), -1),
                           ('no history', lambda: lib.ezdit_sampler_set_multistep(m._h, arr(ch), steps, None, st), -1),
                           ('table with sigma', lambda: lib.ezdit_sampler_set_sample_params(m._h, g2, arr([0.0, 0.0]), co, 2, st), -1),
                           ('set_step(2)', lambda: lib.ezdit_set_step(m._h, 2, st), -3)):
        assert call() == rc, what
        assert lib.ezdit_last_error()
        assert _rewind(lib, smp) == 0                                   # ezdit_set_step(0) is fine: c_hist_0 = 0
        assert torch.equal(_finish(smp), two), what                     # the refused call left nothing behind
    # a table WITHOUT sigma is accepted next to the solver, and the solver next to such a table
    co0 = (_lib.EzditDdimCoef * (steps * 2))(*[_lib.EzditDdimCoef(*c) for c in _scheduler(steps).ddim_coefficients(0) for _ in range(2)])
    assert lib.ezdit_sampler_set_sample_params(m._h, g2, arr([0.0, 0.0]), co0, 2, st) == 0
    assert lib.ezdit_sampler_set_multistep(m._h, arr(ch), steps, hp, st) == 0
    assert _rewind(lib, smp) == 0
    assert torch.equal(_finish(smp), two)                               # a table of the call's scalars: the same bits
    assert lib.ezdit_sampler_set_sample_params(m._h, None, None, None, 0, st) == 0
    # NULL switches it off: the DDIM run, bit for bit, and rewinding anywhere is allowed again
    assert lib.ezdit_sampler_set_multistep(m._h, None, 0, None, st) == 0
    assert _rewind(lib, smp) == 0
    off = _finish(smp)
    assert torch.equal(off[0:1], ddim) and torch.equal(off[1:2], ddim)
    assert lib.ezdit_set_step(m._h, 2, st) == 0
    with pytest.raises(ValueError, match='eta=0'):
        _prepare('dpmpp_2m', eta=1.0, step_noises=noise)
    with pytest.raises(ValueError, match='solver'):
        _prepare('unipc')
