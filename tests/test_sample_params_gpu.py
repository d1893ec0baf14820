"""GPU tests of per-sample sampler settings: guidance_scale, guidance_rescale and eta per prompt of one batched call
(ezdit_sampler_set_sample_params, ezdit_cfg_ddim_step_per_sample, LatentSampler.prepare with lists).

Contract: every sample comes out as the call with that sample alone and its own settings gives it -- so the judges are reference goldens
minted with different settings on the same weights (tools/mint_sampler_settings_golden.py; a sample given a neighbour's settings lands
0.3 ... 0.9 rel-L2 off its golden, the gate is 2e-2) and, bit for bit, the scalar path: the forward of a row depends on that row only at
an equal batch shape, so row i of the mixed call equals row i of the same batch run with sample i's settings for everybody.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle.weights import make_state_dict, model_config
from tests.util import DIFF, record, rel_l2, sampler_case

pytestmark = pytest.mark.gpu

NEW = ['smp_xs_b', 'smp_xs_d', 'smp_xs_n', 'smp_xs_c60']
_models = {}


def get_model(size, seed):
    from ezaudio_amd import MaskDiT
    key = (size, seed)
    if key not in _models:
        cfg = model_config(size)
        m = MaskDiT(device='cuda:0', **cfg)
        m.load_state_dict(make_state_dict(cfg, seed))
        _models[key] = m
    return _models[key]


def t_(a, dev='cuda:0'):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def _row(name):
    cfg, sd, inp, init, noises, g, meta = sampler_case(name)
    assert (meta['size'], meta['seed_w'], meta['steps'], meta['Lc'], meta['with_gt']) == ('xs', 1, 50, 20, False)
    return dict(name=name, ctx=inp['ctx'], mask=inp['ctx_mask'], init=init, noises=noises, L=meta['L'], gold=g['latent'][0],
                gs=float(meta['guidance_scale'] or 0.0), gr=float(meta['guidance_rescale']), eta=float(meta['eta']))


def _padded(a, L, fill):
    out = np.full(a.shape[:-1] + (L,), fill, dtype=a.dtype)
    out[..., :a.shape[-1]] = a
    return out


def _inputs(rows, draws=None):
    """Batch tensors of `rows`, padded to the longest with NaN; the step noise of sample i is NaN everywhere when draws[i] is False
    (a sample that draws no noise must not read its slice)."""
    Lmax, steps, nan = max(r['L'] for r in rows), 50, np.float32(np.nan)
    draws = draws or [True] * len(rows)
    text, tm = t_(np.stack([r['ctx'][0] for r in rows])), t_(np.stack([r['mask'][0] for r in rows]))
    un, um = t_(np.stack([r['ctx'][1] for r in rows])), t_(np.stack([r['mask'][1] for r in rows]))
    init = t_(np.concatenate([_padded(r['init'], Lmax, nan) for r in rows], 0))
    sn = torch.stack([t_(np.concatenate([_padded(r['noises'][i], Lmax, nan) if d else np.full((1, 128, Lmax), nan, np.float32)
                                         for r, d in zip(rows, draws)], 0)) for i in range(steps)], 0)
    return text, tm, un, um, init, sn


def _prepare(m, rows, gs, gr, eta, lengths=None, draws=None, **kw):
    from ezaudio_amd.sampler import LatentSampler
    from ezaudio_amd.scheduler import DDIMScheduler
    smp = LatentSampler(m, DDIMScheduler(**DIFF))
    text, tm, un, um, init, sn = _inputs(rows, draws)
    smp.prepare(text, tm, un, um, init, sn, gs, gr, 50, eta, **(dict(lengths=lengths) if lengths else {}), **kw)
    return smp, init


def _finish(smp, use_graph=True):
    smp.run(use_graph=use_graph)
    lat = smp.finish().clone()
    torch.cuda.synchronize()
    return lat


def _rewind(lib, m, smp, init):
    with torch.cuda.stream(smp.stream):
        smp.latents.copy_(init)
        assert lib.ezdit_set_step(m._h, 0, C.c_void_p(smp.stream.cuda_stream)) == 0


def _settings(rows):
    return [r['gs'] for r in rows], [r['gr'] for r in rows], [r['eta'] for r in rows]


# ---------------------------------------------------------------------------------------------------
# 0. the new fixtures by themselves, through the scalar path: is 2e-2 a fair gate for them?
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NEW)
def test_each_new_fixture_alone_through_the_scalar_path(lib, name):
    r = _row(name)
    m = get_model('xs', 1)
    smp, _ = _prepare(m, [r], r['gs'] or None, r['gr'], r['eta'])
    lat = _finish(smp)
    e = rel_l2(lat[0].cpu().numpy(), r['gold'])
    record(f'{name} alone, scalar path (guidance {r["gs"]}, rescale {r["gr"]}, eta {r["eta"]}): final-latent rel-L2 {e:.3e}')
    assert torch.isfinite(lat).all() and e < 2e-2, (name, e)


# ---------------------------------------------------------------------------------------------------
# 1. kernel level: ezdit_cfg_ddim_step_per_sample against float64
# ---------------------------------------------------------------------------------------------------
def _fp64_step(pred, lat, noise, params, lens):
    """oracle/sampler.py cfg_combine + rescale_noise_cfg and the DDIM update of oracle/ddim.py, per sample over its valid frames, in float64."""
    P = lat.shape[0]
    out = np.zeros(lat.shape, np.float64)
    for p in range(P):
        gs, phi, sa, sb, cx0, cdir, sigma = (float(v) for v in params[p, :7])
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
        if sigma != 0:
            prev = prev + sigma * noise[p, :, :n].astype(np.float64)
        out[p, :, :n] = prev
    return out


@pytest.mark.parametrize('L,lens', [(96, None), (150, None), (150, [150, 77, 1])])
def test_per_sample_step_operator_against_fp64(lib, L, lens):
    """P = 3, n = 128 L: 12288 elements are less than one grid sweep of 64 x 256 (some workgroups get none), 19200 one sweep and a partial
    one.  Sample 0 (5.0, 0.75, eta 1); sample 1 (2.0, no rescale, sigma 0) with NaN in its noise slice; sample 2 no guidance with NaN in its
    unconditional prediction.  With lengths the padded frames of every input hold NaN.  Gate: rel-L2 < 5e-6, that of
    tests/test_gpu.py::test_cfg_ddim_step_operator_against_oracle, here against float64 and per sample."""
    from ezaudio_amd import DDIMScheduler
    P, Cc = 3, 128
    n = Cc * L
    g = torch.Generator().manual_seed(1000 + L)
    pred = (torch.randn(2 * P, Cc, L, generator=g) * 1.3).numpy()
    lat = torch.randn(P, Cc, L, generator=g).numpy()
    noise = torch.randn(P, Cc, L, generator=g).numpy()
    sch = DDIMScheduler(**DIFF)
    sch.set_timesteps(50)
    t = int(sch.timesteps[7])
    params = np.zeros((P, 8), np.float32)
    params[0, :7] = (5.0, 0.75) + sch._coef(t, 1.0)
    params[1, :7] = (2.0, 0.0) + sch._coef(t, 0.0)
    params[2, :7] = (0.0, 0.4) + sch._coef(t, 1.0)
    assert params[1, 6] == 0.0 and params[0, 6] > 0.0
    ln = lens or [L] * P
    ref = _fp64_step(pred, lat, noise, params, ln)
    noise[1] = np.nan
    pred[P + 2] = np.nan
    for p, k in enumerate(ln):
        pred[p, :, k:] = np.nan
        pred[P + p, :, k:] = np.nan
        lat[p, :, k:] = np.nan
        noise[p, :, k:] = np.nan
    pd, ld, nd, pr = t_(pred), t_(lat), t_(noise), t_(params)
    scratch = torch.zeros(P * 256, device='cuda:0')
    kl = torch.tensor(ln, dtype=torch.int32, device='cuda:0') if lens else None
    rc = lib.ezdit_cfg_ddim_step_per_sample(pd.data_ptr(), ld.data_ptr(), nd.data_ptr(), pr.data_ptr(), kl.data_ptr() if lens else None,
                                            L, P, n, scratch.data_ptr(), None)
    assert rc == 0, lib.ezdit_last_error()
    torch.cuda.synchronize()
    got = ld.cpu().numpy()
    assert np.isfinite(got).all()
    for p, k in enumerate(ln):
        e = rel_l2(got[p, :, :k], ref[p, :, :k])
        record(f'per-sample step operator L={L} lens={lens} sample {p}: rel-L2 vs fp64 {e:.3e}')
        assert e < 5e-6, (p, e)
        assert np.array_equal(got[p, :, k:], np.zeros((Cc, L - k), np.float32)), 'padded frames must be exactly 0'
    assert lib.ezdit_cfg_ddim_step_per_sample(pd.data_ptr(), ld.data_ptr(), nd.data_ptr(), pr.data_ptr(), None, L, P, n, None, None) == -1
    assert lib.ezdit_cfg_ddim_step_per_sample(pd.data_ptr(), ld.data_ptr(), nd.data_ptr(), None, None, L, P, n, scratch.data_ptr(), None) == -1


# ---------------------------------------------------------------------------------------------------
# 2. a table of equal values is the scalar path, bit for bit
# ---------------------------------------------------------------------------------------------------
def test_a_table_of_the_calls_scalars_is_bitwise_the_scalar_path(lib):
    m = get_model('xs', 1)
    rows = [_row('smp_xs'), _row('smp_xs_b')]
    for use_graph in (True, False):
        smp, _ = _prepare(m, rows, 5.0, 0.75, 1.0)
        scalar = _finish(smp, use_graph)
        smp, _ = _prepare(m, rows, 5.0, 0.75, 1.0)
        smp.set_sample_params([5.0, 5.0], [0.75, 0.75], [1.0, 1.0])   # (prepare itself collapses equal lists to the scalar call)
        table = _finish(smp, use_graph)
        assert torch.isfinite(scalar).all() and torch.equal(scalar, table), use_graph
    smp, _ = _prepare(m, rows, [5.0, 5.0], [0.75, 0.75], [1.0, 1.0])
    assert torch.equal(_finish(smp), scalar)


# ---------------------------------------------------------------------------------------------------
# 3. each sample as if alone
# ---------------------------------------------------------------------------------------------------
def test_each_sample_of_a_mixed_call_is_the_call_with_its_settings(lib):
    m = get_model('xs', 1)
    rows = [_row(n) for n in ('smp_xs', 'smp_xs_b', 'smp_xs_d', 'smp_xs_n')]
    gs, gr, eta = _settings(rows)
    assert gs == [5.0, 2.0, 7.0, 0.0] and gr == [0.75, 0.3, 0.0, 0.0] and eta == [1.0, 0.5, 1.0, 1.0]
    smp, _ = _prepare(m, rows, gs, gr, eta)
    mixed = _finish(smp)
    assert torch.isfinite(mixed).all()
    for i, r in enumerate(rows):
        e = rel_l2(mixed[i].cpu().numpy(), r['gold'])
        record(f'mixed settings row {i} ({r["name"]}: guidance {gs[i]}, rescale {gr[i]}, eta {eta[i]}): final-latent rel-L2 {e:.3e}')
        assert e < 2e-2, (i, e)
    smp, _ = _prepare(m, rows, gs, gr, eta)
    assert torch.equal(_finish(smp, use_graph=False), mixed), 'graph replay must be bitwise the eager loop'
    for i, r in enumerate(rows):
        if gs[i] > 0:   # the scalar path over the same four inputs with sample i's settings for everybody
            smp, _ = _prepare(m, rows, gs[i], gr[i], eta[i])
        else:           # no guidance at the same batch shape (2 P rows): the table with guidance 0 for every row
            smp, _ = _prepare(m, rows, 5.0, 0.0, eta[i])
            smp.set_sample_params([0.0] * 4, [0.0] * 4, [eta[i]] * 4)
        same = _finish(smp)
        d = rel_l2(mixed[i].cpu().numpy(), same[i].cpu().numpy())
        record(f'mixed settings row {i} against the whole batch under its settings: rel-L2 {d:.3e} (bitwise {bool(torch.equal(mixed[i], same[i]))})')
        assert torch.equal(mixed[i], same[i]), i
    # negative control: sample 1 under sample 0's settings misses its golden by far (the fixtures can tell)
    smp, _ = _prepare(m, rows, gs[0], gr[0], eta[0])
    wrong = rel_l2(_finish(smp)[1].cpu().numpy(), rows[1]['gold'])
    record(f'control: smp_xs_b under smp_xs\'s settings: rel-L2 {wrong:.3e}')
    assert wrong > 0.2


# ---------------------------------------------------------------------------------------------------
# 4. settings and lengths together
# ---------------------------------------------------------------------------------------------------
def test_per_sample_settings_together_with_per_sample_lengths(lib):
    m = get_model('xs', 1)
    rows = [_row('smp_xs'), _row('smp_xs_c60')]
    gs, gr, eta = _settings(rows)
    assert eta == [1.0, 0.0] and [r['L'] for r in rows] == [96, 60]
    smp, _ = _prepare(m, rows, gs, gr, eta, lengths=[96, 60], draws=[True, False])
    lat = _finish(smp)
    assert torch.isfinite(lat).all()
    for i, r in enumerate(rows):
        e = rel_l2(lat[i, :, :r['L']].cpu().numpy(), r['gold'])
        record(f'settings + lengths row {i} ({r["name"]}, L {r["L"]}): final-latent rel-L2 {e:.3e}')
        assert e < 2e-2, (i, e)
        assert torch.equal(lat[i, :, r['L']:], torch.zeros_like(lat[i, :, r['L']:])), 'padded latent frames must be exactly 0'
    m.set_lengths(None)


# ---------------------------------------------------------------------------------------------------
# 5. the table is read at run time
# ---------------------------------------------------------------------------------------------------
def test_a_captured_step_reads_the_sample_settings_at_run_time(lib):
    m = get_model('xs', 1)
    rows = [_row('smp_xs'), _row('smp_xs_b')]
    s1 = ([5.0, 2.0], [0.75, 0.3], [1.0, 0.5])
    s2 = ([3.0, 6.0], [0.0, 0.5], [0.5, 1.0])
    smp, init = _prepare(m, rows, *s1)
    first = _finish(smp)                       # captures the step
    smp.set_sample_params(*s2)                 # other values, same graph
    _rewind(lib, m, smp, init)
    replay = _finish(smp)
    assert not torch.equal(first, replay)
    smp2, _ = _prepare(m, rows, *s2)
    assert torch.equal(_finish(smp2, use_graph=False), replay)
    # table off: the scalars ezdit_sampler_begin was given hold again (prepare passes max guidance, the first rescale, max eta)
    smp3, _ = _prepare(m, rows, *s1)
    smp3.set_sample_params()
    cleared = _finish(smp3)
    smp4, _ = _prepare(m, rows, 5.0, 0.75, 1.0)
    assert torch.equal(_finish(smp4), cleared) and torch.isfinite(cleared).all()
    assert not torch.equal(cleared, first)


# ---------------------------------------------------------------------------------------------------
# 6. with a ControlNet attached
# ---------------------------------------------------------------------------------------------------
def test_equal_sample_settings_with_a_controlnet_are_bitwise_the_scalar_run(lib):
    from ezaudio_amd import DiTControlNet
    from oracle.controlnet import CN_DEFAULT, make_controlnet_state_dict
    from oracle.weights import uniform_pm1
    cfg = model_config('xs')
    m = get_model('xs', 1)
    ccfg = dict(cfg)
    ccfg.update(CN_DEFAULT)
    cn = DiTControlNet(device='cuda:0', **ccfg)
    cn.load_state_dict(make_controlnet_state_dict(cfg, CN_DEFAULT, 1))
    rows = [_row('smp_xs'), _row('smp_xs_b')]
    cond = t_((0.5 + 0.5 * uniform_pm1('sp.cond', 2 * 2 * 96, 3)).reshape(2, 1, 192).astype(np.float32))
    kw = dict(controlnet=cn, condition=cond, conditioning_scale=0.8)
    try:
        smp, _ = _prepare(m, rows, 3.5, 0.4, 1.0, **kw)
        scalar = _finish(smp)
        smp, _ = _prepare(m, rows, 3.5, 0.4, 1.0, **kw)
        smp.set_sample_params([3.5, 3.5], [0.4, 0.4], [1.0, 1.0])
        table = _finish(smp)
        assert torch.isfinite(scalar).all() and torch.equal(scalar, table)
        smp, _ = _prepare(m, rows, [3.5, 1.5], [0.4, 0.0], [1.0, 1.0], **kw)     # and other values are accepted and matter
        other = _finish(smp)
        assert torch.equal(other[0], scalar[0]) and not torch.equal(other[1], scalar[1])
    finally:
        assert lib.ezdit_sampler_attach_controlnet(m._h, None, 1.0) == 0


# ---------------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------------
def test_set_sample_params_refusals(lib):
    from ezaudio_amd import MaskDiT, _lib
    cfg = model_config('xs')
    m = MaskDiT(device='cuda:0', **cfg)
    m.load_state_dict(make_state_dict(cfg, 1))
    rows = [_row('smp_xs'), _row('smp_xs_b')]

    def set_(gs, gr, n_coef=None, P=None, sigma=0.0, bad=None):
        P = len(gs) if P is None else P
        n_coef = 50 * len(gs) if n_coef is None else n_coef
        co = (_lib.EzditDdimCoef * n_coef)(*[_lib.EzditDdimCoef(0.9, 0.4, 0.95, 0.3, sigma) for _ in range(n_coef)])
        if bad is not None:
            co[bad].c_dir = float('nan')
        return lib.ezdit_sampler_set_sample_params(m._h, (C.c_float * len(gs))(*gs), (C.c_float * len(gr))(*gr), co, P, None)

    assert set_([5.0, 5.0], [0.0, 0.0]) == -3                                     # before ezdit_sampler_begin
    assert lib.ezdit_sampler_set_sample_params(None, None, None, None, 0, None) == -1
    smp, _ = _prepare(m, rows, 5.0, 0.75, 1.0)
    ref = _finish(smp)

    def scalar_again():
        smp, _ = _prepare(m, rows, 5.0, 0.75, 1.0)
        return smp

    for what, call in (('wrong P', lambda: set_([5.0] * 3, [0.0] * 3)),
                       ('NaN guidance', lambda: set_([5.0, float('nan')], [0.0, 0.0])),
                       ('inf rescale', lambda: set_([5.0, 5.0], [0.0, float('inf')])),
                       ('NaN coefficient', lambda: set_([5.0, 5.0], [0.0, 0.0], bad=37)),
                       ('only some arrays', lambda: lib.ezdit_sampler_set_sample_params(m._h, (C.c_float * 2)(5.0, 5.0), None, None, 2, None))):
        smp = scalar_again()
        assert call() == -1, what
        assert lib.ezdit_last_error()
        assert torch.equal(_finish(smp), ref), what                                 # the refused call left nothing behind
    # a sampler begun without CFG rows (B == P) takes no guidance, but per-sample eta
    smp, _ = _prepare(m, rows, None, 0.0, 1.0)
    plain = _finish(smp)
    smp, _ = _prepare(m, rows, None, 0.0, 1.0)
    assert set_([0.0, 2.0], [0.0, 0.0]) == -1
    assert torch.equal(_finish(smp), plain)
    smp, _ = _prepare(m, rows, None, 0.0, [1.0, 0.0], draws=[True, False])
    assert torch.isfinite(_finish(smp)).all()
    # sigma != 0 on a sampler begun without noise
    smp, _ = _prepare(m, rows, 5.0, 0.75, 0.0)
    assert set_([5.0, 5.0], [0.0, 0.0], sigma=0.1) == -1 and set_([5.0, 5.0], [0.0, 0.0], sigma=0.0) == 0
    assert lib.ezdit_sampler_set_sample_params(m._h, None, None, None, 0, None) == 0
    with pytest.raises(ValueError):
        _prepare(m, rows, [5.0, 5.0, 5.0], 0.0, 1.0)
    from ezaudio_amd.sampler import LatentSampler
    from ezaudio_amd.scheduler import DDIMScheduler
    with pytest.raises(ValueError):            # some sample has eta > 0: the step noise is needed
        LatentSampler(m, DDIMScheduler(**DIFF)).prepare(*_inputs(rows)[:5], None, [5.0, 2.0], 0.0, 50, [1.0, 0.0])
    with pytest.raises(ValueError):
        LatentSampler(m, DDIMScheduler(**DIFF)).prepare(*_inputs(rows), 5.0, 0.0, [50, 25], 1.0)
