"""Sliding-window self-attention through the model and the fused sampler (run with -m gpu on an MI355X): ezdit_set_attention_window / MaskDiT.set_attention_window.

1. forward: xs and xs64 at L 96, radius 20, against the numpy oracle with the band (tests/golden/forward_window_*.npz, tools/mint_window_golden.py) at the gate
   tests/test_gpu.py::test_forward_matches_reference_golden applies to those sizes.
2. sampler loop: the inputs of smp_xs_e0 (20 steps), DDIM and dpmpp_2m, against the oracle loop with the band (tests/golden/sampler_window_xs.npz) at the fused-loop gate
   2e-2.  The fixture's radius is 8: the one of 8 .. 32 that separates the windowed from the full-attention result most at L = 96 (2.7e-1, the meta keeps every figure).
3. identities, bitwise: a radius that covers the row is the window-off run with the same launch count; window off after on, on the same handle, gives the bits from before;
   graph replay, eager and a run in pieces agree; a mixed-length batch against each sample's single windowed call.
4. states: the setter inside a stream capture, a negative radius, a ControlNet with another radius; a refused call leaves the next run's bits unchanged."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests.test_sample_params_gpu import get_model, t_
from tests.util import DIFF, golden_case, load_golden, record, rel_l2, sampler_case

pytestmark = pytest.mark.gpu

REL_TOL, ABS_TOL = 2e-2, 0.15      # tests/test_gpu.py
LOOP_GATE = 2e-2                   # tests/test_gpu.py::test_sampler_matches_reference_loop_golden, tests/test_ragged_gpu.py


def _scheduler(steps):
    from ezaudio_amd.scheduler import DDIMScheduler
    sch = DDIMScheduler(**DIFF)
    sch.set_timesteps(steps)
    return sch


@pytest.fixture(autouse=True)
def _window_off_afterwards():
    yield
    from tests.test_sample_params_gpu import _models      # the models are shared with other test files: none leaves here with a window
    for m in _models.values():
        m.set_attention_window(None)


# ---------------------------------------------------------------------------------------------------
# 1. forward
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['xs', 'xs64'])
def test_windowed_forward_matches_the_oracle_with_the_band(lib, name):
    cfg, sd, inp, kw, g0, meta = golden_case(name)
    g, wm = load_golden('forward_window_' + name)
    assert wm['base'] == 'dit_' + name and wm['L'] == meta['L'] == 96 and wm['radius'] == 20 and not kw
    m = get_model(meta['size'], meta['seed_w'])
    fwd = lambda t: m(t_(inp['x']), torch.tensor(t), t_(inp['ctx']), context_mask=t_(inp['ctx_mask']), cls_token=None)[0].cpu().numpy()   # noqa: E731
    off = {t: fwd(t) for t in meta['timesteps']}
    n_off = m.last_launch_count
    m.set_attention_window(wm['radius'])
    for t in meta['timesteps']:
        pred, ref = fwd(t), g[f'pred_t{t}']
        assert np.isfinite(pred).all()
        r, a = rel_l2(pred, ref), float(np.abs(pred - ref).max())
        away = rel_l2(pred, g0[f'pred_t{t}'])
        record(f'forward_window_{name} t={t} radius {wm["radius"]}: rel-L2 {r:.3e} max-abs {a:.3e} vs the oracle with the band; {away:.3e} from the full-attention golden '
               f'(the oracles differ by {wm["window_vs_full"][t]:.3e})')
        assert r < REL_TOL and a < ABS_TOL * max(1.0, float(ref.std()) / 1.48), (name, t, r, a)
        assert away > 5 * REL_TOL, away                      # the window is really applied
    assert m.last_launch_count == n_off                      # the band form replaces the launch, it adds none
    m.set_attention_window(None)
    for t in meta['timesteps']:
        assert np.array_equal(fwd(t), off[t]), t             # off again: the bits from before


# ---------------------------------------------------------------------------------------------------
# 2. - 3. the fused loop
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case():
    cfg, sd, inp, init, noises, g, meta = sampler_case('smp_xs_e0')
    assert (meta['size'], meta['seed_w'], meta['steps'], meta['eta'], meta['with_gt'], meta['L']) == ('xs', 1, 20, 0.0, True, 96)
    return inp, init, meta


def _prepare(solver='ddim', radius=None, with_gt=True, lengths=None, L=None):
    """the fixture's prompt; lengths: a padded batch of its first lengths[p] frames each; L: the single call of its first L frames"""
    from ezaudio_amd.sampler import LatentSampler
    inp, init, meta = _case()
    m = get_model('xs', 1)
    m.set_attention_window(radius)
    smp = LatentSampler(m, _scheduler(meta['steps']))
    P = len(lengths) if lengths else 1
    L = max(lengths) if lengths else (L or meta['L'])
    rep = lambda a: t_(a).repeat(P, *([1] * (a.ndim - 1)))      # noqa: E731
    x0 = torch.zeros(P, init.shape[1], L, device='cuda:0')
    for p in range(P):
        n = lengths[p] if lengths else L
        x0[p, :, :n] = t_(init)[0, :, :n]
    gt = rep(inp['gt'][0:1])[..., :L] if with_gt else None
    gm = rep(inp['gt_mask'][0:1])[..., :L] if with_gt else None
    smp.prepare(rep(inp['ctx'][0:1]), rep(inp['ctx_mask'][0:1]), rep(inp['ctx'][1:2]), rep(inp['ctx_mask'][1:2]), x0, None, meta['guidance_scale'],
                meta['guidance_rescale'], meta['steps'], 0.0, gt=gt, gt_mask=gm, solver=solver, **(dict(lengths=list(lengths)) if lengths else {}))
    return smp


def _finish(smp, use_graph=True, pieces=None):
    for n in (pieces or [None]):
        smp.run(n, use_graph=use_graph)
    lat = smp.finish().clone()
    torch.cuda.synchronize()
    return lat


@functools.lru_cache(maxsize=None)
def _runs(radius):
    """(DDIM, 2M, launches per step) of the fixture's inputs at `radius`, graph replay: computed once, shared, never modified"""
    ddim = _finish(_prepare('ddim', radius))
    ms = _finish(_prepare('dpmpp_2m', radius))
    return ddim, ms, get_model('xs', 1).last_launch_count


def test_windowed_sampler_loop_against_the_oracle_loop_with_the_band(lib):
    inp, init, meta = _case()
    g, wm = load_golden('sampler_window_xs')
    assert wm['base'] == 'smp_xs_e0' and wm['steps'] == meta['steps'] and 8 <= wm['radius'] <= 32
    assert min(wm['window_vs_full_ddim'], wm['window_vs_full_dpmpp_2m']) > LOOP_GATE and wm['target_met']
    gt, gm = t_(inp['gt'][0:1]), t_(inp['gt_mask'][0:1])
    fin = lambda lat: torch.where(gm, lat, gt).cpu().numpy()      # noqa: E731  src/inference.py:104-105
    ddim, ms, _ = _runs(wm['radius'])
    full_ddim, full_ms, _ = _runs(None)
    for solver, lat, full in (('ddim', ddim, full_ddim), ('dpmpp_2m', ms, full_ms)):
        e = rel_l2(fin(lat), g['latent_' + solver])
        d = rel_l2(fin(lat), fin(full))
        record(f'sampler_window_xs {solver} radius {wm["radius"]}, {meta["steps"]} steps: final-latent rel-L2 vs the numpy oracle loop with the band {e:.3e}; windowed vs '
               f'full attention {d:.3e} (oracle: {wm["window_vs_full_" + solver]:.3e})')
        assert torch.isfinite(lat).all() and e < LOOP_GATE, (solver, e)
        assert d > LOOP_GATE, (solver, d)                        # what separates the feature from its absence


def test_a_window_that_covers_the_row_is_the_window_off_run_and_off_after_on_is_the_run_from_before(lib):
    inp, init, meta = _case()
    full_ddim, full_ms, n_full = _runs(None)
    for radius in (meta['L'] - 1, meta['L'], 4 * meta['L']):
        smp = _prepare('ddim', radius)
        assert torch.equal(_finish(smp), full_ddim), radius
        assert get_model('xs', 1).last_launch_count == n_full, radius
    win_ddim, _, n_win = _runs(8)
    assert n_win == n_full                                       # the band form: the same launches per step
    assert not torch.equal(win_ddim, full_ddim)
    # the same handle, window on, then off: the graph of the windowed step is gone and the plain kernel is back
    m = get_model('xs', 1)
    smp = _prepare('ddim', 8)
    assert torch.equal(_finish(smp), win_ddim)
    m.set_attention_window(None)
    with torch.cuda.stream(smp.stream):
        smp.latents.copy_(t_(init))
        assert lib.ezdit_set_step(m._h, 0, C.c_void_p(smp.stream.cuda_stream)) == 0
    assert torch.equal(_finish(smp), full_ddim)
    assert torch.equal(_finish(_prepare('dpmpp_2m', None)), full_ms)


def test_windowed_graph_equals_eager_and_runs_in_pieces(lib):
    inp, init, meta = _case()
    ddim, ms, _ = _runs(8)
    rest = meta['steps'] - 3
    assert torch.equal(_finish(_prepare('ddim', 8), use_graph=False), ddim)
    assert torch.equal(_finish(_prepare('ddim', 8), pieces=[1, 2, rest]), ddim)
    assert torch.equal(_finish(_prepare('ddim', 8), use_graph=False, pieces=[1, 2, rest]), ddim)
    assert torch.equal(_finish(_prepare('dpmpp_2m', 8), use_graph=False), ms)
    assert torch.equal(_finish(_prepare('dpmpp_2m', 8), pieces=[1, 2, rest]), ms)


def test_a_mixed_length_batch_under_the_window_matches_each_samples_single_call(lib):
    """[96, 80, 33] frames in one padded call, radius 8: every sample within the loop gate of the windowed call with it alone at its own length (the gate
    tests/test_ragged_gpu.py holds a padded batch to), frames beyond a sample's length exactly 0"""
    lengths = [96, 80, 33]
    lat = _finish(_prepare('ddim', 8, with_gt=False, lengths=lengths))
    for p, n in enumerate(lengths):
        single = _finish(_prepare('ddim', 8, with_gt=False, L=n))
        e = rel_l2(lat[p, :, :n].cpu().numpy(), single[0].cpu().numpy())
        record(f'windowed ragged batch {lengths} radius 8: sample {p} (L {n}) vs its single windowed call: rel-L2 {e:.3e}')
        assert e < LOOP_GATE, (p, e)
        assert bool((lat[p, :, n:] == 0).all()), p
    get_model('xs', 1).set_lengths(None)


# ---------------------------------------------------------------------------------------------------
# 4. states
# ---------------------------------------------------------------------------------------------------
def test_setter_refusals_and_the_attach_check_leave_the_next_run_unchanged(lib):
    from ezaudio_amd import DiTControlNet
    from oracle.controlnet import CN_DEFAULT
    from oracle.weights import model_config
    inp, init, meta = _case()
    win_ddim, _, _ = _runs(8)
    m = get_model('xs', 1)
    smp = _prepare('ddim', 8)
    st = C.c_void_p(smp.stream.cuda_stream)
    assert torch.equal(_finish(smp), win_ddim)

    def rewind():
        with torch.cuda.stream(smp.stream):
            smp.latents.copy_(t_(init))
            return lib.ezdit_set_step(m._h, 0, st)

    def in_capture():
        x = torch.zeros(8, device='cuda:0')
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=smp.stream):
            x.add_(1.0)
            rc = lib.ezdit_set_attention_window(m._h, 20)
        return rc
    for what, call, rc in (('negative', lambda: lib.ezdit_set_attention_window(m._h, -1), -1), ('capture', in_capture, -3)):
        assert call() == rc, what
        assert lib.ezdit_last_error()
        assert rewind() == 0
        assert torch.equal(_finish(smp), win_ddim), what         # the refused call left nothing behind: still radius 8
    assert lib.ezdit_set_attention_window(None, 4) == -1
    # a ControlNet with another radius is refused at the attach, with equal radii accepted; the handle-level setter works on a ControlNet handle
    ccfg = dict(model_config('xs'))
    ccfg.update(CN_DEFAULT)
    cn = DiTControlNet(device='cuda:0', **ccfg)
    try:
        assert lib.ezdit_sampler_attach_controlnet(m._h, cn._h, 1.0) == -1 and b'window' in lib.ezdit_last_error()      # 8 against 0
        cn.set_attention_window(20)
        assert lib.ezdit_sampler_attach_controlnet(m._h, cn._h, 1.0) == -1
        cn.set_attention_window(8)
        assert lib.ezdit_sampler_attach_controlnet(m._h, cn._h, 1.0) == 0
        assert lib.ezdit_sampler_attach_controlnet(m._h, None, 1.0) == 0
        m.set_attention_window(None)
        cn.set_attention_window(None)
        assert lib.ezdit_sampler_attach_controlnet(m._h, cn._h, 1.0) == 0                                               # both 0: today's case
    finally:
        assert lib.ezdit_sampler_attach_controlnet(m._h, None, 1.0) == 0
    assert torch.equal(_finish(_prepare('ddim', 8)), win_ddim)
