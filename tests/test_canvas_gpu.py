"""GPU tests of long-form generation: the P samples of one sampler call as overlapping windows of one canvas, blended inside the captured step
(ezdit_canvas_blend, ezdit_sampler_set_canvas, LatentSampler.prepare(canvas=) / canvas_latents(), inference(canvas_offsets=)).

The reference samples one row of the trained length.  The judges are the blend in float64 (kernel level), the numpy oracle's loop over the windows with a
float64 blend (tests/golden/sampler_canvas_xs.npz, tools/mint_canvas_golden.py), bit for bit the existing path (one window, windows without overlap, the table
switched off) and bit for bit agreement of the windows on the frames they share.  xs width throughout.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle.weights import uniform_pm1
from tests.test_sample_params_gpu import get_model, t_
from tests.test_start_gpu import _Enc, _mini_autoencoder, _scheduler, _Tok
from tests.util import load_golden, record, rel_l2, sampler_case

pytestmark = pytest.mark.gpu

CH = 128


def _arr(v):
    return (C.c_int32 * len(v))(*v)


def _holders(offs, L, T):
    cnt = np.zeros(T, np.int64)
    for o in offs:
        cnt[o:o + L] += 1
    return cnt


def _blend64(x, offs, T, ramp):
    """x [P][C][L] -> (blended float64 [P][C][L], mask [P][L] of the frames two or more windows hold)."""
    P, _, L = x.shape
    r = np.arange(L)
    w = np.minimum(np.minimum(r + 1, L - r), ramp).astype(np.float64)
    num, den = np.zeros((x.shape[1], T)), np.zeros(T)
    for p in range(P):
        num[:, offs[p]:offs[p] + L] += w * np.nan_to_num(x[p].astype(np.float64))
        den[offs[p]:offs[p] + L] += w
    cnt = _holders(offs, L, T)
    out, mask = x.astype(np.float64).copy(), np.zeros((P, L), bool)
    for p in range(P):
        sl = slice(offs[p], offs[p] + L)
        mask[p] = cnt[sl] >= 2
        out[p][:, mask[p]] = (num[:, sl] / den[sl])[:, mask[p]]
    return out, mask


def _aliases_agree(lat, offs):
    """Every frame two windows share holds the same bits in both (lat: tensor [P][C][L])."""
    L = lat.shape[-1]
    for p in range(len(offs)):
        for q in range(p + 1, len(offs)):
            d = offs[q] - offs[p]
            if d < L and not torch.equal(lat[p, :, d:].view(torch.int32), lat[q, :, :L - d].view(torch.int32)):
                return False
    return True


# ---------------------------------------------------------------------------------------------------
# 1. kernel level: ezdit_canvas_blend against float64
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L,offs,ramp', [(96, [0, 52, 104], 44), (96, [0, 30, 60], 1), (96, [0, 30, 60], 30), (150, [0, 149, 298], 1), (150, [0, 150, 300], 7)])
def test_canvas_blend_operator_against_fp64(lib, L, offs, ramp):
    """P = 3, C = 128.  [0, 30, 60]: frames 60 .. 95 have three holders; [0, 149, 298]: overlap 1 at odd, unaligned offsets (T = 448: two blocks of 256 threads
    along the canvas, as T = 450); [0, 150, 300]: no overlap.  Every element with ONE holder is NaN on entry and must come back with its bits; the shared ones
    against the float64 blend at rel-L2 5e-6, the operator gate of tests/test_gpu.py::test_cfg_ddim_step_operator_against_oracle, and bit-identical between
    their holders."""
    P, T = 3, offs[-1] + L
    g = torch.Generator().manual_seed(4000 + L + offs[1] + ramp)
    x = (torch.randn(P, CH, L, generator=g) * 1.3).numpy()
    ref, shared = _blend64(x, offs, T, ramp)
    for p in range(P):
        x[p][:, ~shared[p]] = np.nan
    xd, od = t_(x), torch.tensor(offs, dtype=torch.int32, device='cuda:0')
    assert lib.ezdit_canvas_blend(xd.data_ptr(), od.data_ptr(), P, CH, L, T, ramp, None) == 0, lib.ezdit_last_error()
    torch.cuda.synchronize()
    got = xd.cpu().numpy()
    m3 = np.broadcast_to(shared[:, None, :], got.shape)
    assert np.array_equal(got[~m3].view(np.int32), x[~m3].view(np.int32)), 'an element with one holder is neither read nor written'
    if shared.any():
        e = rel_l2(got[m3], ref[m3])
        record(f'canvas_blend operator L={L} offsets {offs} ramp {ramp}: {int(shared.sum())} shared frames, rel-L2 vs fp64 {e:.3e}')
        assert np.isfinite(got[m3]).all() and e < 5e-6, e
        assert _aliases_agree(xd, offs)
    else:
        assert np.array_equal(got.view(np.int32), x.view(np.int32))
        y = torch.randn(P, CH, L, generator=g).cuda()                     # ... and finite data without overlap: bitwise the input
        y0 = y.clone()
        assert lib.ezdit_canvas_blend(y.data_ptr(), od.data_ptr(), P, CH, L, T, ramp, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(y, y0)
    # refused calls: their code, nothing launched.  (The table is on the device and the operator does not wait for it: a gap, a first offset other than 0 and
    # a T that is not the last window's end are refused where the table is a host array, by ezdit_sampler_set_canvas -- the states test; here a T that no table
    # of P windows gives.)
    args = (xd.data_ptr(), od.data_ptr(), P, CH, L, T, ramp, None)
    for bad in ((None,) + args[1:], args[:1] + (None,) + args[2:], args[:6] + (0,) + args[7:], args[:5] + (L - 1,) + args[6:], args[:5] + (P * L + 1,) + args[6:],
                args[:2] + (0,) + args[3:]):
        assert lib.ezdit_canvas_blend(*bad) == -1 and lib.ezdit_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(xd.cpu().numpy().view(np.int32), got.view(np.int32))


# ---------------------------------------------------------------------------------------------------
# the fused loop on smp_xs_e0's inputs without gt: three windows under the fixture's one prompt, the canvas noise of tools/mint_canvas_golden.py
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case():
    cfg, sd, inp, init, noises, g, meta = sampler_case('smp_xs_e0')
    assert (meta['size'], meta['seed_w'], meta['steps'], meta['eta'], meta['L']) == ('xs', 1, 20, 0.0, 96)
    return inp, meta


def _noise(key, T):
    _, meta = _case()
    return (uniform_pm1(key, CH * T, meta['seed_in']) * np.float32(np.sqrt(3.0))).reshape(1, CH, T)


def _cut(canvas, offs, L=96):
    return np.concatenate([canvas[:, :, o:o + L] for o in offs], 0)


def _prepare(offs, canvas=None, solver='ddim', eta=0.0, **kw):
    """P = len(offs) windows of the canvas noise; canvas = (T, ramp) blends them, None leaves them independent."""
    from ezaudio_amd.sampler import LatentSampler
    inp, meta = _case()
    P, K, T = len(offs), meta['steps'], offs[-1] + 96
    m = get_model('xs', 1)
    smp = LatentSampler(m, _scheduler(K))
    text, tm = t_(inp['ctx'][0:1]).repeat(P, 1, 1), t_(inp['ctx_mask'][0:1]).repeat(P, 1)
    un, um = t_(inp['ctx'][1:2]).repeat(P, 1, 1), t_(inp['ctx_mask'][1:2]).repeat(P, 1)
    sn = None if eta <= 0 else torch.stack([t_(_cut(_noise(f'canvas.z{i}', T), offs)) for i in range(K)])
    if canvas is not None:
        kw['canvas'] = canvas if len(canvas) == 3 else (offs, canvas[0], canvas[1])
    smp.prepare(text, tm, un, um, t_(_cut(_noise('canvas.init', T), offs)), sn, meta['guidance_scale'], meta['guidance_rescale'], K, eta, solver=solver, **kw)
    return smp


def _finish(smp, use_graph=True, pieces=None):
    for n in (pieces or [None]):
        smp.run(n, use_graph=use_graph)
    lat = smp.finish().clone()
    torch.cuda.synchronize()
    return lat


A_OFFS, A = [0, 52, 104], (200, 44)


@functools.lru_cache(maxsize=None)
def _blended():
    """Case a of the golden, graph replay: computed once, shared, never modified.  (windows, canvas, launches of its step)"""
    smp = _prepare(A_OFFS, A)
    lat = _finish(smp)
    return lat, smp.canvas_latents().clone(), get_model('xs', 1).last_launch_count


@functools.lru_cache(maxsize=None)
def _independent():
    """The same windows without the table: the plain batched call of three prompts."""
    smp = _prepare(A_OFFS)
    return _finish(smp), get_model('xs', 1).last_launch_count


# ---------------------------------------------------------------------------------------------------
# 2. bitwise identities
# ---------------------------------------------------------------------------------------------------
def test_one_window_and_windows_without_overlap_are_bitwise_the_plain_call(lib):
    plain1 = _finish(_prepare([0]))
    smp = _prepare([0], (96, 5))
    assert torch.equal(_finish(smp), plain1) and torch.isfinite(plain1).all()
    assert torch.equal(smp.canvas_latents(), plain1)
    plain2 = _finish(_prepare([0, 96]))
    smp = _prepare([0, 96], (192, 7))
    assert torch.equal(_finish(smp), plain2)
    assert torch.equal(smp.canvas_latents(), torch.cat([plain2[0], plain2[1]], dim=1)[None])
    with pytest.raises(ValueError, match='canvas'):
        _prepare([0]).canvas_latents()
    inp, _ = _case()
    for bad in (dict(canvas=([0, 97], 193, 1)), dict(canvas=([0, 52], 148, 0)), dict(canvas=([0, 52], 149, 1)), dict(canvas=([0, 52, 104], 200, 1)),
                dict(canvas=([0, 52], 148, 1), lengths=[96, 90]), dict(canvas=([0, 52], 148, 1), gt=t_(inp['gt'][0:1]), gt_mask=t_(inp['gt_mask'][0:1]))):
        with pytest.raises(ValueError):
            _prepare([0, 52], **bad)


def test_graph_replay_eager_and_a_run_in_pieces_agree_bitwise_with_the_blend_on(lib):
    lat, canvas, _ = _blended()
    assert torch.isfinite(lat).all()
    assert torch.equal(_finish(_prepare(A_OFFS, A), use_graph=False), lat)
    for use_graph in (True, False):
        assert torch.equal(_finish(_prepare(A_OFFS, A), use_graph=use_graph, pieces=[1, 2, 17]), lat), use_graph
    smp = _prepare(A_OFFS, A, solver='dpmpp_2m')
    ms = _finish(smp)
    assert torch.equal(_finish(_prepare(A_OFFS, A, solver='dpmpp_2m'), use_graph=False, pieces=[1, 2, 17]), ms) and not torch.equal(ms, lat)


# ---------------------------------------------------------------------------------------------------
# 3. coupling
# ---------------------------------------------------------------------------------------------------
def test_the_windows_agree_on_their_shared_frames_after_every_step(lib):
    K = _case()[1]['steps']
    for offs, cv, eta in ((A_OFFS, A, 0.0), ([0, 30, 60], (156, 1), 1.0)):
        smp = _prepare(offs, cv, eta=eta)
        smp.stream.synchronize()
        assert _aliases_agree(smp.latents, offs)                         # (the init noise is one canvas draw)
        for n in (1, 1, K - 2):
            smp.run(n)
            smp.stream.synchronize()
            assert _aliases_agree(smp.latents, offs) and torch.isfinite(smp.latents).all(), (offs, n)
    lat, canvas, n_on = _blended()
    ind, n_off = _independent()
    assert not _aliases_agree(ind, A_OFFS)
    d = rel_l2(lat.cpu().numpy(), ind.cpu().numpy())
    record(f'canvas {A_OFFS} ramp {A[1]}: blended windows vs the same windows run independently rel-L2 {d:.3e}')
    assert d > 2e-2
    assert n_on == n_off + 1, 'the blend is one launch more; without it the step issues the launches it has always issued'
    # the assembled canvas: every window's frames, the lowest window where two hold one
    for p, o in enumerate(A_OFFS):
        assert torch.equal(canvas[0, :, o:o + 96], lat[p])


# ---------------------------------------------------------------------------------------------------
# 4. the numpy oracle's loop
# ---------------------------------------------------------------------------------------------------
def test_canvas_runs_against_the_numpy_oracle(lib):
    """Gate: the fused-loop gate 2e-2 (tests/test_gpu.py::test_sampler_matches_reference_loop_golden).  The golden's own distance to the unblended run of the
    same windows is 7.9e-2 .. 8.8e-2 (meta: unblended_rel_l2; tools/mint_canvas_golden.py on why not more)."""
    g, gmeta = load_golden('sampler_canvas_xs')
    inp, meta = _case()
    assert gmeta['base'] == 'smp_xs_e0' and gmeta['steps'] == meta['steps'] and gmeta['L'] == 96 and len(gmeta['cases']) == 3
    for c in gmeta['cases']:
        smp = _prepare(c['offsets'], (c['T'], c['ramp']), solver=c['solver'], eta=c['eta'])
        _finish(smp)
        got = smp.canvas_latents()
        assert got.shape == (1, CH, c['T'])
        e = rel_l2(got.cpu().numpy(), g['canvas_' + c['key']])
        record(f"sampler_canvas_xs case {c['key']} offsets {c['offsets']} ramp {c['ramp']} eta {c['eta']} {c['solver']}: canvas rel-L2 vs the numpy oracle loop {e:.3e} "
               f"(the unblended canvas is {c['unblended_rel_l2']:.3e} away)")
        assert torch.isfinite(got).all() and e < 2e-2, (c['key'], e)


# ---------------------------------------------------------------------------------------------------
# 5. states
# ---------------------------------------------------------------------------------------------------
def test_set_canvas_refusals_new_offsets_off_and_begin(lib):
    from ezaudio_amd import DiTControlNet, _lib
    from oracle.controlnet import CN_DEFAULT
    from oracle.weights import model_config
    inp, meta = _case()
    K = meta['steps']
    m = get_model('xs', 1)
    cfg = model_config('xs')
    # before ezdit_sampler_begin (a fresh handle)
    c = _lib.EzditConfig(cfg['embed_dim'], cfg['num_heads'], cfg['depth'], cfg['in_chans'], cfg['out_chans'], cfg['context_dim'],
                         cfg['ada_sola_rank'], float(cfg['ada_sola_alpha']), float(cfg['mlp_ratio']), 2048)
    h = C.c_void_p()
    assert lib.ezdit_create(C.byref(c), C.byref(h)) == 0
    try:
        assert lib.ezdit_sampler_set_canvas(h, _arr(A_OFFS), 3, 200, 44, None) == -3 and b'ezdit_sampler_begin' in lib.ezdit_last_error()
    finally:
        lib.ezdit_destroy(h)
    lat, _, _ = _blended()
    ind, _ = _independent()
    init = t_(_cut(_noise('canvas.init', 200), A_OFFS))

    # what the canvas does not combine with: refused with the table of that call in place, and the other way round
    on = lambda s: lib.ezdit_sampler_set_canvas(m._h, _arr(A_OFFS), 3, 200, 44, C.c_void_p(s.stream.cuda_stream))   # noqa: E731
    try:
        smp = _prepare(A_OFFS, lengths=[96, 90, 80])
        assert on(smp) == -2 and b'length' in lib.ezdit_last_error()
    finally:
        m.set_lengths(None)
    smp = _prepare(A_OFFS, init_latents=torch.zeros(3, CH, 96, device='cuda:0'), start_steps=[0, 3, 5])
    assert on(smp) == -2 and b'start' in lib.ezdit_last_error()
    smp = _prepare(A_OFFS, gt=t_(inp['gt'][0:1]), gt_mask=t_(inp['gt_mask'][0:1]))
    assert on(smp) == -2 and b'gt' in lib.ezdit_last_error()
    ccfg = dict(cfg)
    ccfg.update(CN_DEFAULT)
    cn = DiTControlNet(device='cuda:0', **ccfg)
    smp = _prepare(A_OFFS)
    st = C.c_void_p(smp.stream.cuda_stream)
    try:
        assert lib.ezdit_sampler_attach_controlnet(m._h, cn._h, 1.0) == 0
        assert on(smp) == -2 and b'ControlNet' in lib.ezdit_last_error()
    finally:
        assert lib.ezdit_sampler_attach_controlnet(m._h, None, 1.0) == 0
    assert torch.equal(_finish(smp), ind)                               # the refused calls left the plain call behind

    smp = _prepare(A_OFFS, A)
    st = C.c_void_p(smp.stream.cuda_stream)
    assert torch.equal(_finish(smp), lat)
    assert lib.ezdit_set_lengths(m._h, _arr([96, 90, 80] * 2), 6, st) == -2
    assert lib.ezdit_sampler_set_start(m._h, _arr([0, 3, 5]), 3, st) == -2
    assert lib.ezdit_sampler_attach_controlnet(m._h, cn._h, 1.0) == -2

    def rewind(start=init):
        with torch.cuda.stream(smp.stream):
            smp.latents.copy_(start)
            return lib.ezdit_set_step(m._h, 0, st)

    def in_capture():
        x = torch.zeros(8, device='cuda:0')
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=smp.stream):
            x.add_(1.0)
            rc = lib.ezdit_sampler_set_canvas(m._h, _arr([0, 40, 104]), 3, 200, 44, st)
        return rc
    sc = lambda offs, T, ramp, P=3: lib.ezdit_sampler_set_canvas(m._h, _arr(offs), P, T, ramp, st)   # noqa: E731
    for what, call, rc in (('wrong P', lambda: sc([0, 52], 148, 44, 2), -1), ('first offset', lambda: sc([1, 52, 104], 200, 44), -1),
                           ('a gap', lambda: sc([0, 97, 104], 200, 44), -1), ('not ascending', lambda: sc([0, 104, 104], 200, 44), -1),
                           ('T', lambda: sc(A_OFFS, 201, 44), -1), ('ramp 0', lambda: sc(A_OFFS, 200, 0), -1), ('capture', in_capture, -3)):
        assert call() == rc, what
        assert lib.ezdit_last_error()
        assert rewind() == 0
        assert torch.equal(_finish(smp), lat), what                     # the refused call left nothing behind
    # new offsets of the same T and ramp on the prepared call (the captured step reads the device table): the run a fresh call with them gives
    new = [0, 40, 104]
    assert sc(new, 200, 44) == 0
    init2 = t_(_cut(_noise('canvas.init', 200), new))
    assert rewind(init2) == 0
    moved = _finish(smp)
    assert torch.equal(moved, _finish(_prepare(new, A))) and _aliases_agree(moved, new) and not _aliases_agree(moved, A_OFFS)
    # off: the plain call's bits; on again, another ramp
    smp = _prepare(A_OFFS, A)
    st = C.c_void_p(smp.stream.cuda_stream)
    assert lib.ezdit_sampler_set_canvas(m._h, None, 0, 0, 1, st) == 0
    assert torch.equal(_finish(smp), ind)
    assert sc(A_OFFS, 200, 1) == 0 and rewind() == 0
    mean = _finish(smp)
    assert _aliases_agree(mean, A_OFFS) and not torch.equal(mean, lat)
    # ezdit_sampler_begin clears the table: a plain prepare on the same model behind a canvas call
    assert torch.equal(_finish(_prepare(A_OFFS)), ind)
    smp = _prepare(A_OFFS, A)
    co = _scheduler(K).ddim_coefficients(0.0)
    arr = (_lib.EzditDdimCoef * K)(*[_lib.EzditDdimCoef(*c) for c in co])
    st = C.c_void_p(smp.stream.cuda_stream)
    with torch.cuda.stream(smp.stream):
        assert lib.ezdit_sampler_begin(m._h, smp.latents.data_ptr(), 3, None, arr, K, float(meta['guidance_scale']), float(meta['guidance_rescale']),
                                       None, None, st) == 0
    assert torch.equal(_finish(smp), ind)


# ---------------------------------------------------------------------------------------------------
# 6. end to end: inference(canvas_offsets=) with the mini VAE and a stand-in text encoder
# ---------------------------------------------------------------------------------------------------
def test_inference_decodes_the_canvas_in_one_call(lib, monkeypatch):
    from ezaudio_amd import sampler as S
    from oracle.weights import model_config
    cfg = model_config('xs')
    params = {'text_encoder': {'max_length': 20}, 'model': {'out_chans': CH}, 'autoencoder': {'scale': 0.5, 'shift': -0.3, 'sr': 24000, 'latent_sr': 3000}}
    vae, m = _mini_autoencoder(), get_model('xs', 1)
    kept = []

    class Keep(S.LatentSampler):
        def __init__(self, *a):
            super().__init__(*a)
            kept.append(self)
    monkeypatch.setattr(S, 'LatentSampler', Keep)
    offs, L = [0, 52, 104], 96
    args = (vae, m, None, None, _Tok(), _Enc(cfg['context_dim']), params, _scheduler(20))
    wav = S.inference(*args, ['rain on a roof', 'a dog barking twice', 'rain on a roof'], None, L, 3.5, 0.5, 20, 1, 3, 'cuda', canvas_offsets=offs)
    assert wav.shape == (1, 1, 200 * 8) and torch.isfinite(wav).all() and wav.std() > 0
    smp = kept[-1]
    assert smp.canvas == (offs, 200, 44) and _aliases_agree(smp.latents, offs)
    assert torch.equal(wav, vae(embedding=S.scale_shift_re(smp.canvas_latents(), 0.5, -0.3)))
    one = S.inference(*args, 'rain on a roof', None, L, 3.5, 0.5, 20, 1, 3, 'cuda', canvas_offsets=[0])
    assert torch.equal(one, S.inference(*args, 'rain on a roof', None, L, 3.5, 0.5, 20, 1, 3, 'cuda')) and one.shape == (1, 1, L * 8)
