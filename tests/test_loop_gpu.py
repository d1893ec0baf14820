"""GPU tests of seamless loops: the P samples of one sampler call as windows of a RING of latent frames, blended through the wrap inside the captured step
(ezdit_canvas_blend_loop, ezdit_sampler_set_canvas_loop, LatentSampler.prepare(canvas_loop=) / canvas_latents(), inference(canvas_loop=)) and decoded as a
ring (decode_circular).

The judges are the wrap blend in float64 (kernel level), the numpy oracle's loop over the windows with a float64 wrap blend
(tests/golden/sampler_loop_xs.npz, tools/mint_loop_golden.py), bit for bit the paths that existed (the linear canvas where no window wraps, the plain batched
call with the table off), bit for bit agreement of the windows on the frames they share -- across the wrap too -- and, for the decode, the middle third of
the decode of the ring tiled three times.  xs width, the inputs of smp_xs_e0, C = 128, L = 96, 20 steps, as tests/test_canvas_gpu.py.
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


def _ix(o, L, T):
    return (o + np.arange(L)) % T


def _blend64(x, offs, T, ramp):
    """x [P][C][L] on a ring of T -> (blended float64 [P][C][L], mask [P][L] of the frames two or more windows hold)."""
    P, _, L = x.shape
    r = np.arange(L)
    w = np.minimum(np.minimum(r + 1, L - r), ramp).astype(np.float64)
    num, den, cnt = np.zeros((x.shape[1], T)), np.zeros(T), np.zeros(T, np.int64)
    for p in range(P):
        ix = _ix(offs[p], L, T)
        num[:, ix] += w * np.nan_to_num(x[p].astype(np.float64))
        den[ix] += w
        cnt[ix] += 1
    out, mask = x.astype(np.float64).copy(), np.zeros((P, L), bool)
    for p in range(P):
        ix = _ix(offs[p], L, T)
        mask[p] = cnt[ix] >= 2
        out[p][:, mask[p]] = (num[:, ix] / den[ix])[:, mask[p]]
    return out, mask


def _aliases_agree(lat, offs, T):
    """Every ring frame holds the same bits in all of its holders (lat: tensor [P][C][L]); the ring is rebuilt from the lowest holder and cut again."""
    P, _, L = lat.shape
    bits = lat.view(torch.int32)
    ring = torch.zeros(lat.shape[1], T, dtype=torch.int32, device=lat.device)
    ix = [torch.from_numpy(_ix(o, L, T)).to(lat.device) for o in offs]
    for p in reversed(range(P)):
        ring[:, ix[p]] = bits[p]
    return all(torch.equal(ring[:, ix[p]], bits[p]) for p in range(P))


# ---------------------------------------------------------------------------------------------------
# 1. kernel level: ezdit_canvas_blend_loop against float64
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L,offs,T,ramp', [(96, [0, 52, 104], 170, 30), (96, [0, 30, 60], 100, 1), (96, [0, 52, 104], 200, 44), (96, [0, 48], 96, 48),
                                           (150, [0, 149, 298], 447, 1), (150, [0, 149, 298], 448, 1)])
def test_canvas_blend_loop_operator_against_fp64(lib, L, offs, T, ramp):
    """C = 128.  [0, 52, 104] on 170: window 2 shares the ring frames 0 .. 29 with window 0 through the wrap; [0, 30, 60] on 100: window 2 wraps by 56 frames and
    88 frames have three holders, windows 1 and 2 both wrap; [0, 48] on 96 (P = 2, L = T): every frame has two holders; [0, 149, 298] on 447: a
    wrap overlap of ONE frame at odd offsets, two blocks of 256 threads along the ring.  T = 200 and T = 448: the last window ends at T, nothing wraps, and the
    result must be ezdit_canvas_blend's bit for bit.  Every element with ONE holder is NaN on entry and must come back with its bits; the shared ones against
    the float64 blend at rel-L2 5e-6, the operator gate of tests/test_gpu.py::test_cfg_ddim_step_operator_against_oracle, and bit-identical between holders."""
    P = len(offs)
    g = torch.Generator().manual_seed(5000 + L + T + ramp)
    x = (torch.randn(P, CH, L, generator=g) * 1.3).numpy()
    ref, shared = _blend64(x, offs, T, ramp)
    assert shared.any()
    if T == 96:
        assert shared.all()
    if T == 100:
        assert (sum(np.bincount(_ix(o, L, T), minlength=T) for o in offs) == 3).sum() == 88
    for p in range(P):
        x[p][:, ~shared[p]] = np.nan
    xd, od = t_(x), torch.tensor(offs, dtype=torch.int32, device='cuda:0')
    assert lib.ezdit_canvas_blend_loop(xd.data_ptr(), od.data_ptr(), P, CH, L, T, ramp, None) == 0, lib.ezdit_last_error()
    torch.cuda.synchronize()
    got = xd.cpu().numpy()
    m3 = np.broadcast_to(shared[:, None, :], got.shape)
    assert np.array_equal(got[~m3].view(np.int32), x[~m3].view(np.int32)), 'an element with one holder is neither read nor written'
    e = rel_l2(got[m3], ref[m3])
    record(f'canvas_blend_loop operator L={L} offsets {offs} T {T} ramp {ramp}: {int(shared.sum())} shared frames, rel-L2 vs fp64 {e:.3e}')
    assert np.isfinite(got[m3]).all() and e < 5e-6, e
    assert _aliases_agree(xd, offs, T)
    if offs[-1] + L == T:                                                    # no window wraps: the linear operator, bit for bit
        yd = t_(x)
        assert lib.ezdit_canvas_blend(yd.data_ptr(), od.data_ptr(), P, CH, L, T, ramp, None) == 0, lib.ezdit_last_error()
        torch.cuda.synchronize()
        assert torch.equal(yd.view(torch.int32), xd.view(torch.int32))
    # refused argument sets: -1, nothing launched (null pointers, P / C / L < 1, ramp < 1, L > T, T > P L)
    args = (xd.data_ptr(), od.data_ptr(), P, CH, L, T, ramp, None)
    for bad in ((None,) + args[1:], args[:1] + (None,) + args[2:], args[:2] + (0,) + args[3:], args[:3] + (0,) + args[4:], args[:4] + (0,) + args[5:],
                args[:6] + (0,) + args[7:], args[:5] + (L - 1,) + args[6:], args[:5] + (P * L + 1,) + args[6:]):
        assert lib.ezdit_canvas_blend_loop(*bad) == -1 and lib.ezdit_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(xd.cpu().numpy().view(np.int32), got.view(np.int32))


# ---------------------------------------------------------------------------------------------------
# the fused loop on smp_xs_e0's inputs without gt: three windows under the fixture's one prompt, the ring noise of tools/mint_loop_golden.py
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case():
    cfg, sd, inp, init, noises, g, meta = sampler_case('smp_xs_e0')
    assert (meta['size'], meta['seed_w'], meta['steps'], meta['eta'], meta['L']) == ('xs', 1, 20, 0.0, 96)
    return inp, meta


def _noise(key, T):
    _, meta = _case()
    return (uniform_pm1(key, CH * T, meta['seed_in']) * np.float32(np.sqrt(3.0))).reshape(1, CH, T)


def _cut(ring, offs, L=96):
    T = ring.shape[-1]
    return np.concatenate([ring[:, :, _ix(o, L, T)] for o in offs], 0)


def _prepare(offs, T, loop=None, line=None, solver='ddim', eta=0.0, **kw):
    """P = len(offs) windows cut from the ring noise of T frames; loop = ramp blends them on the ring, line = (T_line, ramp) as a linear canvas, neither leaves
    them independent."""
    from ezaudio_amd.sampler import LatentSampler
    inp, meta = _case()
    P, K = len(offs), meta['steps']
    m = get_model('xs', 1)
    smp = LatentSampler(m, _scheduler(K))
    text, tm = t_(inp['ctx'][0:1]).repeat(P, 1, 1), t_(inp['ctx_mask'][0:1]).repeat(P, 1)
    un, um = t_(inp['ctx'][1:2]).repeat(P, 1, 1), t_(inp['ctx_mask'][1:2]).repeat(P, 1)
    sn = None if eta <= 0 else torch.stack([t_(_cut(_noise(f'loop.z{i}', T), offs)) for i in range(K)])
    if loop is not None:
        kw['canvas_loop'] = (offs, T, loop)
    if line is not None:
        kw['canvas'] = (offs, line[0], line[1])
    smp.prepare(text, tm, un, um, t_(_cut(_noise('loop.init', T), offs)), sn, meta['guidance_scale'], meta['guidance_rescale'], K, eta, solver=solver, **kw)
    return smp


def _finish(smp, use_graph=True, pieces=None):
    for n in (pieces or [None]):
        smp.run(n, use_graph=use_graph)
    lat = smp.finish().clone()
    torch.cuda.synchronize()
    return lat


OFFS, T_RING, RAMP = [0, 52, 104], 170, 30          # the golden's ring: window 2 ends at 200 = 170 + 30
WRAP = 30


@functools.lru_cache(maxsize=None)
def _looped():
    """Case a of the golden, graph replay: computed once, shared, never modified.  (windows, ring, launches of its step)"""
    smp = _prepare(OFFS, T_RING, loop=RAMP)
    lat = _finish(smp)
    return lat, smp.canvas_latents().clone(), get_model('xs', 1).last_launch_count


@functools.lru_cache(maxsize=None)
def _independent():
    """The same windows without the table: the plain batched call of three prompts."""
    smp = _prepare(OFFS, T_RING)
    return _finish(smp), get_model('xs', 1).last_launch_count


# ---------------------------------------------------------------------------------------------------
# 2. bitwise identities
# ---------------------------------------------------------------------------------------------------
def test_a_loop_table_without_wrap_is_the_linear_canvas_and_off_is_the_plain_call(lib):
    line = _finish(_prepare(OFFS, 200, line=(200, 44)))
    smp = _prepare(OFFS, 200, loop=44)
    assert torch.equal(_finish(smp), line) and torch.isfinite(line).all()
    assert smp.loop
    ring = smp.canvas_latents()
    for p, o in enumerate(OFFS):
        assert torch.equal(ring[0, :, o:o + 96], line[p])
    # the table off: bitwise the plain batched call of the same windows
    ind, _ = _independent()
    smp = _prepare(OFFS, T_RING, loop=RAMP)
    smp.set_canvas_loop()
    assert torch.equal(_finish(smp), ind)
    smp = _prepare(OFFS, T_RING, loop=RAMP)
    smp.set_canvas()                                                         # (NULL on either setter clears the one table)
    assert torch.equal(_finish(smp), ind)
    inp, _ = _case()
    for bad in (dict(canvas_loop=([0, 52, 104], 201, 1)), dict(canvas_loop=([0, 52, 104], 95, 1)), dict(canvas_loop=([0, 52, 104], 170, 0)),
                dict(canvas_loop=([0, 52], 148, 1)), dict(canvas_loop=(OFFS, 170, 1), canvas=(OFFS, 200, 1)), dict(canvas_loop=(OFFS, 170, 1), lengths=[96, 90, 80]),
                dict(canvas_loop=(OFFS, 170, 1), gt=t_(inp['gt'][0:1]), gt_mask=t_(inp['gt_mask'][0:1]))):
        with pytest.raises(ValueError):
            _prepare(OFFS, T_RING, **bad)


def test_graph_replay_eager_and_a_run_in_pieces_agree_bitwise_with_the_loop_on(lib):
    lat, ring, _ = _looped()
    assert torch.isfinite(lat).all()
    assert torch.equal(_finish(_prepare(OFFS, T_RING, loop=RAMP), use_graph=False), lat)
    for use_graph in (True, False):
        assert torch.equal(_finish(_prepare(OFFS, T_RING, loop=RAMP), use_graph=use_graph, pieces=[1, 2, 17]), lat), use_graph
    ms = _finish(_prepare(OFFS, T_RING, loop=RAMP, solver='dpmpp_2m'))
    assert torch.equal(_finish(_prepare(OFFS, T_RING, loop=RAMP, solver='dpmpp_2m'), use_graph=False), ms) and not torch.equal(ms, lat)
    for use_graph in (True, False):
        assert torch.equal(_finish(_prepare(OFFS, T_RING, loop=RAMP, solver='dpmpp_2m'), use_graph=use_graph, pieces=[1, 2, 17]), ms), use_graph
    assert _aliases_agree(ms, OFFS, T_RING)


# ---------------------------------------------------------------------------------------------------
# 3. coupling
# ---------------------------------------------------------------------------------------------------
def test_the_windows_agree_through_the_wrap_after_every_step(lib):
    K = _case()[1]['steps']
    for offs, T, ramp, eta in ((OFFS, T_RING, RAMP, 0.0), ([0, 30, 60], 100, 1, 1.0)):
        smp = _prepare(offs, T, loop=ramp, eta=eta)
        smp.stream.synchronize()
        assert _aliases_agree(smp.latents, offs, T)                          # (the init noise is one ring draw)
        for _ in range(K):
            smp.run(1)
            smp.stream.synchronize()
            assert _aliases_agree(smp.latents, offs, T) and torch.isfinite(smp.latents).all(), (offs, eta)
    lat, ring, n_on = _looped()
    ind, n_off = _independent()
    assert torch.equal(lat[2, :, 96 - WRAP:], lat[0, :, :WRAP])             # the last window runs into the first
    assert not _aliases_agree(ind, OFFS, T_RING)
    assert n_on == n_off + 1, 'the wrap blend is one launch more; without it the step issues the launches it has always issued'
    # the linear canvas of the same offsets (and the same windows) never couples the frames shared through the wrap
    smp = _prepare(OFFS, T_RING, line=(200, RAMP))
    line = _finish(smp)
    assert get_model('xs', 1).last_launch_count == n_on                      # the same count as the linear canvas
    assert torch.equal(line[0, :, 52:], line[1, :, :44]) and not torch.equal(line[2, :, 96 - WRAP:], line[0, :, :WRAP])
    d = rel_l2(lat[0, :, :WRAP].cpu().numpy(), line[0, :, :WRAP].cpu().numpy())
    record(f'loop {OFFS} on {T_RING} ramp {RAMP}: the {WRAP} wrap frames of window 0 vs the linear canvas of the same offsets rel-L2 {d:.3e}; '
           f'vs the independent windows {rel_l2(lat.cpu().numpy(), ind.cpu().numpy()):.3e}')
    assert d > 0
    # the assembled ring: every window's frames, cut at window 0's first frame
    assert ring.shape == (1, CH, T_RING)
    for p, o in enumerate(OFFS):
        assert torch.equal(ring[0][:, torch.from_numpy(_ix(o, 96, T_RING)).cuda()], lat[p])


# ---------------------------------------------------------------------------------------------------
# 4. the numpy oracle's loop
# ---------------------------------------------------------------------------------------------------
def test_loop_runs_against_the_numpy_oracle(lib):
    """Gate: the fused-loop gate 2e-2 (tests/test_gpu.py::test_sampler_matches_reference_loop_golden), on the whole ring and on the frames shared through the
    wrap alone.  The golden is 1.2e-1 .. 1.3e-1 from the unblended run on those frames (meta: unblended_rel_l2_wrap; tools/mint_loop_golden.py refuses to write
    one below 4e-2)."""
    g, gmeta = load_golden('sampler_loop_xs')
    inp, meta = _case()
    assert gmeta['base'] == 'smp_xs_e0' and gmeta['steps'] == meta['steps'] and gmeta['L'] == 96 and len(gmeta['cases']) == 3
    assert (gmeta['offsets'], gmeta['T'], gmeta['ramp'], gmeta['wrap_frames']) == (OFFS, T_RING, RAMP, WRAP)
    assert [(c['eta'], c['solver']) for c in gmeta['cases']] == [(0.0, 'ddim'), (1.0, 'ddim'), (0.0, 'dpmpp_2m')]
    for c in gmeta['cases']:
        assert c['unblended_rel_l2_wrap'] >= 4e-2
        smp = _prepare(OFFS, T_RING, loop=RAMP, solver=c['solver'], eta=c['eta'])
        _finish(smp)
        got = smp.canvas_latents()
        assert got.shape == (1, CH, T_RING)
        want = g['loop_' + c['key']]
        e, ew = rel_l2(got.cpu().numpy(), want), rel_l2(got.cpu().numpy()[..., :WRAP], want[..., :WRAP])
        record(f"sampler_loop_xs case {c['key']} eta {c['eta']} {c['solver']}: ring rel-L2 vs the numpy oracle loop {e:.3e}, on the {WRAP} wrap frames {ew:.3e} "
               f"(the unblended run is {c['unblended_rel_l2_wrap']:.3e} away there)")
        assert torch.isfinite(got).all() and e < 2e-2 and ew < 2e-2, (c['key'], e, ew)


# ---------------------------------------------------------------------------------------------------
# 5. states
# ---------------------------------------------------------------------------------------------------
def test_set_canvas_loop_refusals_replacement_and_begin(lib):
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
        assert lib.ezdit_sampler_set_canvas_loop(h, _arr(OFFS), 3, T_RING, RAMP, None) == -3 and b'ezdit_sampler_begin' in lib.ezdit_last_error()
    finally:
        lib.ezdit_destroy(h)
    lat, _, _ = _looped()
    ind, _ = _independent()
    init = t_(_cut(_noise('loop.init', T_RING), OFFS))
    ws = lib.ezdit_workspace_bytes(m._h, 6, 96, 20, K)

    # what the loop does not combine with: refused with the table of that call in place, and the other way round
    on = lambda s: lib.ezdit_sampler_set_canvas_loop(m._h, _arr(OFFS), 3, T_RING, RAMP, C.c_void_p(s.stream.cuda_stream))   # noqa: E731
    try:
        smp = _prepare(OFFS, T_RING, lengths=[96, 90, 80])
        assert on(smp) == -2 and b'length' in lib.ezdit_last_error()
    finally:
        m.set_lengths(None)
    smp = _prepare(OFFS, T_RING, init_latents=torch.zeros(3, CH, 96, device='cuda:0'), start_steps=[0, 3, 5])
    assert on(smp) == -2 and b'start' in lib.ezdit_last_error()
    smp = _prepare(OFFS, T_RING, gt=t_(inp['gt'][0:1]), gt_mask=t_(inp['gt_mask'][0:1]))
    assert on(smp) == -2 and b'gt' in lib.ezdit_last_error()
    ccfg = dict(cfg)
    ccfg.update(CN_DEFAULT)
    cn = DiTControlNet(device='cuda:0', **ccfg)
    smp = _prepare(OFFS, T_RING)
    st = C.c_void_p(smp.stream.cuda_stream)
    try:
        assert lib.ezdit_sampler_attach_controlnet(m._h, cn._h, 1.0) == 0
        assert on(smp) == -2 and b'ControlNet' in lib.ezdit_last_error()
    finally:
        assert lib.ezdit_sampler_attach_controlnet(m._h, None, 1.0) == 0
    assert torch.equal(_finish(smp), ind)                                   # the refused calls left the plain call behind

    smp = _prepare(OFFS, T_RING, loop=RAMP)
    st = C.c_void_p(smp.stream.cuda_stream)
    assert torch.equal(_finish(smp), lat)
    assert lib.ezdit_set_lengths(m._h, _arr([96, 90, 80] * 2), 6, st) == -2
    assert lib.ezdit_sampler_set_start(m._h, _arr([0, 3, 5]), 3, st) == -2
    assert lib.ezdit_sampler_attach_controlnet(m._h, cn._h, 1.0) == -2
    assert lib.ezdit_workspace_bytes(m._h, 6, 96, 20, K) == ws

    def rewind(start=init):
        with torch.cuda.stream(smp.stream):
            smp.latents.copy_(start)
            return lib.ezdit_set_step(m._h, 0, st)

    def in_capture():
        x = torch.zeros(8, device='cuda:0')
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=smp.stream):
            x.add_(1.0)
            rc = lib.ezdit_sampler_set_canvas_loop(m._h, _arr([0, 40, 104]), 3, T_RING, RAMP, st)
        return rc
    sl = lambda offs, T, ramp, P=3: lib.ezdit_sampler_set_canvas_loop(m._h, _arr(offs), P, T, ramp, st)   # noqa: E731
    for what, call, rc in (('wrong P', lambda: sl([0, 52], 148, RAMP, 2), -1), ('first offset', lambda: sl([1, 52, 104], T_RING, RAMP), -1),
                           ('not ascending', lambda: sl([0, 104, 104], T_RING, RAMP), -1), ('a gap', lambda: sl([0, 97, 104], T_RING, RAMP), -1),
                           ('last offset at T', lambda: sl(OFFS, 104, RAMP), -1), ('a gap at the wrap', lambda: sl(OFFS, 201, RAMP), -1),
                           ('L > T', lambda: sl([0, 40, 80], 95, RAMP), -1), ('ramp 0', lambda: sl(OFFS, T_RING, 0), -1), ('capture', in_capture, -3)):
        assert call() == rc, what
        assert lib.ezdit_last_error()
        assert rewind() == 0
        assert torch.equal(_finish(smp), lat), what                         # the refused call left nothing behind
    # the two setters replace each other: the line over the ring on the prepared call is the run a fresh linear call of these windows gives, and back
    assert lib.ezdit_sampler_set_canvas(m._h, _arr(OFFS), 3, 200, RAMP, st) == 0 and rewind() == 0
    line = _finish(smp)
    assert not torch.equal(line, lat) and torch.equal(line, _finish(_prepare(OFFS, T_RING, line=(200, RAMP))))
    smp = _prepare(OFFS, T_RING, line=(200, RAMP))
    st = C.c_void_p(smp.stream.cuda_stream)
    assert sl(OFFS, T_RING, RAMP) == 0
    assert torch.equal(_finish(smp), lat)
    # new offsets of the same T and ramp on the prepared call (the captured step reads the device table): the run a fresh call with them gives
    new = [0, 40, 104]
    assert sl(new, T_RING, RAMP) == 0
    assert rewind(t_(_cut(_noise('loop.init', T_RING), new))) == 0
    moved = _finish(smp)
    assert torch.equal(moved, _finish(_prepare(new, T_RING, loop=RAMP))) and _aliases_agree(moved, new, T_RING) and not _aliases_agree(moved, OFFS, T_RING)
    # NULL on the OTHER setter clears the ring; ezdit_sampler_begin clears it
    smp = _prepare(OFFS, T_RING, loop=RAMP)
    st = C.c_void_p(smp.stream.cuda_stream)
    assert lib.ezdit_sampler_set_canvas(m._h, None, 0, 0, 1, st) == 0
    assert torch.equal(_finish(smp), ind)
    assert torch.equal(_finish(_prepare(OFFS, T_RING)), ind)                # a plain prepare on the same model behind a loop call
    smp = _prepare(OFFS, T_RING, loop=RAMP)
    co = _scheduler(K).ddim_coefficients(0.0)
    arr = (_lib.EzditDdimCoef * K)(*[_lib.EzditDdimCoef(*c) for c in co])
    st = C.c_void_p(smp.stream.cuda_stream)
    with torch.cuda.stream(smp.stream):
        assert lib.ezdit_sampler_begin(m._h, smp.latents.data_ptr(), 3, None, arr, K, float(meta['guidance_scale']), float(meta['guidance_rescale']),
                                       None, None, st) == 0
    assert torch.equal(_finish(smp), ind)


# ---------------------------------------------------------------------------------------------------
# 6. end to end: inference(canvas_loop=) with the mini VAE and a stand-in text encoder
# ---------------------------------------------------------------------------------------------------
def test_inference_decodes_the_ring_as_a_ring(lib, monkeypatch):
    """decode_circular on the GPU decoder against the middle third of the decode of the ring tiled three times.  Bitwise: a GEMM row depends on its own
    operand rows only, so a frame decodes to the same bits wherever it lies in the stacked sequence once its receptive field is real data."""
    from ezaudio_amd import sampler as S
    from oracle.weights import model_config
    cfg = model_config('xs')
    params = {'text_encoder': {'max_length': 20}, 'model': {'out_chans': CH}, 'autoencoder': {'scale': 0.5, 'shift': -0.3, 'sr': 24000, 'latent_sr': 3000}}
    vae, m = _mini_autoencoder(), get_model('xs', 1)
    ctx = vae.decoder_context_frames()
    assert ctx == 19
    kept = []

    class Keep(S.LatentSampler):
        def __init__(self, *a):
            super().__init__(*a)
            kept.append(self)
    monkeypatch.setattr(S, 'LatentSampler', Keep)
    L = 96
    args = (vae, m, None, None, _Tok(), _Enc(cfg['context_dim']), params, _scheduler(20))
    wav = S.inference(*args, ['rain on a roof', 'a dog barking twice', 'rain on a roof'], None, L, 3.5, 0.5, 20, 1, 3, 'cuda', canvas_offsets=OFFS, canvas_loop=T_RING)
    assert wav.shape == (1, 1, T_RING * 8) and torch.isfinite(wav).all() and wav.std() > 0
    smp = kept[-1]
    assert smp.canvas == (OFFS, T_RING, RAMP) and smp.loop and _aliases_agree(smp.latents, OFFS, T_RING)      # the default ramp: the smallest cyclic overlap
    z = S.scale_shift_re(smp.canvas_latents(), 0.5, -0.3)
    third = vae(embedding=z.repeat(1, 1, 3))[..., T_RING * 8:2 * T_RING * 8]
    e = rel_l2(wav.cpu().numpy(), third.cpu().numpy())
    record(f'decode_circular, mini VAE, T {T_RING}, context {ctx}: rel-L2 vs the middle third of the tiled decode {e:.3e} (bitwise: {torch.equal(wav, third)})')
    assert torch.equal(wav, third)
    assert torch.equal(S.decode_circular(vae, z), wav) and torch.equal(S.decode_circular(vae, z, 2 * ctx), wav)          # twice the context agrees
    for k in (1, 37):                                                        # rolling the latents by k frames rolls the waveform by 8 k samples
        assert torch.equal(S.decode_circular(vae, torch.roll(z, k, dims=2)), torch.roll(wav, 8 * k, dims=2)), k
    zero_halo = vae(embedding=z)
    assert not torch.equal(zero_halo[..., :8], wav[..., :8]) and torch.equal(zero_halo[..., ctx * 8:-ctx * 8], wav[..., ctx * 8:-ctx * 8])
    # a ring that fits one window runs as two windows
    for T in (96, 50):
        offs, win = S.loop_windows(T, L, 24)
        assert offs == [0, T // 2] and win == T
        one = S.inference(*args, 'rain on a roof', None, win, 3.5, 0.5, 20, 1, 3, 'cuda', canvas_offsets=offs, canvas_loop=T)
        smp = kept[-1]
        assert one.shape == (1, 1, T * 8) and torch.isfinite(one).all() and smp.P == 2 and smp.canvas == (offs, T, T // 2)
        assert _aliases_agree(smp.latents, offs, T) and torch.equal(smp.latents[0], torch.roll(smp.latents[1], T // 2, dims=1))
