"""GPU tests of the batched ControlNet: per-prompt length, condition and conditioning scale in one fused sampler call
(ezdit_sampler_set_pair_lengths, ezdit_sampler_set_cn_scales, LatentSampler.prepare(lengths=, controlnet=, conditioning_scale=[..])).

Contract: sample i of a padded batch comes out as if it had been run ALONE at its own length, with its own control signal and scale.  The
judge is the numpy oracle run on each sample alone at its own length (oracle.controlnet.ControlNetOracle + oracle.dit.DiTOracle +
oracle.sampler.sample, pinned by the reference goldens cn_*); one reference golden (sampler_smp_cn_l) rides along in a ragged call.
What the padded region of the inputs holds (NaN here) is ignored; padded output frames are exactly 0.

Gates are the project's: REL_TOL / ABS_TOL of tests/test_gpu.py for forwards and residuals (scaled as tests/test_ragged_gpu.py::_gate),
2e-2 rel-L2 for final latents.  Size xs (D 144, depth 2, one residual), Lmax 96.

Measured on MI355X with this change: embed rows against fp64 <= 4e-8 (control 1.5e-3 on the last valid frame); residuals 3.7e-3, predictions
5.0e-3 ... 5.3e-3 rel-L2 (controls 0.26 / 0.35); final latents after 10 steps 1.4e-3 ... 1.7e-3 (scale control 7.4e-2); M = 1152 after two steps
3.3e-4 ... 3.6e-4; smp_cn_l next to its neighbour 7.0e-3.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle.controlnet import CN_DEFAULT, ControlNetOracle, make_controlnet_state_dict
from oracle.ddim import DDIMOracle
from oracle.dit import DiTOracle
from oracle.sampler import sample as oracle_sample
from oracle.weights import make_inputs, make_state_dict, model_config, uniform_pm1
from tests.util import DIFF, GOLDEN, record, rel_l2

pytestmark = pytest.mark.gpu

REL_TOL, ABS_TOL = 2e-2, 0.15   # tests/test_gpu.py
SIZE, SEED_W, LMAX, LC = 'xs', 1, 96, 20
GUIDANCE, ETA = 3.5, 1.0
# 10 steps at eta 1 are the FIRST 10 of the 50-step schedule (as tests/test_controlnet.py runs 6 of 50): a 10-step schedule has no judge at eta 1 -- the reference's
# scheduler, and oracle/ddim.py with it, returns NaN at t = 999 there (sqrt of a rounding-negative 1 - alpha_prev - sigma^2; the product clamps at 0)
STEPS, RUN = 50, 10
NAN = np.float32(np.nan)

_pairs = {}


def get_pair(size=SIZE, seed=SEED_W):
    from ezaudio_amd import DiTControlNet, MaskDiT
    key = (size, seed)
    if key not in _pairs:
        cfg = model_config(size)
        m = MaskDiT(device='cuda:0', **cfg)
        m.load_state_dict(make_state_dict(cfg, seed))
        ccfg = dict(cfg)
        ccfg.update(CN_DEFAULT)
        cn = DiTControlNet(device='cuda:0', **ccfg)
        cn.load_state_dict(make_controlnet_state_dict(cfg, CN_DEFAULT, seed))
        _pairs[key] = (m, cn)
    return _pairs[key]


@functools.lru_cache(maxsize=None)
def oracles(dtype=np.float32):
    cfg = model_config(SIZE)
    return (cfg, DiTOracle(cfg, make_state_dict(cfg, SEED_W), dtype),
            ControlNetOracle(cfg, make_controlnet_state_dict(cfg, CN_DEFAULT, SEED_W), dtype=dtype))


def t_(a, dev='cuda:0'):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _padded(a, L, fill):
    """[.., l] -> [.., L] with `fill` behind the data."""
    out = np.full(a.shape[:-1] + (L,), fill, dtype=a.dtype)
    out[..., :a.shape[-1]] = a
    return out


def _gate(pred, ref, what):
    r, a = rel_l2(pred, ref), float(np.abs(pred - ref).max())
    record(f'{what}: rel-L2 {r:.3e} max-abs {a:.3e}')
    assert np.isfinite(pred).all(), what
    assert r < REL_TOL and a < ABS_TOL * max(1.0, float(ref.std()) / 1.48), (what, r, a)


@functools.lru_cache(maxsize=None)
def sample_inputs(L, seed, steps=RUN):
    """One request: (text, negative text) context pair, initial latent, step noises and control signal, all at the sample's OWN length."""
    cfg = model_config(SIZE)
    Cc = cfg['out_chans']
    inp = make_inputs(cfg, B=2, L=L, Lc=LC, n_valid=(7, 1), seed=seed)
    s3 = np.float32(np.sqrt(3.0))
    init = (uniform_pm1('cnb.init', Cc * L, seed) * s3).reshape(1, Cc, L)
    noises = tuple((uniform_pm1(f'cnb.z{i}', Cc * L, seed) * s3).reshape(1, Cc, L) for i in range(steps))
    cond = (0.5 + 0.5 * uniform_pm1('cnb.cond', 2 * L, seed)).reshape(1, 1, 2 * L).astype(np.float32)
    return dict(ctx=inp['ctx'], mask=inp['ctx_mask'], init=init, noises=noises, cond=cond, L=L, seed=seed)


def _denoise_alone(row, scale):
    _, o, co = oracles()
    cond2 = np.concatenate([row['cond'], row['cond']], 0)

    def denoise(x, t, ctx, msk, gt, gm):
        x257, _ = o.assemble_input(x)
        res = co.forward(x257, t, ctx, msk, cond2, scale)
        return o.udit_forward(x257, t, ctx, msk, controlnet_skips=res)
    return denoise


@functools.lru_cache(maxsize=None)
def judge(L, seed, scale, upto=RUN):
    """Latent of oracle.sampler.sample on the sample ALONE at its own length and scale after the first `upto` steps of the schedule."""
    row = sample_inputs(L, seed)
    den = _denoise_alone(row, scale)
    tr = []

    class _Stop(Exception):
        pass

    def denoise(*a):   # (the loop is left once the steps asked for are done: the later timesteps are not needed)
        if len(tr) == upto:
            raise _Stop
        return den(*a)
    try:
        oracle_sample(denoise, row['ctx'][0:1], row['mask'][0:1], row['ctx'][1:2], row['mask'][1:2], row['init'], list(row['noises']),
                      guidance_scale=GUIDANCE, guidance_rescale=0.0, ddim_steps=STEPS, eta=ETA, diff_params=DIFF, trace=tr)
    except _Stop:
        pass
    assert len(tr) == upto and np.isfinite(tr[-1]).all()
    return tr[-1][0]


def _batch(rows, fill):
    Lmax = max(r['L'] for r in rows)
    text, tm = t_(np.stack([r['ctx'][0] for r in rows])), t_(np.stack([r['mask'][0] for r in rows]))
    un, um = t_(np.stack([r['ctx'][1] for r in rows])), t_(np.stack([r['mask'][1] for r in rows]))
    init = t_(np.concatenate([_padded(r['init'], Lmax, fill) for r in rows], 0))
    sn = torch.zeros(STEPS, len(rows), init.shape[1], Lmax, device='cuda:0')   # (only the first RUN steps are run)
    sn[:RUN] = torch.stack([t_(np.concatenate([_padded(r['noises'][i], Lmax, fill) for r in rows], 0)) for i in range(RUN)], 0)
    cond = t_(np.concatenate([_padded(r['cond'], 2 * Lmax, fill) for r in rows], 0))
    return text, tm, un, um, init, sn, cond


def _prepare(rows, scales, lengths=True, fill=NAN, pair=None):
    from ezaudio_amd.sampler import LatentSampler
    from ezaudio_amd.scheduler import DDIMScheduler
    m, cn = pair or get_pair()
    smp = LatentSampler(m, DDIMScheduler(**DIFF))
    text, tm, un, um, init, sn, cond = _batch(rows, fill)
    kw = dict(lengths=[r['L'] for r in rows]) if lengths else {}
    smp.prepare(text, tm, un, um, init, sn, GUIDANCE, 0.0, STEPS, ETA, controlnet=cn, condition=cond, conditioning_scale=scales, **kw)
    return smp, init, cond


def _finish(smp, rows, n=RUN, use_graph=True, check_zero=True):
    smp.run(n, use_graph=use_graph)
    lat = smp.finish().clone()
    torch.cuda.synchronize()
    if check_zero:
        for i, r in enumerate(rows):
            assert torch.equal(lat[i, :, r['L']:], torch.zeros_like(lat[i, :, r['L']:])), 'padded latent frames must be exactly 0'
    return lat


def _rewind(lib, m, smp, init):
    with torch.cuda.stream(smp.stream):
        smp.latents.copy_(init)
        assert lib.ezdit_set_step(m._h, 0, C.c_void_p(smp.stream.cuda_stream)) == 0


def _pair_lengths(lib, m, vals, stream=None):
    if vals is None:
        return lib.ezdit_sampler_set_pair_lengths(m._h, None, 0, stream)
    return lib.ezdit_sampler_set_pair_lengths(m._h, (C.c_int32 * len(vals))(*vals), len(vals), stream)


def _cn_scales(lib, m, vals, stream=None):
    if vals is None:
        return lib.ezdit_sampler_set_cn_scales(m._h, None, 0, stream)
    return lib.ezdit_sampler_set_cn_scales(m._h, (C.c_float * len(vals))(*vals), len(vals), stream)


# ---------------------------------------------------------------------------------------------------
# 1. the condition embed's own boundary, fp32 against fp64
# ---------------------------------------------------------------------------------------------------
def test_condition_embed_of_a_padded_batch_against_fp64_per_sample(lib):
    """Four samples of 96, 77, 2 and 1 latent frames (the two shortest only exist for the embed: nothing runs attention here), the padded
    region of the condition NaN.  Each sample's embed rows against ControlNetOracle(float64).embed of its OWN [1, 1, 2 len] condition: a
    value accumulates at most ~200 fp32 products of O(1) terms (3 x 65 taps in the widest layer), error ~1e-5: gate max-abs 2e-5.  Rows
    beyond len exactly 0.  Negative control: zero padded without lengths, the last valid frame of every short sample is off by more than
    5e-4 (the k = 3 layer reads conv_in's bias at frame 2 len; the CPU oracle gives 1.4e-3), every other valid frame still inside the gate."""
    cfg, _, co = oracles(np.float64)
    m, cn = get_pair()
    D = cfg['embed_dim']
    lens = [96, 77, 2, 1]
    conds = [(0.5 + 0.5 * uniform_pm1('cnb.embed', 2 * n, 40 + i)).reshape(1, 1, 2 * n).astype(np.float32) for i, n in enumerate(lens)]
    refs = [co.embed(c)[0] for c in conds]                                   # [len, D] float64
    m.bind(4, LMAX, LC, 1)
    cn.bind(4, LMAX, LC, 1)
    assert lib.ezdit_sampler_attach_controlnet(m._h, cn._h, 1.0) == 0
    try:
        assert _pair_lengths(lib, m, lens) == 0, lib.ezdit_last_error()
        cn.prepare_condition(t_(np.concatenate([_padded(c, 2 * LMAX, NAN) for c in conds], 0)))
        torch.cuda.synchronize()
        got = cn.debug_buffer('cembed', torch.float32, (4, LMAX, D)).cpu().numpy()
        assert np.isfinite(got).all()
        for b, n in enumerate(lens):
            e = float(np.abs(got[b, :n] - refs[b]).max())
            record(f'condition embed, padded batch, sample {b} (len {n}): max-abs vs fp64 {e:.3e}')
            assert e < 2e-5, (b, n, e)
            assert np.array_equal(got[b, n:], np.zeros((LMAX - n, D), np.float32)), 'embed rows beyond the length must be exactly 0'
        assert _pair_lengths(lib, m, None) == 0
        cn.prepare_condition(t_(np.concatenate([_padded(c, 2 * LMAX, np.float32(0)) for c in conds], 0)))
        torch.cuda.synchronize()
        ctl = cn.debug_buffer('cembed', torch.float32, (4, LMAX, D)).cpu().numpy()
        for b, n in enumerate(lens):
            d = np.abs(ctl[b, :n] - refs[b]).max(axis=1)
            record(f'condition embed, zero padded without lengths, sample {b} (len {n}): last valid frame off by {d[-1]:.3e}, the others by {d[:-1].max() if n > 1 else 0.0:.3e}')
            if n < LMAX:
                assert d[-1] > 5e-4, 'the fixture cannot tell a moved convolution boundary from rounding'
            else:
                assert d[-1] < 2e-5
            assert n == 1 or d[:-1].max() < 2e-5
    finally:
        assert lib.ezdit_sampler_attach_controlnet(m._h, None, 1.0) == 0


# ---------------------------------------------------------------------------------------------------
# 2. residuals and prediction of one fused step over a padded batch
# ---------------------------------------------------------------------------------------------------
def test_residuals_and_prediction_of_a_padded_batch_match_each_pair_alone(lib):
    """B = 4 = two CFG pairs of 96 and 77 frames, everything behind a sample's length NaN.  One eager fused step; the ControlNet's residual
    (residual_views, unscaled) and the backbone's prediction of every row against the oracle on that pair ALONE.  Padded prediction frames
    exactly 0; padded residual rows finite (nobody reads them).  Negative control: zero padded without lengths -- the short rows miss by
    rel-L2 > 0.1 (CPU oracle: 0.27 on the residual, 0.37 on the prediction at 77 of 96 frames)."""
    cfg, o, co = oracles()
    m, cn = get_pair()
    Cc, D = cfg['out_chans'], cfg['embed_dim']
    rows = [sample_inputs(96, 21), sample_inputs(77, 22)]
    sched = DDIMOracle(**DIFF)
    sched.set_timesteps(STEPS)
    t0 = int(sched.timesteps[0])
    ref_res, ref_pred = [], []
    for r in rows:
        x257, _ = o.assemble_input(np.concatenate([r['init'], r['init']], 0))
        res = co.forward(x257, t0, r['ctx'], r['mask'], np.concatenate([r['cond'], r['cond']], 0), 1.0)
        ref_res.append(res[0])
        ref_pred.append(o.udit_forward(x257, t0, r['ctx'], r['mask'], controlnet_skips=res))

    def step(lengths, fill):
        smp, _, _ = _prepare(rows, 1.0, lengths=lengths, fill=fill)
        smp.run(1, use_graph=False)
        smp.finish()
        torch.cuda.synchronize()
        res = cn.residual_views(4, LMAX)[0].clone().cpu().numpy()
        pred = m.debug_buffer('pred', torch.float32, (4, Cc, LMAX)).cpu().numpy()
        return res, pred

    res, pred = step(True, NAN)
    assert np.isfinite(res).all() and np.isfinite(pred).all()
    for j, r in enumerate(rows):
        n = r['L']
        for k in range(2):   # batch rows: [cond 0, cond 1, uncond 0, uncond 1]
            b = 2 * k + j
            _gate(res[b, :n], ref_res[j][k], f'padded batch row {b} (len {n}): ControlNet residual')
            _gate(pred[b, :, :n], ref_pred[j][k], f'padded batch row {b} (len {n}): backbone prediction')
            assert np.array_equal(pred[b, :, n:], np.zeros((Cc, LMAX - n), np.float32)), 'padded prediction frames must be exactly 0'
    cres, cpred = step(False, np.float32(0))
    for k in range(2):
        b = 2 * k + 1
        rr, rp = rel_l2(cres[b, :77], ref_res[1][k]), rel_l2(cpred[b, :, :77], ref_pred[1][k])
        record(f'control (zero padded, no lengths) row {b}: residual rel-L2 {rr:.3e}, prediction rel-L2 {rp:.3e}')
        assert rr > 0.1 and rp > 0.1, 'the fixtures cannot tell a padded batch from a ragged one'
        assert np.array_equal(cres[2 * k], res[2 * k]) and np.array_equal(cpred[2 * k], pred[2 * k])   # the long rows never see the short ones


# ---------------------------------------------------------------------------------------------------
# 3. sampler loop: two lengths, two scales
# ---------------------------------------------------------------------------------------------------
def test_sampler_loop_of_a_padded_batch_with_per_sample_scales(lib):
    """P = 2, 10 steps (the first 10 of the 50-step schedule, see STEPS), guidance 3.5, eta 1, lengths (96, 77), scales (1.0, 0.5): each final latent within 2e-2 of oracle.sampler.sample on
    that sample alone at its own length and scale.  Control: with both samples at scale 1.0 the short sample must MISS its scale-0.5 judge
    (one oracle forward at scale 1 against 0.5 differs by rel-L2 0.26; asserted: above the gate).  Graph replay bitwise the eager loop;
    the prompts swapped on the same model give the swapped result."""
    A, B = sample_inputs(96, 21), sample_inputs(77, 22)
    jA, jB = judge(96, 21, 1.0), judge(77, 22, 0.5)

    def check(lat, rows, judges, tag):
        for i, (r, j) in enumerate(zip(rows, judges)):
            e = rel_l2(lat[i, :, :r['L']].cpu().numpy(), j)
            record(f'batched ControlNet sampler {tag} sample {i} (len {r["L"]}): final-latent rel-L2 {e:.3e}')
            assert e < 2e-2, (tag, i, e)

    smp, _, _ = _prepare([A, B], [1.0, 0.5])
    lat = _finish(smp, [A, B])
    assert torch.isfinite(lat).all()
    check(lat, [A, B], [jA, jB], 'lengths (96, 77) scales (1.0, 0.5)')
    smp, _, _ = _prepare([A, B], [1.0, 0.5])
    eager = _finish(smp, [A, B], use_graph=False)
    assert torch.equal(lat, eager)
    smp, _, _ = _prepare([A, B], [1.0, 1.0])
    ones = _finish(smp, [A, B])
    e = rel_l2(ones[1, :, :77].cpu().numpy(), jB)
    record(f'control: short sample at scale 1.0 against its scale-0.5 judge: rel-L2 {e:.3e}')
    assert e > 2e-2, 'the fixture cannot tell one conditioning scale from another'
    assert torch.equal(ones[0], lat[0])                                     # the neighbour's scale is the neighbour's business
    smp, _, _ = _prepare([B, A], [0.5, 1.0])
    swapped = _finish(smp, [B, A])
    check(swapped, [B, A], [jB, jA], 'swapped')


# ---------------------------------------------------------------------------------------------------
# 4. above 1024 token rows: the row kernel's plain (non-affine) form
# ---------------------------------------------------------------------------------------------------
def test_padded_batch_above_1024_token_rows(lib):
    """P = 6 with CFG: B = 12, M = 1152 token rows.  Lengths cycle (96, 77, 50), scales (1.0, 0.5, 0.25); two steps of the schedule,
    each sample against the oracle alone; samples with equal inputs, length and scale bitwise equal."""
    rows = [sample_inputs(96, 21), sample_inputs(77, 22), sample_inputs(50, 23)] * 2
    scales = [1.0, 0.5, 0.25] * 2
    smp, _, _ = _prepare(rows, scales)
    lat = _finish(smp, rows, n=2)
    assert torch.isfinite(lat).all()
    for i in range(3):
        j = judge(rows[i]['L'], rows[i]['seed'], scales[i], upto=2)
        e = rel_l2(lat[i, :, :rows[i]['L']].cpu().numpy(), j)
        record(f'M = 1152 sample {i} (len {rows[i]["L"]}, scale {scales[i]}): latent after 2 steps rel-L2 {e:.3e}')
        assert e < 2e-2, (i, e)
        assert torch.equal(lat[i], lat[i + 3])


# ---------------------------------------------------------------------------------------------------
# 5. the captured step reads both tables at run time
# ---------------------------------------------------------------------------------------------------
def test_a_captured_step_reads_scales_and_pair_lengths_at_run_time(lib):
    """The SAME captured graph replayed after set_cn_scales with other values, and again after the pair call with other lengths plus
    prepare_condition, equals bit for bit a fresh call with those values -- and differs from the run before."""
    m, cn = get_pair()
    A = sample_inputs(96, 21)
    rows = [A, A]
    smp, init, cond = _prepare(rows, [1.0, 0.5], fill=np.float32(0))
    st = C.c_void_p(smp.stream.cuda_stream)
    first = _finish(smp, rows, check_zero=False)
    # other scales, same graph
    smp.set_cn_scales([0.25, 1.0])
    _rewind(lib, m, smp, init)
    second = _finish(smp, rows, check_zero=False)
    assert not torch.equal(first, second)
    fresh, _, _ = _prepare(rows, [0.25, 1.0], fill=np.float32(0))
    assert torch.equal(second, _finish(fresh, rows, check_zero=False))
    # back on the sampler whose graph was captured first: `fresh` re-prepared the pair, so set everything this run reads again
    smp2, init2, cond2 = _prepare(rows, [1.0, 0.5], fill=np.float32(0))
    base = _finish(smp2, rows, check_zero=False)
    assert torch.equal(base, first)
    st = C.c_void_p(smp2.stream.cuda_stream)
    assert _pair_lengths(lib, m, [50, 96], st) == 0, lib.ezdit_last_error()
    with torch.cuda.stream(smp2.stream):
        cn.prepare_condition(torch.cat([cond2, cond2], 0))
    _rewind(lib, m, smp2, init2)
    third = _finish(smp2, rows, check_zero=False)
    assert not torch.equal(third, base)
    assert torch.equal(third[0, :, 50:], torch.zeros_like(third[0, :, 50:])) and torch.isfinite(third).all()
    B50 = dict(A, L=50)
    fresh, _, _ = _prepare([B50, A], [1.0, 0.5], fill=np.float32(0))   # (`_batch` pads to the longest: sample 0 keeps its 96 frames of input, the table says 50)
    assert torch.equal(third, _finish(fresh, [B50, A]))


# ---------------------------------------------------------------------------------------------------
# 6. identities
# ---------------------------------------------------------------------------------------------------
def test_full_lengths_and_equal_scales_are_bitwise_the_plain_call(lib):
    m, cn = get_pair()
    A, A2 = sample_inputs(96, 21), sample_inputs(96, 24)
    rows = [A, A2]
    outs, counts = [], []
    for lengths, scales in ((False, 0.8), (True, [0.8, 0.8]), (False, [0.8, 0.8]), (False, 0.8)):
        smp, _, _ = _prepare(rows, scales, lengths=lengths)
        outs.append(_finish(smp, rows, use_graph=False))
        counts.append(m.last_launch_count)
    assert torch.isfinite(outs[0]).all() and counts[0] > 0
    for o, c in zip(outs[1:], counts[1:]):
        assert torch.equal(outs[0], o) and c == counts[0]
    # ... and below the Python layer's collapse: a TABLE of equal scales against the scalar
    smp, _, _ = _prepare(rows, 0.8, lengths=False)
    smp.set_cn_scales([0.8, 0.8])
    assert torch.equal(outs[0], _finish(smp, rows, use_graph=False)) and m.last_launch_count == counts[0]
    smp.set_cn_scales(None)


# ---------------------------------------------------------------------------------------------------
# 7. a reference golden rides along in a ragged call
# ---------------------------------------------------------------------------------------------------
def test_reference_controlnet_loop_golden_next_to_a_shorter_neighbour(lib):
    """Sample 0 = sampler_smp_cn_l (L width, 500 frames, scale 1.0, 50 steps; inputs as tests/test_controlnet.py builds them), sample 1 a
    300-frame neighbour at scale 0.5 in the same call.  Sample 0 within 2e-2 of the reference's own loop; sample 1 finite and exactly 0
    beyond frame 300 (no judge exists at this width)."""
    import ast
    import os
    from ezaudio_amd.sampler import LatentSampler
    from ezaudio_amd.scheduler import DDIMScheduler
    g = np.load(os.path.join(GOLDEN, 'sampler_smp_cn_l.npz'))
    meta = ast.literal_eval(str(g['meta']))
    cfg = model_config(meta['size'])
    pair = get_pair(meta['size'], meta['seed_w'])
    try:
        L, Lc, steps, Cc = meta['L'], meta['Lc'], meta['steps'], cfg['out_chans']
        L1 = 300
        s3 = np.float32(np.sqrt(3.0))
        inp = make_inputs(cfg, B=2, L=L, Lc=Lc, seed=meta['seed_in'])
        init = (uniform_pm1('smp.init', Cc * L, meta['seed_in']) * s3).reshape(1, Cc, L)
        noises = [(uniform_pm1(f'smp.z{i}', Cc * L, meta['seed_in']) * s3).reshape(1, Cc, L) for i in range(steps)]
        cond = (0.5 + 0.5 * uniform_pm1('smp.cond', 2 * L, meta['seed_in'])).reshape(1, 1, 2 * L).astype(np.float32)
        s1 = meta['seed_in'] + 1
        inp1 = make_inputs(cfg, B=2, L=L1, Lc=Lc, seed=s1)
        init1 = (uniform_pm1('smp.init', Cc * L1, s1) * s3).reshape(1, Cc, L1)
        noises1 = [(uniform_pm1(f'smp.z{i}', Cc * L1, s1) * s3).reshape(1, Cc, L1) for i in range(steps)]
        cond1 = (0.5 + 0.5 * uniform_pm1('smp.cond', 2 * L1, s1)).reshape(1, 1, 2 * L1).astype(np.float32)
        smp = LatentSampler(pair[0], DDIMScheduler(**DIFF))
        smp.prepare(t_(np.concatenate([inp['ctx'][0:1], inp1['ctx'][0:1]])), t_(np.concatenate([inp['ctx_mask'][0:1], inp1['ctx_mask'][0:1]])),
                    t_(np.concatenate([inp['ctx'][1:2], inp1['ctx'][1:2]])), t_(np.concatenate([inp['ctx_mask'][1:2], inp1['ctx_mask'][1:2]])),
                    t_(np.concatenate([init, _padded(init1, L, NAN)])),
                    torch.stack([t_(np.concatenate([a, _padded(b, L, NAN)])) for a, b in zip(noises, noises1)], 0),
                    meta['guidance_scale'], meta['guidance_rescale'], steps, meta['eta'], controlnet=pair[1],
                    condition=t_(np.concatenate([cond, _padded(cond1, 2 * L, NAN)])), conditioning_scale=[meta['scale'], 0.5], lengths=[L, L1])
        smp.run(steps)
        lat = smp.finish().clone()
        torch.cuda.synchronize()
        r = rel_l2(lat[0:1].cpu().numpy(), g['latent'])
        record(f'smp_cn_l next to a 300-frame neighbour at scale 0.5: final-latent rel-L2 {r:.3e}')
        assert torch.isfinite(lat).all() and r < 2e-2
        assert torch.equal(lat[1, :, L1:], torch.zeros_like(lat[1, :, L1:])) and float(lat[1, :, :L1].abs().max()) > 0
    finally:
        _pairs.pop((meta['size'], meta['seed_w']), None)   # the L-width pair is not needed again


# ---------------------------------------------------------------------------------------------------
# 8. refusals and state
# ---------------------------------------------------------------------------------------------------
def test_pair_calls_refusals_and_state(lib):
    """Return codes only, and that a refused call launches nothing and leaves the outputs alone."""
    from ezaudio_amd import DiTControlNet, MaskDiT
    cfg = model_config(SIZE)
    m = MaskDiT(device='cuda:0', **cfg)
    m.load_state_dict(make_state_dict(cfg, SEED_W))
    ccfg = dict(cfg)
    ccfg.update(CN_DEFAULT)
    cn = DiTControlNet(device='cuda:0', **ccfg)
    cn.load_state_dict(make_controlnet_state_dict(cfg, CN_DEFAULT, SEED_W))
    assert _pair_lengths(lib, m, [96, 77]) == -3 and b'workspace' in lib.ezdit_last_error()
    m.bind(4, LMAX, LC, STEPS)
    assert _pair_lengths(lib, m, [96, 77]) == -3 and b'attached' in lib.ezdit_last_error()      # no ControlNet attached
    assert _cn_scales(lib, m, [1.0, 0.5]) == -3
    assert lib.ezdit_sampler_set_pair_lengths(cn._h, None, 0, None) == -1                          # a ControlNet handle is not a backbone
    cn.bind(4, 80, LC, STEPS)
    assert lib.ezdit_sampler_attach_controlnet(m._h, cn._h, 1.0) == 0
    assert _pair_lengths(lib, m, [80, 77]) == -3 and b'bound' in lib.ezdit_last_error()           # shapes differ
    cn.bind(4, LMAX, LC, STEPS)
    for bad in ([96, 0], [97, 96], [-5], [96, 96, 96]):
        assert _pair_lengths(lib, m, bad) == -1, bad
    for bad in ([1.0, 0.5, 0.25], [1.0] * 5, [float('nan'), 1.0], [float('inf')]):
        assert _cn_scales(lib, m, bad) == -1, bad                                                  # n does not divide B, non-finite
    assert _cn_scales(lib, m, [1.0, 0.5]) == 0 and _cn_scales(lib, m, None) == 0
    # a condition with the wrong row count
    with pytest.raises(AssertionError, match='rows'):
        cn.prepare_condition(torch.zeros(2, 1, 2 * LMAX, device='cuda:0'))
    # a full call, then another table without a new prepare_condition: refused, nothing launched, latents untouched
    A, B = sample_inputs(96, 21), sample_inputs(77, 22)
    smp, init, cond = _prepare([A, B], [1.0, 0.5], pair=(m, cn))
    st = C.c_void_p(smp.stream.cuda_stream)
    smp.run(2)
    smp.finish()
    before = smp.latents.clone()
    assert _pair_lengths(lib, m, [96, 50], st) == 0
    for use_graph in (1, 0):   # the replay of the captured graph and the eager step alike
        assert lib.ezdit_sampler_run(m._h, 1, use_graph, st) == -3 and b'ezdit_prepare_condition' in lib.ezdit_last_error()
    assert lib.ezdit_controlnet_forward(cn._h, init.data_ptr(), cfg['out_chans'], 2, None, None, m._mask_embed.data_ptr(), st) == -3
    torch.cuda.synchronize()
    assert torch.equal(before, smp.latents)
    # the same table again keeps the embed; the backbone's table cleared behind the pair's back is a named mismatch
    with torch.cuda.stream(smp.stream):
        cn.prepare_condition(torch.cat([cond, cond], 0))
    assert _pair_lengths(lib, m, [96, 50], st) == 0
    assert lib.ezdit_set_lengths(m._h, None, 0, st) == 0
    assert lib.ezdit_sampler_run(m._h, 1, 1, st) == -3 and b'ControlNet only' in lib.ezdit_last_error()
    torch.cuda.synchronize()
    assert torch.equal(before, smp.latents)
    # detaching clears the ControlNet's table and leaves the backbone free for the plain call
    assert _pair_lengths(lib, m, [96, 50], st) == 0
    assert lib.ezdit_sampler_attach_controlnet(m._h, None, 1.0) == 0
    arr = (C.c_int32 * 2)(96, 77)
    assert lib.ezdit_set_lengths(m._h, arr, 2, st) == 0 and lib.ezdit_set_lengths(m._h, None, 0, st) == 0
    assert lib.ezdit_set_lengths(cn._h, arr, 2, st) == -2                                        # and that call keeps refusing a ControlNet handle
    # destroying one handle leaves the other usable
    assert lib.ezdit_sampler_attach_controlnet(m._h, cn._h, 1.0) == 0
    assert _pair_lengths(lib, m, [96, 50], st) == 0
    assert lib.ezdit_destroy(cn._h) == 0
    cn._h = C.c_void_p()                                                                         # (its __del__ must not destroy it twice)
    assert lib.ezdit_set_lengths(m._h, arr, 2, None) == 0 and lib.ezdit_set_lengths(m._h, None, 0, None) == 0
    inp = make_inputs(cfg, B=2, L=LMAX, Lc=LC, n_valid=(7, 1), seed=11)
    pred, _ = m(t_(inp['x']), torch.tensor(499), t_(inp['ctx']), context_mask=t_(inp['ctx_mask']))
    torch.cuda.synchronize()
    assert torch.isfinite(pred).all()
