"""GPU tests of mixed-length batches (ezdit_set_lengths, MaskDiT.forward(x_lens=), LatentSampler.prepare(lengths=)).

Contract: sample i of a padded batch comes out as if it had been run ALONE at its own length -- which is all the reference ever does --
so the judges are the reference goldens minted at those lengths (they come in pairs of different length with the same weights, timestep
and sampler settings) and, where no golden pair exists, the numpy oracle run on each row alone.  Output frames beyond a sample's length
are exactly 0; what the padded region of the inputs holds (NaN here) is ignored.

Gates are the project's: REL_TOL / ABS_TOL of tests/test_gpu.py for forwards, 2e-2 rel-L2 for final latents.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.weights import make_inputs, make_state_dict, model_config
from tests.util import DIFF, golden_case, load_golden, record, rel_l2, sampler_case

pytestmark = pytest.mark.gpu

REL_TOL, ABS_TOL = 2e-2, 0.15   # tests/test_gpu.py

_models = {}


def get_model(size, seed):
    from ezaudio_amd import MaskDiT
    key = (size, seed)
    if key not in _models:
        if len(_models) >= 2:
            _models.pop(next(iter(_models)))
        cfg = model_config(size)
        m = MaskDiT(device='cuda:0', **cfg)
        m.load_state_dict(make_state_dict(cfg, seed))
        _models[key] = m
    return _models[key]


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


# ---------------------------------------------------------------------------------------------------
# 1. forward at three widths: a long plain golden and a short editing golden in ONE call
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('long,short', [('xs', 'xs_edit'), ('s', 's_edit'), ('l', 'l_edit')])
def test_forward_of_a_padded_batch_matches_each_rows_own_golden(lib, long, short):
    """B = 4: rows 0, 1 = the plain golden at Lmax (expressed as gt_mask all ones: the reference's no-gt input), rows 2, 3 = the editing
    golden at Lshort, padded to Lmax with NaN in x, gt (and gt_mask False = 'take gt' there).  Each row's valid frames against its own
    golden; padded output frames exactly 0; the last valid frame of the short rows -- what the zero conv boundary decides -- inside the
    elementwise gate by itself.  Negative control: the same batch zero-padded WITHOUT lengths must miss the short rows' golden (the numpy
    oracle on the zero-padded, unmasked input misses by rel-L2 0.37 (xs) / 0.61 (s), max-abs 2.6 / 4.3): rel-L2 > 0.1."""
    _, _, inA, _, gA, mA = golden_case(long)
    _, _, inB, kwB, gB, mB = golden_case(short)
    assert mA['seed_w'] == mB['seed_w'] and mA['Lc'] == mB['Lc'] and mA['size'] == mB['size'] and mB['with_gt'] and not mA['with_gt']
    m = get_model(mA['size'], mA['seed_w'])
    Lmax, Ls = mA['L'], mB['L']
    C_ = inA['x'].shape[1]
    refA, refB = gA['pred_t499'], gB['pred_t499']
    ctx, cm = np.concatenate([inA['ctx'], inB['ctx']]), np.concatenate([inA['ctx_mask'], inB['ctx_mask']])

    def run(fill, lens):
        x = np.concatenate([inA['x'], _padded(inB['x'], Lmax, np.float32(fill))])
        gt = np.concatenate([np.zeros_like(inA['x']), _padded(inB['gt'], Lmax, np.float32(fill))])
        gm = np.concatenate([np.ones((2, C_, Lmax), dtype=bool), _padded(inB['gt_mask'], Lmax, False)])
        pred, _ = m(t_(x), torch.tensor(499), t_(ctx), context_mask=t_(cm), gt=t_(gt), mae_mask_infer=t_(gm), **lens)
        torch.cuda.synchronize()
        return pred.cpu().numpy()

    pred = run(np.nan, dict(x_lens=[Lmax, Lmax, Ls, Ls]))
    assert pred.shape == (4, C_, Lmax)
    for i in range(2):
        _gate(pred[i], refA[i], f'{long}+{short} row {i} (L {Lmax})')
        _gate(pred[2 + i, :, :Ls], refB[i], f'{long}+{short} row {2 + i} (L {Ls} of {Lmax})')
        assert np.array_equal(pred[2 + i, :, Ls:], np.zeros((C_, Lmax - Ls), np.float32)), 'padded output frames must be exactly 0'
        e = float(np.abs(pred[2 + i, :, Ls - 1] - refB[i, :, Ls - 1]).max())
        record(f'{long}+{short} row {2 + i}: last valid frame max-abs {e:.3e}')
        assert e < ABS_TOL * max(1.0, float(refB.std()) / 1.48), (long, short, i, e)
    ctl = run(0.0, {})
    assert np.isfinite(ctl).all()
    r = rel_l2(ctl[2:, :, :Ls], refB)
    record(f'{long}+{short} control (zero padded, no lengths): short rows rel-L2 {r:.3e} max-abs {float(np.abs(ctl[2:, :, :Ls] - refB).max()):.3e}')
    assert r > 0.1, 'the fixtures cannot tell a padded batch from a ragged one'
    for i in range(2):   # the long rows never see the short ones, with or without lengths
        assert np.array_equal(ctl[i], pred[i])


# ---------------------------------------------------------------------------------------------------
# 2. sampler loop: smp_l (L 500) + smp_l_edit (L 300, editing) in one call
# ---------------------------------------------------------------------------------------------------
def _smp_row(name):
    cfg, sd, inp, init, noises, g, meta = sampler_case(name)
    row = dict(ctx=inp['ctx'], mask=inp['ctx_mask'], init=init, noises=noises, L=meta['L'], gold=g['latent'][0], gt=None, gm=None)
    if meta['with_gt']:
        row['gt'], row['gm'] = inp['gt'][0:1], inp['gt_mask'][0:1]
    return row, meta


def _prepare_ragged(m, rows, meta, lengths=True, fill=np.nan):
    from ezaudio_amd.sampler import LatentSampler
    from ezaudio_amd.scheduler import DDIMScheduler
    smp = LatentSampler(m, DDIMScheduler(**DIFF))
    steps, Lmax = meta['steps'], max(r['L'] for r in rows)
    C_ = rows[0]['init'].shape[1]
    f = np.float32(fill)
    text, tm = t_(np.stack([r['ctx'][0] for r in rows])), t_(np.stack([r['mask'][0] for r in rows]))
    un, um = t_(np.stack([r['ctx'][1] for r in rows])), t_(np.stack([r['mask'][1] for r in rows]))
    init = t_(np.concatenate([_padded(r['init'], Lmax, f) for r in rows], 0))
    sn = torch.stack([t_(np.concatenate([_padded(r['noises'][i], Lmax, f) for r in rows], 0)) for i in range(steps)], 0)
    gt = gm = None
    if any(r['gt'] is not None for r in rows):   # rows without a reference clip: gt_mask all ones
        gt = t_(np.concatenate([_padded(r['gt'], Lmax, f) if r['gt'] is not None else np.zeros((1, C_, Lmax), np.float32) for r in rows], 0))
        gm = t_(np.concatenate([_padded(r['gm'], Lmax, False) if r['gm'] is not None else np.ones((1, C_, Lmax), bool) for r in rows], 0))
    kw = dict(lengths=[r['L'] for r in rows]) if lengths else {}
    smp.prepare(text, tm, un, um, init, sn, meta['guidance_scale'], meta['guidance_rescale'], steps, meta['eta'], gt=gt, gt_mask=gm, **kw)
    return smp, init, gt, gm


def _finish_ragged(smp, rows, gt, gm, use_graph):
    smp.run(use_graph=use_graph)
    lat = smp.finish()
    torch.cuda.synchronize()
    lat = lat.clone()
    for i, r in enumerate(rows):
        assert torch.equal(lat[i, :, r['L']:], torch.zeros_like(lat[i, :, r['L']:])), 'padded latent frames must be exactly 0'
    if gt is not None:
        lat = torch.where(gm, lat, gt)   # src/inference.py:104-105
    return [lat[i, :, :r['L']].cpu().numpy() for i, r in enumerate(rows)]


def _run_ragged(m, rows, meta, use_graph=True):
    smp, _, gt, gm = _prepare_ragged(m, rows, meta)
    return _finish_ragged(smp, rows, gt, gm, use_graph)


def test_sampler_of_a_padded_batch_matches_each_samples_own_loop_golden(lib):
    """One LatentSampler call over smp_l (500 frames) and smp_l_edit (300 frames, editing): each final latent within 2e-2 of the golden of
    the reference's own loop at that length (which also judges the rescale statistics: a count of C * 500 instead of C * 300 moves the
    std by sqrt(5 / 3)).  Again with P = 4 (M = 4000 token rows: the large-M kernel forms), equal prompts bitwise equal; graph replay
    bitwise the eager loop; then the prompts swapped on the same model -- the table decides, not what an earlier call left behind."""
    A, metaA = _smp_row('smp_l')
    B, metaB = _smp_row('smp_l_edit')
    for k in ('size', 'seed_w', 'steps', 'guidance_scale', 'guidance_rescale', 'eta', 'Lc'):
        assert metaA[k] == metaB[k], k
    m = get_model(metaA['size'], metaA['seed_w'])

    def check(lats, rows, tag):
        for i, (lat, r) in enumerate(zip(lats, rows)):
            assert np.isfinite(lat).all()
            e = rel_l2(lat, r['gold'])
            record(f'ragged sampler {tag} row {i} (L {r["L"]}): final-latent rel-L2 {e:.3e}')
            assert e < 2e-2, (tag, i, e)

    two = _run_ragged(m, [A, B], metaA)
    check(two, [A, B], 'P=2 (500, 300)')
    four = _run_ragged(m, [A, B, A, B], metaA)
    check(four, [A, B, A, B], 'P=4')
    assert np.array_equal(four[0], four[2]) and np.array_equal(four[1], four[3])
    eager = _run_ragged(m, [A, B, A, B], metaA, use_graph=False)
    for a, b in zip(four, eager):
        assert np.array_equal(a, b)
    swapped = _run_ragged(m, [B, A], metaA)
    check(swapped, [B, A], 'P=2 (300, 500)')


def test_a_captured_step_reads_the_lengths_at_run_time(lib):
    """The SAME captured graph replayed after ezdit_set_lengths with other lengths equals, bit for bit, a fresh call with those lengths."""
    A, meta = _smp_row('smp_xs')
    m = get_model(meta['size'], meta['seed_w'])
    L = A['L']
    rows = [A, A]
    smp, init, _, _ = _prepare_ragged(m, rows, meta, lengths=False, fill=0.0)
    st = C.c_void_p(smp.stream.cuda_stream)
    m.set_lengths([L, 77], st)
    smp.run(use_graph=True)
    smp.finish()
    first = smp.latents.clone()
    # other lengths, same graph: rewind the step counter, restore the initial latents, replay
    m.set_lengths([50, L], st)
    with torch.cuda.stream(smp.stream):
        smp.latents.copy_(init)
        assert lib.ezdit_set_step(m._h, 0, st) == 0
    smp.run(use_graph=True)
    smp.finish()
    replay = smp.latents.clone()
    assert not torch.equal(first, replay)
    smp2, _, _, _ = _prepare_ragged(m, rows, meta, lengths=False, fill=0.0)
    m.set_lengths([50, L], C.c_void_p(smp2.stream.cuda_stream))
    smp2.run(use_graph=True)
    smp2.finish()
    assert torch.equal(replay, smp2.latents)
    assert torch.equal(replay[0, :, 50:], torch.zeros_like(replay[0, :, 50:])) and torch.isfinite(replay).all()
    m.set_lengths(None)


# ---------------------------------------------------------------------------------------------------
# 3. XL width above 2048 token rows (no golden pair): every row against the oracle run on that row alone
# ---------------------------------------------------------------------------------------------------
def test_forward_of_a_padded_batch_above_2048_rows_against_the_oracle_per_row(lib):
    """B = 8 at XL width, four lengths as CFG pairs (M = 4000: the ping-pong producers, the co-resident QKV GEMM, 4-wave attention)."""
    from oracle.dit import DiTOracle
    size, seed = 'xl', 1234
    cfg = model_config(size)
    o = DiTOracle(cfg, make_state_dict(cfg, seed))
    m = get_model(size, seed)
    lens = [500, 300, 131, 77] * 2
    Lmax, C_ = 500, cfg['out_chans']
    rows = []
    for j, L in enumerate(lens[:4]):   # pair j = (cond row j, uncond row 4 + j) with their own inputs
        rows.append(make_inputs(cfg, B=2, L=L, Lc=100, n_valid=(12 - j, 1), seed=31 + j))
    order = [(j, 0) for j in range(4)] + [(j, 1) for j in range(4)]
    x = np.concatenate([_padded(rows[j]['x'][r:r + 1], Lmax, np.float32(np.nan)) for j, r in order])
    ctx = np.concatenate([rows[j]['ctx'][r:r + 1] for j, r in order])
    cm = np.concatenate([rows[j]['ctx_mask'][r:r + 1] for j, r in order])
    pred, _ = m(t_(x), torch.tensor(499), t_(ctx), context_mask=t_(cm), x_lens=lens)
    torch.cuda.synchronize()
    pred = pred.cpu().numpy()
    for b, (j, r) in enumerate(order):
        L = lens[b]
        ref, _ = o.forward(rows[j]['x'][r:r + 1], 499, rows[j]['ctx'][r:r + 1], rows[j]['ctx_mask'][r:r + 1])
        _gate(pred[b, :, :L], ref[0], f'xl B=8 ragged row {b} (L {L})')
        assert np.array_equal(pred[b, :, L:], np.zeros((C_, Lmax - L), np.float32))


# ---------------------------------------------------------------------------------------------------
# 4. identity: all lengths equal to L = no lengths, bit for bit
# ---------------------------------------------------------------------------------------------------
def test_full_lengths_are_bitwise_the_call_without_lengths(lib):
    _, _, inp, _, _, meta = golden_case('xl')
    m = get_model(meta['size'], meta['seed_w'])
    args = (t_(inp['x']), torch.tensor(499), t_(inp['ctx']))
    a, _ = m(*args, context_mask=t_(inp['ctx_mask']))
    na = m.last_launch_count
    b, _ = m(*args, context_mask=t_(inp['ctx_mask']), x_lens=[meta['L']] * 2)
    nb = m.last_launch_count
    c, _ = m(*args, context_mask=t_(inp['ctx_mask']))
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c) and na == nb and na > 0

    A, smeta = _smp_row('smp_xs')
    ms = get_model(smeta['size'], smeta['seed_w'])
    outs = []
    for lengths in (False, True, False):
        smp, _, _, _ = _prepare_ragged(ms, [A, A], smeta, lengths=lengths)
        smp.run()
        outs.append(smp.finish().clone())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]) and torch.isfinite(outs[0]).all()


# ---------------------------------------------------------------------------------------------------
# 5. kernel level
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('xcd', [0, 1])
@pytest.mark.parametrize('nkh', [2, 4])        # 64-key tiles / 4 waves and 128-key tiles / 8 waves
@pytest.mark.parametrize('size', ['xs', 'xs64'])   # head sizes 72 and 64
def test_attention_with_per_sample_key_lengths_against_fp64_softmax(lib, size, nkh, xcd):
    """ezdit_test_attention_varlen against an fp64 softmax over the keys < klen_b; tolerances of test_attention_against_softmax_reference
    (P and O are bf16).  Lengths: 1, one below / at / above the edges of both tile sizes, Lmax.  K / V rows beyond klen_b hold large finite
    values (a key the mask forgot would be seen at once); query rows >= klen_b must come back exactly 0."""
    m = get_model(size, 1)
    cfg = model_config(size)
    H, D = cfg['num_heads'], cfg['embed_dim']
    dh = D // H
    DQK, DV = (64, 64) if dh == 64 else (80, 96)
    L = 300
    klen = [1, 63, 64, 65, 127, 128, 129, L]
    B = len(klen)
    Lp = (L + 127) // 128 * 128
    g = torch.Generator().manual_seed(1000 * nkh + dh)
    q = torch.randn(B, H, L, dh, generator=g).to(torch.bfloat16)
    k = torch.randn(B, H, L, dh, generator=g).to(torch.bfloat16)
    v = torch.randn(B, H, L, dh, generator=g).to(torch.bfloat16)
    k[0, 0, 0] *= 6.0
    k[4, 1, 3] *= 6.0   # a spiked key: a large running-max jump in the online softmax
    ref = torch.zeros(B, L, D, dtype=torch.float64)
    for b, n in enumerate(klen):
        s = (q[b, :, :n].double() @ k[b, :, :n].double().transpose(1, 2)) * dh ** -0.5
        ref[b, :n] = (torch.softmax(s, -1) @ v[b, :, :n].double()).transpose(0, 1).reshape(n, D)
        k[b, :, n:] = 3.0e4
        v[b, :, n:] = -3.0e4
    qp = torch.zeros(B, H, Lp, DQK, dtype=torch.bfloat16); qp[:, :, :L, :dh] = q
    kp = torch.zeros(B, H, Lp, DQK, dtype=torch.bfloat16); kp[:, :, :L, :dh] = k
    vp = torch.zeros(B, H, Lp, DV, dtype=torch.bfloat16); vp[:, :, :L, :dh] = v
    ldD = (D + 63) // 64 * 64
    out = torch.full((B * L, ldD), 7.0, dtype=torch.bfloat16, device='cuda:0')
    qd, kd, vd = qp.cuda(), kp.cuda(), vp.cuda()
    kl = torch.tensor(klen, dtype=torch.int32, device='cuda:0')
    try:
        assert lib.ezdit_set_option(m._h, b'attn_nkh', nkh) == 0 and lib.ezdit_set_option(m._h, b'attn_xcd', xcd) == 0
        rc = lib.ezdit_test_attention_varlen(m._h, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), None, out.data_ptr(), B, L, L, Lp, Lp,
                                             kl.data_ptr(), None)
        assert rc == 0, lib.ezdit_last_error()
        torch.cuda.synchronize()
        bad = torch.tensor([1, 0], dtype=torch.int32, device='cuda:0')   # klen_b = 0 is refused on the host
        assert lib.ezdit_test_attention_varlen(m._h, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), None, out.data_ptr(), 2, L, L, Lp, Lp,
                                               bad.data_ptr(), None) == -1
    finally:
        assert lib.ezdit_set_option(m._h, b'attn_nkh', 0) == 0 and lib.ezdit_set_option(m._h, b'attn_xcd', 1) == 0
    got = out.float().cpu()[:, :D].reshape(B, L, D)
    assert torch.isfinite(got).all()
    for b, n in enumerate(klen):
        assert torch.equal(got[b, n:], torch.zeros(L - n, D)), f'klen {n}: query rows beyond the length must be exactly 0'
        r, a = rel_l2(got[b, :n].numpy(), ref[b, :n].numpy()), (got[b, :n].double() - ref[b, :n]).abs().max().item()
        record(f'attention varlen {size} nkh={nkh} xcd={xcd} klen={n}: rel-L2 {r:.3e} max-abs {a:.3e}')
        assert r < 1.2e-2 and a < 0.06, (n, r, a)


@pytest.mark.parametrize('L,lens', [(50, None), (50, [50, 33, 1, 4]), (77, None), (77, [76, 77, 2, 41])])
def test_final_conv_against_fp64_convolution_of_each_sample_alone(lib, L, lens):
    """k_final_conv accumulates 3 C fp32 products per output (plus bias): |err| <= 3 C 2^-24 sum(|w| |x|) per element -- derived, not
    measured.  With lengths the padded rows of the input hold NaN: they must not be read."""
    Cc, B = 128, 4
    g = torch.Generator().manual_seed(L)
    y = torch.randn(B, L, Cc, generator=g)
    w = torch.randn(Cc, Cc, 3, generator=g) * 0.1
    bias = torch.randn(Cc, generator=g) * 0.1
    ln = lens or [L] * B
    ref = torch.zeros(B, Cc, L, dtype=torch.float64)
    bound = torch.zeros(B, Cc, L, dtype=torch.float64)
    for b, n in enumerate(ln):
        xb = y[b, :n].double().t()[None]                                   # the sample alone: [1, C, n]
        ref[b, :, :n] = torch.nn.functional.conv1d(xb, w.double(), bias.double(), padding=1)[0]
        bound[b, :, :n] = 3 * Cc * 2.0 ** -24 * torch.nn.functional.conv1d(xb.abs(), w.double().abs(), None, padding=1)[0]
        if lens:
            y[b, n:] = float('nan')
    yd, wd, bd = y.reshape(B * L, Cc).cuda(), w.cuda(), bias.cuda()
    out = torch.full((B, Cc, L), 7.0, device='cuda:0')
    kl = torch.tensor(ln, dtype=torch.int32, device='cuda:0') if lens else None
    rc = lib.ezdit_test_final_conv(yd.data_ptr(), Cc, wd.data_ptr(), bd.data_ptr(), out.data_ptr(), B, Cc, L,
                                   kl.data_ptr() if lens else None, None)
    assert rc == 0, lib.ezdit_last_error()
    torch.cuda.synchronize()
    got = out.cpu().double()
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    record(f'final conv L={L} lens={lens}: max err {err.max().item():.3e}, max err / bound {(err / bound.clamp_min(1e-300))[bound > 0].max().item():.3e}')
    assert (err <= bound).all()
    for b, n in enumerate(ln):
        assert torch.equal(got[b, :, n:], torch.zeros(Cc, L - n, dtype=torch.float64))
    assert lib.ezdit_test_final_conv(yd.data_ptr(), Cc, wd.data_ptr(), bd.data_ptr(), out.data_ptr(), B, 12, L, None, None) == -2   # C % 8


# ---------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------
def test_set_lengths_refusals(lib):
    from ezaudio_amd import DiTControlNet, MaskDiT
    from oracle.controlnet import CN_DEFAULT, make_controlnet_state_dict
    cfg = model_config('xs')
    sd = make_state_dict(cfg, 1)
    inp = make_inputs(cfg, B=2, L=96, Lc=20, n_valid=(7, 1), seed=11)
    m = MaskDiT(device='cuda:0', **cfg)
    m.load_state_dict(sd)

    def set_(h, vals):
        arr = (C.c_int32 * len(vals))(*vals)
        return lib.ezdit_set_lengths(h, arr, len(vals), None)

    assert set_(m._h, [96, 96]) == -3                       # before a workspace is bound
    x, ctx, cm = t_(inp['x']), t_(inp['ctx']), t_(inp['ctx_mask'])
    ref, _ = m(x, torch.tensor(499), ctx, context_mask=cm)
    n0 = m.last_launch_count
    assert set_(m._h, [96, 0]) == -1 and set_(m._h, [97, 96]) == -1 and set_(m._h, [-5]) == -1
    assert set_(m._h, [96, 96, 96]) == -1                   # n does not divide B
    assert lib.ezdit_set_lengths(m._h, None, 0, None) == 0  # clearing is always allowed
    # cn_skips with lengths set
    assert set_(m._h, [96, 77]) == 0
    D, nh = cfg['embed_dim'], cfg['depth'] // 2
    skips = [torch.zeros(2, 96, D, device='cuda:0') for _ in range(nh)]
    arr = (C.c_void_p * nh)(*[s.data_ptr() for s in skips])
    out = torch.full((2, cfg['out_chans'], 96), 7.0, device='cuda:0')
    x257 = torch.zeros(2, cfg['in_chans'], 96, device='cuda:0')
    rc = lib.ezdit_forward(m._h, x257.data_ptr(), cfg['in_chans'], 2, None, None, arr, nh, out.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == -2 and m.last_launch_count == n0 and bool((out == 7.0).all())     # nothing launched
    assert lib.ezdit_set_lengths(m._h, None, 0, None) == 0
    again, _ = m(x, torch.tensor(499), ctx, context_mask=cm)
    assert torch.equal(ref, again)                          # the refused calls left nothing behind
    # a ControlNet handle, and a backbone with one attached
    ccfg = dict(cfg)
    ccfg.update(CN_DEFAULT)
    cn = DiTControlNet(device='cuda:0', **ccfg)
    cn.load_state_dict(make_controlnet_state_dict(cfg, CN_DEFAULT, 1))
    cn.bind(2, 96, 20, 1)
    assert set_(cn._h, [96, 77]) == -2
    assert lib.ezdit_sampler_attach_controlnet(m._h, cn._h, 1.0) == 0
    assert set_(m._h, [96, 77]) == -2
    assert lib.ezdit_sampler_attach_controlnet(m._h, None, 1.0) == 0
    assert set_(m._h, [96, 77]) == 0 and lib.ezdit_set_lengths(m._h, None, 0, None) == 0
    with pytest.raises(NotImplementedError):
        m(x, torch.tensor(499), ctx, context_mask=cm, x_mask=torch.ones(2, 96, dtype=torch.bool, device='cuda:0'))
