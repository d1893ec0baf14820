"""GPU tests of the HIP T5 encoder (csrc/t5.hip, ezaudio_amd/t5.py) against the fp64 judge of tests/t5_ref.py.

The gate of the encode and attention tests: rel-L2 and max-abs error against the fp64 judge each at most 2 x the same error of the
bf16-operand emulation (t5_ref with emulate=True: same rounding points, exact accumulation) against the judge, plus a floor of 1e-6
for shapes where the emulation happens to be exact.  The factor covers accumulation order and the fp32 softmax / norm arithmetic."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import t5_ref
from tests.util import record, rel_l2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
SEED_W, SEED_IN = 1, 3          # tools/mint_t5_golden.py
LENGTHS = (7, 100, 130)
FLOOR = 1e-6


def t_(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bf16_bits(a):
    """fp64 / fp32 array -> torch bf16 tensor on the device holding bf16_round(a) exactly"""
    return t_(t5_ref.bf16_round(a).astype(np.float32)).to(torch.bfloat16)


_cache = {}


def _encoder(name):
    from ezaudio_amd import T5Encoder
    if ('enc', name) not in _cache:
        cfg = t5_ref.config(name)
        sd = t5_ref.make_weights(cfg, SEED_W)
        enc = T5Encoder(cfg, DEV).load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        _cache[('enc', name)] = (cfg, sd, enc)
    return _cache[('enc', name)]


def _case(name, L):
    """ids, mask, judge, emulation of one (configuration, length); computed once per session and never modified"""
    if ('case', name, L) not in _cache:
        cfg, sd, _ = _encoder(name)
        ids = t5_ref.make_ids(cfg, 3, L, SEED_IN)
        mask = t5_ref.make_mask(3, L, (1, min(37, L), L))
        ref = t5_ref.encode(cfg, sd, ids, mask)
        emu = t5_ref.encode(cfg, sd, ids, mask, emulate=True)
        for a in (ids, mask, ref, emu):
            a.setflags(write=False)
        _cache[('case', name, L)] = (ids, mask, ref, emu)
    return _cache[('case', name, L)]


def _run(enc, ids, mask):
    out = enc(input_ids=t_(ids), attention_mask=t_(mask)).last_hidden_state
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _budget(emu, ref):
    """the emulation's own (rel-L2, max-abs) error against the judge"""
    return rel_l2(emu, ref), float(np.abs(emu - ref).max())


def _gate(tag, got, ref, budget):
    """2 x the emulation's error against the judge, floor 1e-6; arrays restricted to the positions that count"""
    r, a = rel_l2(got, ref), float(np.abs(got - ref).max())
    er, ea = budget
    record(f'{tag}: rel-L2 {r:.3e} (emulation {er:.3e}) max-abs {a:.3e} (emulation {ea:.3e})')
    assert r <= 2 * er + FLOOR and a <= 2 * ea + FLOOR, (tag, r, er, a, ea)


@pytest.mark.parametrize('L', LENGTHS)
@pytest.mark.parametrize('name', ['a', 'b'])
def test_encode_matches_the_judge_and_the_transformers_goldens(lib, name, L):
    """B = 3 with (1, 37, L) valid tokens in one batch (the single-token row is the empty prompt of every CFG call); L = 7 is less than one key tile,
    100 the shipped max_length and no tile multiple, 130 three 64-key tiles with distances past max_distance (the last bucket clamps)."""
    cfg, sd, enc = _encoder(name)
    ids, mask, ref, emu = _case(name, L)
    got = _run(enc, ids, mask)
    assert got.shape == (3, L, cfg['d_model']) and got.dtype == np.float32
    assert np.isfinite(got).all()                       # padded positions included
    valid = mask.astype(bool)
    budget = _budget(emu[valid], ref[valid])
    _gate(f't5 encode {name} L={L}', got[valid], ref[valid], budget)
    g = np.load(os.path.join(ROOT, 'tests', 'golden', f't5_tiny_{name}.npz'))
    assert np.array_equal(g[f'ids_{L}'], ids) and np.array_equal(g[f'mask_{L}'], mask)
    gold = g[f'out_{L}'].astype(np.float64)
    _gate(f't5 encode {name} L={L} vs transformers golden', got[valid], gold[valid], budget)


def _attn_masks(B, L):
    cut = max(1, min(L - 1, 64 * (L // 128) + 37))   # a cut in the middle of a 64-key tile
    return t5_ref.make_mask(B, L, (1, L, cut))


@pytest.mark.parametrize('L', [1, 63, 64, 65, 130, 512])
def test_attention_hook_matches_fp64_softmax(lib, L):
    """k_t5_attn alone: bias and key mask, no scale; masks with one valid key, all valid and a cut inside a tile; NaN in K and V of masked keys stays out"""
    from oracle.weights import uniform_pm1
    B, H, d = 3, 2, 64
    mask = _attn_masks(B, L)
    q, k, v = (t5_ref.bf16_round((uniform_pm1(f't5.attn.{n}', B * L * H * d, L) * s).reshape(B, L, H, d)) for n, s in (('q', 1.0), ('k', 1.5), ('v', 2.0)))
    tab = (uniform_pm1('t5.attn.tab', 32 * H, L) * 2.0).astype(np.float64).reshape(32, H)
    rel = np.arange(L)[None, :] - np.arange(L)[:, None]
    bias = tab[t5_ref.bucket(rel)].transpose(2, 0, 1)                                  # [H, query, key]
    table = np.ascontiguousarray(tab[t5_ref.bucket(np.arange(-(L - 1), L))].T).astype(np.float32)   # [H, 2 L - 1]
    hd = lambda a: a.transpose(0, 2, 1, 3)
    ref = hd(t5_ref.attention(hd(q), hd(k), hd(v), bias, mask))                        # [B, L, H, d]
    emu = t5_ref.bf16_round(hd(t5_ref.attention(hd(q), hd(k), hd(v), bias, mask, emulate=True)))   # the kernel's output is bf16
    kn, vn = k.copy(), v.copy()
    kn[mask == 0] = np.nan
    vn[mask == 0] = np.nan
    out = torch.full((B * L, H * d), float('nan'), dtype=torch.bfloat16, device=DEV)
    dq, dk, dv, dt, dm = _bf16_bits(q), t_(kn.astype(np.float32)).to(torch.bfloat16), t_(vn.astype(np.float32)).to(torch.bfloat16), t_(table), t_(mask)
    rc = lib.ezt5_test_attention(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dt.data_ptr(), dm.data_ptr(), out.data_ptr(), B, H, L,
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.ezdit_last_error()
    torch.cuda.synchronize()
    got = out.float().cpu().numpy().astype(np.float64).reshape(B, L, H, d)
    assert np.isfinite(got).all()
    _gate(f't5 attention L={L}', got, ref, _budget(emu, ref))


@pytest.mark.parametrize('scale', [1.0, 1e4])
def test_rms_norm_is_within_one_bf16_ulp_of_fp64(lib, scale):
    """k_t5_embed_rms on a residual stream of magnitude 1 and 1e4 (where a 16-bit stream would have lost the small terms): the bf16 operand
    is within one bf16 ulp of the fp64 result, element by element; D = 192 (lanes past the row end) and 2048 (eight passes per lane), 5 rows (two blocks)"""
    from oracle.weights import make_tensor, uniform_pm1
    for D in (192, 2048):
        M = 5
        x = (uniform_pm1(f't5.rms.x{D}', M * D, 2).reshape(M, D) * np.float32(scale)).astype(np.float32)
        x[:, ::7] *= np.float32(1e-3)      # small entries next to large ones
        w = make_tensor(f't5.rms.w{D}', (D,), 'ln_w', 2)
        want = t5_ref.rms(x.astype(np.float64), w.astype(np.float64), 1e-6)
        out = torch.empty(M, D, dtype=torch.bfloat16, device=DEV)
        dx, dw = t_(x), t_(w)
        rc = lib.ezt5_test_rms(dx.data_ptr(), dw.data_ptr(), C.c_float(1e-6), out.data_ptr(), M, D, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.ezdit_last_error()
        torch.cuda.synchronize()
        got = out.float().cpu().numpy().astype(np.float64)
        err = np.abs(got - want) / t5_ref.bf16_ulp(want)
        record(f't5 rms scale={scale:g} D={D}: max error {err.max():.3f} bf16 ulp')
        assert err.max() <= 1.0


def test_rows_are_independent_of_the_batch_and_of_masked_ids(lib):
    """Row b of a batch equals the same row encoded alone BIT FOR BIT (the GEMM tile id does not depend on the row count, csrc/t5.hip), and nothing
    depends on what the ids hold at masked positions (valid positions bit for bit)."""
    cfg, sd, enc = _encoder('b')
    for L in (100, 130):
        ids, mask, _, _ = _case('b', L)
        full = _run(enc, ids, mask)
        for b in range(3):
            alone = _run(enc, ids[b:b + 1], mask[b:b + 1])
            assert np.array_equal(alone[0], full[b]), (L, b)
        ids2 = ids.copy()
        ids2[mask == 0] = (ids2[mask == 0] + 41) % cfg['vocab_size']
        assert not np.array_equal(ids2, ids)
        other = _run(enc, ids2, mask)
        valid = mask.astype(bool)
        assert np.array_equal(other[valid], full[valid]), L


def test_context_drops_into_the_denoiser(lib):
    """model_config('xs')['context_dim'] is 96, no multiple of 64, so a T5 of that width cannot be built; the xs denoiser is built with context_dim 128
    instead (configuration a's width).  One MaskDiT forward with the native encoder's context and one with the fp64 judge's, same mask and inputs:
    the predictions agree within the tolerance tests/test_gpu.py holds the denoiser to.  Then inference(..., text_encoder=enc) end to end."""
    from ezaudio_amd import MaskDiT
    from ezaudio_amd.sampler import inference
    from ezaudio_amd.scheduler import DDIMScheduler
    from oracle.weights import make_inputs, make_state_dict, model_config
    REL_TOL, ABS_TOL = 2e-2, 0.15   # tests/test_gpu.py
    from tests.util import DIFF
    assert model_config('xs')['context_dim'] % 64 != 0
    tcfg, tsd, enc = _encoder('a')
    cfg = dict(model_config('xs'), context_dim=tcfg['d_model'])
    m = MaskDiT(device=DEV, **cfg)
    m.load_state_dict(make_state_dict(cfg, 1))
    L = 100
    ids, mask, ref, _ = _case('a', L)
    ids, mask, ref = ids[1:3], mask[1:3], ref[1:3]          # 37 and 100 valid tokens
    inp = make_inputs(cfg, B=2, L=64, Lc=L)
    native = enc(input_ids=t_(ids), attention_mask=t_(mask)).last_hidden_state
    preds = []
    for ctx in (native, t_(ref.astype(np.float32))):
        pred, _ = m(t_(inp['x']), torch.tensor(500), ctx, context_mask=t_(mask.astype(bool)), cls_token=None)
        preds.append(pred.cpu().numpy())
    got, want = preds
    assert np.isfinite(got).all()
    r, a = rel_l2(got, want), float(np.abs(got - want).max())
    record(f't5 drop-in xs(context 128): rel-L2 {r:.3e} max-abs {a:.3e}')
    assert r < REL_TOL and a < ABS_TOL * max(1.0, float(want.std()) / 1.48)

    class Tok:
        def __call__(self, texts, max_length, padding, truncation, return_tensors):
            n = len(texts)
            tm = np.zeros((n, max_length), dtype=np.int64)
            for i, t in enumerate(texts):
                tm[i, :max(1, min(max_length, len(t.split()) + 1))] = 1
            return type('Batch', (), dict(input_ids=torch.from_numpy(t5_ref.make_ids(tcfg, n, max_length, 5)), attention_mask=torch.from_numpy(tm)))()
    params = dict(text_encoder=dict(max_length=100), model=dict(out_chans=cfg['out_chans']), autoencoder=dict(scale=1.0, shift=0.0))
    wav = inference(lambda embedding: embedding, m, None, None, Tok(), enc, params, DDIMScheduler(**DIFF), ['a dog barking in the rain'],
                    audio_frames=64, guidance_scale=3, ddim_steps=4, random_seed=3, device=DEV)
    assert wav.shape == (1, cfg['out_chans'], 64) and torch.isfinite(wav).all() and float(wav.std()) > 0


def test_call_order_length_limit_and_rebinding(lib):
    """ezt5_encode before weights / workspace -> EZDIT_E_STATE; L > max_len -> EZDIT_E_UNSUPPORTED with the output untouched; two encodes at
    different (B, L) on one handle give what fresh handles give."""
    from ezaudio_amd import T5Encoder, _lib
    cfg, sd, enc = _encoder('a')
    st = torch.cuda.current_stream().cuda_stream
    fresh = lambda **kw: T5Encoder(cfg, DEV, **kw)
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    ids = torch.zeros(2, 8, dtype=torch.int32, device=DEV)
    msk = torch.ones(2, 8, dtype=torch.uint8, device=DEV)
    out = torch.full((2, 8, cfg['d_model']), 7.0, device=DEV)
    e0 = fresh()
    assert lib.ezt5_encode(e0._h, ids.data_ptr(), msk.data_ptr(), out.data_ptr(), 2, 8, st) == -3      # no weights
    with pytest.raises(_lib.EzditError):
        e0(input_ids=ids, attention_mask=msk)
    e0.load_state_dict(tsd)
    assert lib.ezt5_encode(e0._h, ids.data_ptr(), msk.data_ptr(), out.data_ptr(), 2, 8, st) == -3      # no workspace
    e0._bind(2, 8)
    assert lib.ezt5_encode(e0._h, ids.data_ptr(), msk.data_ptr(), out.data_ptr(), 2, 9, st) == -3      # bound for another shape
    small = fresh(max_len=64).load_state_dict(tsd)
    big_ids = torch.zeros(1, 65, dtype=torch.int32, device=DEV)
    big_out = torch.full((1, 65, cfg['d_model']), 7.0, device=DEV)
    assert lib.ezt5_encode(small._h, big_ids.data_ptr(), msk.data_ptr(), big_out.data_ptr(), 1, 65, st) == -2
    with pytest.raises(NotImplementedError, match='max_len'):
        small(input_ids=big_ids, attention_mask=torch.ones(1, 65, device=DEV))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((big_out == 7.0).all())
    # one handle, two shapes, back and forth == fresh handles
    ia, ma, _, _ = _case('a', 7)
    ib, mb, _, _ = _case('a', 100)
    first = _run(enc, ia, ma)
    second = _run(enc, ib[:2], mb[:2])
    third = _run(enc, ia, ma)
    assert np.array_equal(first, third)
    assert np.array_equal(first, _run(fresh().load_state_dict(tsd), ia, ma))
    assert np.array_equal(second, _run(fresh().load_state_dict(tsd), ib[:2], mb[:2]))
