"""Kernel-level GPU tests of the T5 encoder (csrc/t5.hip) against the fp64 references of tests/t5_emul.py: k_t5_attn in both operand forms, k_t5_embed_rms on its four paths,
k_t5_gated_gelu and the encoder's GEMM call, each alone through its hook; the hooks chained into a layer against ezt5_encode, bit for bit; ezt5_encode gated per valid row.

No gate here is a number chosen by hand: each is a derived bound (stated in tests/t5_emul.py), twice a floor the emulation there gives (ATTN_FLOORS;
tests/test_t5_kernels_host.py holds the record to the emulation), bitwise, or one of the two share conditions."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import t5_emul as E
from tests import t5_ref
from tests.util import record

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
f32 = np.float32


def t_(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bf_(a):
    """bf16-valued fp32 array (NaN allowed) -> bf16 tensor on the device"""
    return t_(np.asarray(a, f32)).to(torch.bfloat16)


def np_(t):
    torch.cuda.synchronize()
    return t.float().cpu().numpy()


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---- attention ----------------------------------------------------------------------------------------------------------------------
def _attn_run(lib, c, form, flat=None, only_b=None):
    """k_t5_attn on the case's buffers through ezt5_test_attention_ex -> the whole out buffer [rows][ldo] as fp32.  form 'bf16': three bf16 buffers, ld = 64 H; 'f32': ONE
    interleaved fp32 buffer, ld = 3 inner, k = q + inner (as ezt5_encode passes them).  only_b: that batch element alone, B = 1, written to its place in a fresh buffer."""
    base, qo, ko, vo, ld = c.operands(form)
    flat = base if flat is None else flat
    buf = t_(flat) if form == 'f32' else bf_(flat)
    es = 4 if form == 'f32' else 2
    b0, B = (0, c.B) if only_b is None else (only_b, 1)
    row = (E.GUARD + b0 * c.L)
    tab, mask = t_(c.table), t_(c.mask)
    out = torch.full((c.B * c.L + 2 * E.GUARD, c.ldo), E.SENTINEL, dtype=torch.bfloat16, device=DEV)
    p = lambda off: buf.data_ptr() + (off + row * ld) * es
    rc = lib.ezt5_test_attention_ex(p(qo), p(ko), p(vo), int(form == 'f32'), ld, tab.data_ptr(), c.bias_ld, c.bias_half, mask.data_ptr() + b0 * c.L,
                                    out.data_ptr() + row * c.ldo * 2, c.ldo, B, c.H, c.L, stream())
    assert rc == 0, lib.ezdit_last_error()
    return np_(out)


@pytest.mark.parametrize('L', E.ATTN_LENGTHS)
def test_attention_both_forms_against_fp64(lib, L):
    """every (L, max_len) case of tests/t5_emul.py in the bf16 form and in the production form (fp32 operands in one interleaved buffer, a bias row of 2 max_len - 1): worst
    (batch element, head) rel-L2, worst query-row rel-L2 and max-abs against reference (a), and (b) for the fp32 form, each at most 2 x ATTN_FLOORS; finite; sentinels in
    the columns [64 H, ldo) and the guard rows intact; the empty element's rows zero; each batch element alone equals its slice; the two forms agree bit for bit on
    operands that are bf16 values."""
    gates = E.attn_gates()
    for ml in E.attn_max_lens(L):
        c = E.attn_case(L, ml)
        outs = {}
        for form in ('bf16', 'f32'):
            out = outs[form] = _attn_run(lib, c, form)
            worst = {}
            for w in E.attn_refs(form):
                for qn, val in c.measure(out, w).items():
                    worst[f'{qn}_{w}'] = val
            record(f't5 attn {c.id()} {form} ({",".join(c.kinds)}): ' + ' '.join(f'{k} {v:.3e} (gate {gates[k]:.2e})' for k, v in worst.items()))
            assert c.bitwise_ok(out), (c.id(), form)
            for k, v in worst.items():
                assert v <= gates[k], (c.id(), form, k, v, gates[k])
        base = c.operands('f32')[0]
        exact = _attn_run(lib, c, 'f32', flat=E.bf16r(base))
        assert np.array_equal(exact.view(np.uint32), outs['bf16'].view(np.uint32)), f'{c.id()}: the fp32 form on bf16-valued operands differs from the bf16 form'
        full = outs['f32']
        for b in range(c.B):
            alone = _attn_run(lib, c, 'f32', only_b=b)
            r0 = E.GUARD + b * c.L
            want = np.full_like(full, E.SENTINEL)
            want[r0:r0 + c.L, :c.I] = full[r0:r0 + c.L, :c.I]
            assert np.array_equal(alone.view(np.uint32), want.view(np.uint32)), f'{c.id()}: batch element {b} alone differs from its slice'


# ---- norm ---------------------------------------------------------------------------------------------------------------------------
def _norm_run(lib, c, path, alias=False):
    """-> (result fp32 [M][D], x_out or None, rows behind M of every output)"""
    M, D = c.M, c.D
    gather, to_f32 = path.startswith('ids'), path.endswith('f32')
    emb, ids = t_(c.emb), t_(c.ids)
    w = t_(np.concatenate([c.w, np.full(8, E.NAN, f32)]))
    x_in = t_(np.concatenate([c.x, np.full((E.GUARD, D), E.NAN, f32)]))
    x_out = torch.full((M + E.GUARD, D), E.SENTINEL, dtype=torch.float32, device=DEV)
    res = torch.full((M + E.GUARD, D), E.SENTINEL, dtype=torch.float32 if to_f32 else torch.bfloat16, device=DEV)
    xo_ptr = x_out.data_ptr() if gather else (x_in.data_ptr() if alias else None)
    rc = lib.ezt5_test_embed_rms(ids.data_ptr() if gather else None, emb.data_ptr() + E.GUARD * D * 4 if gather else None, c.V if gather else 0,
                                 None if gather else x_in.data_ptr(), xo_ptr, w.data_ptr(), C.c_float(E.NORM_EPS), None if to_f32 else res.data_ptr(),
                                 res.data_ptr() if to_f32 else None, M, D, stream())
    assert rc == 0, lib.ezdit_last_error()
    r, xo, xi = np_(res), np_(x_out), np_(x_in)
    assert (r[M:] == E.SENTINEL).all() and (xo[M:] == E.SENTINEL).all(), f'{c.id()} {path}: rows >= M written'
    if not gather:
        assert (xo == E.SENTINEL).all() and np.array_equal(xi[:M].view(np.uint32), c.x.view(np.uint32)), f'{c.id()} {path}: x_out written or x_in changed'
    return r[:M], (xo[:M] if gather else None)


@pytest.mark.parametrize('D', E.NORM_D)
def test_embed_rms_four_paths_against_fp64(lib, D):
    """k_t5_embed_rms at M in {1, 3, 4, 5, 133} and stream scales 1, 1e4, 1e-4 (eps of the order of the mean square) on x_in -> bf16, x_in -> fp32, ids -> bf16 with x_out and
    ids -> fp32: bf16 within one bf16 ulp of fp64 and under the share cap, fp32 within the derived bound norm_f32_rel(D); x_out == emb[clip(ids)], the gather path's result ==
    the x_in path's, x_in unchanged when x_out aliases it with ids null, rows >= M untouched -- bit for bit."""
    worst = {p: [0.0, 0.0] for p in E.NORM_PATHS}
    for M in E.NORM_M:
        for s in E.NORM_SCALES:
            c = E.norm_case(D, M, s)
            got = {}
            for path in E.NORM_PATHS:
                res, xo = got[path] = _norm_run(lib, c, path)
                xp = got[path.replace('ids', 'x')][0] if path.startswith('ids') else None
                bit, err, share = c.verdict(path, res, xo, xp)
                worst[path] = [max(worst[path][0], err), max(worst[path][1], share)]
                assert bit, f'{c.id()} {path}: not finite, x_out != emb[clip(ids)] or the gather path differs from the x_in path'
                assert err <= 1.0 and share <= 1.0, (c.id(), path, err, share)
            alias = _norm_run(lib, c, 'x_bf16', alias=True)[0]
            assert np.array_equal(alias.view(np.uint32), got['x_bf16'][0].view(np.uint32))
    record(f't5 embed_rms D={D}: bf16 worst {worst["x_bf16"][0]:.3f} bf16 ulp (gate 1), share / cap {worst["x_bf16"][1]:.3f}; '
           f'fp32 worst error / derived bound {worst["x_f32"][0]:.3f} (bound {E.norm_f32_rel(D):.2e} |ref|); gather paths {worst["ids_bf16"][0]:.3f} / {worst["ids_f32"][0]:.3f}')


# ---- gated GELU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F', E.GELU_F)
def test_gated_gelu_against_fp64(lib, F):
    """k_t5_gated_gelu: |error| <= half a bf16 ulp of the reference + the derived fp32 term (tests/t5_emul.py), the share condition over the elements where the rounding decides
    the bits, finite wherever the reference is, rows >= M untouched"""
    w = [0.0, 0.0]
    for M in E.GELU_M:
        c = E.gelu_case(M, F)
        h = t_(c.h)
        g = torch.full((M + E.GUARD, F), E.SENTINEL, dtype=torch.bfloat16, device=DEV)
        rc = lib.ezt5_test_gated_gelu(h.data_ptr() + E.GUARD * 2 * F * 4, g.data_ptr(), M, F, stream())
        assert rc == 0, lib.ezdit_last_error()
        got = np_(g)
        assert (got[M:] == E.SENTINEL).all(), f'{c.id()}: rows >= M written'
        fin, err, share = c.verdict(got[:M])
        w = [max(w[0], err), max(w[1], share)]
        assert fin and err <= 1.0 and share <= 1.0, (c.id(), fin, err, share)
    record(f't5 gated gelu F={F}: worst error / bound {w[0]:.3f}, share / cap {w[1]:.3f}')


# ---- GEMM ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', E.gemm_shapes(), ids=lambda s: s[0])
def test_gemm_at_the_encoder_shapes(lib, shape):
    """t5_gemm (tile 25, the residual in the epilogue) alone at M in {1, 5, 200}: 1 ... 5 rows inside a 128-row tile, two row tiles, K up to 5120 (80 K tiles), a residual of
    magnitude 1e4; per element (K + 3) 2^-24 (sum |a w| + |resid|) against the exact product of the bf16 operands; A between NaN guard rows, sentinel rows behind M"""
    name, N, K, res = shape
    worst = 0.0
    for M in E.GEMM_M:
        c = E.GemmCase(name, N, K, res, M)
        A, W = bf_(c.A), bf_(c.W)
        r = t_(c.resid) if res else None
        out = torch.full((M + E.GUARD, N), E.SENTINEL, dtype=torch.float32, device=DEV)
        rc = lib.ezt5_test_gemm(A.data_ptr() + E.GUARD * K * 2, K, W.data_ptr(), N, r.data_ptr() if res else None, out.data_ptr(), M, stream())
        assert rc == 0, lib.ezdit_last_error()
        got = np_(out)
        assert (got[M:] == E.SENTINEL).all(), f'{c.id()}: rows >= M written'
        ref, bound = c.ref_and_bound()
        worst = max(worst, E.worst_ratio(got[:M], ref, bound))
        assert worst <= 1.0, (c.id(), worst)
    record(f't5 gemm {name} N={N} K={K}{" +resid 1e4" if res else ""}: worst error / derived bound {worst:.3f}')


# ---- hooks equal production ---------------------------------------------------------------------------------------------------------
def _enc(cfg):
    from ezaudio_amd import T5Encoder
    sd = t5_ref.make_weights(cfg, 1)
    return sd, T5Encoder(cfg, DEV).load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})


def _slot(enc, name):
    t = {t['name']: t for t in enc.table}[name]
    return enc._blob.data_ptr() + t['offset']


def test_zero_layer_encode_is_the_embed_rms_hook(lib):
    cfg = t5_ref.config('b', num_layers=0)
    sd, enc = _enc(cfg)
    B, L, D = 3, 7, cfg['d_model']
    ids = t5_ref.make_ids(cfg, B, L, 3).astype(np.int32)
    want = np_(enc(input_ids=t_(ids), attention_mask=t_(t5_ref.make_mask(B, L, (1, 5, L)))).last_hidden_state).reshape(B * L, D)
    dids = t_(ids)
    x_out = torch.empty(B * L, D, device=DEV)
    out = torch.empty(B * L, D, device=DEV)
    rc = lib.ezt5_test_embed_rms(dids.data_ptr(), _slot(enc, 'embed'), cfg['vocab_size'], None, x_out.data_ptr(), _slot(enc, 'final_ln'), C.c_float(enc.cfg['eps']), None,
                                 out.data_ptr(), B * L, D, stream())
    assert rc == 0, lib.ezdit_last_error()
    assert np.array_equal(np_(out).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(np_(x_out), sd['shared.weight'][ids.reshape(-1)])


@pytest.mark.parametrize('L', [7, 100])
def test_one_layer_encode_is_the_nine_hooks_chained(lib, L):
    """configuration b with one layer, B = 3 with (1, 37, L) valid tokens: the nine launches of ezt5_encode, made through the hooks on the encoder's own weight blob, give
    ezt5_encode's output bit for bit -- which is what lets the kernel tests above speak for the encoder"""
    cfg = t5_ref.config('b', num_layers=1)
    sd, enc = _enc(cfg)
    B, D, H, F = 3, cfg['d_model'], cfg['num_heads'], cfg['d_ff']
    I, M, ml = 64 * H, B * L, enc.cfg['max_len']
    ids = t_(t5_ref.make_ids(cfg, B, L, 3).astype(np.int32))
    mask = t_(t5_ref.make_mask(B, L, (1, min(37, L), L)))
    want = np_(enc(input_ids=ids, attention_mask=mask).last_hidden_state).reshape(M, D)
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    x, xn, qkv, hff, out = z(M, D), z(M, D), z(M, 3 * I), z(M, 2 * F), z(M, D)
    u, ao, g = z(M, D, dt=torch.bfloat16), z(M, I, dt=torch.bfloat16), z(M, F, dt=torch.bfloat16)
    eps, st, P = C.c_float(enc.cfg['eps']), stream(), lambda t: t.data_ptr()
    rcs = [lib.ezt5_test_embed_rms(P(ids), _slot(enc, 'embed'), cfg['vocab_size'], None, P(x), _slot(enc, 'blk0.ln0'), eps, P(u), None, M, D, st),
           lib.ezt5_test_gemm(P(u), D, _slot(enc, 'blk0.wqkv'), 3 * I, None, P(qkv), M, st),
           lib.ezt5_test_attention_ex(P(qkv), P(qkv) + 4 * I, P(qkv) + 8 * I, 1, 3 * I, _slot(enc, 'bias_table'), 2 * ml - 1, ml - 1, P(mask), P(ao), I, B, H, L, st),
           lib.ezt5_test_gemm(P(ao), I, _slot(enc, 'blk0.wo'), D, P(x), P(xn), M, st),
           lib.ezt5_test_embed_rms(None, None, 0, P(xn), P(xn), _slot(enc, 'blk0.ln1'), eps, P(u), None, M, D, st),
           lib.ezt5_test_gemm(P(u), D, _slot(enc, 'blk0.wi'), 2 * F, None, P(hff), M, st),
           lib.ezt5_test_gated_gelu(P(hff), P(g), M, F, st),
           lib.ezt5_test_gemm(P(g), F, _slot(enc, 'blk0.wff'), D, P(xn), P(x), M, st),
           lib.ezt5_test_embed_rms(None, None, 0, P(x), P(x), _slot(enc, 'final_ln'), eps, None, P(out), M, D, st)]
    assert rcs == [0] * 9, (rcs, lib.ezdit_last_error())
    assert np.array_equal(np_(out).view(np.uint32), want.view(np.uint32))


# ---- ezt5_encode per valid row ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', [7, 100, 130])
@pytest.mark.parametrize('name', ['a', 'b'])
def test_encode_per_valid_row(lib, name, L):
    """the whole-encode test of tests/test_t5_gpu.py, its cases and its judge, gated per valid ROW: the row's rel-L2 against the fp64 judge at most 2 x the same row's error
    of t5_ref.encode(emulate=True), plus that test's floor of 1e-6.  The single-token row (batch element 0: the empty prompt of every CFG pair) is named in the record."""
    from tests.test_t5_gpu import FLOOR, _case, _encoder, _run
    cfg, sd, enc = _encoder(name)
    ids, mask, ref, emu = _case(name, L)
    got = _run(enc, ids, mask)
    valid = mask.astype(bool)
    row = lambda a: np.linalg.norm(a - ref, axis=-1) / np.maximum(np.linalg.norm(ref, axis=-1), 1e-30)
    rg, re = row(got.astype(np.float64)), row(emu)
    ratio = np.where(valid, rg / (2 * re + FLOOR), 0.0)
    b, i = np.unravel_index(int(ratio.argmax()), ratio.shape)
    record(f't5 encode rows {name} L={L}: worst row (b={b}, token {i}) rel-L2 {rg[b, i]:.3e} (emulation {re[b, i]:.3e}, ratio to gate {ratio[b, i]:.3f}); '
           f'single-token row rel-L2 {rg[0, 0]:.3e} (emulation {re[0, 0]:.3e})')
    assert np.isfinite(got).all() and ratio.max() <= 1.0, (name, L, b, i, rg[b, i], re[b, i])
