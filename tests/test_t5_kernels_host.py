"""CPU tests of tests/t5_emul.py, the fixtures of the kernel-level T5 encoder tests (tests/test_t5_kernels_gpu.py): the fp32 emulation of every kernel stays inside every gate
in every case, every deliberate mistake is caught where it can be made, the recorded floors are the emulation's, and the four hooks refuse what bounds an address without
touching a GPU.

A mistake counts as caught where it exceeds a gate MUT_FACTOR = 3 times over or breaks a bitwise check; it must be caught in at least 90 % of the cases in which it can be made,
for both operand forms.  The cases in which a mistake cannot show are listed in the docstring of tests/t5_emul.py and decided by attn_applies / NormCase.applies /
GeluCase.applies: the bias mistakes at L = 1 (one key), bias_half_Lm1 at max_len = L, key_L_admitted at L % 64 == 0, mask_ignored_last_tile without a masked key in the last
tile, max_over_masked without the underflow construction, halves_not_combined and key_order_mismatch at L <= 4, stride_64H and truncation in the bf16 form; eps mistakes away
from the stream scale 1e-4 (eps_omitted also shows on the zero row), neighbour_row and row_stride_F at one row, id mistakes on the x_in paths."""
import numpy as np
import pytest

from tests import t5_emul as E

NEED = 0.9


def test_attention_cases_cover_what_they_claim():
    """every mask kind occurs, every case has a different mask per batch element (L >= 31) and one empty element, bias_half != L - 1 is exercised, the two-pass maximum matters
    (rows whose maximum lies in the LAST key tile, rows whose maximum lies in the first) and the underflow construction occurs"""
    kinds, last, first, under = set(), 0, 0, 0
    for L, ml in E.attn_specs():
        c = E.attn_case(L, ml)
        assert c.B * c.H <= 12 and 'empty' in c.kinds and not c.mask[c.empty].any()
        kinds |= set(c.kinds)
        if L >= 31:
            assert len({m.tobytes() for m in c.mask}) == c.B, c.id()
        lo = c.bias_half - (L - 1)
        assert np.isfinite(c.table[:, lo:lo + 2 * L - 1]).all() and np.isnan(c.table[:, :lo]).all() and np.isnan(c.table[:, lo + 2 * L - 1:]).all()
        st = {}
        c.emul('f32', stats=st)
        last, first, under = last + st['max_in_last_tile'], first + st['max_in_first_tile'], under + st['underflow_rows']
        assert (st['underflow_rows'] > 0) == c.underflow, c.id()
        if L >= 65:
            assert st['max_in_last_tile'] > 0 and st['max_in_first_tile'] > 0, c.id()
    assert kinds == set(E.MASK_KINDS) | {'empty'}
    assert {ml for _, ml in E.attn_specs()} >= {300, 512} and any(ml == L for L, ml in E.attn_specs())
    assert last > 0 and first > 0 and under > 0


def test_attention_gates_are_twice_the_recorded_floors_and_the_record_is_the_emulation():
    """the gates of the GPU test are 2 x ATTN_FLOORS, nothing else, and ATTN_FLOORS is what the emulation gives over all cases (worst of exp exact, +-1 and +-2 ulp)"""
    fl = E.attn_floors()
    for k, v in E.ATTN_FLOORS.items():
        print(f't5 attention floor {k}: recorded {v:.3e} emulated {fl[k]:.4e}')
        assert abs(fl[k] / v - 1) <= 0.05, (k, v, fl[k])
        assert E.attn_gates()[k] == 2.0 * v
    assert E.ATTN_GATE_FACTOR == 2.0 and E.MUT_FACTOR == 3.0


@pytest.mark.parametrize('L', E.ATTN_LENGTHS)
def test_attention_emulation_stays_inside_every_gate(L):
    for ml in E.attn_max_lens(L):
        c = E.attn_case(L, ml)
        for form in ('bf16', 'f32'):
            outs = [c.emul(form, exp_ulp=n) for n in (0, 1, 2)]
            for o in outs:
                assert c.bitwise_ok(o), (c.id(), form)
                assert E.attn_within(c, o, form), (c.id(), form, c.measure(o, 'a'))
        # the two forms are the same numbers: the fp32 loader rounds to the bf16 form's operands
        assert np.array_equal(c.emul('bf16').view(np.uint32), c.emul('f32').view(np.uint32))


@pytest.mark.parametrize('form', ['bf16', 'f32'])
def test_every_attention_mistake_is_caught(form):
    rates = {}
    for mut in E.ATTN_MUTANTS:
        hit = tot = 0
        for L, ml in E.attn_specs():
            c = E.attn_case(L, ml)
            if not E.attn_applies(c, form, mut):
                continue
            tot += 1
            hit += bool(E.attn_caught(c, c.emul(form, mut), form))
        rates[mut] = (hit, tot)
    print(form, rates)
    for mut, (hit, tot) in rates.items():
        if mut in ('stride_64H', 'truncation') and form == 'bf16':
            assert tot == 0
            continue
        assert tot >= 20 and hit >= NEED * tot, (form, mut, hit, tot)


def test_a_mistake_that_cannot_show_does_not_show():
    """the statements of attn_applies, checked where they are cheap: the mistake gives the bits of the emulation, or stays inside the gates"""
    c = E.attn_case(1, 300)
    for mut in ('bias_omitted', 'bias_query_minus_key', 'bias_of_head0', 'halves_not_combined', 'key_order_mismatch', 'scale_applied'):
        assert np.array_equal(c.emul('f32', mut).view(np.uint32), c.emul('f32').view(np.uint32)), mut
    c = E.attn_case(100, 100)
    assert np.array_equal(c.emul('f32', 'bias_half_Lm1').view(np.uint32), c.emul('f32').view(np.uint32))
    c = E.attn_case(64, 300)
    assert np.array_equal(c.emul('bf16', 'stride_64H').view(np.uint32), c.emul('bf16').view(np.uint32))


# ---- norm ---------------------------------------------------------------------------------------------------------------------------
def _norm_verdict(c, path, mut=None, rsq_ulp=0):
    res, xo = c.emul(path, mut, rsq_ulp)
    xp = c.emul(path.replace('ids', 'x'), rsq_ulp=rsq_ulp)[0] if path.startswith('ids') else None
    return c.verdict(path, res, xo, xp)


@pytest.mark.parametrize('D', E.NORM_D)
def test_norm_emulation_stays_inside_every_gate(D):
    """one bf16 ulp, the share cap and the derived fp32 bound with the reciprocal square root exact and one ulp off either way; numpy float32 of the same operation stays
    under a third of the share cap (the cap is a condition on the kernel, not a measurement of it)"""
    for M in E.NORM_M:
        for s in E.NORM_SCALES:
            c = E.norm_case(D, M, s)
            assert set(c.ids.tolist()) >= ({E.ENERGY_ROW} if M < 7 else {0, c.V - 1, -1, c.V + 5, E.ENERGY_ROW, E.ZERO_ROW})
            for path in E.NORM_PATHS:
                for n in (0, -1, 1):
                    bit, err, share = _norm_verdict(c, path, rsq_ulp=n)
                    assert bit and err <= 1.0 and share <= 1.0, (c.id(), path, n, err, share)
            x = c.x
            with np.errstate(invalid='ignore'):
                o = x / np.sqrt((x * x).mean(-1, keepdims=True, dtype=np.float32) + np.float32(E.NORM_EPS)) * c.w
            cap, _ = c.share_cap()
            assert E.not_equal_count(E.bf16r(o), c.ref()) / o.size <= cap / 3, c.id()
            if c.has_zero:
                z = int(np.flatnonzero(c.ids == E.ZERO_ROW)[0])
                assert (c.emul('x_f32')[0][z] == 0).all()


def test_every_norm_mistake_is_caught():
    for mut in E.NORM_MUTANTS:
        for path in E.NORM_PATHS:
            hit = tot = 0
            for spec in E.norm_specs():
                c = E.norm_case(*spec)
                if not c.applies(path, mut):
                    continue
                tot += 1
                hit += bool(E.norm_caught(*_norm_verdict(c, path, mut)))
            if mut.startswith('id_') and path.startswith('x'):
                assert tot == 0
                continue
            assert tot >= 30 and hit >= NEED * tot, (mut, path, hit, tot)


def test_norm_bound_is_the_stated_operation_count():
    assert E.norm_f32_rel(64) == ((4 * 1 + 9) / 2 + 5) * 2.0 ** -24 * 1.01
    assert E.norm_f32_rel(260) == ((4 * 2 + 9) / 2 + 5) * 2.0 ** -24 * 1.01
    assert E.norm_f32_rel(2048) == ((4 * 8 + 9) / 2 + 5) * 2.0 ** -24 * 1.01


# ---- gated GELU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F', E.GELU_F)
def test_gelu_emulation_stays_inside_the_gate_and_every_mistake_is_caught(F):
    for M in E.GELU_M:
        c = E.gelu_case(M, F)
        a, b = c.ab()
        assert (np.abs(a) <= 6).mean() > 0.6 and np.abs(a).max() >= 1e20 and (a == 0).sum() >= 2 and ((a != 0) & (np.abs(a) < 1e-38)).any()
        assert (b > 0).any() and (b < 0).any() and np.abs(b).min() >= 1e-3 and np.abs(b).max() <= 1e4
        assert np.isfinite(c.ref()).all() and c.sel().mean() > 0.5
        for k in (0, 1, 2):
            fin, err, share = c.verdict(c.emul(tanh_ulp=k))
            assert fin and err <= 1.0 and share <= 1.0, (c.id(), k, err, share)
        with np.errstate(all='ignore'):
            o = (np.float32(0.5) * a * (np.float32(1) + np.tanh(np.float32(E.GELU_C) * (a + np.float32(E.GELU_A) * a * a * a)))) * b
        cap, _ = c.share_cap()
        assert c.not_equal(E.bf16r(o)) / int(c.sel().sum()) <= cap / 3, c.id()
        for mut in E.GELU_MUTANTS:
            if c.applies(mut):
                assert E.norm_caught(*c.verdict(c.emul(mut))), (c.id(), mut)      # every case, not 90 %


# ---- GEMM ---------------------------------------------------------------------------------------------------------------------------
def test_gemm_cases_and_bound():
    """the eight projection shapes; an fp32 product of the same operands is inside the derived bound, a product that loses the residual or the last K tile is far outside"""
    shapes = E.gemm_shapes()
    assert [s[1:] for s in shapes] == [(384, 192, False), (192, 128, True), (512, 192, False), (192, 256, True),
                                       (1088, 2048, False), (1088, 2048, True), (1088, 2048, False), (1088, 5120, True)]
    for name, N, K, res in shapes:
        c = E.GemmCase(name, N, K, res, 5)
        ref, bound = c.ref_and_bound()
        a, w = c.A[E.GUARD:E.GUARD + 5], c.W
        got = a @ w.T + (c.resid if res else 0)
        assert E.worst_ratio(got, ref, bound) <= 1.0
        assert E.worst_ratio(a[:, :K - 64] @ w[:, :K - 64].T + (c.resid if res else 0), ref, bound) > 3
        if res:
            assert E.worst_ratio(a @ w.T, ref, bound) > 3 and float(np.abs(c.resid).max()) > 1e4


# ---- hooks --------------------------------------------------------------------------------------------------------------------------
def test_hooks_refuse_what_bounds_an_address_before_any_gpu_call(lib):
    """no GPU here: every refusal below is decided on the host.  The pointers are never dereferenced."""
    p = 1 << 20
    att = lambda **k: lib.ezt5_test_attention_ex(*[{**dict(q=p, k=p, v=p, f32=0, ld=192, bias=p, bias_ld=199, bias_half=99, mask=p, out=p, ldo=200, B=2, H=3, L=100, st=None), **k}[n]
                                                  for n in ('q', 'k', 'v', 'f32', 'ld', 'bias', 'bias_ld', 'bias_half', 'mask', 'out', 'ldo', 'B', 'H', 'L', 'st')])
    for bad in (dict(q=None), dict(mask=None), dict(out=None), dict(B=0), dict(H=0), dict(L=0), dict(B=65536), dict(ld=191), dict(ld=184), dict(ld=196), dict(ldo=191),
                dict(ldo=198), dict(bias_half=98), dict(bias_ld=198), dict(q=p + 8), dict(out=p + 4)):
        assert att(**bad) == -1, bad
    assert att(L=513, bias_ld=1025, bias_half=512) == -2
    rms = lambda **k: lib.ezt5_test_embed_rms(*[{**dict(ids=None, emb=None, vocab=0, x_in=p, x_out=None, w=p, eps=1e-6, u=p, o=None, M=3, D=64, st=None), **k}[n]
                                                for n in ('ids', 'emb', 'vocab', 'x_in', 'x_out', 'w', 'eps', 'u', 'o', 'M', 'D', 'st')])
    for bad in (dict(ids=p), dict(x_in=None), dict(o=p), dict(u=None), dict(w=None), dict(D=66), dict(D=0), dict(M=0), dict(ids=p, x_in=None, emb=p, x_out=p, vocab=0),
                dict(ids=p, x_in=None, emb=None, x_out=p, vocab=5), dict(ids=p, x_in=None, emb=p, x_out=None, vocab=5), dict(x_in=p + 4)):
        assert rms(**bad) == -1, bad
    for args in ((None, p, 3, 64), (p, None, 3, 64), (p, p, 0, 64), (p, p, 3, 0), (p, p, 3, 66), (p + 4, p, 3, 64)):
        assert lib.ezt5_test_gated_gelu(*args, None) == -1, args
    assert lib.ezt5_test_gemm(None, 64, p, 64, None, p, 3, None) == -1
    assert lib.ezt5_test_gemm(p, 64, p, 64, None, p, 0, None) == -1
    assert lib.ezt5_test_gemm(p, 100, p, 64, None, p, 3, None) == -2 and b'GEMM refuses' in lib.ezdit_last_error()
    assert lib.ezt5_test_gemm(p, 64, p, 66, None, p, 3, None) == -2
    assert lib.ezt5_test_gemm(p, 1 << 20, p, 4096, None, p, 3, None) == -2
