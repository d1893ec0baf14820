"""The prompt timeline of cross-attention, one launch at a time against fp64 (run with -m gpu on an MI355X): the TL instantiations of k_attn (csrc/attn.hip) through
ezdit_test_attention_timeline (plain 8-wave form) and ezdit_test_cross_attention_timeline (fused projection, 32- and 64-row query tiles).  Inputs, the reference, the fp32
emulation, the deliberate mistakes and the gates with their emulated floors: tests/xattn_timeline_emul.py (tests/test_attention_timeline_host.py holds the gates against the
emulation on the CPU).  K rows that no weighted query may see hold +3e4 and their V rows -3e4 in every case, whole unweighted prompts included."""
import ctypes as C

import pytest
import torch

from oracle.weights import make_state_dict, model_config
from tests import attn_emul as AE
from tests import xattn_timeline_emul as TE
from tests.util import record

pytestmark = pytest.mark.gpu

_models = {}


def get_model(size):
    from ezaudio_amd import MaskDiT
    if size not in _models:
        cfg = model_config(size)
        m = MaskDiT(device='cuda:0', **cfg)
        m.load_state_dict(make_state_dict(cfg, 1))
        _models[size] = m
    return _models[size]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return 'cuda:0'


def _bits(t):
    return t.contiguous().view(torch.int16)


def _farr(w):
    w = w.contiguous().float().reshape(-1)
    return (C.c_float * w.numel())(*w.tolist())


def _launch(lib, c, dev, b0=0, nB=None, prompt=None, tl=True, xcd=1, w=None):
    """one launch over the batch elements [b0, b0 + nB) of the case; returns the output buffer [B Lq + PAD_ROWS][ldD] (bf16, prefilled; the rows of batch element b at
    b Lq) on the CPU.  prompt = s: the context is prompt s alone (S = 1, Lk = 128).  tl False: the hook without a timeline on the same inputs.  w: weights [nB][S][Lq]
    (default: the case's, or ones for a single prompt)"""
    nB = c.B - b0 if nB is None else nB
    ks = slice(0, c.Lk) if prompt is None else slice(128 * prompt, 128 * prompt + 128)
    S, Lk = (TE.S, c.Lk) if prompt is None else (1, 128)
    if w is None:
        w = c.w[b0:b0 + nB] if prompt is None else torch.ones(nB, 1, c.Lq)
    wa = _farr(w)
    out = torch.full((c.B * c.Lq + AE.PAD_ROWS, c.ldD), AE.SENTINEL, dtype=torch.bfloat16, device=dev)
    k, v, km = c.k[:, :, ks].contiguous().to(dev), c.v[:, :, ks].contiguous().to(dev), c.kmask[:, ks].contiguous().to(dev)
    if c.form == 'plain':
        m = get_model(c.size)
        sl = slice(b0, b0 + nB)
        q = c.q[sl].contiguous().to(dev)
        o = out[b0 * c.Lq:]
        assert lib.ezdit_set_option(m._h, b'attn_xcd', xcd) == 0
        try:
            kk, vv, mm = k[sl].contiguous(), v[sl].contiguous(), km[sl].contiguous()
            args = (m._h, q.data_ptr(), kk.data_ptr(), vv.data_ptr(), mm.data_ptr(), o.data_ptr(), nB, c.Lq, Lk, c.Lqp, Lk)
            if tl:
                rc = lib.ezdit_test_attention_timeline(*args, wa, S, None)
            else:
                assert lib.ezdit_set_option(m._h, b'attn_nkh', 4) == 0
                rc = lib.ezdit_test_attention(*args, None)
        finally:
            assert lib.ezdit_set_option(m._h, b'attn_xcd', 1) == 0 and lib.ezdit_set_option(m._h, b'attn_nkh', 0) == 0
    else:
        cc, D, K = c.cons, c.D, c.xK
        M = c.B * c.Lq
        A = torch.zeros(M, K, dtype=torch.bfloat16); A[:, :D] = cc.A
        Wp = torch.zeros(K, K, dtype=torch.bfloat16); Wp[:D, :D] = cc.W
        dv = [t.to(dev) for t in (A, Wp, c.qn_w, c.qn_b, cc.stats, cc.G[cc.cur_step].contiguous(), cc.C[cc.cur_step].contiguous())]
        args = (dv[0].data_ptr(), K, dv[1].data_ptr(), K, K, K, dv[2].data_ptr(), dv[3].data_ptr(), k.data_ptr(), v.data_ptr(), km.data_ptr(), out.data_ptr(), c.ldD,
                nB, b0, c.H, c.dh, c.Lq, Lk, c.Lqp, Lk, dv[4].data_ptr(), cc.rows_alloc, cc.zparts, D, 96, dv[5].data_ptr(), dv[6].data_ptr(), 1e-5, 1, c.qt, xcd)
        rc = lib.ezdit_test_cross_attention_timeline(*args, wa, S, None) if tl else lib.ezdit_test_cross_attention(*args, None)
    assert rc == 0, lib.ezdit_last_error()
    torch.cuda.synchronize()
    return out.cpu()


def _rows(buf, c, b):
    return buf[b * c.Lq:(b + 1) * c.Lq]


@pytest.mark.parametrize('case', TE.TL_CASES, ids=TE.case_id)
def test_timeline_attention_against_fp64(lib, dev, case):
    """Gates of tests/xattn_timeline_emul.py against the fp64 formula (plain form: worst head, worst row, max-abs; fused forms: same operand, true LayerNorm, max-abs).
    Bitwise: everything finite although every K / V row that no weighted query may see is poisoned, the columns [D, ldD) and the rows behind B Lq still the prefill;
    the XCD-aware and the plain workgroup map give the same bits (the 32-row form exists with the map only); every batch element launched alone gives the bits of its slice."""
    c = TE.tl_case(*case)
    g = TE.gates(case)
    out = _launch(lib, c, dev)
    f = c.stats(out)
    e = c.stats(c.emulated[0])
    record(f'timeline attention {TE.case_id(case)}: ' + ', '.join(f'{k} {f[k]:.3e} (emulated {e[k]:.3e}, gate {g[k]:.1e})' for k in TE.stat_keys(case)))
    assert f['finite'], 'non-finite output'
    assert f['cols'], 'columns [D, ldD) must keep the prefill'
    assert f['rows'], 'rows behind B Lq must keep the prefill'
    assert TE.within_gates(f, g), (f, g)
    if c.qt == 64:
        assert torch.equal(_bits(_launch(lib, c, dev, xcd=0)), _bits(out)), 'attn_xcd 0 and 1 differ'
    for b in range(c.B):
        ob = _launch(lib, c, dev, b, 1)
        assert torch.equal(_bits(_rows(ob, c, b)), _bits(_rows(out, c, b))), f'batch element {b} alone differs from its slice'
        keep = torch.ones(ob.shape[0], dtype=torch.bool); keep[b * c.Lq:(b + 1) * c.Lq] = False
        assert bool((ob[keep].float() == AE.SENTINEL).all()), f'batch element {b} alone: rows of other batch elements written'


@pytest.mark.parametrize('case', TE.ONES_CASES, ids=TE.case_id)
def test_fused_forms_walk_three_key_tiles_with_every_weight_one(lib, dev, case):
    """The multi-tile loop of the fused-projection forms (Lk = 384; the shipped model runs them at one key tile): every weight 1, so the timeline masks nothing -- against
    fp64 at the gates of the fused forms, and bit for bit the same kernel without the TL switch on the same inputs."""
    c = TE.tl_case(*case)
    g = TE.gates(case)
    out = _launch(lib, c, dev)
    f, e = c.stats(out), c.stats(c.emulated[0])
    record(f'timeline attention {TE.case_id(case)}: ' + ', '.join(f'{k} {f[k]:.3e} (emulated {e[k]:.3e}, gate {g[k]:.1e})' for k in TE.stat_keys(case)))
    assert AE.bitwise_ok(f), f
    assert TE.within_gates(f, g), (f, g)
    assert torch.equal(_bits(_launch(lib, c, dev, tl=False)), _bits(out)), 'every weight 1 differs from the kernel without a timeline'


@pytest.mark.parametrize('form,qt', [('plain', 64), ('fused', 32), ('fused', 64)])
@pytest.mark.parametrize('size', ['xs', 'xs64'])
def test_one_prompt_with_weight_one_is_the_kernel_without_a_timeline(lib, dev, size, form, qt):
    """S = 1 with weight 1 everywhere takes the paths and returns the bits of the instantiation without TL (ezdit_test_attention / ezdit_test_cross_attention), on each
    prompt of the case as the only context; and case `one` -- prompt 1 alone weighted in a context of three -- returns the bits of the plain hook on prompt 1's keys alone."""
    for Lq in TE.LQS:
        c = TE.tl_case(size, Lq, 'b', form, qt)
        for s in range(TE.S):
            a, b_ = _launch(lib, c, dev, prompt=s), _launch(lib, c, dev, prompt=s, tl=False)
            assert bool(torch.isfinite(a.float()).all())
            assert torch.equal(_bits(a), _bits(b_)), f'Lq {Lq}, prompt {s}: S = 1 with weight 1 differs from the kernel without a timeline'
        b = TE.GROUPS['b'].index('one')
        three = _launch(lib, c, dev, b, 1)
        alone = _launch(lib, c, dev, b, 1, prompt=1, tl=False)
        assert torch.equal(_bits(_rows(three, c, b)), _bits(_rows(alone, c, b))), f'Lq {Lq}: prompt 1 weighted alone differs from the plain kernel on its keys'


def test_timeline_hook_refusals_leave_the_output_untouched(lib, dev):
    c = TE.tl_case('xs', 33, 'a', 'plain', 64)
    m = get_model('xs')
    q, k, v, km = (t.to(dev) for t in (c.q, c.k, c.v, c.kmask))
    out = torch.full((c.B * c.Lq, c.ldD), AE.SENTINEL, dtype=torch.bfloat16, device=dev)

    def call(w=c.w, S=TE.S, Lk=c.Lk, Lkp=c.Lkp, q_=q.data_ptr()):
        return lib.ezdit_test_attention_timeline(m._h, q_, k.data_ptr(), v.data_ptr(), km.data_ptr(), out.data_ptr(), c.B, c.Lq, Lk, c.Lqp, Lkp, _farr(w), S, None)
    neg, nan, none = c.w.clone(), c.w.clone(), c.w.clone()
    neg[1, 0, 3] = -0.5
    nan[2, 1, 0] = float('nan')
    none[0, :, 7] = 0.0
    for kw in (dict(w=neg), dict(w=nan), dict(w=none), dict(S=2), dict(S=0), dict(S=17), dict(Lk=c.Lk - 28), dict(q_=None)):
        assert call(**kw) == -1 and lib.ezdit_last_error(), kw
    assert lib.ezdit_test_attention_timeline(m._h, q.data_ptr(), k.data_ptr(), v.data_ptr(), km.data_ptr(), out.data_ptr(), c.B, c.Lq, c.Lk, c.Lqp, c.Lkp, None, TE.S, None) == -1
    torch.cuda.synchronize()
    assert bool((out.float() == AE.SENTINEL).all())
    assert call() == 0, lib.ezdit_last_error()
