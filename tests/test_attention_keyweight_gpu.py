"""Prompt emphasis of cross-attention, one launch at a time against fp64 (run with -m gpu on an MI355X): the KW instantiations of k_attn (csrc/attn.hip) through
ezdit_test_attention_keyweights (plain 8-wave form) and ezdit_test_cross_attention_keyweights (fused projection, 32- and 64-row query tiles).  Inputs, the reference, the fp32
emulation, the deliberate mistakes and the gates with their emulated floors: tests/xattn_keyweight_emul.py (tests/test_attention_keyweight_host.py holds the gates against the
emulation on the CPU).  Masked K rows hold +3e4, their V rows -3e4 and their weights NaN in every case."""
import ctypes as C

import pytest
import torch

from oracle.weights import make_state_dict, model_config
from tests import attn_emul as AE
from tests import xattn_keyweight_emul as WE
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


def _launch(lib, c, dev, b0=0, nB=None, kw=True, keep_on=0, xcd=1):
    """one launch over the batch elements [b0, b0 + nB) of the case; returns the output buffer [B Lq + PAD_ROWS][ldD] (bf16, prefilled; the rows of batch element b at
    b Lq) on the CPU.  kw False: the hook without weights on the same inputs"""
    nB = c.B - b0 if nB is None else nB
    wa = _farr(c.w[b0:b0 + nB])
    out = torch.full((c.B * c.Lq + AE.PAD_ROWS, c.ldD), AE.SENTINEL, dtype=torch.bfloat16, device=dev)
    k, v, km = c.k.contiguous().to(dev), c.v.contiguous().to(dev), c.kmask.contiguous().to(dev)
    if c.form == 'plain':
        m = get_model(c.size)
        sl = slice(b0, b0 + nB)
        q = c.q[sl].contiguous().to(dev)
        o = out[b0 * c.Lq:]
        assert lib.ezdit_set_option(m._h, b'attn_xcd', xcd) == 0
        try:
            kk, vv, mm = k[sl].contiguous(), v[sl].contiguous(), km[sl].contiguous()
            args = (m._h, q.data_ptr(), kk.data_ptr(), vv.data_ptr(), mm.data_ptr(), o.data_ptr(), nB, c.Lq, c.Lk, c.Lqp, c.Lkp)
            if kw:
                rc = lib.ezdit_test_attention_keyweights(*args, wa, keep_on, None)
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
                nB, b0, c.H, c.dh, c.Lq, c.Lk, c.Lqp, c.Lkp, dv[4].data_ptr(), cc.rows_alloc, cc.zparts, D, 96, dv[5].data_ptr(), dv[6].data_ptr(), 1e-5, 1, c.qt, xcd)
        rc = lib.ezdit_test_cross_attention_keyweights(*args, wa, keep_on, None) if kw else lib.ezdit_test_cross_attention(*args, None)
    assert rc == 0, lib.ezdit_last_error()
    torch.cuda.synchronize()
    return out.cpu()


def _rows(buf, c, b):
    return buf[b * c.Lq:(b + 1) * c.Lq]


@pytest.mark.parametrize('case', WE.KW_CASES, ids=WE.case_id)
def test_keyweight_attention_against_fp64(lib, dev, case):
    """Gates of tests/xattn_keyweight_emul.py against the fp64 formula (plain form: worst head, worst row, max-abs; fused forms: same operand, true LayerNorm, max-abs).
    Bitwise: everything finite although every masked K / V row is poisoned and its weight NaN, the columns [D, ldD) and the rows behind B Lq still the prefill; the XCD-aware
    and the plain workgroup map give the same bits (the 32-row form exists with the map only); every batch element launched alone gives the bits of its slice."""
    c = WE.kw_case(*case)
    g = WE.gates(case)
    out = _launch(lib, c, dev)
    f = c.stats(out)
    e = c.stats(c.emulated[0])
    record(f'keyweight attention {WE.case_id(case)}: ' + ', '.join(f'{k} {f[k]:.3e} (emulated {e[k]:.3e}, gate {g[k]:.1e})' for k in WE.stat_keys(case)))
    assert f['finite'], 'non-finite output'
    assert f['cols'], 'columns [D, ldD) must keep the prefill'
    assert f['rows'], 'rows behind B Lq must keep the prefill'
    assert WE.within_gates(f, g), (f, g)
    if c.qt == 64:
        assert torch.equal(_bits(_launch(lib, c, dev, xcd=0)), _bits(out)), 'attn_xcd 0 and 1 differ'
    for b in range(c.B):
        ob = _launch(lib, c, dev, b, 1)
        assert torch.equal(_bits(_rows(ob, c, b)), _bits(_rows(out, c, b))), f'batch element {b} alone differs from its slice'
        keep = torch.ones(ob.shape[0], dtype=torch.bool); keep[b * c.Lq:(b + 1) * c.Lq] = False
        assert bool((ob[keep].float() == AE.SENTINEL).all()), f'batch element {b} alone: rows of other batch elements written'


@pytest.mark.parametrize('case', WE.UNIFORM_CASES, ids=WE.case_id)
def test_uniform_weights_kept_on_are_the_kernel_without_weights(lib, dev, case):
    """Every weight 3.0 is a table of zeros: with keep_on = 1 the KW instantiation runs over three key tiles, full and mixed path, and returns the bits of the hook without
    weights on the same inputs (ezdit_test_attention / ezdit_test_cross_attention); with keep_on = 0 the hook launches that plain instantiation itself.  Against fp64 as well."""
    c = WE.kw_case(*case)
    g = WE.gates(case)
    out = _launch(lib, c, dev, keep_on=1)
    f, e = c.stats(out), c.stats(c.emulated[0])
    record(f'keyweight attention {WE.case_id(case)}: ' + ', '.join(f'{k} {f[k]:.3e} (emulated {e[k]:.3e}, gate {g[k]:.1e})' for k in WE.stat_keys(case)))
    assert AE.bitwise_ok(f), f
    assert WE.within_gates(f, g), (f, g)
    plain = _launch(lib, c, dev, kw=False)
    assert torch.equal(_bits(plain), _bits(out)), 'a table of zeros in the KW instantiation differs from the kernel without weights'
    assert torch.equal(_bits(_launch(lib, c, dev, keep_on=0)), _bits(plain))


def test_keyweight_hook_refusals_leave_the_output_untouched(lib, dev):
    c = WE.kw_case('xs', 33, 384, 'g', 'plain', 64)
    m = get_model('xs')
    q, k, v, km = (t.to(dev) for t in (c.q, c.k, c.v, c.kmask))
    out = torch.full((c.B * c.Lq, c.ldD), AE.SENTINEL, dtype=torch.bfloat16, device=dev)

    def call(w=c.w, Lk=c.Lk, Lkp=c.Lkp, q_=q.data_ptr()):
        return lib.ezdit_test_attention_keyweights(m._h, q_, k.data_ptr(), v.data_ptr(), km.data_ptr(), out.data_ptr(), c.B, c.Lq, Lk, c.Lqp, Lkp, _farr(w), 1, None)
    j = [int(c.valid[b].nonzero()[0]) for b in range(c.B)]
    zero, neg, nan, inf, ratio = (c.w.clone() for _ in range(5))
    zero[0, j[0]] = 0.0
    neg[1, j[1]] = -0.5
    nan[2, j[2]] = float('nan')
    inf[1, j[1]] = float('inf')
    ratio[WE.GROUP.index('peak'), j[0]] = 0.25      # 2^20 over 2^-2
    for kw in (dict(w=zero), dict(w=neg), dict(w=nan), dict(w=inf), dict(w=ratio), dict(Lk=c.Lk - 28, Lkp=c.Lkp - 64), dict(q_=None)):
        assert call(**kw) == -1 and lib.ezdit_last_error(), kw
    assert call(w=torch.ones(c.B, 300), Lk=300, Lkp=320) == -2 and lib.ezdit_last_error()      # a padded length that is no multiple of the 128-key tile: no 8-wave form
    assert lib.ezdit_test_attention_keyweights(m._h, q.data_ptr(), k.data_ptr(), v.data_ptr(), km.data_ptr(), out.data_ptr(), c.B, c.Lq, c.Lk, c.Lqp, c.Lkp, None, 1, None) == -1
    torch.cuda.synchronize()
    assert bool((out.float() == AE.SENTINEL).all())
    assert call() == 0, lib.ezdit_last_error()
