"""Plain self-attention, one launch at a time against fp64 (run with -m gpu on an MI355X): k_attn<64 | 72, 2 | 4> of csrc/attn.hip through ezdit_test_attention (with and
without a key mask) and ezdit_test_attention_varlen (per-batch-element lengths).  Inputs, the reference, the fp32 emulation, the deliberate mistakes and the gates with their
emulated floors: tests/attn_emul.py (tests/test_attention_kernels_host.py holds the gates against the emulation on the CPU).  The shapes are the smallest at which each edge of
the kernel exists; nothing runs at the workload's size."""
import pytest
import torch

from oracle.weights import make_state_dict, model_config
from tests import attn_emul as AE
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


def _launch(lib, m, c, dev, b0=0, B=None):
    """one launch over the batch elements [b0, b0 + B) of the case, as a batch of its own; returns the output buffer [B Lq + PAD_ROWS][ldD] (bf16, prefilled) on the CPU"""
    B = c.B if B is None else B
    sl = slice(b0, b0 + B)
    q, k, v = (t[sl].contiguous().to(dev) for t in (c.q, c.k, c.v))
    out = torch.full((B * c.Lq + AE.PAD_ROWS, c.ldD), AE.SENTINEL, dtype=torch.bfloat16, device=dev)
    km = c.kmask[sl].contiguous().to(dev) if c.kmask is not None else None
    args = (m._h, q.data_ptr(), k.data_ptr(), v.data_ptr(), km.data_ptr() if km is not None else None, out.data_ptr(), B, c.Lq, c.Lk, c.Lqp, c.Lkp)
    if c.klen:
        kl = torch.tensor(c.klen[sl], dtype=torch.int32, device=dev)
        rc = lib.ezdit_test_attention_varlen(*args, kl.data_ptr(), None)
    else:
        rc = lib.ezdit_test_attention(*args, None)
    assert rc == 0, lib.ezdit_last_error()
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize('case', AE.ATTN_CASES, ids=AE.case_id)
def test_attention_against_fp64_per_head_and_per_row(lib, dev, case):
    """Gates of tests/attn_emul.py (twice the emulated floor): worst (batch element, head) rel-L2, worst query row of a head, max-abs, all against the fp64 softmax over the valid
    keys.  Bitwise: everything finite, query rows >= klen[b] exactly 0, the columns [D, ldD) and the rows behind B Lq still the prefill; the XCD-aware and the plain workgroup
    map give the same bits; every batch element launched alone gives the bits of its slice of the batched launch."""
    c = AE.attn_case(*case)
    m = get_model(c.size)
    try:
        assert lib.ezdit_set_option(m._h, b'attn_nkh', c.nkh) == 0 and lib.ezdit_set_option(m._h, b'attn_xcd', 1) == 0
        out = _launch(lib, m, c, dev)
        alone = [_launch(lib, m, c, dev, b, 1) for b in range(c.B)]
        assert lib.ezdit_set_option(m._h, b'attn_xcd', 0) == 0
        out0 = _launch(lib, m, c, dev)
    finally:
        assert lib.ezdit_set_option(m._h, b'attn_nkh', 0) == 0 and lib.ezdit_set_option(m._h, b'attn_xcd', 1) == 0
    f = c.figures(out)
    e = c.figures(c.emulated[0])
    record(f'attention {AE.case_id(case)}: worst head rel-L2 {f["head"]:.3e} (emulated {e["head"]:.3e}, gate {AE.GATE_HEAD:.1e}), worst row {f["row"]:.3e} '
           f'(emulated {e["row"]:.3e}, gate {AE.GATE_ROW:.1e}), max-abs {f["abs"]:.3e} (emulated {e["abs"]:.3e}, gate {AE.GATE_ABS:.1e})')
    assert f['finite'], 'non-finite output'
    assert f['zeros'], 'query rows beyond klen[b] must be exactly 0'
    assert f['cols'], 'columns [D, ldD) must keep the prefill'
    assert f['rows'], 'rows behind B Lq must keep the prefill'
    assert f['head'] < AE.GATE_HEAD and f['row'] < AE.GATE_ROW and f['abs'] < AE.GATE_ABS, f
    assert torch.equal(_bits(out0), _bits(out)), 'attn_xcd 0 and 1 differ'
    for b, ob in enumerate(alone):
        assert torch.equal(_bits(ob[:c.Lq]), _bits(out[b * c.Lq:(b + 1) * c.Lq])), f'batch element {b} alone differs from its slice'
        assert bool((ob[c.Lq:].float() == AE.SENTINEL).all()), f'batch element {b} alone: rows behind Lq written'


def test_a_key_mask_that_leaves_a_batch_element_without_a_key_is_refused(lib, dev):
    c = AE.attn_case('xs', 64, 20, 'kmask', 2)
    m = get_model('xs')
    q, k, v = (t.to(dev) for t in (c.q, c.k, c.v))
    out = torch.full((c.B * c.Lq, c.ldD), AE.SENTINEL, dtype=torch.bfloat16, device=dev)
    km = c.kmask.clone()
    km[1] = 0
    km = km.to(dev)
    for hook, tail in ((lib.ezdit_test_attention, (None,)), (lib.ezdit_test_attention_varlen, (None, None))):
        rc = hook(m._h, q.data_ptr(), k.data_ptr(), v.data_ptr(), km.data_ptr(), out.data_ptr(), c.B, c.Lq, c.Lk, c.Lqp, c.Lkp, *tail)
        assert rc == -1 and b'without a valid key' in lib.ezdit_last_error()
    torch.cuda.synchronize()
    assert bool((out.float() == AE.SENTINEL).all())
