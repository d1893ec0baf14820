"""Sliding-window self-attention, one launch at a time against fp64 (run with -m gpu on an MI355X): the BAND instantiations of k_attn (csrc/attn.hip) through
ezdit_test_attention_band.  Inputs, the reference, the fp32 emulation, the deliberate mistakes and the gates with their emulated floors: tests/attn_band_emul.py
(tests/test_attention_band_host.py holds the gates against the emulation on the CPU).  The shapes are the smallest at which each edge of the band exists."""
import pytest
import torch

from oracle.weights import make_state_dict, model_config
from tests import attn_band_emul as BE
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


def _launch(lib, m, c, dev, b0=0, B=None, plain=False):
    """one launch over the batch elements [b0, b0 + B) of the case, as a batch of its own; returns the output buffer [B L + PAD_ROWS][ldD] (bf16, prefilled) on the CPU.
    plain: the same inputs through ezdit_test_attention (no band, no lengths)"""
    B = c.B if B is None else B
    sl = slice(b0, b0 + B)
    q, k, v = (t[sl].contiguous().to(dev) for t in (c.q, c.k, c.v))
    out = torch.full((B * c.Lq + AE.PAD_ROWS, c.ldD), AE.SENTINEL, dtype=torch.bfloat16, device=dev)
    if plain:
        rc = lib.ezdit_test_attention(m._h, q.data_ptr(), k.data_ptr(), v.data_ptr(), None, out.data_ptr(), B, c.Lq, c.Lq, c.Lqp, c.Lqp, None)
    else:
        kl = torch.tensor(c.klen[sl], dtype=torch.int32, device=dev) if c.klen else None
        rc = lib.ezdit_test_attention_band(m._h, q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, c.Lq, c.Lqp, kl.data_ptr() if c.klen else None,
                                           c.radius, None)
    assert rc == 0, lib.ezdit_last_error()
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize('case', BE.BAND_CASES, ids=BE.case_id)
def test_band_attention_against_fp64_per_head_and_per_row(lib, dev, case):
    """Gates of tests/attn_band_emul.py: worst (batch element, head) rel-L2, worst query row of a head, max-abs, all against the fp64 softmax over each row's own keys.
    Bitwise: everything finite, query rows >= klen[b] exactly 0, the columns [D, ldD) and the rows behind B L still the prefill; the XCD-aware and the plain workgroup map give
    the same bits; every batch element launched alone gives the bits of its slice; and a radius of L - 1 (nothing masked) gives the bits of the plain kernel."""
    c = BE.band_case(*case)
    m = get_model(c.size)
    g = BE.gates(case)
    plain = None
    try:
        assert lib.ezdit_set_option(m._h, b'attn_nkh', c.nkh) == 0 and lib.ezdit_set_option(m._h, b'attn_xcd', 1) == 0
        out = _launch(lib, m, c, dev)
        alone = [_launch(lib, m, c, dev, b, 1) for b in range(c.B)]
        if c.radius >= c.Lq - 1 and not c.klen:
            plain = _launch(lib, m, c, dev, plain=True)
        assert lib.ezdit_set_option(m._h, b'attn_xcd', 0) == 0
        out0 = _launch(lib, m, c, dev)
    finally:
        assert lib.ezdit_set_option(m._h, b'attn_nkh', 0) == 0 and lib.ezdit_set_option(m._h, b'attn_xcd', 1) == 0
    f = c.figures(out)
    e = c.figures(c.emulated[0])
    record(f'band attention {BE.case_id(case)}: worst head rel-L2 {f["head"]:.3e} (emulated {e["head"]:.3e}, gate {g["head"]:.1e}), worst row {f["row"]:.3e} '
           f'(emulated {e["row"]:.3e}, gate {g["row"]:.1e}), max-abs {f["abs"]:.3e} (emulated {e["abs"]:.3e}, gate {g["abs"]:.1e})')
    assert f['finite'], 'non-finite output'
    assert f['zeros'], 'query rows beyond klen[b] must be exactly 0'
    assert f['cols'], 'columns [D, ldD) must keep the prefill'
    assert f['rows'], 'rows behind B L must keep the prefill'
    assert BE.within_gates(f, g), (f, g)
    assert torch.equal(_bits(out0), _bits(out)), 'attn_xcd 0 and 1 differ'
    for b, ob in enumerate(alone):
        assert torch.equal(_bits(ob[:c.Lq]), _bits(out[b * c.Lq:(b + 1) * c.Lq])), f'batch element {b} alone differs from its slice'
        assert bool((ob[c.Lq:].float() == AE.SENTINEL).all()), f'batch element {b} alone: rows behind L written'
    if plain is not None:
        assert torch.equal(_bits(plain), _bits(out)), 'the band form with nothing masked differs from the plain kernel'


def test_band_hook_refusals_leave_the_output_untouched(lib, dev):
    c = BE.band_case('xs', 130, 20, None, 2)
    m = get_model('xs')
    q, k, v = (t.to(dev) for t in (c.q, c.k, c.v))
    out = torch.full((c.B * c.Lq, c.ldD), AE.SENTINEL, dtype=torch.bfloat16, device=dev)

    def call(q_=q.data_ptr(), k_=k.data_ptr(), v_=v.data_ptr(), out_=out.data_ptr(), Lp=c.Lqp, radius=20):
        return lib.ezdit_test_attention_band(m._h, q_, k_, v_, out_, c.B, c.Lq, Lp, None, radius, None)
    for kw in (dict(radius=0), dict(radius=-4), dict(Lp=c.Lqp + 32), dict(Lp=c.Lq), dict(q_=None), dict(k_=None), dict(v_=None)):
        assert call(**kw) == -1 and lib.ezdit_last_error(), kw
    assert call(out_=None) == -1
    kl = torch.tensor([c.Lq + 1, 5], dtype=torch.int32, device=dev)
    assert lib.ezdit_test_attention_band(m._h, q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), c.B, c.Lq, c.Lqp, kl.data_ptr(), 20, None) == -1
    assert b'klen' in lib.ezdit_last_error()
    torch.cuda.synchronize()
    assert bool((out.float() == AE.SENTINEL).all())
