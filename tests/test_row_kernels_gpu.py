"""The streaming kernels of csrc/rowops.hip / csrc/rowbody.h, one launch at a time against fp64 (run with -m gpu on an MI355X): the row operator (k_row, k_row_w<false>,
k_row_w<true>) through ezdit_test_row, the per-head LayerNorm + RoPE (k_headnorm) through ezdit_test_headnorm, the input assembly (k_assemble) through ezdit_test_assemble.
Inputs, references, the fp32 emulation, the deliberate mistakes and the gates with their emulated floors: tests/row_emul.py (tests/test_row_kernels_host.py holds the gates
against the emulation on the CPU).  Nothing runs at the workload's size: the shapes are the smallest at which each path can still go wrong."""
import ctypes as C

import pytest
import torch

from tests import row_emul as RE
from tests.util import record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return 'cuda:0'


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---------------------------------------------------------------------------------------------------
# row operator
# ---------------------------------------------------------------------------------------------------
class _RowDev:
    """device copies of one tests/row_emul.py RowCase: every input PAD_ROWS rows longer than M with NaN there, slabs with rows of D + 8 (NaN in the 8), tables with NaN
    between the slots"""

    def __init__(self, c, dev):
        self.c = c
        M, D = c.M, c.D
        up = lambda t: None if t is None else RE.pad_rows(t).to(dev)
        self.h_in = up(c.h_in)
        self.ld_part = D + 8
        self.parts = None
        if c.mode != RE.COPY and c.nsplit > 0:
            p = torch.full((c.nsplit, M + RE.PAD_ROWS, self.ld_part), RE.NAN, dtype=c.parts.dtype)
            p[:, :M, :D] = c.parts
            self.parts = p.to(dev)
        self.bias = c.bias_v.to(dev) if c.bias else None
        self.gate = c.gate_t.to(dev) if c.gate else None
        self.ln_g, self.ln_c = c.ln_g.to(dev), c.ln_c.to(dev)
        self.skip, self.cn = up(c.skip), up(c.cn)
        self.cn_tab = c.cn_tab.to(dev) if c.cn_tab is not None else None
        self.cur = None if c.static else torch.tensor([c.cur_step], dtype=torch.int32, device=dev)
        self.rs = None if c.static else c.row_slot.to(dev)
        self.dev = dev

    def launch(self, lib, variant, affine=0, wt=0, h_out=True, u=True, cn_tab=True, n_slots=None):
        """one launch; returns (rc, h_out [M + PAD_ROWS][D] or None, u [M + PAD_ROWS][ld_u] or None) on the CPU.  Outputs start as the sentinel (in place: as h_in)."""
        from ezaudio_amd import _lib
        c = self.c
        rows = c.M + RE.PAD_ROWS
        ho = uo = None
        if h_out and c.h_out:
            ho = self.h_in.clone() if c.inplace else torch.full((rows, c.D), RE.SENTINEL, device=self.dev)
        if u and c.u:
            uo = torch.full((rows, c.ld_u), RE.SENTINEL, dtype=torch.bfloat16, device=self.dev)
        h_in = ho if (c.inplace and ho is not None) else self.h_in
        a = _lib.EzditTestRowArgs()
        a.h_in, a.h_out = _ptr(h_in), _ptr(ho)
        a.part, a.nsplit, a.ld_part, a.part_stride, a.part_bf16, a.mode = _ptr(self.parts), c.nsplit, self.ld_part, rows * self.ld_part, int(c.part_bf16), c.mode
        a.bias, a.gate, a.gate_slot_stride = _ptr(self.bias), _ptr(self.gate), 0 if c.static else c.D + c.stride_pad
        a.ln_g, a.ln_c, a.ln_slot_stride = _ptr(self.ln_g), _ptr(self.ln_c), 0 if c.static else c.width + c.stride_pad
        a.skip, a.cn, a.cn_tab, a.cn_scale, a.ld_u = _ptr(self.skip), _ptr(self.cn), _ptr(self.cn_tab) if cn_tab else None, c.cn_scale, c.ld_u
        a.u = _ptr(uo)
        a.M, a.D, a.L, a.n_slots = c.M, c.D, c.L, self.ln_g.shape[0] if n_slots is None else n_slots
        a.cur_step, a.row_slot = _ptr(self.cur), _ptr(self.rs)
        a.wt, a.variant, a.affine = wt, variant, affine
        rc = lib.ezdit_test_row(C.byref(a), None)
        torch.cuda.synchronize()
        return rc, (ho.cpu() if ho is not None else None), (uo.cpu() if uo is not None else None)


def _check_row(c, h, u, what):
    """one launch's outputs against the fp64 reference of the case"""
    M, D, W = c.M, c.D, c.width
    h64, u64 = c.ref
    if h is not None:
        got = h[:M]
        assert torch.isfinite(got).all(), f'{what}: h_out not finite'
        if c.mode == RE.COPY:
            assert torch.equal(_bits(got), _bits(c.h_in)), f'{what}: COPY is not bit-exact'
        elif c.mode == RE.SET and not c.part_bf16 and c.nsplit == 1 and not c.bias:
            assert torch.equal(got, c.parts[0]), f'{what}: SET of one fp32 slab is not bit-exact'
        err, bound = (got.double() - h64).abs(), c.h_bound()
        ratio = float((err / bound.clamp_min(1e-300)).max()) if float(bound.max()) > 0 else 0.0
        record(f'{what}: h_out worst error / bound {ratio:.3f} (fp32 summation bound x 2), rel-L2 {RE.rel_l2(got, h64):.2e}')
        assert (err <= bound).all(), (what, ratio)
        tail = h[M:]
        if c.inplace:
            assert torch.isnan(tail).all(), f'{what}: rows >= M of the in-place stream written'
        else:
            assert (tail == RE.SENTINEL).all(), f'{what}: rows >= M of h_out written'
    if u is not None:
        got = u[:M, :W].float()
        assert torch.isfinite(got).all(), f'{what}: u not finite'
        assert (u[:M, W:].float() == 0).all(), f'{what}: columns [width, ld_u) are not zero'
        assert (u[M:].float() == RE.SENTINEL).all(), f'{what}: rows >= M of u written'
        gate = RE.GATE_ROW_U_D4 if D == 4 else RE.GATE_ROW_U
        wr, ex = RE.worst_row_rel(got, u64), RE.u_excess(got, u64, c.u_scale())
        n = RE.not_equal_count(got, u64)
        n_e = max(RE.not_equal_count(e[1], u64) for e in c.emul3)
        cap = RE.share_cap(n_e, got.numel())
        record(f'{what}: u worst row rel-L2 {wr:.3e} (gate {gate:.1e}), whole {RE.rel_l2(got, u64):.3e}, excess over half an ulp {ex:.2e} (|g| + |c|) (gate {RE.A_REL:.1e}), '
               f'not bit-equal {n / got.numel():.2e} (emulation {n_e / got.numel():.2e}, cap {cap:.2e})')
        assert wr < gate, (what, wr)
        assert ex <= RE.A_REL, (what, ex)
        assert n / got.numel() <= cap, (what, n, n_e)
        if 'constant' in c.rows and c.exact_rows:
            r = c.rows['constant']
            want = c.ln_c[c.slot[r], :W].to(torch.bfloat16).float()
            assert torch.equal(got[r], want), f'{what}: the constant row is not bf16(ln_c)'
            assert (got[r][want == 0] == 0).all()


@pytest.mark.parametrize('spec', RE.ROW_CASES, ids=RE.row_id)
def test_row_operator_against_fp64(lib, dev, spec):
    """ezdit_test_row on one case of tests/row_emul.py ROW_CASES, in the workgroup-per-row form (variant 0) and the wave-per-row form (variant 1; D > 1280, more than 4 bf16
    slabs or more than 1 fp32 slab: launch_row takes the workgroup form there too).  Per launch: h_out elementwise within (nsplit + 3) 2^-23 (|h_in| + |gate| (sum |part_s| +
    |bias|)), COPY and SET of one fp32 slab bit-exact; u per ROW under the rel-L2 gate, every element within 2^-8 |ref| + A_REL (|ln_g| + |ln_c|), the share of elements not
    bit-equal to bf16(ref) at most ULP_SHARE_CAP x the emulation's (+ the Poisson allowance); the constant row equal to bf16(ln_c); columns [width, ld_u) zero; rows >= M of
    both outputs untouched.  Across launches, bitwise: write-through stores on / off, the XCD-affine row map on / off, h_out or u not requested, cn_tab of the scalar's value
    against the scalar."""
    c = RE.row_case(spec)
    d = _RowDev(c, dev)
    base = {}
    for variant in (0, 1):
        what = f'row {RE.row_id(spec)} variant {variant}'
        rc, h, u = d.launch(lib, variant)
        assert rc == 0, lib.ezdit_last_error()
        _check_row(c, h, u, what)
        base[variant] = (h, u)
        same = lambda x, y: (x is None and y is None) or torch.equal(_bits(x), _bits(y))
        rc, h2, u2 = d.launch(lib, variant, wt=1)
        assert rc == 0 and same(h, h2) and same(u, u2), f'{what}: write-through stores change the result'
        if variant == 1:
            rc, h2, u2 = d.launch(lib, variant, affine=1, wt=1)
            assert rc == 0 and same(h, h2) and same(u, u2), f'{what}: the XCD-affine row map changes the result'
        if h is not None and u is not None:
            rc, h2, u2 = d.launch(lib, variant, h_out=False)
            assert rc == 0 and h2 is None and same(u, u2), f'{what}: u changes when h_out is not stored'
            if not c.concat:      # (the concatenation exists for the LayerNorm only: the hook refuses skip without u)
                rc, h2, u2 = d.launch(lib, variant, u=False)
                assert rc == 0 and u2 is None and same(h, h2), f'{what}: h_out changes when u is not requested'
        if c.concat == 'tab_eq':
            rc, h2, u2 = d.launch(lib, variant, cn_tab=False)
            assert rc == 0 and same(h, h2) and same(u, u2), f'{what}: a cn_tab of equal values does not give the bits of the scalar'


def test_row_hook_refuses_slots_outside_the_tables(lib, dev):
    """the slot check needs the device's cur_step / row_slot: cur_step 2 + row_slot up to 2 needs 5 slots"""
    c = RE.row_case(dict(D=64, M=133, mode=RE.RES, nsplit=2, bias=True, gate=True, B=3, cur_step=2))
    d = _RowDev(c, dev)
    rc, h, u = d.launch(lib, 1, n_slots=4)
    assert rc == -1 and b'slot' in lib.ezdit_last_error()
    assert (h == RE.SENTINEL).all() and (u.float() == RE.SENTINEL).all()      # nothing was launched
    assert d.launch(lib, 1, n_slots=5)[0] == 0


# ---------------------------------------------------------------------------------------------------
# head norm
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', RE.HEAD_CASES, ids=lambda t: 'H%d-dh%d-B%d-L%d-Lp%d-%s' % t)
def test_headnorm_against_fp64(lib, dev, case):
    """ezdit_test_headnorm in the three forms a forward builds: q + k + v with RoPE (ldx = 3 D), context k + v without q and without RoPE (ldx = 2 D), q alone (ldx = D).
    q, k per (batch element, head) under the rel-L2 gate and the bit-equal share rule; v bit-equal to bf16(x); the channels [dh, DQK) / [dh, DV), the rows [L, Lp) and the
    buffers of absent parts keep the sentinel.  The RoPE tables are float32(rope_tables64), uploaded: the kernel's own table generator is not under test here."""
    c = RE.head_case(*case)
    B, H, L, Lp, dh = c.B, c.H, c.L, c.Lp, c.dh
    x = RE.pad_rows(c.x).to(dev)
    aff = [t.to(dev) for t in (c.qn_w, c.qn_b, c.kn_w, c.kn_b)]
    cos, sin = RE.pad_rows(c.cos[:L].contiguous()).to(dev), RE.pad_rows(c.sin[:L].contiguous()).to(dev)
    out = {n: torch.full((B, H, Lp, c.DV if n == 'v' else c.DQK), RE.SENTINEL, dtype=torch.bfloat16, device=dev) for n in 'qkv'}
    present = c.parts()
    p = lambda n: out[n].data_ptr() if n in present else None
    rc = lib.ezdit_test_headnorm(x.data_ptr(), c.ldx, *c.cols, aff[0].data_ptr() if 'q' in present else None, aff[1].data_ptr() if 'q' in present else None,
                                 aff[2].data_ptr() if 'k' in present else None, aff[3].data_ptr() if 'k' in present else None,
                                 cos.data_ptr() if c.rope_on else None, sin.data_ptr() if c.rope_on else None, p('q'), p('k'), p('v'), B, H, L, Lp, dh, None)
    assert rc == 0, lib.ezdit_last_error()
    torch.cuda.synchronize()
    got = {n: t.cpu() for n, t in out.items()}
    what = f'headnorm {c!r}'
    for n in 'qkv':
        t = got[n].float()
        if n not in present:
            assert (t == RE.SENTINEL).all(), f'{what}: the absent part {n} was written'
            continue
        assert (t[:, :, L:] == RE.SENTINEL).all(), f'{what} {n}: rows [L, Lp) written'
        assert (t[:, :, :, dh:] == RE.SENTINEL).all(), f'{what} {n}: channels [dh, ..) written'
        val, ref = t[:, :, :L, :dh], c.ref[n]
        assert torch.isfinite(val).all()
        if n == 'v':
            assert torch.equal(val, RE.bf16r(ref.float())), f'{what}: v is not bf16(x)'
            continue
        w = RE.per_head_rel_qk(val, ref)
        cnt = RE.not_equal_count(val, ref)
        n_e = max(RE.not_equal_count(e[n], ref) for e in c.emul3)
        cap = RE.share_cap(n_e, val.numel())
        record(f'{what} {n}: worst head rel-L2 {w:.3e} (gate {RE.GATE_HEAD:.1e}), not bit-equal {cnt / val.numel():.2e} (emulation {n_e / val.numel():.2e}, cap {cap:.2e})')
        assert w < RE.GATE_HEAD, (what, n, w)
        assert cnt / val.numel() <= cap, (what, n, cnt, n_e)


# ---------------------------------------------------------------------------------------------------
# input assembly
# ---------------------------------------------------------------------------------------------------
def _assemble(lib, dev, c, lens=True):
    x = c.x.to(dev)
    gt = c.gt.to(dev) if c.gt is not None else None
    gm = c.gt_mask.to(dev) if c.gt_mask is not None else None
    me = c.mask_embed.to(dev)
    ln = c.lens.to(dev) if (lens and c.lens is not None) else None
    out = torch.full((c.B * c.L + RE.PAD_ROWS, c.ldo), RE.SENTINEL, dtype=torch.bfloat16, device=dev)
    rc = lib.ezdit_test_assemble(x.data_ptr(), c.x_rows, c.in_ch, _ptr(gt), _ptr(gm), me.data_ptr(), out.data_ptr(), c.ldo, c.B, c.C, c.L, _ptr(ln), None)
    torch.cuda.synchronize()
    return rc, out.cpu()


@pytest.mark.parametrize('case', RE.ASM_CASES, ids=lambda t: 'C%d-L%d-xrows%d-%s' % t)
def test_assemble_is_bit_equal_to_the_expected_operand(lib, dev, case):
    """ezdit_test_assemble: [x[b % x_rows] | gt where gt_mask == 0, else mask_embed | gt_mask channel 0, or 1 without gt | zeros], frames >= lens[b] zero rows although x / gt
    hold NaN there, the pre-assembled form a transpose + cast: bit-equal to bf16(expected) everywhere, padding columns included; and once without lens."""
    c = RE.AsmCase(*case)
    rc, out = _assemble(lib, dev, c)
    assert rc == 0, lib.ezdit_last_error()
    n = c.B * c.L
    want = c.expected().to(torch.bfloat16)
    assert torch.equal(_bits(out[:n]), _bits(want)), f'assemble {case}: {int((_bits(out[:n]) != _bits(want)).sum())} elements differ'
    assert (out[n:].float() == RE.SENTINEL).all()
    c2 = RE.AsmCase(*case, with_lens=False)
    rc, out = _assemble(lib, dev, c2)
    assert rc == 0 and torch.equal(_bits(out[:n]), _bits(c2.expected().to(torch.bfloat16)))


def test_assemble_hook_refuses_lengths_outside_the_frames(lib, dev):
    c = RE.AsmCase(8, 77, 4, 'plain')
    for bad in ([77, 0, 76, 2], [78, 1, 76, 2]):
        c.lens = torch.tensor(bad, dtype=torch.int32)
        rc, out = _assemble(lib, dev, c)
        assert rc == -1 and b'lens' in lib.ezdit_last_error()
        assert (out.float() == RE.SENTINEL).all()
