"""The un-split 8-wave form of the fused QKV GEMM (tile 67: k_gemm_pp<128, 2 dh, 8, 1, 4, EPI_QKV, SCHED 1>, csrc/gemm_pp.h), alone through `ezdit_test_consumer`
and inside the step (qkv_form = 1 is the default; `qkv_co` + 4 selects qkv_form = 0, the k-split form).  Run with -m gpu on an MI355X.

Kernel level: against float64 of the same bf16 operands and tables, the way tests/test_gpu.py::test_fused_qkv_gemm_consumer_against_fp64 does it -- the emulation
(tests/kernel_emul.py QkvCase) and its gates are reused unchanged; only the operand width K is freed from H dh, so that the smallest K-tile counts can be reached
with two heads per tile: K = 128 is 2 K tiles (fewer than the ring of 4: the prologue alone feeds the loop), K = 320 is 5 (the ring wraps, every tail variant of
the counted waits runs).  M = 130 is two row tiles, the second with 2 valid rows.  Each shape runs with the LayerNorm algebra on (VAR 64: statistics, G' / C') and
off (VAR 0: the plain projection of a finished operand; the "true LayerNorm" reference has no meaning there and is not compared).
Step level: the xs / s forwards and the smp_xs sampler loop at the gates of tests/test_gpu.py, equal launch counts for both forms."""
import numpy as np
import pytest
import torch

from oracle.weights import make_state_dict, model_config
from tests import kernel_emul as KE
from tests.util import DIFF, golden_case, record, rel_l2, sampler_case

pytestmark = pytest.mark.gpu

REL_TOL, ABS_TOL = 2e-2, 0.15   # tests/test_gpu.py
TILE = 67
QKV_CO_DEFAULT = 1              # tests/test_gpu.py DEFAULT_OPTS: co-resident kernel above 2048 rows, the un-split form (tile 67, qkv_form = 1) below
QKV_KSPLIT = 4                  # + 4: qkv_form = 0, the k-split form (tile 61) up to 2048 rows


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return 'cuda:0'


_models = {}


def get_model(size, seed):
    from ezaudio_amd import MaskDiT
    key = (size, seed)
    if key not in _models:
        cfg = model_config(size)
        m = MaskDiT(device='cuda:0', **cfg)
        m.load_state_dict(make_state_dict(cfg, seed))
        _models[key] = m
    return _models[key]


def t_(a, dev='cuda:0'):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class UnsplitCase(KE.QkvCase):
    """KE.QkvCase (fused q | k | v, N = 3 H dh) over an operand of K columns instead of H dh; algebra = False: the operand is taken as finished (no statistics, no G' / C')."""

    def __init__(self, H, dh, B, L, K, algebra):
        g = torch.Generator().manual_seed(6700 + 31 * H + dh + 7 * B + L + K)
        D = H * dh
        self.H, self.dh, self.B, self.L, self.D, self.q_only, self.K, self.algebra = H, dh, B, L, D, False, K, algebra
        self.Lp = (L + 63) // 64 * 64
        self.DQK, self.DV = (64, 64) if dh == 64 else (80, 96)
        self.nparts = 3
        self.c = KE.Consumer(g, B * L, K, 96, 3 * D, B, False, bias=False)
        self.c.rows_per_b = L
        self.qn_w, self.qn_b = 1 + 0.2 * torch.randn(dh, generator=g), 0.2 * torch.randn(dh, generator=g)
        self.kn_w, self.kn_b = 1 + 0.2 * torch.randn(dh, generator=g), 0.2 * torch.randn(dh, generator=g)
        self.cos, self.sin = KE.rope_tables64(B * L, dh)

    def ref_a(self, cos=None, sin=None):
        if self.algebra:
            return super().ref_a(cos, sin)
        return self.finish(self.c.A.double() @ self.c.W.double().T, torch.float64, cos, sin)

    def emul(self, mut=None, cos=None, sin=None):
        if self.algebra:
            return super().emul(mut, cos, sin)
        return [KE.bf16r(t) for t in self.finish(self.c.acc32, torch.float32, cos, sin)]


#         H, dh, B, L,   K
SHAPES = [(2, 72, 1, 130, 128),    # N = 432: one q, one k, one v tile; 2 K tiles
          (2, 72, 1, 130, 320),    # 5 K tiles
          (2, 64, 1, 130, 320),    # the 128 x 128 instantiation
          (2, 72, 2, 65, 320)]     # a row tile that straddles the batch boundary: RoPE position restarts at row 65, statistics per row
_cases = {}


def case_of(H, dh, B, L, K, algebra):
    key = (H, dh, B, L, K, algebra)
    if key not in _cases:
        _cases[key] = UnsplitCase(*key)
    return _cases[key]


class Launch:
    """device operands of one case, uploaded once; run() = one launch into fresh zeroed outputs (like the workspace)"""

    def __init__(self, lib, dev, c):
        cc = c.c
        self.lib, self.dev, self.c = lib, dev, c
        W, G, C = c.device_weights()
        self.M, self.N = c.B * c.L, 3 * c.D
        self.wrows = (self.N + 127) // 128 * 128
        Wp = torch.zeros(self.wrows, c.K, dtype=torch.bfloat16); Wp[:self.N] = W
        self.A, self.W = cc.A.contiguous().to(dev), Wp.to(dev)
        self.stats, self.G, self.C = cc.stats.to(dev), G.contiguous().to(dev), C.contiguous().to(dev)
        self.cur = torch.tensor([cc.cur_step], dtype=torch.int32, device=dev)
        self.aff = [x.to(dev) for x in (c.qn_w, c.qn_b, c.kn_w, c.kn_b)]
        self.cos = torch.zeros(c.L, c.dh // 2, device=dev); self.sin = torch.zeros(c.L, c.dh // 2, device=dev)
        assert lib.ezdit_test_rope_table(self.cos.data_ptr(), self.sin.data_ptr(), c.L, c.dh, None) == 0

    def run(self):
        c, cc, lib, dev = self.c, self.c.c, self.lib, self.dev
        q = torch.zeros(c.B, c.H, c.Lp, c.DQK, dtype=torch.bfloat16, device=dev)
        k = torch.zeros(c.B, c.H, c.Lp, c.DQK, dtype=torch.bfloat16, device=dev)
        v = torch.zeros(c.B, c.H, c.Lp, c.DV, dtype=torch.bfloat16, device=dev)
        z = c.algebra
        rc = lib.ezdit_test_consumer(TILE, 3, 0, self.A.data_ptr(), c.K, self.W.data_ptr(), c.K, self.wrows, None, None, 0, self.M, self.N, c.K,
                                     self.stats.data_ptr() if z else None, cc.rows_alloc if z else 0, cc.zparts if z else 0, c.K, 96,
                                     self.G.data_ptr() if z else None, self.C.data_ptr() if z else None, self.N, 1e-5,
                                     self.cur.data_ptr(), None, c.L, self.aff[0].data_ptr(), self.aff[1].data_ptr(), self.aff[2].data_ptr(), self.aff[3].data_ptr(),
                                     self.cos.data_ptr(), self.sin.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), c.B, c.H, c.L, c.Lp, c.dh, 1, None)
        assert rc == 0, lib.ezdit_last_error()
        torch.cuda.synchronize()
        return [x.cpu() for x in (q, k, v)]


def assert_bf16_bits(got_bf16, emul, ref_a, what):
    """tests/test_gpu.py _assert_bf16_bits: every element within one bf16 ulp of bf16(reference (a)), the share of elements not bit-equal at most twice the emulation's
    (+ the Poisson scatter of small counts)."""
    want = ref_a.float().to(torch.bfloat16).float()
    floor = float(ref_a.pow(2).mean().sqrt()) * 2.0 ** -10
    ulp = torch.exp2(torch.floor(torch.log2(ref_a.abs().float().clamp_min(floor))) - 7)
    worst = float(((got_bf16.float() - want).abs() / ulp).max())
    share = float((got_bf16.float() != want).double().mean())
    n_e = int((emul != want).sum())
    cap = (KE.ULP_SHARE_CAP * n_e + 3 * (KE.ULP_SHARE_CAP * n_e) ** 0.5 + 3) / want.numel()
    record(f'{what}: worst distance {worst:.2f} bf16 ulp, not bit-equal {share:.2e} (emulation {n_e / want.numel():.2e}, cap {cap:.2e})')
    assert worst <= 1.0, worst
    assert share <= cap, (share, cap)


@pytest.mark.parametrize('algebra', [True, False])
@pytest.mark.parametrize('H,dh,B,L,K', SHAPES)
def test_unsplit_fused_qkv_gemm_against_fp64(lib, dev, H, dh, B, L, K, algebra):
    """Gates per head (tests/kernel_emul.py, unchanged): same operand 4e-3, true LayerNorm 5e-3 (algebra on only), q . k^T 1.1e-3 of |q| |k|; every element within one
    bf16 ulp of the fp64 reference; the padding rows [L, Lp) and columns [dh, ..) stay as the launch found them."""
    c = case_of(H, dh, B, L, K, algebra)
    la = Launch(lib, dev, c)
    got = la.run()
    cos, sin = la.cos.cpu(), la.sin.cpu()
    what = f'un-split fused QKV tile {TILE} H={H} dh={dh} B={B} L={L} K={K} algebra={int(algebra)}'
    for name, t in zip('qkv', got):
        assert (t[:, :, L:] == 0).all(), f'{name}: rows [L, Lp) written'
        assert (t[:, :, :, dh:] == 0).all(), f'{name}: columns [dh, ..) written'
    rc64, rs64 = KE.rope_tables64(L, dh)
    assert (cos.double() - rc64.double()).abs().max() < 1e-4 and (sin.double() - rs64.double()).abs().max() < 1e-4
    val = [t[:, :, :L, :dh] for t in got]
    nat = [c.unpermute(val[0]), c.unpermute(val[1]), val[2]]
    ra, em = c.ref_a(cos, sin), c.emul(None, cos, sin)
    rb = c.ref_b() if algebra else [None] * 3
    for name, g_, a_, b_, e_ in zip('qkv', nat, ra, rb, em):
        assert torch.isfinite(g_.float()).all()
        ea = KE.per_head_rel(g_, a_)
        record(f'{what} {name}: worst head rel-L2 same operand {ea:.3e} (gate {KE.GATE_QKV_A:.1e})')
        assert ea < KE.GATE_QKV_A
        if algebra:
            eb = KE.per_head_rel(g_, b_)
            record(f'{what} {name}: worst head rel-L2 true LayerNorm {eb:.3e} (gate {KE.GATE_QKV_B:.1e})')
            assert eb < KE.GATE_QKV_B
        assert_bf16_bits(g_.contiguous(), e_, a_, f'{what} {name}')
    e = KE.qkt_err(val[0], val[1], ra[0], ra[1])
    record(f'{what} q.k^T: worst head error / (|q| |k|) {e:.3e} (gate {KE.GATE_QKT:.1e})')
    assert e < KE.GATE_QKT


def test_unsplit_fused_qkv_gemm_is_bit_reproducible(lib, dev):
    """Same build, same inputs, same bits: the first shape (2 K tiles, ragged second row tile), LayerNorm algebra on, 20 launches."""
    la = Launch(lib, dev, case_of(*SHAPES[0], True))
    first = la.run()
    for i in range(19):
        for name, a, b in zip('qkv', first, la.run()):
            assert torch.equal(a, b), (i + 1, name)


def _forward(m, inp, t):
    pred, _ = m(t_(inp['x']), torch.tensor(t), t_(inp['ctx']), context_mask=t_(inp['ctx_mask']), cls_token=None)
    return pred.cpu().numpy()


@pytest.mark.parametrize('name', ['xs', 's'])
def test_step_with_either_qkv_form_matches_reference_golden(lib, dev, name):
    """qkv_form 1 (default) and 0 (qkv_co + 4) inside the step: both within the gates of the default path, the same number of launches."""
    cfg, sd, inp, kw, g, meta = golden_case(name)
    assert not kw
    m = get_model(meta['size'], meta['seed_w'])
    t = meta['timesteps'][0]
    ref = g[f'pred_t{t}']
    counts = []
    try:
        for form in (1, 0):
            assert lib.ezdit_set_option(m._h, b'qkv_co', QKV_CO_DEFAULT + QKV_KSPLIT * (1 - form)) == 0
            pred = _forward(m, inp, t)
            counts.append(m.last_launch_count)
            r, a = rel_l2(pred, ref), float(np.abs(pred - ref).max())
            record(f'{name} t={t} qkv_form {form}: rel-L2 {r:.3e} max-abs {a:.3e}, {counts[-1]} launches')
            assert np.isfinite(pred).all()
            assert r < REL_TOL and a < ABS_TOL * max(1.0, float(ref.std()) / 1.48), (name, form, r, a)
    finally:
        assert lib.ezdit_set_option(m._h, b'qkv_co', QKV_CO_DEFAULT) == 0
    assert counts[0] == counts[1], counts


def test_sampler_loop_with_the_unsplit_qkv_form_matches_reference_golden(lib, dev):
    """smp_xs (tests/test_gpu.py::test_sampler_matches_reference_loop_golden) with qkv_form = 1: final latent within 2e-2 of the reference's own loop."""
    from ezaudio_amd.sampler import LatentSampler
    from ezaudio_amd.scheduler import DDIMScheduler
    cfg, sd, inp, init, noises, g, meta = sampler_case('smp_xs')
    assert not meta['with_gt']
    m = get_model(meta['size'], meta['seed_w'])
    try:
        assert lib.ezdit_set_option(m._h, b'qkv_co', QKV_CO_DEFAULT) == 0
        smp = LatentSampler(m, DDIMScheduler(**DIFF))
        steps = meta['steps']
        ctx, mask = inp['ctx'], inp['ctx_mask']
        sn = torch.stack([t_(noises[i]) for i in range(steps)], 0) if meta['eta'] > 0 else None
        smp.prepare(t_(ctx[0:1]), t_(mask[0:1]), t_(ctx[1:2]), t_(mask[1:2]), t_(init), sn, meta['guidance_scale'], meta['guidance_rescale'], steps, meta['eta'])
        smp.run()
        lat = smp.finish()
        torch.cuda.synchronize()
        lat = lat.clone().cpu().numpy()
    finally:
        assert lib.ezdit_set_option(m._h, b'qkv_co', QKV_CO_DEFAULT) == 0
    r = rel_l2(lat, g['latent'])
    record(f'smp_xs qkv_form 1: final-latent rel-L2 {r:.3e}')
    assert np.isfinite(lat).all() and r < 2e-2
