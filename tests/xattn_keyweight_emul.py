"""Seeded inputs, the fp64 reference, an fp32 emulation and deliberate mistakes for the kernel-level tests of prompt emphasis: the KW instantiations of k_attn
(csrc/attn.hip) as ezdit_test_attention_keyweights (plain 8-wave form) and ezdit_test_cross_attention_keyweights (fused projection with the LayerNorm algebra, 32- and 64-row
query tiles) launch them.  Test infrastructure, not code under test; the method is that of tests/xattn_timeline_emul.py, whose case class this one extends (the fused
projection, the statistics of both forms).  tests/test_attention_keyweight_host.py holds the gates against the emulation on the CPU, tests/test_attention_keyweight_gpu.py
the kernel against the gates.

Reference (fp64, on the bf16-valued q, k, v): batch element b has valid keys V_b and weights w_bj > 0
    out_i = sum_{j in V_b} w_bj exp(q_i k_j / sqrt(dh)) v_j / sum_{j in V_b} w_bj exp(q_i k_j / sqrt(dh))
With integer weights this is the unweighted attention over the keys repeated w times (reference_repeated).

Emulation: tests/attn_emul.py's at NKH = 4 (128-key tiles), with what the emphasis adds, in the kernel's order.
  table        bias[b][j] = fp32(log2(w_bj / max over V_b)) (computed in fp64), 0 at masked and padding keys; w is not read at a masked key
  full path    (no key of the 32-key sub-tile masked) tile maximum over fma(s, c, bias); ONE rounding in fma(s, c, bias - m) for the exponent
  mixed path   fma(s, c, bias) per valid element and the sentinel -1e30 for the others, then (that) - m: two roundings, as the plain kernel's s c - m
  validity     the mask alone: a masked key takes P = 0 by a select and its bias is never used
At a bias of 0 every one of these is the plain emulation's expression: uniform weights give its bits (the host test asserts it against tests/attn_emul.py).
Not modelled, as there: the order of the fp32 sums inside an MFMA and of the 32 P of a row, the hardware's exp2.

Inputs: B = 3, sizes xs / xs64, Lq 130 / 33.  Lk = Lkp = 384 (three key tiles): tile s of batch element b has VALID[(s + b) % 3] valid keys at its front; and Lk = 100 in
Lkp = 128 (the shipped shape): batch element b has VALID[b] valid keys at the front.  randn cast to bf16, k of (b 0, h 0) times 6 at its last valid key of tile 0.  Poison: K rows
+3e4 and V rows -3e4 at every masked key and in [Lk, Lkp); NaN weights at masked keys (one of them +1e9 in `wide`: the heaviest key of the row is masked); q rows [Lq, Lqp)
+3e4 (plain form); V channels [dh, DV) +3e4.  The weight cases come three to a launch, one per batch element (GROUP); `uniform` (every weight 3.0) is a launch of its own.
Fused forms: as tests/xattn_timeline_emul.py.

Weight cases: peak -- one valid key 2^20 above the rest; int -- integers 1 .. 4; wide -- 2^-20 at every third valid key beside 1 (on the single-key rows: the one key at 2^-20,
which must change nothing); uniform -- every weight 3.0.

Gates: plain form GATE_HEAD / GATE_ROW / GATE_ABS of tests/attn_emul.py, fused forms GATE_XATTN_A / _B / _ABS of tests/kernel_emul.py, unless the emulation's own floor of a case
exceeds half of one: that case then takes twice its emulated floor (KW_GATES below, with the floors; tests/test_attention_keyweight_host.py asserts both directions)."""
import functools
import math

import torch

from tests import attn_emul as AE
from tests import kernel_emul as KE
from tests import xattn_timeline_emul as TE
from tests.kernel_emul import bf16r

NEG = AE.NEG
RESCALE_THR = AE.RESCALE_THR
B, TK = 3, 128
VALID = (100, 12, 1)
GROUP = ('peak', 'int', 'wide')      # batch element b's weight case
UNIFORM = 'uniform'
LQS = (130, 33)
LKS = (384, 100)
TINY = 2.0 ** -20
PEAK = 2.0 ** 20
HEAVY_MASKED = 1.0e9

MUTANTS = ('bias_natural_log', 'bias_times_scale', 'batch0_weights_for_all', 'key_index_linear', 'first_subblock_for_all_kh', 'next_tile_early',
           'masked_key_through_exponent', 'b0_ignored')

FORMS = (('plain', 64), ('fused', 32), ('fused', 64))
KW_CASES = [(size, Lq, Lk, 'g', form, qt) for size in ('xs', 'xs64') for Lq in LQS for Lk in LKS for form, qt in FORMS]      # (size, Lq, Lk, weights, form, query tile)
UNIFORM_CASES = [(size, 130, 384, UNIFORM, form, qt) for size in ('xs', 'xs64') for form, qt in FORMS]

# per-case gates where the emulation's own floor exceeds half of a gate: case id -> {statistic: (gate = twice the floor, emulated floor)}; every other case keeps the gates above
# Only the fused forms' max-abs (against the true LayerNorm) is ever over: GATE_XATTN_ABS is the attention test's 0.06, not twice a floor (tests/kernel_emul.py: floor 0.039)
KW_GATES = {
    'xs-Lq130-Lk384-g-fused-qt32': {'abs': (6.17e-2, 3.0852e-2)},
    'xs-Lq130-Lk384-g-fused-qt64': {'abs': (6.17e-2, 3.0852e-2)},
    'xs-Lq130-Lk100-g-fused-qt32': {'abs': (6.71e-2, 3.3555e-2)},
    'xs-Lq130-Lk100-g-fused-qt64': {'abs': (6.71e-2, 3.3555e-2)},
}


def case_id(t):
    return '%s-Lq%d-Lk%d-%s-%s-qt%d' % t


def gates(t):
    if t[4] == 'plain':
        g = dict(head=AE.GATE_HEAD, row=AE.GATE_ROW, abs=AE.GATE_ABS)
    else:
        g = dict(a=KE.GATE_XATTN_A, b=KE.GATE_XATTN_B, abs=KE.GATE_XATTN_ABS)
    for k, (gate, _floor) in KW_GATES.get(case_id(t), {}).items():
        g[k] = gate
    return g


def stat_keys(t):
    return ('head', 'row', 'abs') if t[4] == 'plain' else ('a', 'b', 'abs')


within_gates = TE.within_gates
caught = TE.caught


def weights_of(name, valid, g):
    """natural weights [Lk] of one weight case for the validity `valid` [Lk]; NaN at masked keys"""
    Lk = valid.numel()
    idx = valid.nonzero().flatten()
    w = torch.ones(Lk, dtype=torch.float32)
    if name == 'int':
        w = torch.randint(1, 5, (Lk,), generator=g).float()
    elif name == 'wide':
        w[idx[::3]] = TINY
    elif name == 'peak':
        w[idx[len(idx) // 2]] = PEAK
    elif name == UNIFORM:
        w[:] = 3.0
    else:
        raise KeyError(name)
    w[~valid] = float('nan')
    if name == 'wide' and bool((~valid).any()):
        w[int((~valid).nonzero()[0])] = HEAVY_MASKED
    return w


def bias_table(w, valid, Lkp, unit=1.0):
    """natural weights [B][Lk] and validity [B][Lk] -> bias fp32 [B][Lkp] as the library's setter builds it: log2(w / max over the valid keys), 0 elsewhere"""
    B_, Lk = w.shape
    wd = torch.where(valid, w.double(), torch.zeros((), dtype=torch.float64))
    mx = wd.max(-1, keepdim=True).values
    bias = torch.zeros(B_, Lkp, dtype=torch.float32)
    bias[:, :Lk] = torch.where(valid, (torch.log2((wd / mx).clamp_min(1e-300)) * unit).float(), torch.zeros((), dtype=torch.float32))
    return bias


class KeyWeightCase(TE.TimelineCase):
    """One launch of an emphasis form.  q, k, v are the padded bf16 buffers as the device gets them (fused: q is the emulated projection, the device computes its own)."""

    def __init__(self, size, Lq, Lk, wname, form, qt):      # noqa: super().__init__ builds another family of inputs
        H, dh = AE.SIZES[size]
        self.size, self.H, self.dh, self.Lq, self.Lk, self.group, self.form, self.qt = size, H, dh, Lq, Lk, wname, form, qt
        self.nkh = 4
        self.B = B
        self.D = D = H * dh
        self.ldD = (D + 63) // 64 * 64
        self.DQK, self.DV = (64, 64) if dh == 64 else (80, 96)
        self.Lqp, self.Lkp = (Lq + 63) // 64 * 64, (Lk + 127) // 128 * 128
        self.klen = None
        self.lk_b = [Lk] * B
        self.names = GROUP if wname != UNIFORM else (UNIFORM,) * B
        g = torch.Generator().manual_seed(7000 + 131 * H + dh + 7 * Lq + 3 * Lk + sum(map(ord, wname)) + (1000 if form == 'fused' else 0))
        q = torch.randn(B, H, Lq, dh, generator=g)
        k = torch.randn(B, H, Lk, dh, generator=g)
        v = torch.randn(B, H, Lk, dh, generator=g)
        valid = torch.zeros(B, Lk, dtype=torch.bool)
        for b in range(B):
            if Lk > 128:
                for s in range(Lk // 128):
                    valid[b, 128 * s:128 * s + VALID[(s + b) % 3]] = True
            else:
                valid[b, :VALID[b]] = True
        self.valid = valid
        self.seen = valid      # (TimelineCase.figures: the keys some query may see)
        self.kmask = valid.to(torch.uint8)
        self.w = torch.stack([weights_of(n, valid[b], g) for b, n in enumerate(self.names)])      # [B][Lk]
        k[0, 0, VALID[0] - 1] *= 6.0
        q, k, v = q.to(torch.bfloat16), k.to(torch.bfloat16), v.to(torch.bfloat16)
        self.k = torch.zeros(B, H, self.Lkp, self.DQK, dtype=torch.bfloat16)
        self.v = torch.full((B, H, self.Lkp, self.DV), -AE.V_POISON, dtype=torch.bfloat16)
        self.k[:, :, :, :dh] = AE.K_POISON
        self.v[:, :, :, :dh] = AE.V_POISON
        sm = valid[:, None, :, None].expand(B, H, Lk, dh)
        self.k[:, :, :Lk, :dh] = torch.where(sm, k, self.k[:, :, :Lk, :dh])
        self.v[:, :, :Lk, :dh] = torch.where(sm, v, self.v[:, :, :Lk, :dh])
        self.cons = None
        if form == 'plain':
            self.q = torch.zeros(B, H, self.Lqp, self.DQK, dtype=torch.bfloat16)
            self.q[:, :, Lq:, :dh] = AE.Q_POISON
            self.q[:, :, :Lq, :dh] = q
        else:
            self.cons = KE.Consumer(g, B * Lq, D, 96, D, B, False, mean_scale=2.0, bias=False)
            self.cons.rows_per_b = Lq
            self.qn_w, self.qn_b = 1 + 0.2 * torch.randn(dh, generator=g), 0.2 * torch.randn(dh, generator=g)
            self.xK = (D + 127) // 128 * 128
            self.q = self._q_of(self.cons.emul(), torch.float32, True).to(torch.bfloat16)

    def __repr__(self):
        return 'keyweight(%s)' % case_id((self.size, self.Lq, self.Lk, self.group, self.form, self.qt))

    # ---- fp64 reference [B][Lq][D] of the formula, on the given q [B][H][>= Lq][>= dh] (default: the bf16 q of the case)
    def reference(self, q=None, w=None):
        B_, dh, Lq, Lk = self.B, self.dh, self.Lq, self.Lk
        q = (self.q if q is None else q)[:, :, :Lq, :dh].double()
        k, v = self.k[:, :, :Lk, :dh].double(), self.v[:, :, :Lk, :dh].double()
        w = self.w if w is None else w
        lw = torch.log(torch.where(self.valid, w.double(), torch.ones((), dtype=torch.float64)))      # [B][Lk]
        s = (q @ k.transpose(2, 3)) * dh ** -0.5 + lw[:, None, None, :]
        s = s.masked_fill(~self.valid[:, None, None, :], float('-inf'))
        v = torch.where(self.valid[:, None, :, None], v, torch.zeros_like(v))
        return (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B_, Lq, self.D)

    def reference_repeated(self, b):
        """batch element b (integer weights): the UNWEIGHTED fp64 attention over its valid keys, key j repeated w_bj times -> [Lq][D]"""
        dh, Lq = self.dh, self.Lq
        idx = self.valid[b].nonzero().flatten()
        rep = torch.repeat_interleave(idx, self.w[b, idx].long())
        q = self.q[b, :, :Lq, :dh].double()
        k, v = self.k[b, :, rep, :dh].double(), self.v[b, :, rep, :dh].double()
        s = (q @ k.transpose(1, 2)) * dh ** -0.5
        return (torch.softmax(s, -1) @ v).permute(1, 0, 2).reshape(Lq, self.D)

    def applies(self, mut):
        """None if the mistake can be made (and seen) in this case, else the reason it cannot."""
        if mut == 'next_tile_early' and self.Lkp == TK:
            return 'one key tile'
        if not bool((bias_table(self.w, self.valid, self.Lkp) != 0).any()):
            return 'every bias is 0' if mut != 'masked_key_through_exponent' else None
        return None

    def emul(self, mut=None):
        B_, H, dh, Lq, Lk, Lp, Lkp, nkh = self.B, self.H, self.dh, self.Lq, self.Lk, self.Lqp, self.Lkp, 4
        f32 = torch.float32
        c = torch.tensor(1.4426950408889634, dtype=f32) * torch.rsqrt(torch.tensor(float(dh), dtype=f32))
        bias = bias_table(self.w, self.valid, Lkp, unit=math.log(2.0) if mut == 'bias_natural_log' else 1.0)      # [B][Lkp]
        if mut == 'batch0_weights_for_all':
            bias = bias[0:1].expand(B_, Lkp).clone()
        if mut == 'b0_ignored':      # a sub-range launch [1, B) that reads the table from its front: batch element b takes the row of b - 1
            bias = torch.cat([bias[0:1], bias[:-1]])
        if mut == 'bias_times_scale':
            bias = bias * c
        valid = torch.zeros(B_, Lkp, dtype=torch.bool)
        valid[:, :Lk] = self.valid
        Sraw = self.q.float() @ self.k.float().transpose(2, 3)      # [B][H][Lp][Lkp]
        V = self.v.float()
        real_row = (torch.arange(Lp) < Lq)[None, None, :]
        nw = Lp // 32
        # the lane's elements by key offset o in the sub-tile: o = (r & 3) + 8 (r >> 2) + 4 hi.  'key_index_linear': the bias of key0 + r is taken instead
        off = torch.arange(32)
        if mut == 'key_index_linear':
            off = (off & 3) + 4 * (off >> 3)
        counts = dict(fired_t1=0, deferred_t1=0, full=0, mixed=0, full_biased=0, mixed_biased=0)
        ms, ls, os_ = [], [], []
        nt = (Lk + TK - 1) // TK
        for kh in range(nkh):
            m = torch.full((B_, H, Lp), NEG, dtype=f32)
            l = torch.zeros(B_, H, Lp, dtype=f32)
            o = torch.zeros(B_, H, Lp, self.DV, dtype=f32)
            for t in range(nt):
                key0 = t * TK + 32 * kh
                if key0 >= Lk:
                    continue
                tb = min(t + 1, nt - 1) if mut == 'next_tile_early' else t
                bk0 = tb * TK + (0 if mut == 'first_subblock_for_all_kh' else 32 * kh)
                bt = bias[:, bk0:bk0 + 32][:, off]                                                   # [B][32]
                inb = (key0 + torch.arange(32) < Lk)[None, :]
                vm = valid[:, key0:key0 + 32] & inb                                                   # [B][32]
                if mut == 'masked_key_through_exponent':
                    vm = inb.expand(B_, 32)
                full = valid[:, key0:key0 + 32].all(1)[:, None, None] & bool(inb.all())              # [B][1][1]
                vm4 = vm[:, None, None, :]
                b4 = bt[:, None, None, :]
                counts['full'] += int(full.sum()); counts['mixed'] += int((~full).sum())
                counts['full_biased'] += int((full[:, 0, 0] & (bt != 0).any(1)).sum())
                counts['mixed_biased'] += int((~full[:, 0, 0] & ((bt != 0) & vm).any(1)).sum())
                s = Sraw[..., key0:key0 + 32]
                sb = (s.double() * c.double() + b4.double()).float()                                  # fma(s, c, bias): one rounding
                sc = torch.where(vm4, sb, torch.tensor(NEG, dtype=f32))
                tmax = torch.where(full, sb.max(-1).values, sc.max(-1).values)
                over = ~(tmax <= m + RESCALE_THR)
                fire = over.view(B_, H, nw, 32).any(-1, keepdim=True).expand(B_, H, nw, 32).reshape(B_, H, Lp)
                mnew = torch.maximum(m, tmax)
                alpha = torch.exp2(m - mnew)
                m = torch.where(fire, mnew, m)
                l = torch.where(fire, l * alpha, l)
                o = torch.where(fire[..., None], o * alpha[..., None], o)
                bm = b4 - m[..., None]                                                                # bias - m, rounded
                x_full = (s.double() * c.double() + bm.double()).float()                              # fma(s, c, bias - m): one rounding
                x = torch.where(full[..., None], x_full, sc - m[..., None])
                p = torch.where(vm4 | full[..., None], torch.exp2(x), torch.zeros((), dtype=f32))
                l = l + p.sum(-1)
                o = o + bf16r(p) @ V[:, :, key0:key0 + 32]
                if t >= 1:
                    wave = lambda x: x.view(B_, H, nw, 32).any(-1)      # noqa: E731
                    counts['fired_t1'] += int(wave(over & real_row).sum())
                    counts['deferred_t1'] += int(wave((p > 1).any(-1) & real_row & ~fire).sum())
            ms.append(m); ls.append(l); os_.append(o)
        mk = torch.stack(ms)
        mm = mk.max(0).values
        wg = torch.exp2(mk - mm)
        lt = torch.zeros(B_, H, Lp, dtype=f32)
        for i in range(nkh):
            lt = lt + ls[i] * wg[i]
        wg = wg * (1.0 / lt)
        acc = torch.zeros(B_, H, Lp, self.DV, dtype=f32)
        for i in range(nkh):
            acc = acc + os_[i] * wg[i][..., None]
        res = bf16r(acc)
        buf = torch.full((B_ * Lq + AE.PAD_ROWS, self.ldD), AE.SENTINEL, dtype=f32)
        for b in range(B_):
            for h in range(H):
                buf[b * Lq:(b + 1) * Lq, h * dh:(h + 1) * dh] = res[b, h, :Lq, :dh]
        return buf, counts

    def plain_twin(self):
        """the plain emulation (tests/attn_emul.py, nkh 4, key mask) on the same buffers: what a table of zeros must equal bit for bit"""
        c = AE.AttnCase.__new__(AE.AttnCase)
        c.size, c.H, c.dh, c.Lq, c.Lk, c.form, c.nkh = self.size, self.H, self.dh, self.Lq, self.Lk, 'kmask', 4
        c.D, c.ldD, c.DQK, c.DV = self.D, self.ldD, self.DQK, self.DV
        c.klen, c.B, c.Lqp, c.Lkp = None, self.B, self.Lqp, self.Lkp
        c.valid, c.kmask, c.lk_b = self.valid, self.kmask, [self.Lk] * self.B
        c.q, c.k, c.v = self.q, self.k, self.v
        return c


@functools.lru_cache(maxsize=64)
def kw_case(size, Lq, Lk, wname, form, qt):
    return KeyWeightCase(size, Lq, Lk, wname, form, qt)
