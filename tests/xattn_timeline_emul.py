"""Seeded inputs, the fp64 reference, an fp32 emulation and deliberate mistakes for the kernel-level tests of the prompt timeline: the TL instantiations of k_attn
(csrc/attn.hip) as ezdit_test_attention_timeline (plain 8-wave form) and ezdit_test_cross_attention_timeline (fused projection with the LayerNorm algebra, 32- and 64-row
query tiles) launch them.  Test infrastructure, not code under test; the method is that of tests/attn_band_emul.py, the statistics of the plain form are AttnCase.figures of
tests/attn_emul.py, those of the fused forms the rel-L2 / max-abs of tests/kernel_emul.py.  tests/test_attention_timeline_host.py holds the gates against the emulation on the
CPU, tests/test_attention_timeline_gpu.py the kernel against the gates.

Reference (fp64, on the bf16-valued q, k, v): for batch element b, query frame i, prompts s = 0 .. S - 1 with valid keys K_s and weights w[b][s][i] >= 0
    out_i = sum_s sum_{j in K_s} w_si exp(q_i k_j / sqrt(dh)) v_j / sum_s sum_{j in K_s} w_si exp(q_i k_j / sqrt(dh))

Emulation: tests/attn_emul.py's at NKH = 4 (128-key tiles: tile t IS prompt t), with what the timeline adds, in the kernel's order.
  table        bias[b][s][i] = fp32(log2(w / max_s w)) (computed in fp64), OFF for a weight of 0; sup[b][s] = (first, last + 1) frame of weight > 0.  A padding query (row >= Lq)
               takes the bias of frame Lq - 1: it is a copy of an existing query of its workgroup and stands in no class of its own
  tile range   the workgroup of query tile qt (QT = 64, or 32 in the fused form) walks [t_lo, t_hi): the first to the last prompt whose support meets [QT qt, min(QT qt + QT, Lq)).
               (The hull of the support: a prompt whose weights have a gap over all of the workgroup's frames is staged and skipped by every wave -- as `gap` does on purpose)
  sub-tiles    wave (32 queries, key sub-block kh): SKIPS tile t when none of its queries weights prompt t; the FULL path (max(s) c + bias for the tile maximum, ONE rounding in
               fma(s, c, bias - m), no selects) when no key of the sub-tile is masked and every query of the wave weights the prompt; otherwise the MIXED path,
               fma(s, c, bias) per valid element and the sentinel for the others
  sentinel     an element whose key is masked OR whose query weights the prompt 0 scores -1e30 and takes P = 0 by a select: while the row's m is still -1e30,
               exp2(-1e30 - m) would be 1
  merge        as in tests/attn_emul.py; a key sub-block that met no weighted valid key of a query holds m = -1e30, l = 0, O = 0 for it and merges with weight exactly 0
Not modelled, as there: the order of the fp32 sums inside an MFMA and of the 32 P of a row, the hardware's exp2.

Inputs: S = 3 prompts (Lk = Lkp = 384), B = 3; prompt s of batch element b has VALID[(s + b) % 3] valid keys at its front; randn cast to bf16, k of (b 0, h 0) times 6 at the last
valid key of prompt 0.  Poison: K rows +3e4 and V rows -3e4 at every masked key and in every prompt that no frame of the batch element weights; q rows [Lq, Lqp) +3e4 (plain form);
V channels [dh, DV) +3e4.  The weight cases come three to a launch, one per batch element: GROUPS.
Fused forms: q is the fused projection of tests/kernel_emul.py's Consumer (LayerNorm algebra, per-head LayerNorm, bf16), K padded to a multiple of 128 so that the 32-row form
(an even number of K tiles) exists at both widths; padding query rows repeat the last row, as the kernel's clamped operand rows do.

Gates: plain form GATE_HEAD / GATE_ROW / GATE_ABS of tests/attn_emul.py, fused forms GATE_XATTN_A / _B / _ABS of tests/kernel_emul.py, unless the emulation's own floor of a case
exceeds half of one: that case then takes twice its emulated floor (TL_GATES below, with the floors; tests/test_attention_timeline_host.py asserts both directions)."""
import functools
import math

import torch

from tests import attn_emul as AE
from tests import kernel_emul as KE
from tests.kernel_emul import bf16r

NEG = AE.NEG
OFF = -1e30               # stored bias of a zero weight (common.h TL_OFF)
RESCALE_THR = AE.RESCALE_THR
S, B, TK = 3, 3, 128
VALID = (100, 12, 1)
GROUPS = {'a': ('switch', 'fade', 'mix'), 'b': ('gap', 'one', 'tiny')}
ONES = 'w1'               # a group outside the cases: every weight 1, nothing masked by the timeline (the multi-tile loop of the fused forms, and the bits of the kernel without TL)
LQS = (130, 33)
TINY = 2.0 ** -20
TINY_FRAME = 5

MUTANTS = ('bias_natural_log', 'bias_before_scale', 'zero_through_exponent_and_empty_partner_weight_one', 'batch0_weights_for_all', 'weights_by_key_position',
           'frame_off_by_one', 'segment_off_by_one', 't_lo_from_last_query', 't_hi_from_first_query')
# the two halves of 'zero_through_exponent_and_empty_partner_weight_one', each harmless alone BY DESIGN, as in tests/attn_band_emul.py (the host test asserts bit-identity)
HALF_MUTANTS = ('p_without_select', 'weight_one_for_empty_partner')
# a mistake that no output can show (queries are independent: a tile walked for nothing changes no bit): padding queries counted as weighting every prompt.  The emulation's
# walked-tile count shows it, and the host test asserts that and the bit-identity
RANGE_MUTANT = 'padding_queries_widen_range'

PLAIN_CASES = [(size, Lq, grp, 'plain', 64) for size in ('xs', 'xs64') for Lq in LQS for grp in GROUPS]
FUSED_CASES = [(size, Lq, grp, 'fused', qt) for size in ('xs', 'xs64') for Lq in LQS for grp in GROUPS for qt in (32, 64)]
TL_CASES = PLAIN_CASES + FUSED_CASES      # (size, Lq, group, form, query tile)
ONES_CASES = [(size, 130, ONES, 'fused', qt) for size in ('xs', 'xs64') for qt in (32, 64)]      # the fused forms over three key tiles with nothing masked by the timeline

# per-case gates where the emulation's own floor exceeds half of a gate: case id -> {statistic: (gate = twice the floor, emulated floor)}; every other case keeps the gates above
# Only the fused forms' max-abs (against the true LayerNorm) is ever over: GATE_XATTN_ABS is the attention test's 0.06, not twice a floor (tests/kernel_emul.py: floor 0.039)
TL_GATES = {
    'xs-Lq130-b-fused-qt32': {'abs': (7.32e-2, 3.6561e-2)},
    'xs-Lq130-b-fused-qt64': {'abs': (7.32e-2, 3.6561e-2)},
    'xs64-Lq130-w1-fused-qt32': {'abs': (7.78e-2, 3.8855e-2)},
    'xs64-Lq130-w1-fused-qt64': {'abs': (7.78e-2, 3.8855e-2)},
}


def case_id(t):
    return '%s-Lq%d-%s-%s-qt%d' % t


def gates(t):
    if t[3] == 'plain':
        g = dict(head=AE.GATE_HEAD, row=AE.GATE_ROW, abs=AE.GATE_ABS)
    else:
        g = dict(a=KE.GATE_XATTN_A, b=KE.GATE_XATTN_B, abs=KE.GATE_XATTN_ABS)
    for k, (gate, _floor) in TL_GATES.get(case_id(t), {}).items():
        g[k] = gate
    return g


def weights_of(name, Lq):
    """natural weights [S][Lq] of one weight case"""
    i = torch.arange(Lq, dtype=torch.float64)
    w = torch.zeros(S, Lq, dtype=torch.float64)
    if name == 'switch':      # hard switches at frames 70 and 100
        w[0], w[1], w[2] = (i < 70), (i >= 70) & (i < 100), (i >= 100)
    elif name == 'fade':      # a linear cross-fade over [50, 90), prompt 2 never
        a = ((i - 50) / 40).clamp(0, 1)
        w[0], w[1] = 1 - a, a
    elif name == 'mix':
        w[0], w[1] = 0.7, 0.3
    elif name == 'gap':       # prompt 1 never: an interior tile that is staged and skipped by every wave
        w[0], w[2] = 0.6, 0.4
    elif name == 'one':       # prompt 1 alone: t_lo = 1, and the bits of the plain kernel on its keys
        w[1] = 1.0
    elif name == 'tiny':      # 2^-20 beside 1, and one frame whose only weight is 2^-20
        w[0], w[1] = 1.0, TINY
        w[0, min(TINY_FRAME, Lq - 1)] = 0.0
    elif name == 'ones':
        w[:] = 1.0
    else:
        raise KeyError(name)
    return w.float()


def bias_table(w, unit=1.0):
    """[..][S][Lq] natural weights -> (bias fp32, OFF for 0; sup [..][S][2] first / last + 1 weighted frame), as the library's setter builds them"""
    wd = w.double()
    mx = wd.max(-2, keepdim=True).values
    bias = torch.where(wd > 0, (torch.log2(wd / mx) * unit).float(), torch.tensor(OFF))
    pos = wd > 0
    Lq = w.shape[-1]
    idx = torch.arange(Lq)
    first = torch.where(pos, idx, torch.tensor(Lq)).min(-1).values
    last = torch.where(pos, idx + 1, torch.tensor(0)).max(-1).values
    first = torch.where(last == 0, torch.zeros_like(first), first)
    return bias, torch.stack([first, last], -1)


class TimelineCase(AE.AttnCase):
    """One launch of a timeline form.  q, k, v are the padded bf16 buffers as the device gets them (fused: q is the emulated projection, the device computes its own)."""

    def __init__(self, size, Lq, group, form, qt):      # noqa: super().__init__ builds another family of inputs
        H, dh = AE.SIZES[size]
        self.size, self.H, self.dh, self.Lq, self.Lk, self.group, self.form, self.qt = size, H, dh, Lq, 128 * S, group, form, qt
        self.nkh = 4
        self.B = B
        self.D = D = H * dh
        self.ldD = (D + 63) // 64 * 64
        self.DQK, self.DV = (64, 64) if dh == 64 else (80, 96)
        self.Lqp, self.Lkp = (Lq + 63) // 64 * 64, 128 * S
        self.klen = None
        self.lk_b = [self.Lk] * B
        self.names = GROUPS[group] if group != ONES else ('ones',) * B
        self.w = torch.stack([weights_of(n, Lq) for n in self.names])                      # [B][S][Lq]
        g = torch.Generator().manual_seed(5000 + 131 * H + dh + 7 * Lq + 3 * sum(map(ord, group)) + (1000 if form == 'fused' else 0))
        q = torch.randn(B, H, Lq, dh, generator=g)
        k = torch.randn(B, H, self.Lk, dh, generator=g)
        v = torch.randn(B, H, self.Lk, dh, generator=g)
        valid = torch.zeros(B, self.Lk, dtype=torch.bool)
        for b in range(B):
            for s in range(S):
                valid[b, 128 * s:128 * s + VALID[(s + b) % 3]] = True
        self.valid = valid
        self.kmask = valid.to(torch.uint8)
        k[0, 0, VALID[0] - 1] *= 6.0
        q, k, v = q.to(torch.bfloat16), k.to(torch.bfloat16), v.to(torch.bfloat16)
        # keys some weighted frame may see: valid, in a prompt the batch element weights somewhere
        seen = valid & (self.w > 0).any(-1).repeat_interleave(128, dim=1)                  # [B][Lk]
        self.seen = seen
        self.k = torch.zeros(B, H, self.Lkp, self.DQK, dtype=torch.bfloat16)
        self.v = torch.full((B, H, self.Lkp, self.DV), -AE.V_POISON, dtype=torch.bfloat16)
        self.k[:, :, :, :dh] = AE.K_POISON
        self.v[:, :, :, :dh] = AE.V_POISON
        sm = seen[:, None, :, None].expand(B, H, self.Lk, dh)
        self.k[:, :, :, :dh] = torch.where(sm, k, self.k[:, :, :, :dh])
        self.v[:, :, :, :dh] = torch.where(sm, v, self.v[:, :, :, :dh])
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
        return 'timeline(%s)' % case_id((self.size, self.Lq, self.group, self.form, self.qt))

    def _q_of(self, y, dtype, emul=False):
        """the projection's output [B Lq][D] -> per-head LayerNorm -> [B][H][Lqp][DQK] (zero channels behind dh; the rows behind Lq repeat row Lq - 1)"""
        B_, H, dh, Lq = self.B, self.H, self.dh, self.Lq
        q = KE.head_ln(y.reshape(B_, Lq, H, dh).permute(0, 2, 1, 3).to(dtype), self.qn_w.to(dtype), self.qn_b.to(dtype), dh)
        if emul:
            q = bf16r(q)
        out = torch.zeros(B_, H, self.Lqp, self.DQK, dtype=dtype)
        out[:, :, :Lq, :dh] = q
        out[:, :, Lq:, :dh] = q[:, :, Lq - 1:Lq]
        return out

    # ---- fp64 reference [B][Lq][D] of the formula, on the given q [B][H][>= Lq][>= dh] (default: the bf16 q of the case)
    def reference(self, q=None):
        B_, H, dh, Lq, Lk = self.B, self.H, self.dh, self.Lq, self.Lk
        q = (self.q if q is None else q)[:, :, :Lq, :dh].double()
        k, v = self.k[:, :, :Lk, :dh].double(), self.v[:, :, :Lk, :dh].double()
        wk = self.w.double().repeat_interleave(128, dim=1).transpose(1, 2)                 # [B][Lq][Lk]
        ok = (wk > 0) & self.valid[:, None, :]
        s = (q @ k.transpose(2, 3)) * dh ** -0.5 + torch.log(wk.clamp_min(1e-300))[:, None]
        s = s.masked_fill(~ok[:, None], float('-inf'))
        v = torch.where(self.seen[:, None, :, None], v, torch.zeros_like(v))
        return (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B_, Lq, self.D)

    @functools.cached_property
    def ref(self):
        return self.reference()

    @functools.cached_property
    def ref_a(self):      # fused: same operand, no roundings
        return self.reference(self._q_of(self.cons.ref_a(), torch.float64))

    @functools.cached_property
    def ref_b(self):      # fused: the true LayerNorm
        return self.reference(self._q_of(self.cons.ref_b(), torch.float64))

    def applies(self, mut):
        """None if the mistake can be made (and seen) in this case, else the reason it cannot."""
        if mut in ('bias_natural_log', 'bias_before_scale'):
            b, _ = bias_table(self.w)
            if not bool(((b != 0) & (b != OFF)).any()):
                return 'every bias is 0 or off'
        if mut == 'zero_through_exponent_and_empty_partner_weight_one' and not (self.emulated[1]['empty_partners'] and self.emulated[1]['sentinel_rows']):
            return 'no key sub-block stays without a weighted valid key of a query after an unweighted element under the sentinel'
        if mut in ('t_lo_from_last_query', 't_hi_from_first_query', RANGE_MUTANT):
            base, moved = self._ranges(None), self._ranges(mut)
            if bool((base[0] == moved[0]).all()) and bool((base[1] == moved[1]).all()):
                return 'the tile range is the same'
        return None

    def _ranges(self, mut):
        """(t_lo, t_hi) [B][nw] of the workgroup of each 32-query wave block"""
        Lq, QT = self.Lq, self.qt
        nw = self.Lqp // 32
        _, sup = bias_table(self.w)
        t_lo = torch.zeros(B, nw, dtype=torch.long)
        t_hi = torch.zeros(B, nw, dtype=torch.long)
        for w_ in range(nw):
            qa = 32 * w_ // QT * QT
            qb = min(qa + QT, Lq)
            if qa >= Lq:
                continue
            if mut == 't_lo_from_last_query':
                ra, rb = (qb - 1, qb), (qa, qb)
            elif mut == 't_hi_from_first_query':
                ra, rb = (qa, qb), (qa, qa + 1)
            else:
                ra = rb = (qa, qb)
            for b in range(B):
                meets = lambda r: [s for s in range(S) if int(sup[b, s, 0]) < r[1] and int(sup[b, s, 1]) > r[0]]      # noqa: E731
                lo, hi = meets(ra), meets(rb)
                t_lo[b, w_] = min(lo) if lo else 0
                t_hi[b, w_] = max(hi) + 1 if hi else 1
                if mut == RANGE_MUTANT and qa + QT > Lq:
                    t_lo[b, w_], t_hi[b, w_] = 0, S
        return t_lo, t_hi

    def emul(self, mut=None):
        B_, H, dh, Lq, Lp, nkh = self.B, self.H, self.dh, self.Lq, self.Lqp, 4
        f32 = torch.float32
        c = torch.tensor(1.4426950408889634, dtype=f32) * torch.rsqrt(torch.tensor(float(dh), dtype=f32))
        w = self.w.clone()
        if mut == 'batch0_weights_for_all':
            w[:] = w[0]
        bias, _ = bias_table(w, unit=math.log(2.0) if mut == 'bias_natural_log' else 1.0)          # [B][S][Lq]
        fr = torch.arange(Lp).clamp(max=Lq - 1)                                                     # the frame whose weights query row i takes
        if mut == 'frame_off_by_one':
            fr = (fr + 1).clamp(max=Lq - 1)
        bias = bias[:, :, fr]                                                                        # [B][S][Lp]
        if mut == 'segment_off_by_one':
            bias = torch.roll(bias, -1, dims=1)
        t_lo, t_hi = self._ranges(mut)
        nw = Lp // 32
        alive = torch.tensor([32 * w_ // self.qt * self.qt < Lq for w_ in range(nw)])[None, :].expand(B_, nw)
        kvalid = torch.zeros(B_, self.Lkp, dtype=torch.bool)
        kvalid[:, :self.Lk] = self.valid
        Sraw = self.q.float() @ self.k.float().transpose(2, 3)                                      # [B][H][Lp][Lkp]
        V = self.v.float()
        real_row = (torch.arange(Lp) < Lq)[None, None, :]
        counts = dict(fired_t1=0, deferred_t1=0, skipped=0, full=0, mixed=0, sentinel_rows=0, empty_partners=0, t_lo_pos=0, t_hi_short=0, walked=0)
        counts['t_lo_pos'] = int(((t_lo > 0) & alive).sum())
        counts['t_hi_short'] = int(((t_hi < S) & alive).sum())
        counts['walked'] = int(((t_hi - t_lo) * alive).sum())
        expand = lambda x: x[:, None, :, None].expand(B_, H, nw, 32).reshape(B_, H, Lp)      # noqa: E731  [B][nw] -> [B][H][Lp]
        ms, ls, os_ = [], [], []
        for kh in range(nkh):
            m = torch.full((B_, H, Lp), NEG, dtype=f32)
            l = torch.zeros(B_, H, Lp, dtype=f32)
            o = torch.zeros(B_, H, Lp, self.DV, dtype=f32)
            for t in range(S):
                key0 = t * TK + 32 * kh
                in_range = (t >= t_lo) & (t < t_hi) & alive                                         # [B][nw]
                bt = bias[:, t]                                                                      # [B][Lp]: the lane's bias of this tile
                if mut == 'weights_by_key_position':      # the frame index taken from the key's place in the prompt (lane r32 <-> key 32 kh + r32)
                    kf = (32 * kh + torch.arange(Lp) % 32).clamp(max=Lq - 1)
                    bt = bias_table(w)[0][:, t][:, kf]
                wpos = bt > 0.5 * OFF                                                                # [B][Lp]
                any_w = wpos.view(B_, nw, 32).any(-1)
                all_w = wpos.view(B_, nw, 32).all(-1)
                ent_w = in_range & any_w
                if not bool(ent_w.any()):
                    continue
                kfull = kvalid[:, key0:key0 + 32].all(-1)[:, None]                                   # [B][1]
                full_w = ent_w & all_w & kfull
                counts['skipped'] += int((in_range & ~ent_w).sum())
                counts['full'] += int(full_w.sum())
                counts['mixed'] += int((ent_w & ~full_w).sum())
                ent = expand(ent_w)
                full = expand(full_w)[..., None]
                vm4 = (kvalid[:, None, None, key0:key0 + 32] & wpos[:, None, :, None]).expand(B_, H, Lp, 32) & ent[..., None]
                s = Sraw[..., key0:key0 + 32]
                b4 = torch.where(wpos, bt, torch.zeros((), dtype=f32))[:, None, :, None]             # (an off bias is never added)
                if mut == 'bias_before_scale':
                    sb = (s + b4) * c
                else:
                    sb = (s.double() * c.double() + b4.double()).float()                             # fma(s, c, bias): one rounding
                sc = torch.where(vm4, sb, torch.tensor(NEG, dtype=f32))
                if mut == 'bias_before_scale':
                    tmax_full = (s.max(-1).values + b4[..., 0]) * c
                else:
                    tmax_full = s.max(-1).values * c + b4[..., 0]
                tmax = torch.where(full[..., 0], tmax_full, sc.max(-1).values)
                over = ~(tmax <= m + RESCALE_THR) & ent
                fire = over.view(B_, H, nw, 32).any(-1, keepdim=True).expand(B_, H, nw, 32).reshape(B_, H, Lp)
                mnew = torch.maximum(m, tmax)
                alpha = torch.exp2(m - mnew)
                counts['sentinel_rows'] += int((ent & ~full[..., 0] & (m == NEG) & ~vm4.any(-1) & real_row).sum())
                m = torch.where(fire, mnew, m)
                l = torch.where(fire, l * alpha, l)
                o = torch.where(fire[..., None], o * alpha[..., None], o)
                if mut == 'bias_before_scale':
                    x_full = sb - m[..., None]
                else:
                    nm = b4[..., 0] - m                                                              # fma(s, c, bias - m): one rounding
                    x_full = (s.double() * c.double() + nm.double()[..., None]).float()
                x = torch.where(full, x_full, sc - m[..., None])
                p = torch.where(vm4 | full, torch.exp2(x), torch.zeros((), dtype=f32))
                if mut in ('zero_through_exponent_and_empty_partner_weight_one', 'p_without_select'):
                    p = torch.where(vm4 | full, p, torch.exp2(NEG - m)[..., None].expand_as(p))
                p = torch.where(ent[..., None], p, torch.zeros((), dtype=f32))
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
        counts['empty_partners'] = int(((mk == NEG) & (mm != NEG)[None] & real_row[None]).sum())
        if mut in ('zero_through_exponent_and_empty_partner_weight_one', 'weight_one_for_empty_partner'):
            wg = torch.where((mk == NEG) & (mm != NEG)[None], torch.ones((), dtype=f32), wg)
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

    def plain_on_prompt(self, s, b):
        """the plain emulation (tests/attn_emul.py, nkh 4) of batch element b on prompt s's 128 keys alone: what weight 1 on that prompt and 0 elsewhere must equal bit for bit"""
        c = AE.AttnCase.__new__(AE.AttnCase)
        c.size, c.H, c.dh, c.Lq, c.Lk, c.form, c.nkh = self.size, self.H, self.dh, self.Lq, 128, 'kmask', 4
        c.D, c.ldD, c.DQK, c.DV = self.D, self.ldD, self.DQK, self.DV
        c.klen, c.B, c.Lqp, c.Lkp = None, 1, self.Lqp, 128
        c.valid = self.valid[b:b + 1, 128 * s:128 * s + 128]
        c.kmask = c.valid.to(torch.uint8)
        c.lk_b = [128]
        c.q = self.q[b:b + 1]
        c.k = self.k[b:b + 1, :, 128 * s:128 * s + 128]
        c.v = self.v[b:b + 1, :, 128 * s:128 * s + 128]
        return c

    # ---- the statistics of the fused forms on an output buffer [B Lq + PAD_ROWS][ldD]
    def figures_fused(self, buf):
        got = buf.float()[:self.B * self.Lq, :self.D].reshape(self.B, self.Lq, self.D)
        fin = bool(torch.isfinite(got).all())
        got = torch.nan_to_num(got, nan=float('inf'))
        sent = torch.tensor(AE.SENTINEL).to(torch.bfloat16).float()
        return dict(a=KE.rel_l2(got, self.ref_a), b=KE.rel_l2(got, self.ref_b), abs=float((got.double() - self.ref_b).abs().max()), finite=fin, zeros=True,
                    cols=bool((buf.float()[:self.B * self.Lq, self.D:] == sent).all()), rows=bool((buf.float()[self.B * self.Lq:] == sent).all()))

    def stats(self, buf):
        return self.figures(buf) if self.form == 'plain' else self.figures_fused(buf)


def stat_keys(t):
    return ('head', 'row', 'abs') if t[3] == 'plain' else ('a', 'b', 'abs')


def within_gates(f, g):
    return all(f[k] < g[k] for k in g)


def caught(f, g):
    """as AE.caught: a bitwise check breaks, or a gated statistic is at three times its gate"""
    return (not AE.bitwise_ok(f)) or any(f[k] >= 3 * g[k] for k in g)


@functools.lru_cache(maxsize=64)
def tl_case(size, Lq, group, form, qt):
    return TimelineCase(size, Lq, group, form, qt)
