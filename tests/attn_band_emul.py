"""Seeded inputs, the fp64 reference, an fp32 emulation and deliberate mistakes for the kernel-level tests of sliding-window self-attention: the BAND instantiations
k_attn<64 | 72, 2 | 4, false, 64, true> of csrc/attn.hip as ezdit_test_attention_band launches them.  Test infrastructure, not code under test; the method, the statistics
(AttnCase.figures) and the starting gates are those of tests/attn_emul.py.  tests/test_attention_band_host.py holds the gates against the emulation on the CPU,
tests/test_attention_band_gpu.py the kernel against the gates.

Reference: fp64 softmax(q k^T / sqrt(dh)) v over the keys j with |i - j| <= radius and j < klen[b] (L without lengths), on the bf16-valued q, k, v; query rows >= klen[b] are 0.

Emulation: tests/attn_emul.py's, with what the band adds, in the kernel's order.
  tile range   the workgroup of query tile qt (64 rows) walks the key tiles [t_lo, t_hi): t_lo = max(0, 64 qt - radius) // TK, t_hi = min(ntiles, (min(64 qt + 63, klen[b] - 1) +
               radius) // TK + 1), ntiles = ceil(klen[b] / TK), TK = 32 NKH.  A query tile with 64 qt >= klen[b] stores zeros and leaves
  sub-tiles    wave (query sub-block q0 .. q0 + 31, key sub-block key0 .. key0 + 31), qlast = min(q0 + 31, klen[b] - 1) its last query that exists: it SKIPS the sub-tile when
               key0 >= klen[b], key0 - qlast > radius or q0 - (key0 + 31) > radius; takes the FULL path (max(s) c, one rounding in fma(s, c, -m), no selects) when
               key0 + 31 - q0 <= radius, qlast - key0 <= radius and key0 + 32 <= klen[b]; otherwise the MIXED path with per-element validity |i - j| <= radius and j < klen[b]
  sentinel     a masked element scores -1e30 and takes P = 0 by a select: while the row's m is still -1e30, exp2(-1e30 - m) would be 1
  rescale      per wave at RESCALE_THR = 4, as in tests/attn_emul.py (padding query rows [L, Lp) take part: they are rows of the wave)
  merge        as in tests/attn_emul.py; a key sub-block that met no valid key of a query holds m = -1e30, l = 0, O = 0 for it and merges with weight exp2(-1e30 - max m) = 0
Not modelled, as there: the order of the fp32 sums inside an MFMA and of the 32 P of a row, the hardware's exp2.

Inputs: randn cast to bf16; the staircase head of tests/attn_emul.py in batch element 0 (every query row scores key 32 j at STAIR_BASE + 0.25 kh + stair(t) log2 units when the band lets
it see that key: rescales fire and are deferred in turn); k of (b 0, h 0) times 6 at its last valid key.  Poison as there: K rows +3e4 and V rows -3e4 at the keys >= klen[b] and in
[L, Lp), q rows [L, Lp) +3e4, V channels [dh, DV) +3e4.

Gates: GATE_HEAD, GATE_ROW, GATE_ABS of tests/attn_emul.py -- twice the emulated floor of the unmasked kernel -- unless the band emulation's own floor of a case exceeds half of one;
that case then takes twice its emulated floor (BAND_GATES below, with the floors; tests/test_attention_band_host.py asserts both directions)."""
import functools

import torch

from tests import attn_emul as AE
from tests.kernel_emul import bf16r

NEG = AE.NEG
RESCALE_THR = AE.RESCALE_THR

# the deliberate mistakes.  Each must be caught (AE.caught with the case's gates) by at least one case it applies to
MUTANTS = ('upper_radius_plus_one', 'upper_radius_minus_one', 'lower_radius_plus_one', 'lower_radius_minus_one', 'one_sided', 'sentinel_and_empty_partner_weight_one',
           't_lo_from_last_query', 't_hi_from_first_query', 'klen_ignored_in_band')
# 'sentinel_and_empty_partner_weight_one' is two mistakes made together: P = exp2(s - m) without the select (1 for a masked element while m = -1e30) AND weight 1 in the merge for a
# partner that still holds m = -1e30.  Each alone is harmless BY DESIGN, as in tests/attn_emul.py (the host test asserts bit-identity): without the select the junk a wave gathers
# under the sentinel is wiped by the first real rescale (alpha = exp2(-1e30 - m) = 0) or, if no valid key ever comes, merges with weight exp2(-1e30 - max m) = 0; and a weight of 1
# for a partner with l = 0 multiplies l = 0 and O = 0
HALF_MUTANTS = ('p_without_select', 'weight_one_for_empty_partner')

R_EDGES = (1, 5, 31, 32, 33, 63, 64, 65)
KLEN5 = (130, 65, 33, 1)
KLEN6 = (260, 200)


def _cases():
    c = []
    for size in ('xs', 'xs64'):
        for nkh in (2, 4):
            for r in R_EDGES:
                c.append((size, 130, r, None, nkh))          # 1: sub-tile and tile boundaries on both sides
            c.append((size, 130, 129, None, nkh))            # 2: nothing masked -- the plain kernel's bits
            c.append((size, 130, 20, KLEN5, nkh))            # 5: B = 4 with lengths
            c.append((size, 260, 20, KLEN6, nkh))            # 6: a length that ends inside a band
        c.append((size, 260, 20, None, 2))                   # 3: t_lo > 0 and t_hi < ntiles at nkh 2
        c.append((size, 390, 20, None, 4))                   # 4: ... at nkh 4: query tile 5 sees key tile 2 only
    return c


BAND_CASES = _cases()      # (size, L, radius, klen, nkh)

# per-case gates where the band emulation's own floor exceeds half of a gate of tests/attn_emul.py: case id -> {statistic: (gate = twice the floor, emulated floor)}; every
# other case and statistic keeps AE.GATE_*.  Only max-abs is ever over: a row that sees few keys averages less, its outputs reach [4, 8), and half a bf16 ulp there is 1.6e-2
# against the 7.8e-3 of [2, 4) that AE.GATE_ABS was sized on.  The worst head and row floors over BAND_CASES are 2.33e-3 and 3.73e-3, below AE's 2.92e-3 and 3.99e-3
BAND_GATES = {
    'xs-L130-r65-full-nkh2': {'abs': (2.57e-2, 1.2842e-2)},
    'xs-L130-r1-full-nkh4': {'abs': (1.81e-2, 9.0424e-3)},
    'xs-L130-r129-full-nkh4': {'abs': (2.48e-2, 1.2416e-2)},
    'xs64-L130-r1-full-nkh2': {'abs': (2.06e-2, 1.0301e-2)},
    'xs64-L130-r31-full-nkh2': {'abs': (2.49e-2, 1.2455e-2)},
    'xs64-L130-r65-full-nkh2': {'abs': (1.84e-2, 9.1842e-3)},
    'xs64-L130-r5-full-nkh4': {'abs': (2.72e-2, 1.3590e-2)},
}


def case_id(t):
    size, L, r, klen, nkh = t
    return '%s-L%d-r%d-%s-nkh%d' % (size, L, r, 'klen' + '_'.join(str(n) for n in klen) if klen else 'full', nkh)


def gates(t):
    g = dict(head=AE.GATE_HEAD, row=AE.GATE_ROW, abs=AE.GATE_ABS)
    for k, (gate, _floor) in BAND_GATES.get(case_id(t), {}).items():
        g[k] = gate
    return g


class BandCase(AE.AttnCase):
    """One launch of the band form.  q, k, v are the padded bf16 buffers as the device gets them; figures() is AttnCase's."""

    def __init__(self, size, L, radius, klen, nkh):      # noqa: super().__init__ builds another family of inputs
        H, dh = AE.SIZES[size]
        self.size, self.H, self.dh, self.Lq, self.Lk, self.nkh, self.radius = size, H, dh, L, L, nkh, radius
        self.form = 'band'
        self.D = H * dh
        self.ldD = (self.D + 63) // 64 * 64
        self.DQK, self.DV = (64, 64) if dh == 64 else (80, 96)
        self.klen = list(klen) if klen else None
        self.B = B = len(klen) if klen else 2
        self.Lqp = self.Lkp = (L + 127) // 128 * 128 if nkh == 4 else (L + 63) // 64 * 64
        self.kmask = None
        self.lk_b = [int(n) for n in (self.klen or [L] * B)]
        g = torch.Generator().manual_seed(7000 + 131 * H + dh + 7 * L + 3 * radius + 1000 * nkh + (17 if klen else 0))
        q = torch.randn(B, H, L, dh, generator=g)
        k = torch.randn(B, H, L, dh, generator=g)
        v = torch.randn(B, H, L, dh, generator=g)
        k[0, 0, self.lk_b[0] - 1] *= 6.0
        c = 1.4426950408889634 / dh ** 0.5
        q[0, 0, :, 0] = AE.STAIR_Q
        for j in range((L + 31) // 32):
            t, kh = divmod(j, nkh)
            level = AE.STAIR_BASE + 0.25 * kh + 4.0 * t - 0.5 * (t % 2)
            k[0, 0, 32 * j] = 0.0
            k[0, 0, 32 * j, 0] = level / (c * AE.STAIR_Q)
        q, k, v = q.to(torch.bfloat16), k.to(torch.bfloat16), v.to(torch.bfloat16)
        self.q = torch.zeros(B, H, self.Lqp, self.DQK, dtype=torch.bfloat16)
        self.q[:, :, L:, :dh] = AE.Q_POISON
        self.q[:, :, :L, :dh] = q
        self.k = torch.zeros(B, H, self.Lkp, self.DQK, dtype=torch.bfloat16)
        self.v = torch.full((B, H, self.Lkp, self.DV), -AE.V_POISON, dtype=torch.bfloat16)
        self.k[:, :, :, :dh] = AE.K_POISON
        self.v[:, :, :, :dh] = AE.V_POISON
        for b, n in enumerate(self.lk_b):
            self.k[b, :, :n, :dh] = k[b, :, :n]
            self.v[b, :, :n, :dh] = v[b, :, :n]

    def __repr__(self):
        return 'band(%s)' % case_id((self.size, self.Lq, self.radius, self.klen, self.nkh))

    def pair_valid(self, lo=None, up=None, lk_b=None, rows=None):
        """[B][rows][Lkp] bool: key j exists for query i: -lo <= j - i <= up and j < lk_b[b]"""
        lo = self.radius if lo is None else lo
        up = self.radius if up is None else up
        rows = self.Lqp if rows is None else rows
        i = torch.arange(rows)[:, None]
        j = torch.arange(self.Lkp)[None, :]
        band = (j - i <= up) & (i - j <= lo)
        lens = torch.tensor(self.lk_b if lk_b is None else lk_b)[:, None, None]
        return band[None] & (j[None] < lens)

    @functools.cached_property
    def ref(self):
        B, H, dh, L = self.B, self.H, self.dh, self.Lq
        q, k, v = self.q[:, :, :L, :dh].double(), self.k[:, :, :L, :dh].double(), self.v[:, :, :L, :dh].double()
        ok = self.pair_valid(rows=L)[:, None, :, :L]                       # [B][1][L][L]
        s = (q @ k.transpose(2, 3)) * dh ** -0.5
        s = s.masked_fill(~ok, float('-inf'))
        p = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)               # (rows >= klen[b] may see no key: zeroed below)
        o = (p @ v).permute(0, 2, 1, 3).reshape(B, L, self.D)
        for b in range(B):
            o[b, self.rows_b(b):] = 0.0
        return o

    def applies(self, mut):
        """None if the mistake can be made (and seen) in this case, else the reason it cannot."""
        R, L, nkh = self.radius, self.Lq, self.nkh
        TK = 32 * nkh
        longest = max(self.lk_b)
        if mut in ('upper_radius_plus_one', 'lower_radius_plus_one') and R + 1 > longest - 1:
            return 'no pair of keys at distance radius + 1'
        if mut in ('upper_radius_minus_one', 'lower_radius_minus_one') and R > longest - 1:
            return 'no pair of keys at distance radius'
        if mut == 'one_sided' and longest < 2:
            return 'one key'
        if mut == 'sentinel_and_empty_partner_weight_one' and not (self.emulated[1]['empty_partners'] and self.emulated[1]['sentinel_rows']):
            return 'no key sub-block stays without a valid key of a query after a masked element under the sentinel'
        if mut in ('t_lo_from_last_query', 't_hi_from_first_query'):
            moved = False
            for b, n in enumerate(self.lk_b):
                for qt in range((min(n, L) + 63) // 64):
                    nt = (n + TK - 1) // TK
                    if mut == 't_lo_from_last_query':
                        moved = moved or max(0, 64 * qt + 63 - R) // TK != max(0, 64 * qt - R) // TK
                    else:
                        moved = moved or min(nt, (64 * qt + R) // TK + 1) != min(nt, (min(64 * qt + 63, n - 1) + R) // TK + 1)
            if not moved:
                return 'the tile range is the same'
        if mut == 'klen_ignored_in_band' and not any(n < L and n % 32 for n in self.lk_b):
            return 'no length that ends inside an entered sub-tile'
        return None

    def emul(self, mut=None):
        B, H, dh, L, Lp, nkh, R = self.B, self.H, self.dh, self.Lq, self.Lqp, self.nkh, self.radius
        TK = 32 * nkh
        f32 = torch.float32
        c = torch.tensor(1.4426950408889634, dtype=f32) * torch.rsqrt(torch.tensor(float(dh), dtype=f32))
        up = R + (mut == 'upper_radius_plus_one') - (mut == 'upper_radius_minus_one')
        lo = R + (mut == 'lower_radius_plus_one') - (mut == 'lower_radius_minus_one')
        if mut == 'one_sided':
            up = 0
        lk_b = list(self.lk_b)
        lk_mask = [self.Lkp] * B if mut == 'klen_ignored_in_band' else lk_b      # what the element mask and the FULL class compare keys with
        valid = self.pair_valid(lo, up, lk_mask)                                   # [B][Lp][Lkp]
        S = self.q.float() @ self.k.float().transpose(2, 3)
        V = self.v.float()
        nw = Lp // 32
        q0 = 32 * torch.arange(nw)                                                 # first query of each wave row block
        qt0 = q0 // 64 * 64                                                        # first query of its workgroup
        real_row = (torch.arange(Lp) < L)[None, None, :]
        counts = dict(fired_t1=0, deferred_t1=0, skipped=0, full=0, mixed=0, sentinel_rows=0, empty_partners=0, t_lo_pos=0, t_hi_short=0)
        lens = torch.tensor(lk_b)
        ntiles = (lens + TK - 1) // TK                                             # [B]
        first_q = qt0 + (63 if mut == 't_lo_from_last_query' else 0)
        last_q = qt0[None, :].expand(B, nw) if mut == 't_hi_from_first_query' else torch.minimum((qt0 + 63)[None, :], lens[:, None] - 1)      # [B][nw]
        t_lo = torch.clamp(first_q - lo, min=0) // TK                             # [nw]  (the tile range uses the band as the kernel holds it)
        t_hi = torch.minimum((last_q + up) // TK + 1, ntiles[:, None])            # [B][nw]
        qlast = torch.minimum((q0 + 31)[None, :], lens[:, None] - 1)               # [B][nw]: the last query of the wave that exists
        alive = (qt0[None, :] < lens[:, None])                                     # [B][nw]: the workgroup does not leave at once
        counts['t_lo_pos'] = int(((t_lo > 0)[None, :] & alive).sum())
        counts['t_hi_short'] = int(((t_hi < ntiles[:, None]) & alive).sum())
        expand = lambda x: x[:, None, :, None].expand(B, H, nw, 32).reshape(B, H, Lp)      # noqa: E731  [B][nw] -> [B][H][Lp]
        ms, ls, os_ = [], [], []
        for kh in range(nkh):
            m = torch.full((B, H, Lp), NEG, dtype=f32)
            l = torch.zeros(B, H, Lp, dtype=f32)
            o = torch.zeros(B, H, Lp, self.DV, dtype=f32)
            for t in range(self.Lkp // TK):
                key0 = t * TK + 32 * kh
                in_range = (t >= t_lo)[None, :] & (t < t_hi) & alive                                             # [B][nw]
                near = (key0 - qlast <= up) & (q0 - (key0 + 31) <= lo)[None, :]                                 # [B][nw]
                ent_w = in_range & near & (key0 < lens)[:, None]                                                 # [B][nw]
                if not bool(ent_w.any()):
                    continue
                lm = torch.tensor(lk_mask)
                full_w = ent_w & (key0 + 31 - q0 <= up)[None, :] & (qlast - key0 <= lo) & (key0 + 32 <= lm)[:, None]
                counts['skipped'] += int((in_range & ~ent_w).sum())
                counts['full'] += int(full_w.sum())
                counts['mixed'] += int((ent_w & ~full_w).sum())
                ent = expand(ent_w)
                full = expand(full_w)[..., None]
                vm4 = (valid[:, :, key0:key0 + 32])[:, None].expand(B, H, Lp, 32) & ent[..., None]
                s = S[..., key0:key0 + 32]
                sc = torch.where(vm4, s * c, torch.tensor(NEG, dtype=f32))
                tmax = torch.where(full[..., 0], s.max(-1).values * c, sc.max(-1).values)
                over = ~(tmax <= m + RESCALE_THR) & ent
                fire = over.view(B, H, nw, 32).any(-1, keepdim=True).expand(B, H, nw, 32).reshape(B, H, Lp)
                mnew = torch.maximum(m, tmax)
                alpha = torch.exp2(m - mnew)
                counts['sentinel_rows'] += int((ent & ~full[..., 0] & (m == NEG) & ~vm4.any(-1) & real_row).sum())
                m = torch.where(fire, mnew, m)
                l = torch.where(fire, l * alpha, l)
                o = torch.where(fire[..., None], o * alpha[..., None], o)
                x_full = (s.double() * c.double() - m.double()[..., None]).float()
                x = torch.where(full, x_full, sc - m[..., None])
                p = torch.where(vm4 | full, torch.exp2(x), torch.zeros((), dtype=f32))
                if mut in ('sentinel_and_empty_partner_weight_one', 'p_without_select'):
                    p = torch.where(vm4 | full, p, torch.exp2(NEG - m)[..., None].expand_as(p))
                p = torch.where(ent[..., None], p, torch.zeros((), dtype=f32))
                l = l + p.sum(-1)
                o = o + bf16r(p) @ V[:, :, key0:key0 + 32]
                if t >= 1:
                    wave = lambda x: x.view(B, H, nw, 32).any(-1)      # noqa: E731
                    counts['fired_t1'] += int(wave(over & real_row).sum())
                    counts['deferred_t1'] += int(wave((p > 1).any(-1) & real_row & ~fire).sum())
            ms.append(m); ls.append(l); os_.append(o)
        mk = torch.stack(ms)
        mm = mk.max(0).values
        w = torch.exp2(mk - mm)
        rows_live = torch.stack([(torch.arange(Lp) < min(n, L)) for n in lk_b])[:, None, :]
        counts['empty_partners'] = int(((mk == NEG) & (mm != NEG)[None] & rows_live[None]).sum())
        if mut in ('sentinel_and_empty_partner_weight_one', 'weight_one_for_empty_partner'):
            w = torch.where((mk == NEG) & (mm != NEG)[None], torch.ones((), dtype=f32), w)
        lt = torch.zeros(B, H, Lp, dtype=f32)
        for i in range(nkh):
            lt = lt + ls[i] * w[i]
        w = w * (1.0 / lt)
        acc = torch.zeros(B, H, Lp, self.DV, dtype=f32)
        for i in range(nkh):
            acc = acc + os_[i] * w[i][..., None]
        res = bf16r(acc)
        buf = torch.full((B * L + AE.PAD_ROWS, self.ldD), AE.SENTINEL, dtype=f32)
        for b in range(B):
            for h in range(H):
                buf[b * L:(b + 1) * L, h * dh:(h + 1) * dh] = res[b, h, :L, :dh]
            if self.klen:
                buf[b * L + lk_b[b]:(b + 1) * L, :self.D] = 0.0
        return buf, counts


def bitwise_ok(f):
    return AE.bitwise_ok(f)


def within_gates(f, g):
    return f['head'] < g['head'] and f['row'] < g['row'] and f['abs'] < g['abs']


def caught(f, g):
    """as AE.caught: a bitwise check breaks, or a gated statistic is at three times its gate"""
    return (not AE.bitwise_ok(f)) or f['head'] >= 3 * g['head'] or f['row'] >= 3 * g['row'] or f['abs'] >= 3 * g['abs']


@functools.lru_cache(maxsize=64)
def band_case(size, L, radius, klen, nkh):
    return BandCase(size, L, radius, klen, nkh)
