"""Seeded inputs, the fp64 reference, an fp32 emulation and deliberate mistakes for the kernel-level tests of plain self-attention: k_attn<64 | 72, 2 | 4> of csrc/attn.hip as
ezdit_test_attention / ezdit_test_attention_varlen launch it (no fused projection).  Test infrastructure, not code under test; same shape as tests/row_emul.py and
tests/vae_emul.py.  tests/test_attention_kernels_host.py holds the gates against the emulation on the CPU, tests/test_attention_kernels_gpu.py the kernel against the gates.

Reference: fp64 softmax(q k^T / sqrt(dh)) v over the valid keys of each batch element, on the bf16-valued q, k, v.

Emulation: the kernel's arithmetic in the kernel's order, in fp32 torch on the CPU.
  scores      fp32 q . k, in log2 units: times c = log2(e) / sqrt(dh) (dh, not the padded 80)
  ownership   key sub-block kh of NKH owns the keys [t TK + 32 kh, + 32) of every tile t, TK = 32 NKH; a sub-tile whose first key is >= Lk (klen[b]) is not entered
  validity    key < Lk (klen[b]) and kmask[b][key]; an invalid key scores -1e30 and gets P = 0 by a select.  A sub-tile without an invalid key takes the kernel's other
              path: max(s) c for the tile maximum and ONE rounding in fma(s, c, -m)
  rescale     decided per WAVE -- the 32 query rows q0 .. q0 + 31, padding rows [Lq, Lqp) included: when any of them has tmax > m + 4, EVERY row takes m = max(m, tmax) and
              scales l and O by exp2(m_old - m); otherwise all keep their m and P may reach 2^4
  P, l        l sums the unrounded P; P . V runs on bf16(P) in fp32
  merge       the NKH partials (m, l, O) by log-sum-exp: w_k = exp2(m_k - max m), l = sum l_k w_k, O = sum O_k (w_k / l), then ONE bf16 rounding.  A sub-block that saw no
              valid key has m = -1e30, l = 0, O = 0 and weight exp2(-1e30 - max m) = 0
  store       rows < Lq, columns h dh .. + dh of a [B Lq][ldD] buffer; with klen the query rows >= klen[b] are stored as zeros
Not modelled: the order of the fp32 sums inside an MFMA and of the 32 P of a row, and the hardware's exp2 (1 ulp).  The emulation returns coverage counts beside its output:
(wave, sub-tile) events at t >= 1 (and, of those, at kh >= 1) where the rescale fired because of a row < Lq, and where it was deferred with some P > 1 in a row < Lq.

Inputs: randn cast to bf16, plus
  * k of (b 0, h 0) times 6 at its last valid key, k of the last (b, h) times 6 at a valid key of the second 64-key tile (where there is one)
  * one staircase head: its q hold 4 in channel 0 and key 32 j (first of sub-tile j) is alpha_j e_0, so that the key scores exactly STAIR_BASE + 0.25 kh + stair(t) log2
    units for EVERY query row, stair(t) climbing by 3.5 and 4.5 in turn: in every sub-block the rescale fires at t = 0, is deferred at t = 1 with P = 2^3.5, fires at t = 2 ...
  * `sharp`: q times 3 (a near one-hot softmax)
Poison (large and finite: 0 x NaN through the MFMA is NaN by design): K rows no query may see hold +3e4, V rows -3e4 (keys in [Lk, Lkp), masked keys, keys >= klen[b]), q rows
[Lq, Lqp) +3e4, V channels [dh, DV) +3e4.  q and k channels [dh, DQK) are zero, as the contract requires.

Gates: twice the worst emulated floor of the statistic over ATTN_CASES, never above the 1.2e-2 / 0.06 of the two older attention tests (tests/test_gpu.py,
tests/test_ragged_gpu.py).  The values measured on MI355X are in DESIGN.md section 2 ("Kernel-level tests of plain self-attention")."""
import functools

import torch

from tests.kernel_emul import bf16r

# ---- gates, each with the emulated floor behind it (CPU, worst over ATTN_CASES; tests/test_attention_kernels_host.py asserts floor <= FLOOR * 1.005 and gate <= 2 FLOOR)
FLOOR_HEAD, FLOOR_ROW, FLOOR_ABS = 2.92e-3, 3.99e-3, 9.03e-3
GATE_HEAD = 5.8e-3    # worst (batch element, head) rel-L2 over the valid query rows: emulated floor 2.92e-3 (s, 130 x 130, nkh 4), MI355X worst 2.92e-3; the older tests' 1.2e-2 is 4.1 x the floor
GATE_ROW = 7.9e-3     # worst query row of a head, rel-L2 over its dh values: emulated floor 3.99e-3 (s, 130 x 130, nkh 2), MI355X worst 3.99e-3
GATE_ABS = 1.8e-2     # max-abs: emulated floor 9.03e-3, MI355X worst 9.03e-3 (half a bf16 ulp of an output in [2, 4) is 7.8e-3); twice the floor is far below the older tests' 0.06, which does not bind
OLD_REL, OLD_ABS = 1.2e-2, 0.06     # the gates of the older tests: no gate here is above them

SENTINEL = 7.0        # prefill of the output buffer
PAD_ROWS = 64         # rows behind the B Lq of the output buffer: a store to a query row in [Lq, Lqp) of the last batch element lands there
K_POISON, V_POISON, Q_POISON = 3.0e4, -3.0e4, 3.0e4
RESCALE_THR = 4.0
STAIR_BASE, STAIR_Q = 10.0, 4.0
NEG = -1e30

MUTANTS = ('drop_last_valid_key', 'admit_first_pad_key', 'mask_ignored_in_last_subtile', 'batch0_validity_for_all', 'rescale_skips_o', 'rescale_skips_l',
           'merge_unweighted', 'merge_drops_last_partial', 'empty_partial_weight_one', 'scale_by_dqk', 'p_keys_swapped', 'v_tiles_swapped', 'head_offset_dqk',
           'rows_beyond_lq_written', 'klen_pad_rows_unzeroed', 'cols_beyond_d_written')
# the two halves of 'empty_partial_weight_one', each harmless alone BY DESIGN (the host test asserts bit-identity): P = exp2(s - m) without the validity select is 1 for an
# invalid key while m is still -1e30, but such a partial merges with weight exp2(-1e30 - max m) = 0; and a weight of 1 for an m = -1e30 partial multiplies l = 0, O = 0
HALF_MUTANTS = ('p_without_select', 'weight_one_for_empty_m')

SIZES = {'xs': (2, 72), 'xs64': (2, 64), 's': (8, 72)}      # (H, dh) of the test models whose handle the hook takes them from
KLEN = (1, 32, 33, 64, 65, 128, 129, 130)


def _cases():
    c = []
    for size in ('xs', 'xs64'):
        for nkh in (2, 4):
            for Lq, Lk in ((130, 130), (77, 385), (65, 257), (1, 64), (33, 1)):
                c.append((size, Lq, Lk, 'plain', nkh))
            c.append((size, 96, 96, 'sharp', nkh))
            c.append((size, 64, 20, 'kmask', nkh))
            c.append((size, 130, 129, 'kmask', nkh))
            c.append((size, 130, 130, 'klen', nkh))
    for nkh in (2, 4):
        c.append(('s', 130, 130, 'plain', nkh))
        c.append(('s', 130, 129, 'kmask', nkh))
    return c


ATTN_CASES = _cases()      # (size, Lq, Lk, form, nkh)


def case_id(t):
    return '%s-Lq%d-Lk%d-%s-nkh%d' % t


class AttnCase:
    """One launch.  form: 'plain' | 'sharp' (plain with q x 3) | 'kmask' | 'klen'.  q, k, v are the padded bf16 buffers as the device gets them."""

    def __init__(self, size, Lq, Lk, form, nkh):
        H, dh = SIZES[size]
        self.size, self.H, self.dh, self.Lq, self.Lk, self.form, self.nkh = size, H, dh, Lq, Lk, form, nkh
        self.D = H * dh
        self.ldD = (self.D + 63) // 64 * 64
        self.DQK, self.DV = (64, 64) if dh == 64 else (80, 96)
        self.klen = list(KLEN) if form == 'klen' else None
        self.B = B = len(KLEN) if form == 'klen' else 3
        self.Lqp = (Lq + 63) // 64 * 64
        self.Lkp = (Lk + 127) // 128 * 128 if nkh == 4 else (Lk + 63) // 64 * 64
        g = torch.Generator().manual_seed(9000 + 131 * H + dh + 7 * Lq + 3 * Lk + len(form) + 1000 * nkh)
        q = torch.randn(B, H, Lq, dh, generator=g)
        k = torch.randn(B, H, Lk, dh, generator=g)
        v = torch.randn(B, H, Lk, dh, generator=g)
        if form == 'sharp':
            q = 3.0 * q
        # ---- validity [B][Lk]
        valid = torch.ones(B, Lk, dtype=torch.bool)
        self.kmask = None
        if form == 'kmask':
            if Lk < 64:       # prefix | key 0 alone | every third key masked
                valid[0, 12:] = False
                valid[1, 1:] = False
                valid[2, 2::3] = False
            else:             # suffix alone (the first sub-tiles wholly masked: m stays -1e30 across tiles) | one whole sub-tile masked in the middle | key 0 alone
                valid[0, :100] = False
                valid[1, 32:64] = False
                valid[2, 1:] = False
            self.kmask = valid.to(torch.uint8)
        if form == 'klen':
            for b, n in enumerate(self.klen):
                valid[b, n:] = False
        self.valid = valid
        self.lk_b = [int(n) for n in (self.klen or [Lk] * B)]      # what the kernel holds in `Lk` for batch element b
        # ---- spikes and the staircase
        last0 = int(valid[0].nonzero().max())
        k[0, 0, last0] *= 6.0
        second = [j for j in range(64, min(Lk, 128)) if valid[B - 1, j] and j % 32 != 0]
        if second:
            k[B - 1, H - 1, second[len(second) // 2]] *= 6.0
        self.stair_b = sb = B - 1 if form == 'klen' else 1
        c = 1.4426950408889634 / dh ** 0.5
        q[sb, 0, :, 0] = STAIR_Q
        for j in range((Lk + 31) // 32):
            t, kh = divmod(j, nkh)
            level = STAIR_BASE + 0.25 * kh + 4.0 * t - 0.5 * (t % 2)      # increments of 3.5 and 4.5 in turn
            k[sb, 0, 32 * j] = 0.0
            k[sb, 0, 32 * j, 0] = level / (c * STAIR_Q)
        q, k, v = q.to(torch.bfloat16), k.to(torch.bfloat16), v.to(torch.bfloat16)
        # ---- the padded, poisoned buffers
        self.q = torch.zeros(B, H, self.Lqp, self.DQK, dtype=torch.bfloat16)
        self.q[:, :, Lq:, :dh] = Q_POISON
        self.q[:, :, :Lq, :dh] = q
        self.k = torch.zeros(B, H, self.Lkp, self.DQK, dtype=torch.bfloat16)
        self.v = torch.full((B, H, self.Lkp, self.DV), -V_POISON, dtype=torch.bfloat16)
        self.k[:, :, :, :dh] = K_POISON
        self.v[:, :, :, :dh] = V_POISON
        vm = valid[:, None, :, None].expand(B, H, Lk, dh)
        self.k[:, :, :Lk, :dh] = torch.where(vm, k, self.k[:, :, :Lk, :dh])
        self.v[:, :, :Lk, :dh] = torch.where(vm, v, self.v[:, :, :Lk, :dh])

    def __repr__(self):
        return 'attn(%s)' % case_id((self.size, self.Lq, self.Lk, self.form, self.nkh))

    def rows_b(self, b):
        """query rows of batch element b that hold a result (the others: zeros with klen)"""
        return min(self.lk_b[b], self.Lq) if self.klen else self.Lq

    # ---- fp64 reference [B][Lq][D]; zeros in the query rows >= klen[b]
    @functools.cached_property
    def ref(self):
        B, H, dh, Lq, Lk = self.B, self.H, self.dh, self.Lq, self.Lk
        q, k, v = self.q[:, :, :Lq, :dh].double(), self.k[:, :, :Lk, :dh].double(), self.v[:, :, :Lk, :dh].double()
        s = (q @ k.transpose(2, 3)) * dh ** -0.5
        s = s.masked_fill(~self.valid[:, None, None, :], float('-inf'))
        v = torch.where(self.valid[:, None, :, None], v, torch.zeros_like(v))
        o = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B, Lq, self.D)
        for b in range(B):
            o[b, self.rows_b(b):] = 0.0
        return o

    def applies(self, mut):
        """None if the mistake can be made (and seen) in this case, else the reason it cannot."""
        B, H, dh, nkh = self.B, self.H, self.dh, self.nkh
        nvalid = self.valid.sum(1)
        if mut == 'drop_last_valid_key' and int(nvalid.max()) < 2:
            return 'one valid key'
        if mut == 'admit_first_pad_key' and all(n >= self.Lkp for n in self.lk_b):
            return 'no padding key: Lk == Lkp'
        if mut == 'mask_ignored_in_last_subtile':
            if self.kmask is None:
                return 'no kmask'
            k0 = (self.Lk - 1) // 32 * 32
            if bool(self.valid[:, k0:].all()):
                return 'no masked key in the last sub-tile'
        if mut == 'batch0_validity_for_all' and self.form not in ('kmask', 'klen'):
            return 'no per-batch-element validity'
        if mut in ('rescale_skips_o', 'rescale_skips_l') and max(self.lk_b) <= 32 * nkh:
            return 'one tile: the only rescale is the first, of l = 0 and O = 0'
        if mut in ('merge_unweighted', 'merge_drops_last_partial') and max(self.lk_b) <= 32 * (nkh - 1):
            return 'the last partial is empty'
        if mut == 'merge_unweighted' and max(self.lk_b) <= 32:
            return 'one partial'
        if mut == 'empty_partial_weight_one':
            if self.kmask is None:
                return 'no kmask: a sub-tile without a valid key is not entered'
            ok = False
            for b in range(B):
                for kh in range(nkh):
                    own = [j for j in range(self.Lk) if (j // 32) % nkh == kh]
                    if own and not bool(self.valid[b, own].any()):
                        ok = True
            if not ok:
                return 'every entered sub-block has a valid key'
        if mut == 'scale_by_dqk' and (self.DQK == dh or int(nvalid.max()) < 2):
            return 'DQK = dh' if self.DQK == dh else 'one valid key: P = 1 at every scale'
        if mut == 'p_keys_swapped' and int(nvalid.max()) < 9:
            return 'fewer than nine keys'
        if mut == 'v_tiles_swapped':
            return None
        if mut == 'head_offset_dqk' and (self.DQK == dh or (H - 1) * self.DQK + dh > self.ldD):
            return 'DQK = dh' if self.DQK == dh else 'head H - 1 would leave the row'
        if mut == 'rows_beyond_lq_written' and self.Lq == self.Lqp:
            return 'Lq == Lqp'
        if mut == 'klen_pad_rows_unzeroed' and self.klen is None:
            return 'no klen'
        if mut == 'cols_beyond_d_written' and (self.DV == dh or (H - 1) * dh + self.DV > self.ldD):
            return 'DV = dh' if self.DV == dh else 'head H - 1 would leave the row'
        return None

    # ---- the emulation: (output buffer fp32-valued bf16 [B Lq + PAD_ROWS][ldD], coverage counts)
    def emul(self, mut=None):
        B, H, dh, Lq, Lk, Lqp, Lkp, nkh = self.B, self.H, self.dh, self.Lq, self.Lk, self.Lqp, self.Lkp, self.nkh
        TK = 32 * nkh
        f32 = torch.float32
        cs = self.DQK if mut == 'scale_by_dqk' else dh
        c = torch.tensor(1.4426950408889634, dtype=f32) * torch.rsqrt(torch.tensor(float(cs), dtype=f32))
        # validity over the padded keys and the kernel's `Lk` per batch element
        valid = torch.zeros(B, Lkp, dtype=torch.bool)
        valid[:, :Lk] = self.valid
        lk_b = list(self.lk_b)
        if mut == 'batch0_validity_for_all':
            valid[:] = valid[0]
            lk_b = [lk_b[0]] * B
        if mut == 'drop_last_valid_key':
            for b in range(B):
                idx = valid[b].nonzero()
                if len(idx) > 1:
                    valid[b, int(idx.max())] = False
        if mut == 'admit_first_pad_key':
            for b in range(B):
                if lk_b[b] < Lkp:
                    valid[b, lk_b[b]] = True
                    lk_b[b] += 1
        if mut == 'mask_ignored_in_last_subtile':
            k0 = (Lk - 1) // 32 * 32
            valid[:, k0:Lk] = True
        S = self.q.float() @ self.k.float().transpose(2, 3)      # [B][H][Lqp][Lkp], raw
        V = self.v.float()
        real_row = (torch.arange(Lqp) < Lq)[None, None, :]
        swap = torch.arange(32)
        if mut == 'p_keys_swapped':
            swap = torch.tensor([16 * (j // 16) + {1: 2, 2: 1}.get((j % 16) // 4, (j % 16) // 4) * 4 + j % 4 for j in range(32)])
        counts = dict(fired_t1=0, fired_t1_kh1=0, deferred_t1=0, deferred_t1_kh1=0)
        ms, ls, os_ = [], [], []
        for kh in range(nkh):
            m = torch.full((B, H, Lqp), NEG, dtype=f32)
            l = torch.zeros(B, H, Lqp, dtype=f32)
            o = torch.zeros(B, H, Lqp, self.DV, dtype=f32)
            for t in range((Lkp + TK - 1) // TK):
                key0 = t * TK + 32 * kh
                ent = torch.tensor([key0 < n for n in lk_b])      # [B]: the sub-tile is entered
                if key0 >= Lkp or not bool(ent.any()):
                    continue
                inb = torch.tensor([[key0 + j < n for j in range(32)] for n in lk_b])
                vm = valid[:, key0:key0 + 32] & inb & ent[:, None]                    # [B][32]
                full = vm.all(1)[:, None, None]                                      # [B][1][1]
                vm4 = vm[:, None, None, :]
                s = S[..., key0:key0 + 32]
                sc = torch.where(vm4, s * c, torch.tensor(NEG, dtype=f32))
                tmax = torch.where(full, s.max(-1).values * c, sc.max(-1).values)
                over = ~(tmax <= m + RESCALE_THR) & ent[:, None, None]
                fire = over.view(B, H, Lqp // 32, 32).any(-1, keepdim=True).expand(B, H, Lqp // 32, 32).reshape(B, H, Lqp)
                mnew = torch.maximum(m, tmax)
                alpha = torch.exp2(m - mnew)
                m = torch.where(fire, mnew, m)
                if mut != 'rescale_skips_l':
                    l = torch.where(fire, l * alpha, l)
                if mut != 'rescale_skips_o':
                    o = torch.where(fire[..., None], o * alpha[..., None], o)
                x_full = (s.double() * c.double() - m.double()[..., None]).float()      # fma(s, c, -m): one rounding
                x = torch.where(full[..., None], x_full, sc - m[..., None])
                p = torch.where(vm4, torch.exp2(x), torch.zeros((), dtype=f32))
                if mut in ('empty_partial_weight_one', 'p_without_select'):
                    p = torch.where(vm4, p, torch.exp2(NEG - m)[..., None].expand_as(p))
                    p = torch.where(ent[:, None, None, None], p, torch.zeros((), dtype=f32))
                l = l + p.sum(-1)
                o = o + bf16r(p)[..., swap] @ V[:, :, key0:key0 + 32]
                if t >= 1:
                    wave = lambda x: x.view(B, H, Lqp // 32, 32).any(-1)
                    f_ev = wave(over & real_row)
                    d_ev = wave((p > 1).any(-1) & real_row & ~fire)
                    counts['fired_t1'] += int(f_ev.sum())
                    counts['deferred_t1'] += int(d_ev.sum())
                    if kh >= 1:
                        counts['fired_t1_kh1'] += int(f_ev.sum())
                        counts['deferred_t1_kh1'] += int(d_ev.sum())
            ms.append(m); ls.append(l); os_.append(o)
        # ---- merge
        n_merge = nkh - 1 if mut == 'merge_drops_last_partial' else nkh
        mk = torch.stack(ms[:n_merge])
        mm = mk.max(0).values
        w = torch.exp2(mk - mm)
        if mut in ('empty_partial_weight_one', 'weight_one_for_empty_m'):
            w = torch.where(mk == NEG, torch.ones((), dtype=f32), w)
        lt = torch.zeros(B, H, Lqp, dtype=f32)
        for i in range(n_merge):
            lt = lt + ls[i] * w[i]
        inv = 1.0 / lt
        w = inv.expand_as(w) if mut == 'merge_unweighted' else w * inv
        acc = torch.zeros(B, H, Lqp, self.DV, dtype=f32)
        for i in range(n_merge):
            acc = acc + os_[i] * w[i][..., None]
        res = bf16r(acc)
        if mut == 'v_tiles_swapped':
            res = torch.cat([res[..., 32:64], res[..., :32], res[..., 64:]], -1)
        # ---- store
        buf = torch.full((B * Lq + PAD_ROWS, self.ldD), SENTINEL, dtype=f32)
        rows = Lqp if mut == 'rows_beyond_lq_written' else Lq
        hs = self.DQK if mut == 'head_offset_dqk' else dh
        width = self.DV if mut == 'cols_beyond_d_written' else dh
        for b in range(B):
            for h in range(H):
                buf[b * Lq:b * Lq + rows, h * hs:h * hs + width] = res[b, h, :rows, :width]
            if self.klen:
                n = lk_b[b]
                if mut != 'klen_pad_rows_unzeroed':
                    buf[b * Lq + n:(b + 1) * Lq, :self.D] = 0.0
                else:      # a query tile wholly beyond the length is left before anything is computed
                    buf[b * Lq + (n + 63) // 64 * 64:(b + 1) * Lq, :self.D] = SENTINEL
        return buf, counts

    @functools.cached_property
    def emulated(self):
        return self.emul()

    # ---- what the tests measure of an output buffer [B Lq + PAD_ROWS][ldD]
    def figures(self, buf):
        """dict: head / row / abs (worst (b, h) rel-L2, worst query row of a head, max-abs, all over the rows that hold a result; inf where not finite), and the bitwise
        checks: finite (the written region), zeros (klen: query rows >= klen[b] exactly 0), cols (columns [D, ldD) still the prefill), rows (the rows behind B Lq)."""
        B, H, dh, Lq, D = self.B, self.H, self.dh, self.Lq, self.D
        buf = buf.float()
        got = buf[:B * Lq, :D].reshape(B, Lq, D).double()
        fin = bool(torch.isfinite(got).all())
        head = row = mabs = 0.0
        zeros = True
        for b in range(B):
            n = self.rows_b(b)
            g = torch.nan_to_num(got[b, :n], nan=float('inf')).reshape(n, H, dh)
            r = self.ref[b, :n].reshape(n, H, dh)
            d = g - r
            head = max(head, float(((d ** 2).sum((0, 2)).sqrt() / (r ** 2).sum((0, 2)).sqrt().clamp_min(1e-30)).max()))
            row = max(row, float(((d ** 2).sum(2).sqrt() / (r ** 2).sum(2).sqrt().clamp_min(1e-30)).max()))
            mabs = max(mabs, float(d.abs().max()))
            zeros = zeros and bool((got[b, n:] == 0).all())
        nan2inf = lambda x: float('inf') if x != x else x
        sent = torch.tensor(SENTINEL).to(torch.bfloat16).float()
        return dict(head=nan2inf(head), row=nan2inf(row), abs=nan2inf(mabs), finite=fin, zeros=zeros,
                    cols=bool((buf[:B * Lq, D:] == sent).all()), rows=bool((buf[B * Lq:] == sent).all()))


def bitwise_ok(f):
    return f['finite'] and f['zeros'] and f['cols'] and f['rows']


def within_gates(f):
    return f['head'] < GATE_HEAD and f['row'] < GATE_ROW and f['abs'] < GATE_ABS


def caught(f):
    """a mistake counts as caught when a bitwise check breaks or a gated statistic is at three times its gate"""
    return (not bitwise_ok(f)) or f['head'] >= 3 * GATE_HEAD or f['row'] >= 3 * GATE_ROW or f['abs'] >= 3 * GATE_ABS


@functools.lru_cache(maxsize=8)
def attn_case(size, Lq, Lk, form, nkh):
    return AttnCase(size, Lq, Lk, form, nkh)
