"""Seeded inputs, fp64 references, fp32 emulations and deliberate mistakes for the kernel-level tests of the streaming kernels of csrc/rowops.hip / csrc/rowbody.h:
the row operator (k_row, k_row_w), the per-head LayerNorm + RoPE (k_headnorm) and the input assembly (k_assemble).  Test infrastructure, not code under test; same shape as
tests/kernel_emul.py, whose helpers it imports.

Every case is built on the CPU from a seeded torch.Generator; every input is fp32 or bf16 exactly as the kernel reads it, so the fp64 reference sees the same numbers.  Rows
>= M of every input buffer hold NaN, output buffers are 8 rows longer than M and pre-filled with the finite sentinel 7.0 (tests/test_row_kernels_gpu.py).

Row operator, reference in fp64 (emulation: the same in fp32 with a bf16 store):
  h_new = h_in (COPY) | h_in + gate[slot] (sum_s part_s + bias) (RES) | sum_s part_s + bias (SET)
  u     = LN(h_new) ln_g[slot] + ln_c[slot] over D; with skip: LN over [h_new | skip + s_b cn] of width 2 D with ln_g / ln_c of length 2 D
  slot  = cur_step + row_slot[row / L],  s_b = cn_tab[row / L] or cn_scale,  eps = 1e-5
Rows of a case (as many as M holds, in this order; M = 1: the far-mean row alone):
  small     spread 1e-3: the variance is 1e-6, eps = 1e-5 decides the scale
  constant  variance 0: u must equal bf16(ln_c), and exactly 0 where ln_c is 0
  far       mean at five times the spread
  spike     (the last row when M >= 4, else the far row) 3 max(2, sqrt(width) / 4) added to the last four columns of the normalised width -- about a quarter of the
            row's sum of squares at every width: the chunk a wrong variance would lose
In the small and the constant row the slabs cancel the bias exactly (slab values 0, one slab = -bias, bias values bf16-exact), so that h_new IS the row described whatever
the order of the sum (the far row keeps ordinary slabs: half a spread of noise leaves its mean where it is).  Where no slab can do that (RES without slab, SET with fewer than two) the rows are special only before the bias: `exact_rows` is False, the constant-row
assertion and the `no_eps` mistake do not apply there.

Gates.  Measured on the fp32 emulation over ROW_CASES / HEAD_CASES (tests/test_row_kernels_host.py asserts the relations below on the CPU), never on the kernel:
  GATE_ROW_U / GATE_HEAD   worst ROW (worst head) rel-L2 of the bf16 output against the fp64 reference: twice the emulated floor, capped by kernel_emul.GATE_DUAL_ZU (one bf16
                           rounding).  Under the cap the emulation cannot keep a factor of two: it keeps its floor, as the capped gates of kernel_emul.py do.
  A_REL                    |got - ref64| <= 2^-8 |ref64| + A_REL (|ln_g| + |ln_c|): the first term is half a bf16 ulp, the second the fp32 error in front of the rounding
                           (twice the emulated worst; near-zero outputs are several ulps off, which is why this is not "one ulp").
  h_out                    elementwise (nsplit + 3) 2^-23 (|h_in| + |gate| (sum |part_s| + |bias|)): twice the standard fp32 summation bound, nothing measured.
  bit-equal share          elements of u, q, k not bit-equal to bf16(ref64): at most kernel_emul.ULP_SHARE_CAP x the emulation's count + the Poisson allowance of tests/test_gpu.py.
The emulation repeats the kernels' rounding points in torch, not their summation order, and torch's reciprocal square root is correctly rounded where the hardware's is
specified to one ulp: floors and counts are the worst of three emulations, with that factor exact, one fp32 ulp low and one high (`emul3`).
"""
import functools

import torch

from tests.kernel_emul import EPS, GATE_DUAL_ZU, NAN, ULP_SHARE_CAP, bf16_ulp_stats, bf16r, head_ln, make_rows, rel_l2, rope, rope_tables64  # noqa: F401

# ---- gates, each with the emulated floor behind it (CPU, worst over ROW_CASES / HEAD_CASES with the reciprocal square root exact and one ulp off either way).  The values
# measured on MI355X are in DESIGN.md section 2 ("Kernel-level tests of the streaming kernels").
GATE_ROW_U = GATE_DUAL_ZU   # worst row of u, D >= 64: emulated floor 2.39e-3 (a 64-column row); 2 x floor = 4.8e-3, capped by the one-bf16-rounding gate 3.0e-3
GATE_ROW_U_D4 = 4.0e-3      # ... of a four-column row: emulated floor 3.43e-3.  Four values, each up to half a bf16 ulp = 2^-8 = 3.9e-3 of itself off: the format's own bound on
                            # such a row is 2^-8, ABOVE the 3.0e-3 that holds as a root-mean-square over long rows; the gate here is the older tests' bound for one bf16
                            # rounding (tests/test_gpu.py, 4e-3), and the elementwise check below binds every one of the four values at half an ulp
GATE_HEAD = GATE_DUAL_ZU    # worst (batch element, head) of q / k: emulated floor 2.17e-3 (one position, 64 values); 2 x floor = 4.3e-3, capped
A_REL = 9.9e-7              # twice the emulated worst excess over half an ulp, 4.92e-7 (|ln_g| + |ln_c|)
FLOOR_ROW_U, FLOOR_ROW_U_D4, FLOOR_HEAD = 2.39e-3, 3.43e-3, 2.17e-3
SENTINEL = 7.0
PAD_ROWS = 8

ROW_MUTANTS = ('row+1', 'drop_last_slab', 'slab_twice', 'no_bias', 'gate_neighbour_slot', 'ln_neighbour_slot', 'slot_ignores_row_slot', 'last_chunk_out_of_variance',
               'no_eps', 'concat_mean_over_D', 'skip_half_uses_first_half_affine', 'cn_scalar_instead_of_table', 'cn_table_of_neighbour_batch', 'cn_unscaled')
H_MUTANTS = ('row+1', 'drop_last_slab', 'slab_twice', 'no_bias', 'gate_neighbour_slot')      # mistakes the fp32 stream shows (the others change u only, or h through the gate's slot)
HEAD_MUTANTS = ('rope_pair_swapped', 'rope_no_reset', 'ln_over_dqk', 'k_with_q_affine', 'rope_on_when_null', 'head+1')

COPY, RES, SET = 0, 1, 2
N_SLOTS = 5
CN_SCALE = 0.75
CN_TAB = (0.5, 1.25, 2.0)


def pad_rows(t, fill=NAN):
    """[M][..] -> [M + PAD_ROWS][..] with `fill` in the added rows."""
    out = torch.full((t.shape[0] + PAD_ROWS,) + tuple(t.shape[1:]), fill, dtype=t.dtype)
    out[:t.shape[0]] = t
    return out


class RowCase:
    """One launch of the row operator.  concat: None | 'skip' | 'cn' (scalar scale) | 'tab' (cn_tab of distinct values) | 'tab_eq' (cn_tab of the scalar's value)."""

    def __init__(self, D, M, mode, nsplit=0, bf16=True, bias=False, gate=False, B=1, cur_step=0, static=False, concat=None, h_out=True, inplace=False, u=True):
        self.key = dict(D=D, M=M, mode=mode, nsplit=nsplit, bf16=bf16, bias=bias, gate=gate, B=B, cur_step=cur_step, static=static, concat=concat, h_out=h_out,
                        inplace=inplace, u=u)
        self.__dict__.update(self.key)
        g = torch.Generator().manual_seed(5000 + 7 * D + M + 13 * mode + 3 * nsplit + int(bf16) + 2 * int(bias) + 4 * int(gate) + 17 * B + cur_step + len(concat or ''))
        self.L = (M + B - 1) // B
        self.width = 2 * D if concat else D
        self.ld_u = (self.width + 63) // 64 * 64
        self.part_bf16 = bool(bf16) and mode != COPY
        if mode == COPY:
            self.nsplit = nsplit = 0
            self.bias = bias = False
            self.gate = gate = False
        if mode == SET:
            self.gate = gate = False           # (the kernels apply the gate to the residual form only)
        # ---- which rows are special
        if M == 1:
            self.rows = dict(far=0, spike=0)
        elif M < 4:
            self.rows = dict(small=0, constant=1, far=2, spike=2)
        else:
            self.rows = dict(small=M // 3, constant=M // 3 + 1, far=2 * M // 3, spike=M - 1)
        cancel = {COPY: True, RES: nsplit >= 1, SET: nsplit >= 2}[mode]
        self.exact_rows = (not bias) or cancel
        # ---- the rows as they should leave: T (first half) and Y (the skip half before the ControlNet residual)
        halves = [make_rows(g, M, D) for _ in range(2 if concat else 1)]
        cval = 0.625
        for r_name, r in self.rows.items():
            if r_name == 'small':
                for t in halves:
                    t[r] = 1e-3 * (torch.randn(D, generator=g) + 0.5)
            elif r_name == 'constant':
                for t in halves:
                    t[r] = cval
            elif r_name == 'far':
                sig = 1.5
                for t in halves:
                    t[r] = sig * torch.randn(D, generator=g) + 5 * sig
        r = self.rows['spike']
        halves[-1][r, D - 4:] += 3.0 * max(2.0, self.width ** 0.5 / 4)      # about a quarter of the row's sum of squares, at every width
        T = halves[0]
        special = sorted(v for k, v in self.rows.items() if k in ('small', 'constant'))
        if self.part_bf16 and mode == SET:
            T[special] = bf16r(T[special])
        # ---- slabs, bias, gate
        self.bias_v = bf16r(0.2 * torch.randn(D, generator=g)) if bias else None      # (bf16-exact values: a bf16 slab can hold -bias)
        self.stride_pad = 0 if static else 12
        ns_tab = 1 if static else N_SLOTS
        gs = D + self.stride_pad
        self.gate_t = None
        if gate:
            self.gate_t = torch.full((ns_tab, gs), NAN)
            self.gate_t[:, :D] = 1 - 0.5 * torch.rand(ns_tab, D, generator=g)
        parts = None
        if mode != COPY:
            sig = T.std(1, keepdim=True) if D > 1 else torch.ones(M, 1)
            parts = 0.5 * sig * torch.randn(max(nsplit, 1), M, D, generator=g)
            if mode == SET and nsplit >= 1:
                parts[0] = T - parts[1:nsplit].sum(0) - (self.bias_v if bias else 0)
            parts[:, special] = 0
            if mode == SET and nsplit >= 1:
                parts[0, special] = T[special]
            if bias and cancel:
                parts[0 if mode == RES else 1, special] = -self.bias_v
            parts = parts[:nsplit]
            if self.part_bf16:
                parts = parts.to(torch.bfloat16)
        self.parts = parts
        self.h_in = None if mode == SET else T
        # ---- slots and LayerNorm tables
        if static:
            self.cur_step, self.row_slot = None, None
            self.slot = torch.zeros(M, dtype=torch.long)
        else:
            self.row_slot = torch.tensor([(2 * b + 1) % 3 for b in range(B)], dtype=torch.int32)
            self.slot = cur_step + self.row_slot.long()[torch.arange(M) // self.L]
        ls = self.width + self.stride_pad
        self.ln_g = torch.full((ns_tab, ls), NAN)
        self.ln_c = torch.full((ns_tab, ls), NAN)
        self.ln_g[:, :self.width] = 1 + 0.3 * torch.randn(ns_tab, self.width, generator=g)
        self.ln_c[:, :self.width] = 0.3 * torch.randn(ns_tab, self.width, generator=g)
        self.ln_c[:, 3:self.width:7] = 0.0
        # ---- skip half
        self.skip = self.cn = self.cn_tab = None
        self.cn_scale = 1.0
        if concat:
            Y = halves[1]
            self.skip = Y
            if concat != 'skip':
                sig = Y.std(1, keepdim=True)
                cn = 0.5 * sig * torch.randn(M, D, generator=g)
                if 'constant' in self.rows:
                    cn[self.rows['constant']] = 0
                self.cn = cn           # (half a spread of each row: the small row stays small, the constant row constant)
                self.cn_scale = CN_SCALE
                if concat == 'tab':
                    self.cn_tab = torch.tensor(CN_TAB[:B])
                elif concat == 'tab_eq':
                    self.cn_tab = torch.full((B,), CN_SCALE)

    def __repr__(self):
        return 'row(' + ', '.join(f'{k}={v}' for k, v in self.key.items()) + ')'

    # ---- the operator in `dtype`: (h_new [M][D], u before its bf16 rounding [M][width])
    def forward(self, dtype, mut=None, rsq_ulp=0):
        M, D = self.M, self.D
        rows = torch.arange(M)
        src = (rows + 1) % M if mut == 'row+1' else rows
        slot = self.slot
        if mut == 'slot_ignores_row_slot':
            slot = torch.full_like(slot, self.cur_step)
        if self.mode == SET:
            h = torch.zeros(M, D, dtype=dtype)
        else:
            h = self.h_in[src].to(dtype)
        if self.mode != COPY:
            s = torch.zeros(M, D, dtype=dtype)
            if self.bias and mut != 'no_bias':
                s = s + self.bias_v.to(dtype)
            slabs = [self.parts[i][src].to(dtype) for i in range(self.nsplit)]
            if mut == 'drop_last_slab':
                slabs = slabs[:-1]
            if mut == 'slab_twice':
                slabs = slabs + slabs[:1]
            for p in slabs:
                s = s + p
            if self.mode == RES:
                if self.gate:
                    gslot = (slot + 1) % self.gate_t.shape[0] if mut == 'gate_neighbour_slot' else slot
                    s = self.gate_t[gslot, :D].to(dtype) * s
                h = h + s
            else:
                h = s
        x = h
        if self.concat:
            y = self.skip[src].to(dtype)
            if self.cn is not None:
                b = rows // self.L
                if self.cn_tab is not None and mut != 'cn_scalar_instead_of_table':
                    sc = self.cn_tab[(b + 1) % self.B if mut == 'cn_table_of_neighbour_batch' else b].to(dtype)[:, None]
                else:
                    sc = torch.full((M, 1), self.cn_scale, dtype=dtype)
                if mut == 'cn_unscaled':
                    sc = torch.ones(M, 1, dtype=dtype)
                y = y + sc * self.cn[src].to(dtype)
            x = torch.cat([h, y], 1)
        W = x.shape[1]
        st = h if mut == 'concat_mean_over_D' else x
        mean = st.sum(1, keepdim=True) / st.shape[1]
        d = st - mean
        if mut == 'last_chunk_out_of_variance':
            d = d[:, :-4]
        var = (d * d).sum(1, keepdim=True) / st.shape[1]
        rstd = torch.rsqrt(var + (0.0 if mut == 'no_eps' else EPS))
        if rsq_ulp:
            rstd = rstd * torch.tensor(1 + rsq_ulp * 2.0 ** -23, dtype=dtype)
        lslot = (slot + 1) % self.ln_g.shape[0] if mut == 'ln_neighbour_slot' else slot
        lg, lc = self.ln_g[lslot, :W].to(dtype), self.ln_c[lslot, :W].to(dtype)
        if mut == 'skip_half_uses_first_half_affine':
            lg, lc = torch.cat([lg[:, :D], lg[:, :D]], 1), torch.cat([lc[:, :D], lc[:, :D]], 1)
        return h, (x - mean) * rstd * lg + lc

    @functools.cached_property
    def ref(self):
        return self.forward(torch.float64)

    def emul(self, mut=None, rsq_ulp=0):
        """rsq_ulp: the reciprocal square root one fp32 ulp high (+1) or low (-1) -- what the hardware instruction is specified to (1 ulp), torch's is correctly rounded"""
        h, u = self.forward(torch.float32, mut, rsq_ulp)
        return h, bf16r(u)

    @functools.cached_property
    def emul3(self):
        """the emulation with the reciprocal square root exact, one ulp low and one ulp high: floors and bit-equal shares are the worst of the three"""
        return [self.emul(None, k) for k in (0, -1, 1)]

    def applies(self, mut):
        """None if the mistake can be made (and seen) in this case, else the reason it cannot."""
        M, B = self.M, self.B
        slotted = not self.static
        if not self.u and (mut not in H_MUTANTS + ('slot_ignores_row_slot',) or (mut == 'slot_ignores_row_slot' and not self.gate)):
            return 'no LayerNorm output'
        if mut == 'row+1' and M == 1:
            return 'one row'
        if mut in ('drop_last_slab', 'slab_twice') and (self.mode == COPY or self.nsplit == 0):
            return 'no slab'
        if mut == 'no_bias' and not self.bias:
            return 'no bias'
        if mut == 'gate_neighbour_slot' and (not self.gate or not slotted):
            return 'no per-slot gate'
        if mut == 'ln_neighbour_slot' and not slotted:
            return 'static LayerNorm vectors'
        if mut == 'slot_ignores_row_slot' and not slotted:
            return 'no row_slot table'
        if mut == 'no_eps' and ('small' not in self.rows or not self.exact_rows):
            return 'no row whose variance is near eps'
        if mut in ('concat_mean_over_D', 'skip_half_uses_first_half_affine') and not self.concat:
            return 'no concatenation'
        if mut == 'cn_unscaled' and self.cn is None:
            return 'no cn'
        if mut == 'cn_scalar_instead_of_table' and self.concat != 'tab':
            return 'no cn_tab that differs from the scalar'
        if mut == 'cn_table_of_neighbour_batch' and (self.concat != 'tab' or B == 1):
            return 'no second batch element in cn_tab'
        return None

    def h_bound(self):
        """elementwise bound on |h_out - ref64|: (nsplit + 3) 2^-23 (|h_in| + |gate| (sum |part_s| + |bias|))"""
        M, D = self.M, self.D
        a = self.h_in.double().abs() if self.mode != SET else torch.zeros(M, D, dtype=torch.float64)
        if self.mode != COPY:
            s = torch.zeros(M, D, dtype=torch.float64)
            for i in range(self.nsplit):
                s = s + self.parts[i].double().abs()
            if self.bias:
                s = s + self.bias_v.double().abs()
            if self.gate:
                s = s * self.gate_t[self.slot, :D].double().abs()
            a = a + s
        return (self.nsplit + 3) * 2.0 ** -23 * a

    def u_scale(self):
        """|ln_g| + |ln_c| of every element of u [M][width]"""
        return self.ln_g[self.slot, :self.width].double().abs() + self.ln_c[self.slot, :self.width].double().abs()


def worst_row_rel(got, ref):
    """largest rel-L2 over the rows of [M][W]; a reference row of zeros counts on the scale of one (its outputs are exact zeros or bf16(ln_c))."""
    g, r = got.double(), ref.double()
    num = ((g - r) ** 2).sum(1).sqrt()
    den = (r ** 2).sum(1).sqrt().clamp_min(1e-30)
    e = num / den
    return float(torch.where(torch.isfinite(e), e, torch.full_like(e, float('inf'))).max())


def u_excess(got, ref, scale):
    """largest (|got - ref| - 2^-8 |ref|) / scale: the elementwise check passes where this is <= A_REL.  NaN / inf in `got` count as infinite."""
    e = ((got.double() - ref).abs() - 2.0 ** -8 * ref.abs()) / scale
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, float('inf')))
    return float(e.max())


def not_equal_count(got, ref64):
    """number of elements of the bf16-valued `got` that are not bit-equal to bf16(ref64)"""
    return int((got.float().to(torch.bfloat16).view(torch.int16) != ref64.float().to(torch.bfloat16).view(torch.int16)).sum())


def share_cap(n_emul, numel):
    """cap on the share of elements not bit-equal: ULP_SHARE_CAP x the emulation's count plus the Poisson allowance of tests/test_gpu.py (_assert_bf16_bits)"""
    return (ULP_SHARE_CAP * n_emul + 3 * (ULP_SHARE_CAP * n_emul) ** 0.5 + 3) / numel


def _row_cases():
    c = []
    add = lambda *a, **k: c.append(dict(zip(('D', 'M', 'mode'), a), **k))
    # every width at 133 rows (1284 and 2048: the workgroup form whatever the variant), residual form, two bf16 slabs, a slot per batch element
    for D in (4, 64, 160, 576, 1152, 1280, 1284, 2048):
        add(D, 133, RES, nsplit=2, bias=True, gate=True, B=3, cur_step=2)
    # the other row counts: one row, fewer rows than a workgroup's four, eight full panels; 1029: the second group of the XCD-affine row map
    for D in (4, 64, 160, 576, 1152, 1280):
        add(D, 1, RES, nsplit=1, bias=True, gate=True, B=1, cur_step=2)
        add(D, 3, SET, nsplit=3, bias=True, B=3, cur_step=2)
        add(D, 1024, RES, nsplit=4, bias=True, gate=True, B=3)
    add(64, 1029, RES, nsplit=1, bias=True, gate=True, B=3, cur_step=2)
    # COPY: the final LayerNorm (no h_out), with h_out, one row
    add(576, 133, COPY, h_out=False, B=3, cur_step=2)
    add(160, 133, COPY, static=True)
    add(1152, 1, COPY, B=1)
    # modes and slabs at 576 / 160 columns: 5 and 8 bf16 slabs, 2 fp32 slabs fall back to the workgroup form
    for ns in (1, 2, 3, 4, 5, 8):
        add(576, 133, SET, nsplit=ns, bias=ns % 2 == 0, B=3, cur_step=2)
        add(576 if ns < 4 else 160, 133, RES, nsplit=ns, bias=ns % 2 == 1, gate=ns != 2, B=3)
    add(576, 133, RES, nsplit=0, bf16=False, bias=True, gate=True, B=3)
    add(576, 133, SET, nsplit=1, bf16=False, static=True)                       # bit-exact
    add(1152, 133, RES, nsplit=1, bf16=False, B=3, cur_step=2)                 # LN1 of block 0 of a ControlNet forward: one fp32 slab, no gate
    add(576, 133, RES, nsplit=2, bf16=False, bias=True, gate=True, B=3)
    add(160, 3, SET, nsplit=2, bf16=False, bias=True, B=1)
    add(1152, 133, RES, nsplit=2, bias=True, gate=True, B=3, inplace=True)     # the cross-out edge
    add(576, 133, RES, nsplit=2, bias=True, gate=True, static=True)
    add(576, 133, RES, nsplit=2, bias=True, gate=True, B=3, u=False)           # no LayerNorm output
    # the concatenation [h_new | skip + s cn]: without cn, with the scalar, with a table of distinct values, with a table of the scalar's value
    full = dict(bias=True, gate=True, B=3, cur_step=2)
    for D in (160, 576, 1152):
        for concat in ('skip', 'cn', 'tab', 'tab_eq'):
            add(D, 133, RES, nsplit=2, concat=concat, **full)
    add(576, 1024, COPY, B=3, concat='tab')
    add(576, 3, SET, nsplit=2, bias=True, B=3, concat='tab')
    add(160, 1, COPY, concat='cn')
    add(1152, 133, COPY, static=True, concat='skip')
    # ... and the slab forms, the other widths and row counts under the per-prompt table (every mistake of ROW_MUTANTS can be made in these)
    for D in (160, 576, 1152):
        for ns in (1, 3, 4, 5, 8):
            add(D, 133, RES, nsplit=ns, concat='tab', **full)
    for D in (160, 576):
        for ns in (2, 4, 8):
            add(D, 133, SET, nsplit=ns, bias=True, B=3, cur_step=2, concat='tab')
    for ns in (1, 2):
        add(576, 133, RES, nsplit=ns, bf16=False, concat='tab', **full)
    for D in (4, 64, 1280, 1284, 2048):           # 1280: the wave form's five chunks per lane in both halves; above: the workgroup form
        add(D, 133, RES, nsplit=3, concat='tab', **full)
    add(160, 1024, RES, nsplit=3, concat='tab', **full)
    add(1152, 1024, RES, nsplit=2, concat='tab', **full)
    add(64, 1029, RES, nsplit=1, concat='tab', **full)
    add(1152, 133, RES, nsplit=2, concat='tab', inplace=True, bias=True, gate=True, B=3)
    for D in (64, 1280):
        add(D, 3, RES, nsplit=2, concat='tab', **full)
    for D in (4, 64, 1280):
        add(D, 133, RES, nsplit=1, concat='tab', **full)
    add(576, 1024, RES, nsplit=4, concat='tab', **full)
    for D, ns in ((1152, 3), (1152, 5), (1280, 2), (2048, 4)):
        add(D, 133, SET, nsplit=ns, bias=True, B=3, cur_step=2, concat='tab')
    return c


ROW_CASES = _row_cases()


@functools.lru_cache(maxsize=4)
def _row_case(items):
    return RowCase(**dict(items))


def row_case(spec):
    return _row_case(tuple(sorted(spec.items())))


def row_id(spec):
    m = {COPY: 'copy', RES: 'res', SET: 'set'}[spec['mode']]
    extra = ''.join(f'-{k}{"" if v is True else v}' for k, v in spec.items() if k not in ('D', 'M', 'mode') and v not in (False, None, 0))
    return f"D{spec['D']}-M{spec['M']}-{m}{extra}"


# --------------------------------------------------------------------------------------------------------------------------------
# head norm
# --------------------------------------------------------------------------------------------------------------------------------
HEAD_SHAPES = [(3, 72), (5, 64), (16, 72), (4, 64)]                       # (H, dh): an odd head count is what sends q / k / v through k_headnorm in a forward
HEAD_BL = [(2, 1, 64), (2, 77, 128), (3, 131, 256), (1, 300, 384)]        # (B, L, Lp)
HEAD_FORMS = ('qkv', 'kv', 'q')     # q + k + v with RoPE at ldx = 3 D | context k + v at ldx = 2 D, no RoPE | q alone at ldx = D, no RoPE (cross-attention, unfused projection)


class HeadCase:
    def __init__(self, H, dh, B, L, Lp, form):
        g = torch.Generator().manual_seed(6000 + 31 * H + dh + 7 * B + L + len(form))
        D = H * dh
        self.H, self.dh, self.B, self.L, self.Lp, self.form, self.D = H, dh, B, L, Lp, form, D
        self.M = B * L
        self.DQK, self.DV = (64, 64) if dh == 64 else (80, 96)
        self.cols = dict(qkv=(0, D, 2 * D), kv=(-1, 0, D), q=(0, -1, -1))[form]
        self.ldx = {'qkv': 3, 'kv': 2, 'q': 1}[form] * D
        self.rope_on = form == 'qkv'
        self.x = make_rows(g, self.M, self.ldx)
        # heads with their own mean and spread inside a row, one constant head (variance 0 -> the affine's shift alone)
        hs = 0.5 + torch.rand(1, self.ldx // dh, 1, generator=g)
        self.x = (self.x.reshape(self.M, -1, dh) * hs + (torch.rand(1, self.ldx // dh, 1, generator=g) - 0.5)).reshape(self.M, self.ldx).contiguous()
        self.x[self.M // 2, :dh] = 0.375
        self.qn_w, self.qn_b = 1 + 0.2 * torch.randn(dh, generator=g), 0.2 * torch.randn(dh, generator=g)
        self.kn_w, self.kn_b = 1 + 0.2 * torch.randn(dh, generator=g), 0.2 * torch.randn(dh, generator=g)
        self.cos, self.sin = rope_tables64(B * L, dh)     # fp32; the launch gets the first L rows, the rest serves `rope_no_reset`

    def __repr__(self):
        return f'head(H={self.H}, dh={self.dh}, B={self.B}, L={self.L}, Lp={self.Lp}, {self.form})'

    def parts(self):
        return [n for n, c in zip('qkv', self.cols) if c >= 0]

    def forward(self, dtype, mut=None, rsq_ulp=0):
        """dict part -> [B][H][L][dh] in `dtype` (v: the input itself); rsq_ulp: the normalised values scaled as by a reciprocal square root that many fp32 ulps off"""
        M, H, dh = self.M, self.H, self.dh
        pos = torch.arange(M) if mut == 'rope_no_reset' else torch.arange(M) % self.L
        out = {}
        for name, col in zip('qkv', self.cols):
            if col < 0:
                continue
            t = self.x[:, col:col + self.D].reshape(M, H, dh).to(dtype)
            if name != 'v':
                if mut == 'head+1':
                    t = torch.roll(t, -1, dims=1)
                w, b = (self.qn_w, self.qn_b) if (name == 'q' or mut == 'k_with_q_affine') else (self.kn_w, self.kn_b)
                t = head_ln(t, w.to(dtype), b.to(dtype), dh, self.DQK if mut == 'ln_over_dqk' else None)
                if rsq_ulp:
                    t = (t - b.to(dtype)) * torch.tensor(1 + rsq_ulp * 2.0 ** -23, dtype=dtype) + b.to(dtype)
                if self.rope_on or mut == 'rope_on_when_null':
                    t = rope(t, self.cos, self.sin, pos)
                    if mut == 'rope_pair_swapped':
                        t = t.clone()
                        t[:, 1 % H, [3, 3 + dh // 2]] = t[:, 1 % H, [3 + dh // 2, 3]]
            out[name] = t.reshape(self.B, self.L, H, dh).permute(0, 2, 1, 3)
        return out

    @functools.cached_property
    def ref(self):
        return self.forward(torch.float64)

    def emul(self, mut=None, rsq_ulp=0):
        return {k: bf16r(v) for k, v in self.forward(torch.float32, mut, rsq_ulp).items()}

    @functools.cached_property
    def emul3(self):
        return [self.emul(None, k) for k in (0, -1, 1)]

    def applies(self, mut):
        if mut in ('rope_pair_swapped', 'rope_no_reset') and not self.rope_on:
            return 'no RoPE'
        if mut == 'rope_no_reset' and self.B == 1:
            return 'one batch element'
        if mut == 'ln_over_dqk' and self.dh != 72:
            return 'DQK = dh'
        if mut == 'k_with_q_affine' and self.cols[1] < 0:
            return 'no k'
        if mut == 'rope_on_when_null' and (self.rope_on or self.L == 1):
            return 'RoPE is on' if self.rope_on else 'position 0 alone: the rotation is the identity'
        if mut == 'head+1' and self.H == 1:
            return 'one head'
        return None


HEAD_CASES = [(H, dh, B, L, Lp, form) for (H, dh), (B, L, Lp) in zip(HEAD_SHAPES * 4, [bl for i in range(4) for bl in HEAD_BL[i:] + HEAD_BL[:i]]) for form in HEAD_FORMS]


@functools.lru_cache(maxsize=4)
def head_case(H, dh, B, L, Lp, form):
    return HeadCase(H, dh, B, L, Lp, form)


def per_head_rel_qk(got, ref):
    """largest rel-L2 over (batch element, head) of [B][H][L][dh]"""
    g, r = got.double(), ref.double()
    num = ((g - r) ** 2).sum((2, 3)).sqrt()
    den = (r ** 2).sum((2, 3)).sqrt().clamp_min(1e-30)
    return float((num / den).max())


# --------------------------------------------------------------------------------------------------------------------------------
# input assembly
# --------------------------------------------------------------------------------------------------------------------------------
ASM_CASES = [(C, L, x_rows, form) for C in (8, 128) for L in (1, 77) for x_rows in (4, 2, 1) for form in ('plain', 'gt', 'pre') if not (form == 'pre' and x_rows != 4)]


class AsmCase:
    """B = 4 batch elements; lens = [L, 1, L - 1, 2] (L = 1: all 1) with NaN in x / gt beyond each length."""

    def __init__(self, C, L, x_rows, form, with_lens=True):
        g = torch.Generator().manual_seed(7000 + C + 3 * L + x_rows + len(form))
        B = 4
        self.B, self.C, self.L, self.x_rows, self.form = B, C, L, x_rows, form
        self.in_ch = 2 * C + 1 if form == 'pre' else C
        self.ldo = (2 * C + 1 + 63) // 64 * 64
        self.lens = torch.tensor([L, 1, max(L - 1, 1), min(2, L)], dtype=torch.int32) if with_lens else None
        rows = B if form == 'pre' else x_rows
        self.x = torch.randn(rows, self.in_ch, L, generator=g)
        self.mask_embed = torch.randn(C, generator=g)
        self.gt = self.gt_mask = None
        if form == 'gt':
            self.gt = torch.randn(x_rows, C, L, generator=g)
            m = torch.zeros(x_rows, C, L, dtype=torch.uint8)
            m[:, :, L // 3:L // 3 + max(L // 4, 1)] = 1          # a masked span, the same for every channel (channel 0 is the one read for the mask channel)
            m[0, 1:, :] = 1 - m[0, 1:, :] if C > 1 else m[0, 1:, :]   # ... but for latent row 0, whose other channels are masked where channel 0 is not
            self.gt_mask = m
        # NaN beyond the longest length among the batch elements that read a latent row: nothing there may reach the output
        if with_lens:
            for r in range(rows):
                n = max(int(self.lens[b]) for b in range(B) if b % rows == r)
                self.x[r, :, n:] = NAN
                if self.gt is not None:
                    self.gt[r, :, n:] = NAN

    def expected(self):
        """fp32 [B L][ldo]"""
        B, C, L = self.B, self.C, self.L
        out = torch.zeros(B, L, self.ldo)
        for b in range(B):
            if self.form == 'pre':
                out[b, :, :self.in_ch] = self.x[b].T
            else:
                r = b % self.x_rows
                out[b, :, :C] = self.x[r].T
                if self.gt is not None:
                    out[b, :, C:2 * C] = torch.where(self.gt_mask[r].T != 0, self.mask_embed[None, :].expand(L, C), self.gt[r].T)
                    out[b, :, 2 * C] = (self.gt_mask[r, 0] != 0).float()
                else:
                    out[b, :, C:2 * C] = self.mask_embed
                    out[b, :, 2 * C] = 1.0
            if self.lens is not None:
                out[b, int(self.lens[b]):] = 0.0
        return out.reshape(B * L, self.ldo)
