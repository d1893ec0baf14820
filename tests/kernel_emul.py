"""Seeded inputs, fp64 references and CPU emulations for the kernel-level tests of the LayerNorm-algebra consumers (GEGLU GEMM, fused QKV GEMM, cross-attention
with its own q projection) and of the DUAL form of the un-split residual projection.  Test infrastructure, not code under test.

Every case is built on the CPU from a seeded torch.Generator.  A consumer's operand is A' = bf16(x g) of an fp32 x whose rows each have their own mean and spread; its
partial statistics are fp32 (sum, sum of squares) over zw-column parts, laid out part-major as a producer stores them, with NaN in every row >= M and every part >= zparts.

Two references per consumer case, both fp64:
  (a) same operand:  r (A' W^T - mu G') + C'  on the bf16 A' and the given fp32 partials merged in fp64 -- what the kernel computes, without its roundings;
  (b) true LayerNorm: (LN(x) g + c) W^T + b on the unrounded x -- what the algebra stands for.
The emulation repeats the kernel's documented rounding points in torch on the CPU (bf16 operand, fp32 accumulation, fp32 statistics merge and epilogue, bf16 store; attention:
P in bf16) but not its summation order.  `mut` selects one deliberate mistake (tests/test_host.py checks that every gate sees each of them)."""
import functools
import math

import torch

from ezaudio_amd.weights import _geglu8, _qkrope, qkrope_col

EPS = 1e-5
NAN = float('nan')

# ---- gates (rel-L2 unless noted): twice the worst value the emulation shows over the cases of the test (tests/test_host.py asserts that relation on the CPU), capped by the
# gate of the nearest older test: 4e-3 one bf16 output rounding, 5e-3 the bf16 rounding of x g against a true LayerNorm (ZIN), 1.2e-2 / 0.06 attention, 1e-5 fp32 output.
# Emulated floors (worst case over the test's shapes, this file, CPU): see DESIGN.md section 2 ("Kernel-level consumer tests") for the table with the values measured on MI355X.
GATE_GEGLU_A = 3.6e-3      # floor 1.8e-3 (one bf16 rounding of the output)
GATE_GEGLU_B = 5.0e-3      # floor 3.3e-3 (operand + output rounding); 2 x floor = 6.6e-3 is capped by the ZIN gate
GATE_GEGLU_B_FAR = 1.5e-2  # row means at five times the spread: floor 7.4e-3 (the bf16 rounding of x g grows with |mean| / sigma; the cap above belongs to |mean| <= sigma)
GATE_QKV_A = 4.0e-3        # worst head of q, k, v: floor 2.02e-3 (2 x floor = 4.04e-3, capped by the one-bf16-rounding gate)
GATE_QKV_B = 5.0e-3        # floor 2.9e-3; capped by the ZIN gate
GATE_QKT = 1.1e-3          # q . k^T per head on the scale |q| |k| (qkt_err): floor 5.3e-4
GATE_XATTN_A = 5.8e-3      # cross-attention output against (a): floor 2.87e-3 (q, P and O in bf16)
GATE_XATTN_B = 8.3e-3      # ... against (b): floor 4.14e-3
GATE_XATTN_ABS = 0.06      # max-abs: the attention test's (floor 0.039)
GATE_DUAL_H = 1.0e-5       # fp32 stream: floor 6.4e-8; the gate of the other fp32 outputs
GATE_DUAL_ZU = 3.0e-3      # one bf16 rounding: floor 1.68e-3; 2 x floor = 3.4e-3 is capped by the producer tests' gate
ULP_SHARE_CAP = 2.0        # share of elements not bit-equal to bf16(reference (a)) <= this x the share the emulation shows (+ the Poisson scatter of small counts: test_gpu.py)


def bf16r(x):
    return x.float().to(torch.bfloat16).float()


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def bf16_ulp_stats(got_bf16, ref64):
    """(largest distance in bf16 ulps, share of elements not bit-equal) between bf16 values and bf16(reference)."""
    want = ref64.float().to(torch.bfloat16)
    gi, wi = got_bf16.view(torch.int16).int(), want.view(torch.int16).int()
    # sign-magnitude -> monotone integers
    gi = torch.where(gi < 0, -(gi & 0x7fff), gi)
    wi = torch.where(wi < 0, -(wi & 0x7fff), wi)
    d = (gi - wi).abs()
    return int(d.max()), float((d != 0).double().mean())


# --------------------------------------------------------------------------------------------------------------------------------
# operand rows and their partial statistics
# --------------------------------------------------------------------------------------------------------------------------------
def make_rows(g, M, D, mean_scale=1.0):
    """fp32 [M][D]: row m has its own spread sigma_m in [1, 2) and its own mean, |mean| up to ~mean_scale sigma."""
    sig = 1 + torch.rand(M, 1, generator=g)
    return torch.randn(M, D, generator=g) * sig + mean_scale * sig * (2 * torch.rand(M, 1, generator=g) - 1)


def part_stats(x, zw, rows_alloc, parts_alloc=12):
    """fp32 (sum, sum of squares) of each zw-column part of each row, part-major [parts_alloc][rows_alloc][2]; NaN where the consumer must not look."""
    M, D = x.shape
    zparts = (D + zw - 1) // zw
    t = torch.full((parts_alloc, rows_alloc, 2), NAN)
    for p in range(zparts):
        c = x[:, p * zw:min((p + 1) * zw, D)].float()
        t[p, :M, 0], t[p, :M, 1] = c.sum(1), (c * c).sum(1)
    return t, zparts


def merge(stats, M, zparts, D, dtype, mut=None):
    """(mu, r) [M][1] from the partials, in `dtype` (fp64: reference; fp32: the kernel's one-pass form, common.h z_row_stats_finish)."""
    st = stats[:zparts, :M].to(dtype)
    if mut == 'row+1':
        st = torch.roll(st, -1, dims=1)
    if mut == 'drop_last_part':
        st = st[:zparts - 1]
    s, q = st[..., 0].sum(0), st[..., 1].sum(0)
    if mut == 'part_twice':
        s, q = s + st[0, :, 0], q + st[0, :, 1]
    mu = s / D
    var = (q / D - mu * mu).clamp_min(0)
    return mu[:, None], torch.rsqrt(var + EPS)[:, None]


def slots_of(M, rows_per_b, cur_step, row_slot):
    b = torch.arange(M) // rows_per_b
    return cur_step + (row_slot[b] if row_slot is not None else 0)


# --------------------------------------------------------------------------------------------------------------------------------
# a consumer GEMM up to the finish  r (acc - mu G') + C'
# --------------------------------------------------------------------------------------------------------------------------------
class Consumer:
    """x [M][D] -> LN(x) gam[slot] + bet[slot] -> Linear(W [N][D] bf16, bias): operands, tables and the finished projection (references and emulation)."""

    def __init__(self, g, M, D, zw, N, B, per_row, mean_scale=1.0, nslots=5, bias=True, w_scale=1.0):
        self.M, self.D, self.zw, self.N, self.B = M, D, zw, N, B
        self.rows_per_b = (M + B - 1) // B
        self.cur_step = 2
        self.row_slot = torch.tensor([(2 * b + 1) % 3 for b in range(B)], dtype=torch.int32) if per_row else None    # slots 2 .. 4 of 5
        self.nslots = nslots
        self.slot = slots_of(M, self.rows_per_b, self.cur_step, self.row_slot.long() if per_row else None) + torch.zeros(M, dtype=torch.long)
        x = make_rows(g, M, D, mean_scale)
        self.x = x
        self.gam = 1 + 0.3 * torch.randn(nslots, D, generator=g)
        self.bet = 0.3 * torch.randn(nslots, D, generator=g)
        self.W = (w_scale * torch.randn(N, D, generator=g) / D ** 0.5).to(torch.bfloat16)
        self.bias = 0.2 * torch.randn(N, generator=g) if bias else torch.zeros(N)
        self.A = (x * self.gam[self.slot]).to(torch.bfloat16)                       # A' = bf16(x g)
        self.rows_alloc = (M + 127) // 128 * 128 + 5
        self.stats, self.zparts = part_stats(x, zw, self.rows_alloc)
        Wd = self.W.double()
        self.G = (self.gam.double() @ Wd.T).float()                                  # G' [slots][N]
        self.C = (self.bet.double() @ Wd.T + self.bias.double()).float()             # C' [slots][N] (the bias folded in)

    def ref_a(self):
        mu, r = merge(self.stats, self.M, self.zparts, self.D, torch.float64)
        acc = self.A.double() @ self.W.double().T
        return r * (acc - mu * self.G.double()[self.slot]) + self.C.double()[self.slot]

    def ref_b(self):
        x = self.x.double()
        mu, var = x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
        y = (x - mu) / torch.sqrt(var + EPS) * self.gam.double()[self.slot] + self.bet.double()[self.slot]
        return y @ self.W.double().T + self.bias.double()

    @functools.cached_property
    def acc32(self):
        return self.A.float() @ self.W.float().T

    def emul(self, mut=None):
        """fp32: statistics merge, then fmaf(r, acc, fmaf(-(r mu), G', C')) as the epilogues do."""
        mu, r = merge(self.stats, self.M, self.zparts, self.D, torch.float32, mut)
        gs = (self.slot + 1) % self.nslots if mut == 'G_neighbour_slot' else self.slot
        return r * self.acc32 + (-(r * mu) * self.G[gs] + self.C[self.slot])


# ---- GEGLU ----
GEGLU_CASES = [(1000, 1152, 96, 576), (4000, 1152, 144, 576), (300, 576, 96, 584), (77, 160, 96, 576), (500, 1024, 96, 576), (1, 1152, 96, 576)]   # (M, D, zw, inner)
GEGLU_FAR_MEAN = (192, 1152, 96, 576)    # row means at five times the spread


@functools.lru_cache(maxsize=2)
def geglu_case(M, D, zw, inner, per_row, mean_scale=1.0):
    g = torch.Generator().manual_seed(1000 + M + D + zw + inner + int(per_row))
    return Consumer(g, M, D, zw, 2 * inner, 1 if M == 1 else 2, per_row, mean_scale)


def geglu(h):
    inner = h.shape[1] // 2
    return h[:, :inner] * torch.nn.functional.gelu(h[:, inner:])


def geglu_device_order(c):
    """(W, G', C', bias) with rows / columns in the interleaved 8 value / 8 gate order the GEMM reads (weights.py _geglu8)."""
    il = lambda t: _geglu8(t.T.contiguous()).T.contiguous()
    return _geglu8(c.W.float()).to(torch.bfloat16), il(c.G), il(c.C), _geglu8(c.bias.reshape(-1, 1)).reshape(-1)


# ---- fused QKV ----
QKV_HEADS = [(16, 72), (2, 72), (16, 64), (4, 64)]
QKV_BL = [(2, 500), (2, 77), (8, 500), (3, 131), (2, 1)]


def rope_tables64(L, dh):
    """rotary.py:42,56-68 as oracle/dit.py rope_tables builds them, [L][dh / 2] (the two halves of a head share one table)."""
    from oracle.dit import rope_tables
    import numpy as np
    inv_freq = (1.0 / (10000.0 ** (np.arange(0, dh, 2, dtype=np.float32) / np.float32(dh)))).astype(np.float32)
    cos, sin = rope_tables(L, inv_freq)
    return torch.from_numpy(cos[:, :dh // 2].copy()), torch.from_numpy(sin[:, :dh // 2].copy())


def head_ln(x, w, b, dh, n=None):
    """LayerNorm over the last axis ([.., dh]) with the shared affine; n: the divisor a wrong kernel would use."""
    n = n or dh
    mean = x.sum(-1, keepdim=True) / n
    d = x - mean
    var = ((d * d).sum(-1, keepdim=True) + (n - dh) * mean * mean) / n      # n > dh: zero padding columns counted
    return d * torch.rsqrt(var + EPS) * w + b


def rope(x, cos, sin, pos):
    """oracle/dit.py apply_rope: x cos + rotate_half(x) sin, rotate_half = [-x2 | x1]; x [M][H][dh], pos [M]."""
    half = x.shape[-1] // 2
    c, s = cos[pos][:, None, :].to(x.dtype), sin[pos][:, None, :].to(x.dtype)
    x1, x2 = x[..., :half], x[..., half:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)


class QkvCase:
    def __init__(self, H, dh, B, L, per_row, q_only=False):
        g = torch.Generator().manual_seed(2000 + 31 * H + dh + 7 * B + L + int(per_row) + 2 * int(q_only))
        D = H * dh
        self.H, self.dh, self.B, self.L, self.D, self.q_only = H, dh, B, L, D, q_only
        self.Lp = (L + 63) // 64 * 64
        self.DQK, self.DV = (64, 64) if dh == 64 else (80, 96)
        self.nparts = 1 if q_only else 3
        self.c = Consumer(g, B * L, D, 96, self.nparts * D, B, per_row, bias=False)
        self.c.rows_per_b = L
        self.qn_w, self.qn_b = 1 + 0.2 * torch.randn(dh, generator=g), 0.2 * torch.randn(dh, generator=g)
        self.kn_w, self.kn_b = 1 + 0.2 * torch.randn(dh, generator=g), 0.2 * torch.randn(dh, generator=g)
        self.cos, self.sin = rope_tables64(B * L, dh)     # (the launch gets the first L rows; the rest serves the position-not-reset mutation)

    def finish(self, y, dtype, cos=None, sin=None, mut=None):
        """finished projection [M][nparts D] -> (q, k, v) [B][H][L][dh] in `dtype`: split heads, LayerNorm per head, RoPE (not for the q-only form)."""
        M, H, dh = y.shape[0], self.H, self.dh
        cos, sin = (self.cos if cos is None else cos), (self.sin if sin is None else sin)
        pos = torch.arange(M) % self.L
        if mut == 'rope_no_reset':
            pos = torch.arange(M)
        out = []
        for part in range(self.nparts):
            t = y[:, part * self.D:(part + 1) * self.D].reshape(M, H, dh).to(dtype)
            if part < 2:
                w, b = (self.qn_w, self.qn_b) if part == 0 else (self.kn_w, self.kn_b)
                t = head_ln(t, w.to(dtype), b.to(dtype), dh, self.DQK if mut == 'ln_over_dqk' else None)
                if not self.q_only:
                    t = rope(t, cos, sin, pos)
                    if mut == 'rope_pair_swapped' and part == 0:
                        t = t.clone()
                        t[:, 1 % H, [3, 3 + dh // 2]] = t[:, 1 % H, [3 + dh // 2, 3]]
            out.append(t.reshape(self.B, self.L, H, dh).permute(0, 2, 1, 3))
        return out

    def ref_a(self, cos=None, sin=None):
        return self.finish(self.c.ref_a(), torch.float64, cos, sin)

    def ref_b(self):
        return self.finish(self.c.ref_b(), torch.float64)

    def emul(self, mut=None, cos=None, sin=None):
        return [bf16r(t) for t in self.finish(self.c.emul(mut), torch.float32, cos, sin, mut)]

    def col_order(self):
        """[2][dh]: channel that stored column cc of a head at tile position hh (= head % 2) holds (EZDIT_T_QKROPE)."""
        o = torch.zeros(2, self.dh, dtype=torch.long)
        for c in range(2 * self.dh):
            hh, ch = qkrope_col(self.dh, c)
            assert hh == c // self.dh
            o[hh, c % self.dh] = ch
        return o

    def device_weights(self):
        """(W, G', C') in the row / column order the launch reads: q and k rows in RoPE-pair order for the fused form, natural for the q-only form."""
        c = self.c
        if self.q_only:
            return c.W, c.G, c.C
        pk = lambda t: _qkrope(t.T.contiguous(), self.dh).T.contiguous()
        return _qkrope(c.W.float(), self.dh).to(torch.bfloat16), pk(c.G), pk(c.C)

    def unpermute(self, t):
        """q or k as stored ([B][H][L][dh], stored column order) -> natural channel order."""
        if self.q_only:
            return t
        o = self.col_order()
        out = torch.empty_like(t)
        for hh in range(2):
            out[:, hh::2][..., o[hh]] = t[:, hh::2]
        return out


@functools.lru_cache(maxsize=2)
def qkv_case(H, dh, B, L, per_row, q_only=False):
    return QkvCase(H, dh, B, L, per_row, q_only)


def per_head_rel(got, ref):
    """largest rel-L2 over the heads of [B][H][L][d] tensors."""
    g, r = got.double(), ref.double()
    num = ((g - r) ** 2).sum((0, 2, 3)).sqrt()
    den = (r ** 2).sum((0, 2, 3)).sqrt().clamp_min(1e-30)
    return float((num / den).max())


def qkt_err(q, k, qr, kr):
    """error of q . k^T per (batch element, head) on the scale of a dot product's rounding error, |q|_F |k|_F (the values themselves cancel to nothing when L = 1); worst head."""
    d = q.double() @ k.double().transpose(2, 3) - qr.double() @ kr.double().transpose(2, 3)
    num = (d ** 2).sum((0, 2, 3)).sqrt()
    den = ((qr.double() ** 2).sum((2, 3)) * (kr.double() ** 2).sum((2, 3))).sum(0).sqrt()
    return float((num / den).max())


# ---- cross-attention with its own q projection ----
XATTN_WIDTHS = [(16, 72), (6, 64)]                 # XL (xK = 1152) and a head_dim-64 width (xK = 384)
XATTN_B = [(2, 0, 2), (1, 1, 2), (2, 1, 4)]        # (B, b0, batch elements in the buffers)
XATTN_LQ = [500, 77, 1]
XATTN_VALID = [100, 12, 2]
POISON = 30.0                                       # V rows no query may see (masked keys and the padding rows [Lk, Lkp))


class XattnCase:
    def __init__(self, H, dh, Btot, Lq, n_valid, Lk=100):
        g = torch.Generator().manual_seed(3000 + 31 * H + dh + 7 * Btot + Lq + 3 * n_valid)
        D = H * dh
        self.H, self.dh, self.Btot, self.Lq, self.Lk, self.D = H, dh, Btot, Lq, Lk, D
        self.Lkp, self.Lqp = (Lk + 127) // 128 * 128, (Lq + 63) // 64 * 64
        self.DQK, self.DV = (64, 64) if dh == 64 else (80, 96)
        self.c = Consumer(g, Btot * Lq, D, 96, D, Btot, False, mean_scale=2.0, bias=False)     # (means up to twice the spread: a dropped or doubled part must show through two keys)
        self.c.rows_per_b = Lq
        self.qn_w, self.qn_b = 1 + 0.2 * torch.randn(dh, generator=g), 0.2 * torch.randn(dh, generator=g)
        self.k = torch.randn(Btot, H, self.Lkp, dh, generator=g).to(torch.bfloat16)     # rows >= Lk: finite values the mask must keep out
        self.v = torch.randn(Btot, H, self.Lkp, dh, generator=g).to(torch.bfloat16)
        self.k[0, 0, 3] *= 6.0                                                            # the spiked key of test_attention_against_softmax_reference
        self.mask = torch.zeros(Btot, Lk, dtype=torch.bool)
        for b in range(Btot):
            if b % 2 == 0:
                self.mask[b, :n_valid] = True
            else:
                self.mask[b, Lk - n_valid:] = True
        full = torch.zeros(Btot, self.Lkp, dtype=torch.bool)
        full[:, :Lk] = self.mask
        self.full = full
        self.v[~full[:, None, :].expand(Btot, H, self.Lkp)] = POISON

    def attend(self, y, dtype, emul=False, mut=None):
        B, H, dh = self.Btot, self.H, self.dh
        q = head_ln(y.reshape(B, self.Lq, H, dh).permute(0, 2, 1, 3).to(dtype), self.qn_w.to(dtype), self.qn_b.to(dtype), dh)
        if emul:
            q = bf16r(q)
        s = (q @ self.k.to(dtype).transpose(2, 3)) * dh ** -0.5
        m = self.full.clone()
        if mut == 'one_key_beyond_mask':
            m[:, self.Lk] = True      # the first padding row
        s = s.masked_fill(~m[:, None, None, :], float('-inf'))
        p = torch.exp(s - s.amax(-1, keepdim=True))
        o = ((bf16r(p) if emul else p) @ self.v.to(dtype)) / p.sum(-1, keepdim=True)
        o = o.permute(0, 2, 1, 3).reshape(B * self.Lq, self.D)
        return bf16r(o) if emul else o

    def ref_a(self):
        return self.attend(self.c.ref_a(), torch.float64)

    def ref_b(self):
        return self.attend(self.c.ref_b(), torch.float64)

    def emul(self, mut=None):
        return self.attend(self.c.emul(mut), torch.float32, True, mut)


@functools.lru_cache(maxsize=2)
def xattn_case(H, dh, Btot, Lq, n_valid):
    return XattnCase(H, dh, Btot, Lq, n_valid)


# ---- DUAL form of the un-split residual projection ----
DUAL_SHAPES = [(1000, 1152), (300, 576), (77, 160)]     # the shapes of test_skip_path_forms_of_the_residual_gemm


def dual_ranges(M):
    return {'empty': (0, 0), 'whole': (0, M), 'middle': (M // 5 + 3, M - M // 4 - 5)}     # ends on no tile boundary (tiles of 48 / 128 rows)


class DualCase:
    def __init__(self, M, D, B=4):
        g = torch.Generator().manual_seed(4000 + M + D)
        self.M, self.D, self.B, self.K = M, D, B, D
        self.rows_per_b = (M + B - 1) // B
        self.A = torch.randn(M, D, generator=g).to(torch.bfloat16)
        self.W = (torch.randn(D, D, generator=g) / D ** 0.5).to(torch.bfloat16)
        self.bias, self.gate = torch.randn(D, generator=g), torch.rand(D, generator=g)
        self.zg, self.zg2 = 1 + 0.3 * torch.randn(D, generator=g), 1 + 0.3 * torch.randn(D, generator=g)
        self.h_in = torch.randn(M, D, generator=g) + 0.7
        self.zd = torch.randn(B, D, generator=g)

    def forms(self, r0, r1, dtype, mut=None):
        """(h_out, zu before its bf16 rounding) in `dtype`."""
        acc = (self.A.double() @ self.W.double().T) if dtype == torch.float64 else (self.A.float() @ self.W.float().T)
        row = torch.arange(self.M)
        alt = ((row < r0) | (row >= r1))[:, None]
        h = self.h_in.to(dtype) + self.gate.to(dtype) * (acc + self.bias.to(dtype))
        zd = self.zd.to(dtype)[row // self.rows_per_b]
        h = h + (zd if mut == 'zd_inside' else torch.where(alt, zd, torch.zeros_like(zd)))
        return h, h * torch.where(alt, self.zg2.to(dtype), self.zg.to(dtype))


@functools.lru_cache(maxsize=2)
def dual_case(M, D):
    return DualCase(M, D)
