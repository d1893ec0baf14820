"""Cases, fp64 references, fp32 emulations in the kernels' order and deliberate mistakes for the kernel-level tests of the T5 encoder (csrc/t5.hip): k_t5_attn in both
operand forms, k_t5_embed_rms, k_t5_gated_gelu and the encoder's GEMM call (t5_gemm).  Test infrastructure, not code under test; the shape of tests/attn_emul.py,
tests/row_emul.py and tests/table_emul.py.  numpy throughout.  tests/t5_ref.py stays the judge of whole encodes.

ATTENTION.  A case is (L, max_len); B = 4 batch elements with a different key mask each (three taken in turn from MASK_KINDS, one with no valid key), H = 3 heads:
  head 0   the score-spread head: q holds +4 (even query rows) / -4 (odd rows) in channel 0 and key j holds (j // 32) there, so the 32-key sub-tiles form a staircase of
           whole log units, 4 per step, climbing for the even rows (their maximum lies in the LAST key tile) and falling for the odd ones (maximum in the first)
  head 1   the key-order head: V = r0 + 3 bit2(key) r1 + 5 bit3(key) r2 + 7 bit5(key) r3 (+ a little noise), r* random sign vectors over the 64 channels: keys 4 apart, 8 apart
           and in the two 32-key halves of a tile differ strongly.  Where a batch element masks key 0, the bias of distance -(L - 1) -- which only the pair (key 0, last query row)
           has -- is UNDERFLOW_BIAS = 300: that masked key's score (its bias alone, its K is staged as zeros) exceeds every valid score of the row by more than 104
  head 2   the P head: channel 1 of q is 2 and of key j is bit2(j) + 2 bit3(j) - 1.5 bit5(j): P differs by e^2, e^4 between keys 4 and 8 apart inside a 16-key group
The bias table holds an independent value in +-10 per (head, distance) -- not bucketed: every distance is distinguishable, and key - query from query - key -- in a row of
2 max_len - 1 slots, bias_half = max_len - 1; the slots outside the distances -(L - 1) .. L - 1 hold NaN.  Operands: the fp32 form is ONE buffer [rows][q | k | v] with
ld = 3 inner (k = q + inner), the bf16 form three buffers of ld = inner holding bf16(the same values); NaN in K and V at masked keys and in GUARD rows before row 0 and after row
B L - 1.  Half of the fp32 values lie a quarter of a bf16 ulp below a bf16 value (round to nearest goes up, truncation goes a whole ulp down).  out has ldo = 64 H + 8 and guard
rows, prefilled with SENTINEL.
  references  (a) fp64 on the bf16-rounded operands, (b) fp64 on the unrounded fp32 operands (fp32 form only)
  emulation   operands to bf16 (nearest even); scores by an fp32 product, bias added in fp32; row maximum over the valid keys only; exp in fp32; the row sum from the unrounded P;
              P V on bf16(P) with fp32 accumulation; o (1 / l); one bf16 rounding.  exp as numpy gives it and moved by a seeded +-1 and +-2 ulp (the device's __expf is
              specified to an accuracy, not to numpy's bits): a floor is the worst of the three.  Not modelled: the order of the fp32 sums inside an MFMA and of the row sum.
  gates       worst (batch element, head) rel-L2, worst query-row rel-L2 over its 64 values and max-abs, each 2 x ATTN_FLOORS (the emulation's worst over ALL cases; the host
              test recomputes them and holds this record to them).  Bitwise: finite, sentinels, zero rows of the empty element.
Mistakes that cannot show (ATTN_MUTANTS, `attn_applies`): every bias mistake at L = 1 (one key: the softmax is 1 whatever the score); bias_half_Lm1 at max_len = L; key_L_admitted
at L % 64 == 0 (no tile has a slot for key L); mask_ignored_last_tile where no element masks a key of the last tile; max_over_masked without the underflow construction (a larger
maximum alone only rescales P and l together); halves_not_combined and key_order_mismatch at L <= 4 (all keys in one lane half / none moved); stride_64H and truncation in the
bf16 form; empty_row_nan without an empty element (every case has one).  Truncation is made in every fp32 case but shows only from L = 31 on and, bitwise, at L = 1 (one key:
the result is bf16(v)); at L = 2 a softmax over at most two keys passes V through and one bf16 ulp of an operand is what the format itself allows a row.

NORM (k_t5_embed_rms).  Rows come from a table of NORM_VOCAB rows between NaN guard rows: row 3 carries most of its energy in the columns of the LAST 256-column pass, row 5 is
all zero, every row has its own amplitude and mean; ids are (3, V - 1, -1, 5, V + 5, 0, 3, random ...): 0, V - 1, repeats and the out-of-range -1 and V + 5, clamped by contract.
  bf16 output   within one bf16 ulp of fp64 (the existing test's gate); share of elements not bit-equal to bf16(fp64) <= share_cap(emulated count) (a condition; the host test checks
                that numpy float32 of the same operation stays under a third of the cap)
  fp32 output   |got - ref| <= norm_f32_rel(D) |ref|.  Derivation, u = 2^-24, P = ceil(D / 256) passes of a lane: a lane's partial is a sum of 4 P positive squares, each
                rounded (1 u) and added (4 P u along the longest path); six butterfly additions (6 u); the division by D and the addition of eps (2 u): the mean square carries
                (4 P + 9) u.  The reciprocal square root halves that, and is itself one rounding (1 u) of a device instruction specified to one ulp, 2 u more; the two products
                x r w add 2 u.  Together ((4 P + 9) / 2 + 5) u, taken with 1 % of slack for the second-order terms.  Nothing is measured.
Mistakes that cannot show: eps_omitted / eps_outside_root at stream scales 1 and 1e4 unless the case holds the zero row (eps_omitted: 0 x inf); neighbour_row at M = 1; id mistakes
on the x_in paths; id_not_clamped at M = 1 (no id out of range).

GATED GELU.  |got - ref| <= half a bf16 ulp at |ref| + e + e, e the fp32 term: with z = c (x + a x^3) (three products, one sum, one product: 5 u), t = tanh z within 2 ulp (4 u),
s = 1 + t (1 u), g = (0.5 x) s b (2 u):  e = |0.5 x b| (5 u |z| sech^2 z + 4 u |t| + 3 u s).  Share condition as above, counted over the elements whose e is below 1 % of half a
bf16 ulp (GeluCase.sel: about 70 %; below x of about -3.5 the sum 1 + t cancels and fp32 arithmetic, not the rounding, decides the bits -- a sixth of all elements differ
there in any fp32 evaluation, numpy's included, and a count over them hides the form of the function).  On that set the erf form and truncation lie many caps out.
Mistakes that cannot show: row_stride_F at M = 1.

GEMM.  |got - ref| <= (K + 3) 2^-24 (sum |a w| + |resid|) against the exact product of the bf16 operands: the derived bound of tests/vae_emul.py."""
import functools
import math

import numpy as np

f32, f64 = np.float32, np.float64
U24 = 2.0 ** -24
NAN = float('nan')
SENTINEL = -768.0              # exact in bf16; no kernel output of these tests comes near it
GUARD = 2                      # poisoned rows before and after every operand, sentinel rows around every output
MUT_FACTOR = 3.0               # a mistake counts as caught where it exceeds a gate this many times over, or breaks a bitwise check


def bf16r(x):
    """fp32 -> the nearest bf16 value (ties to even), as fp32; NaN stays NaN"""
    x = np.ascontiguousarray(x, dtype=f32)
    u = x.view(np.uint32)
    r = ((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
    out = ((u + r) & np.uint32(0xFFFF0000)).view(f32)
    return np.where(np.isnan(x), x, out)


def bf16t(x):
    """fp32 -> bf16 by truncation (a mistake)"""
    return (np.ascontiguousarray(x, dtype=f32).view(np.uint32) & np.uint32(0xFFFF0000)).view(f32)


def bf16_bits(x):
    """the 16 bits of bf16-valued fp32 numbers"""
    return (np.ascontiguousarray(x, dtype=f32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def bf16_ulp(x):
    """spacing of bf16 (8 significant bits) at |x|"""
    e = np.floor(np.log2(np.maximum(np.abs(np.asarray(x, f64)), 2.0 ** -126)))
    return 2.0 ** (e - 7)


def ulp_shift(x, n, seed):
    """fp32 array with every nonzero finite element moved by a seeded +n or -n ulp (n = 0: unchanged)"""
    x = np.ascontiguousarray(x, dtype=f32)
    if not n:
        return x
    s = np.random.default_rng(seed).integers(0, 2, size=x.shape, dtype=np.int32) * 2 - 1
    ok = np.isfinite(x) & (np.abs(x) > 2.0 ** -120)
    return np.where(ok, (x.view(np.int32) + s * np.int32(n)).view(f32), x)


def share_cap(n_emul, numel):
    """cap on the share of elements not bit-equal to bf16(reference): 2 x the emulation's count plus the Poisson scatter of a count (3 sigma + 3), as tests/row_emul.py"""
    return (2.0 * n_emul + 3 * (2.0 * n_emul) ** 0.5 + 3) / numel


def not_equal_count(got, ref64):
    return int((bf16_bits(got) != bf16_bits(bf16r(np.asarray(ref64, f64).astype(f32)))).sum())


def worst_ratio(got, ref, bound):
    """largest |got - ref| / bound; NaN / inf in `got` count as infinite"""
    with np.errstate(invalid='ignore', divide='ignore'):
        e = np.abs(np.asarray(got, f64) - ref) / bound
    e = np.where(np.abs(np.asarray(got, f64) - ref) == 0, 0.0, e)
    return float(np.where(np.isfinite(e), e, np.inf).max())


# --------------------------------------------------------------------------------------------------------------------------------
# attention
# --------------------------------------------------------------------------------------------------------------------------------
ATTN_LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 130, 511, 512)
ATTN_H, ATTN_B = 3, 4
UNDERFLOW_BIAS = 300.0
MASK_KINDS = ('prefix1', 'prefix_cut', 'full', 'key0_masked', 'suffix', 'every_third', 'last_only', 'tile_masked', 'half_masked')
ATTN_MUTANTS = ('last_valid_dropped', 'key_L_admitted', 'mask_ignored_last_tile', 'mask_of_b0', 'max_over_masked', 'halves_not_combined', 'scale_applied', 'bias_omitted',
                'bias_query_minus_key', 'bias_off_by_one', 'bias_of_head0', 'bias_half_Lm1', 'key_order_mismatch', 'v_halves_swapped', 'v_of_head_minus_1', 'stride_64H',
                'truncation', 'empty_row_nan', 'write_one_head_right')
QUANT = ('head', 'row', 'abs')

# emulated floors over all of attn_cases(): worst (batch element, head) rel-L2, worst query-row rel-L2, max-abs against reference (a) (both forms: their emulations are the same
# numbers) and against (b) (fp32 form), each the worst of the three exp evaluations.  A gate is 2 x its floor.  tests/test_t5_kernels_host.py recomputes them from the emulation
# and holds this record to them; the values measured on MI355X are in DESIGN.md section 2 ("Kernel-level tests of the T5 encoder").
ATTN_FLOORS = {'head_a': 1.91e-3, 'row_a': 3.64e-3, 'abs_a': 6.24e-2, 'head_b': 4.39e-3, 'row_b': 2.26e-2, 'abs_b': 1.21e-1}
ATTN_GATE_FACTOR = 2.0


def attn_max_lens(L):
    return tuple(dict.fromkeys([L] + ([300] if L <= 300 else []) + [512]))


def attn_specs():
    return [(L, ml) for L in ATTN_LENGTHS for ml in attn_max_lens(L)]


def make_mask(kind, L):
    """uint8 [L] or None where L does not allow the kind (or it would equal a simpler one)"""
    m = np.zeros(L, np.uint8)
    if kind == 'empty':
        return m
    if kind == 'full':
        m[:] = 1
    elif kind == 'prefix1':
        if L < 2:
            return None
        m[:1] = 1
    elif kind == 'prefix_cut':          # a cut inside a 64-key tile
        if L < 3:
            return None
        m[:max(2, min(L - 1, 64 * (L // 128) + 37))] = 1
    elif kind == 'key0_masked':
        if L < 3:
            return None
        m[1:] = 1
    elif kind == 'suffix':
        if L < 4:
            return None
        m[L - max(2, L // 3):] = 1
    elif kind == 'every_third':
        if L < 5:
            return None
        m[1::3] = 1
    elif kind == 'last_only':
        if L < 2:
            return None
        m[L - 1] = 1
    elif kind == 'tile_masked':         # a whole 64-key tile: the middle one, the first where there are two
        if L < 65:
            return None
        t = ((L + 63) // 64 - 1) // 2
        m[:] = 1
        m[64 * t:64 * t + 64] = 0
    elif kind == 'half_masked':         # the upper 32-key half of the last tile that has one
        if L < 34:
            return None
        t = (L - 33) // 64
        m[:] = 1
        m[64 * t + 32:64 * t + 64] = 0
    return m


class AttnCase:
    def __init__(self, L, max_len, index):
        self.L, self.max_len, self.index = L, max_len, index
        self.B, self.H = B, H = ATTN_B, ATTN_H
        self.I, self.ldo = 64 * H, 64 * H + 8
        self.bias_ld, self.bias_half = 2 * max_len - 1, max_len - 1
        rng = np.random.default_rng(1000 * L + max_len)
        kinds = [k for k in MASK_KINDS if make_mask(k, L) is not None]
        pick, seen = [], set()
        for j in range(len(kinds)):                              # three in turn, skipping a kind whose mask equals one already taken (L = 65: a masked tile leaves the last key)
            kd = kinds[(3 * index + j) % len(kinds)]
            if make_mask(kd, L).tobytes() not in seen and len(pick) < 3:
                pick.append(kd)
                seen.add(make_mask(kd, L).tobytes())
        pick += ['full'] * (3 - len(pick))
        pick.insert(index % 4, 'empty')
        self.kinds = tuple(pick)
        self.mask = np.stack([make_mask(k, L) for k in pick])
        self.empty = self.kinds.index('empty')
        self.underflow = bool(L >= 2 and any(m.any() and not m[0] for m in self.mask))
        # ---- bias table
        tab = np.full((H, self.bias_ld), NAN, f32)
        lo = self.bias_half - (L - 1)
        tab[:, lo:lo + 2 * L - 1] = rng.uniform(-10, 10, (H, 2 * L - 1)).astype(f32)
        if self.underflow:
            tab[1, lo] = UNDERFLOW_BIAS
        self.table = tab
        # ---- operands fp32 [B][L][H][64]
        q = (0.5 * rng.standard_normal((B, L, H, 64))).astype(f32)
        k = rng.standard_normal((B, L, H, 64)).astype(f32)
        v = rng.standard_normal((B, L, H, 64)).astype(f32)
        key = np.arange(L)
        b2, b3, b5 = ((key >> 2) & 1).astype(f32), ((key >> 3) & 1).astype(f32), ((key >> 5) & 1).astype(f32)
        r = rng.choice(np.array([-1.0, 1.0], f32), (4, 64))
        v[:, :, 1, :] = 0.25 * v[:, :, 1, :] + r[0] + 3 * b2[:, None] * r[1] + 5 * b3[:, None] * r[2] + 7 * b5[:, None] * r[3]
        # half of the values a quarter of a bf16 ulp below a bf16 value
        for a in (q, k, v):
            sel = rng.random(a.shape) < 0.5
            a[...] = np.where(sel, bf16r(a) * f32(1 - 2.0 ** -10), a)
        q[:, :, 0, 1:] *= f32(0.25)
        q[:, 0::2, 0, 0] = 4.0
        q[:, 1::2, 0, 0] = -4.0
        k[:, :, 0, 0] = (key // 32).astype(f32)[None, :]
        q[:, :, 2, 1] = 2.0
        k[:, :, 2, 1] = (b2 + 2 * b3 - 1.5 * b5)[None, :]
        self.q, self.k, self.v = q, k, v
        for a in (self.mask, self.table, q, k, v):
            a.setflags(write=False)

    def id(self):
        return f'L{self.L}-max{self.max_len}'

    # ---- buffers as the hooks get them -------------------------------------------------------------------------------------------
    @functools.lru_cache(maxsize=None)
    def operands(self, form):
        """(flat fp32 array, q offset, k offset, v offset, ld): form 'f32' one interleaved buffer, 'bf16' three buffers one after the other holding bf16 values"""
        B, L, I = self.B, self.L, self.I
        rows = B * L + 2 * GUARD
        keep = self.mask.reshape(B * L, 1).astype(bool)
        body = [a.reshape(B * L, I).copy() for a in (self.q, self.k, self.v)]
        body[1][~keep[:, 0]] = NAN
        body[2][~keep[:, 0]] = NAN
        if form == 'f32':
            buf = np.full((rows, 3 * I), NAN, f32)
            buf[GUARD:GUARD + B * L] = np.concatenate(body, 1)
            off = (0, I, 2 * I)
            ld = 3 * I
        else:
            buf = np.full((3, rows, I), NAN, f32)
            for i in range(3):
                buf[i, GUARD:GUARD + B * L] = bf16r(body[i])
            off = (0, rows * I, 2 * rows * I)
            ld = I
        flat = buf.reshape(-1)
        flat.setflags(write=False)
        return flat, off[0], off[1], off[2], ld

    def flat_table(self):
        return self.table.reshape(-1)

    # ---- references ---------------------------------------------------------------------------------------------------------------
    @functools.lru_cache(maxsize=None)
    def ref(self, which):
        """fp64 [B][L][H][64]: (a) on the bf16-rounded operands, (b) on the fp32 operands; rows of the empty element are 0"""
        r = (lambda a: bf16r(a).astype(f64)) if which == 'a' else (lambda a: a.astype(f64))
        keep = self.mask.astype(bool)
        q = r(self.q).transpose(0, 2, 1, 3)
        k = np.where(keep[:, :, None, None], r(self.k), 0.0).transpose(0, 2, 1, 3)
        v = np.where(keep[:, :, None, None], r(self.v), 0.0).transpose(0, 2, 1, 3)
        L, h = self.L, self.bias_half
        d = np.arange(L)[None, :] - np.arange(L)[:, None]                  # [query, key] = key - query
        bias = self.table.astype(f64)[:, h + d]                               # [H, query, key]
        s = q @ k.transpose(0, 1, 3, 2) + bias[None]
        kk = keep[:, None, None, :]
        s = np.where(kk, s, -np.inf)
        with np.errstate(invalid='ignore'):
            m = s.max(-1, keepdims=True)
            p = np.where(kk, np.exp(s - np.where(np.isfinite(m), m, 0.0)), 0.0)
            o = (p @ v) / p.sum(-1, keepdims=True)
        o = np.where(keep.any(1)[:, None, None, None], o, 0.0).transpose(0, 2, 1, 3)
        o = np.ascontiguousarray(o)
        o.setflags(write=False)
        return o

    # ---- emulation ----------------------------------------------------------------------------------------------------------------
    def emul(self, form, mut=None, exp_ulp=0, stats=None):
        """the out buffer [(GUARD + B L + GUARD)][ldo] as fp32 holding bf16 values; `stats` (dict) receives the coverage counts"""
        B, H, L, I = self.B, self.H, self.L, self.I
        flat, qo, ko, vo, ld = self.operands(form)
        if mut == 'stride_64H':
            ld = I
        nkt = (L + 63) // 64
        Lk = L + 1 if mut == 'key_L_admitted' else L
        keyi = np.arange(Lk)
        src = np.minimum(keyi, L - 1)                        # the clamped load
        mask = self.mask.astype(bool)
        if mut == 'mask_of_b0':
            mask = np.broadcast_to(mask[:1], mask.shape).copy()
        valid = mask[:, src].copy()                          # [B, Lk]
        if mut == 'key_L_admitted':
            valid[:, L] = True
        if mut == 'mask_ignored_last_tile':
            valid[:, 64 * (nkt - 1):] = True
        if mut == 'last_valid_dropped':
            for b in range(B):
                nz = np.flatnonzero(valid[b])
                if len(nz):
                    valid[b, nz[-1]] = False
        cvt = bf16t if mut == 'truncation' else bf16r

        def load(off, rows, hshift=0):
            idx = off + (GUARD + np.arange(B)[:, None, None, None] * L + rows[None, :, None, None]) * ld + (np.arange(H)[None, None, :, None] + hshift) * 64 \
                + np.arange(64)[None, None, None, :]
            return cvt(flat[np.clip(idx, 0, len(flat) - 1)]).transpose(0, 2, 1, 3)     # [B, H, rows, 64]
        qb = load(qo, np.arange(L))
        kz = np.where(valid[:, None, :, None], load(ko, src), f32(0))
        vz = np.where(valid[:, None, :, None], load(vo, src, -1 if mut == 'v_of_head_minus_1' else 0), f32(0))
        # ---- bias, fp32 [H, query, key]
        tab = np.concatenate([np.full(4, NAN, f32), self.flat_table(), np.full(1024, NAN, f32)])
        half = L - 1 if mut == 'bias_half_Lm1' else self.bias_half
        dist = keyi[None, :] - np.arange(L)[:, None]
        if mut == 'bias_query_minus_key':
            dist = -dist
        if mut == 'bias_off_by_one':
            dist = dist + 1
        hb = np.zeros(H, np.int64) if mut == 'bias_of_head0' else np.arange(H)
        bias = tab[4 + hb[:, None, None] * self.bias_ld + half + dist[None]]
        if mut == 'bias_omitted':
            bias = np.zeros_like(bias)
        with np.errstate(invalid='ignore', over='ignore'):
            s = qb @ kz.transpose(0, 1, 3, 2)                                # fp32 [B, H, L, Lk]
            if mut == 'scale_applied':
                s = s * f32(0.125)
            s = s + bias[None]
            vk = valid[:, None, None, :]
            inmax = np.broadcast_to((keyi < L)[None, None, None, :], s.shape) if mut == 'max_over_masked' else np.broadcast_to(vk, s.shape)
            neg = f32(-1e30)
            if mut == 'halves_not_combined':
                hi = ((keyi >> 2) & 1).astype(bool)
                m0 = np.maximum(neg, np.where(inmax & ~hi, s, -np.inf).max(-1, keepdims=True))
                m1 = np.maximum(neg, np.where(inmax & hi, s, -np.inf).max(-1, keepdims=True))
                m = np.where(hi, m1, m0)
            else:
                m = np.maximum(neg, np.where(inmax, s, -np.inf).max(-1, keepdims=True))
            p = np.where(vk, ulp_shift(np.exp((s - m).astype(f32)), exp_ulp, 77 + self.L), f32(0)).astype(f32)
            lsum = p.sum(-1, dtype=f32)
            if stats is not None:
                sv = np.where(vk, s, -np.inf)
                am = sv.argmax(-1)
                has = vk.any(-1) & np.ones_like(am, bool)
                stats['max_in_last_tile'] = int((has & (am // 64 == nkt - 1)).sum()) if nkt > 1 else 0
                stats['max_in_first_tile'] = int((has & (am // 64 == 0)).sum()) if nkt > 1 else 0
                sm = np.where(~vk & (keyi < L)[None, None, None, :], s, -np.inf).max(-1)
                stats['underflow_rows'] = int((has & (sm - sv.max(-1) > 104)).sum())
            # ---- P V in the order of the V^T fragment
            pad = 64 * nkt + 64
            vp = np.zeros((B, H, pad, 64), f32)
            vp[:, :, :Lk] = vz
            kk = np.arange(Lk)
            if mut == 'key_order_mismatch':                   # natural order on the V side only: bits 2 and 3 of the key change places
                kk = (kk & ~12) | ((kk & 4) << 1) | ((kk & 8) >> 1)
            if mut == 'v_halves_swapped':
                kk = kk ^ 32
            o = bf16r(p) @ vp[:, :, kk]
            inv = np.where(lsum > 0, f32(1) / np.where(lsum > 0, lsum, f32(1)), f32(0)).astype(f32)
            res = bf16r(o * inv[..., None])
            if mut == 'empty_row_nan':
                res = np.where((lsum > 0)[..., None], res, f32(NAN))
        out = np.full((B * L + 2 * GUARD) * self.ldo, SENTINEL, f32)
        col = np.arange(H)[None, :, None, None] * 64 + (64 if mut == 'write_one_head_right' else 0) + np.arange(64)[None, None, None, :]
        idx = (GUARD + np.arange(B)[:, None, None, None] * L + np.arange(L)[None, None, :, None]) * self.ldo + col
        out[idx.reshape(-1)] = res.reshape(-1)
        return out.reshape(-1, self.ldo)

    # ---- judging ------------------------------------------------------------------------------------------------------------------
    def body(self, out):
        """[B][L][H][64] of an out buffer"""
        return out[GUARD:GUARD + self.B * self.L, :self.I].reshape(self.B, self.L, self.H, 64)

    def bitwise_ok(self, out):
        """finite; sentinels intact; the empty element's rows zero; at L = 1 the softmax is exactly 1 (exp(0), l = 1) and the result is bf16(v) bit for bit"""
        o = self.body(out)
        ok = bool(np.isfinite(o).all() and (out[:GUARD] == SENTINEL).all() and (out[GUARD + self.B * self.L:] == SENTINEL).all()
                  and (out[:, self.I:] == SENTINEL).all() and (o[self.empty] == 0).all())
        if ok and self.L == 1:
            ok = np.array_equal(bf16_bits(o), bf16_bits(self.ref('a').astype(f32)))
        return ok

    def measure(self, out, which):
        """{'head', 'row', 'abs'} of an out buffer against reference `which`; anything not finite counts as infinite"""
        got, ref = self.body(out).astype(f64), self.ref(which)
        live = [b for b in range(self.B) if b != self.empty]
        d, r = got[live] - ref[live], ref[live]
        if not np.isfinite(d).all():
            return dict(head=np.inf, row=np.inf, abs=np.inf)
        head = np.sqrt((d ** 2).sum((1, 3))) / np.maximum(np.sqrt((r ** 2).sum((1, 3))), 1e-30)
        row = np.sqrt((d ** 2).sum(3)) / np.maximum(np.sqrt((r ** 2).sum(3)), 1e-30)
        return dict(head=float(head.max()), row=float(row.max()), abs=float(np.abs(d).max()))


@functools.lru_cache(maxsize=None)
def attn_case(L, max_len):
    return AttnCase(L, max_len, attn_specs().index((L, max_len)))


def attn_gates(floors=None):
    f = ATTN_FLOORS if floors is None else floors
    return {k: ATTN_GATE_FACTOR * v for k, v in f.items()}


def attn_refs(form):
    return ('a', 'b') if form == 'f32' else ('a',)


def attn_within(c, out, form, gates=None, factor=1.0):
    """every gated quantity of the form at most factor x its gate"""
    g = attn_gates() if gates is None else gates
    return all(c.measure(out, w)[qn] <= factor * g[f'{qn}_{w}'] for w in attn_refs(form) for qn in QUANT)


def attn_caught(c, out, form, gates=None):
    g = attn_gates() if gates is None else gates
    if not c.bitwise_ok(out):
        return True
    return any(c.measure(out, w)[qn] > MUT_FACTOR * g[f'{qn}_{w}'] for w in attn_refs(form) for qn in QUANT)


def attn_applies(c, form, mut):
    """False where the mistake cannot show (the module docstring says why)"""
    L = c.L
    nkt = (L + 63) // 64
    if mut.startswith('bias_') and L == 1:
        return False
    if mut == 'bias_half_Lm1':
        return c.max_len != L
    if mut == 'key_L_admitted':
        return L % 64 != 0
    if mut == 'mask_ignored_last_tile':
        return bool((c.mask[:, 64 * (nkt - 1):] == 0)[[b for b in range(c.B) if b != c.empty]].any())
    if mut == 'mask_of_b0':
        return L > 1 or c.empty != 0
    if mut == 'max_over_masked':
        return c.underflow
    if mut in ('halves_not_combined', 'key_order_mismatch'):
        return L > 4
    if mut == 'scale_applied':
        return L > 1
    if mut in ('stride_64H', 'truncation'):
        return form == 'f32'
    return True


def attn_floors(specs=None):
    """the floors of ATTN_FLOORS from the emulation: worst over the cases and the three exp evaluations"""
    fl = {k: 0.0 for k in ATTN_FLOORS}
    for L, ml in (attn_specs() if specs is None else specs):
        c = attn_case(L, ml)
        for n in (0, 1, 2):
            out = c.emul('f32', exp_ulp=n)
            for w in 'ab':
                for qn, val in c.measure(out, w).items():
                    fl[f'{qn}_{w}'] = max(fl[f'{qn}_{w}'], val)
    return fl


# --------------------------------------------------------------------------------------------------------------------------------
# norm
# --------------------------------------------------------------------------------------------------------------------------------
NORM_D = (64, 68, 128, 192, 260, 2048)
NORM_M = (1, 3, 4, 5, 133)
NORM_SCALES = (1.0, 1e4, 1e-4)
NORM_PATHS = ('x_bf16', 'x_f32', 'ids_bf16', 'ids_f32')
NORM_VOCAB = 13
NORM_EPS = 1e-6
ENERGY_ROW, ZERO_ROW = 3, 5
NORM_MUTANTS = ('mean_subtracted', 'div_D_minus_1', 'eps_omitted', 'eps_outside_root', 'w_col_plus_1', 'w_col_plus_4', 'neighbour_row', 'last_pass_lost', 'id_plus_1',
                'id_not_clamped')


def norm_f32_rel(D):
    P = (D + 255) // 256
    return ((4 * P + 9) / 2 + 5) * U24 * 1.01


class NormCase:
    def __init__(self, D, M, scale):
        self.D, self.M, self.scale, self.V = D, M, scale, NORM_VOCAB
        rng = np.random.default_rng(7 * D + 1000 * M + int(abs(math.log10(scale))))
        V = self.V
        amp = rng.uniform(0.5, 2.0, (V, 1))
        tab = (amp * (rng.standard_normal((V, D)) + 0.5 * rng.uniform(-1, 1, (V, 1))))
        tab[:, ::7] *= 1e-3                                     # small entries next to large ones
        last = 256 * ((D + 255) // 256 - 1)
        tab[ENERGY_ROW, last:] *= 30.0
        tab[ZERO_ROW] = 0.0
        self.emb = np.full((V + 2 * GUARD, D), NAN, f32)         # the table between NaN guard rows
        self.emb[GUARD:GUARD + V] = (tab * scale).astype(f32)
        ids = [ENERGY_ROW, V - 1, -1, ZERO_ROW, V + 5, 0, ENERGY_ROW] + list(rng.integers(0, V, max(0, M - 7)))
        self.ids = np.array(ids[:M], np.int32)
        self.w = (1 + 0.1 * rng.uniform(-1, 1, D)).astype(f32)
        self.x = self.table()[np.clip(self.ids, 0, V - 1)]       # what x_out must hold, and the input of the x_in paths
        self.has_zero = bool((self.ids == ZERO_ROW).any())
        for a in (self.emb, self.ids, self.w, self.x):
            a.setflags(write=False)

    def table(self):
        return self.emb[GUARD:GUARD + self.V]

    def id(self):
        return f'D{self.D}-M{self.M}-s{self.scale:g}'

    @functools.lru_cache(maxsize=None)
    def ref(self):
        x = self.x.astype(f64)
        return x / np.sqrt((x * x).mean(-1, keepdims=True) + NORM_EPS) * self.w.astype(f64)

    def emul(self, path, mut=None, rsq_ulp=0):
        """(result fp32 [M][D] -- bf16 values on the bf16 paths --, x_out or None) in the kernel's order: 64 lane partials of squares, the xor butterfly, rsqrt, two products"""
        D, M, V = self.D, self.M, self.V
        gather = path.startswith('ids')
        if gather:
            ids = self.ids.astype(np.int64)
            if mut != 'id_not_clamped':
                ids = np.clip(ids, 0, V - 1)
            if mut == 'id_plus_1':
                ids = ids + 1
            x = self.emb[np.clip(GUARD + ids, 0, V + 2 * GUARD - 1)]
        else:
            x = self.x
        x = np.ascontiguousarray(x, f32)
        with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
            xs = x - x.mean(-1, keepdims=True, dtype=f32) if mut == 'mean_subtracted' else x
            P = (D + 255) // 256
            xp = np.zeros((M, P * 256), f32)
            xp[:, :D] = xs
            xp = xp.reshape(M, P, 64, 4)
            if mut == 'last_pass_lost':
                xp = xp[:, :P - 1] if P > 1 else xp * f32(0)
            sq = xp * xp
            ss = np.zeros((M, 64), f32)
            for p in range(sq.shape[1]):
                ss = ss + (((sq[:, p, :, 0] + sq[:, p, :, 1]) + sq[:, p, :, 2]) + sq[:, p, :, 3])
            lane = np.arange(64)
            for o in (32, 16, 8, 4, 2, 1):
                ss = ss + ss[:, lane ^ o]
            ss = ss[:, :1]
            if mut == 'neighbour_row':
                ss = np.roll(ss, -1, 0)
            ms = ss / f32(D - 1 if mut == 'div_D_minus_1' else D)
            eps = f32(NORM_EPS)
            if mut == 'eps_omitted':
                r = f32(1) / np.sqrt(ms)
            elif mut == 'eps_outside_root':
                r = f32(1) / (np.sqrt(ms) + eps)
            else:
                r = (1.0 / np.sqrt((ms + eps).astype(f64))).astype(f32)      # correctly rounded, then moved by rsq_ulp
            r = np.ascontiguousarray(r, f32)
            if rsq_ulp:
                r = np.where(np.isfinite(r), (r.view(np.int32) + np.int32(rsq_ulp)).view(f32), r)
            w = self.w
            if mut == 'w_col_plus_1':
                w = np.concatenate([w[1:], [f32(NAN)]])
            if mut == 'w_col_plus_4':
                w = np.concatenate([w[4:], np.full(4, NAN, f32)])
            o = (xs * r) * w
        res = o.astype(f32) if path.endswith('f32') else bf16r(o)
        return res, (x if gather else None)

    def emul3(self, path):
        return [self.emul(path, rsq_ulp=n)[0] for n in (0, -1, 1)]

    @functools.lru_cache(maxsize=None)
    def share_cap(self, path='x_bf16'):
        """(cap on the share not bit-equal, the emulation's count: the worst of the reciprocal square root exact and one ulp off either way)"""
        n = max(not_equal_count(e, self.ref()) for e in self.emul3(path))
        return share_cap(n, self.M * self.D), n

    def verdict(self, path, res, x_out, x_path_res=None):
        """(bitwise ok, worst error over its gate, share over its cap or 0) of one path's outputs"""
        ref = self.ref()
        bit = bool(np.isfinite(res).all())
        if path.startswith('ids'):
            bit = bit and x_out is not None and np.array_equal(x_out.view(np.uint32), self.x.view(np.uint32))
            if x_path_res is not None:
                bit = bit and np.array_equal(np.asarray(res, f32).view(np.uint32), np.asarray(x_path_res, f32).view(np.uint32))
        if path.endswith('f32'):
            return bit, worst_ratio(res, ref, norm_f32_rel(self.D) * np.abs(ref)), 0.0
        cap, _ = self.share_cap()
        return bit, worst_ratio(res, ref, bf16_ulp(ref)), not_equal_count(res, ref) / res.size / cap

    def applies(self, path, mut):
        if mut.startswith('id_'):
            return path.startswith('ids') and (mut == 'id_plus_1' or bool(((self.ids < 0) | (self.ids >= self.V)).any()))
        if mut == 'eps_omitted':
            return self.scale == 1e-4 or self.has_zero
        if mut == 'eps_outside_root':
            return self.scale == 1e-4
        if mut == 'neighbour_row':
            return self.M > 1
        return True


def norm_specs():
    return [(D, M, s) for D in NORM_D for M in NORM_M for s in NORM_SCALES]


@functools.lru_cache(maxsize=None)
def norm_case(D, M, scale):
    return NormCase(D, M, scale)


def norm_caught(bit, err, share):
    return (not bit) or err > MUT_FACTOR or share > MUT_FACTOR


# --------------------------------------------------------------------------------------------------------------------------------
# gated GELU
# --------------------------------------------------------------------------------------------------------------------------------
GELU_F = (64, 192, 256, 5120)
GELU_M = (1, 3, 5)
GELU_MUTANTS = ('halves_swapped', 'erf_form', 'cubic_dropped', 'row_stride_F', 'col_plus_4', 'truncation')
GELU_C, GELU_A = 0.7978845608028654, 0.044715


class GeluCase:
    def __init__(self, M, F):
        self.M, self.F = M, F
        rng = np.random.default_rng(31 * F + M)
        a = rng.uniform(-6, 6, (M, F))
        n = M * F
        flat = a.reshape(-1)
        sp = np.array([0.0, -0.0, 1e-40, -1e-40, 1e-45, 7.0, -7.0, 30.0, -30.0, 1e3, -1e3, 1e4, -1e4, 1e13, -1e13, 1e14, -1e14, 1e20, -1e20, 6.0, -6.0, 1e-8, -1e-8])
        pos = (np.arange(len(sp)) * 2 + 1) % n
        flat[pos] = sp
        b = np.sign(rng.uniform(-1, 1, (M, F))) * 10.0 ** rng.uniform(-3, 4, (M, F))
        h = np.full((M + 2 * GUARD, 2 * F), NAN, f32)
        h[GUARD:GUARD + M, :F] = flat.reshape(M, F).astype(f32)
        h[GUARD:GUARD + M, F:] = b.astype(f32)
        self.h = h
        h.setflags(write=False)

    def id(self):
        return f'M{self.M}-F{self.F}'

    def ab(self):
        return self.h[GUARD:GUARD + self.M, :self.F], self.h[GUARD:GUARD + self.M, self.F:]

    @functools.lru_cache(maxsize=None)
    def ref(self):
        a, b = (t.astype(f64) for t in self.ab())
        return 0.5 * a * (1.0 + np.tanh(GELU_C * (a + GELU_A * a ** 3))) * b

    @functools.lru_cache(maxsize=None)
    def bound(self):
        """half a bf16 ulp at |ref| + e, + e: the fp32 term of the module docstring"""
        a, b = (t.astype(f64) for t in self.ab())
        with np.errstate(over='ignore'):
            z = GELU_C * (a + GELU_A * a ** 3)
            t = np.tanh(z)
            e = np.abs(0.5 * a * b) * (5 * U24 * np.abs(z) / np.cosh(np.minimum(np.abs(z), 300.0)) ** 2 + 4 * U24 * np.abs(t) + 3 * U24 * (1 + t)) + 2.0 ** -149
        bound = 0.5 * bf16_ulp(np.abs(self.ref()) + e) + e
        # the share condition counts the elements whose fp32 term is below 1 % of half a bf16 ulp: elsewhere (x below about -3.5, where 1 + tanh cancels) the fp32
        # arithmetic, not the rounding, decides the bits, and a count there says nothing about the form of the function
        self._sel = (e <= 0.005 * bf16_ulp(self.ref())) & (np.abs(self.ref()) > 2.0 ** -100)
        return bound

    def sel(self):
        self.bound()
        return self._sel

    def emul(self, mut=None, tanh_ulp=0):
        M, F = self.M, self.F
        flat = self.h.reshape(-1)
        stride = F if mut == 'row_stride_F' else 2 * F
        cs = np.arange(F) + (4 if mut == 'col_plus_4' else 0)
        ia = (GUARD * 2 * F + np.arange(M)[:, None] * stride + cs[None, :])
        a, b = flat[ia], flat[ia + F]
        if mut == 'halves_swapped':
            a, b = b, a
        with np.errstate(invalid='ignore', over='ignore'):
            if mut == 'erf_form':
                from math import erf
                g = (0.5 * a.astype(f64) * (1 + np.vectorize(erf)(a.astype(f64) / math.sqrt(2)))).astype(f32)
            else:
                x3 = ((f32(GELU_A) * a) * a) * a
                inner = a if mut == 'cubic_dropped' else a + x3
                t = np.tanh((f32(GELU_C) * inner).astype(f64)).astype(f32)
                if tanh_ulp:
                    t = np.clip(ulp_shift(t, tanh_ulp, 5 + F), f32(-1), f32(1))
                g = (f32(0.5) * a) * (f32(1) + t)
            o = g * b
        return bf16t(o) if mut == 'truncation' else bf16r(o)

    def not_equal(self, res):
        s = self.sel()
        return not_equal_count(np.asarray(res, f32)[s], self.ref()[s])

    @functools.lru_cache(maxsize=None)
    def share_cap(self):
        """(cap on the share over sel(), the emulation's count: the worst of tanh exact and moved by +-1 and +-2 ulp)"""
        n = max(self.not_equal(self.emul(tanh_ulp=k)) for k in (0, 1, 2))
        return share_cap(n, int(self.sel().sum())), n

    def verdict(self, res):
        """(finite wherever the reference is, worst error over its bound, share over its cap)"""
        ref = self.ref()
        fin = bool(np.isfinite(res)[np.isfinite(ref)].all())
        cap, _ = self.share_cap()
        return fin, worst_ratio(res, ref, self.bound()), self.not_equal(res) / int(self.sel().sum()) / cap

    def applies(self, mut):
        return self.M > 1 or mut != 'row_stride_F'        # row 0 starts at 0 whatever the stride


def gelu_specs():
    return [(M, F) for F in GELU_F for M in GELU_M]


@functools.lru_cache(maxsize=None)
def gelu_case(M, F):
    return GeluCase(M, F)


# --------------------------------------------------------------------------------------------------------------------------------
# GEMM through t5_gemm
# --------------------------------------------------------------------------------------------------------------------------------
GEMM_M = (1, 5, 200)
GEMM_N_CUT = 1088
GEMM_RESID_SCALE = 1e4


def gemm_shapes():
    """(name, N, K, residual) of the four projections of configuration b and of flan-t5-xl, N cut to GEMM_N_CUT"""
    out = []
    for name, D, I, F in (('b', 192, 128, 256), ('xl', 2048, 2048, 5120)):
        for proj, N, K, res in (('qkv', 3 * I, D, False), ('o', D, I, True), ('wi', 2 * F, D, False), ('wff', D, F, True)):
            out.append((f'{name}.{proj}', min(N, GEMM_N_CUT), K, res))
    return out


class GemmCase:
    def __init__(self, name, N, K, resid, M):
        self.name, self.N, self.K, self.M, self.has_resid = name, N, K, M, resid
        rng = np.random.default_rng(K * 3 + N + M)
        self.A = np.full((M + 2 * GUARD, K), NAN, f32)
        self.A[GUARD:GUARD + M] = bf16r(rng.standard_normal((M, K)).astype(f32))
        self.W = bf16r((rng.standard_normal((N, K)) / math.sqrt(K)).astype(f32))
        self.resid = (GEMM_RESID_SCALE * rng.standard_normal((M, N))).astype(f32) if resid else None

    def id(self):
        return f'{self.name}-M{self.M}'

    def ref_and_bound(self):
        a, w = self.A[GUARD:GUARD + self.M].astype(f64), self.W.astype(f64)
        ref, mag = a @ w.T, np.abs(a) @ np.abs(w).T
        if self.resid is not None:
            ref, mag = ref + self.resid.astype(f64), mag + np.abs(self.resid.astype(f64))
        return ref, (self.K + 3) * U24 * mag
