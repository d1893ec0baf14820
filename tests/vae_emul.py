"""Seeded operands, float64 references, gates and numpy emulations for the kernel-level tests of the Oobleck VAE ops (ezvae_gemm with its conv-as-GEMM addressing,
ezvae_snake_bf16, ezvae_conv_out1, ezvae_conv_in1, ezvae_sample).  Test infrastructure, not code under test; the companion of tests/kernel_emul.py.

Every case is built on the CPU with numpy.  Operands are what the kernel sees: bf16-rounded activations and weights (kept as float32 arrays that hold only bf16 values, so
the upload is exact), fp32 bias / residual / w / alpha / inv_beta.  Every operand sits in a flat allocation between NaN guards, every output in a buffer filled with a
sentinel; `excess()` of a case turns an output buffer into ONE number: the worst |got - reference| / bound over the elements the op owns, or infinity when a value is not
finite or the sentinel is touched anywhere else.  A result passes when excess <= 1.  The same function judges the GPU's buffer (tests/test_vae_kernels.py) and the buffers of
the numpy emulations with one deliberate mistake each (`mut`; tests/test_vae.py requires excess >= 3 of every one of them).

Bounds (none comes from the code under test); u = 2^-24, the unit roundoff of fp32:
  GEMM       (n + 3) u (sum_k |a_k w_k| + |bias| + |resid|), n = K: fp32 summation of n exact bf16 products in ANY order is within (n - 1) u (1 + O(n u)) of the sum of
             magnitudes (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2), the two epilogue additions add 2 u, the rest absorbs the O(n u) terms;
             and rel-L2 < 1e-5, the gate of test_gemm_against_fp32_matmul
  conv_out1  (7 C + 1) u sum |x w|   (7 C products, each rounded, and their sum)
  conv_in1   8 u (|b| + sum |x w|)   (bias + 7 fused multiply-adds)
  snake      one bf16 ulp at max(|ref|, 2^-10 rms) (tests/test_gpu.py _assert_bf16_bits) + 2 inv_beta |alpha x| u for the rounding of the fp32 product inside sin
             (d/dt sin^2 t = sin 2t, at most 1 in magnitude); share of elements not bit-equal to bf16(reference) <= SNAKE_SHARE_CAP; alpha NULL: bitwise
  sample     rtol = atol = 1e-5 (test_hip_encoder_ragged_length_and_bottleneck)
"""
import math
import zlib

import numpy as np
import torch

from ezaudio_amd.vae import pack_conv_transpose_weight, pack_conv_weight
from oracle import vae as V

U = 2.0 ** -24
GUARD = 24                    # guard rows around every haloed operand (the furthest a mistaken tap / ceiling reaches is 2 x stride 10 rows)
SENT = np.float32(-12345.5)   # fp32 outputs
SENT_BF16 = np.uint16(0xC2F7) # bf16 outputs (-123.5)
GEMM_REL = 1e-5
SNAKE_SHARE_CAP = 5e-3
INF = float('inf')


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def bf16_bits(x):
    """float32 -> bf16 bit patterns, round to nearest even (integer arithmetic on the bits; inf / NaN pass through)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_val(bits):
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x):
    return bf16_val(bf16_bits(x))


def bf16_ulp(v):
    return np.exp2(np.floor(np.log2(v)) - 7)


def bf16_rne64(v):
    """float64 -> nearest bf16 value (ties to even), without the double rounding of a detour through float32; normal range"""
    v = np.asarray(v, dtype=np.float64)
    ulp = bf16_ulp(np.maximum(np.abs(v), 2.0 ** -126))
    return np.round(v / ulp) * ulp          # numpy rounds halves to even


def _guarded(body, guard):
    g = np.full(guard, np.nan, np.float32)
    return np.concatenate([g, np.ascontiguousarray(body, np.float32).reshape(-1), g])


def _ratio(err, bound):
    if not np.isfinite(err).all():
        return INF
    return float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


# --------------------------------------------------------------------------------------------------------------------------------
# ezvae_gemm
# --------------------------------------------------------------------------------------------------------------------------------
class GemmCase:
    """One ezvae_gemm launch.  a: flat float32 allocation (bf16 values, NaN guards) and a0, the element the A pointer names; w [N][K] (ldw = K, wrows = N);
    bias fp32 [N] or None; r: flat fp32 allocation of the residual (NaN wherever the launch must not read), r0 its pointer element, ldr; ref / bound: float64, in the
    space `readback` maps the owned [M][N] block to (the block itself, or the up-sampled sequence of a transposed convolution)."""

    def __init__(self, name, a, a0, lda, w, bias, M, N, K, cpb=0, tap_elems=0, ldo=None, r=None, r0=0, ldr=0, ref=None, readback=None):
        self.name, self.a, self.a0, self.lda, self.w, self.bias = name, a, a0, lda, np.ascontiguousarray(w, np.float32), bias
        self.M, self.N, self.K, self.cpb, self.tap_elems = M, N, K, cpb, tap_elems
        self.ldo = N if ldo is None else ldo
        self.r, self.r0, self.ldr = r, r0, ldr
        self.ref = ref
        self.readback = readback or (lambda own, shift=0: own)
        assert self.w.shape == (N, K) and K % 64 == 0 and N % 4 == 0 and self.ldo % 4 == 0 and lda % 8 == 0 and a0 % 8 == 0

    @property
    def tap_bytes(self):
        return self.tap_elems * 2

    def resid_block(self):
        if self.r is None:
            return None
        idx = self.r0 + np.arange(self.M)[:, None] * self.ldr + np.arange(self.N)[None, :]
        return self.r[idx]

    def model(self, dtype=np.float64, mut=None, absolute=False):
        """A . W^T over the addressing of k_gemm (csrc/gemm.hip `stage`): K tile t of row m starts at element a0 + m lda + (t // cpb) tap_elems + (t % cpb) 64.
        mut: 'tap_shift+1' every tap one row further, 'tap_reversed' tap order reversed, 'tap_sign' the sign of the tap step flipped."""
        a = self.a.astype(dtype)
        w = self.w.astype(dtype)
        if absolute:
            a, w = np.abs(a), np.abs(w)
        rows = self.a0 + np.arange(self.M, dtype=np.int64) * self.lda
        acc = np.zeros((self.M, self.N), dtype)
        if not self.cpb:
            assert mut is None
            step = 4096
            for k0 in range(0, self.K, step):
                k1 = min(self.K, k0 + step)
                acc += a[rows[:, None] + np.arange(k0, k1)[None, :]] @ w[:, k0:k1].T
            return acc
        tw = self.cpb * 64
        ntap = -(-self.K // tw)
        te = {None: self.tap_elems, 'tap_reversed': self.tap_elems, 'tap_sign': -self.tap_elems,
              'tap_shift+1': self.tap_elems + self.lda}[mut]
        for tap in range(ntap):
            k0, k1 = tap * tw, min(self.K, (tap + 1) * tw)
            src = ntap - 1 - tap if mut == 'tap_reversed' else tap
            idx = rows[:, None] + src * te + np.arange(k1 - k0)[None, :]
            acc += a[idx] @ w[:, k0:k1].T
        return acc

    def full(self, dtype=np.float64, mut=None, absolute=False):
        """the owned [M][N] block: model + bias + resid"""
        out = self.model(dtype, mut, absolute)
        for extra in (None if self.bias is None else self.bias[None, :], self.resid_block()):
            if extra is not None:
                out = out + (np.abs(extra) if absolute else extra).astype(dtype)
        return out

    def prepare(self):
        """float64 reference and bound of the whole block, bound in readback space"""
        self.full_ref = self.full()
        self.full_bound = (self.K + 3) * U * self.full(absolute=True)
        self.bound = self.readback(self.full_bound)
        if self.ref is None:
            self.ref = self.readback(self.full_ref)
        assert self.ref.shape == self.bound.shape, (self.name, self.ref.shape, self.bound.shape)
        return self

    def out_alloc(self):
        return np.full((GUARD + self.M + GUARD, self.ldo), SENT, np.float32)

    def emulate(self, dtype=np.float32, mut=None, like=None):
        """the output buffer a kernel with fp32 accumulation leaves behind (in the allocation of `like`: a mistaken launch may own more rows than the right one)"""
        out = (like or self).out_alloc()
        out[GUARD:GUARD + self.M, :self.N] = self.full(dtype, mut).astype(np.float32)
        return out

    def measure(self, out, shift=0):
        """(excess, rel-L2) of an output buffer; shift: the read-back row offset a mistaken host would use (judges the read-back only)"""
        out = out.reshape(GUARD + self.M + GUARD, self.ldo)
        own = out[GUARD:GUARD + self.M, :self.N].astype(np.float64)
        intact = (out[:GUARD] == SENT).all() and (out[GUARD + self.M:] == SENT).all() and (out[GUARD:GUARD + self.M, self.N:] == SENT).all()
        if not intact or not np.isfinite(own).all():
            return INF, INF
        got = self.readback(own, shift)
        ex = _ratio(np.abs(got - self.ref), self.bound)
        if shift == 0:
            ex = max(ex, _ratio(np.abs(own - self.full_ref), self.full_bound))
        rl = rel_l2(got, self.ref)
        return max(ex, rl / GEMM_REL), rl

    def excess(self, out, shift=0):
        return self.measure(out, shift)[0]


def _act(rng, L, C):
    return bf16_round(rng.standard_normal((L, C)))


def conv_case(C, d, L, Co=None, k=7, bias=True, ldo_pad=0, mut=None):
    """Conv1d(C -> Co, kernel k, dilation d, padding (k // 2) d) as _residual_units / conv_in / the encoder's conv_out launch it: an [L + (k - 1) d][C] haloed buffer,
    cpb = C / 64, tap step d C elements.  mut 'halo_short': the first halo row behind the sequence holds the last valid row where a zero belongs."""
    Co = Co or C
    rng = _rng('conv', C, d, L, Co, k)
    x = _act(rng, L, C)
    w = bf16_round(rng.standard_normal((Co, C, k)) / math.sqrt(k * C))
    b = (0.1 * rng.standard_normal(Co)).astype(np.float32) if bias else None
    h = (k // 2) * d
    buf = np.zeros((L + 2 * h, C), np.float32)
    buf[h:h + L] = x
    if mut == 'halo_short':
        buf[h + L] = x[L - 1]
    W = pack_conv_weight(torch.from_numpy(w)).numpy()
    ref = V.conv1d(x.T[None].astype(np.float64), w.astype(np.float64), None if b is None else b.astype(np.float64), padding=h, dilation=d)[0].T
    return GemmCase(f'conv k{k} C{C}->{Co} d{d} L{L}', _guarded(buf, GUARD * C), GUARD * C, C, W, b, L, Co, k * C, C // 64, d * C, ldo=Co + ldo_pad, ref=ref).prepare()


def convt_case(ci, co, s, L, mut=None):
    """ConvTranspose1d(ci -> co, kernel 2 s, stride s, padding ceil(s / 2)) as the decoder launches it: [0 | x | 0], the A pointer one row in, tap step -ci, M = L + 1,
    N = ldo = s co, the bias repeated s times; read back as [(L + 1) s][co] at row offset ceil(s / 2).  mut 'halo_short' as above, 'bias_once': bias not repeated."""
    rng = _rng('convt', ci, co, s, L)
    x = _act(rng, L, ci)
    wt = bf16_round(rng.standard_normal((ci, co, 2 * s)) / math.sqrt(2 * ci))
    b = (0.1 * rng.standard_normal(co)).astype(np.float32)
    buf = np.zeros((L + 2, ci), np.float32)
    buf[1:1 + L] = x
    if mut == 'halo_short':
        buf[L + 1] = x[L - 1]
    W = pack_conv_transpose_weight(torch.from_numpy(wt), s).numpy()
    brep = np.concatenate([b, np.zeros((s - 1) * co, np.float32)]) if mut == 'bias_once' else np.tile(b, s)
    p = -(-s // 2)
    ref = V.conv_transpose1d(x.T[None].astype(np.float64), wt.astype(np.float64), b.astype(np.float64), stride=s, padding=p)[0].T
    rb = lambda own, shift=0: own.reshape((L + 1) * s, co)[p + shift:p + shift + L * s]
    return GemmCase(f'convT {ci}->{co} s{s} L{L}', _guarded(buf, GUARD * ci), GUARD * ci + ci, ci, W, brep, L + 1, s * co, 2 * ci, ci // 64, -ci, ref=ref, readback=rb).prepare()


def strided_case(C, Co, s, T, mut=None):
    """Conv1d(C -> Co, kernel 2 s, stride s, padding s / 2) as the encoder launches it: a plain GEMM over the [T + s][C] buffer viewed with lda = s C, K = 2 s C,
    Lo = T // s rows.  mut 'ceil': Lo = ceil(T / s)."""
    rng = _rng('strided', C, Co, s, T)
    x = _act(rng, T, C)
    w = bf16_round(rng.standard_normal((Co, C, 2 * s)) / math.sqrt(2 * s * C))
    b = (0.1 * rng.standard_normal(Co)).astype(np.float32)
    p = s // 2
    buf = np.zeros((T + 2 * p, C), np.float32)
    buf[p:p + T] = x
    Lo = -(-T // s) if mut == 'ceil' else T // s
    W = pack_conv_weight(torch.from_numpy(w)).numpy()
    ref = V.conv1d(x.T[None].astype(np.float64), w.astype(np.float64), b.astype(np.float64), stride=s, padding=p)[0].T
    c = GemmCase(f'strided {C}->{Co} s{s} T{T}', _guarded(buf, GUARD * C), GUARD * C, s * C, W, b, Lo, Co, 2 * s * C, ref=ref if mut is None else None)
    return c.prepare() if mut is None else c


def pointwise_case(C, L, mut=None):
    """Conv1d(C -> C, kernel 1) + bias + residual (the second convolution of a ResidualUnit); the residual pointer names column 4 of row GUARD of a wider buffer
    (ldr = C + 8) that is NaN everywhere else, as the decoder passes y + p co."""
    rng = _rng('pointwise', C, L)
    x = _act(rng, L, C)
    w = bf16_round(rng.standard_normal((C, C, 1)) / math.sqrt(C))
    b = (0.1 * rng.standard_normal(C)).astype(np.float32)
    res = rng.standard_normal((L, C)).astype(np.float32)
    ldr = C + 8
    rbuf = np.full((GUARD + L + GUARD, ldr), np.nan, np.float32)
    rbuf[GUARD:GUARD + L, 4:4 + C] = res
    ref = V.conv1d(x.T[None].astype(np.float64), w.astype(np.float64), b.astype(np.float64))[0].T + res.astype(np.float64)
    return GemmCase(f'1x1 C{C} L{L} +resid', _guarded(x, GUARD * C), GUARD * C, C, w[:, :, 0], b, L, C, C, r=rbuf.reshape(-1), r0=GUARD * ldr + 4, ldr=ldr, ref=ref).prepare()


def plain_case(M, N, K, lda_pad=8, ldo_pad=12):
    """bias NULL, ldo > N, lda > K (NaN in the padding columns)"""
    rng = _rng('plain', M, N, K)
    a = np.full((M, K + lda_pad), np.nan, np.float32)
    a[:, :K] = _act(rng, M, K)
    w = bf16_round(rng.standard_normal((N, K)) / math.sqrt(K))
    return GemmCase(f'plain {M}x{N}x{K} no bias', _guarded(a, GUARD * (K + lda_pad)), GUARD * (K + lda_pad), K + lda_pad, w, None, M, N, K, ldo=N + ldo_pad).prepare()


BUILDERS = dict(conv=conv_case, convt=convt_case, strided=strided_case, pointwise=pointwise_case, plain=plain_case)

CONV_L = (1, 5, 127, 128, 129, 1000)          # 5 < 3 d: every row reads the halo
CONVT_PAIRS = ((1024, 512, 10), (512, 256, 6), (256, 128, 4), (128, 128, 2), (64, 64, 4))
CONVT_L = (1, 37, 250)
STRIDED = tuple((64, 128, s) for s in (2, 4, 6, 10)) + ((128, 256, 2),)


def strided_T(s):
    return (2 * s - 1, 4 * s + 3, 1001)      # T // s == 1; a few rows; 1001 is a multiple of none of 2, 4, 6, 10


# family -> [(builder, kwargs)]; every case runs on tile 6
GEMM_FAMILIES = {
    'dilated_k7': [('conv', dict(C=C, d=d, L=L)) for C in (64, 128, 256) for d in (1, 3, 9) for L in CONV_L],
    'decoder_conv_in': [('conv', dict(C=128, d=1, L=L, Co=1024)) for L in (1, 77, 250)],
    'encoder_conv_out_k3': [('conv', dict(C=C, d=1, L=L, Co=Co, k=3)) for C, Co in ((1024, 256), (64, 128)) for L in (1, 9, 250)],
    'transposed': [('convt', dict(ci=ci, co=co, s=s, L=L)) for ci, co, s in CONVT_PAIRS for L in CONVT_L],
    'strided': [('strided', dict(C=C, Co=Co, s=s, T=T)) for C, Co, s in STRIDED for T in strided_T(s)],
    'pointwise_resid': [('pointwise', dict(C=C, L=L)) for C in (64, 256) for L in (1, 129, 1000)],      # C = 64: a single K tile
    'no_bias_ldo': [('plain', dict(M=300, N=192, K=320)), ('plain', dict(M=1, N=64, K=64)), ('conv', dict(C=128, d=3, L=129, bias=False, ldo_pad=20))],
    'last_level': [('conv', dict(C=128, d=9, L=120000))],                                                # 938 M tiles through the XCD tile map
}
# one case per family on tile 25 (ring of 4: the prologue is deeper than the K loop of the 1x1 convolution's single tile and of the k3 / transposed / plain cases below)
GEMM_TILE25 = {
    'dilated_k7': ('conv', dict(C=128, d=3, L=129)),
    'decoder_conv_in': ('conv', dict(C=128, d=1, L=77, Co=1024)),
    'encoder_conv_out_k3': ('conv', dict(C=64, d=1, L=9, Co=128, k=3)),
    'transposed': ('convt', dict(ci=64, co=64, s=4, L=37)),
    'strided': ('strided', dict(C=64, Co=128, s=6, T=27)),
    'pointwise_resid': ('pointwise', dict(C=64, L=129)),
    'no_bias_ldo': ('plain', dict(M=300, N=192, K=320)),
    'last_level': ('conv', dict(C=128, d=9, L=120000)),
}


def build(spec, mut=None):
    name, kw = spec
    return BUILDERS[name](**kw) if mut is None else BUILDERS[name](mut=mut, **kw)


# --------------------------------------------------------------------------------------------------------------------------------
# ezvae_snake_bf16
# --------------------------------------------------------------------------------------------------------------------------------
SNAKE_SHAPES = [(C, L) for C in (64, 128, 1024) for L in (1, 3, 1000)]    # L C / 4 is not a multiple of the 256-thread block at C = 64 (16, 48, 16000) and C = 128, L <= 3
SNAKE_HALO = 3
# exact ties (to even: down, up), one bit either side of a tie, round up into the next binade, +-0, the largest magnitudes that stay finite, the smallest normal numbers,
# ties and exact values among the fp32 denormals
CAST_SPECIALS = np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F7FFFFF, 0x3FFFFFFF, 0xBF808000, 0xBF818000, 0xBF7FFFFF, 0x00000000, 0x80000000,
                          0x7F7F7FFF, 0xFF7F7FFF, 0x7F7F0000, 0x7E808000, 0x00800000, 0x00808000, 0x80818000, 0x00010000, 0x00008000, 0x00018000, 0x80018000,
                          0x00007FFF, 0x3F800000, 0x40490FDB], dtype=np.uint32)


class SnakeCase:
    """x fp32 [L][ldx] (ldx = C + 4) between NaN guard rows, NaN in the padding columns; out bf16 [halo + L + halo][ldo] (ldo = C + 8) between guard rows, all sentinel:
    the op owns rows [halo, halo + L) x columns [0, C)."""

    def __init__(self, C, L, params):
        rng = _rng('snake', C, L, params)
        self.C, self.L, self.ldx, self.ldo, self.params = C, L, C + 4, C + 8, params
        if params:
            x = rng.uniform(-3, 3, (L, C)).astype(np.float32)
            self.alpha = np.exp(rng.uniform(math.log(0.3), math.log(100.0), C)).astype(np.float32)
            self.alpha[0] = 100.0                                            # |alpha x| up to 300: sinf's range reduction
            self.beta = np.exp(rng.uniform(-1, 1, C)).astype(np.float32)
            self.inv_beta = (1.0 / (self.beta.astype(np.float64) + 1e-9)).astype(np.float32)
        else:
            x = (rng.standard_normal((L, C)) * 10.0 ** rng.uniform(-30, 30, (L, C))).astype(np.float32)
            flat = x.reshape(-1)
            pos = np.arange(len(CAST_SPECIALS)) * 2 % flat.size
            flat[pos] = CAST_SPECIALS.view(np.float32)
            self.alpha = self.beta = self.inv_beta = None
        self.x = x
        xa = np.full((GUARD + L + GUARD, self.ldx), np.nan, np.float32)
        xa[GUARD:GUARD + L, :C] = x
        self.x_alloc, self.x0 = xa, GUARD * self.ldx
        self.rows = GUARD + SNAKE_HALO + L + SNAKE_HALO + GUARD
        self.out0 = (GUARD + SNAKE_HALO) * self.ldo
        if params:
            x64 = x.astype(np.float64)
            ax = self.alpha.astype(np.float64) * x64
            self.ref = x64 + self.inv_beta.astype(np.float64) * np.sin(ax) ** 2
            self.want = bf16_rne64(self.ref)
            floor = math.sqrt(float((self.ref ** 2).mean())) * 2.0 ** -10
            self.bound = bf16_ulp(np.maximum(np.abs(self.ref), floor)) + 2 * self.inv_beta.astype(np.float64) * np.abs(ax) * U

    def out_alloc(self):
        return np.full((self.rows, self.ldo), SENT_BF16, np.uint16)

    def emulate(self, mut=None):
        """the formula in numpy float32.  mut: 'sin_not_squared', 'beta_not_inverted'"""
        out = self.out_alloc()
        r = self.x
        if self.params:
            s = np.sin(self.x * self.alpha)
            if mut == 'sin_not_squared':
                r = self.x + self.inv_beta * s
            elif mut == 'beta_not_inverted':
                r = self.x + self.beta * s * s
            else:
                r = self.x + self.inv_beta * s * s
        o = GUARD + SNAKE_HALO
        out[o:o + self.L, :self.C] = bf16_bits(r.astype(np.float32))
        return out

    def measure(self, out):
        """(excess, share of elements not bit-equal to bf16(reference)); the cast is bitwise: any differing element is infinity"""
        out = out.reshape(self.rows, self.ldo)
        o = GUARD + SNAKE_HALO
        own = out[o:o + self.L, :self.C]
        if not ((out[:o] == SENT_BF16).all() and (out[o + self.L:] == SENT_BF16).all() and (out[o:o + self.L, self.C:] == SENT_BF16).all()):
            return INF, 1.0
        if not self.params:
            bad = own != bf16_bits(self.x)
            return (INF if bad.any() else 0.0), float(bad.mean())
        got = bf16_val(own).astype(np.float64)
        share = float((got != self.want).mean())
        ex = _ratio(np.abs(got - self.want), self.bound)
        return max(ex, share / SNAKE_SHARE_CAP), share


# --------------------------------------------------------------------------------------------------------------------------------
# ezvae_conv_out1 / ezvae_conv_in1
# --------------------------------------------------------------------------------------------------------------------------------
CONV_OUT1 = [(C, L) for C in (64, 128) for L in (1, 255, 256, 257, 120000)]
CONV_IN1 = [(C, T) for C in (64, 128) for T in (1, 2, 3, 6, 7, 1000)]
VGUARD = 64     # guard elements around the fp32 vectors (wav, the final waveform)


class ConvOut1Case:
    """xb bf16 [3 zero rows | L | 3 zero rows][ldx] (ldx = C + 8, NaN padding columns) between NaN guard rows; w fp32 [7][C]; out fp32 [L] between sentinel guards."""

    def __init__(self, C, L):
        rng = _rng('conv_out1', C, L)
        self.C, self.L, self.ldx = C, L, C + 8
        self.x = _act(rng, L, C)
        self.w = (rng.standard_normal((7, C)) / math.sqrt(7 * C)).astype(np.float32)
        xa = np.full((GUARD + L + 6 + GUARD, self.ldx), np.nan, np.float32)
        xa[GUARD:GUARD + L + 6, :C] = 0
        xa[GUARD + 3:GUARD + 3 + L, :C] = self.x
        self.x_alloc, self.x0 = xa, GUARD * self.ldx
        self.ref = self._run(np.float64)
        self.bound = (7 * C + 1) * U * self._run(np.float64, absolute=True)

    def _run(self, dtype, mut=None, absolute=False):
        """mut: 'clamp' rows outside the sequence repeat the nearest valid row, 'tap_reversed', 'tap_shift+1'"""
        xa, w = self.x_alloc.astype(dtype), self.w.astype(dtype)
        if absolute:
            xa, w = np.abs(xa), np.abs(w)
        acc = np.zeros(self.L, dtype)
        l = np.arange(self.L)
        for k in range(7):
            rows = GUARD + l + k + (1 if mut == 'tap_shift+1' else 0)
            if mut == 'clamp':
                rows = GUARD + 3 + np.clip(l + k - 3, 0, self.L - 1)
            acc += xa[rows, :self.C] @ w[6 - k if mut == 'tap_reversed' else k]
        return acc

    def out_alloc(self):
        return np.full(VGUARD + self.L + VGUARD, SENT, np.float32)

    def emulate(self, mut=None):
        out = self.out_alloc()
        out[VGUARD:VGUARD + self.L] = self._run(np.float32, mut)
        return out

    def excess(self, out):
        own = out[VGUARD:VGUARD + self.L].astype(np.float64)
        if not ((out[:VGUARD] == SENT).all() and (out[VGUARD + self.L:] == SENT).all()):
            return INF
        return _ratio(np.abs(own - self.ref), self.bound)


class ConvIn1Case:
    """wav fp32 [T] between NaN guards (the kernel zero-pads by index, never by reading); w fp32 [7][C]; bias [C]; out fp32 [T][C] between sentinel guard rows.
    zero_guards: the variant whose guards are zeros, which a kernel that pads by reading would pass."""

    def __init__(self, C, T, zero_guards=False):
        rng = _rng('conv_in1', C, T)
        self.C, self.T = C, T
        self.wav = (0.5 * rng.standard_normal(T)).astype(np.float32)
        self.w = (rng.standard_normal((7, C)) / math.sqrt(7.0)).astype(np.float32)
        self.b = (0.1 * rng.standard_normal(C)).astype(np.float32)
        self.wav_alloc = np.concatenate([np.full(VGUARD, 0.0 if zero_guards else np.nan, np.float32), self.wav, np.full(VGUARD, 0.0 if zero_guards else np.nan, np.float32)])
        self.ref = self._run(np.float64)
        self.bound = 8 * U * self._run(np.float64, absolute=True)

    def _run(self, dtype, mut=None, absolute=False):
        """mut: 'clamp' samples outside the waveform repeat the nearest one, 'pad_by_reading' they are whatever lies there, 'tap_reversed'"""
        f = np.abs if absolute else (lambda v: v)
        w, b = f(self.w.astype(dtype)), f(self.b.astype(dtype))
        t = np.arange(self.T)
        acc = np.tile(b, (self.T, 1))
        for k in range(7):
            j = t + k - 3
            if mut == 'clamp':
                xs = self.wav[np.clip(j, 0, self.T - 1)]
            elif mut == 'pad_by_reading':
                xs = self.wav_alloc[VGUARD + j]
            else:
                xs = np.where((j >= 0) & (j < self.T), self.wav[np.clip(j, 0, self.T - 1)], np.float32(0))
            acc = acc + f(xs.astype(dtype))[:, None] * w[6 - k if mut == 'tap_reversed' else k][None, :]
        return acc

    def out_alloc(self):
        return np.full((GUARD + self.T + GUARD, self.C), SENT, np.float32)

    def emulate(self, mut=None):
        out = self.out_alloc()
        out[GUARD:GUARD + self.T] = self._run(np.float32, mut)
        return out

    def excess(self, out):
        out = out.reshape(GUARD + self.T + GUARD, self.C)
        own = out[GUARD:GUARD + self.T].astype(np.float64)
        if not ((out[:GUARD] == SENT).all() and (out[GUARD + self.T:] == SENT).all()):
            return INF
        return _ratio(np.abs(own - self.ref), self.bound)


# --------------------------------------------------------------------------------------------------------------------------------
# ezvae_sample
# --------------------------------------------------------------------------------------------------------------------------------
SAMPLE_SHAPES = [(128, 77), (64, 1), (128, 250), (64, 333)]     # (latent, L), L != latent; 128 x 77 and 64 x 1 are not multiples of the 256-thread block
SAMPLE_SQUARE = (64, 64)                                        # the shape at which swapped indices cannot be seen (tests/test_vae.py shows it)
SCALE_SPECIALS = np.array([-100.0, -88.0, -60.0, -20.0, -1e-3, 0.0, 1e-3, 19.9, 20.0, 20.1, 88.0, 100.0], np.float32)
SAMPLE_TOL = 1e-5


class SampleCase:
    """enc fp32 [L][2 lat] (mean | scale) between NaN guard rows; noise fp32 [lat][L] or None; z fp32 [lat][L] between sentinel guards."""

    def __init__(self, lat, L, with_noise=True):
        rng = _rng('sample', lat, L)
        self.lat, self.L = lat, L
        mean = rng.standard_normal((L, lat)).astype(np.float32)
        scale = np.where(rng.random((L, lat)) < 0.5, rng.uniform(-3, 3, (L, lat)), rng.uniform(-100, 100, (L, lat))).astype(np.float32)
        flat = scale.reshape(-1)
        flat[np.arange(len(SCALE_SPECIALS)) * 5 % flat.size] = SCALE_SPECIALS
        self.enc = np.concatenate([mean, scale], axis=1)
        self.noise = rng.standard_normal((lat, L)).astype(np.float32) if with_noise else None
        ea = np.full((GUARD + L + GUARD, 2 * lat), np.nan, np.float32)
        ea[GUARD:GUARD + L] = self.enc
        self.enc_alloc, self.enc0 = ea, GUARD * 2 * lat
        m64, s64 = mean.T.astype(np.float64), scale.T.astype(np.float64)
        n64 = self.noise.astype(np.float64) if with_noise else np.zeros((lat, L))
        self.ref = n64 * (np.logaddexp(0.0, s64) + 1e-4) + m64
        self.bound = SAMPLE_TOL + SAMPLE_TOL * np.abs(self.ref)

    def out_alloc(self):
        return np.full(VGUARD + self.lat * self.L + VGUARD, SENT, np.float32)

    def emulate(self, mut=None):
        """k_vae_sample in numpy float32.  mut: 'halves_swapped' mean and scale, 'index_swapped' idx split by lat where L belongs (rows of enc that do not exist read
        as the NaN behind it), 'no_threshold' softplus without its branch at 20"""
        lat, L = self.lat, self.L
        idx = np.arange(lat * L)
        c, l = np.divmod(idx, lat if mut == 'index_swapped' else L)
        encp = np.concatenate([self.enc, np.full((max(lat, L), 2 * lat), np.nan, np.float32)])
        c = np.minimum(c, lat - 1)
        mean, sc = encp[l, c], encp[l, lat + c]
        if mut == 'halves_swapped':
            mean, sc = sc, mean
        with np.errstate(over='ignore', invalid='ignore'):
            soft = np.log1p(np.exp(sc))
            if mut != 'no_threshold':
                soft = np.where(sc > np.float32(20), sc, soft)
            n = self.noise.reshape(-1) if self.noise is not None else np.zeros(lat * L, np.float32)
            z = (n * (soft + np.float32(1e-4)) + mean).astype(np.float32)
        out = self.out_alloc()
        out[VGUARD:VGUARD + lat * L] = z
        return out

    def excess(self, out):
        own = out[VGUARD:VGUARD + self.lat * self.L].astype(np.float64).reshape(self.lat, self.L)
        if not ((out[:VGUARD] == SENT).all() and (out[VGUARD + self.lat * self.L:] == SENT).all()):
            return INF
        return _ratio(np.abs(own - self.ref), self.bound)
