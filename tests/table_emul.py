"""Seeded fixtures, fp64 references, fp32 emulations and deliberate mistakes for the kernel-level tests of the once-per-call tables: the time path and the AdaLN-SOLA
modulation (k_linear_f32, k_mod_finalize), the LayerNorm-algebra tables G' = g W^T, C' = c W^T + b (k_z_hilo, the table GEMM, k_z_combine), the constant single-key
cross-attention vector zd (k_gemv_bf16w) and the bf16 casts of the context path (k_cast_bf16), all of csrc/rowops.hip as ezdit_prepare_timesteps / ezdit_prepare_context
(csrc/api.hip) launch them.  Test infrastructure, not code under test; same shape as tests/row_emul.py.  numpy throughout, as the oracle is.

Fixtures: the synthetic checkpoints of oracle/weights.py (seed 1) at xs (D 144: a lane tail in the K loop, ld padding) and xs64 (D 128), depth 2 (in, mid and out block: every
per-block stride is crossed), xs with ada_sola_alpha = 6 (scaling 1.5, exact in fp32; alpha == rank everywhere else, where no test can tell whether the scaling is applied)
and the ControlNet handle at xs (one block, no final block).

References (fp64): oracle.dit.DiTOracle(dtype=float64).time_path and .adaln; `fold` restates k_mod_finalize's fold of the six chunks (shift_msa, scale_msa, gate_msa,
shift_mlp, scale_mlp, gate_mlp) with the LayerNorm affine: per (slot, block)  g1 = n1w (1 + scale_msa), c1 = n1b (1 + scale_msa) + shift_msa, 1 - gate_msa, the same three
of norm3 / *_mlp; per slot for the final block  nfw (1 + scale), nfb (1 + scale) + shift.  The embedding's arguments t f_k stay fp32 by definition (the oracle and the
reference build them so).  G' / C': the exact fp64 product of the fp32 gain / shift vectors with the bf16-rounded weight in the PACKED column order
(ezaudio_amd.weights._qkrope / _geglu8 applied to the state dict, never the blob); slot layouts are those of ezdit_handle::ztab, [slot][item][G' | C'][N].

Emulations (fp32): the time path in the kernel's order -- 64 lane-strided partial sums of fused multiply-adds, then the xor butterfly of wave_sum -- with numpy's expf / sinf /
cosf.  The device's expf is specified to an ulp, not to numpy's bits: the chain is evaluated three times, with the frequencies as numpy gives them and with every frequency
(but f_0 = exp(0) = 1) moved by a seeded +-1 and +-2 ulp; floors are the worst of the three, per timestep.  G' / C': hi + lo bf16 split, fp32 accumulation.

Gates.  Derived, or measured on the emulation (tests/test_call_tables_host.py asserts every relation on the CPU), never on the kernel:
  chain from the timesteps   rel-L2 per (timestep, table) of tt, ada, adaf, mod, modf against the fp64 oracle <= CHAIN_FACTOR = 2 x the emulated floor of that timestep.  The
                             factor covers the device's own expf / sinf / cosf and contraction.  The floors are computed from the emulation for the timesteps of the call
                             (`floors`); FLOORS_A records them for the slots of case (a), and the host test holds the emulation to the record.
  isolated launches (inputs read back from the device, one kernel under test; elementwise, nothing measured):
    k_linear_f32             |got - ref64| <= 2 (K + 2) 2^-24 (sum |x| |W| + |b|); with SiLU that bound x 1.1 + 8 2^-24 |ref|              (lin_bound)
    k_mod_finalize           4 2^-24 sum |terms| per output, from the read-back ada, lora, adaf                                           (fold_bound)
    G' / C'                  (2^-17 + (K + 2) 2^-24) (sum |v| |W| + |bias|), K = D (2 D for the skip table), from the read-back mod         (zt_ref_bound)
                             emulated worst 1.3e-6 of that sum against a bound of 1.6e-5 at K = 144; drop_lo sits at 6.5e-4 ... 8.1e-4
    zd                       2 (K + 2) 2^-24 (sum |v| |W| + |b|), v the bf16 value row read back from vc                                    (lin_bound)
    casts                    within one bf16 ulp of silu64 / the identity of the read-back fp32; pad columns exactly zero
"""
import functools

import numpy as np
import torch

from oracle.controlnet import CN_DEFAULT, ControlNetOracle, make_controlnet_state_dict
from oracle.dit import DiTOracle, layer_norm
from oracle.weights import block_prefixes, make_inputs, make_state_dict, model_config

U24, U17 = 2.0 ** -24, 2.0 ** -17
LIN_SC, GEMV_MAXB, Z_TILE_ROWS = 4, 32, 128      # csrc/rowops.hip, csrc/common.h, the 128-row tile of the table GEMM
SEED_W = 1
SLOTS_A = (999, 979, 499, 19, 1, 0)              # n = 6 leaves a partial chunk of LIN_SC
CHAIN_FACTOR = 2.0
CHAIN_TABLES = ('tt', 'ada', 'adaf', 'mod', 'modf')
MUT_FACTOR = 10.0                                # every mistake lies at least this many gates (hard bounds) from the reference

# emulated floors of the chain for SLOTS_A: rel-L2 per (timestep, table) against the fp64 oracle, worst of the three evaluations (frequencies exact, +-1 ulp, +-2 ulp).
# The gate is CHAIN_FACTOR x these.  The values measured on MI355X are in DESIGN.md section 2 ("Kernel-level tests of the once-per-call tables").
# fixture -> table -> six floats in the order of SLOTS_A
FLOORS_A = {
    'xs': {'tt': (3.44e-05, 4.10e-05, 1.84e-05, 8.46e-07, 1.51e-07, 1.31e-07), 'ada': (3.31e-05, 3.75e-05, 1.66e-05, 7.96e-07, 1.55e-07, 1.38e-07), 'adaf': (3.50e-05, 4.16e-05, 1.73e-05, 7.88e-07, 1.63e-07, 1.48e-07), 'mod': (2.91e-06, 3.15e-06, 1.49e-06, 8.05e-08, 3.66e-08, 3.59e-08), 'modf': (2.96e-06, 3.34e-06, 1.44e-06, 8.12e-08, 4.18e-08, 4.11e-08)},
    'xs64': {'tt': (2.52e-05, 3.56e-05, 1.63e-05, 6.55e-07, 1.51e-07, 1.36e-07), 'ada': (2.64e-05, 3.50e-05, 1.61e-05, 6.41e-07, 1.60e-07, 1.45e-07), 'adaf': (2.47e-05, 3.58e-05, 1.39e-05, 5.86e-07, 1.46e-07, 1.50e-07), 'mod': (2.78e-06, 3.34e-06, 1.32e-06, 6.77e-08, 3.49e-08, 3.46e-08), 'modf': (2.79e-06, 3.56e-06, 1.20e-06, 7.11e-08, 4.18e-08, 3.53e-08)},
    'xs_a6': {'tt': (3.44e-05, 4.10e-05, 1.84e-05, 8.46e-07, 1.51e-07, 1.31e-07), 'ada': (3.31e-05, 3.75e-05, 1.66e-05, 7.96e-07, 1.55e-07, 1.38e-07), 'adaf': (3.50e-05, 4.16e-05, 1.73e-05, 7.88e-07, 1.63e-07, 1.48e-07), 'mod': (3.35e-06, 3.65e-06, 1.72e-06, 8.75e-08, 3.57e-08, 3.65e-08), 'modf': (2.96e-06, 3.34e-06, 1.44e-06, 8.12e-08, 4.18e-08, 4.11e-08)},
    'cn_xs': {'tt': (4.33e-05, 3.10e-05, 1.88e-05, 8.77e-07, 1.54e-07, 1.56e-07), 'ada': (4.07e-05, 2.83e-05, 1.83e-05, 8.32e-07, 1.69e-07, 1.70e-07), 'mod': (3.91e-06, 3.06e-06, 1.76e-06, 7.66e-08, 3.73e-08, 3.71e-08)},
}

TIME_MUTANTS = ('sin_cos_swapped', 'freq_over_half_minus_1', 'no_time_act', 'silu_on_ada', 'neighbour_slot', 'chunk_tail_lost')
MOD_MUTANTS = ('lora_unscaled', 'lora_of_neighbour_block', 'table_of_neighbour_block', 'gate_not_one_minus', 'shift_scale_swapped', 'norm3_with_norm1_affine',
               'affine_bias_not_modulated', 'final_shift_scale_swapped')
ZT_MUTANTS = ('drop_lo', 'c_without_bias', 'g_c_swapped', 'slot_stride_of_one_block', 'natural_order_columns', 'rows_past_128_lost')
ZD_MUTANTS = ('v_not_rounded', 'key_0', 'k_half_for_v_half', 'bias_missing', 'w_of_neighbour_block')

f32, f64 = np.float32, np.float64


def bf16r(x):
    """fp32 -> the nearest bf16 value (ties to even), as fp32"""
    u = np.ascontiguousarray(x, dtype=f32).view(np.uint32)
    r = ((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
    return ((u + r) & np.uint32(0xFFFF0000)).view(f32)


def rel_rows(got, ref):
    """rel-L2 per leading index (slot): everything behind the first axis is one vector"""
    g, r = np.asarray(got, f64).reshape(len(got), -1), np.asarray(ref, f64).reshape(len(ref), -1)
    d = np.linalg.norm(g - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-300)
    return np.where(np.isfinite(d), d, np.inf)


def worst_ratio(got, ref, bound):
    """largest |got - ref| / bound; NaN / inf in `got` count as infinite"""
    e = np.abs(np.asarray(got, f64) - ref) / bound
    return float(np.where(np.isfinite(e), e, np.inf).max())


# --------------------------------------------------------------------------------------------------------------------------------
# fixtures
# --------------------------------------------------------------------------------------------------------------------------------
class Fixture:
    def __init__(self, name):
        self.name = name
        self.is_cn = name.startswith('cn_')
        size = name.split('_')[1] if self.is_cn else name.split('_')[0]
        self.cfg = dict(model_config(size))
        if name.endswith('_a6'):
            self.cfg['ada_sola_alpha'] = 6
        if self.is_cn:
            self.sd = make_controlnet_state_dict(self.cfg, CN_DEFAULT, SEED_W)
            self.prefix = ''
            self.blocks = [f'in_blocks.{i}' for i in range(self.cfg['depth'] // 2)]
        else:
            self.sd = make_state_dict(self.cfg, SEED_W)
            self.prefix = 'model.'
            self.blocks = block_prefixes(self.cfg)
        self.D = self.cfg['embed_dim']
        self.I = int(self.D * self.cfg['mlp_ratio'])
        self.dh = self.D // self.cfg['num_heads']
        self.nblk, self.nhalf = len(self.blocks), self.cfg['depth'] // 2
        self.r6 = 6 * self.cfg['ada_sola_rank']
        self.scaling = self.cfg['ada_sola_alpha'] / self.cfg['ada_sola_rank']
        self.has_final = not self.is_cn

    def oracle(self, dtype):
        if self.is_cn:
            return ControlNetOracle(self.cfg, self.sd, dtype=dtype)
        return DiTOracle(self.cfg, self.sd, dtype=dtype)

    @functools.cached_property
    def o64(self):
        return self.oracle(f64)

    def p(self, key):
        return self.sd[key]

    def blk(self, b, key):
        return self.sd[f'{self.blocks[b]}.{key}']

    def stack(self, key):
        return np.stack([self.blk(b, key) for b in range(self.nblk)])


FIXTURES = ('xs', 'xs64', 'xs_a6', 'cn_xs')


@functools.lru_cache(maxsize=None)
def fixture(name):
    return Fixture(name)


# --------------------------------------------------------------------------------------------------------------------------------
# the fold of k_mod_finalize, in any dtype
# --------------------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c, dtype):
    """a b + c with one rounding in fp32 (the product of two fp32 values is exact in fp64); plain arithmetic in fp64"""
    if dtype == f64:
        return a * b + c
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def six_of(fx, ada, lora, dtype, mut=None):
    """ada [n][6 D], lora [n][nblk][6 D] (unscaled, as the kernel stores it) -> the six modulation vectors [n][nblk][6][D]"""
    n = ada.shape[0]
    nb = fx.nblk
    lo = lora.astype(dtype)
    if mut == 'lora_of_neighbour_block':
        lo = np.roll(lo, -1, axis=1)
    tab = fx.stack('adaln.scale_shift_table').reshape(nb, -1).astype(dtype)
    if mut == 'table_of_neighbour_block':
        tab = np.roll(tab, -1, axis=0)
    sc = dtype(1.0 if mut == 'lora_unscaled' else fx.scaling)
    six = _fma(np.broadcast_to(np.asarray(sc, dtype), lo.shape), lo, np.broadcast_to(ada.astype(dtype)[:, None], lo.shape), dtype) + tab[None]
    return six.reshape(n, nb, 6, fx.D)


def fold(fx, six, dtype, mut=None):
    """[n][nblk][6][D] six -> mod [n][nblk][6][D]: (g1, c1, 1 - gate_msa, g3, c3, 1 - gate_mlp)"""
    w1, b1 = fx.stack('norm1.weight').astype(dtype)[None], fx.stack('norm1.bias').astype(dtype)[None]
    w3, b3 = fx.stack('norm3.weight').astype(dtype)[None], fx.stack('norm3.bias').astype(dtype)[None]
    if mut == 'norm3_with_norm1_affine':
        w3, b3 = w1, b1
    s = [six[:, :, i] for i in range(6)]
    if mut == 'shift_scale_swapped':
        s[0], s[1], s[3], s[4] = s[1], s[0], s[4], s[3]
    one = dtype(1.0)
    out = np.empty_like(six)
    for o, (w, b, sh, scl, gt) in ((0, (w1, b1, s[0], s[1], s[2])), (3, (w3, b3, s[3], s[4], s[5]))):
        k = one + scl
        out[:, :, o] = w * k
        out[:, :, o + 1] = b + sh if mut == 'affine_bias_not_modulated' else _fma(np.broadcast_to(b, k.shape), k, sh, dtype)
        out[:, :, o + 2] = gt if mut == 'gate_not_one_minus' else one - gt
    return out


def fold_final(fx, adaf, dtype, mut=None):
    """adaf [n][2 D] (shift first) -> modf [n][2][D]"""
    D = fx.D
    nw, nb = fx.p(fx.prefix + 'final_block.norm.weight').astype(dtype), fx.p(fx.prefix + 'final_block.norm.bias').astype(dtype)
    shift, scale = adaf[:, :D].astype(dtype), adaf[:, D:].astype(dtype)
    if mut == 'final_shift_scale_swapped':
        shift, scale = scale, shift
    k = dtype(1.0) + scale
    return np.stack([nw[None] * k, _fma(np.broadcast_to(nb[None], k.shape), k, shift, dtype)], 1)


def fold_bound(fx, ada, lora, adaf=None):
    """4 2^-24 sum |terms| per output of k_mod_finalize, from its (read-back) inputs: (mod bound [n][nblk][6][D], modf bound [n][2][D] or None)"""
    n, nb, D = ada.shape[0], fx.nblk, fx.D
    tab = np.abs(fx.stack('adaln.scale_shift_table').reshape(nb, -1).astype(f64))
    S = (np.abs(ada.astype(f64))[:, None] + abs(fx.scaling) * np.abs(lora.astype(f64)) + tab[None]).reshape(n, nb, 6, D)
    out = np.empty((n, nb, 6, D))
    for o, nm in ((0, 'norm1'), (3, 'norm3')):
        w, b = np.abs(fx.stack(nm + '.weight').astype(f64))[None], np.abs(fx.stack(nm + '.bias').astype(f64))[None]
        out[:, :, o] = w * (1 + S[:, :, o + 1])
        out[:, :, o + 1] = b * (1 + S[:, :, o + 1]) + S[:, :, o]
        out[:, :, o + 2] = 1 + S[:, :, o + 2]
    bf = None
    if adaf is not None:
        nw, nbb = np.abs(fx.p(fx.prefix + 'final_block.norm.weight').astype(f64)), np.abs(fx.p(fx.prefix + 'final_block.norm.bias').astype(f64))
        sh, sc = np.abs(adaf[:, :D].astype(f64)), np.abs(adaf[:, D:].astype(f64))
        bf = 4 * U24 * np.stack([nw[None] * (1 + sc), nbb[None] * (1 + sc) + sh], 1)
    return 4 * U24 * out, bf


# --------------------------------------------------------------------------------------------------------------------------------
# references in fp64
# --------------------------------------------------------------------------------------------------------------------------------
def ref_chain(fx, ts):
    """dict of the fp64 tables of the timesteps `ts`: tt [n][D], ada [n][6 D], adaf [n][2 D] (backbone), lora [n][nblk][6 D] (unscaled), mod [n][nblk][6][D], modf [n][2][D]"""
    o = fx.o64
    ts = np.asarray(ts)
    tt, ada, adaf = o.time_path(ts, len(ts))
    six = np.stack([o.adaln(p, tt, ada) for p in fx.blocks], 1)          # [n][nblk][6][D]
    out = dict(tt=tt, ada=ada, mod=fold(fx, six, f64))
    out['lora'] = np.stack([(tt @ o.p(p + '.adaln.lora_a.weight').T) @ o.p(p + '.adaln.lora_b.weight').T for p in fx.blocks], 1)
    if fx.has_final:
        out['adaf'] = adaf
        out['modf'] = fold_final(fx, adaf, f64)
    return out


def lin_ref(x, W, b=None, act=False):
    y = np.asarray(x, f64) @ np.asarray(W, f64).T
    if b is not None:
        y = y + np.asarray(b, f64)
    return y / (1 + np.exp(-y)) if act else y


def lin_bound(x, W, b=None, act=False, ref=None):
    """2 (K + 2) 2^-24 (sum |x| |W| + |b|); with SiLU that bound x 1.1 + 8 2^-24 |ref|"""
    K = np.shape(W)[1]
    s = np.abs(np.asarray(x, f64)) @ np.abs(np.asarray(W, f64)).T
    if b is not None:
        s = s + np.abs(np.asarray(b, f64))
    bound = 2 * (K + 2) * U24 * s
    return 1.1 * bound + 8 * U24 * np.abs(ref) if act else bound


# --------------------------------------------------------------------------------------------------------------------------------
# the time path and the modulation in fp32, in the kernel's order
# --------------------------------------------------------------------------------------------------------------------------------
_XOR = [np.arange(64) ^ o for o in (32, 16, 8, 4, 2, 1)]


def lin_emul(x, W, b=None, act=False):
    """k_linear_f32 / k_gemv_bf16w: lane l sums k = l, l + 64, ... with fused multiply-adds, wave_sum's butterfly adds the 64 partial sums, then the bias and SiLU"""
    x, W = np.asarray(x, f32), np.asarray(W, f32)
    n, K = x.shape
    acc = np.zeros((n, W.shape[0], 64), f32)
    for k0 in range(0, K, 64):
        m = min(64, K - k0)
        acc[..., :m] = (acc[..., :m].astype(f64) + x[:, None, k0:k0 + m].astype(f64) * W[None, :, k0:k0 + m].astype(f64)).astype(f32)
    for idx in _XOR:
        acc = acc + acc[..., idx]
    y = acc[..., 0]
    if b is not None:
        y = y + np.asarray(b, f32)[None]
    if act:
        y = y / (f32(1) + np.exp(-y))
    return y.astype(f32)


def embed_emul(ts, freq_ulp=0, mut=None):
    """timestep_embedding(t, 256) as k_linear_f32 forms it: [cos(t f) | sin(t f)], f_k = expf(-ln(1e4) k / 128), everything fp32"""
    half = 128
    k = np.arange(half, dtype=f32)
    den = f32(half - 1 if mut == 'freq_over_half_minus_1' else half)
    f = np.exp(f32(-9.210340371976184) * k / den).astype(f32)
    if freq_ulp:
        sign = np.random.default_rng(4100 + freq_ulp).choice(np.array([-1, 1], np.int32), half)
        sign[0] = 0                                              # exp(0) is 1 in every implementation
        f = (f.view(np.int32) + sign * np.int32(freq_ulp)).view(f32)
    arg = np.asarray(ts, f32)[:, None] * f[None]
    c, s = np.cos(arg), np.sin(arg)
    if mut == 'sin_cos_swapped':
        c, s = s, c
    return np.concatenate([c, s], 1).astype(f32)


def emul_chain(fx, ts, freq_ulp=0, mut=None):
    """the tables of ezdit_prepare_timesteps in fp32, kernel order: dict t1, tt, ada, adaf, lora, mod, modf (as ref_chain).  `mut`: one of TIME_MUTANTS / MOD_MUTANTS"""
    m = fx.prefix
    ts = np.asarray(ts)
    n = len(ts)
    if mut == 'neighbour_slot':
        ts = np.roll(ts, -1)
    tm = mut if mut in TIME_MUTANTS else None
    e = embed_emul(ts, freq_ulp, tm)
    t1 = lin_emul(e, fx.p(m + 'time_embed.mlp.0.weight'), fx.p(m + 'time_embed.mlp.0.bias'), act=True)
    tt = lin_emul(t1, fx.p(m + 'time_embed.mlp.2.weight'), fx.p(m + 'time_embed.mlp.2.bias'), act=mut != 'no_time_act')
    ada = lin_emul(tt, fx.p(m + 'time_ada.weight'), fx.p(m + 'time_ada.bias'), act=mut == 'silu_on_ada')
    lora = np.stack([lin_emul(lin_emul(tt, fx.blk(b, 'adaln.lora_a.weight')), fx.blk(b, 'adaln.lora_b.weight')) for b in range(fx.nblk)], 1)
    out = dict(t1=t1, tt=tt, ada=ada, lora=lora)
    if fx.has_final:
        out['adaf'] = lin_emul(tt, fx.p(m + 'time_ada_final.weight'), fx.p(m + 'time_ada_final.bias'))
    if mut == 'chunk_tail_lost':       # slots past the last full chunk of LIN_SC repeat the slot before them
        s0 = n // LIN_SC * LIN_SC
        for v in out.values():
            v[s0:] = v[s0 - 1]
    mm = mut if mut in MOD_MUTANTS else None
    out['mod'] = fold(fx, six_of(fx, ada, lora, f32, mm), f32, mm)
    if fx.has_final:
        out['modf'] = fold_final(fx, out['adaf'], f32, mm)
    return out


def chain_tables(fx):
    return tuple(t for t in CHAIN_TABLES if fx.has_final or t not in ('adaf', 'modf'))


def chain_distances(fx, got, ref):
    """table -> rel-L2 per slot of `got` against the fp64 `ref`"""
    return {t: rel_rows(got[t], ref[t]) for t in chain_tables(fx)}


@functools.lru_cache(maxsize=None)
def _floors(name, ts):
    fx = fixture(name)
    ref = ref_chain(fx, ts)
    d = [chain_distances(fx, emul_chain(fx, ts, u), ref) for u in (0, 1, 2)]
    return ref, {t: np.max([x[t] for x in d], axis=0) for t in chain_tables(fx)}


def floors(fx, ts):
    """(fp64 reference tables, table -> emulated floor per slot: the worst of the three evaluations).  The chain gate is CHAIN_FACTOR x these."""
    return _floors(fx.name, tuple(int(t) for t in ts))


def applies_chain(fx, n, mut):
    """None if the mistake can be made (and seen) with this fixture and slot count, else the reason it cannot"""
    if mut == 'lora_unscaled' and fx.scaling == 1.0:
        return 'scaling is 1'
    if mut in ('lora_of_neighbour_block', 'table_of_neighbour_block') and fx.nblk == 1:
        return 'one block'
    if mut == 'final_shift_scale_swapped' and not fx.has_final:
        return 'no final block'
    if mut == 'neighbour_slot' and n == 1:
        return 'one slot'
    if mut == 'chunk_tail_lost' and (n < LIN_SC or n % LIN_SC == 0):
        return 'no partial chunk behind a full one'
    return None


# --------------------------------------------------------------------------------------------------------------------------------
# G' / C'
# --------------------------------------------------------------------------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32))


@functools.lru_cache(maxsize=None)
def _packed(name, b, which, natural):
    from ezaudio_amd.weights import _geglu8, _qkrope
    fx = fixture(name)
    bias = None
    if which == 'qkv':
        W = torch.cat([_t(fx.blk(b, f'attn.{w}.weight')) for w in ('to_q', 'to_k', 'to_v')], 0)
        W = W if natural else _qkrope(W, fx.dh)
    elif which == 'geglu':
        W, bias = _t(fx.blk(b, 'mlp.net.0.proj.weight')), _t(fx.blk(b, 'mlp.net.0.proj.bias'))
        if not natural:
            W, bias = _geglu8(W), _geglu8(bias.reshape(-1, 1)).reshape(-1)
    elif which == 'q2':
        W = _t(fx.blk(b, 'cross_attn.to_q.weight'))
    else:
        W, bias = _t(fx.blk(b, 'skip_linear.weight')), _t(fx.blk(b, 'skip_linear.bias'))
    return bf16r(W.numpy()), None if bias is None else bias.numpy().astype(f32)


def packed(fx, b, which, natural=False):
    """(bf16-rounded weight [N][K] in the packed row order, fp32 bias [N] or None) of table `which` of block b: qkv | geglu | q2 | skip"""
    return _packed(fx.name, b, which, natural)


def zt_sources(fx, mod, b, which):
    """the fp32 gain / shift vectors [slots][K] that table `which` of block b is built from (`mod`: [n][nblk][6][D])"""
    if which == 'qkv':
        return mod[:, b, 0], mod[:, b, 1]
    if which == 'geglu':
        return mod[:, b, 3], mod[:, b, 4]
    if which == 'q2':
        return fx.blk(b, 'norm2.weight')[None], fx.blk(b, 'norm2.bias')[None]
    return fx.blk(b, 'skip_norm.weight')[None], fx.blk(b, 'skip_norm.bias')[None]


def zt_items(fx):
    """(table, item, block) of every table item the handle builds"""
    out = [(w, b, b) for w in ('qkv', 'geglu', 'q2') for b in range(fx.nblk)]
    if not fx.is_cn:
        out += [('skip', j, fx.nhalf + 1 + j) for j in range(fx.nhalf)]
    return out


def zt_ref_bound(fx, mod, which, b):
    """(fp64 reference [slots][2][N], bound [slots][2][N]) of one table item from the fp32 `mod`"""
    W, bias = packed(fx, b, which)
    g, c = zt_sources(fx, mod, b, which)
    W64, K = W.astype(f64), W.shape[1]
    ref, bound = [], []
    for v, bb in ((g, None), (c, bias)):
        r = v.astype(f64) @ W64.T
        s = np.abs(v.astype(f64)) @ np.abs(W64).T
        if bb is not None:
            r, s = r + bb.astype(f64), s + np.abs(bb.astype(f64))
        ref.append(r)
        bound.append((U17 + (K + 2) * U24) * s)
    return np.stack(ref, 1), np.stack(bound, 1)


def _hilo(v, W, drop_lo):
    hi = bf16r(v)
    out = hi @ W.T
    return out if drop_lo else out + bf16r(v - hi) @ W.T


def zt_emul(fx, mod, mut=None):
    """the four tables in fp32 as ezdit_prepare_timesteps leaves them, from the fp32 `mod` [n][nblk][6][D]: dict qkv [n][nblk][2][3 D], geglu [n][nblk][2][2 I],
    q2 [nblk][2][D], skip [nhalf][2][D] (backbone)"""
    n = mod.shape[0]
    out = {}
    for which, item, b in zt_items(fx):
        W, bias = packed(fx, b, which, natural=mut == 'natural_order_columns')
        g, c = zt_sources(fx, mod.astype(f32), b, which)
        G, Cc = _hilo(g.astype(f32), W, mut == 'drop_lo'), _hilo(c.astype(f32), W, mut == 'drop_lo')
        if mut == 'rows_past_128_lost':
            lost = np.arange(len(G)) * 4 >= Z_TILE_ROWS
            G[lost], Cc[lost] = 0, 0
        if bias is not None and mut != 'c_without_bias':
            Cc = Cc + bias[None]
        if mut == 'g_c_swapped':
            G, Cc = Cc, G
        pair = np.stack([G, Cc], 1).astype(f32)      # [slots][2][N]
        N = W.shape[0]
        if which in ('qkv', 'geglu'):
            items = fx.nblk
            buf = out.setdefault(which, np.zeros(n * items * 2 * N, f32))
            stride = 2 * N * (1 if mut == 'slot_stride_of_one_block' else items)
            for s in range(n):
                o = s * stride + item * 2 * N
                if o + 2 * N <= buf.size:
                    buf[o:o + 2 * N] = pair[s].reshape(-1)
        else:
            items = fx.nblk if which == 'q2' else fx.nhalf
            buf = out.setdefault(which, np.zeros(items * 2 * N, f32))
            buf[item * 2 * N:(item + 1) * 2 * N] = pair[0].reshape(-1)
    D, I = fx.D, fx.I
    out['qkv'] = out['qkv'].reshape(n, fx.nblk, 2, 3 * D)
    out['geglu'] = out['geglu'].reshape(n, fx.nblk, 2, 2 * I)
    out['q2'] = out['q2'].reshape(fx.nblk, 2, D)
    if 'skip' in out:
        out['skip'] = out['skip'].reshape(fx.nhalf, 2, D)
    return out


def zt_ratios(fx, mod, zt):
    """table -> worst |got - ref64| / bound over every slot and item.  `zt`: dict as zt_emul returns it (slot-indexed tables cut to the slots of `mod`)"""
    out = {}
    for which, item, b in zt_items(fx):
        ref, bound = zt_ref_bound(fx, mod, which, b)
        got = zt[which][:, item] if which in ('qkv', 'geglu') else zt[which][item][None]
        out[which] = max(out.get(which, 0.0), worst_ratio(got, ref, bound))
    return out


def applies_zt(fx, n, mut):
    if mut == 'rows_past_128_lost' and 4 * n <= Z_TILE_ROWS:
        return 'no operand row past 128'
    if mut == 'slot_stride_of_one_block' and (n == 1 or fx.nblk == 1):
        return 'one slot or one block'
    return None


ZT_MUTANT_TABLES = dict(drop_lo=('qkv', 'geglu', 'q2', 'skip'), c_without_bias=('geglu', 'skip'), g_c_swapped=('qkv', 'geglu', 'q2', 'skip'),
                        slot_stride_of_one_block=('qkv', 'geglu'), natural_order_columns=('qkv', 'geglu'), rows_past_128_lost=('qkv', 'geglu'))


# --------------------------------------------------------------------------------------------------------------------------------
# zd: the constant cross-attention-out vector of the single-key batch elements
# --------------------------------------------------------------------------------------------------------------------------------
def zd_masks(B, Lc):
    """key masks of case (h): B = 4 -> 1, 6, 20 and 1 valid keys; any other B -> one multi-key element in front of B - 1 single-key ones.  The single key of the LAST
    element is not at position 0.  Returns (mask [B][Lc] bool, key1 [B]: the valid key of a single-key element, -1 otherwise)."""
    mask = np.zeros((B, Lc), bool)
    if B == 4:
        mask[0, 0] = True
        mask[1, :6] = True
        mask[2, :Lc] = True
    else:
        mask[0, :7] = True
        for b in range(1, B - 1):
            mask[b, (3 * b) % Lc if b % 2 else 0] = True
    mask[B - 1, 5] = True
    key1 = np.array([int(np.argmax(r)) if r.sum() == 1 else -1 for r in mask])
    return mask, key1


@functools.lru_cache(maxsize=None)
def zd_ckv(name, B, Lc):
    """(context [B][Lc][Dc], fp32 k | v projection of every block [nblk][B][Lc][2 D]) -- the buffer `ckv` of ezdit_prepare_context, per block, from the fp32 oracle"""
    fx = fixture(name)
    o = fx.oracle(f32)
    ctx = make_inputs(fx.cfg, B=B, L=8, Lc=Lc, seed=11)['ctx']
    c = o.context_embed(ctx)
    ckv = []
    for p in fx.blocks:
        cn = layer_norm(c, o.p(p + '.norm_context.weight'), o.p(p + '.norm_context.bias'))
        ckv.append(np.concatenate([cn @ o.p(p + '.cross_attn.to_k.weight').T, cn @ o.p(p + '.cross_attn.to_v.weight').T], -1))
    return ctx, np.stack(ckv).astype(f32)


def zd_w(fx, b):
    return bf16r(fx.blk(b, 'cross_attn.proj.weight')), fx.blk(b, 'cross_attn.proj.bias').astype(f32)


def zd_ref_bound(fx, v):
    """v: the bf16 value rows [nblk][rows][D] (as fp32) -> (fp64 reference, bound), both [nblk][rows][D]"""
    ref, bound = [], []
    for b in range(fx.nblk):
        W, bias = zd_w(fx, b)
        ref.append(lin_ref(v[b], W, bias))
        bound.append(lin_bound(v[b], W, bias))
    return np.stack(ref), np.stack(bound)


def zd_emul(fx, ckv, key1, mut=None):
    """zd [nblk][single-key elements][D] in fp32, kernel order, from the fp32 `ckv` [nblk][B][Lc][2 D]"""
    D = fx.D
    el = np.nonzero(key1 >= 0)[0]
    out = []
    for b in range(fx.nblk):
        W, bias = zd_w(fx, (b + 1) % fx.nblk if mut == 'w_of_neighbour_block' else b)
        key = np.zeros_like(key1[el]) if mut == 'key_0' else key1[el]
        rows = ckv[b, el, key]
        x = rows[:, :D] if mut == 'k_half_for_v_half' else rows[:, D:]
        x = x if mut == 'v_not_rounded' else bf16r(x)
        out.append(lin_emul(x, W, None if mut == 'bias_missing' else bias))
    return np.stack(out)


def applies_zd(fx, mut):
    return 'one block' if mut == 'w_of_neighbour_block' and fx.nblk == 1 else None


def bf16_ulp_bound(ref):
    """one bf16 ulp of `ref`: 2^(e - 7) for 2^e <= |ref| < 2^(e + 1) (the smallest normal's for zero and values that round to it)"""
    _, e = np.frexp(np.maximum(np.abs(np.asarray(ref, f64)), 2.0 ** -126))      # |ref| = m 2^e, 0.5 <= m < 1
    return np.ldexp(1.0, e - 1 - 7)
